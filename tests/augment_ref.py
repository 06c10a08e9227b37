"""Numpy restatement of the batch augmentation's generator (csrc/sp_augment.hip:sp_rng_uniform_pm1), shared by
tests/test_augment_host.py (Random123 known answers) and tests/test_gpu_augment.py (bit equality with the kernel)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two ints -> four uint32 arrays (Salmon et al., SC11)"""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in counter]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)          # 32 x 32 -> 64 bits, no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return [v.astype(np.uint32) for v in c]


def uniform_pm1(nfields, per_field, seed, call):
    """what sp_rng_uniform_pm1 writes: (nfields, per_field) fp32 in [-1, 1)"""
    e = np.arange(per_field, dtype=np.uint64)
    out = np.empty((nfields, per_field), dtype=np.float32)
    for f in range(nfields):
        words = philox4x32_10((e >> np.uint64(2), np.full(per_field, f), np.full(per_field, call & MASK), np.full(per_field, call >> 32)),
                              (seed & MASK, seed >> 32))
        w = np.stack(words, axis=1)[np.arange(per_field), (e & np.uint64(3)).astype(np.int64)]
        u = (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
        out[f] = np.float32(2.0) * u - np.float32(1.0)
    return out
