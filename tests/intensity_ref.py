"""Numpy restatement of the batch intensity augmentation (csrc/sp_intensity.hip; common/data.py:IntensityAugment), shared by
tests/test_intensity_host.py and tests/test_gpu_intensity.py.  Two evaluations of the same semantics: float64 (the reference the
kernels are held to) and all-float32 (every operation rounded to fp32 in the kernels' order: what separates it from the float64
one is the error any fp32 implementation makes, and the tolerance of the GPU tests is derived from that distance).  The Philox
words come from tests/augment_ref.py."""
import numpy as np

import augment_ref as A

CHUNKS = 64
EPS = np.float32(1e-7)
F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------ inputs and parameter tables

def smooth_volumes(nfields, shape_zyx, seed):
    """(nfields, Z, Y, X) fp32: smooth random volumes of unit scale (max |x| = 1 per field, both signs) inside a zero border one
    voxel wide, as the padded patches have"""
    from scipy import ndimage
    rs = np.random.RandomState(seed)
    out = np.zeros((nfields,) + tuple(shape_zyx), dtype=np.float32)
    for f in range(nfields):
        v = ndimage.gaussian_filter(rs.randn(*shape_zyx), 1.5, mode="reflect")
        v[[0, -1]] = 0
        v[:, [0, -1]] = 0
        v[:, :, [0, -1]] = 0
        out[f] = (v / np.abs(v).max()).astype(np.float32)
    return out


def row(sigma_n=0.0, gain=1.0, contrast=1.0, gamma=1.0, invert=False):
    return [sigma_n, gain, contrast, gamma, float(invert), 0, 0, 0]


NEUTRAL = row()
# the two hand-made tables of the tolerance tests, four fields each (B = 2, C0 = 2)
TABLES = {
    "single": np.array([row(sigma_n=0.3), row(contrast=1.2), row(gamma=0.7), row(gamma=1.5, invert=True)], dtype=np.float32),
    "chained": np.array([row(0.2, 1.2, 0.8, 1.4), row(0.25, 0.8, 1.25, 0.75, True), row(gain=1.1, contrast=0.8), row(sigma_n=0.3, gamma=0.7)],
                        dtype=np.float32),
}
SHAPES = [(7, 10, 13), (8, 12, 16), (28, 52, 52)]      # scalar tail and short chunks; 16-byte path; a chunk loop that iterates
SEED, CALL, INPUT_SEED = 2024, 3, 11


# ------------------------------------------------------------------------------------------------ blur

def gaussian_weights(sigma, radius=None, truncate=4.0):
    """scipy.ndimage's _gaussian_kernel1d(sigma, 0, int(truncate * sigma + 0.5)) in float64, zero-padded to `radius`"""
    r = int(truncate * float(sigma) + 0.5)
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    radius = r if radius is None else radius
    out = np.zeros(2 * radius + 1)
    out[radius - r:radius + r + 1] = phi
    return out


def weights_table(sigmas):
    """fp32 (nfields, 2 radius + 1): the taps of every field, the delta kernel where sigma is None"""
    radius = max(int(4.0 * s + 0.5) for s in sigmas if s is not None)
    table = np.zeros((len(sigmas), 2 * radius + 1), dtype=np.float32)
    for f, s in enumerate(sigmas):
        if s is None:
            table[f, radius] = 1.0
        else:
            table[f] = gaussian_weights(s, radius)
    return table


def _fma(a, b, c, dtype):
    if dtype == F64:
        return a * b + c
    return (a.astype(F64) * F64(b) + c.astype(F64)).astype(F32)      # the product of two fp32 is exact in float64


def blur_field(x, w, dtype=F64):
    """one (Z, Y, X) field through the taps `w` along x, then y, then z; border d c b a | a b c d | d c b a; taps summed lowest
    to highest"""
    radius = (len(w) - 1) // 2
    y = np.asarray(x, dtype=dtype)
    w = np.asarray(w, dtype=dtype)
    for axis in (2, 1, 0):
        n = y.shape[axis]
        assert n >= radius
        pad = [(0, 0)] * 3
        pad[axis] = (radius, radius)
        p = np.pad(y, pad, mode="symmetric")
        acc = np.zeros_like(y)
        for t in range(2 * radius + 1):
            acc = _fma(np.take(p, np.arange(t, t + n), axis=axis), w[t], acc, dtype)
        y = acc
    return y


def blur(x, weights, dtype=F64):
    return np.stack([blur_field(x[f], weights[f], dtype) for f in range(len(x))])


# ------------------------------------------------------------------------------------------------ noise

def normals(field, per_field, seed, call, dtype=F64):
    """the standard normals of one field: counter (e >> 2, 0x80000000 | field, call lo, call hi), key (seed lo, seed hi); words
    (w0, w1) -> elements 4q, 4q + 1 and (w2, w3) -> 4q + 2, 4q + 3 by Box-Muller"""
    nq = (per_field + 3) // 4
    q = np.arange(nq, dtype=np.uint64)
    full = lambda v: np.full(nq, v, dtype=np.uint64)
    w = A.philox4x32_10((q, full(0x80000000 | field), full(call & A.MASK), full(call >> 32)), (seed & A.MASK, seed >> 32))
    out = np.empty((nq, 4), dtype=dtype)
    two_pi = dtype(6.2831853071795864769)
    for p in range(2):
        u1 = ((w[2 * p] >> np.uint32(8)).astype(dtype) + dtype(1)) * dtype(2.0 ** -24)
        u2 = (w[2 * p + 1] >> np.uint32(8)).astype(dtype) * dtype(2.0 ** -24)
        r = np.sqrt(dtype(-2) * np.log(u1))
        a = two_pi * u2
        out[:, 2 * p] = r * np.cos(a)
        out[:, 2 * p + 1] = r * np.sin(a)
    return out.reshape(-1)[:per_field]


def noisy(x, params, seed, call, dtype=F64):
    """y1 of (nfields, ...) fields, flattened per field"""
    nf = len(x)
    y = np.asarray(x, dtype=dtype).reshape(nf, -1).copy()
    for f in range(nf):
        sn = dtype(params[f][0])
        if sn != 0:
            y[f] = y[f] + sn * normals(f, y.shape[1], seed, call, dtype)
    return y


# ------------------------------------------------------------------------------------------------ statistics, apply

def chunk_length(per_field):
    return ((per_field + CHUNKS - 1) // CHUNKS + 3) // 4 * 4


def stats(y1, dtype=F64):
    """(min, max, mean) of a flat field; in fp32 the sum runs per chunk in fp32 and over the chunks in float64, as on the device"""
    if dtype == F64:
        return y1.min(), y1.max(), y1.mean()
    c = chunk_length(len(y1))
    total = sum(F64(np.add.reduce(y1[i:i + c], dtype=F32)) for i in range(0, len(y1), c))
    return y1.min(), y1.max(), F32(total / F64(len(y1)))


def apply(x, params, seed, call, dtype=F64):
    """stages 2 to 6 on (nfields, Z, Y, X) fields (blur them first); a neutral stage is skipped"""
    x = np.asarray(x)
    y1 = noisy(x, params, seed, call, dtype)
    out = np.empty_like(y1)
    eps = dtype(EPS)
    for f in range(len(x)):
        g, k, gm = (dtype(params[f][i]) for i in (1, 2, 3))
        invert = params[f][4] != 0
        mn, mx, mean = stats(y1[f], dtype)
        y = y1[f]
        if g != 1:
            y = g * y
        m2, min2, max2 = g * mean, g * mn, g * mx
        contrast = lambda v: np.minimum(np.maximum(_fma(np.asarray(v - m2, dtype=dtype), k, np.asarray(m2, dtype=dtype), dtype), min2), max2)
        min3, max3 = min2, max2
        if k != 1:
            y, min3, max3 = contrast(y), contrast(min2), contrast(max2)
        if gm != 1 or invert:
            R = max3 - min3
            if invert:
                y = max3 - np.power(np.maximum((max3 - y) / (R + eps), dtype(0)), gm) * R
            else:
                y = np.power(np.maximum((y - min3) / (R + eps), dtype(0)), gm) * R + min3
        assert y.dtype == dtype
        out[f] = y
    return out.reshape(x.shape)


def fp32_distance(table, shape_zyx):
    """the largest |fp32 evaluation - float64 evaluation| of `apply` on the inputs of the GPU tolerance tests"""
    x = smooth_volumes(len(table), shape_zyx, INPUT_SEED)
    return float(np.abs(apply(x, table, SEED, CALL, F32).astype(F64) - apply(x, table, SEED, CALL, F64)).max())
