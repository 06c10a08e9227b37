"""numpy restatement of ``sp_fg_row_index`` / ``sp_patch_origins_fg`` (include/stroke_amd.h, csrc/sp_fgpatch.hip): the mask and the
numbering through ``np.flatnonzero``, the prefix through ``cumsum``, ``k`` through Python integers -- no bisection, no ballots."""
import numpy as np


def fg_mask(labels, chanmask, thr):
    """labels (N, C1, Z, Y, X) -> bool (N, Z, Y, X): above ``thr`` (strictly) in a channel whose bit is set in ``chanmask``"""
    labels = np.asarray(labels, dtype=np.float32)
    chans = [c for c in range(labels.shape[1]) if (int(chanmask) >> c) & 1]
    assert chans, "chanmask selects no channel"
    return (labels[:, chans] > np.float32(thr)).any(axis=1)


def row_prefix(labels, chanmask, thr):
    """int32 (N, Z * Y + 1): exclusive prefix sum of the per-x-row foreground counts; the last column is the case's total"""
    m = fg_mask(labels, chanmask, thr)
    N, Z, Y, X = m.shape
    out = np.zeros((N, Z * Y + 1), dtype=np.int64)
    out[:, 1:] = np.cumsum(m.reshape(N, Z * Y, X).sum(axis=2), axis=1)
    return out.astype(np.int32)


def u_for(k, total):
    """the smallest 32-bit u with (u * total) >> 32 == k, for 0 <= k < total"""
    k, total = int(k), int(total)
    assert 0 <= k < total
    return -((-k << 32) // total)          # ceil(k * 2^32 / total)


def resolve(labels, table, draws, ext1, omax, chanmask, thr):
    """-> (table after the kernel, int64 (B, 5); picked, int64 (B, 4) = (k, fx, fy, fz) or -1s where the row stays as it is).
    ``draws`` (B, 5): force, u (any integer; its low 32 bits count), jx, jy, jz."""
    m = fg_mask(labels, chanmask, thr)
    N, Z, Y, X = m.shape
    table = np.array(table, dtype=np.int64).reshape(-1, 5)
    draws = np.asarray(draws, dtype=np.int64).reshape(-1, 5)
    picked = np.full((table.shape[0], 4), -1, dtype=np.int64)
    for b, ((slot, _, _, _, flip), (force, u, jx, jy, jz)) in enumerate(zip(table.tolist(), draws.tolist())):
        if force == 0 or not 0 <= slot < N:
            continue
        flat = np.flatnonzero(m[slot])
        total = int(flat.size)
        if total == 0:
            continue
        k = ((int(u) & 0xFFFFFFFF) * total) >> 32
        fz, fy, fx = (int(v) for v in np.unravel_index(int(flat[k]), (Z, Y, X)))
        picked[b] = (k, fx, fy, fz)
        f = (X - 1 - fx if flip else fx, fy, fz)
        j = [min(max(int(a), 0), int(e) - 1) for a, e in zip((jx, jy, jz), ext1)]
        table[b, 1:4] = [min(max(fa - ja, 0), int(ma)) for fa, ja, ma in zip(f, j, omax)]
    return table, picked
