"""numpy restatement of ``sp_patch_gather_batch`` (include/stroke_amd.h, csrc/sp_gather.hip): the formula of the header comment,
element by element through index arrays -- no flip, pad or slice call of the transform classes it stands in for."""
import numpy as np


def gather_group(src, table, ext, pad, padval):
    """src (N, C, Z, Y, X) fp32; table int (B, 5): case, ox, oy, oz, flip; ext = (w, h, d); pad = (px, py, pz) ->
    dst (B, C, d, h, w): dst[b, c, z, y, x] = src[case, c, oz + z - pz, oy + y - py, flip ? X - 1 - u : u], u = ox + x - px,
    ``padval`` where (u, v, s) leaves the volume or the case leaves [0, N)."""
    src = np.asarray(src, dtype=np.float32)
    table = np.asarray(table, dtype=np.int64).reshape(-1, 5)
    N, C, Z, Y, X = src.shape
    w, h, d = (int(e) for e in ext)
    px, py, pz = (int(p) for p in pad)
    out = np.full((table.shape[0], C, d, h, w), np.float32(padval), dtype=np.float32)
    for b, (case, ox, oy, oz, flip) in enumerate(table):
        if not 0 <= case < N:
            continue
        u, v, s = ox + np.arange(w) - px, oy + np.arange(h) - py, oz + np.arange(d) - pz
        iu, iv, is_ = (u >= 0) & (u < X), (v >= 0) & (v < Y), (s >= 0) & (s < Z)
        xs = X - 1 - u[iu] if flip else u[iu]
        block = src[case][:, s[is_]][:, :, v[iv]][:, :, :, xs]
        out[b][np.ix_(np.arange(C), np.nonzero(is_)[0], np.nonzero(iv)[0], np.nonzero(iu)[0])] = block
    return out


def gather_ref(src0, src1, table, ext0, pad0, padval0, ext1, pad1, padval1=0.0):
    """both groups of one launch; an empty group (``None``) gives ``None``"""
    return (gather_group(src0, table, ext0, pad0, padval0) if src0 is not None else None,
            gather_group(src1, table, ext1, pad1, padval1) if src1 is not None else None)
