"""numpy restatement of ``sp_patch_sample_batch`` (include/stroke_amd.h): the cached-patch gather read through a per-sample affine
map, an optional displacement field and an optional intensity change.  Plain loops over the batch, the channels and the eight
corners; no scipy.  ``dtype`` selects the arithmetic of the coordinates, weights and sums: ``numpy.float64`` is the reference,
``numpy.float32`` follows the kernel's order of operations (without its fused multiply-adds) and shows what fp32 coordinates cost."""
import numpy as np


def _sample_volume(vol, qx, qy, qz, dtype):
    """S = sum of w_k vol_k and W = sum of w_k over the corners floor(q) + {0, 1}^3 that lie inside ``vol`` (Z, Y, X)"""
    Z, Y, X = vol.shape
    one = dtype(1)
    fl = [np.floor(q) for q in (qx, qy, qz)]
    fr = [q - f for q, f in zip((qx, qy, qz), fl)]
    # positions far outside have no corner inside; clip before the integer conversion
    ix, iy, iz = [np.clip(f, -2, n + 1).astype(np.int64) for f, n in zip(fl, (X, Y, Z))]
    wx, wy, wz = [(one - f, f) for f in fr]
    S = np.zeros(qx.shape, dtype=dtype)
    W = np.zeros(qx.shape, dtype=dtype)
    src = vol.astype(dtype)
    for kz in (0, 1):
        for ky in (0, 1):
            wzy = wz[kz] * wy[ky]
            for kx in (0, 1):
                sx, sy, sz = ix + kx, iy + ky, iz + kz
                wk = wzy * wx[kx]
                inside = (sx >= 0) & (sx < X) & (sy >= 0) & (sy < Y) & (sz >= 0) & (sz < Z)
                val = src[np.clip(sz, 0, Z - 1), np.clip(sy, 0, Y - 1), np.clip(sx, 0, X - 1)]
                S = S + np.where(inside, wk * val, dtype(0))
                W = W + np.where(inside, wk, dtype(0))
    return S, W


def sample_ref(img, lab, table, ext0, pad0, padval0, ext1, pad1, thresh1, xform, fields=None, intensity=None, dtype=np.float64):
    """img (N, C0, Z, Y, X) / lab (N, C1, Z, Y, X) or None; table rows (slot, ox, oy, oz, flip); xform (B, 16); fields (B, 3, d0, h0, w0)
    or None; intensity (B, C0, 2) or None -> (dst0 (B, C0, d0, h0, w0), dst1 (B, C1, d1, h1, w1)) fp32, None for an absent group."""
    dtype = np.dtype(dtype).type
    src = img if img is not None else lab
    N, (Z, Y, X) = src.shape[0], src.shape[2:]
    table = np.asarray(table, dtype=np.int64).reshape(-1, 5)
    xform = np.asarray(xform, dtype=np.float32).reshape(-1, 16).astype(dtype)
    B = len(table)
    centre = [(dtype(e) - dtype(1)) / dtype(2) for e in ext0]
    outs = []
    for t, (vols, ext, pad, padval) in enumerate(((img, ext0, pad0, padval0), (lab, ext1, pad1, 0.0))):
        if vols is None:
            outs.append(None)
            continue
        C = vols.shape[1]
        w, h, d = ext
        out = np.empty((B, C, d, h, w), dtype=np.float32)
        off = [int(a) - int(b) for a, b in zip(pad0, pad)]
        pz, py, px = np.meshgrid(np.arange(d) + off[2], np.arange(h) + off[1], np.arange(w) + off[0], indexing="ij")
        for b in range(B):
            slot, ox, oy, oz, flip = [int(v) for v in table[b]]
            M, tr, axy, alz = xform[b, :9].reshape(3, 3), xform[b, 9:12], xform[b, 12], xform[b, 13]
            rel = [px.astype(dtype) - centre[0], py.astype(dtype) - centre[1], pz.astype(dtype) - centre[2]]
            q = []
            for a, o in enumerate((ox, oy, oz)):
                base = dtype(o - int(pad0[a])) + centre[a]
                q.append(base + (M[a, 0] * rel[0] + M[a, 1] * rel[1] + M[a, 2] * rel[2]) + tr[a])
            if fields is not None:
                f = np.asarray(fields[b], dtype=np.float32).astype(dtype)[:, pz, py, px]
                q = [q[0] + axy * f[0], q[1] + axy * f[1], q[2] + alz * f[2]]
            if flip:
                q[0] = dtype(X - 1) - q[0]
            for c in range(C):
                if 0 <= slot < N:
                    S, W = _sample_volume(vols[slot, c], q[0], q[1], q[2], dtype)
                else:
                    S, W = np.zeros(px.shape, dtype=dtype), np.zeros(px.shape, dtype=dtype)
                if t == 0:
                    gain, bias = (dtype(1), dtype(0)) if intensity is None else [dtype(v) for v in np.asarray(intensity, np.float32)[b, c]]
                    val = gain * S + bias * W + dtype(padval) * (dtype(1) - W)
                else:
                    val = S
                    if thresh1 >= 0:
                        val = np.where(val >= dtype(np.float32(thresh1)), dtype(1), dtype(0))
                out[b, c] = val.astype(np.float32)
        outs.append(out)
    return outs[0], outs[1]


# ------------------------------------------------------------------------------------------------ the inputs the tests share

ZYX = (9, 22, 26)
PAD0 = (3, 2, 1)
PADVAL0 = -1.0
PATCHES = {"vector": (16, 12, 8), "scalar": (13, 11, 7)}      # w0 % 4 == 0: 16-byte stores; odd: one element per lane


def smooth(a, passes=3):
    """a few (1, 2, 1) / 4 passes along the last three axes, edges replicated: smooth volumes without scipy"""
    a = np.asarray(a, dtype=np.float64)
    for _ in range(passes):
        for ax in (-3, -2, -1):
            p = np.concatenate([np.take(a, [0], axis=ax), a, np.take(a, [-1], axis=ax)], axis=ax)
            n = a.shape[ax]
            a = 0.25 * np.take(p, range(0, n), axis=ax) + 0.5 * np.take(p, range(1, n + 1), axis=ax) + 0.25 * np.take(p, range(2, n + 2), axis=ax)
    return a


def cache_arrays(seed=0, N=3, C0=2, C1=2, zyx=ZYX):
    """smooth images in [0, 1] and binary blob labels (a smooth volume above its median)"""
    rs = np.random.RandomState(seed)
    img = smooth(rs.rand(N, C0, *zyx), 2)
    img = (img - img.min()) / (img.max() - img.min())
    blob = smooth(rs.rand(N, C1, *zyx), 3)
    lab = blob > np.median(blob)
    return img.astype(np.float32), lab.astype(np.float32)


def geometry(kind, pad0=PAD0):
    ext0 = PATCHES[kind] if isinstance(kind, str) else tuple(kind)
    ext1 = tuple(e - 2 * p for e, p in zip(ext0, pad0))
    return ext0, ext1


def table_for(ext0, pad0=PAD0, zyx=ZYX):
    """three rows: flipped at the largest x origin (the patch overhangs the volume's high x face), origin (0, 0, 0) (it overhangs
    the low face on every axis), and a slot outside the cache"""
    Z, Y, X = zyx
    return [[1, X + 2 * pad0[0] - ext0[0], 5, 1, 1], [2, 0, 0, 0, 0], [-1, 4, 3, 1, 0]]


def identity_xform(B):
    x = np.zeros((B, 16), dtype=np.float32)
    x[:, 0] = x[:, 4] = x[:, 8] = 1.0
    return x


def affine_xform(angles_deg, scales, t=(0.0, 0.0, 0.0), alpha_xy=0.0, alpha_z=0.0):
    x = identity_xform(len(angles_deg))
    for b, (a, s) in enumerate(zip(angles_deg, scales)):
        c, sn = np.cos(np.deg2rad(a)) / s, np.sin(np.deg2rad(a)) / s
        x[b, 0:2] = (c, -sn)
        x[b, 3:5] = (sn, c)
    x[:, 9:12] = t
    x[:, 12], x[:, 13] = alpha_xy, alpha_z
    return x


def general_case(kind, seed=3):
    """the general transform of the tests: generic angles, scales and shifts and a smooth field of about +-0.3, to be scaled by
    alpha_xy = 6 and alpha_z = 1.3 (a displacement of up to two voxels in plane)"""
    ext0, ext1 = geometry(kind)
    table = table_for(ext0)
    xform = affine_xform([11.0, -7.0, 3.0], [0.9, 1.1, 1.0], t=(0.37, -1.21, 0.43), alpha_xy=6.0, alpha_z=1.3)
    rs = np.random.RandomState(seed)
    f = smooth(rs.rand(len(table), 3, ext0[2], ext0[1], ext0[0]) * 2 - 1, 3)
    fields = (0.3 * f / np.abs(f).max()).astype(np.float32)
    return ext0, ext1, table, xform, fields
