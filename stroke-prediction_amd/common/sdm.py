"""The signed-distance-map (SDM) interpolation baseline of the reference (``test_sdm_resampling.py:15-52``) on the HIP path.

Core and penumbra become signed distance maps, which are downsampled to the CAE's latent size by ``scipy.ndimage.zoom``
semantics, blended by the normalised time to treatment, upsampled again and cropped (``resample``), or blended at full
resolution (``resample=False``).  Every arithmetic step runs in the kernels of ``csrc/sp_sdm.hip`` (fp64 throughout); torch
only allocates.  One call reads the device once: the 32-byte info record, which carries the artificial-core decision (for the
reference's printed line) and the degenerate-input bits (raised as ``ValueError``).
"""
import ctypes as C

import numpy as np
import torch

ARTIFICIAL_CORE_PREFIX = '------------------------------------> artifical core'
# the transforms of sp_sdm_signed_fields, in the order of the info record's degenerate bits
_DEGENERATE = ("the penumbra mask (penu > threshold) fills the volume",
               "the penumbra is empty (every voxel is below the threshold)",
               "core and penumbra masks are both empty",
               "the core mask (core > threshold) fills the volume")
SP_SDM_F64, SP_SDM_I8, SP_SDM_F32_AS_I8, SP_SDM_MASK_GT0, SP_SDM_MASK_LT0, SP_SDM_F32 = 0, 1, 2, 3, 4, 5

host_reads = 0      # device -> host reads made by sdm_interpolate_torch (one per call)


def _rt():
    from stroke_prediction_amd.runtime import lib as L, ops as O
    return L, O


def plan(D, H, W, zoom=12, resample=True, T=1):
    """sp_sdm_plan: ((latent D, h, w), (recon D, h, w), workspace bytes)"""
    L, _ = _rt()
    ext = (C.c_int32 * 6)()
    ws = C.c_int64()
    L.call("sp_sdm_plan", int(D), int(H), int(W), float(zoom), int(bool(resample)), int(T), ext, C.byref(ws))
    return tuple(ext[0:3]), tuple(ext[3:6]), int(ws.value)


def zoom_plan(in_dims, factors, batch=1):
    """sp_sdm_zoom_plan: (full output extents, workspace bytes)"""
    L, _ = _rt()
    nd = len(in_dims)
    full = (C.c_int32 * nd)()
    ws = C.c_int64()
    L.call("sp_sdm_zoom_plan", nd, (C.c_int32 * nd)(*in_dims), (C.c_double * nd)(*[float(f) for f in factors]), int(batch), full,
           C.byref(ws))
    return tuple(full), int(ws.value)


_SRC = {torch.float64: SP_SDM_F64, torch.int8: SP_SDM_I8}
_DST = {"f64": (SP_SDM_F64, torch.float64), "i8": (SP_SDM_I8, torch.int8), "gt0": (SP_SDM_MASK_GT0, torch.float32),
        "lt0": (SP_SDM_MASK_LT0, torch.float32)}


def zoom_torch(x, factors, crop=None, out="f64", batch=False, ws=None, src_as_int8=False):
    """``scipy.ndimage.zoom(x, factors)`` (order 3, mode "constant") of a CUDA tensor on the device (sp_sdm_zoom).

    x: float64 or int8 (or float32 with ``src_as_int8``: ``x.astype(int8)`` first), rank <= 3, plus a leading batch axis when
    ``batch``.  crop: per-axis ``(start, stop)`` window of the full output (None: all).  out: "f64", "i8" (scipy's integer
    rounding), "gt0" / "lt0" (fp32 0/1 masks of the zoomed values)."""
    L, O = _rt()
    x = x.contiguous()
    if src_as_int8:
        if x.dtype != torch.float32:
            raise TypeError("zoom_torch: src_as_int8 takes a float32 tensor")
        src = SP_SDM_F32_AS_I8
    elif x.dtype in _SRC:
        src = _SRC[x.dtype]
    else:
        raise TypeError("zoom_torch: float64 or int8 input (got %s)" % x.dtype)
    nb = x.shape[0] if batch else 1
    dims = tuple(x.shape[1:] if batch else x.shape)
    full, need = zoom_plan(dims, factors, nb)
    lo = [0] * len(dims)
    n = list(full)
    if crop is not None:
        for a, c in enumerate(crop):
            if c is not None:
                start, stop = max(0, c[0]), min(full[a], c[1])
                lo[a], n[a] = start, stop - start
    code, dtype = _DST[out]
    y = torch.empty(((nb,) if batch else ()) + tuple(n), dtype=dtype, device=x.device)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    nd = len(dims)
    I = C.c_int32 * nd
    L.call("sp_sdm_zoom", O.ptr(x), src, O.ptr(y), code, nb, nd, I(*dims), I(*full), I(*lo), I(*n), O.ptr(ws), ws.numel(), O.stream())
    return y


def _volume(x, name):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise TypeError("sdm_interpolate_torch: %s must be a CUDA tensor" % name)
    if x.dim() == 5:
        if x.shape[0] != 1 or x.shape[1] != 1:
            raise ValueError("sdm_interpolate_torch: %s of shape %s, (1, 1, D, H, W) expected" % (name, tuple(x.shape)))
        x = x[0, 0]
    if x.dim() != 3:
        raise ValueError("sdm_interpolate_torch: %s must be (1, 1, D, H, W) or (D, H, W), got %s" % (name, tuple(x.shape)))
    return x.detach().float().contiguous()


def _pinned_upload(a, device):
    host = torch.from_numpy(np.ascontiguousarray(a)).pin_memory()
    return host.to(device, non_blocking=True)


def _times(interpolation, device):
    """-> (device tensor of T values, dtype code, T, vector?)  The values keep their dtype: a float32 t makes (1 - t) a
    float32 rounding, as numpy computes it for the reference's float32 scalar."""
    if isinstance(interpolation, torch.Tensor):
        if interpolation.dim() > 1:
            raise ValueError("sdm_interpolate_torch: interpolation must be a scalar or a 1-D tensor")
        vector = interpolation.dim() == 1
        t = interpolation.detach().reshape(-1)
        if t.dtype not in (torch.float32, torch.float64):
            raise TypeError("sdm_interpolate_torch: interpolation of dtype %s (float32 / float64)" % t.dtype)
        if t.device != device:
            t = _pinned_upload(t.cpu().numpy(), device) if not t.is_cuda else t.to(device)
        t = t.contiguous()
    else:
        a = np.asarray(interpolation)
        if a.ndim > 1:
            raise ValueError("sdm_interpolate_torch: interpolation must be a scalar or a 1-D array")
        vector = a.ndim == 1
        a = a.reshape(-1).astype(np.float32 if a.dtype == np.float32 else np.float64)
        t = _pinned_upload(a, device)
    if t.numel() < 1:
        raise ValueError("sdm_interpolate_torch: no interpolation value")
    return t, (SP_SDM_F32 if t.dtype == torch.float32 else SP_SDM_F64), t.numel(), vector


def _read_info(info):
    """the one device -> host read of a call"""
    global host_reads
    host = torch.empty(8, dtype=torch.int32, pin_memory=True)
    host.copy_(info, non_blocking=True)
    torch.cuda.current_stream(info.device).synchronize()
    host_reads += 1
    return host.tolist()


def sdm_interpolate_torch(core, penu, interpolation, threshold=0.5, zoom=12, dilate=3, resample=True, masks=False):
    """``sdm_interpolate_numpy`` of the reference on CUDA tensors ((1, 1, D, H, W) or (D, H, W)).

    Returns ``recon_core, recon_intp, recon_penu, latent_core, latent_intp, latent_penu`` as float64 CUDA tensors; with a
    1-D ``interpolation`` of T values, ``recon_intp`` / ``latent_intp`` get a leading T axis.  ``masks=True`` appends a
    seventh element, the fp32 0/1 volumes ``(recon_intp > 0, recon_core < 0, recon_penu > 0)`` for the measures.
    Raises ``ValueError`` where the reference's distance transforms are meaningless (a mask that fills the volume, an empty
    penumbra)."""
    L, O = _rt()
    core = _volume(core, "core")
    penu = _volume(penu, "penu")
    if core.shape != penu.shape or core.device != penu.device:
        raise ValueError("sdm_interpolate_torch: core %s and penu %s differ" % (tuple(core.shape), tuple(penu.shape)))
    dev = core.device
    D, H, W = core.shape
    t, t_code, T, vector = _times(interpolation, dev)
    (lD, lh, lw), (rD, rh, rw), need = plan(D, H, W, zoom, resample, T)
    n, nl, nr = D * H * W, lD * lh * lw, rD * rh * rw
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    info = torch.empty(8, dtype=torch.int32, device=dev)
    fields = torch.empty(2, D, H, W, dtype=torch.float64, device=dev)         # core_dist, penu_dist
    latents = torch.empty(2 + T, lD, lh, lw, dtype=torch.float64, device=dev)  # core, penu, intp[T]
    st = O.stream()
    L.call("sp_sdm_signed_fields", O.ptr(core), O.ptr(penu), D, H, W, float(threshold), int(dilate), O.ptr(fields[0]), O.ptr(fields[1]),
           O.ptr(info), O.ptr(ws), need, st)
    I3 = C.c_int32 * 3
    L.call("sp_sdm_zoom", O.ptr(fields), SP_SDM_F64, O.ptr(latents), SP_SDM_F64, 2, 3, I3(D, H, W), I3(lD, lh, lw), None, None,
           O.ptr(ws), need, st)
    L.call("sp_sdm_blend", O.ptr(latents[1]), O.ptr(latents[0]), O.ptr(t), t_code, T, nl, None, O.ptr(latents[2:]), None, st)
    mk = torch.empty(T + 2, rD, rh, rw, dtype=torch.float32, device=dev) if masks else None
    if resample:
        recon = torch.empty(2 + T, rD, rh, rw, dtype=torch.float64, device=dev)
        full, _ = zoom_plan((lD, lh, lw), (1.0, float(zoom), float(zoom)), 2 + T)
        L.call("sp_sdm_zoom", O.ptr(latents), SP_SDM_F64, O.ptr(recon), SP_SDM_F64, 2 + T, 3, I3(lD, lh, lw), I3(*full), I3(0, 2, 2),
               I3(rD, rh, rw), O.ptr(ws), need, st)
        if masks:
            L.call("sp_sdm_blend", O.ptr(recon[1]), O.ptr(recon[0]), None, SP_SDM_F64, T, nr, O.ptr(recon[2:]), None, O.ptr(mk), st)
        recon_core, recon_penu, recon_intp = recon[0], recon[1], recon[2:]
    else:
        recon_intp = torch.empty(T, D, H, W, dtype=torch.float64, device=dev)
        L.call("sp_sdm_blend", O.ptr(fields[1]), O.ptr(fields[0]), O.ptr(t), t_code, T, n, None, O.ptr(recon_intp), O.ptr(mk), st)
        recon_core, recon_penu = fields[0], fields[1]
    flags = _read_info(info)
    bad = [_DEGENERATE[k] for k in range(4) if flags[4] >> k & 1]
    if bad:
        raise ValueError("sdm_interpolate_torch: degenerate input: " + "; ".join(bad))
    if flags[0]:
        print(ARTIFICIAL_CORE_PREFIX, flags[1:4])
    latent_core, latent_penu, latent_intp = latents[0], latents[1], latents[2:]
    if not vector:
        recon_intp, latent_intp = recon_intp[0], latent_intp[0]
    out = (recon_core, recon_intp, recon_penu, latent_core, latent_intp, latent_penu)
    if masks:
        out = out + ((mk[:T] if vector else mk[0], mk[T], mk[T + 1]),)
    return out


def sdm_interpolate_numpy(core, penu, interpolation, threshold=0.5, zoom=12, dilate=3, resample=True):
    """The reference's signature and return types (numpy float64): uploads once (as float32, the dtype the reference's
    script hands it) and runs ``sdm_interpolate_torch``."""
    if not torch.cuda.is_available():
        raise RuntimeError("sdm_interpolate_numpy (stroke_prediction_amd) runs on the GPU: no CUDA device available")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    out = sdm_interpolate_torch(up(core), up(penu), interpolation, threshold=threshold, zoom=zoom, dilate=dilate, resample=resample)
    return tuple(o.cpu().numpy() for o in out)
