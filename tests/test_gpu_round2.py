"""Round-2 GPU parity tests ("What's weak" 1-4 and ADVICE r1):

* every 3x3x3 layer of BASELINE configs[1] at its HEADLINE shape, in bf16, through the production ``ConvLayer`` path
  (planner choices, z-marching / DMA kernels, plane-major concat inputs) -- forward, data gradient, weight gradient and
  the BatchNorm-backward sums against CPU ``F.conv3d`` autograd on the same bf16-rounded operands;
* three FusedAdam steps of the U-Net against the multi-step fixtures recorded from the reference;
* the 4-scale network (BASELINE configs[4] topology) against its reference fixture;
* regression tests for the cache / optimiser-state / stale-activation findings of ADVICE r1.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import nets, weights as W
from stroke_prediction_amd.common.model.Unet3D import Unet3D, LargeUnet3D
import stroke_prediction_amd.common.dto.UnetDto as UnetDtoUtil
from stroke_prediction_amd.runtime import lib as L
from stroke_prediction_amd.runtime import ops as O
from stroke_prediction_amd.runtime import layers as LY

CH = [2, 16, 32, 64, 32, 16, 32, 2]
CH4 = [2, 32, 64, 128, 256, 128, 64, 32, 32, 2]
DEV = "cuda:0"
LEAKY = 0.01


@pytest.fixture(autouse=True)
def production_kernel_choices():
    """these tests measure what the bench runs"""
    keep = O.ZM_MIN_PLANES
    O.ZM_MIN_PLANES = 256          # batch 1 here, batch 4 in the bench: every layer the bench runs on the z-marching kernel does so here
    yield
    O.ZM_MIN_PLANES = keep


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def bf(t):
    return t.bfloat16().float()


# (name, cin, cout, input dims, planar concat input, first layer) -- the ten 3x3x3 layers at 2 x 128^3
HEADLINE_LAYERS = [
    ("b1c1", 2, 16, 128, False, True), ("b1c2", 16, 16, 126, False, False),
    ("b2c1", 16, 32, 62, False, False), ("b2c2", 32, 32, 60, False, False),
    ("b3c1", 32, 64, 29, False, False), ("b3c2", 64, 64, 27, False, False),
    ("b4c1", 96, 32, 50, True, False), ("b4c2", 32, 32, 48, False, False),
    ("b5c1", 48, 16, 92, True, False), ("b5c2", 16, 16, 90, False, False),
]


def _to_cl(x, cp):
    B, C = x.shape[:2]
    dst = O.alloc_cl(B, x.shape[2:], cp, L.SP_BF16, DEV)
    O.ncdhw_to_cl(x.contiguous().to(DEV), dst, L.SP_BF16)
    return dst


def _from_cl(t, c):
    out = torch.empty((t.shape[0], c) + tuple(t.shape[1:4]), dtype=torch.float32, device=DEV)
    O.cl_to_ncdhw(t, out, L.SP_BF16)
    return out.cpu()


@pytest.mark.parametrize("name,cin,cout,n,planar,first", HEADLINE_LAYERS)
def test_headline_layer_shapes_bf16(name, cin, cout, n, planar, first):
    """One ``[BatchNorm] -> Conv3d(3, p0) -> LeakyReLU`` unit (Unet3D.py:18-20) of the headline network in bf16 at its real
    spatial size (batch 1), exactly as ``UnetEngine`` builds and drives it.  Reference: plain torch on the CPU with the
    operands the kernels see -- the bf16 input, the BatchNorm folded into bf16 weights (forward), bf16 weights (data
    gradient), bf16 dz -- fp32 accumulation.  Tolerances: outputs are stored as bf16 (2^-9 relative) of sums over
    27 x Cin products."""
    B, dims = 1, (n, n, n)
    g = torch.Generator().manual_seed(1000 + n + cin)
    sc = LY.Scratch(DEV)
    kw = dict(bn_prefix="bn", conv_prefix="cv", act=L.ACT_LEAKY, act_param=LEAKY)
    if first:
        if not LY.FirstConvLayer.supported(cin, cout, 3, 1, 0, L.SP_BF16, True):
            pytest.skip("packed first-layer kernels not available")
        lay = LY.FirstConvLayer(name, "conv", cin, cout, 3, 1, 0, dims, B, L.SP_BF16, DEV, sc, need_input_grad=False,
                                cpi=O.cpad(cin, 16), **kw)
    else:
        lay = LY.ConvLayer(name, "conv", cin, cout, 3, 1, 0, dims, B, L.SP_BF16, DEV, sc, need_input_grad=True, **kw)
    lay.reserve_bwd_scratch()
    sc.finalize()
    assert lay.fold or first, "headline layers run on the folded DMA path"
    if planar:
        assert O.CAT_PLANAR and O.wgrad_dma_ok(lay.cpi, lay.cpo, L.SP_BF16)
        lay.x_planar = True
    x = torch.randn(B, cin, *dims, generator=g) * (0.5 + torch.rand(cin, generator=g)).view(1, -1, 1, 1, 1) \
        + torch.randn(cin, generator=g).view(1, -1, 1, 1, 1) * 0.3
    x = x if first else bf(x)                       # the first layer reads the fp32 network input itself
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) / math.sqrt(cin * 27)
    b = torch.randn(cout, generator=g) * 0.1
    gamma, beta = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.1
    params = {"bn.weight": gamma.to(DEV), "bn.bias": beta.to(DEV), "cv.weight": w.to(DEV).contiguous(), "cv.bias": b.to(DEV)}
    bufs = {"bn.running_mean": torch.zeros(cin, device=DEV), "bn.running_var": torch.ones(cin, device=DEV),
            "bn.num_batches_tracked": torch.zeros((), dtype=torch.int64, device=DEV)}
    grads = {k: torch.zeros_like(v) for k, v in params.items()}
    sc.zero()
    # ---- input in the layout the engine hands over, batch statistics as its producer kernel would have left them
    if first:
        xd = x.to(DEV).contiguous()
        lay.input_stats(xd)
    else:
        xcl = _to_cl(x, lay.cpi)
        O.bn_stats(xcl, L.SP_BF16, lay.in_sums)
        if planar:      # [C/16][B][D][H][W][16]
            xd = xcl.view(B, n, n, n, lay.cpi // 16, 16).permute(4, 0, 1, 2, 3, 5).contiguous().view(B, n, n, n, lay.cpi)
        else:
            xd = xcl
    out_stats = torch.zeros(LY.STATS_NREP * lay.cpo * 2, dtype=torch.float64, device=DEV)
    y = lay.forward(xd, params, bufs, True, out_stats)
    # ---- reference forward: BatchNorm (batch statistics, fp32) folded into bf16 weights, fp32 accumulation
    mean = x.mean(dim=(0, 2, 3, 4))
    var = x.var(dim=(0, 2, 3, 4), unbiased=False)
    s = gamma / torch.sqrt(var + 1e-5)
    t = beta - mean * s
    wf = bf(w * s.view(1, -1, 1, 1, 1))
    bias_f = b + (w * t.view(1, -1, 1, 1, 1)).sum(dim=(1, 2, 3, 4))
    xin = bf(x) if first else x
    z_ref = F.conv3d(xin, wf, bias_f)
    y_ref = F.leaky_relu(z_ref, LEAKY)
    got = _from_cl(y, cout)
    scale = float(y_ref.abs().max())
    err = float((got - y_ref).abs().max())
    assert err <= 2.5e-2 * scale, (name, "fwd", err, scale)
    assert rel_l2(got, y_ref) < 6e-3, (name, "fwd l2", rel_l2(got, y_ref))
    st = out_stats.view(LY.STATS_NREP, lay.cpo, 2).sum(0).cpu()
    torch.testing.assert_close(st[:cout, 0], got.double().sum(dim=(0, 2, 3, 4)), rtol=1e-4, atol=1e-2)
    torch.testing.assert_close(st[:cout, 1], (got.double() ** 2).sum(dim=(0, 2, 3, 4)), rtol=1e-4, atol=1e-2)
    # ---- backward: dz given (as the consumer of y would form it), sum of dz per channel in the replica rows
    lay._init_bwd()
    dz = bf(torch.randn(z_ref.shape, generator=g) * (y_ref != 0).float())
    dzd = _to_cl(dz, lay.cpo)
    lay.dz.copy_(dzd)
    lay.dbias_sums.zero_()
    lay.dbias_sums[0, :cout] = dz.double().sum(dim=(0, 2, 3, 4)).to(DEV)
    if first:
        lay.backward(xd, params, grads)
        g_dev = None
    else:
        g_dev, coef = lay.backward(xd, params, grads)
    torch.cuda.synchronize()
    # reference: z = conv(x_hat, W) + b with x_hat = s * x + t;  dW from the UN-rounded normalised input (the kernel folds the
    # BatchNorm into the finish step: dW = s * sum(dz x) + t * sum(dz)), dgrad with bf16 weights
    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    xh = F.batch_norm(xr, None, None, gr, br, True, 0.1, 1e-5)
    zz = F.conv3d(xh, wr, b)
    dw_ref, dgamma_ref, dbeta_ref = torch.autograd.grad(zz, (wr, gr, br), dz)
    e = rel_l2(grads["cv.weight"].cpu(), dw_ref)
    assert e < 1.5e-2, (name, "wgrad", e)
    torch.testing.assert_close(grads["cv.bias"].cpu(), dz.sum(dim=(0, 2, 3, 4)), rtol=1e-3, atol=1e-2)
    # BatchNorm gamma / beta gradients come out of the weight-gradient accumulator (layers.py: bn_from_wgrad)
    sg = float(dgamma_ref.abs().max()) + 1e-6
    assert float((grads["bn.weight"].cpu() - dgamma_ref).abs().max()) <= 3e-2 * sg + 5e-2, (name, "dgamma")
    sb = float(dbeta_ref.abs().max()) + 1e-6
    assert float((grads["bn.bias"].cpu() - dbeta_ref).abs().max()) <= 3e-2 * sb + 5e-2, (name, "dbeta")
    if g_dev is not None:
        g_ref = F.conv_transpose3d(dz, bf(w))            # dL/dx_hat with the weights the data-gradient kernel packs
        gg = _from_cl(g_dev, cin)
        sg = float(g_ref.abs().max())
        assert float((gg - g_ref).abs().max()) <= 2.5e-2 * sg, (name, "dgrad", float((gg - g_ref).abs().max()), sg)
        assert rel_l2(gg, g_ref) < 6e-3, (name, "dgrad l2", rel_l2(gg, g_ref))
        # BatchNorm-backward coefficients: dx = c0 * g + c1 * x + c2 must reproduce autograd's dx
        dx_ref = torch.autograd.grad(F.conv3d(F.batch_norm(xr, None, None, gamma, beta, True, 0.1, 1e-5), bf(w), b), xr, dz)[0]
        c = coef.cpu()
        dx = c[0, :cin].view(1, -1, 1, 1, 1) * gg + c[1, :cin].view(1, -1, 1, 1, 1) * x + c[2, :cin].view(1, -1, 1, 1, 1)
        assert rel_l2(dx, dx_ref) < 2e-2, (name, "dx", rel_l2(dx, dx_ref))


ZM_CASES = [
    # cin, cout, dims, batch -- ragged rows / columns / few planes, every (P, NT) kernel, forward and data gradient
    (16, 16, (7, 37, 21), 2), (16, 16, (3, 70, 35), 1), (16, 32, (6, 19, 33), 2), (16, 48, (5, 21, 18), 1),
    (32, 16, (9, 35, 17), 1), (32, 32, (6, 20, 40), 2), (48, 16, (5, 19, 37), 1),
    # planes whose rows are no multiple of 16: the flattened (row, column) tiles of plan.zm_tile -- 50 x 50 outputs as 25 x 10
    # tiles (52 x 52 for the data gradient), 88 x 88 as 22 x 22, a 25 x 25 plane
    (32, 32, (4, 52, 52), 1), (16, 16, (4, 90, 90), 1), (48, 16, (4, 27, 27), 2), (16, 48, (3, 50, 50), 1),
]


@pytest.mark.parametrize("cin,cout,dims,B", ZM_CASES)
def test_z_marching_kernel_matches_conv3d(cin, cout, dims, B):
    """csrc/sp_conv_zm.hip alone: valid 3x3x3 convolution (+ bias, LeakyReLU, statistics) and its data gradient ("full"
    correlation: padding chunks come from the zero page) on ragged volumes, against torch on bf16-rounded operands"""
    from stroke_prediction_amd.runtime import plan as P
    O.ZM_MIN_PLANES = 0
    g = torch.Generator().manual_seed(cin * 7 + cout)
    x = bf(torch.randn(B, cin, *dims, generator=g))
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) / math.sqrt(27 * cin)
    b = torch.randn(cout, generator=g) * 0.1
    op = P.conv_fwd_op(cin, cout, 3, 1, 0, dims, cin, cout, L.SP_BF16)
    run = O.ConvRunner(op, DEV, zm_batch=B)
    assert run.uses_zm()
    if dims[1:] == (52, 52):
        assert (run.zm["TW"], run.zm["TH"]) == (25, 10)
    run.prep(w.to(DEV), b.to(DEV))
    xs = _to_cl(x, cin)
    y = O.alloc_cl(B, op.y_dims, cout, L.SP_BF16, DEV)
    y.fill_(7.0)
    nrep = 4
    stats = torch.zeros(nrep * cout * 2, dtype=torch.float64, device=DEV)
    run.run(xs, y, B, None, None, L.ACT_LEAKY, LEAKY, stats, stats_nrep=nrep)
    ref = F.leaky_relu(F.conv3d(x, bf(w), b), LEAKY)
    got = _from_cl(y, cout)
    torch.testing.assert_close(got, ref, rtol=3e-2, atol=3e-2)
    # the kernel accumulates the statistics of the fp32 values it is about to round (what an fp32 BatchNorm would see): against
    # the sums of the stored bf16 tensor that is 2^-9 relative noise per element, averaging out with the voxel count
    st = stats.view(nrep, cout, 2).sum(0).cpu()
    nvox = got.numel() / cout
    torch.testing.assert_close(st[:, 0], got.double().sum(dim=(0, 2, 3, 4)), rtol=1e-3, atol=4e-3 * math.sqrt(nvox))
    torch.testing.assert_close(st[:, 1], (got.double() ** 2).sum(dim=(0, 2, 3, 4)), rtol=1e-3, atol=4e-3 * math.sqrt(nvox))
    # data gradient through the same kernel family (cout planes in, cin tiles out)
    dz = bf(torch.randn(ref.shape, generator=g))
    dop = P.conv_dgrad_op(cin, cout, 3, 1, 0, dims, cout, cin, L.SP_BF16)
    drun = O.ConvRunner(dop, DEV, zm_batch=B)
    assert drun.uses_zm()
    drun.prep(w.to(DEV))
    gbuf = O.alloc_cl(B, dims, cin, L.SP_BF16, DEV)
    gbuf.fill_(7.0)
    drun.run(_to_cl(dz, cout), gbuf, B)
    torch.testing.assert_close(_from_cl(gbuf, cin), F.conv_transpose3d(dz, bf(w)), rtol=3e-2, atol=3e-2)
    # the planar (plane-major) input layout of the concat buffers
    if cin >= 32:
        xp = xs.view(B, *dims, cin // 16, 16).permute(4, 0, 1, 2, 3, 5).contiguous().view(B, *dims, cin)
        y2 = O.alloc_cl(B, op.y_dims, cout, L.SP_BF16, DEV)
        run.run(xp, y2, B, None, None, L.ACT_LEAKY, LEAKY, None, x_planar=True)
        assert torch.equal(y2, y)


ZR_CASES = [   # cin, cout, input dims, batch, plane-major input, workgroups (None: the production choice)
    (16, 16, (11, 21, 45), 2, False, None), (16, 16, (13, 10, 70), 1, False, 24), (32, 16, (9, 13, 40), 2, False, None),
    (16, 32, (7, 15, 36), 2, False, 8), (32, 32, (8, 12, 37), 2, False, None), (48, 16, (6, 19, 37), 1, True, 16),
    (96, 32, (5, 11, 35), 2, True, None), (64, 64, (7, 9, 11), 2, False, None), (32, 64, (9, 9, 9), 3, False, 40),
]
ZR_CASES = [c + ((0, 0, 0),) for c in ZR_CASES] + [      # the CAE's padded layers (Cae3D.py:41-70, 186-218)
    (16, 16, (9, 20, 37), 2, False, None, (1, 0, 0)), (32, 32, (7, 12, 35), 1, False, 16, (1, 2, 2)),
    (16, 32, (6, 14, 33), 2, False, None, (1, 1, 1)), (32, 16, (3, 9, 31), 2, False, 24, (2, 2, 2)),
]


@pytest.mark.parametrize("cin,cout,dims,B,planar,nblocks,pad", ZR_CASES)
def test_row_sliding_weight_gradient_matches_autograd(cin, cout, dims, B, planar, nblocks, pad, monkeypatch):
    """csrc/sp_wgrad_zr.hip alone (every (cout tile, cin tile) blocking, ragged rows and widths, pieces that start in the
    middle of a column, more workgroups than planes, plane-major concat input) against F.conv3d autograd on the same
    bf16-rounded operands, and against the tap-major kernels it replaces (same operands: fp32 summation order only)."""
    g = torch.Generator().manual_seed(cin * 11 + cout)
    od = tuple(d - 2 + 2 * q for d, q in zip(dims, pad))
    x = bf(torch.randn(B, cin, *dims, generator=g))
    dz = bf(torch.randn(B, cout, *od, generator=g))
    wr = torch.zeros(cout, cin, 3, 3, 3, requires_grad=True)
    F.conv3d(x, wr, padding=pad).backward(dz)
    xs, dzs = _to_cl(x, cin), _to_cl(dz, cout)
    if planar:
        xs = xs.view(B, *dims, cin // 16, 16).permute(4, 0, 1, 2, 3, 5).contiguous().view(B, *dims, cin)
    got = {}
    for zr in ("1", "0"):
        monkeypatch.setenv("SP_WGRAD_ZR", zr)        # read per launch (sp_wgrad_zr.hip)
        if nblocks is not None:
            monkeypatch.setenv("SP_WGRAD_BLOCKS", str(nblocks))
        wg = O.WgradRunner(cin, cout, 3, 1, pad, dims, od, cin, cout, cin * 27, 27, L.SP_BF16, DEV)
        assert wg.dma
        dw = torch.zeros(cout, cin, 3, 3, 3, device=DEV)
        wg.run(xs, dzs, B, dw, x_planar=planar)
        got[zr] = dw.cpu()
    scale = float(wr.grad.abs().max())
    torch.testing.assert_close(got["1"], wr.grad, rtol=2e-3, atol=2e-3 * scale)
    torch.testing.assert_close(got["1"], got["0"], rtol=1e-4, atol=1e-4 * scale)


@pytest.mark.parametrize("C0,C1,ldims,B", [(32, 16, (5, 7, 9), 2), (64, 32, (3, 4, 6), 1), (16, 16, (2, 2, 2), 3)])
def test_row_ordered_upsample_crop_concat(C0, C1, ldims, B):
    """sp_upsample2_crop_cat_fwd with a plane-major output (upcat_rows_kernel: one 16-channel plane per blockIdx.y, lanes
    along the output row) against F.interpolate + crop + cat (Unet3D.py:67-72), with the statistics of every channel."""
    g = torch.Generator().manual_seed(C0 + C1)
    low = bf(torch.randn(B, C0, *ldims, generator=g))
    sdims = tuple(2 * d + 4 + 2 * (i % 2) for i, d in enumerate(ldims))
    skip = bf(torch.randn(B, C1, *sdims, generator=g))
    cdims = tuple(2 * d for d in ldims)
    off = [(sdims[a] - cdims[a]) // 2 for a in range(3)]
    ref = torch.cat((F.interpolate(low, scale_factor=2, mode="trilinear", align_corners=False),
                     skip[:, :, off[0]:off[0] + cdims[0], off[1]:off[1] + cdims[1], off[2]:off[2] + cdims[2]]), 1)
    lows, skips = _to_cl(low, C0), _to_cl(skip, C1)
    cat = O.alloc_cl(B, cdims, C0 + C1, L.SP_BF16, DEV)
    cat.fill_(3.0)
    st = O.reduce_rows(C0 + C1, 2, DEV)
    O.upsample2_crop_cat_fwd(lows, skips, cat, L.SP_BF16, st, planar=True)
    np_ = (C0 + C1) // 16
    got_cl = cat.view(np_, B, *cdims, 16).permute(1, 2, 3, 4, 0, 5).reshape(B, *cdims, C0 + C1).contiguous()
    got = _from_cl(got_cl, C0 + C1)
    torch.testing.assert_close(got, ref, rtol=1e-2, atol=1e-2)
    torch.testing.assert_close(got[:, C0:], ref[:, C0:], rtol=0, atol=0)           # the crop is a copy
    st = st.sum(0).cpu()
    torch.testing.assert_close(st[:, 0], got.double().sum(dim=(0, 2, 3, 4)), rtol=1e-5, atol=1e-3)
    torch.testing.assert_close(st[:, 1], (got.double() ** 2).sum(dim=(0, 2, 3, 4)), rtol=1e-5, atol=1e-3)
    # the channels-last (block-per-thread) kernel computes the same tensor up to the last bf16 bit
    cat2 = O.alloc_cl(B, cdims, C0 + C1, L.SP_BF16, DEV)
    O.upsample2_crop_cat_fwd(lows, skips, cat2, L.SP_BF16, None, planar=False)
    torch.testing.assert_close(_from_cl(cat2, C0 + C1), got, rtol=8e-3, atol=1e-3)


@pytest.mark.parametrize("cin,cout,grad,fold", [(16, 16, 0, True), (32, 32, 0, False), (48, 16, 0, True), (16, 32, 1, False),
                                                (32, 16, 1, False)])
def test_header_only_conv3d_entry_points(cin, cout, grad, fold):
    """include/stroke_amd.h alone (sp_conv3d_plan / _init / _set_weights / _run: no runtime/plan.py, no ConvRunner): a valid
    3x3x3 convolution with a folded BatchNorm, bias and LeakyReLU, and the data gradient, against torch on bf16 operands"""
    import ctypes as C
    lib = L.load()
    B, dims = 2, (9, 21, 37)
    g = torch.Generator().manual_seed(cin + 3 * cout + grad)
    d = L.Conv3dDesc(B, cin, cout, *dims, grad)
    pl = L.Conv3dPlan()
    assert lib.sp_conv3d_plan(C.byref(d), C.byref(pl)) == 0, L.last_error()
    ws = torch.empty(pl.workspace_bytes, dtype=torch.uint8, device=DEV)
    st = O.stream()
    assert lib.sp_conv3d_init(C.byref(d), C.byref(pl), ws.data_ptr(), st) == 0, L.last_error()
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) / math.sqrt(27 * cin)
    b = torch.randn(cout, generator=g) * 0.1
    scale, shift = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.1
    wd, bd, scd, shd = w.to(DEV), b.to(DEV), scale.to(DEV), shift.to(DEV)
    if grad:
        dz = bf(torch.randn(B, cout, *(x - 2 for x in dims), generator=g))
        xin = _to_cl(dz, cout)
        assert lib.sp_conv3d_set_weights(C.byref(d), C.byref(pl), ws.data_ptr(), wd.data_ptr(), None, None, None, st) == 0, L.last_error()
        ref = F.conv_transpose3d(dz, bf(w))
    else:
        x = bf(torch.randn(B, cin, *dims, generator=g))
        xin = _to_cl(x, cin)
        assert lib.sp_conv3d_set_weights(C.byref(d), C.byref(pl), ws.data_ptr(), wd.data_ptr(), bd.data_ptr(),
                                         scd.data_ptr() if fold else None, shd.data_ptr() if fold else None, st) == 0, L.last_error()
        if fold:
            ref = F.conv3d(x, bf(w * scale.view(1, -1, 1, 1, 1))) + (b + (w * shift.view(1, -1, 1, 1, 1)).sum((1, 2, 3, 4))).view(1, -1, 1, 1, 1)
        else:
            ref = F.conv3d(x, bf(w), b)
        ref = F.leaky_relu(ref, LEAKY)
    assert xin.numel() == pl.x_elems
    y = torch.full((B, pl.Do, pl.Ho, pl.Wo, pl.cout_op), 7.0, dtype=torch.bfloat16, device=DEV)
    assert y.numel() == pl.y_elems
    nrep = 4
    stats = torch.zeros(nrep, pl.cout_op, 2, dtype=torch.float64, device=DEV)
    rc = lib.sp_conv3d_run(C.byref(d), C.byref(pl), ws.data_ptr(), xin.data_ptr(), y.data_ptr(), 0 if grad else 1,
                           L.ACT_NONE if grad else L.ACT_LEAKY, LEAKY, None if grad else stats.data_ptr(), nrep, 0, st)
    assert rc == 0, L.last_error()
    got = _from_cl(y, pl.cout_op)
    torch.testing.assert_close(got, ref, rtol=3e-2, atol=3e-2)
    if not grad:
        torch.testing.assert_close(stats.sum(0)[:, 0].cpu(), got.double().sum((0, 2, 3, 4)), rtol=1e-3, atol=4e-3 * math.sqrt(got.numel() / cout))


@pytest.mark.parametrize("cin,cout,fold", [(16, 16, True), (32, 16, False), (16, 32, True), (48, 16, True)])
def test_header_only_weight_gradient_entry_points(cin, cout, fold):
    """the third GEMM of the layer from include/stroke_amd.h alone (sp_conv3d_wgrad_plan / _init / _run: no
    runtime/plan.py, no WgradRunner) -- dW, the bias gradient and, with the BatchNorm folded, the BatchNorm-backward sums -- against
    F.conv3d autograd on the same bf16 operands.  Together with sp_conv3d_plan(grad = 0 / 1) a C caller trains one Block3x3x3 conv."""
    import ctypes as C
    lib = L.load()
    B, dims = 2, (9, 21, 37)
    g = torch.Generator().manual_seed(cin * 5 + cout + int(fold))
    d = L.Conv3dDesc(B, cin, cout, *dims, 2)
    pl = L.Conv3dWgradPlan()
    assert lib.sp_conv3d_wgrad_plan(C.byref(d), C.byref(pl)) == 0, L.last_error()
    assert (pl.Do, pl.Ho, pl.Wo) == tuple(x - 2 for x in dims) and pl.nblocks % 8 == 0
    ws = torch.empty(pl.workspace_bytes, dtype=torch.uint8, device=DEV)
    st = O.stream()
    assert lib.sp_conv3d_wgrad_init(C.byref(d), C.byref(pl), ws.data_ptr(), st) == 0, L.last_error()
    x = bf(torch.randn(B, cin, *dims, generator=g))
    dz = bf(torch.randn(B, cout, pl.Do, pl.Ho, pl.Wo, generator=g))
    w = (torch.randn(cout, cin, 3, 3, 3, generator=g) / math.sqrt(27 * cin))
    scale, shift = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.1
    xd, dzd, wd, scd, shd = _to_cl(x, cin), _to_cl(dz, cout), w.to(DEV), scale.to(DEV), shift.to(DEV)
    dw = torch.zeros(cout, cin, 3, 3, 3, device=DEV)
    db = torch.zeros(cout, device=DEV)
    dbias_sums = dz.double().sum((0, 2, 3, 4)).to(DEV)                # one row (dbias_stride = 0)
    nrep = 4
    bn_sums = torch.zeros(nrep, cin, 2, dtype=torch.float64, device=DEV)
    rc = lib.sp_conv3d_wgrad_run(C.byref(d), C.byref(pl), ws.data_ptr(), xd.data_ptr(), dzd.data_ptr(), dw.data_ptr(),
                                 scd.data_ptr() if fold else None, shd.data_ptr() if fold else None, dbias_sums.data_ptr(), 0, db.data_ptr(),
                                 wd.data_ptr() if fold else None, bn_sums.data_ptr() if fold else None, nrep, 0, st)
    assert rc == 0, L.last_error()
    # reference: autograd of conv3d(scale * x + shift, w) contracted with dz
    xin = (x * scale.view(1, -1, 1, 1, 1) + shift.view(1, -1, 1, 1, 1)) if fold else x
    xin = xin.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    (F.conv3d(xin, wr) * dz).sum().backward()
    scale_ref = float(wr.grad.abs().max())
    assert float((dw.cpu() - wr.grad).abs().max()) < 2e-2 * scale_ref + 1e-3, (float((dw.cpu() - wr.grad).abs().max()), scale_ref)
    torch.testing.assert_close(db.cpu(), dz.sum((0, 2, 3, 4)), rtol=1e-4, atol=1e-3)
    if fold:      # BatchNorm-backward sums of the input gradient g = conv_transpose(dz, w): (sum g, sum g * x) per input channel
        gin = F.conv_transpose3d(dz, w)
        ref = torch.stack((gin.double().sum((0, 2, 3, 4)), (gin.double() * x.double()).sum((0, 2, 3, 4))), 1)
        got = bn_sums.sum(0).cpu()
        torch.testing.assert_close(got, ref, rtol=2e-2, atol=2e-2 * float(ref.abs().max()))
    # descriptors the entry points must refuse, with a message
    bad = L.Conv3dDesc(1, 24, 16, 9, 9, 9, 2)
    assert lib.sp_conv3d_wgrad_plan(C.byref(bad), C.byref(pl)) != 0 and "multiples of 16" in L.last_error()


@pytest.mark.parametrize("cin,cout,dims,B,pad", [(16, 16, (9, 36, 40), 2, (1, 0, 0)), (24, 24, (6, 34, 36), 1, (1, 2, 2)),
                                                 (16, 24, (5, 33, 20), 2, (1, 1, 1)), (32, 16, (4, 40, 17), 2, (0, 0, 0))])
def test_z_marching_kernel_padded_elu(cin, cout, dims, B, pad):
    """the CAE's stride-1 3x3x3 layers on the z-marching kernel: zero padding from the zero page, ELU epilogue, channel
    counts that are not multiples of 16 (24 -> pitch 32, zero weights and bias on the pad channels), statistics"""
    from stroke_prediction_amd.runtime import plan as P
    O.ZM_MIN_PLANES = 0
    g = torch.Generator().manual_seed(cin * 5 + cout)
    cpi, cpo = O.cpad(cin, 16), O.cpad(cout, 16)
    x = bf(torch.randn(B, cin, *dims, generator=g))
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) / math.sqrt(27 * cin)
    b = torch.randn(cout, generator=g) * 0.1
    op = P.conv_fwd_op(cin, cout, 3, 1, pad, dims, cpi, cpo, L.SP_BF16)
    run = O.ConvRunner(op, DEV, zm_batch=B)
    assert run.uses_zm()
    run.prep(w.to(DEV), b.to(DEV))
    xs = _to_cl(x, cpi)
    y = O.alloc_cl(B, op.y_dims, cpo, L.SP_BF16, DEV)
    y.fill_(7.0)
    nrep = 4
    stats = torch.zeros(nrep * cpo * 2, dtype=torch.float64, device=DEV)
    run.run(xs, y, B, None, None, L.ACT_ELU, 1.0, stats, stats_nrep=nrep)
    ref = F.elu(F.conv3d(x, bf(w), b, padding=pad), 1.0)
    got = _from_cl(y, cout)
    torch.testing.assert_close(got, ref, rtol=3e-2, atol=3e-2)
    if cpo > cout:
        assert float(y[..., cout:].float().abs().max()) == 0.0
    st = stats.view(nrep, cpo, 2).sum(0).cpu()
    nvox = got.numel() / cout
    torch.testing.assert_close(st[:cout, 0], got.double().sum(dim=(0, 2, 3, 4)), rtol=1e-3, atol=4e-3 * math.sqrt(nvox))
    torch.testing.assert_close(st[:cout, 1], (got.double() ** 2).sum(dim=(0, 2, 3, 4)), rtol=1e-3, atol=4e-3 * math.sqrt(nvox))
    assert float(st[cout:].abs().max()) == 0.0 if cpo > cout else True


# ------------------------------------------------------------------------------------------------ multi-step fixtures
def _build(ch, seed, dtype, cls=Unet3D):
    model = cls(ch, dtype=dtype)
    model.load_state_dict(W.make_state_dict(W.unet_spec(ch), seed))
    return model.to(DEV)


@pytest.mark.parametrize("fname", ["unet_44.npz", "unet_48.npz", "unet_44x48x52.npz"])
def test_unet_three_fusedadam_steps_match_reference_fixture(golden_dir, fname):
    """forward + (Dice + Dice) / 2 + backward + FusedAdam, three times, against what three steps of the REAL reference
    (torch.optim.Adam lr 1e-3, betas (0.99, 0.999), weight decay 1e-5) left behind: the losses of steps 1 and 2, the
    BatchNorm running statistics after step 3, the parameters after step 3, and the eval-mode segmentation of the trained
    model.  Adam's first updates are lr * sign(g): an element whose tiny gradient changes sign (LeakyReLU kink flips,
    test_gpu_unet.py) moves by 2 lr instead of 0 -- hence a bulk criterion plus a hard bound of 3 steps x 2 lr."""
    from stroke_prediction_amd.optim import FusedAdam
    fx = np.load(os.path.join(golden_dir, fname))
    seed = int(fx["seed"])
    size = tuple(int(s) for s in np.atleast_1d(fx["size"]))
    size = size * 3 if len(size) == 1 else size
    x, y = W.unet_inputs(2, size, seed)
    xd, yd = x.to(DEV), y.to(DEV)
    model = _build(CH, seed, "f32").train()
    opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=1e-5, betas=(0.99, 0.999))
    for step in range(3):
        dto = model(UnetDtoUtil.init_dto(xd, yd[:, 0:1], yd[:, 1:2]))
        loss = nets.unet_loss(torch.cat((dto.outputs.core, dto.outputs.penu), 1), yd)
        # runs are bit-reproducible since round 3 (ordered reductions, tests/test_gpu_round3.py); what remains is the distance
        # from the reference's own summation orders, amplified by Adam's lr * sign(g) first steps on bottleneck weights with
        # |g| ~ eps: measured 9e-8 / 1e-5 / 1.3e-4 over the three fixtures (tools/probes/three_step_spread.py; the loss falls by
        # 1.2e-2 per step)
        tol = (1e-6, 5e-5, 5e-4)[step]
        assert abs(loss.item() - float(fx["loss/%d" % step])) < tol, (step, loss.item(), float(fx["loss/%d" % step]))
        opt.zero_grad()
        loss.backward()
        opt.step()
        if step in (0, 2):
            for n, b in model.named_buffers():
                if n.endswith("num_batches_tracked"):
                    assert int(b) == step + 1
                else:      # after three steps the parameters carry the 2 lr sign flips described above: looser
                    np.testing.assert_allclose(b.cpu().numpy(), fx["buf%d/%s" % (step + 1, n)], rtol=5e-3,
                                               atol=2e-4 if step == 0 else 5e-3, err_msg=n)
    diffs, total = [], 0
    for n, p in model.named_parameters():
        d = np.abs(p.detach().reshape(-1)[:8].cpu().numpy() - fx["phead3/" + n])
        assert d.max() <= 6.5e-3, (n, d.max())
        diffs.append(d)
        pn = float(fx["pnorm3/" + n])
        assert abs(float(p.detach().double().norm()) - pn) <= 2e-3 * pn + 2e-3, n
    diffs = np.concatenate(diffs)
    assert (diffs <= 3e-4).mean() >= 0.8, float((diffs <= 3e-4).mean())
    model.eval()
    with torch.no_grad():
        dto = model(UnetDtoUtil.init_dto(xd))
    seg = torch.cat((dto.outputs.core, dto.outputs.penu), 1).cpu().numpy()
    np.testing.assert_allclose(seg, fx["seg_eval3"], rtol=0, atol=5e-3)


@pytest.mark.parametrize("fname,dtype", [("unet4_92.npz", "f32"), ("unet4_92x100x96.npz", "f32"), ("unet4_92.npz", "bf16")])
def test_four_scale_unet_matches_reference_fixture(golden_dir, fname, dtype):
    """BASELINE configs[4] topology (2 32 64 128 256 128 64 32 [32] 2): ``LargeUnet3D`` on the HIP path against outputs,
    loss and gradient norms recorded from the reference's own class (tests/golden/make_golden.py:reference_large_unet)."""
    fx = np.load(os.path.join(golden_dir, fname))
    seed = int(fx["seed"])
    ch = [int(c) for c in fx["channels"]]
    assert ch == CH4
    size = tuple(int(s) for s in np.atleast_1d(fx["size"]))
    size = size * 3 if len(size) == 1 else size
    x, y = W.unet_inputs(2, size, seed, scales=4)
    model = _build(ch, seed, dtype, LargeUnet3D).train()
    assert tuple(model.output_size(size)) == tuple(y.shape[2:])
    dto = model(UnetDtoUtil.init_dto(x.to(DEV)))
    seg = torch.cat((dto.outputs.core, dto.outputs.penu), 1)
    tol = 1e-4 if dtype == "f32" else 2.5e-2
    np.testing.assert_allclose(seg.detach().cpu().numpy(), fx["seg"], rtol=0, atol=tol)
    if dtype == "f32":      # north_star: logits within 1e-3 relative
        lg = lambda p: np.log(p / (1 - p))
        a, r = lg(seg.detach().cpu().double().numpy()), lg(fx["seg"].astype(np.float64))
        assert np.abs(a - r).max() / np.abs(r).max() < 1e-3
    loss = nets.unet_loss(seg, y.to(DEV))
    assert abs(loss.item() - float(fx["loss/0"])) < (1e-5 if dtype == "f32" else 5e-3)
    loss.backward()
    bad = []
    for name, p in model.named_parameters():
        gn = float(fx["gnorm/" + name])
        rel = abs(float(p.grad.double().norm()) - gn) / (gn + 1e-12)
        small = p.numel() <= 64         # cancellation-heavy BatchNorm / bias gradients (test_gpu_unet.py): 2x head-room in
        tol = (6e-2 if small else 3e-2) if dtype == "f32" else (1.0 if small else 0.35)      # parity mode, norm only in bf16
        if rel > tol:
            bad.append((name, rel, gn))
    assert not bad, bad
    for n, b in model.named_buffers():
        if n.endswith("num_batches_tracked"):
            assert int(b) == 1


def test_four_scale_bf16_matches_emulating_oracle():
    """fast mode of the 4-scale net against the oracle run with the same bf16 storage points (as the 3-scale net is tested)"""
    seed, size = 33, (92, 92, 92)
    x, y = W.unet_inputs(2, size, seed, scales=4)
    sd = W.make_state_dict(W.unet_spec(CH4), seed)
    with torch.no_grad():
        ref = nets.unet_forward(sd, x, training=True, q=nets.round_bf16)
    model = _build(CH4, seed, "bf16", LargeUnet3D).train()
    dto = model(UnetDtoUtil.init_dto(x.to(DEV)))
    seg = torch.cat((dto.outputs.core, dto.outputs.penu), 1).detach().cpu()
    torch.testing.assert_close(seg, ref, rtol=0, atol=1.2e-2)


# ------------------------------------------------------------------------------------------------ ADVICE r1 regressions
def test_weight_cache_follows_load_state_dict_and_torch_optim():
    """packed-weight caches must see parameter changes made outside FusedAdam."""
    seed = 11
    x, y = W.unet_inputs(2, (44, 44, 44), seed)
    xd, yd = x.to(DEV), y.to(DEV)
    model = _build(CH, seed, "f32").eval()

    def fwd(m):
        with torch.no_grad():
            dto = m(UnetDtoUtil.init_dto(xd))
        return torch.cat((dto.outputs.core, dto.outputs.penu), 1).clone()

    a = fwd(model)
    other = W.make_state_dict(W.unet_spec(CH), seed + 1)
    model.load_state_dict(other)
    b = fwd(model)
    ref = fwd(_build(CH, seed + 1, "f32").eval())
    assert float((a - b).abs().max()) > 1e-3, "forward did not change after load_state_dict"
    torch.testing.assert_close(b, ref, rtol=0, atol=1e-6)
    # torch.optim.Adam (what the reference's scripts build) on the HIP model: outputs must follow the updates, and the
    # data-gradient weights too (second step's gradients differ from a stale-cache run)
    model = _build(CH, seed, "f32").train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    outs = []
    for step in range(3):
        dto = model(UnetDtoUtil.init_dto(xd, yd[:, 0:1], yd[:, 1:2]))
        seg = torch.cat((dto.outputs.core, dto.outputs.penu), 1)
        outs.append(seg.detach().clone())
        loss = nets.unet_loss(seg, yd)
        opt.zero_grad()
        loss.backward()
        opt.step()
    assert float((outs[1] - outs[0]).abs().max()) > 1e-4 and float((outs[2] - outs[1]).abs().max()) > 1e-4
    # in-place edit through .data (invisible to version counters) + explicit epoch bump still works
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(1.0)
    # CAE with torch.optim.Adam: the un-folded conv fragments were the stale ones
    from stroke_prediction_amd.common.model.Cae3D import Cae3D, Enc3D, Dec3D
    ch = [1, 16, 24, 32, 100, 200, 1]
    cae = Cae3D(Enc3D(64, 28, ch, 5, 1.0, dtype="f32"), Dec3D(64, 28, ch, 5, 1.0, dtype="f32"))
    cae.load_state_dict(W.make_state_dict(W.cae_spec(ch), 5))
    cae = cae.to(DEV).train()
    labels, _ = W.cae_inputs(2, 28, 64, 5)
    vol = labels[:, 0:1].to(DEV)
    opt = torch.optim.Adam(cae.parameters(), lr=1e-2)
    recs = []
    for step in range(2):
        rec = cae.dec._forward_single(cae.enc._forward_single(vol))
        recs.append(rec.detach().clone())
        loss = ((rec - vol) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
    assert float((recs[1] - recs[0]).abs().max()) > 1e-4, "CAE forward ignores torch.optim.Adam updates"


def test_second_forward_before_backward_is_refused_and_eval_backward_too():
    """activations live in the per-shape engine; a stale backward must raise, not return garbage."""
    seed = 11
    x, y = W.unet_inputs(2, (44, 44, 44), seed)
    xd, yd = x.to(DEV), y.to(DEV)
    model = _build(CH, seed, "f32").train()
    dto1 = model(UnetDtoUtil.init_dto(xd))
    loss1 = nets.unet_loss(torch.cat((dto1.outputs.core, dto1.outputs.penu), 1), yd)
    dto2 = model(UnetDtoUtil.init_dto(xd * 0.5))          # same shape: overwrites the activations of the first pass
    with pytest.raises(RuntimeError, match="another forward pass"):
        loss1.backward()
    loss2 = nets.unet_loss(torch.cat((dto2.outputs.core, dto2.outputs.penu), 1), yd)
    loss2.backward()                                       # the resident pass still differentiates
    # a no_grad / eval forward in between is the same hazard
    dto3 = model(UnetDtoUtil.init_dto(xd))
    loss3 = nets.unet_loss(torch.cat((dto3.outputs.core, dto3.outputs.penu), 1), yd)
    with torch.no_grad():
        model(UnetDtoUtil.init_dto(xd))
    with pytest.raises(RuntimeError, match="another forward pass"):
        loss3.backward()
    model.eval()
    dto4 = model(UnetDtoUtil.init_dto(xd))
    loss4 = nets.unet_loss(torch.cat((dto4.outputs.core, dto4.outputs.penu), 1), yd)
    with pytest.raises(RuntimeError, match="eval-mode forward"):
        loss4.backward()
    # CAE: a grad-enabled forward that is never differentiated returns its context to the pool when the graph dies
    from stroke_prediction_amd.common.model.Cae3D import Enc3D
    import gc
    ch = [1, 16, 24, 32, 100, 200, 1]
    enc = Enc3D(64, 28, ch, 5, 1.0, dtype="bf16").to(DEV).train()
    vol = torch.rand(2, 1, 28, 64, 64, device=DEV)
    for _ in range(5):
        out = enc._forward_single(vol)
        del out
        gc.collect()
    pool = enc._pool()
    assert sum(len(v) for v in pool.free.values()) >= 1, "contexts of dropped graphs were not released"
    created = sum(len(v) for v in pool.free.values())
    assert created <= 2, created


def test_fusedadam_state_dict_round_trip_and_reflatten(tmp_path):
    """load_state_dict must replace the flat moments; capturable step counts must be saved and
    survive a .cpu()/.cuda() round trip of the model (Learner.save_model)."""
    from stroke_prediction_amd.optim import FusedAdam
    seed = 11
    x, y = W.unet_inputs(2, (44, 44, 44), seed)
    xd, yd = x.to(DEV), y.to(DEV)

    def run(model, opt, n):
        for _ in range(n):
            dto = model(UnetDtoUtil.init_dto(xd, yd[:, 0:1], yd[:, 1:2]))
            loss = nets.unet_loss(torch.cat((dto.outputs.core, dto.outputs.penu), 1), yd)
            opt.zero_grad()
            loss.backward()
            opt.step()
        return float(loss)

    for capturable in (False, True):
        a = _build(CH, seed, "f32").train()
        oa = FusedAdam(a.parameters(), lr=1e-3, betas=(0.99, 0.999), capturable=capturable)
        run(a, oa, 2)
        sd_model = {k: v.clone() for k, v in a.state_dict().items()}
        sd_opt = oa.state_dict()
        assert all(int(s["step"]) == 2 for s in sd_opt["state"].values()), "step count not saved"
        path = str(tmp_path / "o.optim")
        torch.save(sd_opt, path)
        la = run(a, oa, 1)                                   # third step of the original
        # a fresh pair that already took a (different) step, then loads the checkpoint: must continue identically
        b = _build(CH, seed + 1, "f32").train()
        ob = FusedAdam(b.parameters(), lr=1e-3, betas=(0.99, 0.999), capturable=capturable)
        run(b, ob, 1)
        b.load_state_dict(sd_model)
        ob.load_state_dict(torch.load(path, weights_only=False))
        lb = run(b, ob, 1)
        # two runs of the same step differ by ~1e-7 in the gradients (order of the fp64 statistics atomics); Adam turns that
        # into up to ~1e-4 * lr-sized differences on elements whose gradient is of the order of eps (tools/dbg_steps.py).
        # A lost moment buffer or a restarted bias correction shows as O(lr) = 1e-3 on EVERY element.
        assert abs(la - lb) < 1e-5, (capturable, la, lb)
        for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
            d = (p - q).abs()
            assert float(d.max()) <= 2e-4 and float(d.mean()) <= 2e-6, (capturable, n, float(d.max()), float(d.mean()))
        # the save_model round trip re-flattens: bias correction must not restart
        a.cpu()
        a.to(DEV)
        run(a, oa, 1)
        oa.state_dict()
        assert all(int(s["step"]) == 4 for s in oa.state_dict()["state"].values())


def test_learner_graph_mode_matches_eager_and_follows_schedulers(tmp_path):
    """``Learner(graph=True)`` replays train_batch as one hipGraph; MultiStepLR and adapt_betas must
    still change the update under replay (hyper-parameters are read from device memory)."""
    from stroke_prediction_amd.optim import FusedAdam, attach_flat_grads
    from stroke_prediction_amd.common.metrics import BatchDiceLoss
    from stroke_prediction_amd.learner.UnetSegmentationLearner import UnetSegmentationLearner

    class Loader(list):
        batch_size = 2
    seed = 11
    x, y = W.unet_inputs(2, (52, 52, 52), seed)
    batches = [{"case_id": [0, 1], "images": x * (1.0 + 0.1 * i), "labels": y, "clinical": torch.zeros(2, 5, 1, 1, 1)} for i in range(2)]
    traj = {}
    for tag, graph in (("eager", False), ("eager2", False), ("graph", True)):
        model = _build(CH, seed, "f32").train()
        opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=1e-5, betas=(0.99, 0.999), capturable=True)
        attach_flat_grads(model)
        sched = torch.optim.lr_scheduler.MultiStepLR(opt, [1], gamma=0.1)        # epoch 1 onwards: lr 1e-4
        learner = UnetSegmentationLearner(Loader(batches), None, model, opt, sched, 3, BatchDiceLoss([1.0]), None,
                                          str(tmp_path / tag), graph=graph, batch_metrics=False)
        learner.GRAPH_WARMUP = 1
        losses, deltas = [], []
        for epoch in range(3):
            if epoch > 0:
                learner.adapt_lr(epoch)
            for b in batches:
                before = model.flat_buffers()[0].clone()
                losses.append(learner.train_batch(b, epoch).loss)
                deltas.append(float((model.flat_buffers()[0] - before).abs().max()))
        traj[tag] = (np.array(losses), np.array(deltas), model.flat_buffers()[0].clone())
        if graph:
            assert any(g["graph"] is not None for g in learner._graphs.values()), "no step was captured"
    le, de, pe = traj["eager"]
    l2, d2, p2 = traj["eager2"]
    lg, dg, pg = traj["graph"]
    # Two eager runs of the same trajectory already differ: the fp64 BatchNorm atomics change the last bit of a scale, a
    # LeakyReLU branch flips, and Adam's sign-like first updates turn that into 2 lr on an element.  The replayed graph must
    # stay within three times that run-to-run distance of the eager trajectory (floor 2e-4).
    noise = np.abs(l2 - le)
    print("eager-vs-eager loss distance", noise, "graph-vs-eager", np.abs(lg - le))
    assert np.all(np.abs(lg - le) <= np.maximum(3.0 * noise, 2e-4) + 2e-3 * (np.arange(len(le)) >= 2)), (lg, le, l2)
    # the first steps move every element by ~lr (Adam): after the milestone the largest move must shrink ~10x -- in BOTH modes
    assert de[0] > 5e-4 and de[-1] < 0.35 * de[1], de
    assert dg[0] > 5e-4 and dg[-1] < 0.35 * dg[1], dg
    np.testing.assert_allclose(dg, de, rtol=0.25, atol=1e-5)
    assert float((pg - pe).abs().max()) < 8e-3


def test_learner_split_graph_keeps_the_gradient_exchange_outside_the_capture(tmp_path):
    """Data-parallel replicas under ``Learner(graph=True)``: forward + loss + backward are replayed as one hipGraph, the
    exchange installed by ``parallel.DataParallelSync`` (here: a stand-in that scales the flat gradient buffer, i.e. a
    2-rank all-reduce of identical replicas followed by FusedAdam(grad_scale=1/2)) runs once per step on the whole buffer
    BETWEEN the graph and the fused Adam launch -- never inside the capture, never twice."""
    from stroke_prediction_amd.optim import FusedAdam, attach_flat_grads
    from stroke_prediction_amd.common.metrics import BatchDiceLoss
    from stroke_prediction_amd.learner.UnetSegmentationLearner import UnetSegmentationLearner

    class Loader(list):
        batch_size = 2
    seed = 11
    x, y = W.unet_inputs(2, (52, 52, 52), seed)
    batch = {"case_id": [0, 1], "images": x, "labels": y, "clinical": torch.zeros(2, 5, 1, 1, 1)}
    out = {}
    for tag, graph in (("eager", False), ("graph", True)):
        model = _build(CH, seed, "f32").train()
        opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=1e-5, betas=(0.99, 0.999), capturable=True, grad_scale=0.5)
        attach_flat_grads(model)
        calls = []

        def fake_sync(flat_grad, lo=0, hi=None, calls=calls):
            assert not torch.cuda.is_current_stream_capturing(), "the exchange must not be captured"
            calls.append(("sync", lo, flat_grad.numel() if hi is None else hi))
            flat_grad[lo:hi].mul_(2.0)              # sum over two identical replicas

        def fake_bucket(flat_grad, lo, hi, calls=calls):
            assert not torch.cuda.is_current_stream_capturing(), "the exchange must not be captured"
            calls.append(("bucket", lo, hi))
            flat_grad[lo:hi].mul_(2.0)
        model.grad_sync, model.grad_bucket_ready = fake_sync, fake_bucket
        learner = UnetSegmentationLearner(Loader([batch]), None, model, opt, None, 1, BatchDiceLoss([1.0]), None,
                                          str(tmp_path / tag), graph=graph, batch_metrics=False)
        learner.GRAPH_WARMUP = 1
        n = model.flat_buffers()[1].numel()
        per_step = []
        for step in range(4):
            del calls[:]
            learner.train_batch(batch, 0)
            covered = sorted((lo, hi) for _, lo, hi in calls)
            # every element of the flat gradient buffer exchanged exactly once per step
            assert covered[0][0] == 0 and covered[-1][1] == n and all(a[1] == b[0] for a, b in zip(covered, covered[1:])), (tag, step, calls)
            per_step.append(list(calls))
        if graph:
            assert any(g["graph"] is not None and g.get("split") for g in learner._graphs.values()), "no split capture happened"
            assert per_step[-1] == [("sync", 0, n)], per_step[-1]       # replayed steps: ONE exchange of the whole buffer
        out[tag] = model.flat_buffers()[0].clone()
    # same trajectory up to the run-to-run noise of four Adam steps (see the three-step fixture test)
    assert float((out["graph"] - out["eager"]).abs().max()) < 8e-3 and float((out["graph"] - out["eager"]).abs().mean()) < 2e-4


@pytest.mark.parametrize("cin,cout,d,B", [(256, 64, 8, 2), (384, 128, 8, 1), (272, 48, 6, 3), (192, 64, 8, 2)])
def test_many_plane_concat_input_small_volume(cin, cout, d, B):
    """plane-major (concat-buffer) input with 12-24 planes at the tiny volumes of the 4-scale net's deepest up block: the
    split-K kernel (Cin >= 256, few output voxels) has to read the plane-major layout too -- its fragments are the only
    ones such a runner packs"""
    from stroke_prediction_amd.runtime import plan as P
    dims = (d, d, d)
    g = torch.Generator().manual_seed(cin + cout)
    x = bf(torch.randn(B, cin, *dims, generator=g))
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) / math.sqrt(27 * cin)
    op = P.conv_fwd_op(cin, cout, 3, 1, 0, dims, cin, cout, L.SP_BF16)
    run = O.ConvRunner(op, DEV)
    assert (run.fc is not None) == (cin >= 256)
    run.prep(w.to(DEV), torch.zeros(cout, device=DEV))
    xs = _to_cl(x, cin)
    xp = xs.view(B, *dims, cin // 16, 16).permute(4, 0, 1, 2, 3, 5).contiguous().view(B, *dims, cin)
    ref = F.conv3d(x, bf(w))
    outs = []
    for planar, xin in ((False, xs), (True, xp)):
        y = O.alloc_cl(B, op.y_dims, cout, L.SP_BF16, DEV)
        run.run(xin, y, B, None, None, L.ACT_NONE, 0.0, None, x_planar=planar)
        outs.append(_from_cl(y, cout))
        torch.testing.assert_close(outs[-1], ref, rtol=3e-2, atol=3e-2)
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("kind,cin,cout,dims,B", [("fwd", 32, 64, (6, 20, 40), 2), ("fwd", 16, 80, (5, 19, 33), 1),
                                                  ("dgrad", 96, 32, (7, 18, 37), 2), ("dgrad", 64, 16, (6, 21, 20), 1)])
def test_z_marching_output_slices(kind, cin, cout, dims, B, monkeypatch):
    """ops with more output tiles than a z-marching kernel holds run as one launch per 32-channel slice of the output
    (runtime/plan.py:zm_slices): forward 32 -> 64 with bias / LeakyReLU / statistics, and the data gradient of a 96 -> 32
    convolution (32 -> 96), against torch and against the tiled kernel"""
    from stroke_prediction_amd.runtime import plan as P
    monkeypatch.setattr(O, "ZM_MIN_PLANES", 0)
    monkeypatch.setattr(O, "ZM_SLICE_MIN_PLANES", 0)
    g = torch.Generator().manual_seed(cin * 3 + cout)
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) / math.sqrt(27 * cin)
    b = torch.randn(cout, generator=g) * 0.1
    outs = {}
    for sliced in (True, False):
        monkeypatch.setattr(O, "USE_ZM_SLICES", sliced)
        if kind == "fwd":
            x = bf(torch.randn(B, cin, *dims, generator=torch.Generator().manual_seed(1)))
            op = P.conv_fwd_op(cin, cout, 3, 1, 0, dims, cin, cout, L.SP_BF16)
            run = O.ConvRunner(op, DEV, zm_batch=B)
            assert (run.zms is not None) == sliced and run.zm is None
            run.prep(w.to(DEV), b.to(DEV))
            y = O.alloc_cl(B, op.y_dims, cout, L.SP_BF16, DEV)
            y.fill_(5.0)
            nrep = 4
            stats = torch.zeros(nrep * cout * 2, dtype=torch.float64, device=DEV)
            run.run(_to_cl(x, cin), y, B, None, None, L.ACT_LEAKY, LEAKY, stats, stats_nrep=nrep)
            got = _from_cl(y, cout)
            torch.testing.assert_close(got, F.leaky_relu(F.conv3d(x, bf(w), b), LEAKY), rtol=3e-2, atol=3e-2)
            st = stats.view(nrep, cout, 2).sum(0).cpu()
            torch.testing.assert_close(st[:, 0], got.double().sum(dim=(0, 2, 3, 4)), rtol=1e-3, atol=4e-3 * math.sqrt(got.numel() / cout))
        else:
            od = tuple(v - 2 for v in dims)
            dz = bf(torch.randn(B, cout, *od, generator=torch.Generator().manual_seed(2)))
            dop = P.conv_dgrad_op(cin, cout, 3, 1, 0, dims, cout, cin, L.SP_BF16)
            run = O.ConvRunner(dop, DEV, zm_batch=B)
            assert (run.zms is not None) == sliced and run.zm is None
            run.prep(w.to(DEV))
            y = O.alloc_cl(B, dims, cin, L.SP_BF16, DEV)
            y.fill_(5.0)
            run.run(_to_cl(dz, cout), y, B)
            got = _from_cl(y, cin)
            torch.testing.assert_close(got, F.conv_transpose3d(dz, bf(w)), rtol=3e-2, atol=3e-2)
        outs[sliced] = got
    torch.testing.assert_close(outs[True], outs[False], rtol=2e-2, atol=2e-2)


@pytest.mark.parametrize("cin,cout,dims,B,fold", [(16, 16, (5, 21, 33), 2, True), (16, 1, (7, 18, 20), 2, True), (32, 32, (6, 11, 19), 1, False),
                                                  (32, 2, (4, 9, 35), 3, True), (48, 16, (3, 10, 11), 2, False)])
def test_pointwise_weight_gradient(cin, cout, dims, B, fold, monkeypatch):
    """csrc/sp_wgrad_pw.hip (1x1x1 convolutions: the CAE's tail, generic classify heads) against autograd, with the BatchNorm
    in front of the layer folded into the finish step, and against the generic kernel it replaces"""
    g = torch.Generator().manual_seed(cin * 13 + cout)
    cpi, cpo = O.cpad(cin, 16), O.cpad(cout, 8 if cout == 2 else 16)      # (the U-Net's classify output: pitch 8)
    x = bf(torch.randn(B, cin, *dims, generator=g))
    dz = bf(torch.randn(B, cout, *dims, generator=g))
    scale, shift = torch.rand(cpi, generator=g) + 0.5, torch.randn(cpi, generator=g) * 0.1
    xn = x * scale[:cin].view(1, -1, 1, 1, 1) + shift[:cin].view(1, -1, 1, 1, 1) if fold else x
    wr = torch.zeros(cout, cin, 1, 1, 1, requires_grad=True)
    F.conv3d(xn, wr).backward(dz)
    xs, dzs = _to_cl(x, cpi), _to_cl(dz, cpo)
    dbs = torch.zeros(cpo, dtype=torch.float64, device=DEV)
    dbs[:cout] = dz.double().sum((0, 2, 3, 4)).to(DEV)
    got = {}
    for pw in (True, False):
        monkeypatch.setattr(O, "USE_PW_WGRAD", pw)
        wg = O.WgradRunner(cin, cout, 1, 1, 0, dims, dims, cpi, cpo, cin, 1, L.SP_BF16, DEV)
        assert wg.pw == pw
        dw = torch.zeros(cout, cin, 1, 1, 1, device=DEV)
        db = torch.zeros(cout, device=DEV)
        if fold:
            wg.run(xs, dzs, B, dw, scale.to(DEV), shift.to(DEV), dbias_sums=dbs, dbias_grad=db, nbias=cout)
        else:
            wg.run(xs, dzs, B, dw, dbias_sums=dbs, dbias_grad=db, nbias=cout)
        got[pw] = dw.cpu()
        torch.testing.assert_close(db.cpu(), dz.sum((0, 2, 3, 4)), rtol=1e-4, atol=1e-3)
    sc = float(wr.grad.abs().max())
    torch.testing.assert_close(got[True], wr.grad, rtol=2e-3, atol=4e-3 * sc)
    torch.testing.assert_close(got[True], got[False], rtol=5e-3, atol=6e-3 * sc)
