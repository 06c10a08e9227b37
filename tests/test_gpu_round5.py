"""Round-5 GPU tests: launches folded into their consumers on the headline step's dependent chain.

* ``sp_conv_prep_folded_bn`` / ``sp_first_prep_bn``: the BatchNorm finalize (Unet3D.py:18,21 -- batch statistics -> scale / shift,
  running buffers) inside the weight re-pack kernel of the convolution it is folded into: bit-identical fragments, bias, scale /
  shift / mean / invstd and running statistics with ``sp_bn_finalize`` + ``sp_conv_prep_folded`` / ``sp_first_prep_n``;
* ``sp_conv3d_zm`` with ``stats_mode = 2``: the data gradient of a block's second convolution with the BatchNorm backward and the
  first convolution's LeakyReLU derivative in its epilogue (dz out, coefficients finalized in the kernel's prologue) against the
  three-kernel path it replaces (data gradient -> ``sp_bn_bwd_finalize`` -> ``sp_bn_act_bwd``) and against float64 torch;
* ``sp_conv3d_zm`` with ``pool_y``: MaxPool3d(2) (Unet3D.py:59,62) in the epilogue of the down blocks' second convolution, with the
  statistics of the pooled tensor, against the convolution followed by ``sp_maxpool2_fwd`` (bit-identical tensors);
* the whole training step with all of them on and off: same losses, gradients and BatchNorm buffers.
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from stroke_prediction_amd.runtime import lib as L
from stroke_prediction_amd.runtime import ops as O
from stroke_prediction_amd.runtime import plan as P
from stroke_prediction_amd.runtime import layers as LY

DEV = "cuda:0"
LEAKY = 0.01


def bf(t):
    return t.bfloat16().float()


def _to_cl(x, cp):
    dst = O.alloc_cl(x.shape[0], x.shape[2:], cp, L.SP_BF16, DEV)
    O.ncdhw_to_cl(x.contiguous().to(DEV), dst, L.SP_BF16)
    return dst


def _from_cl(t, c):
    out = torch.empty((t.shape[0], c) + tuple(t.shape[1:4]), dtype=torch.float32, device=DEV)
    O.cl_to_ncdhw(t, out, L.SP_BF16)
    return out.cpu()


def _bn_args(sums, nrep, count, gamma, beta, rm, rv, training, c, cp, scale, shift, mean, invstd):
    f = L.BnFinArgs()
    f.sums, f.gamma, f.beta = O.ptr(sums), O.ptr(gamma), O.ptr(beta)
    f.running_mean, f.running_var = O.ptr(rm), O.ptr(rv)
    f.scale, f.shift, f.mean, f.invstd = O.ptr(scale), O.ptr(shift), O.ptr(mean), O.ptr(invstd)
    f.count, f.momentum, f.eps = float(count), 0.1, 1e-5
    f.nrep, f.training, f.C, f.CP = nrep, int(training), c, cp
    return f


@pytest.mark.parametrize("cin,cout,training", [(16, 16, True), (48, 16, True), (96, 32, True), (32, 32, False), (24, 24, True)])
def test_batchnorm_finalize_inside_the_weight_repack_kernel(cin, cout, training):
    g = torch.Generator().manual_seed(cin + cout)
    cpi, cpo = O.cpad(cin, 16), O.cpad(cout, 16)
    dims = (9, 20, 36)
    op = P.conv_fwd_op(cin, cout, 3, 1, 0, dims, cpi, cpo, L.SP_BF16)
    w = (torch.randn(cout, cin, 3, 3, 3, generator=g) / math.sqrt(27 * cin)).to(DEV)
    b = (torch.randn(cout, generator=g) * 0.1).to(DEV)
    gamma, beta = (torch.rand(cin, generator=g) + 0.5).to(DEV), (torch.randn(cin, generator=g) * 0.1).to(DEV)
    nrep, count = 64, 4321.0
    s1 = torch.randn(nrep, cpi, generator=g, dtype=torch.float64) * 30
    s2 = s1 ** 2 / count * nrep + torch.rand(nrep, cpi, generator=g, dtype=torch.float64) * 80      # positive variances
    sums = torch.stack((s1, s2), -1).contiguous().to(DEV)
    res = []
    for fused in (False, True):
        run = O.ConvRunner(op, DEV, zm_batch=2)
        assert run.can_fuse_bn()
        rm, rv = torch.linspace(-1, 1, cin, device=DEV), torch.linspace(0.5, 2, cin, device=DEV)
        scale, shift, mean, invstd = (torch.full((cpi,), 7.0, device=DEV) for _ in range(4))
        if fused:
            f = _bn_args(sums, nrep, count, gamma, beta, rm, rv, training, cin, cpi, scale, shift, mean, invstd)
            run.prep(w, b, scale, shift, bn=f)
        else:
            O.bn_finalize(sums, count, gamma, beta, rm, rv, 0.1, 1e-5, training, cin, cpi, scale, shift, mean, invstd, nrep=nrep)
            run.prep(w, b, scale, shift)
        torch.cuda.synchronize()
        z = run.zm if run.uses_zm() else run.subs[0]
        res.append((z["hi"].clone(), run.bias.clone(), scale, shift, mean, invstd, rm, rv))
    for a, bb in zip(*res):
        assert torch.equal(a, bb)
    assert float(res[1][2][:cin].abs().min()) > 0 and (cpi == cin or float(res[1][2][cin:].abs().max()) == 0)


@pytest.mark.parametrize("cout,hl", [(16, False), (32, False), (16, True)])
def test_first_layer_repack_with_the_batchnorm_finalize_inside(cout, hl):
    g = torch.Generator().manual_seed(cout)
    w = (torch.randn(cout, 2, 3, 3, 3, generator=g) / 7).to(DEV)
    b = (torch.randn(cout, generator=g) * 0.1).to(DEV)
    gamma, beta = (torch.rand(2, generator=g) + 0.5).to(DEV), (torch.randn(2, generator=g) * 0.1).to(DEV)
    nrep, count, cp = 64, 99999.0, 16
    s1 = torch.randn(nrep, cp, generator=g, dtype=torch.float64) * 30
    s2 = s1 ** 2 / count * nrep + torch.rand(nrep, cp, generator=g, dtype=torch.float64) * 80
    sums = torch.stack((s1, s2), -1).contiguous().to(DEV)
    res = []
    for fused in (False, True):
        rm, rv = torch.zeros(2, device=DEV), torch.ones(2, device=DEV)
        scale, shift, mean, invstd = (torch.full((cp,), 7.0, device=DEV) for _ in range(4))
        wf = torch.zeros((cout // 16) * 3 * 64 * 8, dtype=torch.bfloat16, device=DEV)
        wl = torch.zeros_like(wf) if hl else None
        bias_f = torch.zeros(cout, device=DEV)
        if fused:
            f = _bn_args(sums, nrep, count, gamma, beta, rm, rv, True, 2, cp, scale, shift, mean, invstd)
            L.call("sp_first_prep_bn", O.ptr(w), O.ptr(b), O.ptr(wf), O.ptr(wl), O.ptr(bias_f), cout, C.byref(f), O.stream())
        else:
            O.bn_finalize(sums, count, gamma, beta, rm, rv, 0.1, 1e-5, True, 2, cp, scale, shift, mean, invstd, nrep=nrep)
            if hl:
                L.call("sp_first_prep_hl", O.ptr(w), O.ptr(b), O.ptr(scale), O.ptr(shift), O.ptr(wf), O.ptr(wl), O.ptr(bias_f), cout, O.stream())
            else:
                L.call("sp_first_prep_n", O.ptr(w), O.ptr(b), O.ptr(scale), O.ptr(shift), O.ptr(wf), O.ptr(bias_f), cout, O.stream())
        torch.cuda.synchronize()
        res.append((wf, bias_f, scale, shift, mean, invstd, rm, rv) + ((wl,) if hl else ()))
    for a, bb in zip(*res):
        assert torch.equal(a, bb)


# cin (of the second convolution = channels of x / dz_out), cout, input dims of the second convolution, batch: the (P, NT) instances
# (1, 1) and (2, 2) of the headline network's blocks, (1, 2) / (2, 1), ragged planes, a flattened tile (52 x 52 -> 25 x 10)
DZ_CASES = [(16, 16, (9, 36, 40), 2), (32, 32, (7, 21, 37), 2), (32, 16, (6, 33, 18), 1), (16, 32, (5, 19, 50), 2), (32, 32, (4, 52, 52), 1)]


@pytest.mark.parametrize("cin,cout,dims,B", DZ_CASES)
def test_data_gradient_with_the_batchnorm_and_activation_backward_in_its_epilogue(cin, cout, dims, B, monkeypatch):
    monkeypatch.setattr(O, "ZM_MIN_PLANES", 0)
    g = torch.Generator().manual_seed(cin * 3 + cout + B)
    od = tuple(d - 2 for d in dims)
    x = bf(torch.randn(B, cin, *dims, generator=g))                       # the first convolution's output (LeakyReLU applied)
    dzu = bf(torch.randn(B, cout, *od, generator=g))                      # dz of the second convolution
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) / math.sqrt(27 * cin)
    gamma = (torch.rand(cin, generator=g) + 0.5).to(DEV)
    mean, invstd = (torch.randn(cin, generator=g) * 0.2).to(DEV), (torch.rand(cin, generator=g) + 0.7).to(DEV)
    dop = P.conv_dgrad_op(cin, cout, 3, 1, 0, dims, cout, cin, L.SP_BF16)
    run = O.ConvRunner(dop, DEV, zm_batch=B)
    assert run.zm_bn_bwd_ok()
    run.prep(w.to(DEV))
    xs, dzs = _to_cl(x, cin), _to_cl(dzu, cout)
    count = float(B * dims[0] * dims[1] * dims[2])
    nrep = 64
    # ---- the three-kernel path: g stored, (sum g, sum g x) from its epilogue, finalize, elementwise pass
    gbuf = O.alloc_cl(B, dims, cin, L.SP_BF16, DEV)
    bs = torch.zeros(nrep * cin * 2, dtype=torch.float64, device=DEV)
    run.run(dzs, gbuf, B, stats=bs, stats_nrep=nrep, stats_mode=1, aux=xs)
    dgam_a, dbet_a = torch.zeros(cin, device=DEV), torch.zeros(cin, device=DEV)
    coef = torch.zeros(3, cin, device=DEV)
    O.bn_bwd_finalize(bs, count, gamma, mean, invstd, cin, cin, dgam_a, dbet_a, coef, nrep=nrep)
    dz_a = torch.empty_like(gbuf)
    sums_a = torch.zeros(L.SP_REDUCE_ROWS, cin, dtype=torch.float64, device=DEV)
    O.bn_act_bwd(gbuf, xs, coef, L.SP_BF16, L.ACT_LEAKY, LEAKY, dz_a, sums_a)
    # ---- one kernel
    dz_b = torch.full_like(gbuf, 7.0)
    sums_b = torch.zeros(L.SP_REDUCE_ROWS, cin, dtype=torch.float64, device=DEV)
    dgam_b, dbet_b = torch.zeros(cin, device=DEV), torch.zeros(cin, device=DEV)
    coef_b = torch.zeros(3, cin, device=DEV)
    run.run(dzs, dz_b, B, None, None, L.ACT_LEAKY, LEAKY, None, stats_mode=2, aux=xs, dz_sums=sums_b,
            bnb=dict(sums=bs, nrep=nrep, count=count, gamma=gamma, mean=mean, invstd=invstd, C=cin, CP=cin, dgamma=dgam_b, dbeta=dbet_b, coef=coef_b))
    torch.cuda.synchronize()
    assert torch.equal(coef, coef_b) and torch.equal(dgam_a, dgam_b) and torch.equal(dbet_a, dbet_b)
    a, b_ = _from_cl(dz_a, cin), _from_cl(dz_b, cin)
    # the same arithmetic on the same rounded g up to the contraction of c0 g + c1 x + c2 into fmas: a last-bit difference at most
    scale = float(a.abs().max())
    assert float((a - b_).abs().max()) <= 2.0 ** -7 * scale and float((a != b_).float().mean()) < 0.02
    torch.testing.assert_close(sums_b.sum(0).cpu(), sums_a.sum(0).cpu(), rtol=1e-6, atol=1e-4 * math.sqrt(count))
    # ---- float64 reference of the whole chain from the stored g's definition
    gref = F.conv_transpose3d(dzu.double(), bf(w).double())
    cf = coef.double().cpu()
    ref = (cf[0].view(1, -1, 1, 1, 1) * bf(gref.float()).double() + cf[1].view(1, -1, 1, 1, 1) * x.double() + cf[2].view(1, -1, 1, 1, 1)) \
        * torch.where(x > 0, 1.0, LEAKY).double()
    torch.testing.assert_close(b_.double(), ref, rtol=2e-2, atol=2e-2 * float(ref.abs().max()))


# cin = cout, input dims, batch, bf16 pairs: (1, 1) and (2, 2) instances; odd output extents (floor pooling), pieces that start in
# the middle of a column
POOL_CASES = [(16, (10, 38, 40), 2, False), (32, (9, 23, 37), 2, False), (16, (7, 70, 21), 1, False), (32, (12, 36, 36), 1, False),
              (16, (9, 38, 24), 2, True), (32, (8, 22, 38), 1, True)]


@pytest.mark.parametrize("c,dims,B,hl", POOL_CASES)
def test_maxpool_in_the_convolution_epilogue(c, dims, B, hl, monkeypatch):
    monkeypatch.setattr(O, "ZM_MIN_PLANES", 0)
    g = torch.Generator().manual_seed(c + dims[1] + B)
    dt = L.SP_HL if hl else L.SP_BF16
    op = P.conv_fwd_op(c, c, 3, 1, 0, dims, c, c, dt)
    run = O.ConvRunner(op, DEV, zm_batch=B, zm_tile="classic")
    assert run.zm_pool_ok()
    w = (torch.randn(c, c, 3, 3, 3, generator=g) / math.sqrt(27 * c)).to(DEV)
    b = (torch.randn(c, generator=g) * 0.1).to(DEV)
    sc, sh = (torch.rand(c, generator=g) + 0.5).to(DEV), (torch.randn(c, generator=g) * 0.1).to(DEV)
    run.prep(w, b, sc, sh)
    x = torch.randn(B, c, *dims, generator=g)
    xs = _to_cl(bf(x), c)
    xl = _to_cl(bf(x - bf(x)), c) if hl else None
    od, pd = tuple(op.y_dims), tuple(d // 2 for d in op.y_dims)
    nrep = 64

    def outs():
        y = torch.full((2 if hl else 1, B) + od + (c,), 7.0, dtype=torch.bfloat16, device=DEV)
        p = torch.full((2 if hl else 1, B) + pd + (c,), 7.0, dtype=torch.bfloat16, device=DEV)
        return y, p, torch.zeros(nrep * c * 2, dtype=torch.float64, device=DEV)
    kw = dict(dtype_out=dt, stats_nrep=nrep)
    # ---- convolution, then the pooling kernel
    ya, pa, sa = outs()
    if hl:
        run.run(xs, ya[0], B, None, None, L.ACT_LEAKY, LEAKY, None, x_lo=xl, y_lo=ya[1], **kw)
        L.call("sp_maxpool2_fwd_hl", O.ptr(ya[0]), ya[1].data_ptr() - ya[0].data_ptr(), O.ptr(pa[0]), pa[1].data_ptr() - pa[0].data_ptr(), B, *od, c,
               O.ptr(sa), O.stream())
    else:
        run.run(xs, ya[0], B, None, None, L.ACT_LEAKY, LEAKY, None, **kw)
        O.maxpool2_fwd(ya[0], pa[0], L.SP_BF16, sa)
    # ---- one kernel
    yb, pb, sb = outs()
    if hl:
        run.run(xs, yb[0], B, None, None, L.ACT_LEAKY, LEAKY, sb, x_lo=xl, y_lo=yb[1], pool=(pb[0], pb[1]), **kw)
    else:
        run.run(xs, yb[0], B, None, None, L.ACT_LEAKY, LEAKY, sb, pool=(pb[0], None), **kw)
    torch.cuda.synchronize()
    assert torch.equal(ya, yb)
    if hl:      # the pair kernels pool hi + lo values; the epilogue pools the fp32 values the pairs were split from: equal to 2^-16
        va, vb = pa[0].float() + pa[1].float(), pb[0].float() + pb[1].float()
        assert float((va - vb).abs().max()) <= 2.0 ** -14 * float(va.abs().max())
    else:
        assert torch.equal(pa, pb)
    # SP_REDUCE_ROWS replica rows (the pooling kernel) against the convolution's stats_nrep rows
    ta = sa.view(-1)[:L.SP_REDUCE_ROWS * c * 2].view(L.SP_REDUCE_ROWS, c, 2).sum(0).cpu()
    tb = sb.view(nrep, c, 2).sum(0).cpu()
    n = pa[0].numel() / c
    torch.testing.assert_close(tb, ta, rtol=1e-5, atol=1e-3 * math.sqrt(n))


def test_data_gradient_of_a_concatenating_layer_as_two_dense_tensors(monkeypatch):
    """sp_conv3d_zm with y2 / split_nt: the 16 -> 48 data gradient (block 5's first convolution, Unet3D.py:71-72) writes its first 32
    channels (the upsampled half) and its last 16 (the skip half) into two dense tensors from one launch: bit-identical with the
    channel slices of the one-tensor form"""
    monkeypatch.setattr(O, "ZM_MIN_PLANES", 0)
    g = torch.Generator().manual_seed(9)
    cin, cout, dims, B = 48, 16, (7, 30, 37), 2
    dz = bf(torch.randn(B, cout, *(d - 2 for d in dims), generator=g))
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) / math.sqrt(27 * cin)
    dop = P.conv_dgrad_op(cin, cout, 3, 1, 0, dims, cout, cin, L.SP_BF16)
    run = O.ConvRunner(dop, DEV, zm_batch=B)
    assert run.zm_split_ok()
    run.prep(w.to(DEV))
    dzs = _to_cl(dz, cout)
    whole = torch.full((B,) + dims + (cin,), 7.0, dtype=torch.bfloat16, device=DEV)
    run.run(dzs, whole, B)
    a = torch.full((B,) + dims + (32,), 7.0, dtype=torch.bfloat16, device=DEV)
    b = torch.full((B,) + dims + (16,), 7.0, dtype=torch.bfloat16, device=DEV)
    run.run(dzs, a, B, y2=b, split_nt=2)
    torch.cuda.synchronize()
    assert torch.equal(a, whole[..., :32]) and torch.equal(b, whole[..., 32:])
    torch.testing.assert_close(_from_cl(whole, cin), F.conv_transpose3d(dz, bf(w)), rtol=3e-2, atol=3e-2)


def _train_steps(dtype, fuse, monkeypatch, steps=3, dims=(52, 52, 52)):
    import stroke_prediction_amd  # noqa: F401
    from oracle import weights as W
    from stroke_prediction_amd.common.model.Unet3D import Unet3D
    import stroke_prediction_amd.common.dto.UnetDto as UnetDtoUtil
    from stroke_prediction_amd.common.metrics import BatchDiceLoss
    from stroke_prediction_amd.optim import FusedAdam
    monkeypatch.setattr(O, "FUSE_BN_FINALIZE", fuse)
    monkeypatch.setattr(O, "FUSE_DZ", fuse)
    monkeypatch.setattr(O, "FUSE_POOL", fuse)
    monkeypatch.setattr(O, "SPLIT_G", fuse)
    ch = [2, 16, 32, 64, 32, 16, 32, 2]
    x, y = W.unet_inputs(2, dims, 11)
    model = Unet3D(ch, dtype=dtype)
    model.load_state_dict(W.make_state_dict(W.unet_spec(ch), 11))
    model = model.to(DEV).train()
    opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=1e-5, betas=(0.99, 0.999))
    crit = BatchDiceLoss([1.0])
    xd, yd = x.to(DEV), y.to(DEV)
    losses, g0 = [], None
    for _ in range(steps):
        dto = model(UnetDtoUtil.init_dto(xd, yd[:, 0:1], yd[:, 1:2]))
        loss = (crit(dto.outputs.core, dto.given_variables.core) + crit(dto.outputs.penu, dto.given_variables.penu)) / 2
        opt.zero_grad()
        loss.backward()
        if g0 is None:
            g0 = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
        opt.step()
        losses.append(float(loss))
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return losses, g0, sd


@pytest.mark.parametrize("dtype", ["bf16", "bf16x3"])
def test_training_steps_with_and_without_the_folded_launches(dtype, monkeypatch):
    """three Adam steps of the 3-scale U-Net: BatchNorm finalize inside the re-pack kernels (bit-identical by construction), pooling
    in the convolution epilogue (same tensors, statistics summed in another order) and the dz epilogue of the second convolutions'
    data gradients (last-bit differences of dz) against the un-fused launches"""
    la, ga, sa = _train_steps(dtype, False, monkeypatch)
    lb, gb, sb = _train_steps(dtype, True, monkeypatch)
    assert abs(la[0] - lb[0]) < (2e-6 if dtype == "bf16x3" else 2e-4)      # (the pooled statistics are summed in another order)
    for a, b in zip(la, lb):
        assert abs(a - b) < 2e-3, (la, lb)
    for k in ga:
        den = float(ga[k].norm()) + 1e-12
        assert float((ga[k] - gb[k]).norm()) / den < 2e-2, (k, float((ga[k] - gb[k]).norm()) / den)
    for k in sa:
        if "running" in k or "num_batches" in k:
            torch.testing.assert_close(sa[k].float(), sb[k].float(), rtol=1e-3, atol=1e-4)


# ------------------------------------------------------------------------------------------------ the headline size, backward included
GOLDEN = __import__("os").path.join(__import__("os").path.dirname(__import__("os").path.abspath(__file__)), "golden")


def grad_sample_index(numel, n=64):
    """tests/golden/make_golden.py:grad_sample_index"""
    import numpy as np
    return np.unique(np.linspace(0, numel - 1, num=min(n, numel)).round().astype(np.int64))


# mode -> bounds on: |loss - ref|; the worst per-tensor |norm / ref norm - 1|; per tensor, the rms error of the 64-element sample in
# units of the tensor's rms gradient -- worst and median over the 44 tensors; the cosine of all samples (each tensor scaled to unit
# rms).  Measured on MI355X (profiles/r05_trainstep128_parity.txt), bounds at 1.5-2 x the measurement:
#   f32     loss 1e-7   norm 3.7e-2   worst 3.9e-2   median 7.8e-3   cosine 0.99997
#   f16x3        <1e-7       1.2e-2         4.5e-2          6.4e-3          0.99990
#   bf16x3       1e-7        2.4e-1         3.3e-1          2.2e-2          0.99893
#   f16          1.1e-5      1.8e-1         1.8e-1          6.2e-2          0.99704
#   bf16         1.6e-5      1.9e-1         4.1e-1          1.8e-1          0.97731
# The f32 mode's gradient error is LeakyReLU(0.01) branch flips of near-zero pre-activations under another fp32 summation order
# (the pair mode f16x3, whose forward is as exact, lands at the same place); the worst tensors of every mode are the first
# BatchNorm's gamma / beta, whose gradients are cancelling sums.
TRAINSTEP_BOUNDS = {
    "f32":    dict(loss=2e-5, norm=6e-2, worst=8e-2, median=1.5e-2, cos=0.9999),
    "f16x3":  dict(loss=2e-5, norm=4e-2, worst=1e-1, median=1.5e-2, cos=0.9995),
    "bf16x3": dict(loss=2e-5, norm=4e-1, worst=5e-1, median=5e-2, cos=0.997),
    "f16":    dict(loss=1e-4, norm=3e-1, worst=3e-1, median=1e-1, cos=0.99),
    "bf16":   dict(loss=1e-4, norm=3e-1, worst=6e-1, median=2.7e-1, cos=0.96),
}


@pytest.mark.parametrize("dtype", ["f32", "f16x3", "bf16x3", "f16", "bf16"])
def test_unet_trainstep128_fixture_through_the_hip_path(dtype):
    """one training step at 2 x 2 x 128^3 against what the REFERENCE recorded (tests/golden/unet_trainstep128.npz: loss, gradient norms,
    heads and samples, BatchNorm buffers and parameter norms after Adam): every precision mode with a bound of its own"""
    import numpy as np
    import stroke_prediction_amd  # noqa: F401
    from oracle import weights as W
    from stroke_prediction_amd.common.model.Unet3D import Unet3D
    import stroke_prediction_amd.common.dto.UnetDto as UnetDtoUtil
    from stroke_prediction_amd.common.metrics import BatchDiceLoss
    from stroke_prediction_amd.optim import FusedAdam
    fx = np.load(__import__("os").path.join(GOLDEN, "unet_trainstep128.npz"))
    bd = TRAINSTEP_BOUNDS[dtype]
    seed, B = int(fx["seed"]), int(fx["batch"])
    ch = [2, 16, 32, 64, 32, 16, 32, 2]
    sd = W.make_state_dict(W.unet_spec(ch), seed)
    for k, gain in zip(fx["head_gain_keys"], fx["head_gain"]):
        sd[str(k)] = sd[str(k)] * float(gain)
    model = Unet3D(ch, dtype=dtype)
    model.load_state_dict(sd)
    model = model.to(DEV).train()
    opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=1e-5, betas=(0.99, 0.999))
    crit = BatchDiceLoss([1.0])
    x, y = W.unet_inputs(B, 128, seed)
    xd, yd = x.to(DEV), y.to(DEV)
    dto = model(UnetDtoUtil.init_dto(xd, yd[:, 0:1], yd[:, 1:2]))
    loss = (crit(dto.outputs.core, dto.given_variables.core) + crit(dto.outputs.penu, dto.given_variables.penu)) / 2
    opt.zero_grad()
    loss.backward()
    lv = float(loss.detach())
    assert abs(lv - float(fx["loss"])) < bd["loss"], (lv, float(fx["loss"]))
    errs, dots, na, nb, worst_norm = [], 0.0, 0.0, 0.0, 0.0
    for k, p in model.named_parameters():
        g = p.grad.detach().reshape(-1).double().cpu()
        gn = float(fx["gnorm/" + k])
        worst_norm = max(worst_norm, abs(float(g.norm()) / gn - 1.0))
        ref = torch.from_numpy(fx["gsample/" + k]).double()
        got = g[torch.from_numpy(grad_sample_index(g.numel()))]
        rms = gn / math.sqrt(g.numel())
        errs.append(float((got - ref).norm()) / math.sqrt(len(ref)) / rms)
        dots += float(got @ ref) / rms ** 2; na += float(got @ got) / rms ** 2; nb += float(ref @ ref) / rms ** 2
    errs.sort()
    cos = dots / math.sqrt(na * nb)
    print("trainstep128 %s: loss %.7f (ref %.7f), norm ratio worst %.2e, sample error / rms worst %.2e median %.2e, cosine %.5f"
          % (dtype, lv, float(fx["loss"]), worst_norm, errs[-1], errs[len(errs) // 2], cos))
    assert worst_norm < bd["norm"] and errs[-1] < bd["worst"] and errs[len(errs) // 2] < bd["median"] and cos > bd["cos"]
    opt.step()
    tol = 1e-5 if dtype in ("f32", "f16x3", "bf16x3") else 2e-2
    for k, b in model.named_buffers():
        if k.endswith("running_mean") or k.endswith("running_var"):
            np.testing.assert_allclose(b.detach().cpu().numpy(), fx["buf1/" + k], rtol=max(tol, 2e-5), atol=tol, err_msg=k)
    for k, p in model.named_parameters():
        ref = float(fx["pnorm1/" + k])      # (Adam moves every element by ~lr: elements whose gradient sign differs move the other way)
        assert abs(float(p.detach().double().norm()) - ref) <= 2e-3 * ref + 1e-3 * math.sqrt(p.numel()), k


# ------------------------------------------------------------------------------------------------ drop-in defaults (VERDICT r4 "next" 9)
def test_default_learner_samples_the_surface_distances_and_holds_them(tmp_path, monkeypatch):
    """Learner defaults: every training batch reports the on-device confusion measures, Hausdorff / ASSD are measured on batch 0, k,
    2k, ... and held in between (distance_metrics_every; 1 = the reference's every-batch behaviour, Learner.py:124)"""
    import stroke_prediction_amd  # noqa: F401
    from oracle import weights as W
    from stroke_prediction_amd.common import metrics
    from stroke_prediction_amd.common.model.Unet3D import Unet3D
    from stroke_prediction_amd.learner.UnetSegmentationLearner import UnetSegmentationLearner
    from stroke_prediction_amd.optim import FusedAdam, attach_flat_grads
    import common.metrics as cm                      # (the module object the learner toggles)
    calls = {"n": 0}
    orig = cm._surface_distances_launch

    def counting(*a, **k):
        calls["n"] += 1
        return orig(*a, **k)
    monkeypatch.setattr(cm, "_surface_distances_launch", counting)

    class Loader(list):
        batch_size = 2
    ch = [2, 16, 32, 64, 32, 16, 32, 2]
    x, y = W.unet_inputs(2, (52, 52, 52), 11)
    batch = {"case_id": [0, 1], "images": x.to(DEV), "labels": y.to(DEV), "clinical": torch.zeros(2, 5, 1, 1, 1)}
    for every, steps, expect in ((16, 5, 2), (2, 5, 6), (1, 3, 6), (0, 3, 0)):
        calls["n"] = 0
        model = Unet3D(ch, dtype="bf16")
        model.load_state_dict(W.make_state_dict(W.unet_spec(ch), 11))
        model = model.to(DEV).train()
        opt = FusedAdam(model.parameters(), lr=1e-3, capturable=True)
        attach_flat_grads(model)
        kw = {} if every == 16 else {"distance_metrics_every": every}       # 16 is the default
        learner = UnetSegmentationLearner(Loader([batch]), None, model, opt, None, 1, metrics.BatchDiceLoss([1.0]), None, str(tmp_path / ("m%d" % every)), **kw)
        out = [learner.train_batch(batch, 0) for _ in range(steps)]
        assert calls["n"] == expect, (every, calls["n"])      # two classes per measured batch
        for m in out:
            assert 0.0 <= m.core.dc <= 1.0 and 0.0 <= m.penu.sensitivity <= 1.0
        if every:
            assert all(math.isfinite(m.core.hd) and math.isfinite(m.penu.assd) for m in out)
        if every == 16:
            assert out[1].core.hd == out[0].core.hd and out[4].penu.assd == out[0].penu.assd      # held between samples
        if every == 0:
            assert all(math.isinf(m.core.hd) for m in out)


def test_engine_cache_evicts_the_least_recently_used_shape_only():
    """Unet3D keeps at most ENGINE_CACHE engines (one per input shape): a fifth shape evicts the least recently used one, the
    others -- and graphs captured over their buffers -- stay (the whole cache used to be cleared)"""
    import stroke_prediction_amd  # noqa: F401
    from stroke_prediction_amd.common.model.Unet3D import Unet3D
    import stroke_prediction_amd.common.dto.UnetDto as UnetDtoUtil
    model = Unet3D([2, 16, 32, 64, 32, 16, 32, 2], dtype="bf16").to(DEV).eval()
    sizes = [(44, 44, 44), (44, 44, 48), (44, 48, 44), (48, 44, 44)]
    eng = {}
    with torch.no_grad():
        for s in sizes:
            model(UnetDtoUtil.init_dto(torch.randn(1, 2, *s, device=DEV), None, None))
            eng[s] = next(reversed(model._engines.values()))
        assert len(model._engines) == 4
        model(UnetDtoUtil.init_dto(torch.randn(1, 2, *sizes[0], device=DEV), None, None))       # touch the oldest: now most recent
        model(UnetDtoUtil.init_dto(torch.randn(1, 2, 48, 48, 48, device=DEV), None, None))       # a fifth shape
    live = list(model._engines.values())
    assert len(live) == 4 and eng[sizes[0]] in live and eng[sizes[2]] in live and eng[sizes[3]] in live and eng[sizes[1]] not in live


# ------------------------------------------------------------------------------------------------ header-only C entry points, CAE layer kinds
@pytest.mark.parametrize("kind,cin,cout,pad", [("conv", 16, 16, (1, 0, 0)), ("conv", 32, 32, (1, 2, 2)), ("grad", 32, 32, (1, 2, 2)),
                                                  ("conv", 16, 32, (1, 1, 1)), ("convT", 32, 16, (0, 0, 0)), ("convT", 16, 16, (1, 1, 1))])
def test_header_only_padded_and_transposed_layers(kind, cin, cout, pad):
    """VERDICT r4 "next" 10: include/stroke_amd.h alone (sp_conv3d_plan with padD / padH / padW / transposed, _init, _set_weights,
    _run -- no runtime/plan.py) for the CAE's layer kinds on the z-marching kernel: a padded stride-1 3x3x3 convolution with bias and
    ELU (Cae3D.py:41-44,186-212), its data gradient, and a stride-1 ConvTranspose3d with bias and ELU (Cae3D.py:178-180 in kind)"""
    lib = L.load()
    B, dims = 2, (7, 20, 37)
    g = torch.Generator().manual_seed(cin * 3 + cout + sum(pad))
    d = L.Conv3dDesc(B, cin, cout, *dims, 1 if kind == "grad" else 0, *pad, 1 if kind == "convT" else 0)
    pl = L.Conv3dPlan()
    assert lib.sp_conv3d_plan(C.byref(d), C.byref(pl)) == 0, L.last_error()
    ws = torch.empty(pl.workspace_bytes, dtype=torch.uint8, device=DEV)
    st = O.stream()
    assert lib.sp_conv3d_init(C.byref(d), C.byref(pl), ws.data_ptr(), st) == 0, L.last_error()
    b = torch.randn(cout, generator=g) * 0.1
    if kind == "convT":
        w = torch.randn(cin, cout, 3, 3, 3, generator=g) / math.sqrt(27 * cin)
        x = bf(torch.randn(B, cin, *dims, generator=g))
        ref = F.elu(F.conv_transpose3d(x, bf(w), b, padding=pad), 1.0)
    elif kind == "conv":
        w = torch.randn(cout, cin, 3, 3, 3, generator=g) / math.sqrt(27 * cin)
        x = bf(torch.randn(B, cin, *dims, generator=g))
        ref = F.elu(F.conv3d(x, bf(w), b, padding=pad), 1.0)
    else:
        w = torch.randn(cout, cin, 3, 3, 3, generator=g) / math.sqrt(27 * cin)
        x = bf(torch.randn(B, cout, *(dims[a] + 2 * pad[a] - 2 for a in range(3)), generator=g))      # dz on the conv's output grid
        ref = F.conv_transpose3d(x, bf(w), padding=pad)
    assert tuple(ref.shape[2:]) == (pl.Do, pl.Ho, pl.Wo) and tuple(x.shape[2:]) == (pl.Di, pl.Hi, pl.Wi)
    xin = _to_cl(x, pl.cin_op)
    assert lib.sp_conv3d_set_weights(C.byref(d), C.byref(pl), ws.data_ptr(), w.to(DEV).data_ptr(), None if kind == "grad" else b.to(DEV).data_ptr(),
                                     None, None, st) == 0, L.last_error()
    y = torch.full((B, pl.Do, pl.Ho, pl.Wo, pl.cout_op), 7.0, dtype=torch.bfloat16, device=DEV)
    rc = lib.sp_conv3d_run(C.byref(d), C.byref(pl), ws.data_ptr(), xin.data_ptr(), y.data_ptr(), 0 if kind == "grad" else 1,
                           L.ACT_NONE if kind == "grad" else L.ACT_ELU, 1.0, None, 1, 0, st)
    assert rc == 0, L.last_error()
    torch.testing.assert_close(_from_cl(y, pl.cout_op), ref, rtol=3e-2, atol=3e-2)
    # a BatchNorm in front of a padded layer cannot be folded into the weights: refused with a message
    if kind == "conv" and sum(pad):
        s1 = torch.ones(cin, device=DEV)
        assert lib.sp_conv3d_set_weights(C.byref(d), C.byref(pl), ws.data_ptr(), w.to(DEV).data_ptr(), None, s1.data_ptr(), s1.data_ptr(), st) != 0
        assert "BatchNorm" in L.last_error()


# ------------------------------------------------------------------------------------------------ plane-serial z-march
# cin, cout, input dims, batch, bf16 pairs, plane-major input: 96 -> 32 and 48 -> 16 (the two layers behind a concatenation), a
# two-plane case, ragged planes, volumes small enough that pieces start in the middle of a column
PS_CASES = [(48, 16, (7, 37, 21), 2, False, True), (96, 32, (6, 19, 33), 2, False, True), (48, 16, (5, 30, 30), 1, False, False),
            (96, 32, (9, 20, 40), 1, False, False), (32, 16, (9, 35, 17), 1, False, False), (48, 16, (7, 37, 21), 2, True, True),
            (32, 16, (6, 20, 40), 1, True, False), (96, 32, (6, 19, 33), 2, True, True), (96, 32, (5, 20, 24), 1, True, False)]


@pytest.mark.parametrize("cin,cout,dims,B,hl,planar", PS_CASES)
def test_plane_serial_march_matches_conv3d(cin, cout, dims, B, hl, planar, monkeypatch):
    """sp_conv3d_zm with pser_planes (round 5): one 16-channel plane per sub-step, that plane's weight fragments streamed through two
    LDS buffers -- bias, LeakyReLU and statistics against float64 torch on the operands the kernel sees, for bf16 and bf16-pair
    operands, plane-major (concat buffers) and channels-last inputs"""
    monkeypatch.setattr(O, "ZM_MIN_PLANES", 0)
    monkeypatch.setattr(P, "ZM_PSER_ALL", True)
    monkeypatch.setattr(O, "HL_PSER_SLICES", True)
    g = torch.Generator().manual_seed(cin * 7 + cout + B)
    dt = L.SP_HL if hl else L.SP_BF16
    op = P.conv_fwd_op(cin, cout, 3, 1, 0, dims, cin, cout, dt)
    run = O.ConvRunner(op, DEV, zm_batch=B)
    if hl and cout > 16:      # pairs: one plane-serial launch per 16 output channels (plan.zm_pser_slices)
        assert run.zm is None and len(run.zms) == cout // 16 and all(z.get("pser") and z["PT"] == cin // 16 for z in run.zms)
    else:
        assert run.zm is not None and run.zm.get("pser") and run.zm["PT"] == cin // 16
    x = torch.randn(B, cin, *dims, generator=g)
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) / math.sqrt(27 * cin)
    b = torch.randn(cout, generator=g) * 0.1
    sc, sh = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.1
    run.prep(w.to(DEV), b.to(DEV), sc.to(DEV), sh.to(DEV))

    def lay(t):      # channels-last (B, D, H, W, C) tensor, or its plane-major form in the same shape
        t = _to_cl(t, cin)
        return t.view(B, *dims, cin // 16, 16).permute(4, 0, 1, 2, 3, 5).contiguous().view(B, *dims, cin) if planar else t
    xh = bf(x)
    xs = lay(xh)
    xl = lay(bf(x - xh)) if hl else None
    nrep = 64
    od = tuple(op.y_dims)
    y = torch.full((2 if hl else 1, B) + od + (cout,), 7.0, dtype=torch.bfloat16, device=DEV)
    st = torch.zeros(nrep * cout * 2, dtype=torch.float64, device=DEV)
    kw = dict(x_lo=xl, y_lo=y[1]) if hl else {}
    run.run(xs, y[0], B, None, None, L.ACT_LEAKY, LEAKY, st, dtype_out=dt, stats_nrep=nrep, x_planar=planar, **kw)
    torch.cuda.synchronize()
    xv = (xh + bf(x - xh)) if hl else xh
    wf = w * sc.view(1, -1, 1, 1, 1)
    ref = F.leaky_relu(F.conv3d(xv.double(), wf.double()) + (b + (w * sh.view(1, -1, 1, 1, 1)).sum((1, 2, 3, 4))).double().view(1, -1, 1, 1, 1), LEAKY)
    got = _from_cl(y[0], cout).double() + (_from_cl(y[1], cout).double() if hl else 0)
    tol = 2e-4 if hl else 3e-2
    torch.testing.assert_close(got, ref, rtol=tol, atol=tol * float(ref.abs().max()))
    s = st.view(nrep, cout, 2).sum(0).cpu()
    n = got.numel() / cout
    torch.testing.assert_close(s[:, 0], got.sum(dim=(0, 2, 3, 4)), rtol=1e-3, atol=4e-3 * math.sqrt(n))
    torch.testing.assert_close(s[:, 1], (got ** 2).sum(dim=(0, 2, 3, 4)), rtol=1e-3, atol=4e-3 * math.sqrt(n))


def test_dice_accumulator_clears_itself_between_calls():
    """common/metrics.py keeps ONE accumulator of the Dice sums per (device, channels, stream); sp_dice_finalize_clear zeroes it after
    reading (no fill launch per call).  Three calls in a row, a call after a simulated failure between the two launches, and the
    gradient all agree with the formula of metrics.py:16-28."""
    from common import metrics as M
    torch.manual_seed(5)
    loss_fn = M.BatchDiceLoss([0.4, 0.6])

    def ref(o, t, w=(0.4, 0.6), eps=1e-7):
        num = 2 * (o.double() * t.double()).sum(dim=(0, 2, 3, 4)) + eps
        den = (o.double() ** 2).sum(dim=(0, 2, 3, 4)) + (t.double() ** 2).sum(dim=(0, 2, 3, 4)) + eps
        return 1 - (torch.tensor(w, dtype=torch.float64, device=o.device) * num / den).sum()

    for k in range(3):
        o = torch.rand(2, 2, 9, 10, 11, device=DEV, requires_grad=True)
        t = (torch.rand(2, 2, 9, 10, 11, device=DEV) > 0.5).float()
        loss = loss_fn(o, t)
        assert abs(float(loss) - float(ref(o.detach(), t))) < 2e-6, (k, float(loss))
        loss.backward()
        o2 = o.detach().double().requires_grad_(True)
        ref(o2, t).backward()
        assert torch.allclose(o.grad.double(), o2.grad, rtol=1e-4, atol=1e-9)
    ents = [e for k, e in M._CRIT_SUMS.items() if k[0] == "dice"]
    assert ents and all(float(e[0].abs().sum()) == 0.0 and not e[1] for e in ents)      # left clean
    for e in ents:                                      # a call that died after sp_dice_sums: sums behind, flag up
        e[0].fill_(3.0)
        e[1] = True
    o = torch.rand(2, 2, 9, 10, 11, device=DEV)
    t = (torch.rand(2, 2, 9, 10, 11, device=DEV) > 0.5).float()
    assert abs(float(loss_fn(o, t)) - float(ref(o, t))) < 2e-6
