"""The BCE and Dice + BCE training criteria on the device: the ``sp_vloss_*`` kernels, ``metrics.BCELoss`` / ``DiceBCELoss``, the two
fused routes (``mean_of_channel_losses``, ``cae_reconstruction_loss``), a captured training step and the exact data-parallel mode.

The oracle is ``torch.nn.BCELoss`` and the literal ``BatchDiceLoss`` formula (reference metrics.py:16-28) on the CPU in fp64, fed the
fp32-rounded inputs, with autograd for the gradients.  Outputs are uniform in (0, 1) with planted saturated values -- exact 0, exact 1,
1e-30 and 1 - 2^-24, each against a target of 0 and of 1 -- and binary targets.

Bounds.  The kernels add at most 8 non-negative fp32 terms per thread, then 64 lanes, then 4 waves, then fp64: the sums stay within
about 1e-6 relative of the fp64 oracle (``logf`` included), and rtol 1e-5 leaves tenfold headroom -- the bound
``test_dice_and_output_grad`` holds the same reduction to.  Loss rtol 1e-5; coefficients and gradients rtol 1e-5, atol 1e-9.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
EPS = 1e-7
SHAPES = [(2, 2, 5, 7, 9),        # 315 voxels: one block, a tail, element loads (315 % 4 != 0)
          (2, 3, 1, 61, 101),     # 6161 voxels: four blocks in x, several replica rows, odd length
          (2, 2, 4, 16, 32)]      # 2048 voxels: aligned -> 16-byte loads
PLANTED = [0.0, 1.0, 1e-30, 1.0 - 2.0 ** -24]
GRAD_TOL = dict(rtol=1e-5, atol=1e-9)


@functools.lru_cache(maxsize=None)
def inputs(shape, seed=3):
    """(o, t) fp32 on the host: o uniform with the planted values at the head of every channel row of sample 0, t binary"""
    g = torch.Generator().manual_seed(seed + sum(shape))
    o = torch.rand(*shape, generator=g)
    t = (torch.rand(*shape, generator=g) > 0.7).float()
    for c in range(shape[1]):
        orow, trow = o[0, c].view(-1), t[0, c].view(-1)
        for k, v in enumerate(PLANTED):
            orow[2 * k] = orow[2 * k + 1] = v
            trow[2 * k], trow[2 * k + 1] = 0.0, 1.0
    assert float(o[0, 0].view(-1)[6]) < 1.0          # 1 - 2^-24 is an fp32 number
    return o, t


def oracle(o, t, w_dice, w_bce, upstream=1.0):
    """fp64 on the CPU: per-channel sums (C, 4), loss, coefficients (C, 3) and the gradient of upstream * loss"""
    o64, t64 = o.double().requires_grad_(True), t.double()
    C = o.shape[1]
    dims = [d for d in range(o.dim()) if d != 1]
    I, O_, T = (o64 * t64).sum(dims), (o64 * o64).sum(dims), (t64 * t64).sum(dims)
    S = torch.stack([torch.nn.BCELoss(reduction="sum")(o64[:, c], t64[:, c]) for c in range(C)])
    count = o.numel() // C
    loss = torch.zeros((), dtype=torch.float64)
    coef = torch.zeros(C, 3, dtype=torch.float64)
    if w_dice is not None:
        wd = torch.tensor(w_dice, dtype=torch.float64)
        num, den = 2 * I + EPS, O_ + T + EPS
        loss = loss + 1 - (wd * num / den).sum()
        coef[:, 0], coef[:, 1] = (-2 * wd / den).detach(), (2 * wd * num / den ** 2).detach()
    if w_bce is not None:
        wb = torch.tensor(w_bce, dtype=torch.float64)
        loss = loss + sum(wb[c] * torch.nn.BCELoss()(o64[:, c], t64[:, c]) for c in range(C))
        coef[:, 2] = wb / count
    grad, = torch.autograd.grad(loss * upstream, o64)
    return torch.stack([I, O_, T, S], 1).detach(), float(loss.detach()), coef, grad


def run_vloss(od, td, C, terms, w_dice, w_bce, upstream):
    """the three entry points on (B, C, ...) device tensors (views are read in place) -> sums (C, 4), cleared rows, loss, coef, grad"""
    from stroke_prediction_amd.runtime import lib as L, ops as O
    B = od.shape[0]
    dhw = od[0, 0].numel()
    pitch = L.SP_VLOSS_PITCH(C)
    sums = torch.zeros(L.SP_REDUCE_ROWS, pitch, dtype=torch.float64, device=DEV)
    L.call("sp_vloss_sums", O.ptr(od), od.stride(0), O.ptr(td), td.stride(0), B, C, dhw, terms, O.ptr(sums), O.stream())
    got = sums.sum(0)[:4 * C].view(C, 4).cpu()
    wd = None if w_dice is None else torch.tensor(w_dice, dtype=torch.float32, device=DEV)
    wb = None if w_bce is None else torch.tensor(w_bce, dtype=torch.float32, device=DEV)
    loss, coef = torch.empty((), device=DEV), torch.empty(3 * C, device=DEV)
    L.call("sp_vloss_finalize_clear", O.ptr(sums), None if wd is None else O.ptr(wd), None if wb is None else O.ptr(wb), EPS,
           float(B * dhw), C, O.ptr(loss), O.ptr(coef), O.stream())
    d = torch.full((B, C) + tuple(od.shape[2:]), float("nan"), device=DEV)
    up = torch.tensor(upstream, dtype=torch.float32, device=DEV)
    L.call("sp_vloss_bwd", O.ptr(od), od.stride(0), O.ptr(td), td.stride(0), O.ptr(coef), O.ptr(up), B, C, dhw, O.ptr(d), O.stream())
    return got, sums.cpu(), float(loss), coef.cpu().view(C, 3), d.cpu()


def log_calls(monkeypatch):
    """the call log of the launch-count tests: the name of every entry point called through the binding from here on"""
    from stroke_prediction_amd.runtime import lib as L
    calls, real_call = [], L.call

    def logging_call(name, *args):
        calls.append(name)
        return real_call(name, *args)
    monkeypatch.setattr(L, "call", logging_call)
    return calls


def check_vloss(o, t, od, td, terms):
    C = o.shape[1]
    w_dice = [0.3, 0.7, 0.4][:C] if terms & 1 else None
    w_bce = [0.6, 0.25, 0.15][:C] if terms & 2 else None
    got, cleared, loss, coef, d = run_vloss(od, td, C, terms, w_dice, w_bce, 0.5)
    ref_sums, ref_loss, ref_coef, ref_grad = oracle(o, t, w_dice, w_bce, 0.5)
    print("terms", terms, "sums rel err", ((got - ref_sums).abs() / ref_sums.abs().clamp_min(1e-300)).max().item(), "loss", loss, ref_loss)
    if terms & 1:
        torch.testing.assert_close(got[:, :3], ref_sums[:, :3], rtol=1e-5, atol=0)
    else:
        assert torch.count_nonzero(got[:, :3]) == 0          # moments not asked for are not computed
    if terms & 2:
        torch.testing.assert_close(got[:, 3], ref_sums[:, 3], rtol=1e-5, atol=0)
    else:
        assert torch.count_nonzero(got[:, 3]) == 0
    assert torch.count_nonzero(cleared) == 0, "finalize_clear must leave the accumulator zero"
    assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss), (loss, ref_loss)
    torch.testing.assert_close(coef.double(), ref_coef, **GRAD_TOL)
    assert bool(torch.isfinite(d).all())
    torch.testing.assert_close(d.double(), ref_grad, **GRAD_TOL)


@pytest.mark.parametrize("terms", [1, 2, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_vloss_kernels_against_the_oracle(shape, terms):
    o, t = inputs(shape)
    od, td = o.to(DEV), t.to(DEV)
    check_vloss(o, t, od, td, terms)
    if shape == SHAPES[0]:
        # the channel slice [:, 1:2] read in place: batch stride = both channels, base 4-byte aligned only -> element loads
        assert od[:, 1:2].data_ptr() % 16 != 0
        check_vloss(o[:, 1:2], t[:, 1:2], od[:, 1:2], td[:, 1:2], terms)
    if shape == SHAPES[2]:
        # a length that takes 16-byte loads on a base that does not: one element into an allocation
        buf = torch.empty(o.numel() + 4, device=DEV)
        shifted = buf[1:1 + o.numel()].view(shape).copy_(od)
        assert shifted.data_ptr() % 16 == 4
        check_vloss(o, t, shifted, td, terms)


# (name, shape, view): dense aligned -> 16-byte loads on 48 of a workgroup's lanes; dense, 105 voxels -> element loads, lanes without a
# trip; channels 1..2 of a three-channel tensor that starts one float into its allocation -> a length that would take 16-byte loads on
# row bases that do not (batch stride 3 * 192)
FALLBACK_CASES = [("aligned", (2, 2, 4, 6, 8), False), ("unaligned", (2, 2, 3, 5, 7), False), ("view", (2, 3, 4, 6, 8), True)]


def _fallback_operands(host, view):
    """the device copy of ``host`` the case asks for, and the host tensor the oracle is fed"""
    if not view:
        return host.to(DEV), host
    buf = torch.empty(host.numel() + 4, device=DEV)
    dev = buf[1:1 + host.numel()].view(host.shape).copy_(host.to(DEV))[:, 1:3]
    assert dev.data_ptr() % 16 == 4 and dev[0, 0].numel() % 4 == 0 and dev.stride(0) == 3 * dev[0, 0].numel()
    return dev, host[:, 1:3]


@pytest.mark.parametrize("kind", ["dice", "bce", "dicebce", "boundary", "diceboundary"])
@pytest.mark.parametrize("case", FALLBACK_CASES, ids=[c[0] for c in FALLBACK_CASES])
def test_merged_kernels_choose_the_load_width(case, kind):
    """every instance of the one sums and the one backward template (fourth column absent, BCE, o * phi; with and without Dice) on
    both load widths and on a strided view, against the fp64 oracles and at the tolerances of test_vloss_kernels_against_the_oracle
    and test_bloss_kernels_against_the_oracle.  Those two cover dense aligned and dense odd lengths of several workgroups and a channel
    slice of an odd length; none of them has a workgroup with idle lanes on 16-byte loads or a view whose length is a multiple of four
    on misaligned rows, so no combination is left out here."""
    import test_gpu_boundary as TB
    _, shape, view = case
    if kind in ("boundary", "diceboundary"):
        o, t, phi = TB.loss_inputs(shape)
        (od, oh), (td, th) = _fallback_operands(o, view), _fallback_operands(t, view)
        ph = phi[:, 1:3] if view else phi
        assert 0 < float(th.sum()) < th.numel()
        TB.check_bloss(oh, th, ph, od, td, ph.contiguous().to(DEV), kind)      # phi is dense in every case
    else:
        o, t = inputs(shape)
        (od, oh), (td, th) = _fallback_operands(o, view), _fallback_operands(t, view)
        check_vloss(oh, th, od, td, {"dice": 1, "bce": 2, "dicebce": 3}[kind])


# (B, (D, H, W), latent elements): 210 voxels = one partial workgroup and no latent row; 14760 voxels = eight workgroups along x
CAE_CASES = [(2, (5, 6, 7), 0), (2, (9, 40, 41), 37)]


@functools.lru_cache(maxsize=None)
def cae_inputs(B, dims, nlat):
    """host tensors: the four reconstructions stacked on the batch axis, three binary ground truths, two latents (or None)"""
    g = torch.Generator().manual_seed(11 + nlat)
    stacked = torch.rand(4 * B, 1, *dims, generator=g)
    gts = tuple((torch.rand(B, 1, *dims, generator=g) > 0.6).float() for _ in range(3))
    lat = tuple(torch.randn(nlat, generator=g) for _ in range(2)) if nlat else (None, None)
    return stacked, gts, lat


def run_cae(crit, B, dims, nlat, coef):
    """sp_cae_loss_fwd / _bwd, or (crit) sp_cae_loss_crit_fwd / _bwd with terms = SP_VLOSS_DICE, on the inputs of cae_inputs with the
    reconstructions read in place as slices of the stacked tensor; coef: the caller's buffer -> loss, the six gradients"""
    from stroke_prediction_amd.runtime import lib as L, ops as O
    stacked, gts, lat = cae_inputs(B, dims, nlat)
    stacked = stacked.to(DEV)
    ts = [stacked[k * B:(k + 1) * B] for k in range(4)] + [t.to(DEV) for t in gts]
    z = [None if x is None else x.to(DEV) for x in lat]
    dhw = ts[0][0].numel()
    args = []
    for t in ts:
        args += [O.ptr(t), t.stride(0)]
    zp = [None if x is None else O.ptr(x) for x in z]
    sums = torch.zeros(L.SP_REDUCE_ROWS, 16, dtype=torch.float64, device=DEV)
    loss = torch.full((), float("nan"), device=DEV)
    weights = [0.8, 0.0, L.SP_VLOSS_DICE] if crit else [0.8]
    L.call("sp_cae_loss_crit_fwd" if crit else "sp_cae_loss_fwd", *args, B, dhw, *zp, nlat, *weights, EPS, 0.36, O.ptr(sums), O.ptr(loss),
           O.ptr(coef), O.stream())
    d = [torch.full((B, dhw), float("nan"), device=DEV) for _ in range(4)]
    dz = [torch.full((nlat,), float("nan"), device=DEV) for _ in range(2)]
    up = torch.tensor(0.7, device=DEV)
    L.call("sp_cae_loss_crit_bwd" if crit else "sp_cae_loss_bwd", *args, B, dhw, O.ptr(coef), O.ptr(up), *[O.ptr(x) for x in d], *zp, nlat,
           *[O.ptr(x) if nlat else None for x in dz], O.stream())
    torch.cuda.synchronize()
    return [loss] + d + dz


@pytest.mark.parametrize("B,dims,nlat", CAE_CASES)
def test_plain_and_crit_cae_entry_points_agree(B, dims, nlat):
    """sp_cae_loss_fwd / _bwd are sp_cae_loss_crit_fwd / _bwd with terms = SP_VLOSS_DICE: the loss, coef[0:8], the four reconstruction
    gradients and the two latent gradients, bit for bit"""
    plain_coef, crit_coef = torch.full((8,), float("nan"), device=DEV), torch.full((11,), float("nan"), device=DEV)
    plain, crit = run_cae(False, B, dims, nlat, plain_coef), run_cae(True, B, dims, nlat, crit_coef)
    assert bool(torch.isfinite(plain[0])) and all(bool(torch.isfinite(x).all()) for x in plain[1:])
    assert float(plain[1].abs().max()) > 0 and (nlat == 0 or float(plain[5].abs().max()) > 0)
    assert torch.equal(plain_coef, crit_coef[:8]) and torch.count_nonzero(crit_coef[8:]) == 0
    for a, b in zip(plain, crit):
        assert torch.equal(a, b)


@pytest.mark.parametrize("B,dims,nlat", CAE_CASES)
def test_plain_cae_entry_points_keep_to_eight_coefficients(B, dims, nlat):
    """the header promises sp_cae_loss_fwd / _bwd a coef buffer of 8 floats: what lies behind them is neither written by the forward
    nor read by the backward (a nonzero coef[8] would pick the BCE loop)"""
    runs = []
    for sentinel in (0.0, 1.0):
        buf = torch.full((12,), sentinel, device=DEV)
        runs.append(run_cae(False, B, dims, nlat, buf[:8]))
        assert bool((buf[8:] == sentinel).all()), buf
        assert bool(torch.isfinite(buf[:8]).all())
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_criteria_modules_against_torch():
    """BCELoss() is torch.nn.BCELoss(); DiceBCELoss(w, b) is BatchDiceLoss(w) + b * torch.nn.BCELoss(): value and gradient"""
    from stroke_prediction_amd.common.metrics import BCELoss, DiceBCELoss
    o, t = inputs(SHAPES[0])
    td = t.to(DEV)
    o64 = o.double().requires_grad_(True)
    ref = torch.nn.BCELoss()(o64, t.double())
    ref_grad, = torch.autograd.grad(ref * 1.7, o64)
    od = o.to(DEV).requires_grad_(True)
    loss = BCELoss()(od, td)
    grad, = torch.autograd.grad(loss * 1.7, od)
    print("bce", float(loss.detach()), float(ref.detach()))
    assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref))
    assert bool(torch.isfinite(grad).all())
    torch.testing.assert_close(grad.cpu().double(), ref_grad, **GRAD_TOL)

    w = [0.3, 0.7]
    _, ref_loss, _, ref_grad = oracle(o, t, w, [0.5 / 2] * 2, 1.7)      # 0.5 * mean over everything = 0.25 * each channel's mean
    dims = (0, 2, 3, 4)
    t64 = t.double()
    literal = 1 - (torch.tensor(w, dtype=torch.float64) * (2 * (o64 * t64).sum(dims) + EPS)
                   / ((o64 * o64).sum(dims) + (t64 * t64).sum(dims) + EPS)).sum() + 0.5 * torch.nn.BCELoss()(o64, t64)
    assert abs(ref_loss - float(literal)) < 1e-12
    od = o.to(DEV).requires_grad_(True)
    loss = DiceBCELoss(w, 0.5)(od, td)
    grad, = torch.autograd.grad(loss * 1.7, od)
    print("dicebce", float(loss), ref_loss)
    assert abs(float(loss) - ref_loss) <= 1e-5 * abs(ref_loss)
    assert bool(torch.isfinite(grad).all())
    torch.testing.assert_close(grad.cpu().double(), ref_grad, **GRAD_TOL)


@pytest.mark.parametrize("name", ["bce", "dicebce"])
def test_mean_of_channel_losses_fused_equals_literal(name, monkeypatch):
    """(crit(core) + crit(penu)) / 2 on channel-slice views: one launch set on the base tensors against the literal two calls"""
    from stroke_prediction_amd.common import metrics
    o, t = inputs(SHAPES[0])
    seg = o.to(DEV).requires_grad_(True)
    lab = t.to(DEV)
    crit = metrics.BCELoss() if name == "bce" else metrics.DiceBCELoss([0.8], 0.5)

    def views(s):
        return s[:, 0, :, :, :].unsqueeze(1), s[:, 1, :, :, :].unsqueeze(1)       # Unet3D.forward :76-77
    s2 = seg * 1.0                                   # non-leaf, like the network output
    outs, tgts = views(s2), (lab[:, 0:1], lab[:, 1:2])
    assert metrics._stacked_base(outs) is s2 and metrics._stacked_base(tgts) is lab
    calls = log_calls(monkeypatch)
    fused = metrics.mean_of_channel_losses(crit, outs, tgts)
    gf, = torch.autograd.grad(fused, seg)
    assert calls == ["sp_vloss_sums", "sp_vloss_finalize_clear", "sp_vloss_bwd"], calls      # the stacked route was taken
    s3 = seg * 1.0
    o3 = views(s3)
    lit = (crit(o3[0], tgts[0]) + crit(o3[1], tgts[1])) / 2
    gl, = torch.autograd.grad(lit, seg)
    assert calls[3:] == ["sp_vloss_sums", "sp_vloss_finalize_clear"] * 2 + ["sp_vloss_bwd"] * 2, calls
    print(name, float(fused), float(lit))
    assert abs(float(fused) - float(lit)) < 1e-6 * max(1.0, abs(float(lit)))
    assert bool(torch.isfinite(gf).all())
    torch.testing.assert_close(gf, gl, **GRAD_TOL)


@pytest.mark.parametrize("factor", [0.0, 0.36])
@pytest.mark.parametrize("name", ["bce", "dicebce"])
def test_fused_cae_reconstruction_loss_equals_the_composed_one(name, factor, monkeypatch):
    """metrics.cae_reconstruction_loss on sp_cae_loss_crit_fwd / _bwd (three launches: sums, finalize, backward) against the
    reference's recipe composed of torch operators and criterion calls (CaeReconstructionLearner.py:52-70): value and the gradients
    of the four reconstructions (slices of one stacked tensor) and of the two latents"""
    from types import SimpleNamespace as NS
    from stroke_prediction_amd.common import metrics
    g = torch.Generator().manual_seed(3)
    B, dims = 2, (5, 12, 20)
    stacked = torch.rand(4 * B, 1, *dims, generator=g).to(DEV).requires_grad_(True)
    gts = [(torch.rand(B, 1, *dims, generator=g) > 0.6).float().to(DEV) for _ in range(3)]
    zi = torch.randn(B, 50, 1, 2, 2, generator=g).to(DEV).requires_grad_(True)
    zl = torch.randn(B, 50, 1, 2, 2, generator=g).to(DEV).requires_grad_(True)
    crit = metrics.make_criterion(name)
    calls = log_calls(monkeypatch)
    res = {}
    for fused in (True, False):
        monkeypatch.setenv("SP_CAE_FUSED_LOSS", "1" if fused else "0")
        for t in (stacked, zi, zl):
            t.grad = None
        parts = [stacked[k * B:(k + 1) * B] for k in range(4)]          # decoder passes: core, penu, lesion, interpolation
        rec = NS(core=parts[0], penu=parts[1], lesion=parts[2], interpolation=parts[3])
        gt = NS(core=gts[0], penu=gts[1], lesion=gts[2])
        lat = NS(interpolation=zi, lesion=zl)
        del calls[:]
        loss = metrics.cae_reconstruction_loss(rec, gt, lat, factor, crit)
        assert (loss is not None) == fused
        if loss is None:
            d1, d2 = rec.penu - rec.interpolation, rec.penu - rec.core
            loss = (torch.mean(torch.abs(d1) - d1) + torch.mean(torch.abs(d2) - d2) + crit(rec.core, gt.core) + crit(rec.penu, gt.penu)
                    + crit(rec.lesion, gt.lesion) + factor * torch.mean(torch.abs(zi - zl))) / (5 + factor)
        (loss * 1.7).backward()
        if fused:      # one entry point forward (sums + finalize), one backward: three launches of the project's kernels
            assert calls == ["sp_cae_loss_crit_fwd", "sp_cae_loss_crit_bwd"], calls
        res[fused] = (float(loss), stacked.grad.clone(), zi.grad.clone(), zl.grad.clone())
    a, b = res[True], res[False]
    print(name, factor, "fused", a[0], "composed", b[0], "max |d grad|", float((a[1] - b[1]).abs().max()))
    assert abs(a[0] - b[0]) < 2e-6 * max(1.0, abs(b[0])), (a[0], b[0])
    for k in (1, 2, 3):
        assert bool(torch.isfinite(a[k]).all())
        torch.testing.assert_close(a[k], b[k], **GRAD_TOL)


def test_learner_graph_mode_with_dicebce(tmp_path):
    """the recipe of test_learner_graph_mode_matches_eager_and_follows_schedulers under make_criterion("dicebce"): a step is captured,
    the replayed losses stay within three times the eager-to-eager distance (that test's floors), and the loss falls"""
    from oracle import weights as W
    from stroke_prediction_amd.common.model.Unet3D import Unet3D
    from stroke_prediction_amd.optim import FusedAdam, attach_flat_grads
    from stroke_prediction_amd.common.metrics import make_criterion
    from stroke_prediction_amd.learner.UnetSegmentationLearner import UnetSegmentationLearner
    ch = [2, 16, 32, 64, 32, 16, 32, 2]

    class Loader(list):
        batch_size = 2
    seed = 11
    x, y = W.unet_inputs(2, (52, 52, 52), seed)
    batches = [{"case_id": [0, 1], "images": x * (1.0 + 0.1 * i), "labels": y, "clinical": torch.zeros(2, 5, 1, 1, 1)} for i in range(2)]
    traj = {}
    for tag, graph in (("eager", False), ("eager2", False), ("graph", True)):
        model = Unet3D(ch, dtype="f32")
        model.load_state_dict(W.make_state_dict(W.unet_spec(ch), seed))
        model = model.to(DEV).train()
        opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=1e-5, betas=(0.99, 0.999), capturable=True)
        attach_flat_grads(model)
        sched = torch.optim.lr_scheduler.MultiStepLR(opt, [1], gamma=0.1)
        learner = UnetSegmentationLearner(Loader(batches), None, model, opt, sched, 3, make_criterion("dicebce"), None,
                                          str(tmp_path / tag), graph=graph, batch_metrics=False)
        learner.GRAPH_WARMUP = 1
        losses = []
        for epoch in range(3):
            if epoch > 0:
                learner.adapt_lr(epoch)
            for b in batches:
                losses.append(float(learner.train_batch(b, epoch).loss))
        traj[tag] = np.array(losses)
        if graph:
            assert any(g["graph"] is not None for g in learner._graphs.values()), "no step was captured"
    le, l2, lg = traj["eager"], traj["eager2"], traj["graph"]
    noise = np.abs(l2 - le)
    print("losses eager", le, "graph", lg, "eager-vs-eager", noise, "graph-vs-eager", np.abs(lg - le))
    assert np.all(np.isfinite(lg))
    assert np.all(np.abs(lg - le) <= np.maximum(3.0 * noise, 2e-4) + 2e-3 * (np.arange(len(le)) >= 2)), (lg, le, l2)
    assert lg[5] < lg[0] and le[5] < le[0], (lg, le)


def _run_exact(rank, world, port, q):
    """one of two gloo ranks sharing the GPU: DiceBCELoss on this rank's half of the batch in the exact data-parallel mode against
    the same process's whole-batch evaluation"""
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import stroke_prediction_amd  # noqa: F401
    from stroke_prediction_amd.common.metrics import DiceBCELoss
    from stroke_prediction_amd.runtime import layers
    o, t = inputs((4, 2, 5, 7, 9))
    crit = DiceBCELoss([0.3, 0.7], 0.5)
    od, td = o.to(DEV).requires_grad_(True), t.to(DEV)
    whole = crit(od, td)
    gwhole, = torch.autograd.grad(whole * 1.7, od)
    dist.barrier()
    layers.SYNC.update(group=None, world=world, on=True, direct=None)      # what parallel.DataParallelSync(mode="exact") installs
    lo, hi = rank * 2, rank * 2 + 2
    oh = o[lo:hi].to(DEV).requires_grad_(True)
    loss = crit(oh, td[lo:hi].contiguous())
    ghalf, = torch.autograd.grad(loss * 1.7, oh)
    layers.SYNC.update(group=None, world=1, on=False, direct=None)
    q.put(dict(rank=rank, loss=float(loss.detach()), whole=float(whole.detach()), grad=ghalf.cpu(), want=gwhole[lo:hi].cpu()))
    dist.barrier()
    dist.destroy_process_group()


def test_exact_mode_two_ranks_equal_single_process():
    world, port = 2, 29761
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_run_exact, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=600) for _ in range(world)]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert sorted(r["rank"] for r in got) == [0, 1]
    for r in got:
        print("rank", r["rank"], "loss", r["loss"], "whole batch", r["whole"])
        assert abs(r["loss"] - r["whole"]) <= 1e-6 * abs(r["whole"]), r
        assert bool(torch.isfinite(r["grad"]).all())
        torch.testing.assert_close(r["grad"], r["want"], **GRAD_TOL)
