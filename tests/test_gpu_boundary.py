"""The boundary (signed-distance) criteria on the device: ``sp_signed_distance_batch``, the ``sp_bloss_*`` kernels,
``metrics.BoundaryLoss`` / ``DiceBoundaryLoss``, the stacked route of ``mean_of_channel_losses``, a replayed graph that follows the
scheduled weight, and a short U-Net training run.

The oracle is ``tests/boundary_ref.py``: scipy's exact Euclidean distance transform in fp64 per volume (cast once to fp32) and fp64
torch autograd on that map.

Bounds.  The signed distance is held bit for bit: the kernels keep the squared distances as exact integers and take one fp64 root,
rounded once, which is what scipy computes.  The Dice moments, the coefficients and the gradients keep the bounds of
``tests/test_gpu_criteria.py`` (the accumulation scheme is the same: at most 8 fp32 terms per thread, 64 lanes, 4 waves, then fp64):
rtol 1e-5, gradients rtol 1e-5 and atol 1e-9.  The boundary moment sum o*phi adds terms of both signs and can cancel to near zero,
so its error is held against what was added up: |got - ref| <= 1e-5 * sum |o*phi| (per channel; divided by the count and weighted
where it enters a loss -- ``boundary_ref.boundary_slack``).  A loss may be off by 1e-5 of its Dice bracket plus that slack.
"""
import functools

import numpy as np
import pytest
import torch

import boundary_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = R.EPS
GRAD_TOL = dict(rtol=1e-5, atol=1e-9)


# ------------------------------------------------------------------------------------------------ signed distance
def _balls(shape, n, seed, rmax=3.0):
    """union of n random balls per volume of a (B, C, D, H, W) batch -> float mask"""
    rng = np.random.RandomState(seed)
    B, C, D, H, W = shape
    zz, yy, xx = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    out = np.zeros(shape, dtype=np.float32)
    for b in range(B):
        for c in range(C):
            for _ in range(n):
                cz, cy, cx = rng.uniform(0, D - 1), rng.uniform(0, H - 1), rng.uniform(0, W - 1)
                r = rng.uniform(0.8, rmax)
                out[b, c][(zz - cz) ** 2 + (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 1.0
    return out


@functools.lru_cache(maxsize=None)
def sdf_case(name):
    """(targets fp32 (B, C, D, H, W) on the host, oracle phi) -- computed once, never modified"""
    if name == "blobs":                 # odd extents, 315 voxels per volume
        t = _balls((2, 2, 5, 7, 9), 2, 1, 2.5)
    elif name == "flat":                # an axis of extent 1 is skipped
        t = _balls((1, 1, 1, 6, 10), 2, 2, 2.0)
    elif name == "degenerate":          # one empty volume, one full volume, one single voxel in a corner
        t = np.zeros((3, 1, 4, 4, 4), dtype=np.float32)
        t[1] = 1.0
        t[2, 0, 3, 3, 3] = 1.0
    elif name == "patch":               # the U-Net label patch; a lesion touching two faces (z = 0 and x = W - 1)
        t = _balls((2, 2, 28, 64, 64), 3, 3, 9.0)
        t[0, 0, 0:6, 20:40, 50:64] = 1.0
        assert t[0, 0, 0].any() and t[0, 0, :, :, 63].any()
    elif name == "neighbours":          # adjacent volumes with very different masks: any leak across a volume border shows
        t = np.zeros((2, 2, 4, 5, 6), dtype=np.float32)
        t[0, 0, 3, 4, 5] = 1.0          # one voxel at the very end of volume (0, 0) ...
        t[0, 1, 0, 0, 0] = 1.0          # ... and one at the very start of the next
        t[1, 0] = 1.0
        t[1, 0, 0, 0, 0] = 0.0          # all but the first voxel
        t[1, 1, 1:3, 1:4, 2:5] = 1.0
    else:
        raise KeyError(name)
    t = torch.from_numpy(t)
    return t, R.signed_distance_batch(t)


def run_sdf(td):
    """sp_signed_distance_batch on a (B, C, D, H, W) device tensor or channel-slice view (read in place) -> phi, workspace floats"""
    import ctypes as C
    from stroke_prediction_amd.runtime import lib as L, ops as O
    B, Cn, D, H, W = td.shape
    n = C.c_int64(0)
    L.call("sp_signed_distance_batch_workspace", B, Cn, D, H, W, C.byref(n))
    assert n.value == 4 * td.numel() + 64 * B * Cn
    ws = torch.full((n.value + 64,), float("nan"), device=DEV)          # (a guard band behind the workspace)
    phi = torch.full((B, Cn, D, H, W), float("nan"), device=DEV)
    L.call("sp_signed_distance_batch", O.ptr(td), td.stride(0), B, Cn, D, H, W, O.ptr(phi), O.ptr(ws), n.value, O.stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[n.value:]).all()), "wrote behind the workspace"
    return phi


def assert_bitwise(got, ref):
    got = got.cpu()
    bad = got.view(torch.int32) != ref.view(torch.int32)
    print("phi range", float(ref.min()), float(ref.max()), "differing voxels", int(bad.sum()), "max |d|", float((got - ref).abs().max()))
    assert not bool(bad.any())


@pytest.mark.parametrize("name", ["blobs", "flat", "degenerate", "patch", "neighbours"])
def test_signed_distance_equals_the_oracle_bit_for_bit(name):
    t, ref = sdf_case(name)
    assert_bitwise(run_sdf(t.to(DEV)), ref)
    if name == "degenerate":
        assert not ref[0].any() and not ref[1].any() and float(ref[2, 0, 0, 0, 0]) == float(np.float32(np.sqrt(27.0)))


def test_signed_distance_of_a_channel_slice_and_through_the_module():
    """targets as channels 1..2 of a three-channel tensor: the batch stride is 3 volumes, not C = 2; metrics.signed_distance_batch
    reads the view in place"""
    from stroke_prediction_amd.common import metrics
    t, ref = sdf_case("blobs")
    wide = torch.cat((1.0 - t[:, 0:1], t), 1).to(DEV)
    view = wide[:, 1:3]
    assert view.stride(0) == 3 * 315 and not view.is_contiguous()
    assert_bitwise(run_sdf(view), ref)
    assert metrics._batch_strided(view)[0] is view
    assert_bitwise(metrics.signed_distance_batch(view), ref)
    # a soft label is thresholded at 0.5; a bool / uint8 label is taken as it is
    soft = t * 0.2 + 0.4
    assert_bitwise(metrics.signed_distance_batch(soft.to(DEV)), ref)
    assert_bitwise(metrics.signed_distance_batch((t > 0.5).to(DEV)), ref)


def test_signed_distance_launch_count_does_not_depend_on_the_batch(monkeypatch):
    """one entry-point call per map whatever B and C, and errors for what the axis scan does not take"""
    from stroke_prediction_amd.common import metrics
    from stroke_prediction_amd.runtime import lib as L
    calls, real = [], L.call

    def logging_call(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(L, "call", logging_call)
    for case in ("blobs", "degenerate"):
        del calls[:]
        metrics.signed_distance_batch(sdf_case(case)[0].to(DEV))
        assert calls == ["sp_signed_distance_batch_workspace", "sp_signed_distance_batch"], calls
    with pytest.raises(RuntimeError, match="workspace of 10 floats"):
        t = sdf_case("flat")[0].to(DEV)
        ws = torch.empty(10, device=DEV)
        phi = torch.empty_like(t)
        real("sp_signed_distance_batch", t.data_ptr(), t.stride(0), 1, 1, 1, 6, 10, phi.data_ptr(), ws.data_ptr(), 10, None)


# ------------------------------------------------------------------------------------------------ sums, finalize, backward
LOSS_SHAPES = [(2, 2, 5, 7, 9),        # 315 voxels: one block, a tail, element loads (315 % 4 != 0)
               (2, 2, 5, 21, 43),      # 4515 voxels: three blocks in x, several replica rows, odd length
               (2, 2, 6, 20, 36)]      # 4320 voxels: three blocks, aligned -> 16-byte loads
VARIANTS = {"boundary": (None, [0.5, 0.5], 1.0),
            "diceboundary": ([0.5, 0.5], [0.5, 0.5], 0.01),
            "weighted": ([0.3, 0.7], [0.3, 0.7], 0.25)}


@functools.lru_cache(maxsize=None)
def loss_inputs(shape, seed=3):
    """(o, t, phi) fp32 on the host: o uniform in (0, 1) with exact 0 and 1 planted at the head of every channel row of sample 0
    (against a target of 0 and of 1), t blobs, phi the oracle map of t"""
    g = torch.Generator().manual_seed(seed + sum(shape))
    o = torch.rand(*shape, generator=g)
    t = torch.from_numpy(_balls(shape, 3, seed + sum(shape), 3.5))
    for c in range(shape[1]):
        orow, trow = o[0, c].view(-1), t[0, c].view(-1)
        for k, v in enumerate((0.0, 1.0)):
            orow[2 * k] = orow[2 * k + 1] = v
            trow[2 * k], trow[2 * k + 1] = 0.0, 1.0
    for b in range(shape[0]):
        for c in range(shape[1]):
            assert 0 < float(t[b, c].sum()) < t[b, c].numel()
    return o, t, R.signed_distance_batch(t)


def run_bloss(od, td, pd, w_dice, w_bnd, scale, upstream):
    """the three entry points on (B, C, ...) device tensors -> sums (C, 4), cleared rows, loss, coef (C, 3), grad"""
    from stroke_prediction_amd.runtime import lib as L, ops as O
    B, C = od.shape[0], od.shape[1]
    dhw = od[0, 0].numel()
    sums = torch.zeros(L.SP_REDUCE_ROWS, L.SP_BLOSS_PITCH(C), dtype=torch.float64, device=DEV)
    L.call("sp_bloss_sums", O.ptr(od), od.stride(0), O.ptr(td), td.stride(0), O.ptr(pd), B, C, dhw, 0 if w_dice is None else 1, O.ptr(sums),
           O.stream())
    got = sums.sum(0)[:4 * C].view(C, 4).cpu()
    wd = None if w_dice is None else torch.tensor(w_dice, dtype=torch.float32, device=DEV)
    wb = torch.tensor(w_bnd, dtype=torch.float32, device=DEV)
    sc = torch.tensor([scale], dtype=torch.float32, device=DEV)
    loss, coef = torch.empty((), device=DEV), torch.empty(3 * C, device=DEV)
    L.call("sp_bloss_finalize_clear", O.ptr(sums), None if wd is None else O.ptr(wd), O.ptr(wb), O.ptr(sc), EPS, float(B * dhw), C,
           O.ptr(loss), O.ptr(coef), O.stream())
    d = torch.full((B, C) + tuple(od.shape[2:]), float("nan"), device=DEV)
    up = torch.tensor(upstream, dtype=torch.float32, device=DEV)
    L.call("sp_bloss_bwd", O.ptr(od), od.stride(0), O.ptr(td), td.stride(0), O.ptr(pd), O.ptr(coef), O.ptr(up), B, C, dhw, O.ptr(d),
           O.stream())
    return got, sums.cpu(), float(loss), coef.cpu().view(C, 3), d.cpu()


def loss_tolerance(ref_sums, mag, w_dice, w_bnd, scale, count):
    """1e-5 of the Dice bracket + the boundary slack (module docstring)"""
    dice = 0.0
    if w_dice is not None:
        I, O_, T = ref_sums[:, 0], ref_sums[:, 1], ref_sums[:, 2]
        dice = abs(1.0 - float((torch.tensor(w_dice, dtype=torch.float64) * (2 * I + EPS) / (O_ + T + EPS)).sum()))
    return 1e-5 * dice + R.boundary_slack(mag, w_bnd, scale, count)


def check_bloss(o, t, phi, od, td, pd, variant):
    w_dice, w_bnd, scale = VARIANTS[variant]
    C = o.shape[1]
    count = o.numel() // C
    got, cleared, loss, coef, d = run_bloss(od, td, pd, w_dice, w_bnd, scale, 0.5)
    ref_sums, mag, ref_loss, ref_coef, ref_grad = R.loss_oracle(o, t, phi, w_dice, w_bnd, scale, 0.5)
    print(variant, tuple(o.shape), "boundary moment", got[:, 3].tolist(), "ref", ref_sums[:, 3].tolist(), "magnitude", mag.tolist(),
          "err / magnitude", ((got[:, 3] - ref_sums[:, 3]).abs() / mag).tolist(), "loss", loss, ref_loss)
    if w_dice is not None:
        torch.testing.assert_close(got[:, :3], ref_sums[:, :3], rtol=1e-5, atol=0)
    else:
        assert torch.count_nonzero(got[:, :3]) == 0          # moments not asked for are not computed
    assert bool(((got[:, 3] - ref_sums[:, 3]).abs() <= 1e-5 * mag).all())
    assert torch.count_nonzero(cleared) == 0, "finalize_clear must leave the accumulator zero"
    assert abs(loss - ref_loss) <= loss_tolerance(ref_sums, mag, w_dice, w_bnd, scale, count), (loss, ref_loss)
    torch.testing.assert_close(coef.double(), ref_coef, **GRAD_TOL)
    assert bool(torch.isfinite(d).all())
    torch.testing.assert_close(d.double(), ref_grad, **GRAD_TOL)


def _shifted(x):
    """a copy of x one float into an allocation: 4-byte aligned only"""
    buf = torch.empty(x.numel() + 4, device=DEV)
    out = buf[1:1 + x.numel()].view(x.shape).copy_(x)
    assert out.data_ptr() % 16 == 4
    return out


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("shape", LOSS_SHAPES)
def test_bloss_kernels_against_the_oracle(shape, variant):
    o, t, phi = loss_inputs(shape)
    od, td, pd = o.to(DEV), t.to(DEV), phi.to(DEV)
    assert od.data_ptr() % 16 == 0 and td.data_ptr() % 16 == 0 and pd.data_ptr() % 16 == 0
    check_bloss(o, t, phi, od, td, pd, variant)
    # every operand in turn on a base that is misaligned by one float: element loads whatever the length
    check_bloss(o, t, phi, _shifted(od), td, pd, variant)
    check_bloss(o, t, phi, od, _shifted(td), pd, variant)
    check_bloss(o, t, phi, od, td, _shifted(pd), variant)
    if shape == LOSS_SHAPES[0]:
        # the channel slice [:, 1:2] of outputs and targets read in place (batch stride = both channels), phi dense
        w_dice, w_bnd, scale = VARIANTS[variant]
        got = run_bloss(od[:, 1:2], td[:, 1:2], pd[:, 1:2].contiguous(), None if w_dice is None else w_dice[1:], w_bnd[1:], scale, 0.5)
        ref = R.loss_oracle(o[:, 1:2], t[:, 1:2], phi[:, 1:2], None if w_dice is None else w_dice[1:], w_bnd[1:], scale, 0.5)
        assert abs(got[2] - ref[2]) <= loss_tolerance(ref[0], ref[1], None if w_dice is None else w_dice[1:], w_bnd[1:], scale, 2 * 315)
        torch.testing.assert_close(got[4].double(), ref[4], **GRAD_TOL)


def _module_and_terms(name):
    from stroke_prediction_amd.common import metrics
    if name == "boundary":
        return metrics.BoundaryLoss(), None, [0.5, 0.5], 1.0
    if name == "boundary_weighted":
        return metrics.BoundaryLoss([0.3, 0.7], weight=0.25), None, [0.3, 0.7], 0.25
    if name == "diceboundary":
        return metrics.DiceBoundaryLoss([0.5, 0.5]), [0.5, 0.5], [0.5, 0.5], 0.01
    return metrics.DiceBoundaryLoss([0.3, 0.7], boundary_weight=0.2), [0.3, 0.7], [0.5, 0.5], 0.2


@pytest.mark.parametrize("name", ["boundary", "boundary_weighted", "diceboundary", "diceboundary_weighted"])
def test_criteria_modules_against_the_oracle_and_bit_identical_twice(name):
    """the modules compute their own map: value and gradient against the oracle on the oracle's map; DiceBoundaryLoss is
    BatchDiceLoss + boundary_weight * BoundaryLoss(); a second run gives the same bits"""
    from stroke_prediction_amd.common import metrics
    crit, w_dice, w_bnd, scale = _module_and_terms(name)
    o, t, phi = loss_inputs(LOSS_SHAPES[1])
    td = t.to(DEV)
    ref_sums, mag, ref_loss, _, ref_grad = R.loss_oracle(o, t, phi, w_dice, w_bnd, scale, 1.7)
    runs = []
    for _ in range(2):
        od = o.to(DEV).requires_grad_(True)
        loss = crit(od, td)
        grad, = torch.autograd.grad(loss * 1.7, od)
        runs.append((loss.detach().clone(), grad.clone()))
    loss, grad = runs[0]
    print(name, float(loss), ref_loss)
    assert abs(float(loss) - ref_loss) <= loss_tolerance(ref_sums, mag, w_dice, w_bnd, scale, o.numel() // 2)
    assert bool(torch.isfinite(grad).all())
    torch.testing.assert_close(grad.cpu().double(), ref_grad, **GRAD_TOL)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two runs differ"
    if name == "diceboundary_weighted":
        od = o.to(DEV)
        parts = float(metrics.BatchDiceLoss([0.3, 0.7])(od, td)) + 0.2 * float(metrics.BoundaryLoss()(od, td))
        assert abs(float(loss) - parts) <= 2 * loss_tolerance(ref_sums, mag, w_dice, w_bnd, scale, o.numel() // 2) + 1e-6
    for ent in (e for k, e in metrics._CRIT_SUMS.items() if k[0] == "bloss"):
        assert not ent[1] and torch.count_nonzero(ent[0]) == 0


@pytest.mark.parametrize("name", ["boundary", "diceboundary"])
def test_mean_of_channel_losses_stacked_equals_literal(name, monkeypatch):
    """(crit(core) + crit(penu)) / 2 on channel-slice views: one signed-distance set and one sums / finalize / backward set on the base
    tensors against the literal two calls, within 2e-6 of the magnitude (Dice bracket + weighted sum |o phi| / count); the gradient
    lands on the base tensor"""
    from stroke_prediction_amd.common import metrics
    from stroke_prediction_amd.runtime import lib as L
    o, t, phi = loss_inputs(LOSS_SHAPES[0])
    seg = o.to(DEV).requires_grad_(True)
    lab = t.to(DEV)
    crit = metrics.BoundaryLoss(weight=0.7) if name == "boundary" else metrics.DiceBoundaryLoss([0.8], 0.3)
    w_dice, w_bnd, scale = (None, [0.5, 0.5], 0.7) if name == "boundary" else ([0.4, 0.4], [0.5, 0.5], 0.3)

    def views(s):
        return s[:, 0, :, :, :].unsqueeze(1), s[:, 1, :, :, :].unsqueeze(1)       # Unet3D.forward :76-77
    calls, real = [], L.call

    def logging_call(fn, *args):
        calls.append(fn)
        return real(fn, *args)
    monkeypatch.setattr(L, "call", logging_call)
    s2 = seg * 1.0                                   # non-leaf, like the network output
    outs, tgts = views(s2), (lab[:, 0:1], lab[:, 1:2])
    assert metrics._stacked_base(outs) is s2 and metrics._stacked_base(tgts) is lab
    fused = metrics.mean_of_channel_losses(crit, outs, tgts)
    gf, = torch.autograd.grad(fused, seg)
    sdf = ["sp_signed_distance_batch_workspace", "sp_signed_distance_batch"]
    assert calls == sdf + ["sp_bloss_sums", "sp_bloss_finalize_clear", "sp_bloss_bwd"], calls      # the stacked route was taken
    del calls[:]
    s3 = seg * 1.0
    o3 = views(s3)
    lit = (crit(o3[0], tgts[0]) + crit(o3[1], tgts[1])) / 2
    gl, = torch.autograd.grad(lit, seg)
    assert calls == (sdf + ["sp_bloss_sums", "sp_bloss_finalize_clear"]) * 2 + ["sp_bloss_bwd"] * 2, calls
    ref_sums, mag, ref_loss, _, ref_grad = R.loss_oracle(o, t, phi, w_dice, w_bnd, scale)
    magnitude = loss_tolerance(ref_sums, mag, w_dice, w_bnd, scale, o.numel() // 2) / 1e-5
    print(name, float(fused), float(lit), ref_loss, "magnitude", magnitude)
    assert abs(float(fused) - float(lit)) <= 2e-6 * magnitude
    assert abs(float(fused) - ref_loss) <= 1e-5 * magnitude
    assert gf.shape == seg.shape and bool(torch.isfinite(gf).all())
    torch.testing.assert_close(gf, gl, **GRAD_TOL)
    torch.testing.assert_close(gf.cpu().double(), ref_grad, **GRAD_TOL)


def test_weight_follows_a_replayed_graph():
    """forward + backward of DiceBoundaryLoss captured once; set_boundary_weight between replays changes what the replay computes (the
    finalize kernel reads the scalar from device memory), and the accumulator is zero after every replay"""
    from stroke_prediction_amd.common import metrics
    o, t, phi = loss_inputs(LOSS_SHAPES[0])
    td = t.to(DEV)
    static_o = o.to(DEV).requires_grad_(True)
    crit = metrics.DiceBoundaryLoss([0.3, 0.7], boundary_weight=0.01)

    def eager(weight):
        ref = metrics.DiceBoundaryLoss([0.3, 0.7], boundary_weight=weight)
        od = o.to(DEV).requires_grad_(True)
        loss = ref(od, td)
        grad, = torch.autograd.grad(loss, od)
        return loss.detach().clone(), grad.clone()

    want = {w: eager(w) for w in (0.01, 0.5)}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                    # warm-up: the accumulator of this stream and the weight's device copy exist
        for _ in range(2):
            g, = torch.autograd.grad(crit(static_o, td), static_o)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
        loss = crit(static_o, td)
        grad, = torch.autograd.grad(loss, static_o)
    key = ("bloss", static_o.device, 2, int(side.cuda_stream))
    assert key in metrics._CRIT_SUMS
    for weight in (0.01, 0.5, 0.01):
        crit.set_boundary_weight(weight)
        assert crit.boundary_weight() == weight
        graph.replay()
        torch.cuda.synchronize()
        print("replay at weight", weight, float(loss), "eager", float(want[weight][0]))
        assert torch.equal(loss, want[weight][0]), (weight, float(loss), float(want[weight][0]))
        assert torch.equal(grad, want[weight][1])
        assert torch.count_nonzero(metrics._CRIT_SUMS[key][0]) == 0 and not metrics._CRIT_SUMS[key][1]
    assert not torch.equal(want[0.01][1], want[0.5][1])
    ref = R.loss_oracle(o, t, phi, [0.3, 0.7], [0.5, 0.5], 0.5)
    assert abs(float(want[0.5][0]) - ref[2]) <= loss_tolerance(ref[0], ref[1], [0.3, 0.7], [0.5, 0.5], 0.5, o.numel() // 2)
    del graph


def test_short_unet_training_with_diceboundary():
    """a 3-scale Unet3D at 44^3, two eager steps under make_criterion("diceboundary") through the U-Net learner's loss route: finite
    loss, every parameter gradient finite and nonzero, the first loss equal to the oracle on the model's own outputs"""
    from oracle import weights as W
    from stroke_prediction_amd.common.model.Unet3D import Unet3D
    from stroke_prediction_amd.common import metrics
    import stroke_prediction_amd.common.dto.UnetDto as UnetDtoUtil
    from stroke_prediction_amd.optim import FusedAdam
    ch = [2, 16, 32, 64, 32, 16, 32, 2]
    seed = 7
    x, y = W.unet_inputs(2, (44, 44, 44), seed)
    model = Unet3D(ch, dtype="f32")
    model.load_state_dict(W.make_state_dict(W.unet_spec(ch), seed))
    model = model.to(DEV).train()
    opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=1e-5, betas=(0.99, 0.999))
    crit = metrics.configure_criterion(metrics.make_criterion("diceboundary"), type("A", (), dict(boundaryweight=0.05, boundaryramp=0.01)))
    xd, yd = x.to(DEV), y.to(DEV)
    losses = []
    for step in range(2):
        crit.adapt(step)
        dto = model(UnetDtoUtil.init_dto(xd, yd[:, 0:1], yd[:, 1:2]))
        loss = metrics.mean_of_channel_losses(crit, (dto.outputs.core, dto.outputs.penu), (dto.given_variables.core, dto.given_variables.penu))
        opt.zero_grad()
        loss.backward()
        losses.append(float(loss))
        assert np.isfinite(losses[-1])
        for pname, p in model.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and int(torch.count_nonzero(p.grad)) > 0, pname
        if step == 0:
            seg = torch.cat((dto.outputs.core, dto.outputs.penu), 1).detach().cpu()
            phi = R.signed_distance_batch(y)
            assert float(phi.abs().max()) > 0
            ref = R.loss_oracle(seg, y, phi, [0.5, 0.5], [0.5, 0.5], 0.05)
            print("first loss", losses[0], "oracle", ref[2])
            assert abs(losses[0] - ref[2]) <= loss_tolerance(ref[0], ref[1], [0.5, 0.5], [0.5, 0.5], 0.05, seg.numel() // 2)
        opt.step()
    assert crit.boundary_weight() == pytest.approx(0.06, abs=1e-12)
    print("losses", losses)
