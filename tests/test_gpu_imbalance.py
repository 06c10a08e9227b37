"""The class-imbalance criteria on the device: the ``sp_tloss_*`` kernels, ``metrics.TverskyLoss`` / ``FocalBCELoss`` /
``TverskyFocalBCELoss``, the stacked route of ``mean_of_channel_losses``, a captured training step and the exact data-parallel mode.

The oracle is ``imbalance_ref.oracle``: the formulas of ``include/stroke_amd.h`` in fp64 on the CPU, fed the fp32-rounded inputs, with
autograd for the Tversky gradient and the analytic ``fl'`` for the focal one.  Outputs are uniform in (0, 1) with planted saturated
values -- exact 0, exact 1, 1e-30 and 1 - 2^-24, each against a target of 0 and of 1 -- and binary targets, or one soft target.

Bounds.  The reduction is that of ``sp_vloss_sums`` (at most 8 non-negative fp32 terms per thread, 64 lanes, 4 waves, then fp64), so the
bounds are those of ``test_gpu_criteria``: sums and loss rtol 1e-5; coefficients and, for a focal exponent of 0, 1 or 2 -- multiplies
only --, per-voxel gradients rtol 1e-5, atol 1e-9.  A general exponent goes through ``expf(gamma * logf(x))``, which amplifies the
logarithm's rounding by about ``gamma * |log x|``; that bound is not reasoned but measured: over the five cases below with gamma 2.5
the largest relative error of a per-voxel gradient against the fp64 oracle, beyond the atol of 1e-9, was 1.447e-7 on an MI355X
(``MEASURED_GENERAL_GAMMA_RTOL``; 1.0e-7 to 1.4e-7 for the exponents 0, 1 and 2: where the amplified error is large the value is
below the atol), and the bound is ten times that, 1.447e-6 -- the headroom the criteria tests document.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import imbalance_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
EPS = R.EPS
PLANTED = [0.0, 1.0, 1e-30, 1.0 - 2.0 ** -24]
GRAD_TOL = dict(rtol=1e-5, atol=1e-9)
MEASURED_GENERAL_GAMMA_RTOL = 1.447e-7
GENERAL_GAMMA_TOL = dict(rtol=10 * MEASURED_GENERAL_GAMMA_RTOL, atol=1e-9)
TVERSKY, FOCAL = 1, 2

# name -> (shape of the allocation, channel slice or None): a, b dense; c channels 1..2 of a four-channel tensor that starts one float
# into its allocation (batch stride 4 * 192 > C * DHW, rows 4-byte aligned only: a length that would take 16-byte loads, on element
# loads); d six workgroups along x; e 6 x 12 workgroups, more than SP_REDUCE_ROWS in x + y: the replica rows wrap
SHAPES = {"a": ((2, 2, 3, 5, 7), None), "b": ((2, 3, 4, 6, 8), None), "c": ((2, 4, 4, 6, 8), (1, 3)), "d": ((1, 1, 12, 28, 31), None),
          "e": ((3, 4, 13, 28, 31), None)}
# (shape, terms, tversky gamma, focal gamma, fp, fn, soft target)
CASES = [("a", TVERSKY | FOCAL, 1.0, 2.0, 0.3, 0.7, False),
         ("a", TVERSKY, 4.0 / 3.0, 2.0, 0.5, 0.5, False),
         ("a", FOCAL, 1.0, 2.5, 0.3, 0.7, False),
         ("b", TVERSKY | FOCAL, 4.0 / 3.0, 2.0, 1.0, 0.0, False),
         ("b", FOCAL, 1.0, 0.0, 0.3, 0.7, False),
         ("b", TVERSKY | FOCAL, 1.0, 2.5, 0.5, 0.5, True),
         ("c", TVERSKY | FOCAL, 1.5, 1.0, 0.3, 0.7, False),
         ("c", FOCAL, 1.0, 2.0, 0.3, 0.7, False),
         ("c", TVERSKY | FOCAL, 1.0, 2.5, 1.0, 0.0, False),
         ("d", TVERSKY | FOCAL, 1.0, 0.0, 0.5, 0.5, True),
         ("d", TVERSKY, 1.0, 2.0, 1.0, 0.0, False),
         ("d", TVERSKY | FOCAL, 1.5, 2.5, 0.3, 0.7, False),
         ("e", TVERSKY | FOCAL, 4.0 / 3.0, 2.0, 0.3, 0.7, False),
         ("e", TVERSKY | FOCAL, 1.5, 1.0, 0.5, 0.5, False),
         ("e", FOCAL, 1.0, 2.5, 0.3, 0.7, False)]
ALPHA = 0.3


@functools.lru_cache(maxsize=None)
def inputs(shape, soft=False, seed=5):
    """(o, t) fp32 on the host: o uniform with the planted values at the head of every channel row of sample 0, against targets of 0
    and of 1; t binary, or (soft) uniform in [0, 1] behind the planted pairs"""
    g = torch.Generator().manual_seed(seed + sum(shape))
    o = torch.rand(*shape, generator=g)
    t = torch.rand(*shape, generator=g)
    t = t if soft else (t > 0.7).float()
    for c in range(shape[1]):
        orow, trow = o[0, c].view(-1), t[0, c].view(-1)
        for k, v in enumerate(PLANTED):
            orow[2 * k] = orow[2 * k + 1] = v
            trow[2 * k], trow[2 * k + 1] = 0.0, 1.0
    assert float(o[0, 0].view(-1)[6]) < 1.0          # 1 - 2^-24 is an fp32 number
    return o, t


def operands(name, soft):
    """host (o, t) as the oracle sees them and their device copies as the kernels do"""
    shape, chans = SHAPES[name]
    o, t = inputs(shape, soft)
    if chans is None:
        return o, t, o.to(DEV), t.to(DEV)
    dev = []
    for host in (o, t):
        buf = torch.empty(host.numel() + 4, device=DEV)
        view = buf[1:1 + host.numel()].view(shape).copy_(host.to(DEV))[:, chans[0]:chans[1]]
        assert view.data_ptr() % 16 == 4 and view[0, 0].numel() % 4 == 0 and view.stride(0) > view.shape[1] * view[0, 0].numel()
        dev.append(view)
    return o[:, chans[0]:chans[1]], t[:, chans[0]:chans[1]], dev[0], dev[1]


def run_tloss(od, td, C, terms, w_tversky, w_focal, fp, fn, tg, fg, alpha, upstream):
    """the three entry points on (B, C, ...) device tensors (views are read in place) -> sums (C, 4), cleared rows, loss, coef, grad"""
    from stroke_prediction_amd.runtime import lib as L, ops as O
    B = od.shape[0]
    dhw = od[0, 0].numel()
    sums = torch.zeros(L.SP_REDUCE_ROWS, L.SP_TLOSS_PITCH(C), dtype=torch.float64, device=DEV)
    L.call("sp_tloss_sums", O.ptr(od), od.stride(0), O.ptr(td), td.stride(0), B, C, dhw, terms, fg, alpha, O.ptr(sums), O.stream())
    got = sums.sum(0)[:4 * C].view(C, 4).cpu()
    rows_used = int((sums.abs().sum(1) > 0).sum())
    wt = None if w_tversky is None else torch.tensor(w_tversky, dtype=torch.float32, device=DEV)
    wf = None if w_focal is None else torch.tensor(w_focal, dtype=torch.float32, device=DEV)
    loss, coef = torch.empty((), device=DEV), torch.empty(3 * C, device=DEV)
    L.call("sp_tloss_finalize_clear", O.ptr(sums), None if wt is None else O.ptr(wt), None if wf is None else O.ptr(wf), fp, fn, tg, EPS,
           float(B * dhw), C, O.ptr(loss), O.ptr(coef), O.stream())
    d = torch.full((B, C) + tuple(od.shape[2:]), float("nan"), device=DEV)
    up = torch.tensor(upstream, dtype=torch.float32, device=DEV)
    L.call("sp_tloss_bwd", O.ptr(od), od.stride(0), O.ptr(td), td.stride(0), O.ptr(coef), O.ptr(up), fg, alpha, B, C, dhw, O.ptr(d), O.stream())
    return got, sums.cpu(), float(loss), coef.cpu().view(C, 3), d.cpu(), rows_used


def needed_rtol(got, ref, atol):
    """the smallest rtol at which assert_close(got, ref, rtol, atol) holds"""
    excess = ((got - ref).abs() - atol).clamp_min(0.0)
    return float((excess / ref.abs().clamp_min(1e-300)).max())


@pytest.mark.parametrize("case", CASES, ids=["%s-terms%d-tg%.3g-fg%.3g-fp%.3g-fn%.3g%s" % (c[:6] + ("-soft" if c[6] else "",)) for c in CASES])
def test_tloss_kernels_against_the_oracle(case):
    name, terms, tg, fg, fp, fn, soft = case
    o, t, od, td = operands(name, soft)
    C = o.shape[1]
    w_tversky = [0.3, 0.7, 0.4, 0.6][:C] if terms & TVERSKY else None
    w_focal = [0.6, 0.25, 0.15, 0.5][:C] if terms & FOCAL else None
    got, cleared, loss, coef, d, rows_used = run_tloss(od, td, C, terms, w_tversky, w_focal, fp, fn, tg, fg, ALPHA, 0.5)
    ref_sums, ref_loss, ref_coef, ref_grad = R.oracle(o, t, w_tversky, w_focal, fp, fn, tg, fg, ALPHA, upstream=0.5)
    general = bool(terms & FOCAL) and fg not in (0.0, 1.0, 2.0)
    cols = ([0, 1, 2] if terms & TVERSKY else []) + ([3] if terms & FOCAL else [])
    print(case, "sums rel err", ((got - ref_sums).abs() / ref_sums.abs().clamp_min(1e-300))[:, cols].max().item(), "loss", loss, ref_loss,
          "coef rtol needed", needed_rtol(coef.double(), ref_coef, 1e-9), "grad rtol needed", needed_rtol(d.double(), ref_grad, 1e-9),
          "(general gamma)" if general else "", "replica rows used", rows_used)
    if terms & TVERSKY:
        torch.testing.assert_close(got[:, :3], ref_sums[:, :3], rtol=1e-5, atol=0)
    else:
        assert torch.count_nonzero(got[:, :3]) == 0          # columns not asked for are not computed
    if terms & FOCAL:
        torch.testing.assert_close(got[:, 3], ref_sums[:, 3], rtol=1e-5, atol=0)
    else:
        assert torch.count_nonzero(got[:, 3]) == 0
    if name in ("d", "e"):
        from stroke_prediction_amd.runtime import lib as L
        assert rows_used == min(L.SP_REDUCE_ROWS, 6 + od.shape[0] * C - 1)      # six workgroups along x: several rows; e: all of them, wrapped
    assert torch.count_nonzero(cleared) == 0, "finalize_clear must leave the accumulator zero"
    assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss), (loss, ref_loss)
    torch.testing.assert_close(coef.double(), ref_coef, **GRAD_TOL)
    assert bool(torch.isfinite(d).all())
    torch.testing.assert_close(d.double(), ref_grad, **(GENERAL_GAMMA_TOL if general else GRAD_TOL))


def test_two_calls_in_a_row_give_the_same_bits():
    """the accumulator is zero again after finalize: the second call of a module reads no residue of the first"""
    from stroke_prediction_amd.common import metrics
    o, t = inputs(SHAPES["e"][0])
    od, td = o.to(DEV), t.to(DEV)
    for crit in (metrics.TverskyFocalBCELoss([0.3, 0.7, 0.4, 0.6], 0.5, tversky_gamma=4.0 / 3.0), metrics.FocalBCELoss(gamma=2.5)):
        first = crit(od, td)
        second = crit(od, td)
        third = crit(od, td)
        assert bool(torch.isfinite(first)) and float(first) > 0
        assert torch.equal(first, second) and torch.equal(first, third), (float(first), float(second), float(third))


def test_tversky_half_half_is_the_first_moment_dice():
    """TverskyLoss([1], 0.5, 0.5) = 1 - (sum o t + eps) / (0.5 sum o + 0.5 sum t + eps), computed by torch in fp64"""
    from stroke_prediction_amd.common.metrics import TverskyLoss
    o, t = inputs((2, 1, 3, 5, 7))
    o64, t64 = o.double().requires_grad_(True), t.double()
    ref = 1 - ((o64 * t64).sum() + EPS) / (0.5 * o64.sum() + 0.5 * t64.sum() + EPS)
    ref_grad, = torch.autograd.grad(ref * 1.7, o64)
    od = o.to(DEV).requires_grad_(True)
    loss = TverskyLoss([1.0], 0.5, 0.5)(od, t.to(DEV))
    grad, = torch.autograd.grad(loss * 1.7, od)
    print("tversky 0.5/0.5", float(loss.detach()), float(ref.detach()))
    assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-5 * abs(float(ref.detach()))
    torch.testing.assert_close(grad.cpu().double(), ref_grad, **GRAD_TOL)


def test_focal_gamma_zero_is_half_the_bce():
    """FocalBCELoss(gamma=0, alpha=0.5) = 0.5 * metrics.BCELoss(): loss and gradient within rtol 1e-6, on outputs in [0.01, 0.99].
    At a saturated output the two gradients differ by construction and are not compared: fl' is the derivative of each clamped
    branch (1 / (1 - o) = 1 at o = 0 against a target of 0), while sp_vloss_bwd's (o - t) / max(o (1 - o), 1e-12) is 0 there.  The
    planted points are held to the oracle in test_tloss_kernels_against_the_oracle."""
    from stroke_prediction_amd.common import metrics
    g = torch.Generator().manual_seed(9)
    o = torch.rand(*SHAPES["b"][0], generator=g) * 0.98 + 0.01
    t = (torch.rand(*SHAPES["b"][0], generator=g) > 0.7).float()
    td = t.to(DEV)
    res = []
    for crit in (metrics.FocalBCELoss(gamma=0.0, alpha=0.5), metrics.BCELoss()):
        od = o.to(DEV).requires_grad_(True)
        loss = crit(od, td)
        grad, = torch.autograd.grad(loss, od)
        res.append((float(loss.detach()), grad))
    (lf, gf), (lb, gb) = res
    print("focal(0, 0.5)", lf, "0.5 * bce", 0.5 * lb, "max |d grad|", float((gf - 0.5 * gb).abs().max()))
    assert abs(lf - 0.5 * lb) <= 1e-6 * abs(0.5 * lb)
    assert bool(torch.isfinite(gf).all())
    torch.testing.assert_close(gf, 0.5 * gb, rtol=1e-6, atol=0)


def test_degenerate_channels():
    """an empty channel (target and output all zero) and a perfectly predicted one: finite loss, zero Tversky gradient -- with
    gamma = 4/3 the unclamped derivative is 0^(-1/4)"""
    from stroke_prediction_amd.common.metrics import TverskyLoss
    perfect = (torch.rand(2, 1, 3, 5, 7, generator=torch.Generator().manual_seed(1)) > 0.5).float()
    zero = torch.zeros(2, 1, 3, 5, 7)
    for gamma in (1.0, 4.0 / 3.0):
        for o, t in ((zero, zero), (perfect, perfect)):
            od = o.to(DEV).requires_grad_(True)
            loss = TverskyLoss([1.0], gamma=gamma)(od, t.to(DEV))
            grad, = torch.autograd.grad(loss, od)
            print("gamma", gamma, "sum t", float(t.sum()), "loss", float(loss.detach()))
            assert bool(torch.isfinite(loss)) and abs(float(loss) - 1e-12 ** (1.0 / gamma)) <= 1e-5 * 1e-12 ** (1.0 / gamma)
            assert torch.count_nonzero(grad) == 0
    # beside a channel that learns: its gradient is the oracle's, the empty channel's is zero
    o, t = inputs((2, 2, 3, 5, 7))
    o, t = o.clone(), t.clone()
    o[:, 1], t[:, 1] = 0.0, 0.0
    od = o.to(DEV).requires_grad_(True)
    loss = TverskyLoss([0.5, 0.5], gamma=4.0 / 3.0)(od, t.to(DEV))
    grad, = torch.autograd.grad(loss, od)
    _, ref_loss, _, ref_grad = R.oracle(o, t, [0.5, 0.5], None, 0.3, 0.7, 4.0 / 3.0)
    assert abs(float(loss) - ref_loss) <= 1e-5 * abs(ref_loss)
    assert torch.count_nonzero(grad[:, 1]) == 0 and float(grad[:, 0].abs().max()) > 0
    torch.testing.assert_close(grad.cpu().double(), ref_grad, **GRAD_TOL)


def log_calls(monkeypatch):
    """the call log of the launch-count checks: the name of every entry point called through the binding from here on"""
    from stroke_prediction_amd.runtime import lib as L
    calls, real_call = [], L.call

    def logging_call(name, *args):
        calls.append(name)
        return real_call(name, *args)
    monkeypatch.setattr(L, "call", logging_call)
    return calls


@pytest.mark.parametrize("name", ["tversky", "focaltversky", "focalbce", "tverskyfocalbce"])
def test_mean_of_channel_losses_fused_equals_literal(name, monkeypatch):
    """(crit(core) + crit(penu)) / 2 on channel-slice views: one launch set on the base tensors against the literal two calls"""
    from stroke_prediction_amd.common import metrics
    o, t = inputs(SHAPES["a"][0])
    seg = o.to(DEV).requires_grad_(True)
    lab = t.to(DEV)
    crit = metrics.make_criterion(name)

    def views(s):
        return s[:, 0, :, :, :].unsqueeze(1), s[:, 1, :, :, :].unsqueeze(1)       # Unet3D.forward :76-77
    s2 = seg * 1.0                                   # non-leaf, like the network output
    outs, tgts = views(s2), (lab[:, 0:1], lab[:, 1:2])
    assert metrics._stacked_base(outs) is s2 and metrics._stacked_base(tgts) is lab
    calls = log_calls(monkeypatch)
    fused = metrics.mean_of_channel_losses(crit, outs, tgts)
    gf, = torch.autograd.grad(fused, seg)
    assert calls == ["sp_tloss_sums", "sp_tloss_finalize_clear", "sp_tloss_bwd"], calls      # the stacked route was taken
    s3 = seg * 1.0
    o3 = views(s3)
    lit = (crit(o3[0], tgts[0]) + crit(o3[1], tgts[1])) / 2
    gl, = torch.autograd.grad(lit, seg)
    assert calls[3:] == ["sp_tloss_sums", "sp_tloss_finalize_clear"] * 2 + ["sp_tloss_bwd"] * 2, calls
    print(name, float(fused), float(lit))
    assert abs(float(fused) - float(lit)) < 1e-6 * max(1.0, abs(float(lit)))
    assert bool(torch.isfinite(gf).all())
    torch.testing.assert_close(gf, gl, **GRAD_TOL)


def test_learner_graph_mode_with_tverskyfocalbce(tmp_path):
    """the recipe of test_learner_graph_mode_with_dicebce under make_criterion("tverskyfocalbce"): a step is captured, the replayed
    losses stay within three times the eager-to-eager distance (that test's floors), and the loss falls"""
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
        learner = UnetSegmentationLearner(Loader(batches), None, model, opt, sched, 3, make_criterion("tverskyfocalbce"), None,
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
    """one of two gloo ranks sharing the GPU: the focal Tversky loss -- not linear in the sums, so local sums would show -- on this
    rank's half of the batch in the exact data-parallel mode against the same process's whole-batch evaluation"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import stroke_prediction_amd  # noqa: F401
    from stroke_prediction_amd.common.metrics import TverskyLoss
    from stroke_prediction_amd.runtime import layers
    o, t = inputs((4, 2, 5, 7, 9))
    crit = TverskyLoss([0.3, 0.7], gamma=4.0 / 3.0)
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
    local = crit(o[lo:hi].to(DEV), td[lo:hi].contiguous())                 # this rank's half alone: what local sums would give
    q.put(dict(rank=rank, loss=float(loss.detach()), whole=float(whole.detach()), local=float(local), grad=ghalf.cpu(), want=gwhole[lo:hi].cpu()))
    dist.barrier()
    dist.destroy_process_group()


def test_exact_mode_two_ranks_equal_single_process():
    world, port = 2, 29767
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
        print("rank", r["rank"], "loss", r["loss"], "whole batch", r["whole"], "this half alone", r["local"])
        assert abs(r["local"] - r["whole"]) > 1e-4 * abs(r["whole"]), "the halves do not differ: local sums would pass"
        assert abs(r["loss"] - r["whole"]) <= 1e-6 * abs(r["whole"]), r
        assert bool(torch.isfinite(r["grad"]).all())
        torch.testing.assert_close(r["grad"], r["want"], **GRAD_TOL)
