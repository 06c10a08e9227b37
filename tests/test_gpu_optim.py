"""The fused optimiser family on the GPU (csrc/sp_optim.hip, optim.FusedAdam / FusedAdamW / FusedSGD): the four update rules and
the global-norm clipping against the float64 oracle of tests/optim_ref.py (pinned to torch.optim in tests/test_optim_host.py), the
16-byte / element paths, the norm, the per-tensor route, checkpoints to and from torch.optim, a captured training step and the
U-Net training script."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "stroke-prediction_amd")
DEV = "cuda:0"

import stroke_prediction_amd  # noqa: F401,E402
from stroke_prediction_amd import optim  # noqa: E402
from stroke_prediction_amd.runtime import lib as L  # noqa: E402
from stroke_prediction_amd.runtime import ops as O  # noqa: E402

import optim_ref  # noqa: E402

KIND_CODE = {"adam": 0, "adamw": 1, "sgd": 2, "nesterov": 3}
HYP = dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2, momentum=0.9)
LR_LATE = 3e-3                     # the learning rate from the third step on
STEPS = 4
BIG = 4096 * 256 * 4 + 3           # the grid-stride loops wrap (2048 workgroups of 256 lanes at most) and leave a tail of 3 elements
SIZES = (1, 3, 255, 256, 257, 1027, BIG)


@functools.lru_cache(maxsize=None)
def inputs(n):
    """p0 and the four gradients of a size, fp32 on the host: made once, never changed"""
    gen = torch.Generator().manual_seed(1000 + n % 997)
    p0 = torch.randn(n, generator=gen)
    grads = tuple(torch.randn(n, generator=gen) * (1.0 + 0.5 * i) for i in range(STEPS))
    return p0, grads


@functools.lru_cache(maxsize=None)
def max_norm_for(n, gs, clip):
    """half the smallest of the four actual norms: every step is clipped"""
    if not clip:
        return None
    return 0.5 * min(optim_ref.grad_norm([g], gs) for g in inputs(n)[1])


@functools.lru_cache(maxsize=None)
def references(kind, n, clip, gs):
    """(float64 oracle parameters, the distance d of torch.optim's fp32 CPU run from them, the oracle's norms)"""
    p0, grads = inputs(n)
    mn = max_norm_for(n, gs, clip)
    ref = optim_ref.RefOptimizer(kind, [p0.double()], HYP["lr"], betas=HYP["betas"], eps=HYP["eps"], weight_decay=HYP["weight_decay"],
                                 momentum=HYP["momentum"], grad_scale=gs, max_grad_norm=mn)
    tp = torch.nn.Parameter(p0.clone())
    kw = dict(lr=HYP["lr"], weight_decay=HYP["weight_decay"])
    topt = {"adam": lambda: torch.optim.Adam([tp], betas=HYP["betas"], eps=HYP["eps"], **kw),
            "adamw": lambda: torch.optim.AdamW([tp], betas=HYP["betas"], eps=HYP["eps"], **kw),
            "sgd": lambda: torch.optim.SGD([tp], momentum=HYP["momentum"], **kw),
            "nesterov": lambda: torch.optim.SGD([tp], momentum=HYP["momentum"], nesterov=True, **kw)}[kind]()
    norms = []
    for i, g in enumerate(grads):
        if i == 2:
            ref.hyper["lr"] = topt.param_groups[0]["lr"] = LR_LATE
        ref.step([g.double()])
        norms.append(ref.last_norm)
        tp.grad = g * gs
        if clip:
            torch.nn.utils.clip_grad_norm_([tp], mn)
        topt.step()
    want = ref.params[0]
    d = float((tp.detach().double() - want).abs().max())
    return want, d, tuple(norms)


class Kernels:
    """the two entry points on raw device tensors: what optim._FusedOptimizer._step_family issues for one flat group"""

    def __init__(self, kind, gs, max_norm):
        self.kind, self.gs = KIND_CODE[kind], gs
        self.hyper = torch.tensor([HYP["lr"], HYP["betas"][0], HYP["betas"][1], HYP["eps"], HYP["weight_decay"], max_norm or 0.0,
                                   HYP["momentum"], 0.0], dtype=torch.float32, device=DEV)
        self.step = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.clip = max_norm is not None
        self.partials = torch.full((256,), float("nan"), dtype=torch.float64, device=DEV)      # every slot in use is rewritten by stage 1
        self.norm = torch.zeros(1, dtype=torch.float32, device=DEV)

    def __call__(self, p, g, m, v):
        n = p.numel()
        npart = max(1, min(256, -(-n // 1024)))
        if self.clip:
            L.call("sp_grad_sqnorm_partials", O.ptr(g), n, O.ptr(self.partials), npart, 0, O.stream())
        self.step.add_(1)
        L.call("sp_optim_step_flat", self.kind, O.ptr(p), O.ptr(g), O.ptr(m), O.ptr(v), n, O.ptr(self.hyper), O.ptr(self.step), self.gs,
               O.ptr(self.partials) if self.clip else None, npart if self.clip else 0, O.ptr(self.norm) if self.clip else None, O.stream())


def run_kernels(kind, n, clip, gs, views=None):
    """four steps of the kernels from inputs(n); ``views(name, n)`` supplies the device buffers (default: fresh allocations)"""
    p0, grads = inputs(n)
    views = views or (lambda name, k: torch.zeros(k, dtype=torch.float32, device=DEV))
    p, g, m, v = (views(name, n) for name in "pgmv")
    p.copy_(p0)
    m.zero_()
    v.zero_()
    k = Kernels(kind, gs, max_norm_for(n, gs, clip))
    norms = []
    for i, gi in enumerate(grads):
        if i == 2:
            k.hyper[0] = LR_LATE
        g.copy_(gi)
        k(p, g, m, v)
        norms.append(float(k.norm))
    return p, m, v, norms


def check(kind, n, clip, gs, got, label=""):
    want, d, _ = references(kind, n, clip, gs)
    dist = float((got.detach().cpu().double() - want).abs().max())
    bound = 4.0 * d + 1e-7 * float(want.abs().max())
    print("%s %-8s n=%-8d clip=%-5s gs=%-4g  kernel-oracle %.3e  torch32-oracle %.3e  bound %.3e" % (label, kind, n, clip, gs, dist, d, bound))
    assert dist <= bound, (kind, n, clip, gs, dist, d, bound)


# ------------------------------------------------------------------------------------------------ 1. update rules
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", optim_ref.KINDS)
def test_update_rules_against_the_float64_oracle(kind, n):
    """every kind x clipping x grad_scale, four steps with the learning rate changed before the third: at most 4 d + 1e-7 max|p| from
    the float64 oracle, d being the distance of torch.optim's own fp32 CPU run on the same inputs (the factor 4: another association
    and fma contraction)"""
    for clip in (False, True):
        for gs in (1.0, 0.25):
            p, _, _, norms = run_kernels(kind, n, clip, gs)
            check(kind, n, clip, gs, p)
            if clip:
                for got, want in zip(norms, references(kind, n, clip, gs)[2]):
                    assert abs(got - want) <= 1e-6 * want, (got, want)


@pytest.mark.parametrize("n", SIZES)
def test_adam_kind_without_clipping_has_the_bits_of_sp_adam_step_flat_hyp(n):
    p0, grads = inputs(n)
    p, m, v, _ = run_kernels("adam", n, False, 0.25)
    q, qm, qv, g = (torch.zeros(n, dtype=torch.float32, device=DEV) for _ in range(4))
    q.copy_(p0)
    k = Kernels("adam", 0.25, None)
    for i, gi in enumerate(grads):
        if i == 2:
            k.hyper[0] = LR_LATE
        g.copy_(gi)
        k.step.add_(1)
        L.call("sp_adam_step_flat_hyp", O.ptr(q), O.ptr(g), O.ptr(qm), O.ptr(qv), n, O.ptr(k.hyper), O.ptr(k.step), 0.25, O.stream())
    assert torch.equal(p, q) and torch.equal(m, qm) and torch.equal(v, qv)
    assert float((q.cpu() - p0).abs().max()) > 1e-3


# ------------------------------------------------------------------------------------------------ 2. alignment
SENTINEL = 12345.0


@pytest.mark.parametrize("kind", optim_ref.KINDS)
@pytest.mark.parametrize("offsets", [dict(p=1, g=1, m=1, v=1), dict(p=2, g=2, m=2, v=2), dict(p=3, g=3, m=3, v=3), dict(p=0, g=1, m=0, v=0),
                                     dict(p=0, g=0, m=0, v=0)])
def test_buffers_at_any_four_byte_offset(kind, offsets):
    """n = 1027 with the buffers sliced at element offsets of larger allocations (all four, or the gradient alone; offset 0 is the
    16-byte path beside the same sentinels): the result holds test 1's bound and nothing outside the slices is written"""
    n = 1027
    backing = {}

    def views(name, k):
        backing[name] = torch.full((k + 16,), SENTINEL, dtype=torch.float32, device=DEV)
        return backing[name][4 + offsets[name]:4 + offsets[name] + k]
    for clip in (False, True):
        p, _, _, _ = run_kernels(kind, n, clip, 0.25, views)
        assert p.data_ptr() % 16 == 4 * offsets["p"]
        check(kind, n, clip, 0.25, p, "offsets %s" % (offsets,))
        for name, buf in backing.items():
            lo = 4 + offsets[name]
            assert bool((buf[:lo] == SENTINEL).all()) and bool((buf[lo + n:] == SENTINEL).all()), name
            if name == "v" and kind in ("sgd", "nesterov"):
                assert bool((buf[lo:lo + n] == 0).all())          # unused by the SGD kinds (zeroed by the harness, never written)


# ------------------------------------------------------------------------------------------------ 3. norm
def flat_param(values):
    p = torch.nn.Parameter(values.to(DEV).clone())
    p.grad = torch.zeros_like(p)
    return p


@pytest.mark.parametrize("n", SIZES)
def test_last_grad_norm(n):
    """against float64 sqrt(sum g^2) * grad_scale: double accumulation of exact squares leaves the final fp32 rounding (6e-8)"""
    p0, grads = inputs(n)
    p = flat_param(p0)
    opt = optim.FusedSGD([p], lr=1e-2, momentum=0.9, grad_scale=0.25, max_grad_norm=1.0)
    assert opt.last_grad_norm is None
    p.grad.copy_(grads[0])
    opt.step()
    want = optim_ref.grad_norm([grads[0]], 0.25)
    got = float(opt.last_grad_norm)
    print("n", n, "norm", got, "float64", want, "relative error", abs(got - want) / want)
    assert abs(got - want) <= 1e-6 * want
    assert opt._flat and opt.last_grad_norm.is_cuda


def test_norm_of_gradients_whose_fp32_square_sum_overflows():
    n = 1027
    gen = torch.Generator().manual_seed(5)
    g = torch.randn(n, generator=gen) * 1e20
    p0 = torch.randn(n, generator=gen)
    assert not np.isfinite(float((g * g).sum()))
    p = flat_param(p0)
    opt = optim.FusedSGD([p], lr=1e-2, momentum=0.9, nesterov=True, max_grad_norm=2.0)
    p.grad.copy_(g)
    opt.step()
    want = optim_ref.grad_norm([g])
    got = float(opt.last_grad_norm)
    assert np.isfinite(got) and abs(got - want) <= 1e-6 * want, (got, want)
    ref = optim_ref.RefOptimizer("nesterov", [p0.double()], 1e-2, momentum=0.9, max_grad_norm=2.0)
    ref.step([g.double()])
    assert bool(torch.isfinite(p).all())
    # the clipped gradient has norm 2: the step is lr * (1 + momentum) * that, and one fp32 rounding of the coefficient (6e-8) of it
    assert float((p.detach().cpu().double() - ref.params[0]).abs().max()) <= 1e-7 * float(ref.params[0].abs().max()) + 1e-6 * 1e-2 * 1.9 * 2.0


@pytest.mark.parametrize("cls,kw", [(optim.FusedSGD, dict(lr=1e-2, momentum=0.9, nesterov=True, weight_decay=1e-2)),
                                     (optim.FusedAdamW, dict(lr=1e-2, weight_decay=1e-2)), (optim.FusedAdam, dict(lr=1e-2, weight_decay=1e-2))])
def test_norm_below_the_limit_changes_no_bit_and_runs_repeat(cls, kw):
    n = 1027
    p0, grads = inputs(n)
    big = 10.0 * max(optim_ref.grad_norm([g]) for g in grads)

    def run(max_grad_norm, capturable=True):
        p = flat_param(p0)
        opt = cls([p], max_grad_norm=max_grad_norm, capturable=capturable, **kw)
        for g in grads:
            p.grad.copy_(g)
            opt.step()
        state = [opt.state[p][k].clone() for k in opt.MOMENTS]
        return p.detach().clone(), state, None if opt.last_grad_norm is None else opt.last_grad_norm.clone()
    free, loose, twice = run(None), run(big), run(big)
    assert torch.equal(free[0], loose[0]) and all(torch.equal(a, b) for a, b in zip(free[1], loose[1]))
    assert free[2] is None and float(loose[2]) == pytest.approx(optim_ref.grad_norm([grads[-1]]), rel=1e-6)
    assert torch.equal(loose[0], twice[0]) and all(torch.equal(a, b) for a, b in zip(loose[1], twice[1])) and torch.equal(loose[2], twice[2])
    small = 0.5 * min(optim_ref.grad_norm([g]) for g in grads)
    a, b = run(small), run(small)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1])) and torch.equal(a[2], b[2])
    assert not torch.equal(a[0], free[0])


@pytest.mark.parametrize("kind,cls,kw", [("adam", optim.FusedAdam, {}), ("adamw", optim.FusedAdamW, {}),
                                          ("sgd", optim.FusedSGD, dict(nesterov=False)), ("nesterov", optim.FusedSGD, dict(nesterov=True))])
def test_classes_drive_the_kernels(kind, cls, kw):
    """the optimiser classes on one flat parameter, clipped, hold test 1's bound (lr edited in param_groups before the third step)"""
    n, gs = 1027, 0.25
    p0, grads = inputs(n)
    for capturable in (False, True):
        p = flat_param(p0)
        if cls is optim.FusedSGD:
            opt = cls([p], lr=HYP["lr"], momentum=HYP["momentum"], weight_decay=HYP["weight_decay"], grad_scale=gs, capturable=capturable,
                      max_grad_norm=max_norm_for(n, gs, True), **kw)
        else:
            opt = cls([p], lr=HYP["lr"], betas=HYP["betas"], eps=HYP["eps"], weight_decay=HYP["weight_decay"], grad_scale=gs,
                      capturable=capturable, max_grad_norm=max_norm_for(n, gs, True))
        for i, g in enumerate(grads):
            if i == 2:
                opt.param_groups[0]["lr"] = LR_LATE
            p.grad.copy_(g)
            opt.step()
        check(kind, n, True, gs, p.detach(), "class capturable=%s" % capturable)
        if cls is not optim.FusedSGD:
            assert opt.state_dict()["state"][0]["step"] == STEPS


# ------------------------------------------------------------------------------------------------ 4. fallback route
SHAPES = ((16, 3, 3), (700,), (37, 5))       # 144 + 700 + 185 = 1029 elements


def _params(flat):
    p0, grads = inputs(1029)
    if flat:
        pbuf, gbuf = p0.to(DEV).clone(), torch.zeros(1029, device=DEV)
    ps, o = [], 0
    for s in SHAPES:
        k = int(np.prod(s))
        if flat:
            p = torch.nn.Parameter(pbuf[o:o + k].view(s))
            p.grad = gbuf[o:o + k].view(s)
        else:
            p = torch.nn.Parameter(p0[o:o + k].view(s).to(DEV).clone())
            p.grad = torch.zeros_like(p)
        ps.append(p)
        o += k
    return ps


def _set_grads(ps, g):
    o = 0
    for p in ps:
        if p.grad is None:
            p.grad = torch.zeros_like(p)
        p.grad.copy_(g[o:o + p.numel()].view(p.shape))
        o += p.numel()


@pytest.mark.parametrize("kind,cls,kw", [("adam", optim.FusedAdam, {}), ("adamw", optim.FusedAdamW, {}), ("nesterov", optim.FusedSGD, dict(momentum=0.9, nesterov=True))])
def test_loose_tensors_equal_the_flat_route(kind, cls, kw):
    """parameters that are no views of one buffer (a launch per tensor, one norm over all of them) against the flat route and the
    oracle, test 1's bound"""
    n, gs = 1029, 0.25
    _, grads = inputs(n)
    out = {}
    for flat in (True, False):
        ps = _params(flat)
        if cls is not optim.FusedSGD:
            kw = dict(betas=HYP["betas"], eps=HYP["eps"])
        opt = cls(ps, lr=HYP["lr"], weight_decay=HYP["weight_decay"], grad_scale=gs, max_grad_norm=max_norm_for(n, gs, True), **kw)
        for i, g in enumerate(grads):
            if i == 2:
                opt.param_groups[0]["lr"] = LR_LATE
            _set_grads(ps, g)
            opt.step()
        assert bool(opt._flat) is flat and bool(opt._loose) is (not flat)
        out[flat] = torch.cat([p.detach().reshape(-1) for p in ps])
        check(kind, n, True, gs, out[flat], "flat" if flat else "loose")
        assert float(opt.last_grad_norm) == pytest.approx(references(kind, n, True, gs)[2][-1], rel=1e-6)


def test_loose_tensors_share_one_global_norm():
    """two tensors, one with a large gradient: the small one's update is scaled by the coefficient of the norm over both"""
    a = torch.nn.Parameter(torch.zeros(300, device=DEV))
    b = torch.nn.Parameter(torch.zeros(5, 7, device=DEV))
    ga, gb = torch.full((300,), 100.0), torch.linspace(0.01, 0.1, 35).view(5, 7)
    a.grad, b.grad = ga.to(DEV), gb.to(DEV)
    opt = optim.FusedSGD([a, b], lr=1.0, max_grad_norm=1.0)
    opt.step()
    norm = optim_ref.grad_norm([ga, gb])
    coef = 1.0 / (norm + 1e-6)
    assert float(gb.norm()) < 1.0 < norm            # on its own the small tensor would not be clipped
    assert float(opt.last_grad_norm) == pytest.approx(norm, rel=1e-6)
    torch.testing.assert_close(b.detach().cpu(), -coef * gb, rtol=1e-5, atol=0)
    torch.testing.assert_close(a.detach().cpu(), -coef * ga, rtol=1e-5, atol=0)


# ------------------------------------------------------------------------------------------------ 5. checkpoints
def _one_step_bound(p):
    """step 3 on either side starts from the same fp32 state: the results differ by the roundings of one update, a handful of
    6e-8 relative errors of terms no larger than max|p|"""
    return 5e-7 * float(p.abs().max())


@pytest.mark.parametrize("which", ["sgd", "adamw"])
def test_checkpoints_move_to_and_from_torch_optim(which):
    n = 1029
    p0, grads = inputs(n)

    def make_torch(ps):
        if which == "sgd":
            return torch.optim.SGD(ps, lr=1e-2, momentum=0.9, nesterov=True, weight_decay=1e-2)
        return torch.optim.AdamW(ps, lr=1e-2, betas=HYP["betas"], weight_decay=1e-2)

    def make_fused(ps):
        if which == "sgd":
            return optim.FusedSGD(ps, lr=1e-2, momentum=0.9, nesterov=True, weight_decay=1e-2)
        return optim.FusedAdamW(ps, lr=1e-2, betas=HYP["betas"], weight_decay=1e-2, capturable=True)

    def host_params():
        ps, o = [], 0
        for s in SHAPES:
            k = int(np.prod(s))
            ps.append(torch.nn.Parameter(p0[o:o + k].view(s).clone()))
            o += k
        return ps

    def load_values(dst, src):
        with torch.no_grad():
            for d, s in zip(dst, src):
                d.copy_(s)
    # torch.optim on the host for two steps -> the fused class takes the state and makes the third step
    tp = host_params()
    topt = make_torch(tp)
    for g in grads[:2]:
        _set_grads(tp, g)
        topt.step()
    fp = _params(flat=True)
    load_values(fp, tp)
    fopt = make_fused(fp)
    fopt.load_state_dict(topt.state_dict())
    _set_grads(tp, grads[2])
    topt.step()
    _set_grads(fp, grads[2])
    fopt.step()
    sd = fopt.state_dict()
    if which == "sgd":
        assert sorted(sd["state"][0]) == ["momentum_buffer"] and tuple(sd["state"][2]["momentum_buffer"].shape) == SHAPES[2]
    else:
        assert sorted(sd["state"][0]) == ["exp_avg", "exp_avg_sq", "step"] and sd["state"][0]["step"] == 3      # (read back from the device)
    for a, b in zip(fp, tp):
        assert float((a.detach().cpu() - b.detach()).abs().max()) <= _one_step_bound(b.detach())
    # ... and the other way round: two fused steps -> torch.optim takes the state
    fp = _params(flat=True)
    fopt = make_fused(fp)
    for g in grads[:2]:
        _set_grads(fp, g)
        fopt.step()
    tp = host_params()
    load_values(tp, [p.detach().cpu() for p in fp])
    topt = make_torch(tp)
    sd = fopt.state_dict()
    sd = dict(state={k: {n: (v.cpu() if torch.is_tensor(v) else v) for n, v in s.items()} for k, s in sd["state"].items()},
              param_groups=sd["param_groups"])
    topt.load_state_dict(sd)
    if which == "adamw":
        assert int(topt.state[tp[0]]["step"]) == 2
    _set_grads(tp, grads[2])
    topt.step()
    _set_grads(fp, grads[2])
    fopt.step()
    for a, b in zip(fp, tp):
        assert float((a.detach().cpu() - b.detach()).abs().max()) <= _one_step_bound(b.detach())
    moved = float((torch.cat([p.detach().reshape(-1) for p in tp]) - p0).abs().max())
    assert moved > 1e-3


# ------------------------------------------------------------------------------------------------ 6. captured step
def test_learner_graph_mode_with_fused_sgd_clipping_and_poly_lr(tmp_path):
    """the recipe of test_learner_graph_mode_with_tverskyfocalbce (U-Net 2 16 32 64 32 16 32 2, f32, 2 x 52^3, GRAPH_WARMUP = 1, eager /
    eager2 / graph, that test's margin) under FusedSGD(lr 1e-2, momentum 0.99, nesterov, max_grad_norm below the first step's norm)
    with PolynomialLR: a step is captured, the loss falls, and the replayed step follows lr, and max_grad_norm without recapture.
    (For the max_grad_norm = 1e-12 replay the momentum buffer is zeroed first: at momentum 0.99 the buffer of the earlier steps
    alone moves the parameters by lr * 0.98 * buffer, whatever the clipping does to the new gradient.)"""
    from oracle import weights as W
    from stroke_prediction_amd.common.model.Unet3D import Unet3D
    from stroke_prediction_amd.optim import FusedSGD, attach_flat_grads
    from stroke_prediction_amd.common.metrics import make_criterion
    from stroke_prediction_amd.learner.UnetSegmentationLearner import UnetSegmentationLearner
    ch = [2, 16, 32, 64, 32, 16, 32, 2]

    class Loader(list):
        batch_size = 2
    seed = 11
    x, y = W.unet_inputs(2, (52, 52, 52), seed)
    batches = [{"case_id": [0, 1], "images": x * (1.0 + 0.1 * i), "labels": y, "clinical": torch.zeros(2, 5, 1, 1, 1)} for i in range(2)]

    def build(tag, graph, max_grad_norm):
        model = Unet3D(ch, dtype="f32")
        model.load_state_dict(W.make_state_dict(W.unet_spec(ch), seed))
        model = model.to(DEV).train()
        opt = FusedSGD(model.parameters(), lr=1e-2, momentum=0.99, nesterov=True, max_grad_norm=max_grad_norm, capturable=True)
        flat_grad = attach_flat_grads(model)
        sched = torch.optim.lr_scheduler.PolynomialLR(opt, total_iters=3, power=0.9)
        learner = UnetSegmentationLearner(Loader(batches), None, model, opt, sched, 3, make_criterion("dice"), None,
                                          str(tmp_path / tag), graph=graph, batch_metrics=False)
        learner.GRAPH_WARMUP = 1
        return model, opt, learner, flat_grad
    # the first step's norm, measured with a limit far above it
    _, opt, learner, flat_grad = build("probe", False, 1e9)
    learner.train_batch(batches[0], 0)
    norm0 = float(opt.last_grad_norm)
    assert norm0 == pytest.approx(float(flat_grad.double().norm()), rel=1e-6) and norm0 > 0
    limit = 0.5 * norm0
    traj = {}
    for tag, graph in (("eager", False), ("eager2", False), ("graph", True)):
        model, opt, learner, _ = build(tag, graph, limit)
        losses = []
        for epoch in range(3):
            if epoch > 0:
                learner.adapt_lr(epoch)
            for b in batches:
                losses.append(float(learner.train_batch(b, epoch).loss))
        traj[tag] = np.array(losses)
    assert any(g["graph"] is not None for g in learner._graphs.values()), "no step was captured"
    le, l2, lg = traj["eager"], traj["eager2"], traj["graph"]
    noise = np.abs(l2 - le)
    print("first norm", norm0, "losses eager", le, "graph", lg, "eager-vs-eager", noise, "graph-vs-eager", np.abs(lg - le))
    assert np.all(np.isfinite(lg))
    assert np.all(np.abs(lg - le) <= np.maximum(3.0 * noise, 2e-4) + 2e-3 * (np.arange(len(le)) >= 2)), (lg, le, l2)
    assert lg[5] < lg[0] and le[5] < le[0], (lg, le)
    assert opt.param_groups[0]["lr"] == pytest.approx(1e-2 * (1 - 2 / 3) ** 0.9)
    # the captured step follows the hyper-parameters: lr = 0 leaves every parameter bit as it is ...
    flat, _ = model.flat_buffers()
    ngraphs = len(learner._graphs)
    opt.param_groups[0]["lr"] = 0.0
    before = flat.clone()
    learner.train_batch(batches[0], 2)
    assert torch.equal(flat, before)
    # ... a replay at the learning rate and limit of the run moves them, and max_grad_norm = 1e-12 (from a zeroed momentum buffer) does not
    opt.param_groups[0]["lr"] = 1e-2
    for p in model.parameters():
        opt.state[p]["momentum_buffer"].zero_()
    learner.train_batch(batches[0], 2)
    moved = float((flat - before).abs().max())
    assert moved > 1e-8, moved
    for p in model.parameters():
        opt.state[p]["momentum_buffer"].zero_()
    opt.param_groups[0]["max_grad_norm"] = 1e-12
    before = flat.clone()
    learner.train_batch(batches[0], 2)
    still = float((flat - before).abs().max())
    print("replayed change at the clipping limit %.3e: %.3e, at 1e-12: %.3e" % (limit, moved, still))
    assert still < 1e-9
    assert len(learner._graphs) == ngraphs and float(opt.last_grad_norm) > 1e-12


# ------------------------------------------------------------------------------------------------ 7. script
def test_train_unet_segmentation_script_with_sgd_clipnorm_poly(tmp_path):
    base = str(tmp_path / "unet")
    unetpath = str(tmp_path / "unet.model")
    env = dict(os.environ, SP_SYNTHETIC_DATA="1", MPLBACKEND="Agg")
    common = [sys.executable, os.path.join(PKG, "train_unet_segmentation.py"), unetpath, "--optimizer", "sgd", "--clipnorm", "12",
              "--lrschedule", "poly", "--graph", "--devicecache", "--batchsize", "2", "--fold"] + [str(i) for i in range(8)]
    r = subprocess.run(common + ["--epochs", "1", "--outbasepath", base], capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "optimizer='sgd'" in r.stdout and "Epoch 1/1 training loss" in r.stdout
    sd = torch.load(base + "_unet.optim", weights_only=False)
    g = sd["param_groups"][0]
    assert (g["momentum"], g["nesterov"], g["max_grad_norm"], g["initial_lr"]) == (0.99, True, 12.0, 1e-2)
    assert len(sd["state"]) == len(g["params"]) > 10
    assert all(sorted(s) == ["momentum_buffer"] for s in sd["state"].values())
    assert any(float(s["momentum_buffer"].abs().max()) > 0 for s in sd["state"].values())
    # a second call continues from those files
    base2 = str(tmp_path / "unet2")
    r = subprocess.run(common + ["--epochs", "2", "--inbasepath", base, "--outbasepath", base2], capture_output=True, text=True, env=env,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "Continue training" in r.stdout and "Epoch 2/2 training loss" in r.stdout and "Epoch 1/2 training loss" not in r.stdout
    assert os.path.exists(base2 + "_unet_final.model")
