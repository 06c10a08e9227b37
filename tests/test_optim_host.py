"""The optimiser side (``--optimizer {adam,adamw,sgd} --clipnorm --lrschedule``) as far as a machine without a GPU sees it: the
flags on every training parser, ``optim.make_optimizer`` / ``make_scheduler``, the constructors' refusals, the C ABI of
csrc/sp_optim.hip, and the float64 restatement of the update rules (tests/optim_ref.py, the oracle of tests/test_gpu_optim.py)
against ``torch.optim`` + ``clip_grad_norm_``."""
import argparse
import os

import pytest
import torch

import stroke_prediction_amd  # noqa: F401
from stroke_prediction_amd import optim
from stroke_prediction_amd.runtime import lib as L

import optim_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parsers():
    from common import util
    return ((util.get_args_unet_training, ["/tmp/unet.model"]), (util.get_args_shape_training, []),
            (util.get_args_step_training, ["/tmp/cae.model"]), (util.get_args_shape_prediction_training, ["/tmp/cae.model"]))


def test_parsers_take_the_optimiser_flags(capsys):
    for parse, pos in _parsers():
        a = parse(pos)
        assert (a.optimizer, a.lr, a.momentum, a.nesterov, a.weightdecay, a.clipnorm, a.lrschedule, a.lrpower) == \
            ("adam", None, 0.99, True, None, 0.0, "multistep", 0.9)
        a = parse(pos + ["--optimizer", "sgd", "--lr", "0.02", "--momentum", "0.9", "--no-nesterov", "--weightdecay", "3e-5",
                         "--clipnorm", "12", "--lrschedule", "poly", "--lrpower", "0.8"])
        assert (a.optimizer, a.lr, a.momentum, a.nesterov, a.weightdecay, a.clipnorm, a.lrschedule, a.lrpower) == \
            ("sgd", 0.02, 0.9, False, 3e-5, 12.0, "poly", 0.8)
        assert parse(pos + ["--optimizer", "adamw", "--nesterov"]).nesterov is True
        for bad in (["--optimizer", "lamb"], ["--lrschedule", "cosine"]):
            with pytest.raises(SystemExit):
                parse(pos + bad)
            assert "invalid choice" in capsys.readouterr().err


def test_training_scripts_build_through_make_optimizer():
    pkg = os.path.join(ROOT, "stroke-prediction_amd")
    for script in ("train_unet_segmentation.py", "train_shape_reconstruction.py", "train_shape_prediction.py",
                   "train_interpolationstep_after_reconstruction.py", "train_shape_reconstruction_with_ctp.py"):
        with open(os.path.join(pkg, script)) as f:
            text = f.read()
        assert "optim.make_optimizer(args, params, " in text and "optim.make_scheduler(args, optimizer)" in text, script
        assert "torch.optim.Adam(" not in text and "FusedAdam(" not in text, script


def _args(**kw):
    base = dict(optimizer="adam", lr=None, momentum=0.99, nesterov=True, weightdecay=None, clipnorm=0.0, lrschedule="multistep",
                lrpower=0.9, lrsteps=[], epochs=10, graph=False, fusedadam=False)
    base.update(kw)
    return argparse.Namespace(**base)


# the Adam setting of each script (lr, weight decay, betas): the U-Net and CTP scripts warm up from beta1 0.99
HYPERS = (dict(lr=1e-3, weight_decay=1e-5, betas=(0.99, 0.999)), dict(lr=1e-3, weight_decay=1e-5, betas=(0.9, 0.999)))


def test_make_optimizer_defaults_are_todays_objects():
    for hyper in HYPERS:
        params = [torch.nn.Parameter(torch.zeros(3, 2)), torch.nn.Parameter(torch.zeros(5))]
        opt = optim.make_optimizer(_args(), params, hyper)
        assert type(opt) is torch.optim.Adam
        g = opt.param_groups[0]
        assert (g["lr"], g["weight_decay"], tuple(g["betas"]), g["eps"], g["amsgrad"]) == (1e-3, 1e-5, hyper["betas"], 1e-8, False)
        assert optim.make_scheduler(_args(), opt) is None
        sched = optim.make_scheduler(_args(lrsteps=[3, 6]), opt)
        assert type(sched) is torch.optim.lr_scheduler.MultiStepLR and sorted(sched.milestones) == [3, 6]
        # --fusedadam / --graph: FusedAdam as before, without a clipping key in its groups
        for kw, capturable in ((dict(fusedadam=True), False), (dict(graph=True), True), (dict(graph=True, fusedadam=True), True)):
            opt = optim.make_optimizer(_args(**kw), params, hyper)
            assert type(opt) is optim.FusedAdam and opt.capturable is capturable and opt.grad_scale == 1.0
            assert sorted(opt.param_groups[0]) == ["betas", "eps", "lr", "params", "weight_decay"]
            assert tuple(opt.param_groups[0]["betas"]) == hyper["betas"]
        # the scripts whose learner replays no captured step / which never built a fused optimiser
        assert optim.make_optimizer(_args(fusedadam=True, graph=True), params, hyper, graph=False).capturable is False
        assert type(optim.make_optimizer(_args(fusedadam=True, graph=True), params, hyper, graph=False, fusedadam=False)) is torch.optim.Adam


def test_make_optimizer_new_flags():
    hyper = HYPERS[0]
    params = [torch.nn.Parameter(torch.zeros(4))]
    opt = optim.make_optimizer(_args(clipnorm=12.0), params, hyper)
    assert type(opt) is optim.FusedAdam and opt.param_groups[0]["max_grad_norm"] == 12.0 and opt.capturable is False
    opt = optim.make_optimizer(_args(optimizer="adamw", graph=True, weightdecay=0.05), params, hyper)
    assert type(opt) is optim.FusedAdamW and opt.capturable and opt.param_groups[0]["weight_decay"] == 0.05
    assert "max_grad_norm" not in opt.param_groups[0] and opt.param_groups[0]["lr"] == 1e-3
    opt = optim.make_optimizer(_args(optimizer="sgd", clipnorm=12.0, graph=True), params, hyper)
    g = opt.param_groups[0]
    assert type(opt) is optim.FusedSGD and opt.capturable
    assert (g["lr"], g["momentum"], g["nesterov"], g["weight_decay"], g["dampening"], g["max_grad_norm"]) == (1e-2, 0.99, True, 1e-5, 0, 12.0)
    assert optim.make_optimizer(_args(optimizer="sgd", lr=0.3, nesterov=False), params, hyper).param_groups[0]["lr"] == 0.3
    sched = optim.make_scheduler(_args(lrschedule="poly", epochs=7, lrpower=0.8), opt)
    assert type(sched) is torch.optim.lr_scheduler.PolynomialLR and (sched.total_iters, sched.power) == (7, 0.8)
    sched.step()
    assert abs(opt.param_groups[0]["lr"] - 1e-2 * (1 - 1 / 7) ** 0.8) < 1e-12
    assert opt.last_grad_norm is None


def test_constructors_refuse():
    params = [torch.nn.Parameter(torch.zeros(4))]
    with pytest.raises(ValueError, match="dampening"):
        optim.FusedSGD(params, lr=0.1, momentum=0.9, dampening=0.1)
    with pytest.raises(ValueError, match="Nesterov"):
        optim.FusedSGD(params, lr=0.1, momentum=0, nesterov=True)
    with pytest.raises(ValueError):
        optim.FusedSGD(params, lr=-1.0)
    optim.FusedSGD(params, lr=0.1, momentum=0.9, nesterov=True)


def test_c_abi_of_the_family():
    assert [L.CONSTS["SP_OPT_" + n] for n in ("ADAM", "ADAMW", "SGD", "SGD_NESTEROV")] == [0, 1, 2, 3]
    assert L.SIGS["sp_grad_sqnorm_partials"] == ([L.vp, L.i64, L.vp, L.i32, L.i32, L.vp], L.i32)
    assert L.SIGS["sp_optim_step_flat"] == ([L.i32] + [L.vp] * 4 + [L.i64, L.vp, L.vp, L.f32, L.vp, L.i32, L.vp, L.vp], L.i32)
    assert "sp_optim.hip" in L.SOURCES
    # argument validation happens before any GPU work: callable without a device
    lib = L.load()
    one = 16      # (any non-null address: nothing is dereferenced on the host)
    assert lib.sp_grad_sqnorm_partials(None, 10, one, 4, 0, None) == -1 and "sp_grad_sqnorm_partials" in L.last_error()
    assert lib.sp_grad_sqnorm_partials(one, 0, one, 4, 0, None) == -1
    assert lib.sp_grad_sqnorm_partials(one, 10, one, 0, 0, None) == -1
    assert lib.sp_grad_sqnorm_partials(one, 10, one, 257, 0, None) == -1
    assert lib.sp_optim_step_flat(7, one, one, one, one, 10, one, one, 1.0, None, 0, None, None) == -1 and "kind" in L.last_error()
    assert lib.sp_optim_step_flat(0, None, one, one, one, 10, one, one, 1.0, None, 0, None, None) == -1 and "sp_optim_step_flat" in L.last_error()
    assert lib.sp_optim_step_flat(0, one, one, one, None, 10, one, one, 1.0, None, 0, None, None) == -1       # Adam needs v ...
    assert lib.sp_optim_step_flat(1, one, one, one, one, 10, one, None, 1.0, None, 0, None, None) == -1       # ... and the step count
    assert lib.sp_optim_step_flat(2, one, one, one, None, 0, one, None, 1.0, None, 0, None, None) == -1       # n = 0
    assert lib.sp_optim_step_flat(3, one, one, one, None, 10, one, None, 1.0, one, 300, one, None) == -1 and "partials" in L.last_error()
    assert lib.sp_optim_step_flat(3, one, one, one, None, 10, one, None, 1.0, one, 8, None, None) == -1       # clipping needs the norm scalar


@pytest.mark.parametrize("kind", optim_ref.KINDS)
@pytest.mark.parametrize("clip", [False, True])
def test_reference_rules_equal_torch_in_float64(kind, clip):
    """4 steps of tests/optim_ref.py against torch.optim in float64: two tensors (one global norm), grad_scale 0.25, lr changed
    between steps 2 and 3.  Both compute the same expressions up to association: 1e-12 relative is a few hundred float64 roundings."""
    gen = torch.Generator().manual_seed(3)
    shapes = ((7, 3), (5,))
    p0 = [torch.randn(s, generator=gen, dtype=torch.float64) for s in shapes]
    grads = [[torch.randn(s, generator=gen, dtype=torch.float64) * (3.0 if i == 0 else 0.2) for i, s in enumerate(shapes)] for _ in range(4)]
    gs, lr, wd, betas, mom = 0.25, 1e-2, 1e-2, (0.9, 0.99), 0.9
    max_norm = 0.5 * min(optim_ref.grad_norm(g, gs) for g in grads) if clip else None
    tp = [torch.nn.Parameter(p.clone()) for p in p0]
    topt = {"adam": lambda: torch.optim.Adam(tp, lr=lr, betas=betas, weight_decay=wd),
            "adamw": lambda: torch.optim.AdamW(tp, lr=lr, betas=betas, weight_decay=wd),
            "sgd": lambda: torch.optim.SGD(tp, lr=lr, momentum=mom, weight_decay=wd),
            "nesterov": lambda: torch.optim.SGD(tp, lr=lr, momentum=mom, weight_decay=wd, nesterov=True)}[kind]()
    ref = optim_ref.RefOptimizer(kind, [p.clone() for p in p0], lr, betas=betas, weight_decay=wd, momentum=mom, grad_scale=gs,
                                 max_grad_norm=max_norm)
    for i, g in enumerate(grads):
        if i == 2:
            topt.param_groups[0]["lr"] = ref.hyper["lr"] = 3e-3
        for p, gi in zip(tp, g):
            p.grad = gi * gs
        if clip:
            norm = torch.nn.utils.clip_grad_norm_(tp, max_norm)
            assert float(norm) > max_norm
        topt.step()
        ref.step(g)
        if clip:
            assert abs(ref.last_norm - float(norm)) <= 1e-12 * float(norm)
    for p, q in zip(tp, ref.params):
        assert float((p.detach() - q).abs().max()) <= 1e-12 * float(q.abs().max())
    moved = max(float((q - p).abs().max()) for p, q in zip(p0, ref.params))
    assert moved > 1e-3
