"""The boundary (signed-distance) criteria (``--criterion {boundary,diceboundary}``) as far as a machine without a GPU sees them: the
factory, the flags on every parser, the C ABI, the refusal of host tensors, the routes the new classes do not take, the weight's
schedule (the Python value; the device copy is made on first use on a GPU) and the oracle helper against a brute-force distance."""
import os
import types

import numpy as np
import pytest
import torch

import stroke_prediction_amd  # noqa: F401
from stroke_prediction_amd.runtime import lib as L

import boundary_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parsers():
    from common import util
    return ((util.get_args_unet_training, ["/tmp/unet.model"]), (util.get_args_shape_training, []),
            (util.get_args_step_training, ["/tmp/cae.model"]), (util.get_args_shape_prediction_training, ["/tmp/cae.model"]),
            (util.get_args_sdm, ["/tmp/unet.model"]))


def test_make_criterion_boundary(capsys):
    from common import metrics
    bnd, both = metrics.make_criterion("boundary"), metrics.make_criterion("diceboundary")
    assert type(bnd) is metrics.BoundaryLoss and bnd._label_weights is None and bnd._dim == 1
    assert bnd.weights(1) == (1.0,) and bnd.weights(4) == (0.25,) * 4 and bnd.boundary_weight() == 1.0
    assert type(both) is metrics.DiceBoundaryLoss and list(both._label_weights) == [1.0] and both._dim == 1
    assert both.boundary_weight() == 0.01 and both._epsilon == 1e-7
    assert metrics.BoundaryLoss([0.3, 0.7], weight=0.5).weights(2) == (0.3, 0.7)
    # the three criteria from before are what they were
    assert type(metrics.make_criterion("dice")) is metrics.BatchDiceLoss
    assert type(metrics.make_criterion("bce")) is metrics.BCELoss
    assert type(metrics.make_criterion("dicebce")) is metrics.DiceBCELoss
    for bad in ("focal", "", None, "Dice", "Boundary"):
        with pytest.raises(ValueError) as e:
            metrics.make_criterion(bad)
        for name in ("dice", "bce", "dicebce", "boundary", "diceboundary"):
            assert name in str(e.value)


def test_parsers_take_the_boundary_flags(capsys):
    for parse, pos in _parsers():
        ns = parse(pos)
        assert ns.criterion == "dice" and ns.boundaryweight == 0.01 and ns.boundaryramp == 0.0
        for name in ("boundary", "diceboundary"):
            assert parse(pos + ["--criterion", name]).criterion == name
        ns = parse(pos + ["--criterion", "diceboundary", "--boundaryweight", "0.05", "--boundaryramp", "0.01"])
        assert (ns.boundaryweight, ns.boundaryramp) == (0.05, 0.01)
        with pytest.raises(SystemExit):
            parse(pos + ["--criterion", "focal"])
        assert "invalid choice" in capsys.readouterr().err


def test_training_scripts_configure_the_criterion():
    pkg = os.path.join(ROOT, "stroke-prediction_amd")
    for script in ("train_unet_segmentation.py", "train_shape_reconstruction.py", "train_shape_prediction.py",
                   "train_interpolationstep_after_reconstruction.py", "train_shape_reconstruction_with_ctp.py"):
        with open(os.path.join(pkg, script)) as f:
            lines = f.read().split("\n")
        k, = [i for i, line in enumerate(lines) if "metrics.make_criterion(args.criterion)" in line]
        assert "metrics.configure_criterion(criterion, args)" in lines[k + 1], script


def test_configure_criterion():
    from common import metrics
    args = types.SimpleNamespace(boundaryweight=0.05, boundaryramp=0.02)
    for name in ("dice", "bce", "dicebce"):
        crit = metrics.make_criterion(name)
        before = dict(vars(crit))
        assert metrics.configure_criterion(crit, args) is crit and vars(crit) == before and not hasattr(crit, "adapt")
    for name in ("boundary", "diceboundary"):
        crit = metrics.configure_criterion(metrics.make_criterion(name), args)
        assert crit.boundary_weight() == 0.05
        crit.adapt(3)
        assert crit.boundary_weight() == pytest.approx(0.05 + 0.02 * 3, abs=1e-15)


def test_adapt_follows_the_ramp_and_the_cap():
    from common import metrics
    crit = metrics.DiceBoundaryLoss([1.0], boundary_weight=0.01)
    for epoch in (0, 5, 200):
        crit.adapt(epoch)
        assert crit.boundary_weight() == 0.01          # no ramp: the weight stays
    crit.set_boundary_schedule(0.01, 0.01)            # the paper's schedule
    for epoch in (0, 1, 7, 98, 99, 100, 250):
        crit.adapt(epoch)
        assert crit.boundary_weight() == min(1.0, 0.01 + 0.01 * epoch), epoch
    assert crit.boundary_weight() == 1.0
    crit.adapt(0)                                      # from the start value, not from the last one
    assert crit.boundary_weight() == 0.01
    crit.set_boundary_weight(0.5)
    assert crit.boundary_weight() == 0.5
    bnd = metrics.BoundaryLoss(weight=0.25)
    bnd.adapt(10)
    assert bnd.boundary_weight() == 0.25


def test_learner_hook_calls_adapt_when_there_is_one():
    from learner.Learner import Learner
    seen = []
    with_adapt = types.SimpleNamespace(_criterion=types.SimpleNamespace(adapt=seen.append))
    Learner.adapt_criterion(with_adapt, 7)
    assert seen == [7]
    Learner.adapt_criterion(types.SimpleNamespace(_criterion=object()), 3)       # the criteria from before: nothing happens
    Learner.adapt_criterion(types.SimpleNamespace(), 3)
    assert seen == [7]


def test_boundary_criteria_refuse_host_tensors():
    from common import metrics
    o = torch.rand(2, 2, 3, 4, 5)
    t = (torch.rand(2, 2, 3, 4, 5) > 0.5).float()
    for crit in (metrics.BoundaryLoss(), metrics.BoundaryLoss([0.5, 0.5]), metrics.DiceBoundaryLoss([0.3, 0.7], 0.5)):
        with pytest.raises(RuntimeError, match="runs on the GPU"):
            crit(o, t)
    with pytest.raises(RuntimeError, match="runs on the GPU"):
        metrics.signed_distance_batch(t)


def test_fused_cae_routes_do_not_take_the_boundary_criteria():
    from common import metrics
    for crit in (metrics.BoundaryLoss(), metrics.BoundaryLoss([1.0]), metrics.DiceBoundaryLoss([1.0]), metrics.DiceBoundaryLoss([0.3, 0.7])):
        assert metrics._single_label_terms(crit) is None
    assert metrics._single_label_boundary_terms(metrics.BoundaryLoss()) == (None, 1.0, 0.0)
    assert metrics._single_label_boundary_terms(metrics.DiceBoundaryLoss([0.8], 0.5)) == (0.8, 1.0, 1e-7)
    assert metrics._single_label_boundary_terms(metrics.DiceBoundaryLoss([0.3, 0.7])) is None
    for name in ("dice", "bce", "dicebce"):
        assert metrics._single_label_boundary_terms(metrics.make_criterion(name)) is None


def test_binding_declares_the_boundary_entry_points():
    i32, i64, f64, vp = L.i32, L.i64, L.f64, L.vp
    strided = [vp, i64, vp, i64]
    assert L.SIGS["sp_signed_distance_batch_workspace"] == ([i32] * 5 + [vp], i32)
    assert L.SIGS["sp_signed_distance_batch"] == ([vp, i64] + [i32] * 5 + [vp, vp, i64, vp], i32)
    assert L.SIGS["sp_bloss_sums"] == (strided + [vp, i32, i32, i64, i32, vp, vp], i32)
    assert L.SIGS["sp_bloss_finalize_clear"] == ([vp, vp, vp, vp, f64, f64, i32, vp, vp, vp], i32)
    assert L.SIGS["sp_bloss_bwd"] == (strided + [vp, vp, vp, i32, i32, i64, vp, vp], i32)
    assert [L.SP_BLOSS_PITCH(c) for c in (1, 4, 5)] == [16, 16, 32]
    assert "sp_boundary.hip" in L.SOURCES and os.path.exists(os.path.join(L.CSRC_DIR, "sp_boundary.hip"))
    # the entry points from before keep their signatures
    assert L.SIGS["sp_vloss_sums"] == (strided + [i32, i32, i64, i32, vp, vp], i32)
    assert L.SIGS["sp_vloss_finalize_clear"] == ([vp, vp, vp, f64, f64, i32, vp, vp, vp], i32)
    assert L.SIGS["sp_dice_sums"] == (strided + [i32, i32, i64, vp, vp], i32)


def test_workspace_and_extent_errors():
    """host-only entry point: the size, and the errors for extents the axis scan does not take"""
    import ctypes as C
    n = C.c_int64(0)
    L.call("sp_signed_distance_batch_workspace", 2, 3, 5, 7, 9, C.byref(n))
    assert n.value == 4 * 2 * 3 * 5 * 7 * 9 + 64 * 2 * 3
    for bad in ((1, 1, 4096, 4, 4), (1, 1, 4, 0, 4), (0, 1, 4, 4, 4), (70000, 1, 1, 1, 1)):
        with pytest.raises(RuntimeError, match="sp_signed_distance_batch_workspace"):
            L.call("sp_signed_distance_batch_workspace", *bad, C.byref(n))


def test_oracle_helper_against_brute_force():
    rng = np.random.RandomState(5)
    mask = rng.rand(3, 4, 5) > 0.6
    assert mask.any() and not mask.all()
    ref = R.brute_force_volume(mask)
    got = R.signed_distance_volume(mask)
    assert got.dtype == np.float64 and np.array_equal(got, ref)
    assert (got[mask] <= 0).all() and (got[~mask] >= 1).all()
    corner = np.zeros((3, 4, 5), dtype=bool)
    corner[0, 0, 0] = True
    got = R.signed_distance_volume(corner)
    assert np.array_equal(got, R.brute_force_volume(corner))
    assert got[0, 0, 0] == 0.0 and got[2, 3, 4] == np.sqrt(4 + 9 + 16)
    for degenerate in (np.zeros((3, 4, 5), dtype=bool), np.ones((3, 4, 5), dtype=bool)):
        assert not R.signed_distance_volume(degenerate).any() and not R.brute_force_volume(degenerate).any()
    t = torch.from_numpy(np.stack([mask, corner]).astype(np.float32)).view(2, 1, 3, 4, 5)
    batch = R.signed_distance_batch(t)
    assert batch.dtype == torch.float32 and batch.shape == t.shape
    assert np.array_equal(batch[0, 0].numpy(), ref.astype(np.float32))


def test_loss_oracle_is_the_literal_formula():
    g = torch.Generator().manual_seed(2)
    o = torch.rand(2, 2, 3, 4, 5, generator=g)
    t = (torch.rand(2, 2, 3, 4, 5, generator=g) > 0.6).float()
    phi = R.signed_distance_batch(t)
    sums, mag, loss, coef, grad = R.loss_oracle(o, t, phi, [0.3, 0.7], [0.5, 0.5], 0.2)
    o64, t64, p64 = o.double(), t.double(), phi.double()
    dims = (0, 2, 3, 4)
    dice = 1 - (torch.tensor([0.3, 0.7], dtype=torch.float64) * (2 * (o64 * t64).sum(dims) + R.EPS)
                / ((o64 * o64).sum(dims) + (t64 * t64).sum(dims) + R.EPS)).sum()
    literal = dice + 0.2 * (o64 * p64).mean()
    assert abs(loss - float(literal)) < 1e-14
    want = coef[:, 0].view(1, 2, 1, 1, 1) * t64 + coef[:, 1].view(1, 2, 1, 1, 1) * o64 + coef[:, 2].view(1, 2, 1, 1, 1) * p64
    torch.testing.assert_close(grad, want, rtol=1e-12, atol=1e-15)
    assert bool((mag >= sums[:, 3].abs()).all())
