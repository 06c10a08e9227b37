"""The class-imbalance criteria (``--criterion {tversky,focaltversky,focalbce,tverskyfocalbce}``) as far as a machine without a GPU
sees them: the factory and its defaults, the names and flags on every training parser, the constructors' checks, the refusal of host
tensors, the C ABI, ``configure_criterion``, the routes the classes take and the fp64 oracle against autograd."""
import types

import pytest
import torch

import stroke_prediction_amd  # noqa: F401
from stroke_prediction_amd.runtime import lib as L

import imbalance_ref as R

NAMES = ("tversky", "focaltversky", "focalbce", "tverskyfocalbce")
FLAGS = ("tverskyfp", "tverskyfn", "tverskygamma", "focalgamma", "focalalpha", "focalweight")
ALL_NAMES = ("dice", "bce", "dicebce", "boundary", "diceboundary") + NAMES


def _parsers():
    from common import util
    return ((util.get_args_unet_training, ["/tmp/unet.model"]), (util.get_args_shape_training, []),
            (util.get_args_step_training, ["/tmp/cae.model"]), (util.get_args_shape_prediction_training, ["/tmp/cae.model"]),
            (util.get_args_sdm, ["/tmp/unet.model"]))


def test_parsers_take_the_names_and_the_flags(capsys):
    for parse, pos in _parsers():
        ns = parse(pos)
        assert ns.criterion == "dice"
        assert all(getattr(ns, flag) is None for flag in FLAGS)
        for name in NAMES:
            assert parse(pos + ["--criterion", name]).criterion == name
        ns = parse(pos + ["--criterion", "tverskyfocalbce", "--tverskyfp", "0.2", "--tverskyfn", "0.8", "--tverskygamma", "1.5",
                          "--focalgamma", "3", "--focalalpha", "0.4", "--focalweight", "0.5"])
        assert [getattr(ns, flag) for flag in FLAGS] == [0.2, 0.8, 1.5, 3.0, 0.4, 0.5]
        with pytest.raises(SystemExit):
            parse(pos + ["--criterion", "focal"])
        assert "invalid choice" in capsys.readouterr().err


def test_make_criterion_classes_and_defaults():
    from common import metrics
    tv, ftv = metrics.make_criterion("tversky"), metrics.make_criterion("focaltversky")
    for crit, gamma in ((tv, 1.0), (ftv, 4.0 / 3.0)):
        assert type(crit) is metrics.TverskyLoss and list(crit._label_weights) == [1.0] and crit._dim == 1
        assert (crit._fp_weight, crit._fn_weight, crit._gamma, crit._epsilon) == (0.3, 0.7, gamma, 1e-7)
    fb = metrics.make_criterion("focalbce")
    assert type(fb) is metrics.FocalBCELoss and fb._label_weights is None and fb._dim == 1
    assert (fb._gamma, fb._alpha) == (2.0, 0.25) and fb.weights(1) == (1.0,) and fb.weights(4) == (0.25,) * 4
    assert metrics.FocalBCELoss([0.3, 0.7]).weights(2) == (0.3, 0.7)
    both = metrics.make_criterion("tverskyfocalbce")
    assert type(both) is metrics.TverskyFocalBCELoss and list(both._label_weights) == [1.0] and both._dim == 1
    assert (both._focal_weight, both._fp_weight, both._fn_weight, both._tversky_gamma, both._focal_gamma, both._focal_alpha, both._epsilon) \
        == (1.0, 0.3, 0.7, 1.0, 2.0, 0.25, 1e-7)
    # the five criteria from before are what they were
    for name, cls in (("dice", metrics.BatchDiceLoss), ("bce", metrics.BCELoss), ("dicebce", metrics.DiceBCELoss),
                      ("boundary", metrics.BoundaryLoss), ("diceboundary", metrics.DiceBoundaryLoss)):
        assert type(metrics.make_criterion(name)) is cls


def test_make_criterion_error_lists_nine_names():
    from common import metrics
    for bad in ("focal", "", None, "Tversky", "focal_tversky"):
        with pytest.raises(ValueError) as e:
            metrics.make_criterion(bad)
        listed = str(e.value).split("one of ")[1].split(", ")
        assert sorted(listed) == sorted(ALL_NAMES) and len(listed) == 9


def test_constructors_check_their_scalars():
    from common import metrics
    for kw in (dict(fp_weight=-0.1), dict(fn_weight=-1e-9), dict(gamma=0.99), dict(gamma=0.0), dict(gamma=float("nan"))):
        with pytest.raises(ValueError):
            metrics.TverskyLoss([1.0], **kw)
    for kw in (dict(gamma=0.5), dict(gamma=-1.0), dict(gamma=0.999), dict(alpha=-0.01), dict(alpha=1.01), dict(alpha=float("nan"))):
        with pytest.raises(ValueError):
            metrics.FocalBCELoss(**kw)
    for kw in (dict(fp_weight=-0.1), dict(fn_weight=-0.1), dict(tversky_gamma=0.5), dict(focal_gamma=0.5), dict(focal_alpha=2.0)):
        with pytest.raises(ValueError):
            metrics.TverskyFocalBCELoss([1.0], **kw)
    # the edges are legal
    metrics.TverskyLoss([1.0], fp_weight=0.0, fn_weight=0.0, gamma=1.0)
    metrics.FocalBCELoss(gamma=0.0, alpha=0.0)
    metrics.FocalBCELoss(gamma=1.0, alpha=1.0)
    metrics.TverskyFocalBCELoss([1.0], focal_gamma=0.0, tversky_gamma=4.0 / 3.0)


def test_criteria_refuse_host_tensors():
    from common import metrics
    o = torch.rand(2, 2, 3, 4, 5)
    t = (torch.rand(2, 2, 3, 4, 5) > 0.5).float()
    for crit in (metrics.TverskyLoss([0.5, 0.5]), metrics.TverskyLoss([0.5, 0.5], gamma=4.0 / 3.0), metrics.FocalBCELoss(),
                 metrics.FocalBCELoss([0.5, 0.5]), metrics.TverskyFocalBCELoss([0.3, 0.7], 0.5)):
        with pytest.raises(RuntimeError, match="runs on the GPU"):
            crit(o, t)


def test_binding_declares_the_tloss_entry_points():
    i32, i64, f32, f64, vp = L.i32, L.i64, L.f32, L.f64, L.vp
    strided = [vp, i64, vp, i64]
    assert L.SIGS["sp_tloss_sums"] == (strided + [i32, i32, i64, i32, f32, f32, vp, vp], i32)
    assert L.SIGS["sp_tloss_finalize_clear"] == ([vp, vp, vp, f64, f64, f64, f64, f64, i32, vp, vp, vp], i32)
    assert L.SIGS["sp_tloss_bwd"] == (strided + [vp, vp, f32, f32, i32, i32, i64, vp, vp], i32)
    assert (L.CONSTS["SP_TLOSS_TVERSKY"], L.CONSTS["SP_TLOSS_FOCAL"]) == (1, 2) == (L.SP_TLOSS_TVERSKY, L.SP_TLOSS_FOCAL)
    assert [L.SP_TLOSS_PITCH(c) for c in (1, 2, 4, 5, 9)] == [L.SP_VLOSS_PITCH(c) for c in (1, 2, 4, 5, 9)] == [16, 16, 16, 32, 48]
    # the entry points from before keep their signatures
    assert L.SIGS["sp_vloss_sums"] == (strided + [i32, i32, i64, i32, vp, vp], i32)
    assert L.SIGS["sp_bloss_bwd"] == (strided + [vp, vp, vp, i32, i32, i64, vp, vp], i32)
    for name in ("sp_tloss_sums", "sp_tloss_finalize_clear", "sp_tloss_bwd"):
        assert hasattr(L.load(), name)


def test_entry_points_refuse_bad_scalars():
    """the launchers check their arguments before they touch a pointer: host-only"""
    buf = (L.C.c_double * 256)()
    ptr = L.C.addressof(buf)
    for terms, gamma, alpha in ((0, 2.0, 0.25), (4, 2.0, 0.25), (2, 0.5, 0.25), (3, -1.0, 0.25), (2, 2.0, 1.5), (2, 2.0, -0.1)):
        with pytest.raises(RuntimeError, match="sp_tloss_sums"):
            L.call("sp_tloss_sums", ptr, 8, ptr, 8, 1, 1, 8, terms, gamma, alpha, ptr, None)
    for fp, fn, gamma in ((-0.1, 0.7, 1.0), (0.3, -0.7, 1.0), (0.3, 0.7, 0.9)):
        with pytest.raises(RuntimeError, match="sp_tloss_finalize_clear"):
            L.call("sp_tloss_finalize_clear", ptr, ptr, None, fp, fn, gamma, 1e-7, 8.0, 1, ptr, ptr, None)
    with pytest.raises(RuntimeError, match="sp_tloss_finalize_clear"):
        L.call("sp_tloss_finalize_clear", ptr, None, None, 0.3, 0.7, 1.0, 1e-7, 8.0, 1, ptr, ptr, None)      # no term at all
    with pytest.raises(RuntimeError, match="sp_tloss_bwd"):
        L.call("sp_tloss_bwd", ptr, 8, ptr, 8, ptr, None, 0.5, 0.25, 1, 1, 8, ptr, None)


def test_configure_criterion():
    from common import metrics
    args = types.SimpleNamespace(boundaryweight=0.05, boundaryramp=0.02, tverskyfp=0.2, tverskyfn=0.8, tverskygamma=1.5, focalgamma=3.0,
                                 focalalpha=0.4, focalweight=0.5)
    dice = metrics.BatchDiceLoss([1.0])
    before = dict(vars(dice))
    assert metrics.configure_criterion(dice, args) is dice and vars(dice) == before
    for name in ("bce", "dicebce"):
        crit = metrics.make_criterion(name)
        before = dict(vars(crit))
        assert metrics.configure_criterion(crit, args) is crit and vars(crit) == before
    for name in ("tversky", "focaltversky"):
        crit = metrics.make_criterion(name)
        assert metrics.configure_criterion(crit, args) is crit
        assert (crit._fp_weight, crit._fn_weight, crit._gamma) == (0.2, 0.8, 1.5)
        assert crit.extra()[:3] == (0.2, 0.8, 1.5)
    crit = metrics.configure_criterion(metrics.make_criterion("focalbce"), args)
    assert (crit._gamma, crit._alpha) == (3.0, 0.4) and crit.extra()[3:] == (3.0, 0.4)
    crit = metrics.configure_criterion(metrics.make_criterion("tverskyfocalbce"), args)
    assert crit.extra() == (0.2, 0.8, 1.5, 3.0, 0.4) and crit._focal_weight == 0.5
    # None = the criterion's own value: focaltversky keeps 4/3; a namespace without the flags changes nothing
    none = types.SimpleNamespace(**{flag: None for flag in FLAGS})
    for ns in (none, types.SimpleNamespace()):
        crit = metrics.configure_criterion(metrics.make_criterion("focaltversky"), ns)
        assert (crit._fp_weight, crit._fn_weight, crit._gamma) == (0.3, 0.7, 4.0 / 3.0)
    # a flag the constructor would refuse is refused here too
    with pytest.raises(ValueError):
        metrics.configure_criterion(metrics.make_criterion("focalbce"), types.SimpleNamespace(focalgamma=0.5))
    with pytest.raises(ValueError):
        metrics.configure_criterion(metrics.make_criterion("tversky"), types.SimpleNamespace(tverskyfp=-1.0))


def test_routes_of_the_new_criteria():
    """the fused CAE route does not take them (the learners compose them literally); the stacked route does, for one label class"""
    from common import metrics
    for name in NAMES:
        crit = metrics.make_criterion(name)
        assert metrics._single_label_terms(crit) is None and metrics._single_label_boundary_terms(crit) is None
    assert metrics._single_label_imbalance_terms(metrics.TverskyLoss([0.8], 0.4, 0.6, 1.5)) == (0.8, None, 1e-7, (0.4, 0.6, 1.5, 2.0, 0.25))
    assert metrics._single_label_imbalance_terms(metrics.FocalBCELoss(None, 3.0, 0.4)) == (None, 1.0, 0.0, (0.0, 0.0, 1.0, 3.0, 0.4))
    assert metrics._single_label_imbalance_terms(metrics.FocalBCELoss([0.6])) == (None, 0.6, 0.0, (0.0, 0.0, 1.0, 2.0, 0.25))
    assert metrics._single_label_imbalance_terms(metrics.TverskyFocalBCELoss([0.8], 0.5)) == (0.8, 0.5, 1e-7, (0.3, 0.7, 1.0, 2.0, 0.25))
    for crit in (metrics.TverskyLoss([0.3, 0.7]), metrics.FocalBCELoss([0.3, 0.7]), metrics.TverskyFocalBCELoss([0.3, 0.7])):
        assert metrics._single_label_imbalance_terms(crit) is None
    for name in ("dice", "bce", "dicebce", "boundary", "diceboundary"):
        assert metrics._single_label_imbalance_terms(metrics.make_criterion(name)) is None
    fam = metrics._FAMILIES["tloss"]
    assert (fam.sums, fam.finalize, fam.bwd, fam.ncoef, fam.fourth, fam.phi) == ("sp_tloss_sums", "sp_tloss_finalize_clear", "sp_tloss_bwd", 3, True, False)
    extra = (0.3, 0.7, 1.5, 2.5, 0.4)
    assert (fam.sums_scalars(extra), fam.finalize_scalars(extra), fam.bwd_scalars(extra)) == ((2.5, 0.4), (0.3, 0.7, 1.5), (2.5, 0.4))
    assert fam.select(L, (1.0,), None) == (1,) and fam.select(L, None, (1.0,)) == (2,) and fam.select(L, (1.0,), (1.0,)) == (3,)
    for name in ("dice", "vloss", "bloss"):      # the families from before pass no scalars
        fam = metrics._FAMILIES[name]
        assert fam.sums_scalars(None) == fam.finalize_scalars(None) == fam.bwd_scalars(None) == ()


def _oracle_inputs():
    g = torch.Generator().manual_seed(4)
    o = torch.rand(2, 2, 3, 4, 5, generator=g) * 0.98 + 0.01      # away from saturation: autograd is finite
    t = (torch.rand(2, 2, 3, 4, 5, generator=g) > 0.6).float()
    return o, t


@pytest.mark.parametrize("tg,fg,fp,fn", [(1.0, 2.0, 0.3, 0.7), (4.0 / 3.0, 0.0, 0.5, 0.5), (1.5, 1.0, 1.0, 0.0), (1.0, 2.5, 0.3, 0.7)])
def test_oracle_against_autograd(tg, fg, fp, fn):
    """the closed-form coefficients give autograd's Tversky gradient, the analytic fl' autograd's focal gradient"""
    o, t = _oracle_inputs()
    wt, wf = [0.3, 0.7], [0.6, 0.4]
    sums, loss, coef, grad = R.oracle(o, t, wt, wf, fp, fn, tg, fg, 0.3, upstream=0.5)
    o64, t64 = o.double().requires_grad_(True), t.double()
    count = o.numel() // 2
    literal = R.tversky_loss(o64, t64, wt, fp, fn, tg) + (torch.tensor(wf, dtype=torch.float64)
                                                           * R.focal_term(o64, t64, fg, 0.3).sum((0, 2, 3, 4)) / count).sum()
    assert abs(loss - float(literal.detach())) < 1e-13
    want, = torch.autograd.grad(literal * 0.5, o64)
    torch.testing.assert_close(grad, want, rtol=1e-10, atol=1e-15)
    v = (1, 2, 1, 1, 1)
    closed = 0.5 * (coef[:, 0].view(v) * t64 + coef[:, 1].view(v) + coef[:, 2].view(v) * R.focal_grad(o64.detach(), t64, fg, 0.3))
    torch.testing.assert_close(closed, want, rtol=1e-10, atol=1e-15)


def test_oracle_degenerate_points():
    """the planted outputs: finite values and gradients; the clamp's zero gradient on a perfect and on an empty channel"""
    o = torch.tensor([0.0, 0.0, 1.0, 1.0, 1e-30, 1e-30, 1.0 - 2.0 ** -24, 1.0 - 2.0 ** -24], dtype=torch.float64)
    t = torch.tensor([0.0, 1.0] * 4, dtype=torch.float64)
    for gamma in (0.0, 1.0, 2.0, 2.5):
        assert bool(torch.isfinite(R.focal_term(o, t, gamma, 0.25)).all()) and bool(torch.isfinite(R.focal_grad(o, t, gamma, 0.25)).all())
    assert float(R.focal_term(o, t, 2.0, 0.25)[1]) == 25.0 and float(R.focal_term(o, t, 2.0, 0.25)[2]) == 75.0      # alpha * 100, (1 - alpha) * 100
    perfect = (torch.rand(2, 1, 3, 4, 5) > 0.5).float()
    for o32, t32 in ((perfect, perfect), (torch.zeros(2, 1, 3, 4, 5), torch.zeros(2, 1, 3, 4, 5))):
        _, loss, coef, grad = R.oracle(o32, t32, [1.0], None, 0.3, 0.7, 4.0 / 3.0)
        assert loss == pytest.approx(1e-12 ** 0.75, rel=1e-12) and not coef.any() and not grad.any()
