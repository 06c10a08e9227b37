"""The training criteria (``--criterion {dice,bce,dicebce}``) as far as a machine without a GPU sees them: the flag on every
training parser, ``metrics.make_criterion``, the refusal of host tensors, the C ABI and the accumulator pitch."""
import os
import re

import pytest
import torch

import stroke_prediction_amd  # noqa: F401
from stroke_prediction_amd.runtime import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parsers():
    from common import util
    return ((util.get_args_unet_training, ["/tmp/unet.model"]), (util.get_args_shape_training, []),
            (util.get_args_step_training, ["/tmp/cae.model"]), (util.get_args_shape_prediction_training, ["/tmp/cae.model"]))


def test_parsers_take_criterion(capsys):
    for parse, pos in _parsers():
        assert parse(pos).criterion == "dice"
        for name in ("dice", "bce", "dicebce"):
            assert parse(pos + ["--criterion", name]).criterion == name
        with pytest.raises(SystemExit):
            parse(pos + ["--criterion", "focal"])
        assert "invalid choice" in capsys.readouterr().err


def test_training_scripts_pass_the_flag_on():
    pkg = os.path.join(ROOT, "stroke-prediction_amd")
    for script in ("train_unet_segmentation.py", "train_shape_reconstruction.py", "train_shape_prediction.py",
                   "train_interpolationstep_after_reconstruction.py", "train_shape_reconstruction_with_ctp.py"):
        with open(os.path.join(pkg, script)) as f:
            text = f.read()
        assert "metrics.make_criterion(args.criterion)" in text and "metrics.BatchDiceLoss(" not in text, script


def test_make_criterion(capsys):
    from common import metrics
    dice, bce, both = (metrics.make_criterion(n) for n in ("dice", "bce", "dicebce"))
    assert type(dice) is metrics.BatchDiceLoss and list(dice._label_weights) == [1.0]
    assert type(bce) is metrics.BCELoss and bce._label_weights is None
    assert bce.weights(1) == (1.0,) and bce.weights(4) == (0.25,) * 4
    assert type(both) is metrics.DiceBCELoss and list(both._label_weights) == [1.0] and both._bce_weight == 1.0
    assert both._epsilon == dice._epsilon == 1e-7
    for bad in ("focal", "", None, "Dice"):
        with pytest.raises(ValueError):
            metrics.make_criterion(bad)


def test_criteria_refuse_host_tensors():
    from common import metrics
    o = torch.rand(2, 2, 3, 4, 5)
    t = (torch.rand(2, 2, 3, 4, 5) > 0.5).float()
    for crit in (metrics.BCELoss(), metrics.BCELoss([0.5, 0.5]), metrics.DiceBCELoss([0.3, 0.7], 0.5)):
        with pytest.raises(RuntimeError, match="runs on the GPU"):
            crit(o, t)


def test_binding_declares_the_entry_points():
    i32, i64, f32, f64, vp = L.i32, L.i64, L.f32, L.f64, L.vp
    strided = [vp, i64, vp, i64]
    assert L.SIGS["sp_vloss_sums"] == (strided + [i32, i32, i64, i32, vp, vp], i32)
    assert L.SIGS["sp_vloss_finalize_clear"] == ([vp, vp, vp, f64, f64, i32, vp, vp, vp], i32)
    assert L.SIGS["sp_vloss_bwd"] == (strided + [vp, vp, i32, i32, i64, vp, vp], i32)
    # the argument lists of sp_cae_loss_fwd / _bwd, `float dice_weight` -> (float dice_weight, float bce_weight, int32_t terms)
    fwd = list(L.SIGS["sp_cae_loss_fwd"][0])
    k = fwd.index(f32)
    assert L.SIGS["sp_cae_loss_crit_fwd"] == (fwd[:k] + [f32, f32, i32] + fwd[k + 1:], i32)
    assert L.SIGS["sp_cae_loss_crit_bwd"] == L.SIGS["sp_cae_loss_bwd"]
    assert (L.SP_VLOSS_DICE, L.SP_VLOSS_BCE) == (1, 2)


def test_vloss_pitch():
    assert [L.SP_VLOSS_PITCH(c) for c in (1, 4, 5)] == [16, 16, 32]
    # the header's macro is the same expression
    with open(L.HEADER) as f:
        m = re.search(r"#define SP_VLOSS_PITCH\(C\) (.*)", f.read())
    for c in (1, 4, 5, 8, 9):
        assert eval(m.group(1).replace("/", "//"), {"C": c}) == L.SP_VLOSS_PITCH(c) == (4 * c + 15) // 16 * 16
