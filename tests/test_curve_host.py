"""The evaluation CLIs and the time-to-treatment curve, host side (no GPU): the reference's import paths resolve, the C ABI
declares the batched measures, the curve's schedule is the reference's (tester/CaeReconstructionTesterCurve.py:18-42).  GPU
behaviour: tests/test_gpu_curve.py."""
import ctypes as C
import importlib
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "stroke-prediction_amd")

import stroke_prediction_amd  # noqa: E402,F401


def test_curve_tester_and_clis_import_under_the_reference_paths():
    from tester.CaeReconstructionTesterCurve import CaeReconstructionTesterCurve, curve_schedule  # noqa: F401
    from tester.CaeReconstructionTester import CaeReconstructionTester
    from common.inference.CaeInference import CaeInference
    from common import metrics
    assert issubclass(CaeReconstructionTesterCurve, CaeReconstructionTester)
    assert callable(getattr(CaeInference, "inference_curve")) and callable(metrics.binary_measures_many_torch)
    import inspect
    sig = inspect.signature(CaeReconstructionTesterCurve.__init__)
    assert list(sig.parameters)[1:] == ["dataloader", "path_model", "path_outputs_base", "normalization_hours_penumbra",
                                        "ta_to_tr_fixed_hours", "ta_to_tr_relative_steps"]
    assert sig.parameters["ta_to_tr_fixed_hours"].default == range(11)
    assert sig.parameters["ta_to_tr_relative_steps"].default == [0, 0.25, 0.5, 0.75, 1, 1.25, 1.5, 1.75, 2]
    assert list(inspect.signature(CaeReconstructionTesterCurve.infer_batch).parameters) == ["self", "batch", "step"]
    sys.path.insert(0, PKG)
    try:
        for name in ("test_shape_reconstruction", "test_shape_reconstruction_CurveAnalysis", "test_unet_segmentation"):
            assert os.path.isfile(os.path.join(PKG, name + ".py")), name
            mod = importlib.import_module(name)
            assert callable(mod.evaluate)
            assert not [n for n in dir(mod) if n.startswith("test")], "the CLI must define nothing pytest would collect"
        assert list(importlib.import_module("test_shape_reconstruction_CurveAnalysis").FIXED_HOURS) == list(range(6))
    finally:
        sys.path.remove(PKG)


def test_header_declares_the_batched_measures_and_the_binding_follows():
    from stroke_prediction_amd.runtime import lib as L
    with open(L.HEADER) as f:
        text = f.read()
    assert re.search(r"\bint\s+sp_binary_measures_many\s*\(", text)
    args, ret = L.SIGS["sp_binary_measures_many"]
    #                results stride T      reference thr  ndim   dims  ws    counts out   stream
    assert args == [L.vp, L.i64, L.i32, L.vp, L.f32, L.i32, L.vp, L.vp, L.vp, L.vp, L.vp] and ret is L.i32
    assert L.SIGS["sp_binary_measures_many_workspace"][0] == [L.i32, L.i64, L.vp]
    assert "sp_binary_measures_many" in L.EXPORTS


def test_workspace_formula_is_the_headers_and_monotone_in_T():
    from stroke_prediction_amd.runtime import lib as L
    from stroke_prediction_amd.common.metrics import measures_many_workspace_floats
    with open(L.HEADER) as f:
        text = f.read()
    assert "ws: 2 * (T + 1) * prod(dims) floats" in text
    nvox = 28 * 128 * 128
    sizes = [measures_many_workspace_floats(T, nvox) for T in range(1, 40)]
    assert sizes == [2 * (T + 1) * nvox for T in range(1, 40)]
    assert all(b > a for a, b in zip(sizes, sizes[1:]))
    n = C.c_int64(-1)
    assert L.load().sp_binary_measures_many_workspace(0, nvox, C.byref(n)) == -1 and "sp_binary_measures_many_workspace" in L.last_error()
    # argument checks of the launcher run before anything touches a device
    assert L.load().sp_binary_measures_many(None, 0, 1, None, 0.5, 3, None, None, None, None, None) == -1
    assert "sp_binary_measures_many" in L.last_error()


@pytest.mark.parametrize("fixed", [None, range(6)])
def test_curve_schedule_is_the_references(fixed):
    from tester.CaeReconstructionTesterCurve import CaeReconstructionTesterCurve, curve_schedule
    import inspect
    sig = inspect.signature(CaeReconstructionTesterCurve.__init__)
    ratios = sig.parameters["ta_to_tr_relative_steps"].default
    hours = sig.parameters["ta_to_tr_fixed_hours"].default if fixed is None else fixed
    to_to_ta, ta_to_tr, norm = 2.0, 1.5, 10
    pts = curve_schedule(to_to_ta, ta_to_tr, norm, hours, ratios)
    nf = len(hours)
    assert nf == (11 if fixed is None else 6) and len(pts) == 1 + nf + 9 + 11
    assert pts[0] == (None, '')
    assert [p[0] for p in pts[1:1 + nf]] == list(hours)
    assert [p[1] for p in pts[1:1 + nf]] == ['ta_to_tr fixed=' + str(h) for h in hours]
    rel = pts[1 + nf:1 + nf + 9]
    assert [p[0] for p in rel] == [r * 1.5 for r in ratios]
    assert [p[1] for p in rel] == ['ta_to_tr ratio=' + str(r) + '\t(' + str(r * 1.5) + ')' for r in ratios]
    assert rel[1][1] == 'ta_to_tr ratio=0.25\t(0.375)' and rel[4][1] == 'ta_to_tr ratio=1\t(1.5)'
    pen = pts[1 + nf + 9:]
    fr = [0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0]
    assert [p[0] for p in pen] == [f * 8.0 for f in fr]
    assert [p[1] for p in pen] == ['tr_to_penumbra=' + str(f) + '\t(' + str(f * 8.0) + ')' for f in fr]
    assert pen[5][1] == 'tr_to_penumbra=0.5\t(4.0)' and pen[10][1] == 'tr_to_penumbra=1.0\t(8.0)'


def test_inference_curve_refuses_batches_and_training_mode():
    import torch
    from common import data
    from common.inference.CaeInference import CaeInference
    from common.model.Cae3D import Cae3D, Enc3D, Dec3D
    ch = [1, 16, 24, 32, 100, 200, 1]
    inf = CaeInference(Cae3D(Enc3D(128, 28, ch, 5, 1.0), Dec3D(128, 28, ch, 5, 1.0)))
    batch = {data.KEY_GLOBAL: torch.ones(2, 5, 1, 1, 1), data.KEY_LABELS: torch.zeros(2, 3, 4, 8, 8)}
    with pytest.raises(ValueError, match="batch size 1"):
        inf.inference_curve(batch, [None, 1.0])
    batch = {data.KEY_GLOBAL: torch.ones(1, 5, 1, 1, 1), data.KEY_LABELS: torch.zeros(1, 3, 4, 8, 8)}
    with pytest.raises(RuntimeError, match="eval mode"):
        inf.inference_curve(batch, [None, 1.0])
    assert inf.inference_curve(batch, []) == []
