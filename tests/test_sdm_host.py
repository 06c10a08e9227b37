"""The signed-distance-map baseline (reference test_sdm_resampling.py) on the host: the drop-in CLI module, the time
normalisation, the planning call against the recorded extents, the argument checks of the C entry points, and the fixture's
own precondition for the sign-mask comparison."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import stroke_prediction_amd  # noqa: F401
from stroke_prediction_amd.runtime import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLD)
import make_golden_sdm as G  # noqa: E402

CLI = os.path.join(ROOT, "stroke-prediction_amd", "test_sdm_resampling.py")
FX = dict(np.load(os.path.join(GOLD, "sdm.npz")))
CASES = [("bin128_d4", True), ("bin128_d28", True), ("odd", True), ("odd", False), ("artificial", True), ("artificial", False),
         ("prob", False)]


def _cli():
    spec = importlib.util.spec_from_file_location("sdm_cli_under_test", CLI)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_imports_without_gpu_and_parses_the_reference_command_line(capsys):
    mod = _cli()
    for name in ("sdm_interpolate_numpy", "get_normalized_time", "infer"):
        assert callable(getattr(mod, name)), name
    assert not [n for n in vars(mod) if n.startswith("test_")]
    assert capsys.readouterr().out == ""              # importing prints nothing and runs nothing
    from common import util
    a = util.get_args_sdm(["x.model", "--fold", "22", "--downsample", "0", "--groundtruth", "1"])
    assert a.unet == "x.model" and a.fold == [22] and a.downsample == 0 and a.groundtruth == 1 and a.visualinspection == 0


def test_time_normalisation_matches_the_reference():
    mod = _cli()
    batch = {"clinical": torch.from_numpy(FX["time/clinical"])}
    to_to_ta, norm = mod.get_normalized_time(batch, 10)
    ttt = mod.time_to_treatment(batch, norm)
    for got, key in ((to_to_ta, "time/to_to_ta"), (norm, "time/normalization"), (ttt, "time/time_to_treatment")):
        ref = FX[key]
        assert got.dtype == torch.float32 and tuple(got.shape) == ref.shape, key
        ulp = np.spacing(np.abs(ref).astype(np.float32))
        assert np.all(np.abs(got.numpy() - ref) <= ulp), key


def _stored_shape(case, setting, field):
    return G.decode(FX, "%s/%s/%s" % (case, setting, field)).shape


@pytest.mark.parametrize("case,resample", CASES)
def test_planning_extents_equal_the_recorded_shapes(case, resample):
    from stroke_prediction_amd.common import sdm
    D, H, W = (int(v) for v in FX[case + "/shape"])
    setting = "resample" if resample else "full"
    lat, rec, ws = sdm.plan(D, H, W, 12, resample, 1)
    assert lat == _stored_shape(case, setting, "latent_core") == _stored_shape(case, setting, "latent_intp/t0")
    if case != "bin128_d28":
        assert rec == _stored_shape(case, setting, "recon_core") == _stored_shape(case, setting, "recon_penu")
    assert ws >= 2 * 4 * 4 * D * H * W
    lat32, rec32, ws32 = sdm.plan(D, H, W, 12, resample, 32)
    assert (lat32, rec32) == (lat, rec) and ws32 >= ws


def test_entry_points_refuse_null_arguments_without_a_device():
    lib = L.load()
    i3 = (C.c_int32 * 3)(4, 8, 8)
    f3 = (C.c_double * 3)(1.0, 0.5, 0.5)
    out3 = (C.c_int32 * 6)()
    wsb = C.c_int64()
    checks = {
        "sp_sdm_plan": lambda: lib.sp_sdm_plan(4, 8, 8, 12.0, 1, 1, None, None),
        "sp_sdm_signed_fields": lambda: lib.sp_sdm_signed_fields(None, None, 4, 8, 8, 0.5, 3, None, None, None, None, 0, None),
        "sp_sdm_zoom_plan": lambda: lib.sp_sdm_zoom_plan(3, None, None, 1, None, None),
        "sp_sdm_zoom": lambda: lib.sp_sdm_zoom(None, 0, None, 0, 1, 3, None, None, None, None, None, 0, None),
        "sp_sdm_blend": lambda: lib.sp_sdm_blend(None, None, None, 0, 1, 10, None, None, None, None),
    }
    for name, call in checks.items():
        assert call() == -1, name
        assert name in L.last_error(), (name, L.last_error())
    # and the planning calls answer on the host
    assert lib.sp_sdm_plan(4, 2, 2, 12.0, 1, 1, out3, C.byref(wsb)) == -1 and "sp_sdm_plan" in L.last_error()   # 2 / 12 -> 0
    assert lib.sp_sdm_plan(4, 8, 8, 12.0, 1, 1, out3, C.byref(wsb)) == 0 and tuple(out3) == (4, 1, 1, 4, 10, 10)
    assert lib.sp_sdm_zoom_plan(3, i3, f3, 1, out3, C.byref(wsb)) == 0 and tuple(out3[:3]) == (4, 4, 4)


@pytest.mark.parametrize("case,resample", CASES)
def test_fixture_precondition_near_zero_cap(case, resample):
    """at most 0.1 % of each stored field within 1e-8 of 0 without being exactly 0 (the voxels the mask comparison leaves out)"""
    setting = "resample" if resample else "full"
    keys = sorted({k.rsplit(":", 1)[0] for k in FX if k.startswith("%s/%s/" % (case, setting)) and k.endswith((":q", ":sq"))})
    assert keys
    for k in keys:
        x = G.decode(FX, k)
        assert float(G.near_zero(x).mean()) <= G.CAP, k
