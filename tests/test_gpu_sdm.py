"""The signed-distance-map baseline (reference test_sdm_resampling.py) on the MI355X: every case of the reference fixture
(tests/golden/make_golden_sdm.py) through ``sdm_interpolate_numpy``, the stages at 28 x 128 x 128 against the scipy of this
machine, batched time values, streams and the single host read, degenerate inputs, and the drop-in CLI end to end.

Bounds (the issue's): full-resolution fields 1e-9 (exact integer squared distances, fp64 roots and blend: an fp32 root
anywhere would show as >= 1e-6); latents and resampled fields 1e-8 (magnitudes <= ~200, reordered fp64 sums cost ~1e-12);
the fixture's own encoding error is below 3e-11 (``qerr``).  Sign masks are identical wherever the reference field is not
within 1e-8 of 0 (exact zeros included)."""
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import stroke_prediction_amd  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLD)
import make_golden_sdm as G  # noqa: E402

pytestmark = pytest.mark.gpu
FX = dict(np.load(os.path.join(GOLD, "sdm.npz")))
CLI = os.path.join(ROOT, "stroke-prediction_amd", "test_sdm_resampling.py")
TOL_FULL, TOL_RES = 1e-9, 1e-8
CASES = [("bin128_d4", True), ("bin128_d28", True), ("odd", True), ("odd", False), ("artificial", True), ("artificial", False),
         ("prob", False)]


def _sdm():
    from stroke_prediction_amd.common import sdm
    return sdm


def _inputs(case):
    shape = tuple(int(v) for v in FX[case + "/shape"])
    return G.load_input(FX, case + "/in_core", shape), G.load_input(FX, case + "/in_penu", shape)


def _close(got, ref, tol, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    print("%-40s max|diff| %.3g (bound %g)" % (what, err, tol))
    assert err <= tol, (what, err)


def _same_sign_mask(got, ref, what):
    keep = ~G.near_zero(ref)
    for name, f in (("> 0", lambda x: x > 0), ("< 0", lambda x: x < 0)):
        bad = int((f(got) != f(ref))[keep].sum())
        assert bad == 0, (what, name, bad)


@pytest.mark.parametrize("case,resample", CASES)
def test_fixture_case_matches_the_reference(case, resample, capsys):
    sdm = _sdm()
    core, penu = _inputs(case)
    s = "%s/%s" % (case, "resample" if resample else "full")
    for i, t in enumerate(FX[case + "/t"]):
        out = sdm.sdm_interpolate_numpy(core[None, None], penu[None, None], float(t), resample=resample)
        printed = capsys.readouterr().out
        assert printed == str(FX[s + "/printed"]), (printed, str(FX[s + "/printed"]))
        r = dict(zip(G.FIELDS, out))
        assert all(v.dtype == np.float64 for v in out)
        with capsys.disabled():
            _close(r["latent_core"], G.decode(FX, s + "/latent_core"), TOL_RES, s + " latent_core")
            _close(r["latent_penu"], G.decode(FX, s + "/latent_penu"), TOL_RES, s + " latent_penu")
            _close(r["latent_intp"], G.decode(FX, "%s/latent_intp/t%d" % (s, i)), TOL_RES, "%s latent_intp t=%g" % (s, t))
            if case == "bin128_d28":
                continue
            tol = TOL_RES if resample else TOL_FULL
            rc, rp = G.decode(FX, s + "/recon_core"), G.decode(FX, s + "/recon_penu")
            key = "%s/recon_intp/t%d" % (s, i)
            ri = G.decode(FX, key) if key + ":q" in FX else (-rc if t == 0.0 else rp)   # recorded as exact identities at t = 0 / 1
            _close(r["recon_core"], rc, tol, s + " recon_core")
            _close(r["recon_penu"], rp, tol, s + " recon_penu")
            _close(r["recon_intp"], ri, tol, "%s recon_intp t=%g" % (s, t))
        _same_sign_mask(r["recon_intp"], ri, s + " intp")
        _same_sign_mask(r["recon_core"], rc, s + " core")
        _same_sign_mask(r["recon_penu"], rp, s + " penu")


def test_artificial_core_flag_and_cog():
    sdm = _sdm()
    core, penu = _inputs("artificial")
    dev = lambda a: torch.from_numpy(a).cuda()
    import io
    import contextlib
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        sdm.sdm_interpolate_torch(dev(core), dev(penu), 0.6, resample=False)
    ref = str(FX["artificial/full/printed"])
    assert buf.getvalue() == ref and ref.startswith(sdm.ARTIFICIAL_CORE_PREFIX)
    cog = [int(v) for v in re.findall(r"-?\d+", ref.split("core", 1)[1])]
    from scipy import ndimage
    assert cog == [int(v) for v in ndimage.center_of_mass(penu > 0.5)]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        sdm.sdm_interpolate_torch(dev(_inputs("odd")[0]), dev(_inputs("odd")[1]), 0.6)
    assert buf.getvalue() == ""


# ------------------------------------------------------------------------------------------------ stages against scipy
def _scipy():
    scipy = pytest.importorskip("scipy")
    if tuple(int(v) for v in re.findall(r"\d+", scipy.__version__)[:2]) < (1, 6):
        pytest.skip("scipy %s: mode 'constant' of ndimage.zoom differs before 1.6" % scipy.__version__)
    from scipy import ndimage
    return ndimage


def _d28():
    return G.nested(202, (28, 128, 128), (2.0, 6.0, 6.0))


def test_stage_signed_fields_against_scipy_edt():
    ndi = _scipy()
    sdm = _sdm()
    core, penu = _d28()
    out = sdm.sdm_interpolate_torch(torch.from_numpy(core).cuda(), torch.from_numpy(penu).cuda(), 0.5, resample=False)
    ref_penu = ndi.distance_transform_edt(penu > 0.5) - ndi.distance_transform_edt(penu < 0.5)
    ref_core = ndi.distance_transform_edt(1 - (core > 0.5)) - ndi.distance_transform_edt(core > 0.5)
    _close(out[2].cpu().numpy(), ref_penu, TOL_FULL, "edt penu 28x128x128")
    _close(out[0].cpu().numpy(), ref_core, TOL_FULL, "edt core 28x128x128")


def test_stage_zooms_against_scipy():
    ndi = _scipy()
    sdm = _sdm()
    core, penu = _d28()
    field = ndi.distance_transform_edt(penu > 0.5) - ndi.distance_transform_edt(penu < 0.5)
    x = torch.from_numpy(field).cuda()
    m = float(np.abs(field).max())
    lat = sdm.zoom_torch(x, (1, 1 / 12, 1 / 12)).cpu().numpy()
    lat_ref = ndi.zoom(field, (1, 1.0 / 12, 1.0 / 12))
    _close(lat, lat_ref, 1e-8 * m, "zoom (1, 1/12, 1/12)")
    up = sdm.zoom_torch(torch.from_numpy(lat_ref).cuda(), (1, 12, 12), crop=(None, (2, 130), (2, 130))).cpu().numpy()
    up_ref = ndi.zoom(lat_ref, (1, 12, 12))[:, 2:130, 2:130]
    _close(up, up_ref, 1e-8 * float(np.abs(lat_ref).max()), "zoom (1, 12, 12)[:, 2:130, 2:130]")
    ex_ref = ndi.zoom(field.transpose((2, 1, 0)), (2, 2, 1))
    ex = sdm.zoom_torch(x, (1, 2, 2)).cpu().numpy().transpose((2, 1, 0))
    _close(ex, ex_ref, 1e-8 * m, "zoom (2, 2, 1) of the transpose")
    ex2 = sdm.zoom_torch(torch.from_numpy(np.ascontiguousarray(field.transpose((2, 1, 0)))).cuda(), (2, 2, 1)).cpu().numpy()
    _close(ex2, ex_ref, 1e-8 * m, "zoom (2, 2, 1) contiguous")


def test_stage_int8_export_equals_scipy():
    ndi = _scipy()
    sdm = _sdm()
    core, penu = _d28()
    lesion = ((core + penu) / 2).astype(np.float32)        # 0, 0.5, 1: astype(int8) truncates 0.5 to 0
    ref = ndi.zoom(lesion.astype(np.int8).transpose((2, 1, 0)), zoom=(2, 2, 1))
    assert ref.dtype == np.int8
    got = sdm.zoom_torch(torch.from_numpy(lesion).cuda(), (1, 2, 2), out="i8", src_as_int8=True).cpu().numpy().transpose((2, 1, 0))
    assert got.dtype == np.int8 and got.shape == ref.shape == (256, 256, 28)
    assert np.array_equal(got, ref), int((got != ref).sum())
    got8 = sdm.zoom_torch(torch.from_numpy(penu.astype(np.int8)).cuda(), (1, 2, 2), out="i8").cpu().numpy().transpose((2, 1, 0))
    assert np.array_equal(got8, ndi.zoom(penu.astype(np.int8).transpose((2, 1, 0)), zoom=(2, 2, 1)))


# ------------------------------------------------------------------------------------------------ other behaviour
@pytest.mark.parametrize("resample", [True, False])
def test_batched_time_values_equal_single_calls(resample):
    sdm = _sdm()
    core, penu = (torch.from_numpy(a).cuda() for a in _d28())
    ts = np.random.RandomState(5).uniform(0, 1, 32)
    batched = sdm.sdm_interpolate_torch(core, penu, torch.from_numpy(ts), resample=resample)
    assert batched[1].shape[0] == 32 and batched[4].shape[0] == 32
    for k, t in enumerate(ts):
        single = sdm.sdm_interpolate_torch(core, penu, float(t), resample=resample)
        for j in (0, 2, 3, 5):
            assert torch.equal(single[j], batched[j])
        for j in (1, 4):
            err = float((single[j] - batched[j][k]).abs().max())
            assert err <= 1e-12, (k, j, err)


def test_non_default_stream_and_single_host_read():
    sdm = _sdm()
    core, penu = (torch.from_numpy(a).cuda() for a in _inputs("odd"))
    ref = sdm.sdm_interpolate_torch(core, penu, 0.35, masks=True)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    before = sdm.host_reads
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with torch.cuda.stream(s):
                got = sdm.sdm_interpolate_torch(core, penu, 0.35, masks=True)
        finally:
            torch.cuda.set_sync_debug_mode(0)
    syncs = [str(w.message) for w in caught if "called a synchronizing" in str(w.message)]
    assert sdm.host_reads - before == 1
    assert len(syncs) <= 1, syncs                   # the info record's read, nothing else
    s.synchronize()
    for a, b in zip(ref[:6], got[:6]):
        assert torch.equal(a, b)
    for a, b in zip(ref[6], got[6]):
        assert torch.equal(a, b)


def test_degenerate_inputs_raise():
    sdm = _sdm()
    core, penu = _inputs("odd")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    with pytest.raises(ValueError, match="penumbra mask .* fills the volume"):
        sdm.sdm_interpolate_torch(dev(core), dev(np.ones_like(penu)), 0.5)
    with pytest.raises(ValueError, match="penumbra is empty"):
        sdm.sdm_interpolate_torch(dev(core), dev(np.zeros_like(penu)), 0.5)
    with pytest.raises(ValueError, match="core mask .* fills the volume"):
        sdm.sdm_interpolate_torch(dev(np.ones_like(core)), dev(penu), 0.5)


def _run_cli(tmp, extra):
    out = os.path.join(str(tmp), "sdm")
    env = dict(os.environ, SP_SYNTHETIC_DATA="1")
    cmd = ["timeout", "-k", "10", "600", sys.executable, CLI, "x.model", "--fold", "0", "1", "--outbasepath", out] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=env, timeout=660)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout, out


@pytest.mark.parametrize("extra", [[], ["--downsample", "0"]])
def test_cli_end_to_end(tmp_path, extra):
    stdout, base = _run_cli(tmp_path, extra)
    lines = re.findall(r"^(\d+) TO-->TR (\S+)$", stdout, re.M)
    assert len(lines) == 2, stdout
    for _, t in lines:
        assert np.isfinite(float(t))
    with open(os.path.join(str(tmp_path), "sdm_results.txt")) as f:
        res = f.read().splitlines()
    assert len(res) == 2, res
    pat = re.compile(r"^Evaluate case: (\d+) - DC:(\S+), HD:(\S+), ASSD:(\S+), Core recon DC:(\S+), Penu recon DC:(\S+)$")
    for line in res:
        m = pat.match(line)
        assert m, line
        assert np.isfinite(float(m.group(2))) and np.isfinite(float(m.group(5))) and np.isfinite(float(m.group(6))), line
    for case, _ in lines:
        for kind in ("lesion", "fuctgt", "core", "penu"):
            a = np.load("%s_%s_%s.npy" % (base, case, kind))
            assert a.shape == (256, 256, 28), (kind, a.shape)
            assert a.dtype == (np.int8 if kind == "fuctgt" else np.float32), (kind, a.dtype)
            if kind != "fuctgt":
                assert set(np.unique(a)) <= {0.0, 1.0}
