"""``data.IntensityAugment`` without a GPU: its host draws, the numpy restatement of its kernels (tests/intensity_ref.py) against
scipy and against the statistics of a normal sample, the parser's ``--intensityaugment`` flags and the wiring of
train_unet_segmentation.py."""
import contextlib
import io
import os
import random
import sys

import numpy as np
import pytest
import torch

import stroke_prediction_amd  # noqa: F401
from stroke_prediction_amd.common import data as D, util
from stroke_prediction_amd.runtime import lib as L
import intensity_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "stroke-prediction_amd")


def test_source_header_and_entry_points():
    assert "sp_intensity.hip" in L.SOURCES and os.path.isfile(os.path.join(L.CSRC_DIR, "sp_intensity.hip"))
    assert os.path.isfile(os.path.join(L.CSRC_DIR, "sp_philox.h"))
    for src in ("sp_augment.hip", "sp_intensity.hip"):      # one definition of the generator, included by both
        text = open(os.path.join(L.CSRC_DIR, src)).read()
        assert '#include "sp_philox.h"' in text and "void philox4x32_10" not in text
    vp, i32, i64 = L.vp, L.i32, L.i64
    assert L.SIGS["sp_blur3d_reflect_batch"] == ([vp] * 4 + [i32] * 5 + [vp], i32)
    assert L.SIGS["sp_intensity_stats_partials"] == ([vp] * 3 + [i32, i64, i64, i64, vp], i32)
    assert L.SIGS["sp_intensity_apply_batch"] == ([vp] * 4 + [i32, i64, i64, i64, vp], i32)


def test_arguments_are_checked_before_any_gpu_work():
    lib = L.load()
    einval = L.CONSTS["SP_EINVAL"]
    assert lib.sp_blur3d_reflect_batch(None, None, None, None, 1, 4, 4, 4, 1, None) == einval and "sp_blur3d_reflect_batch" in L.last_error()
    a, b, c, w = 4096, 8192, 12288, 16384      # never dereferenced: every call below fails its argument check
    assert lib.sp_blur3d_reflect_batch(a, b, c, w, 1, 3, 8, 8, 4, None) == einval and "radius" in L.last_error()      # Z < radius
    assert lib.sp_blur3d_reflect_batch(a, b, c, w, 1, 8, 8, 3, 4, None) == einval and "radius" in L.last_error()      # X < radius
    assert lib.sp_blur3d_reflect_batch(a, a, c, w, 1, 8, 8, 8, 4, None) == einval and "different" in L.last_error()
    assert lib.sp_blur3d_reflect_batch(a, b, c, w, 65536, 8, 8, 8, 4, None) == einval and "nfields" in L.last_error()
    assert lib.sp_blur3d_reflect_batch(a, b, c, w, 1, 8, 8, 8, 65, None) == einval
    assert lib.sp_blur3d_reflect_batch(a, b, c, w, 1, 2048, 1024, 1024, 4, None) == einval and "2^31" in L.last_error()
    for name in ("sp_intensity_stats_partials", "sp_intensity_apply_batch"):
        fn = getattr(lib, name)
        ptrs = (a, b, c) if name.endswith("partials") else (a, b, c, w)
        none = (None,) * len(ptrs)
        assert fn(*none, 1, 16, 0, 0, None) == einval and name in L.last_error()
        assert fn(*ptrs, 0, 16, 0, 0, None) == einval and fn(*ptrs, 65536, 16, 0, 0, None) == einval and "nfields" in L.last_error()
        assert fn(*ptrs, 1, 0, 0, 0, None) == einval and fn(*ptrs, 1, 1 << 31, 0, 0, None) == einval and "per_field" in L.last_error()
        assert fn(*ptrs[:-1], ptrs[-1] + 4, 1, 16, 0, 0, None) == einval and "aligned" in L.last_error()      # partials


# ------------------------------------------------------------------------------------------------ host draws

class CountingState(np.random.RandomState):
    """counts the values drawn through the methods ``IntensityAugment.draw`` uses"""

    def __init__(self, seed):
        super().__init__(seed)
        self.drawn = 0

    def rand(self, *shape):
        self.drawn += int(np.prod(shape))
        return super().rand(*shape)

    def uniform(self, low=0.0, high=1.0, size=None):
        self.drawn += int(np.prod(size))
        return super().uniform(low, high, size)


@pytest.mark.parametrize("B,C0", [(2, 2), (6, 2), (3, 1)])
def test_draw_count_does_not_depend_on_the_probabilities(B, C0):
    counts, states = [], []
    for p in (0.0, 1.0, 0.5):
        aug = D.IntensityAugment(p_noise=p, p_blur=p, p_blur_channel=p, p_gain=p, p_contrast=p, p_gamma=p, p_gamma_invert=p, seed=3)
        aug._rs = CountingState(3)
        for _ in range(3):
            aug.draw(B, C0)
        counts.append(aug._rs.drawn)
        states.append(aug._rs.get_state()[1].tolist() + [aug._rs.get_state()[2]])
    assert counts[0] == counts[1] == counts[2] > 0
    assert states[0] == states[1] == states[2]      # and the generator stands where it would with any other tosses


def test_draw_is_reproducible_and_the_call_counter_advances():
    a, b, other = D.IntensityAugment(seed=9), D.IntensityAugment(seed=9), D.IntensityAugment(seed=10)
    on = dict(p_noise=1, p_blur=1, p_blur_channel=1, p_gain=1, p_contrast=1, p_gamma=1)
    full_a, full_b = D.IntensityAugment(seed=9, **on), D.IntensityAugment(seed=9, **on)
    differs = False
    for n in range(4):
        da, db, do = a.draw(3, 2), b.draw(3, 2), other.draw(3, 2)
        assert da["call"] == db["call"] == n
        assert np.array_equal(da["params"], db["params"]) and da["radius"] == db["radius"]
        assert (da["weights"] is None) == (db["weights"] is None) and (da["weights"] is None or np.array_equal(da["weights"], db["weights"]))
        differs = differs or not np.array_equal(da["params"], do["params"])
        fa, fb = full_a.draw(3, 2), full_b.draw(3, 2)
        assert np.array_equal(fa["params"], fb["params"]) and np.array_equal(fa["weights"], fb["weights"])
    assert differs and a._calls == 4


def test_draw_tables():
    off = D.IntensityAugment(p_noise=0, p_blur=0, p_gain=0, p_contrast=0, p_gamma=0, p_gamma_invert=0, seed=1).draw(4, 2)
    assert off["weights"] is None and off["radius"] == 0
    assert off["params"].dtype == np.float32 and np.array_equal(off["params"], np.tile(np.array(R.NEUTRAL, np.float32), (8, 1)))
    aug = D.IntensityAugment(p_noise=1, p_blur=1, p_blur_channel=1, p_gain=1, p_contrast=1, p_gamma=1, p_gamma_invert=0, seed=1)
    d = aug.draw(50, 2)
    p, w = d["params"], d["weights"]
    assert p.shape == (100, 8) and w.shape == (100, 2 * d["radius"] + 1) and d["radius"] == 4      # sigma up to 1.0
    assert (p[:, 0] >= 0).all() and (p[:, 0] <= np.sqrt(0.1) + 1e-6).all() and p[:, 0].std() > 0      # sqrt(variance)
    for col, (lo, hi) in ((1, aug.gain), (2, aug.contrast), (3, aug.gamma)):
        assert (p[:, col] >= np.float32(lo)).all() and (p[:, col] <= np.float32(hi)).all()
        assert (p[:, col] < 1).any() and (p[:, col] > 1).any()
    assert not p[:, 4:].any()
    np.testing.assert_allclose(w.sum(1), 1.0, atol=1e-6)
    assert np.array_equal(w, w[:, ::-1]) and (w[:, 4] > w[:, 3]).all()
    # tosses are per sample, parameters per field: the two channels of a sample share the decision, not the value
    inv = D.IntensityAugment(p_gamma=0, p_gamma_invert=0.5, p_noise=0.5, seed=2).draw(40, 2)["params"].reshape(40, 2, 8)
    assert np.array_equal(inv[:, 0, 4], inv[:, 1, 4]) and 0 < inv[:, 0, 4].sum() < 40
    assert np.array_equal(inv[:, :, 3] != 1, inv[:, :, 4] == 1)      # gamma only where inverted
    assert np.array_equal(inv[:, 0, 0] > 0, inv[:, 1, 0] > 0) and not np.array_equal(inv[:, 0, 0], inv[:, 1, 0])
    # a blurring batch whose fields do not all blur: the others carry the delta kernel at the batch's radius
    mixed = D.IntensityAugment(p_blur=1, p_blur_channel=0.5, seed=5).draw(8, 2)
    delta = np.zeros(2 * mixed["radius"] + 1, np.float32)
    delta[mixed["radius"]] = 1
    is_delta = [np.array_equal(r_, delta) for r_ in mixed["weights"]]
    assert any(is_delta) and not all(is_delta)


def test_python_random_and_numpy_global_streams_are_untouched():
    random.seed(5)
    np.random.seed(5)
    want = (random.random(), np.random.rand())
    random.seed(5)
    np.random.seed(5)
    aug = D.IntensityAugment(seed=1)
    aug.draw(4, 2)
    assert (random.random(), np.random.rand()) == want


def test_constructor_refuses_nonsense():
    for kw in (dict(gain=(0, 1)), dict(contrast=(-1, 1)), dict(gamma=(0, 2)), dict(gain=(1.2, 0.8)), dict(noise_variance=(-0.1, 0.1)),
               dict(p_noise=1.5), dict(p_gamma_invert=-0.1), dict(blur_sigma=(0, 1)), dict(blur_sigma=(1, 40)), dict(gamma=(1,))):
        with pytest.raises(ValueError):
            D.IntensityAugment(**kw)


def test_there_is_no_cpu_path():
    aug = D.IntensityAugment(seed=1)
    labels = torch.zeros((1, 1, 4, 4, 4))
    for images in (torch.zeros((1, 1, 4, 4, 4)), np.zeros((1, 1, 4, 4, 4), np.float32), []):
        with pytest.raises(RuntimeError, match="no CPU path"):
            aug({D.KEY_IMAGES: images, D.KEY_LABELS: labels})
    assert aug._calls == 0      # refused before any draw


# ------------------------------------------------------------------------------------------------ the reference itself

@pytest.mark.parametrize("sigma", [0.5, 0.8, 1.0, 2.3])
def test_reference_blur_equals_scipy(sigma):
    from scipy import ndimage
    x = R.smooth_volumes(1, (9, 14, 17), 3)[0].astype(np.float64)
    w = R.gaussian_weights(sigma)
    assert np.array_equal(w, D.gaussian_weights(sigma)) and len(w) == 2 * int(4 * sigma + 0.5) + 1
    want = ndimage.gaussian_filter(x, sigma)      # mode="reflect", truncate=4: its defaults
    assert np.abs(R.blur_field(x, w) - want).max() < 2e-6      # tests/test_transforms.py's bound for the Gaussian filter
    assert np.abs(R.blur_field(x, R.gaussian_weights(sigma, 9)) - want).max() < 2e-6      # zero-padded to a larger radius
    assert np.abs(R.blur_field(x, w.astype(np.float32), np.float32) - want).max() < 2e-6
    assert np.array_equal(D.gaussian_weights(sigma, 9), R.gaussian_weights(sigma, 9))


def test_reference_blur_at_an_extent_equal_to_the_radius():
    from scipy import ndimage
    x = np.random.RandomState(0).rand(4, 9, 4)
    assert np.abs(R.blur_field(x, R.gaussian_weights(1.0)) - ndimage.gaussian_filter(x, 1.0)).max() < 2e-6


def test_reference_normals_are_standard_normal():
    n = 1 << 16
    v = R.normals(0, n, R.SEED, R.CALL)
    assert abs(v.mean()) < 5 / np.sqrt(n) and abs(v.var() - 1) < 5 * np.sqrt(2.0 / n)
    v32 = R.normals(0, n, R.SEED, R.CALL, np.float32)
    assert v32.dtype == np.float32 and np.abs(v32 - v).max() < 1e-5
    # the value is a function of (seed, call, field, element): another field, call or seed is another stream, a longer field
    # starts with the same values
    assert np.array_equal(R.normals(0, 1000, R.SEED, R.CALL), v[:1000])
    for other in (R.normals(1, n, R.SEED, R.CALL), R.normals(0, n, R.SEED, R.CALL + 1), R.normals(0, n, R.SEED + 1, R.CALL)):
        assert abs(np.corrcoef(v, other)[0, 1]) < 5 / np.sqrt(n)


def test_reference_stream_is_apart_from_the_uniform_noise():
    """field word 0x80000000 | f: with one seed and call the normals' Philox blocks are not those of sp_rng_uniform_pm1"""
    import augment_ref as A
    q = np.arange(64, dtype=np.uint64)
    full = lambda v: np.full(64, v, dtype=np.uint64)
    uni = A.philox4x32_10((q, full(0), full(R.CALL), full(0)), (R.SEED, 0))
    nor = A.philox4x32_10((q, full(0x80000000), full(R.CALL), full(0)), (R.SEED, 0))
    assert not any(np.array_equal(a, b) for a, b in zip(uni, nor))


def test_reference_identities():
    x = R.smooth_volumes(4, (7, 10, 13), 1)
    neutral = np.tile(np.array(R.NEUTRAL, np.float32), (4, 1))
    assert np.array_equal(R.apply(x, neutral, 1, 0, np.float32), x)
    gains = neutral.copy()
    gains[:, 1] = (0.75, 0.9, 1.1, 1.25)
    assert np.array_equal(R.apply(x, gains, 1, 0, np.float32), gains[:, 1, None, None, None] * x)
    # contrast and both gammas keep the field's range; the inverted gamma is the plain one of the negated field
    for table in (R.TABLES["single"][1:2], R.TABLES["single"][2:3], R.TABLES["single"][3:4]):
        y = R.apply(x[:1], table, 1, 0)
        assert abs(y.min() - x[0].min()) < 1e-6 and abs(y.max() - x[0].max()) < 1e-6
    plain = np.array([R.row(gamma=1.5)], np.float32)
    assert np.abs(R.apply(x[:1], R.TABLES["single"][3:4], 1, 0) + R.apply(-x[:1], plain, 1, 0)).max() < 1e-12


def test_tolerances_of_the_gpu_tests_are_four_times_the_measured_fp32_distance():
    import test_gpu_intensity as G
    for name, table in R.TABLES.items():
        measured = max(R.fp32_distance(table, shape) for shape in R.SHAPES)
        print(name, "fp32 evaluation - float64 evaluation: %.4g, constant %.4g" % (measured, G.MEASURED[name]))
        assert measured <= G.MEASURED[name] <= 1.25 * measured
        assert G.TOL[name] == 4 * G.MEASURED[name]


# ------------------------------------------------------------------------------------------------ parser and script

def _parse(argv):
    with contextlib.redirect_stdout(io.StringIO()):
        return util.get_args_unet_training(["/tmp/unet.model"] + argv)


def test_parser_defaults_are_the_constructor_defaults():
    ns = _parse([])
    assert ns.intensityaugment is False
    aug, ref = D.IntensityAugment(seed=1, **util.intensity_augment_kwargs(ns)), D.IntensityAugment(seed=1)
    names = ("noise_variance", "blur_sigma", "gain", "contrast", "gamma", "p_noise", "p_blur", "p_blur_channel", "p_gain", "p_contrast",
             "p_gamma", "p_gamma_invert")
    assert [getattr(aug, n) for n in names] == [getattr(ref, n) for n in names]
    ns = _parse(["--intensityaugment", "--iagamma", "0.5", "2", "--iapblur", "0.75", "--ianoisevariance", "0", "0.05"])
    kw = util.intensity_augment_kwargs(ns)
    assert ns.intensityaugment and kw["gamma"] == (0.5, 2.0) and kw["p_blur"] == 0.75 and kw["noise_variance"] == (0.0, 0.05)


@pytest.mark.parametrize("argv", [["--iagain", "0", "1"], ["--iagain", "-0.5", "1"], ["--iacontrast", "0", "1.25"], ["--iagamma", "0", "1.5"],
                                  ["--iagamma", "1.5", "0.7"], ["--iablursigma", "1.0", "0.5"], ["--iablursigma", "0", "1"],
                                  ["--iablursigma", "1", "30"], ["--ianoisevariance", "-0.1", "0.1"], ["--ianoisevariance", "0.2", "0.1"],
                                  ["--iapnoise", "1.5"], ["--iapblur", "-0.1"], ["--iapblurchannel", "2"], ["--iapgain", "-1"],
                                  ["--iapcontrast", "1.01"], ["--iapgamma", "7"], ["--iapgammainvert", "-0.5"], ["--iagain", "1"]])
def test_parser_errors_fire(argv, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(argv)
    assert e.value.code == 2 and "--ia" in capsys.readouterr().err


@pytest.fixture
def script():
    """train_unet_segmentation.py imported as a module; what the import adds to sys.path and sys.modules (the script's own
    ``common`` / ``learner`` packages) is taken away again"""
    path, modules = list(sys.path), set(sys.modules)
    sys.path.insert(0, PKG)
    try:
        import train_unet_segmentation as S
        yield S
    finally:
        sys.path[:] = path
        for name in set(sys.modules) - modules:
            del sys.modules[name]


def _captured_factory_call(S, monkeypatch, argv):
    seen = {}

    class Loader:
        class sampler:
            indices = [0]

    def factory(*args, **kw):
        seen["args"], seen["kw"] = args, kw
        return Loader(), Loader()

    monkeypatch.setattr(S.data, "get_stroke_shape_training_data", factory)
    state = (random.getstate(), np.random.get_state()[1].tolist())
    with contextlib.redirect_stdout(io.StringIO()):
        S.build_loaders(_parse(argv))
    assert (random.getstate(), np.random.get_state()[1].tolist()) == state      # neither global stream is drawn from
    return seen


def test_script_without_the_flag_calls_the_factory_as_before(script, monkeypatch):
    seen = _captured_factory_call(script, monkeypatch, ["--seed", "6"])
    assert sorted(seen["kw"]) == ["batchsize", "device_cache", "foreground", "patch_augment", "seed"]
    assert seen["kw"]["patch_augment"] is None and seen["kw"]["foreground"] is None and seen["kw"]["device_cache"] is False
    assert len(seen["args"]) == 6


def test_script_with_the_flag_hands_a_seeded_transform_to_the_factory(script, monkeypatch):
    S = script
    seen = _captured_factory_call(S, monkeypatch, ["--seed", "6", "--intensityaugment", "--iapgamma", "1", "--iagamma", "0.8", "1.2"])
    bt = seen["kw"]["batch_transform"]
    assert isinstance(bt, S.data.IntensityAugment) and bt._seed == 6 and bt.p_gamma == 1.0 and bt.gamma == (0.8, 1.2)
    assert sorted(set(seen["kw"]) - {"batch_transform"}) == ["batchsize", "device_cache", "foreground", "patch_augment", "seed"]
    assert seen["kw"]["patch_augment"] is None      # it needs neither --devicecache nor --patchaugment ...
    seen = _captured_factory_call(S, monkeypatch, ["--intensityaugment", "--devicecache", "--patchaugment", "--fgfraction", "0.33"])
    assert isinstance(seen["kw"]["batch_transform"], S.data.IntensityAugment) and seen["kw"]["batch_transform"]._seed == 4      # ... and composes
    assert isinstance(seen["kw"]["patch_augment"], S.data.PatchAugment) and isinstance(seen["kw"]["foreground"], S.data.ForegroundOversample)


def test_validation_loader_never_gets_the_transform(monkeypatch):
    """the factories apply batch_transform to the training loader only (the per-sample path: no GPU needed to build the loaders)"""
    monkeypatch.setenv("SP_SYNTHETIC_DATA", "1")
    aug = D.IntensityAugment(seed=2)
    chain = [D.ToTensor()]
    train, valid = D.split_data_loader3D(["a"], ["x"], [0, 1, 2, 3], 2, random_seed=4, train_transform=chain, valid_transform=chain,
                                         num_workers=0, batch_transform=aug)
    assert train.collate_fn.batch_transform is aug
    assert not isinstance(valid.collate_fn, D._CollateThenTransform)
