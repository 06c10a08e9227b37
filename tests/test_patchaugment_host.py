"""Augmenting patch sampler (common/data.py: PatchAugment, csrc/sp_sample.hip), the parts that need no GPU: the C ABI, the numpy
restatement against scipy, the host draws, the command-line flag, the factories, and the check that the inputs of the GPU tests
keep fp32 coordinate effects inside the share those tests allow."""
import inspect
import os
import random

import numpy as np
import pytest
import torch

import stroke_prediction_amd  # noqa: F401
import sample_ref as R
from gather_ref import gather_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL, FRAC = 2e-4, 1e-3      # the bound of the GPU tests (test_gpu_augment.py::test_batch_transform_matches_scipy uses the same)


def test_header_declares_the_entry_point():
    from stroke_prediction_amd.runtime import lib as L
    with open(L.HEADER) as f:
        _, sigs, _ = L.parse_header(f.read())
    i32, f32, vp = L.i32, L.f32, L.vp
    group = [vp, vp, i32, vp, vp, f32]
    assert sigs["sp_patch_sample_batch"] == (group + group + [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp], i32)
    assert L.SIGS["sp_patch_sample_batch"] == sigs["sp_patch_sample_batch"]
    assert "sp_sample.hip" in L.SOURCES and os.path.isfile(os.path.join(L.CSRC_DIR, "sp_sample.hip"))


def test_argument_errors_need_no_device():
    """the argument checks run on the host before anything is launched; each message names the argument"""
    import ctypes
    from stroke_prediction_amd.runtime import lib as L
    i3 = lambda v: (ctypes.c_int32 * 3)(*v)
    p = ctypes.c_void_p(4096)      # never dereferenced: every call below is refused
    einval = L.CONSTS["SP_EINVAL"]
    call = lambda C0, pad0, pad1, xform, fields, inten: L.load().sp_patch_sample_batch(
        p, p, C0, i3((16, 12, 8)), i3(pad0), -1.0, p, p, 2, i3((10, 8, 6)), i3(pad1), -1.0, p, xform, fields, inten, 3, 3, 9, 22, 26, None)
    assert call(2, (3, 2, 1), (0, 0, 0), None, None, None) == einval and "xform" in L.last_error()
    assert call(2, (3, 2, 1), (4, 0, 0), p, p, None) == einval and "fields" in L.last_error()
    assert call(2, (7, 2, 1), (0, 0, 0), p, p, None) == einval and "fields" in L.last_error()      # ext1 + (pad0 - pad1) > ext0
    assert call(0, (3, 2, 1), (0, 0, 0), p, None, p) == einval and "intensity" in L.last_error()
    assert L.load().sp_patch_sample_batch(None, None, 0, None, None, 0.0, None, None, 0, None, None, -1.0, p, p, None, None, 3, 3, 9, 22, 26,
                                          None) == einval and "both groups are empty" in L.last_error()


def test_sample_ref_matches_scipy_map_coordinates():
    """no padding, no flip: the float64 restatement is scipy.ndimage.map_coordinates(order=1, mode='grid-constant', cval) at the
    coordinates the header states"""
    from scipy import ndimage
    img, lab = R.cache_arrays(5)
    ext = (14, 10, 6)
    table = [[0, 5, 6, 1, 0], [2, 20, 15, 5, 0], [1, -4, -3, -2, 0]]      # inside, overhanging high, overhanging low
    xform = R.affine_xform([11.0, -7.0, 25.0], [0.9, 1.1, 1.3], t=(0.37, -1.21, 0.43))
    got0, got1 = R.sample_ref(img, lab, table, ext, (0, 0, 0), -1.0, ext, (0, 0, 0), -1.0, xform)
    z, y, x = np.meshgrid(np.arange(ext[2]), np.arange(ext[1]), np.arange(ext[0]), indexing="ij")
    c = [(e - 1) / 2 for e in ext]
    for b, (slot, ox, oy, oz, _) in enumerate(table):
        M, t = xform[b, :9].astype(np.float64).reshape(3, 3), xform[b, 9:12].astype(np.float64)
        rel = np.stack([x - c[0], y - c[1], z - c[2]])
        q = np.array([ox, oy, oz])[:, None, None, None] + np.array(c)[:, None, None, None] + np.einsum("ij,jzyx->izyx", M, rel) + t[:, None, None, None]
        for vols, got, cval in ((img, got0, -1.0), (lab, got1, 0.0)):
            for ch in range(2):
                want = ndimage.map_coordinates(vols[slot, ch].astype(np.float64), [q[2], q[1], q[0]], order=1, mode="grid-constant", cval=cval)
                assert np.abs(got[b, ch] - want).max() < 1e-6, (b, ch)


def test_sample_ref_identity_is_the_gather():
    img, lab = R.cache_arrays(1)
    for kind in R.PATCHES:
        ext0, ext1 = R.geometry(kind)
        table = R.table_for(ext0)
        for dtype in (np.float64, np.float32):
            got = R.sample_ref(img, lab, table, ext0, R.PAD0, R.PADVAL0, ext1, (0, 0, 0), -1.0, R.identity_xform(3), dtype=dtype)
            want = gather_ref(img, lab, table, ext0, R.PAD0, R.PADVAL0, ext1, (0, 0, 0))
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # a quarter turn about z on a square patch is rot90 in the (y, x) plane
    ext0, pad0 = (12, 12, 8), (2, 2, 1)
    ext1 = (8, 8, 6)
    table = R.table_for(ext0, pad0)
    turn = R.affine_xform([90.0] * 3, [1.0] * 3)
    turn[:, [0, 4]] = 0.0      # cos(90 deg) in floating point is 6e-17: the entries are 0 and +-1
    got = R.sample_ref(img, lab, table, ext0, pad0, R.PADVAL0, ext1, (0, 0, 0), -1.0, turn, dtype=np.float32)
    want = gather_ref(img, lab, table, ext0, pad0, R.PADVAL0, ext1, (0, 0, 0))
    assert np.array_equal(got[0], np.rot90(want[0], 1, axes=(-2, -1))) and np.array_equal(got[1], np.rot90(want[1], 1, axes=(-2, -1)))


@pytest.mark.parametrize("kind", sorted(R.PATCHES))
def test_fp32_coordinates_stay_inside_the_share_the_gpu_tests_allow(kind):
    """the cap: for the inputs of the general-transform GPU tests the restatement in fp32 differs from the one in float64 by more
    than ATOL at no more than FRAC of the voxels, and no more than FRAC of the soft labels lie within ATOL of the threshold 0.5"""
    img, lab = R.cache_arrays()
    ext0, ext1, table, xform, fields = R.general_case(kind)
    rs = np.random.RandomState(8)
    inten = np.stack([rs.uniform(0.5, 1.5, (3, 2)), rs.uniform(-0.2, 0.2, (3, 2))], axis=2).astype(np.float32)
    args = (img, lab, table, ext0, R.PAD0, R.PADVAL0, ext1, (0, 0, 0), -1.0, xform)
    for kw in (dict(fields=fields), dict(fields=fields, intensity=inten)):
        ref = R.sample_ref(*args, dtype=np.float64, **kw)
        low = R.sample_ref(*args, dtype=np.float32, **kw)
        for a, b in zip(ref, low):
            bad = np.abs(a - b) > ATOL
            print(kind, sorted(kw), "max |f32 - f64| %.3g, above %g: %d of %d" % (np.abs(a - b).max(), ATOL, bad.sum(), bad.size))
            assert bad.mean() <= FRAC
    soft = ref[1]
    near = np.abs(soft - 0.5) <= ATOL
    print(kind, "soft labels within %g of 0.5: %d of %d" % (ATOL, near.sum(), near.size))
    assert near.mean() <= FRAC
    # the inputs exercise what they are meant to: interpolated values, padding, both label classes
    assert ((soft > 0.01) & (soft < 0.99)).mean() > 0.05 and (ref[0] == R.PADVAL0).any() and 0.1 < (soft >= 0.5).mean() < 0.9


def test_patch_augment_draws_are_reproducible_and_leave_random_alone():
    from stroke_prediction_amd.common import data as D
    random.seed(5)
    state = random.getstate()
    a, b, other = D.PatchAugment(seed=4), D.PatchAugment(seed=4), D.PatchAugment(seed=5)
    da, db, do = [a.draw(6, 2) for _ in range(3)], [b.draw(6, 2) for _ in range(3)], [other.draw(6, 2) for _ in range(3)]
    assert random.getstate() == state
    for x, y in zip(da, db):
        assert np.array_equal(x["xform"], y["xform"]) and np.array_equal(x["elastic"], y["elastic"]) and x["call"] == y["call"]
        assert (x["intensity"] is None) == (y["intensity"] is None) and (x["intensity"] is None or np.array_equal(x["intensity"], y["intensity"]))
    assert [d["call"] for d in da] == [0, 1, 2]
    assert any(not np.array_equal(x["xform"], y["xform"]) for x, y in zip(da, do))
    x = np.concatenate([d["xform"] for d in da])
    assert x.dtype == np.float32 and x.shape == (18, 16)
    turned = x[:, 1] != 0
    assert turned.any() and not turned.all()
    # M = (1 / s) R(angle) on x, y and 1 on z: the determinant of the block is 1 / s^2, the angle within +-15 degrees
    s = 1 / np.sqrt(x[:, 0] * x[:, 4] - x[:, 1] * x[:, 3])
    assert np.all((s > 0.85 - 1e-6) & (s < 1.15 + 1e-6)) and np.allclose(x[:, 0], x[:, 4]) and np.allclose(x[:, 1], -x[:, 3])
    assert np.all(np.abs(np.degrees(np.arctan2(x[:, 3], x[:, 0]))) <= 15 + 1e-4)
    assert np.all(x[:, [2, 5, 6, 7, 9, 10, 11, 14, 15]] == 0) and np.all(x[:, 8] == 1)
    on = np.concatenate([d["elastic"] for d in da])
    assert on.any() and not on.all() and np.all(x[on, 12] == 100) and np.allclose(x[on, 13], 22) and np.all(x[~on, 12:14] == 0)
    inten = [d["intensity"] for d in da if d["intensity"] is not None]
    assert inten and all(i.shape == (6, 2, 2) and i.dtype == np.float32 for i in inten)
    g, bi = np.concatenate(inten)[..., 0], np.concatenate(inten)[..., 1]
    assert np.all((g >= 0.9) & (g <= 1.1)) and np.all((bi >= -0.1) & (bi <= 0.1)) and (g != 1).any() and (g == 1).any()
    assert D.PatchAugment(seed=1).thresh1 == 0.5 and D.PatchAugment(label_threshold=None, seed=1).thresh1 == -1.0
    with pytest.raises(ValueError, match="scale"):
        D.PatchAugment(scale=(0.0, 1.0))
    with pytest.raises(ValueError, match="p_elastic"):
        D.PatchAugment(p_elastic=1.5)


def test_zero_probabilities_draw_the_identity():
    from stroke_prediction_amd.common import data as D
    aug = D.PatchAugment(p_affine=0, p_elastic=0, p_intensity=0, seed=3)
    for _ in range(3):
        d = aug.draw(5, 2)
        assert np.array_equal(d["xform"], R.identity_xform(5))      # M = I, t = 0, alphas 0
        assert d["intensity"] is None and not d["elastic"].any()    # gain 1, bias 0: no intensity table at all
        assert aug.make_fields(d, 5, (8, 12, 16), "cpu") is None    # and no noise / filter launches
    always = D.PatchAugment(p_affine=1, p_elastic=1, p_intensity=1, seed=3).draw(4, 2)
    assert always["elastic"].all() and always["intensity"] is not None and np.all(always["xform"][:, 1] != 0)


def test_parser_takes_patchaugment_with_devicecache_only(capsys):
    from common import util
    assert util.get_args_unet_training(["/tmp/unet.model"]).patchaugment is False
    assert util.get_args_unet_training(["/tmp/unet.model", "--devicecache", "--patchaugment"]).patchaugment is True
    assert util.get_args_unet_training(["/tmp/unet.model", "--batchaugment"]).batchaugment is True      # accepted as before
    capsys.readouterr()
    with pytest.raises(SystemExit):
        util.get_args_unet_training(["/tmp/unet.model", "--patchaugment"])
    assert "--patchaugment needs --devicecache" in capsys.readouterr().err
    with pytest.raises(SystemExit):      # the U-Net script's flag only
        util.get_args_shape_training(["--patchaugment"])


def test_factories_take_patch_augment(monkeypatch):
    from stroke_prediction_amd.common import data as D
    monkeypatch.setenv("SP_SYNTHETIC_DATA", "1")
    for fn in (D.split_data_loader3D, D.single_data_loader3D, D.get_stroke_shape_training_data, D.get_stroke_prediction_training_data):
        assert inspect.signature(fn).parameters["patch_augment"].default is None
    assert inspect.signature(D.CachedBatchLoader.__init__).parameters["patch_augment"].default is None
    aug = D.PatchAugment(seed=1)
    tf = [D.ToTensor()]
    with pytest.raises(ValueError, match="patch_augment needs device_cache"):
        D.get_stroke_shape_training_data(["a"], ["x"], tf, tf, [0, 1, 2, 3], 0.5, batchsize=2, patch_augment=aug)
    with pytest.raises(ValueError, match="patch_augment needs device_cache"):
        D.split_data_loader3D(["a"], ["x"], [0, 1, 2, 3], 2, train_transform=tf, valid_transform=tf, patch_augment=aug)
    with pytest.raises(ValueError, match="patch_augment needs device_cache"):
        D.single_data_loader3D(["a"], ["x"], [0, 1], 2, train_transform=tf, patch_augment=aug)
    with pytest.raises(ValueError, match="patch_augment needs device_cache"):
        D.get_stroke_shape_training_data(["a"], ["x"], tf, tf, [0, 1], 0.5, batchsize=2, split=False, patch_augment=aug)


def test_loader_hands_the_draws_to_the_sample_launch(monkeypatch):
    """with an augmenter make_batch goes through _sample_launch (not the gather) with the loader's geometry; Python's random is
    consumed exactly as without one, so the tables agree"""
    from stroke_prediction_amd.common import data as D
    ds = D.SyntheticStrokeDataset3D(modalities=["a", "b"], labels=["x", "y"], transform=D.Compose([D.ResamplePlaneXY(0.5)]), xy=32, z=6, n_cases=4)
    cache = D.DeviceCaseCache(ds, device=None)
    chain = [D.ResamplePlaneXY(0.5), D.HemisphericFlip(), D.PadImages(4, 4, 2, pad_value=0), D.RandomPatch(16, 12, 6, 4, 4, 2), D.ToTensor()]
    seen = []

    def sample(cache, table, ext0, pad0, padval0, ext1, pad1, augment):
        seen.append((table.clone(), ext0, pad0, padval0, ext1, pad1, augment))
        a, b = gather_ref(cache.images.numpy(), cache.labels.numpy(), table.numpy(), ext0, pad0, padval0, ext1, pad1)
        return torch.from_numpy(a), torch.from_numpy(b), table
    monkeypatch.setattr(D, "_sample_launch", sample)
    monkeypatch.setattr(D, "_gather_launch", lambda *a: sample(*a, None))
    aug = D.PatchAugment(seed=2)
    plain, augmented = D.CachedBatchLoader(cache, [0, 1, 2, 3], 3, chain), D.CachedBatchLoader(cache, [0, 1, 2, 3], 3, chain, patch_augment=aug)
    random.seed(9)
    plain.make_batch([3, 0, 2])
    after = random.random()
    random.seed(9)
    batch = augmented.make_batch([3, 0, 2])
    assert random.random() == after
    assert seen[0][6] is None and seen[1][6] is aug and augmented.patch_augment is aug and plain.patch_augment is None
    assert torch.equal(seen[0][0], seen[1][0]) and seen[0][1:6] == seen[1][1:6] == ((16, 12, 6), (4, 4, 2), 0, (8, 4, 2), (0, 0, 0))
    assert sorted(batch) == ["case_id", "clinical", "clinical_idx", "images", "labels"]
