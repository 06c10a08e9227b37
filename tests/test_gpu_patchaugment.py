"""Augmenting patch sampler on the GPU: ``sp_patch_sample_batch`` (csrc/sp_sample.hip) against ``sp_patch_gather_batch`` where the
transform moves whole voxels (bit for bit) and against its numpy restatement in float64 (tests/sample_ref.py) elsewhere,
``CachedBatchLoader(patch_augment=...)`` against the plain loader, and the U-Net script with ``--patchaugment``."""
import ctypes
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import stroke_prediction_amd  # noqa: F401
import sample_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "stroke-prediction_amd")
DEV = "cuda:0"
GUARD, GUARD_VALUE = 64, 777.0
ATOL, FRAC = 2e-4, 1e-3      # test_gpu_augment.py::test_batch_transform_matches_scipy: the same arithmetic, the same bound
NO_PAD1 = (0, 0, 0)


def _i3(v):
    return (ctypes.c_int32 * 3)(*[int(a) for a in v])


def _close_but_for_edge_flips(got, want, atol, frac):
    """fp32 coordinates: a sampling point next to a cell or volume face can land on its other side -- at most a share `frac` of
    the voxels may differ by more than atol (tests/test_patchaugment_host.py holds the fp32 restatement to the same share)"""
    bad = np.abs(got - want) > atol
    print("max |diff| %.3g, voxels above %g: %d of %d (%.3g, allowed %g)" % (float(np.abs(got - want).max()), atol, bad.sum(), bad.size,
                                                                            bad.mean(), frac))
    assert bad.mean() <= frac, (bad.sum(), bad.size, float(np.abs(got - want).max()))


@pytest.fixture(scope="module")
def cache():
    """N = 3 cases, two smooth images in [0, 1], two binary labels, (Z, Y, X) = (9, 22, 26): host arrays and their device copies"""
    img, lab = R.cache_arrays()
    return img, lab, torch.from_numpy(img).to(DEV), torch.from_numpy(lab).to(DEV)


def _buffers(B, C, ext):
    """an output filled with NaN (an element the kernel leaves out shows) followed by a guard tail it must not touch"""
    shape = (B, C, ext[2], ext[1], ext[0])
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    buf[n:] = GUARD_VALUE
    return buf, buf[:n].view(shape)


def _launch(entry, cache, table, ext0, pad0, ext1, scalar1, extra=None, C0=2, C1=2, pad1=NO_PAD1):
    """one launch of the gather (``extra`` None; ``scalar1`` = padval1) or of the sampler (``extra`` = xform, fields, intensity as
    numpy arrays or None; ``scalar1`` = thresh1) on the cached cases -> (rc, dst0, dst1) as numpy"""
    from stroke_prediction_amd.runtime import lib as L, ops as O
    _, _, img, lab = cache
    B = len(table)
    tab = torch.tensor(table, dtype=torch.int32).reshape(-1, 5).to(DEV)
    buf0, d0 = _buffers(B, max(C0, 1), ext0)
    buf1, d1 = _buffers(B, max(C1, 1), ext1)
    held = [None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV) for a in (extra or [])]
    rc = getattr(L.load(), entry)(O.ptr(img), O.ptr(d0), C0, _i3(ext0), _i3(pad0), R.PADVAL0, O.ptr(lab), O.ptr(d1), C1, _i3(ext1), _i3(pad1),
                                  float(scalar1), O.ptr(tab), *[O.ptr(t) if t is not None else None for t in held], 3, B, *R.ZYX, O.stream())
    torch.cuda.synchronize()
    if rc == 0:
        for buf, d in ((buf0, d0), (buf1, d1)):
            assert bool((buf[d.numel():] == GUARD_VALUE).all()), "the kernel wrote behind its output"
    return rc, d0.cpu().numpy(), d1.cpu().numpy()


def _gather(cache, table, ext0, pad0, ext1):
    rc, a, b = _launch("sp_patch_gather_batch", cache, table, ext0, pad0, ext1, 0.0)
    assert rc == 0
    return a, b


def _sample(cache, table, ext0, pad0, ext1, xform, fields=None, intensity=None, thresh1=-1.0, **kw):
    return _launch("sp_patch_sample_batch", cache, table, ext0, pad0, ext1, thresh1, [xform, fields, intensity], **kw)


def _same(got, want):
    assert got.shape == want.shape and np.array_equal(got, want)      # (NaN != NaN: an unwritten element fails here)


@pytest.fixture(scope="module")
def general(cache):
    """the float64 reference of the general transform, once per patch size: (soft outputs, outputs with intensity)"""
    img, lab = cache[:2]
    out = {}
    for kind in R.PATCHES:
        ext0, ext1, table, xform, fields = R.general_case(kind)
        rs = np.random.RandomState(8)
        inten = np.stack([rs.uniform(0.5, 1.5, (3, 2)), rs.uniform(-0.2, 0.2, (3, 2))], axis=2).astype(np.float32)
        args = (img, lab, table, ext0, R.PAD0, R.PADVAL0, ext1, NO_PAD1, -1.0, xform)
        out[kind] = dict(ext0=ext0, ext1=ext1, table=table, xform=xform, fields=fields, inten=inten,
                         soft=R.sample_ref(*args, fields=fields), gained=R.sample_ref(*args, fields=fields, intensity=inten))
    return out


KINDS = sorted(R.PATCHES)


@pytest.mark.parametrize("kind", KINDS)
def test_identity_equals_the_gather(cache, kind):
    ext0, ext1 = R.geometry(kind)
    table = R.table_for(ext0)
    rc, got0, got1 = _sample(cache, table, ext0, R.PAD0, ext1, R.identity_xform(3))
    assert rc == 0
    want0, want1 = _gather(cache, table, ext0, R.PAD0, ext1)
    _same(got0, want0)
    _same(got1, want1)
    assert np.all(got0[2] == R.PADVAL0) and np.all(got1[2] == 0)      # the slot outside the cache
    assert (got0[:2] == R.PADVAL0).any() and (got0[:2] != R.PADVAL0).any()


@pytest.mark.parametrize("kind", KINDS)
def test_integer_translation_equals_the_gather_at_the_shifted_origin(cache, kind):
    ext0, ext1 = R.geometry(kind)
    table = R.table_for(ext0)
    xform = R.identity_xform(3)
    xform[:, 9:12] = (2, -1, 1)
    rc, got0, got1 = _sample(cache, table, ext0, R.PAD0, ext1, xform)
    assert rc == 0
    want0, want1 = _gather(cache, [[s, ox + 2, oy - 1, oz + 1, f] for s, ox, oy, oz, f in table], ext0, R.PAD0, ext1)
    _same(got0, want0)
    _same(got1, want1)


def test_quarter_turn_equals_rot90(cache):
    """a square patch with a square label crop (pad0 = (2, 2, 1): the crop ext0 - 2 pad0 shares the patch centre), M entries 0, +-1"""
    ext0, pad0, ext1 = (12, 12, 8), (2, 2, 1), (8, 8, 6)
    table = R.table_for(ext0, pad0)
    turn = R.identity_xform(3)
    turn[:, 0:2] = (0, -1)
    turn[:, 3:5] = (1, 0)
    rc, got0, got1 = _sample(cache, table, ext0, pad0, ext1, turn)
    assert rc == 0
    want0, want1 = _gather(cache, table, ext0, pad0, ext1)
    _same(got0, np.rot90(want0, 1, axes=(-2, -1)))
    _same(got1, np.rot90(want1, 1, axes=(-2, -1)))
    assert not np.array_equal(got0, want0)


@pytest.mark.parametrize("kind", KINDS)
def test_general_transform_matches_the_reference(cache, general, kind):
    g = general[kind]
    rc, got0, got1 = _sample(cache, g["table"], g["ext0"], R.PAD0, g["ext1"], g["xform"], fields=g["fields"])
    assert rc == 0 and not np.isnan(got0).any() and not np.isnan(got1).any()
    _close_but_for_edge_flips(got0, g["soft"][0], ATOL, FRAC)
    _close_but_for_edge_flips(got1, g["soft"][1], ATOL, FRAC)


@pytest.mark.parametrize("kind", KINDS)
def test_thresholded_labels(cache, general, kind):
    g = general[kind]
    rc, got0, got1 = _sample(cache, g["table"], g["ext0"], R.PAD0, g["ext1"], g["xform"], fields=g["fields"], thresh1=0.5)
    assert rc == 0
    soft = g["soft"][1]
    clear = np.abs(soft - 0.5) > ATOL
    assert (~clear).mean() <= FRAC
    assert set(np.unique(got1)) <= {0.0, 1.0}
    assert np.array_equal(got1[clear], (soft >= 0.5).astype(np.float32)[clear])
    assert 0.1 < got1[:2].mean() < 0.9
    _close_but_for_edge_flips(got0, g["soft"][0], ATOL, FRAC)      # the images do not see the threshold


@pytest.mark.parametrize("kind", KINDS)
def test_intensity(cache, general, kind):
    g = general[kind]
    ext0, ext1, table, inten = g["ext0"], g["ext1"], g["table"], g["inten"]
    plain0, plain1 = _gather(cache, table, ext0, R.PAD0, ext1)
    rc, got0, got1 = _sample(cache, table, ext0, R.PAD0, ext1, R.identity_xform(3), intensity=inten)
    assert rc == 0
    # the padding is where gather_ref marks it: rebuild the mask from a gather of ones
    ones = (cache[0] * 0 + 1, cache[1], torch.ones_like(cache[2]), cache[3])
    inside = _gather(ones, table, ext0, R.PAD0, ext1)[0] == 1
    want = inten[:, :, 0, None, None, None] * plain0 + inten[:, :, 1, None, None, None]
    assert inside.any() and (~inside).any()
    assert np.allclose(got0[inside], want[inside], rtol=1e-5, atol=1e-5)
    assert np.all(got0[~inside] == R.PADVAL0)      # padding never takes the intensity change
    _same(got1, plain1)                            # nor do the labels
    # with the general transform: a partly covered cell takes the bias by its covered weight
    rc, got0, got1 = _sample(cache, table, ext0, R.PAD0, ext1, g["xform"], fields=g["fields"], intensity=inten)
    assert rc == 0
    _close_but_for_edge_flips(got0, g["gained"][0], ATOL, FRAC)
    _close_but_for_edge_flips(got1, g["gained"][1], ATOL, FRAC)


@pytest.mark.parametrize("kind", KINDS)
def test_one_field_moves_both_groups(cache, kind):
    """fx = 2 everywhere, alpha_xy = 1: images and labels equal the gather two voxels further in x, so label voxel v and image
    voxel v + pad0 still show the same source voxel"""
    ext0, ext1 = R.geometry(kind)
    table = R.table_for(ext0)
    xform = R.identity_xform(3)
    xform[:, 12:14] = 1.0
    fields = np.zeros((3, 3, ext0[2], ext0[1], ext0[0]), dtype=np.float32)
    fields[:, 0] = 2.0
    rc, got0, got1 = _sample(cache, table, ext0, R.PAD0, ext1, xform, fields=fields)
    assert rc == 0
    want0, want1 = _gather(cache, [[s, ox + 2, oy, oz, f] for s, ox, oy, oz, f in table], ext0, R.PAD0, ext1)
    _same(got0, want0)
    _same(got1, want1)


def test_argument_errors(cache):
    from stroke_prediction_amd.runtime import lib as L
    ext0, ext1 = R.geometry("vector")
    table = R.table_for(ext0)
    einval = L.CONSTS["SP_EINVAL"]
    fields = np.zeros((3, 3, ext0[2], ext0[1], ext0[0]), dtype=np.float32)
    rc, _, _ = _sample(cache, table, ext0, R.PAD0, ext1, None)
    assert rc == einval and "xform" in L.last_error()
    rc, _, _ = _sample(cache, table, ext0, R.PAD0, ext1, R.identity_xform(3), fields=fields, pad1=(4, 2, 1))      # pad1 > pad0 in x
    assert rc == einval and "fields" in L.last_error()
    rc, _, _ = _sample(cache, table, ext0, R.PAD0, ext1, R.identity_xform(3), intensity=np.ones((3, 2, 2), np.float32), C0=0)
    assert rc == einval and "intensity" in L.last_error()


# ------------------------------------------------------------------------------------------------ loader

def _loaders(D, **augment):
    chain = [D.ResamplePlaneXY(0.5), D.HemisphericFlip(), D.PadImages(4, 4, 2, pad_value=0), D.RandomPatch(16, 12, 6, 4, 4, 2), D.ToTensor()]
    kw = dict(modalities=["a", "b"], labels=["x", "y"], xy=32, z=6, n_cases=6)
    cache = D.DeviceCaseCache(D.SyntheticStrokeDataset3D(transform=D.Compose(D._cache_prefix([chain]), device=DEV), **kw), DEV)
    make = lambda aug: D.CachedBatchLoader(cache, list(range(6)), 4, chain, patch_augment=aug)
    return make, chain


def _assert_same_batch(got, want, equal=True):
    assert sorted(got) == sorted(want)
    same = True
    for k in want:
        if isinstance(want[k], torch.Tensor):
            assert isinstance(got[k], torch.Tensor), k
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].device == want[k].device, k
            same = same and torch.equal(got[k], want[k])
        else:
            assert type(got[k]) is type(want[k]) and got[k] == want[k], k
    assert same == equal


def test_loader_with_zero_probabilities_equals_the_plain_loader():
    from stroke_prediction_amd.common import data as D
    make, _ = _loaders(D)
    plain, off = make(None), make(D.PatchAugment(p_affine=0, p_elastic=0, p_intensity=0, seed=1))
    for items in ([5, 0, 3, 3], [1, 2]):
        random.seed(17)
        want = plain.make_batch(items)
        random.seed(17)
        got = off.make_batch(items)
        _assert_same_batch(got, want)
        assert torch.equal(off.last_table, plain.last_table)


def test_loader_is_reproducible_from_the_seed():
    from stroke_prediction_amd.common import data as D
    make, _ = _loaders(D)
    on = dict(p_affine=1, p_elastic=1, p_intensity=1, alpha=20, sigma=2)
    a, b, other, plain = make(D.PatchAugment(seed=4, **on)), make(D.PatchAugment(seed=4, **on)), make(D.PatchAugment(seed=5, **on)), make(None)
    mixed_a, mixed_b = make(D.PatchAugment(seed=6)), make(D.PatchAugment(seed=6))      # the default tosses: some batches without fields
    for n, items in enumerate(([5, 0, 3, 3], [1, 2, 4, 0], [2, 2])):
        batches = []
        for loader in (a, b, other, plain, mixed_a, mixed_b):
            random.seed(30 + n)
            batches.append(loader.make_batch(items))
        _assert_same_batch(batches[1], batches[0])
        _assert_same_batch(batches[2], batches[0], equal=False)      # another seed: same contract, other values
        _assert_same_batch(batches[0], batches[3], equal=False)      # and the augmenter does change the batch
        _assert_same_batch(batches[5], batches[4])
        for k in ("images", "labels"):
            assert bool(torch.isfinite(batches[0][k]).all())
        assert set(batches[0]["labels"].unique().tolist()) <= {0.0, 1.0}      # label_threshold = 0.5


def test_factories_hand_the_augmenter_to_the_training_loader_only(monkeypatch):
    from stroke_prediction_amd.common import data as D
    monkeypatch.setenv("SP_SYNTHETIC_DATA", "1")
    _, chain = _loaders(D)
    aug = D.PatchAugment(p_affine=1, p_elastic=1, p_intensity=1, alpha=20, sigma=2, seed=2)
    args = (["a", "b"], ["x", "y"], [0, 1, 2, 3, 4, 5], 2)
    kw = dict(random_seed=4, train_transform=chain, valid_transform=chain, device_cache=True)
    train, valid = D.split_data_loader3D(*args, patch_augment=aug, **kw)
    train0, valid0 = D.split_data_loader3D(*args, **kw)
    assert train.patch_augment is aug and valid.patch_augment is None and train0.patch_augment is None
    items = list(valid.sampler.indices)
    assert items == list(valid0.sampler.indices)
    random.seed(3)
    got = valid.make_batch(items)
    random.seed(3)
    want = valid0.make_batch(items)
    _assert_same_batch(got, want)
    single = D.single_data_loader3D(*args, random_seed=4, train_transform=chain, device_cache=True, patch_augment=aug)
    assert single.patch_augment is aug
    random.seed(3)
    got = train.make_batch(list(train.sampler.indices))
    random.seed(3)
    _assert_same_batch(got, train0.make_batch(list(train0.sampler.indices)), equal=False)


# ------------------------------------------------------------------------------------------------ script

def test_train_unet_segmentation_script_with_patchaugment(tmp_path):
    base = str(tmp_path / "unet")
    unetpath = str(tmp_path / "unet.model")
    env = dict(os.environ, SP_SYNTHETIC_DATA="1", MPLBACKEND="Agg")
    common = [sys.executable, os.path.join(PKG, "train_unet_segmentation.py"), unetpath, "--graph", "--fusedadam", "--epochs", "2", "--batchsize",
              "2", "--fold"] + [str(i) for i in range(8)] + ["--outbasepath", base]
    r = subprocess.run(common + ["--patchaugment"], capture_output=True, text=True, env=env, timeout=300, cwd=ROOT)
    assert r.returncode != 0 and "--patchaugment needs --devicecache" in r.stderr
    assert not os.path.exists(unetpath)
    r = subprocess.run(common + ["--devicecache", "--patchaugment"], capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "patchaugment=True" in r.stdout
    losses = [float(v) for v in re.findall(r"Epoch \d/2 training loss: (\S+)", r.stdout)]
    assert len(losses) == 2 and all(np.isfinite(v) for v in losses), r.stdout[-1500:]
    for f in (base + "_unet.model", base + "_unet_final.model", unetpath):
        assert os.path.exists(f), f
