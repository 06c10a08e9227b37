"""Device-resident case cache on the GPU: ``sp_patch_gather_batch`` (csrc/sp_gather.hip) against its numpy restatement
(tests/gather_ref.py), ``CachedBatchLoader`` against the per-sample transform chain it replaces, and the U-Net script with
``--devicecache``.  Pure data movement: every comparison is bit for bit."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch.utils.data import default_collate

import stroke_prediction_amd  # noqa: F401
from gather_ref import gather_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "stroke-prediction_amd")
DEV = "cuda:0"


def _i3(v):
    return (ctypes.c_int32 * 3)(*[int(a) for a in v])


def _gather(img, lab, table, ext0, pad0, padval0, ext1, pad1, padval1, zyx, n_cases, misalign=False):
    """one launch on device copies of the numpy cache arrays -> (rc, dst0, dst1) as numpy; the outputs start as NaN, so an element
    the kernel leaves out shows.  ``misalign``: the outputs start 4 bytes behind a 16-byte boundary."""
    from stroke_prediction_amd.runtime import lib as L, ops as O
    B = len(table)
    tab = torch.tensor(table, dtype=torch.int32).reshape(-1, 5).to(DEV)

    def out(src, ext):
        if src is None:
            return None
        shape = (B, src.shape[1], ext[2], ext[1], ext[0])
        n = int(np.prod(shape))
        buf = torch.full((n + 4,), float("nan"), dtype=torch.float32, device=DEV)
        return buf[1:n + 1].view(shape) if misalign else buf[:n].view(shape)
    s0 = torch.from_numpy(img).to(DEV) if img is not None else None
    s1 = torch.from_numpy(lab).to(DEV) if lab is not None else None
    d0, d1 = out(s0, ext0), out(s1, ext1)
    Z, Y, X = zyx
    rc = L.load().sp_patch_gather_batch(O.ptr(s0), O.ptr(d0), s0.shape[1] if s0 is not None else 0, _i3(ext0), _i3(pad0), padval0,
                                        O.ptr(s1), O.ptr(d1), s1.shape[1] if s1 is not None else 0, _i3(ext1), _i3(pad1), padval1,
                                        O.ptr(tab), n_cases, B, Z, Y, X, O.stream())
    torch.cuda.synchronize()
    return rc, (d0.cpu().numpy() if d0 is not None else None), (d1.cpu().numpy() if d1 is not None else None)


def _check(img, lab, table, ext0, pad0, padval0, ext1, pad1, padval1=0.0, **kw):
    src = img if img is not None else lab
    rc, got0, got1 = _gather(img, lab, table, ext0, pad0, padval0, ext1, pad1, padval1, src.shape[2:], src.shape[0], **kw)
    assert rc == 0
    want0, want1 = gather_ref(img, lab, table, ext0, pad0, padval0, ext1, pad1, padval1)
    for got, want in ((got0, want0), (got1, want1)):
        assert (got is None) == (want is None)
        if want is not None:
            assert got.shape == want.shape and np.array_equal(got, want)      # (NaN != NaN: an unwritten element fails here)


def _cache_arrays(N, C0, C1, zyx, seed):
    rs = np.random.RandomState(seed)
    img = rs.rand(N, C0, *zyx).astype(np.float32) if C0 else None
    lab = (rs.rand(N, C1, *zyx) > 0.5).astype(np.float32) if C1 else None      # labels: zeros in the data
    return img, lab


def test_kernel_scalar_path():
    """odd widths: one element per lane.  Pad value -7.5 differs from the zeros in the data."""
    img, lab = _cache_arrays(3, 2, 3, (5, 7, 13), 0)
    pad, ext0, ext1 = (3, 2, 1), (10, 6, 4), (4, 2, 2)
    table = [[0, 0, 0, 0, 0],            # origin (0, 0, 0)
             [1, 9, 5, 3, 1],            # the maximal origin, flipped
             [1, 4, 2, 1, 1],            # interior, flipped, the same case again
             [2, 19, 0, 0, 0]]           # x window [16, 26) of the padded volume: wholly inside the padding
    _check(img, lab, table, ext0, pad, -7.5, ext1, (0, 0, 0))


@pytest.mark.parametrize("aligned", [True, False])
def test_kernel_vector_path(aligned):
    """X = 16, w = 12 (labels w = 4): 16-byte stores; origins with ox - px a multiple of 4 also load 16 bytes at once"""
    img, lab = _cache_arrays(3, 2, 3, (5, 7, 16), 1)
    pad, ext0, ext1 = (4, 2, 1), (12, 6, 4), (4, 2, 2)
    xs = [0, 4, 8, 12] if aligned else [1, 3, 6, 11]
    table = [[b % 3, ox, (2 * b) % 6, b % 4, flip] for b, ox in enumerate(xs) for flip in (0, 1)]
    _check(img, lab, table, ext0, pad, -7.5, ext1, (0, 0, 0))


def test_kernel_vector_width_on_a_misaligned_output_takes_the_scalar_path():
    img, lab = _cache_arrays(2, 2, 3, (5, 7, 16), 2)
    table = [[0, 4, 1, 0, 0], [1, 7, 3, 2, 1], [1, 12, 5, 3, 1]]
    _check(img, lab, table, (12, 6, 4), (4, 2, 1), -7.5, (4, 2, 2), (0, 0, 0), misalign=True)


def test_kernel_whole_volume_and_empty_groups():
    from stroke_prediction_amd.runtime import lib as L
    img, lab = _cache_arrays(3, 2, 3, (5, 7, 13), 3)
    vol = (13, 7, 5)
    table = [[2, 0, 0, 0, 1], [0, 0, 0, 0, 0], [2, 0, 0, 0, 0]]
    # the whole-volume form of the CAE loaders: pad 0, extents = the volume, no images (the labels travel as group 1)
    _check(None, lab, table, vol, (0, 0, 0), 0.0, vol, (0, 0, 0))
    # no labels
    _check(img, None, table, (10, 6, 4), (3, 2, 1), -7.5, (4, 2, 2), (0, 0, 0))
    # several workgroups per volume and a volume count that is no multiple of anything: 40 x 33 x 9 outputs, B = 5
    big_i, big_l = _cache_arrays(2, 1, 2, (9, 33, 40), 4)
    _check(big_i, big_l, [[b % 2, b, b % 3, b % 2, b % 2] for b in range(5)], (40, 33, 9), (2, 1, 1), 1.5, (36, 31, 7), (0, 0, 0))
    # both groups empty, and the other rejected argument sets
    rc, _, _ = _gather(None, None, table, vol, (0, 0, 0), 0.0, vol, (0, 0, 0), 0.0, (5, 7, 13), 3)
    assert rc == L.CONSTS["SP_EINVAL"] and "both groups are empty" in L.last_error()
    rc, _, _ = _gather(img, lab, table, (10, 0, 4), (3, 2, 1), 0.0, (4, 2, 2), (0, 0, 0), 0.0, (5, 7, 13), 3)
    assert rc == L.CONSTS["SP_EINVAL"] and "must be positive" in L.last_error()
    rc, _, _ = _gather(img, lab, table, (10, 6, 4), (3, 2, 1), 0.0, (4, 2, 2), (0, 0, 0), 0.0, (5, 7, 13), 0)
    assert rc == L.CONSTS["SP_EINVAL"] and "N >= 1" in L.last_error()


def test_kernel_rejects_a_batch_beyond_the_grid_limit():
    """B * C * workgroups per volume >= 2^31: refused on the host, nothing is launched (the pointers are never read)"""
    from stroke_prediction_amd.runtime import lib as L, ops as O
    one = torch.zeros(64, dtype=torch.float32, device=DEV)
    tab = torch.zeros(5, dtype=torch.int32, device=DEV)
    big = (4096, 512, 256)      # 2^29 outputs per volume, 2^19 vector workgroups
    args = lambda B: (O.ptr(one), O.ptr(one), 1, _i3(big), _i3((0, 0, 0)), 0.0, None, None, 0, None, None, 0.0, O.ptr(tab), 1, B, 1, 1, 1,
                      O.stream())
    assert L.load().sp_patch_gather_batch(*args(4096)) == L.CONSTS["SP_EINVAL"] and "grid limit" in L.last_error()
    assert L.load().sp_patch_gather_batch(*args(0)) == L.CONSTS["SP_EINVAL"]


# ------------------------------------------------------------------------------------------------ loader against the chain

def _datasets(D, chain, modalities, labels, n_cases=6):
    """the per-sample data set of the existing loader and a cache over the same cases (32 x 32 x 6 synthetic, resampled to 16)"""
    kw = dict(modalities=modalities, labels=labels, xy=32, z=6, n_cases=n_cases)
    per_sample = D.SyntheticStrokeDataset3D(transform=D.Compose(chain, device=DEV), **kw)
    cache = D.DeviceCaseCache(D.SyntheticStrokeDataset3D(transform=D.Compose(D._cache_prefix([chain]), device=DEV), **kw), DEV)
    return per_sample, cache


def _assert_same_batch(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        if isinstance(want[k], torch.Tensor):
            assert isinstance(got[k], torch.Tensor), k
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].device == want[k].device, k
            assert torch.equal(got[k], want[k]), k
        else:
            assert type(got[k]) is type(want[k]) and got[k] == want[k], k


def _unet_chain(D, flip):
    return [D.ResamplePlaneXY(0.5), flip, D.PadImages(4, 4, 2, pad_value=0), D.RandomPatch(16, 12, 6, 4, 4, 2), D.ToTensor()]


@pytest.mark.parametrize("kind", ["unet", "unet_random_flip", "cae_valid", "cae_flip"])
def test_loader_batch_equals_the_per_sample_chain(kind):
    from stroke_prediction_amd.common import data as D
    if kind.startswith("unet"):
        chain = _unet_chain(D, D.HemisphericFlip() if kind == "unet_random_flip" else D.HemisphericFlipFixedToCaseId(split_id=3))
        modalities, labels = ["a", "b"], ["x", "y"]
    else:
        chain = [D.ResamplePlaneXY(0.5)] + ([D.HemisphericFlip()] if kind == "cae_flip" else []) + [D.ToTensor()]
        modalities, labels = [], ["x", "y", "z"]
    per_sample, cache = _datasets(D, chain, modalities, labels)
    loader = D.CachedBatchLoader(cache, list(range(6)), 4, chain)
    items = [5, 0, 3, 3]
    random.seed(17)
    got = loader.make_batch(items)
    random.seed(17)
    want = default_collate([per_sample[i] for i in items])
    _assert_same_batch(got, want)
    assert loader.last_table.shape == (4, 5) and loader.last_table[:, 0].tolist() == items
    if kind.startswith("unet"):
        assert tuple(got["images"].shape) == (4, 2, 6, 12, 16) and tuple(got["labels"].shape) == (4, 2, 2, 4, 8)
    else:
        assert got["images"] == [] and tuple(got["labels"].shape) == (4, 3, 6, 16, 16)


def test_epochs_cover_every_item_once_and_draw_new_origins():
    from stroke_prediction_amd.common import data as D
    chain = _unet_chain(D, D.HemisphericFlipFixedToCaseId(split_id=3))
    _, cache = _datasets(D, chain, ["a", "b"], ["x", "y"], n_cases=5)
    loader = D.CachedBatchLoader(cache, [0, 1, 2, 3, 4], 2, chain)
    random.seed(0)
    epochs = []
    for _ in range(2):
        rows = []
        sizes = []
        for batch in loader:
            sizes.append(len(batch["case_id"]))
            assert batch["case_id"].tolist() == [cache.case_ids[s] for s in loader.last_table[:, 0].tolist()]
            rows += loader.last_table.tolist()
        assert sizes == [2, 2, 1] and len(loader) == 3
        assert sorted(r[0] for r in rows) == [0, 1, 2, 3, 4]
        epochs.append({r[0]: r[1:4] for r in rows})
    assert epochs[0] != epochs[1]


def test_device_cache_feeds_batch_elastic_deform(monkeypatch):
    """the factories with device_cache=True and batch_transform=BatchElasticDeform(noise="host") against the same transform on
    the existing loader's collated batch of the same cases, on equal generator states"""
    from stroke_prediction_amd.common import data as D
    monkeypatch.setenv("SP_SYNTHETIC_DATA", "1")
    labels = ["x", "y", "z"]
    train_tf = [D.ResamplePlaneXY(0.25), D.ToTensor()]
    bed = D.BatchElasticDeform(flip="random", noise="host")
    fold = [0, 1, 2, 3]
    train, valid = D.get_stroke_shape_training_data([], labels, train_tf, train_tf, fold, 0.5, batchsize=2, batch_transform=bed,
                                                    device_cache=True)
    assert isinstance(train, D.CachedBatchLoader) and isinstance(valid, D.CachedBatchLoader) and train.cache is valid.cache
    assert train.batch_transform is bed and valid.batch_transform is None and len(train.cache) == 4
    old_train, old_valid = D.get_stroke_shape_training_data([], labels, train_tf, train_tf, fold, 0.5, batchsize=2)
    assert sorted(train.sampler.indices) == sorted(old_train.sampler.indices)
    assert sorted(valid.sampler.indices) == sorted(old_valid.sampler.indices)
    items = list(train.sampler.indices)
    collated = default_collate([old_train.dataset[i] for i in items])      # (the synthetic cases seed RandomStates of their own)
    real = D.np.random.RandomState
    monkeypatch.setattr(D.np.random, "RandomState", lambda seed=None: real(9))      # the clock seed of every sample's noise
    random.seed(5)
    got = train.make_batch(items)
    random.seed(5)
    want = bed(collated)
    _assert_same_batch(got, want)
    assert tuple(got["labels"].shape) == (2, 3, 28, 64, 64)
    monkeypatch.undo()
    monkeypatch.setenv("SP_SYNTHETIC_DATA", "1")
    plain = valid.make_batch(list(valid.sampler.indices))
    _assert_same_batch(plain, default_collate([old_valid.dataset[i] for i in valid.sampler.indices]))


def test_train_unet_segmentation_script_with_devicecache(tmp_path):
    base = str(tmp_path / "unet")
    unetpath = str(tmp_path / "unet.model")
    env = dict(os.environ, SP_SYNTHETIC_DATA="1", MPLBACKEND="Agg")
    r = subprocess.run([sys.executable, os.path.join(PKG, "train_unet_segmentation.py"), unetpath, "--devicecache", "--graph", "--fusedadam",
                        "--epochs", "1", "--batchsize", "2", "--fold"] + [str(i) for i in range(8)] + ["--outbasepath", base],
                       capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "devicecache=True" in r.stdout and "Epoch 1/1 training loss" in r.stdout
    assert "Size training set: 4 samples | Size validation set: 4 samples" in r.stdout
    for f in (base + "_unet.model", base + "_unet_final.model", unetpath):
        assert os.path.exists(f), f
