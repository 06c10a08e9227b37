"""Device-resident case cache (common/data.py: DeviceCaseCache / CachedBatchLoader, csrc/sp_gather.hip), the parts that need no
GPU: the C ABI, the numpy restatement of the gather against the recorded outputs of the reference's transform classes and against
the oracle chain, chain recognition, the order of the random draws, and the command-line flag."""
import inspect
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import stroke_prediction_amd  # noqa: F401
from gather_ref import gather_group, gather_ref
from oracle import transforms as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "transforms.npz")


def test_header_declares_the_entry_point():
    from stroke_prediction_amd.runtime import lib as L
    with open(L.HEADER) as f:
        _, sigs, _ = L.parse_header(f.read())
    i32, f32, vp = L.i32, L.f32, L.vp
    group = [vp, vp, i32, vp, vp, f32]
    assert sigs["sp_patch_gather_batch"] == (group + group + [vp, i32, i32, i32, i32, i32, vp], i32)
    assert "sp_gather.hip" in L.SOURCES and os.path.isfile(os.path.join(L.CSRC_DIR, "sp_gather.hip"))


def _cached(a):
    """(x, y, z, c) sample array -> one-case cache array (1, c, z, y, x)"""
    return np.ascontiguousarray(np.transpose(a, (3, 2, 1, 0)))[None]


def test_gather_ref_reproduces_the_reference_fixture():
    """PadImages(2, 3, 1, pad_value=7) and RandomPatch(12, 10, 6, 2, 3, 1) of the reference's own classes on one recorded case"""
    g = np.load(GOLD)
    img, lab = _cached(g["s_images"]), _cached(g["s_labels"])
    X, Y, Z = g["s_images"].shape[:3]
    # the pad step alone: the whole padded volume from origin 0
    pad = (2, 3, 1)
    got = gather_group(img, [[0, 0, 0, 0, 0]], (X + 4, Y + 6, Z + 2), pad, 7.0)
    assert np.array_equal(got[0], T.to_tensor_layout(g["s_pad_images"]))
    assert np.array_equal(gather_group(lab, [[0, 0, 0, 0, 0]], (X, Y, Z), (0, 0, 0), 0.0)[0], T.to_tensor_layout(g["s_pad_labels"]))
    # the patch step: three random.randint draws in x, y, z order after the recorded seed
    random.seed(int(g["s_patch_seed"]))
    o = (random.randint(0, 20 - 12), random.randint(0, 20 - 10), random.randint(0, 8 - 6))
    got0, got1 = gather_ref(img, lab, [[0, o[0], o[1], o[2], 0]], (12, 10, 6), (0, 0, 0), 0.0, (8, 4, 4), (0, 0, 0))
    assert np.array_equal(got0[0], T.to_tensor_layout(g["s_patch_images"]))
    assert np.array_equal(got1[0], T.to_tensor_layout(g["s_patch_labels"]))
    # pad + patch + ToTensor in one step: the same window of the padded volume has its origin shifted by the padding
    got0 = gather_group(img, [[0, o[0] + 2, o[1] + 3, o[2] + 1, 0]], (12, 10, 6), pad, 7.0)
    assert np.array_equal(got0[0], T.to_tensor_layout(g["s_patch_images"]))
    # the fixed flip of the recorded case, whole volume
    got = gather_group(img, [[0, 0, 0, 0, 1]], (X, Y, Z), (0, 0, 0), 0.0)
    assert np.array_equal(got[0], T.to_tensor_layout(g["s_flip_fixed_images"]))


def test_gather_ref_matches_the_oracle_chain_on_random_tables():
    rs = np.random.RandomState(11)
    N, X, Y, Z = 3, 13, 7, 5
    samples = [{"case_id": n, "images": rs.rand(X, Y, Z, 2).astype(np.float32), "labels": rs.rand(X, Y, Z, 3).astype(np.float32),
                "clinical": []} for n in range(N)]
    img = np.concatenate([_cached(s["images"]) for s in samples])
    lab = np.concatenate([_cached(s["labels"]) for s in samples])
    pad, (w, h, d) = (3, 2, 1), (10, 6, 4)
    ext1 = (w - 2 * pad[0], h - 2 * pad[1], d - 2 * pad[2])
    table = [[rs.randint(N), rs.randint(0, X + 2 * pad[0] - w + 1), rs.randint(0, Y + 2 * pad[1] - h + 1),
              rs.randint(0, Z + 2 * pad[2] - d + 1), rs.randint(2)] for _ in range(24)]
    table += [[0, 0, 0, 0, 1], [2, X + 2 * pad[0] - w, Y + 2 * pad[1] - h, Z + 2 * pad[2] - d, 1]]
    got0, got1 = gather_ref(img, lab, table, (w, h, d), pad, -7.5, ext1, (0, 0, 0))
    for b, (case, ox, oy, oz, flip) in enumerate(table):
        s = T.random_patch(T.pad_images(T.hemispheric_flip(samples[case], bool(flip)), pad, -7.5), w, h, d, pad, (ox, oy, oz))
        assert np.array_equal(got0[b], T.to_tensor_layout(s["images"])), b
        assert np.array_equal(got1[b], T.to_tensor_layout(s["labels"])), b
    # anything out of range reads as the pad value, whatever the origin; a case outside the cache too
    far = gather_group(img, [[0, 10 ** 9, 0, 0, 0], [1, -10 ** 9, -5, 2, 1], [7, 0, 0, 0, 0]], (4, 3, 2), (0, 0, 0), 2.5)
    assert np.all(far == 2.5)


def _chains(D):
    unet = [D.ResamplePlaneXY(0.5), D.HemisphericFlipFixedToCaseId(split_id=15), D.PadImages(20, 20, 20, pad_value=0),
            D.RandomPatch(104, 104, 68, 20, 20, 20), D.ToTensor()]
    cae_valid = [D.ResamplePlaneXY(0.5), D.ToTensor()]
    return unet, cae_valid


def test_chain_recognition():
    from stroke_prediction_amd.common import data as D
    unet, cae_valid = _chains(D)
    st = D._parse_chain(unet)
    assert [type(st[k]).__name__ for k in D._CHAIN_ORDER] == ["ResamplePlaneXY", "HemisphericFlipFixedToCaseId", "PadImages", "RandomPatch",
                                                               "ToTensor"]
    assert sorted(D._parse_chain(cae_valid)) == ["ResamplePlaneXY", "ToTensor"]
    assert sorted(D._parse_chain([D.HemisphericFlip(), D.ToTensor()])) == ["ToTensor", "flip"]
    with pytest.raises(ValueError, match=r"ElasticDeform.*batch_transform="):
        D._parse_chain([D.ResamplePlaneXY(0.5), D.HemisphericFlip(), D.ElasticDeform(), D.ToTensor()])
    with pytest.raises(ValueError, match="PadImages out of order"):
        D._parse_chain([D.RandomPatch(8, 8, 4, 1, 1, 1), D.PadImages(1, 1, 1), D.ToTensor()])
    with pytest.raises(ValueError, match="out of order"):
        D._parse_chain([D.HemisphericFlip(), D.HemisphericFlipFixedToCaseId(3), D.ToTensor()])
    with pytest.raises(ValueError, match="end in ToTensor"):
        D._parse_chain([D.ResamplePlaneXY(0.5)])
    with pytest.raises(ValueError, match="Compose"):
        D._parse_chain([D.Compose([D.ToTensor()]), D.ToTensor()])


@pytest.fixture()
def host_cache(monkeypatch):
    """a five-case cache in host memory and a numpy stand-in for the entry point"""
    from stroke_prediction_amd.common import data as D
    ds = D.SyntheticStrokeDataset3D(modalities=["a", "b"], labels=["x", "y", "z"], transform=D.Compose([D.ResamplePlaneXY(0.5)]),
                                    xy=32, z=6, n_cases=5)
    cache = D.DeviceCaseCache(ds, device=None)
    calls = []

    def stand_in(cache, table, ext0, pad0, padval0, ext1, pad1):
        calls.append(table.clone())
        a, b = gather_ref(cache.images.numpy(), cache.labels.numpy(), table.numpy(), ext0, pad0, padval0, ext1, pad1)
        return torch.from_numpy(a), torch.from_numpy(b), table
    monkeypatch.setattr(D, "_gather_launch", stand_in)
    return D, ds, cache, calls


def test_cache_holds_the_totensor_layout(host_cache):
    D, ds, cache, _ = host_cache
    assert tuple(cache.images.shape) == (5, 2, 6, 16, 16) and tuple(cache.labels.shape) == (5, 3, 6, 16, 16)
    assert tuple(cache.clinical.shape) == (5, 5, 1, 1, 1) and cache.clinical.dtype == torch.float32
    assert cache.case_ids == [1, 2, 3, 4, 5] and cache.clinical_idx == [0] * 5 and len(cache) == 5 and cache.shape_zyx == (6, 16, 16)
    assert cache.nbytes == 4 * (5 * 5 * 6 * 16 * 16 + 5 * 5)
    s = D.ToTensor()(ds[3])
    assert np.array_equal(cache.images[3].numpy(), np.asarray(s["images"], dtype=np.float32))
    assert np.array_equal(cache.labels[3].numpy(), np.asarray(s["labels"], dtype=np.float32))
    assert np.array_equal(cache.clinical[3].numpy(), np.asarray(s["clinical"], dtype=np.float32))
    part = D.DeviceCaseCache(ds, device=None, items=[4, 1])
    assert part.case_ids == [2, 5] and part.slot_of == {1: 0, 4: 1}

    class Ragged(object):
        def __len__(self):
            return 2

        def __getitem__(self, i):
            return D.synthetic_sample(i + 1, xy=16 + 16 * i, z=6)
    with pytest.raises(ValueError, match="same extents"):
        D.DeviceCaseCache(Ragged(), device=None)


def test_draw_order_matches_the_per_sample_classes(host_cache, monkeypatch):
    """random.random() of HemisphericFlip, then randint x, y, z of RandomPatch, sample after sample -- read back from the existing
    classes themselves: RandomPatch cuts a volume that holds its own coordinates, HemisphericFlip's toss is seen at _flip"""
    D, ds, cache, calls = host_cache
    pad, patch = (2, 3, 1), (12, 10, 6)
    chain = [D.ResamplePlaneXY(0.5), D.HemisphericFlip(), D.PadImages(*pad, pad_value=-1), D.RandomPatch(*patch, *pad), D.ToTensor()]
    loader = D.CachedBatchLoader(cache, [0, 1, 2, 3, 4], 3, chain)
    items = [4, 0, 2]
    random.seed(21)
    batch = loader.make_batch(items)
    after = random.random()
    # replay with the existing classes
    px, py, pz = 16 + 2 * pad[0], 16 + 2 * pad[1], 6 + 2 * pad[2]
    coords = np.stack(np.meshgrid(np.arange(px), np.arange(py), np.arange(pz), indexing="ij"), axis=3).astype(np.float32)
    flipped = []
    monkeypatch.setattr(D, "_flip", lambda sample: flipped.append(True) or sample)
    random.seed(21)
    want = []
    for item in items:
        n = len(flipped)
        s = D.HemisphericFlip()({"case_id": item + 1, "images": coords, "labels": coords, "clinical": []})
        p = D.RandomPatch(*patch, *pad)(s)
        want.append([item] + [int(v) for v in p["images"][0, 0, 0]] + [int(len(flipped) > n)])
    assert random.random() == after                      # the same number of draws
    assert loader.last_table.dtype == torch.int32 and loader.last_table.tolist() == want
    assert len(calls) == 1 and calls[0].tolist() == want
    assert any(r[4] for r in want) and not all(r[4] for r in want)      # seed 21 tosses both ways
    # the batch contract of the collated per-sample chain
    assert sorted(batch) == ["case_id", "clinical", "clinical_idx", "images", "labels"]
    assert batch["case_id"].tolist() == [5, 1, 3] and batch["case_id"].dtype == torch.int64 and batch["clinical_idx"].tolist() == [0, 0, 0]
    assert tuple(batch["images"].shape) == (3, 2, 6, 10, 12) and tuple(batch["labels"].shape) == (3, 3, 4, 4, 8)
    assert torch.equal(batch["clinical"], cache.clinical[[4, 0, 2]])
    # and its values: the oracle chain at the table's origins
    for b, (slot, ox, oy, oz, flip) in enumerate(want):
        raw = ds[slot]
        s = T.random_patch(T.pad_images(T.hemispheric_flip(raw, bool(flip)), pad, -1), *patch, pad, (ox, oy, oz))
        assert np.array_equal(batch["images"][b].numpy(), T.to_tensor_layout(s["images"]))
        assert np.array_equal(batch["labels"][b].numpy(), T.to_tensor_layout(s["labels"]))


def test_loader_surface_and_epochs(host_cache):
    D, ds, cache, calls = host_cache
    _, cae_valid = _chains(D)
    seen = []
    loader = D.CachedBatchLoader(cache, [3, 0, 4, 1, 2], 2, [D.HemisphericFlipFixedToCaseId(3)] + cae_valid[1:],
                                 batch_transform=lambda b: seen.append(len(b["case_id"])) or dict(b, marked=True))
    assert len(loader) == 3 and loader.batch_size == 2 and loader.dataset is ds and sorted(loader.sampler.indices) == [0, 1, 2, 3, 4]
    batches = list(loader)
    assert seen == [2, 2, 1] and all(b["marked"] for b in batches)
    assert sorted(int(c) for b in batches for c in b["case_id"]) == [1, 2, 3, 4, 5]
    for b in batches:      # whole volumes, flipped for case ids above 3
        assert tuple(b["labels"].shape[1:]) == (3, 6, 16, 16) and tuple(b["images"].shape[1:]) == (2, 6, 16, 16)
        for k, cid in enumerate(int(c) for c in b["case_id"]):
            want = cache.labels[cid - 1].flip(-1) if cid > 3 else cache.labels[cid - 1]
            assert torch.equal(b["labels"][k], want)
    with pytest.raises(ValueError, match="not in the cache"):
        D.CachedBatchLoader(cache, [0, 7], 2, cae_valid)
    with pytest.raises(ValueError, match="ElasticDeform"):
        D.CachedBatchLoader(cache, [0, 1], 2, [D.ElasticDeform(), D.ToTensor()])


def test_factories_take_device_cache(monkeypatch):
    from stroke_prediction_amd.common import data as D
    monkeypatch.setenv("SP_SYNTHETIC_DATA", "1")
    for fn in (D.split_data_loader3D, D.single_data_loader3D, D.get_stroke_shape_training_data, D.get_stroke_prediction_training_data):
        assert inspect.signature(fn).parameters["device_cache"].default is False
    if not torch.cuda.is_available():
        tf = [D.ToTensor()]
        with pytest.raises(RuntimeError, match="needs a GPU"):
            D.get_stroke_shape_training_data([], ["a", "b", "c"], tf, tf, [0, 1, 2, 3], 0.5, batchsize=2, device_cache=True)
        with pytest.raises(RuntimeError, match="needs a GPU"):
            D.single_data_loader3D([], ["a"], [0, 1], 2, train_transform=tf, device_cache=True)
    with pytest.raises(ValueError, match="resample differently"):
        D._cache_prefix([[D.ResamplePlaneXY(0.5), D.ToTensor()], [D.ToTensor()]])
    with pytest.raises(RuntimeError):      # the entry point has no CPU path
        cache = D.DeviceCaseCache(D.SyntheticStrokeDataset3D(labels=["a"], xy=16, z=4, n_cases=2), device=None)
        D.CachedBatchLoader(cache, [0, 1], 2, [D.ToTensor()]).make_batch([0, 1])


def test_parsers_take_devicecache(capsys):
    from common import util
    assert util.get_args_unet_training(["/tmp/unet.model"]).devicecache is False
    assert util.get_args_unet_training(["/tmp/unet.model", "--devicecache"]).devicecache is True
    assert util.get_args_sdm(["/tmp/unet.model"]).devicecache is False
    for parse, pos in ((util.get_args_shape_training, []), (util.get_args_step_training, ["/tmp/cae.model"]),
                       (util.get_args_shape_prediction_training, ["/tmp/cae.model"])):
        assert parse(pos).devicecache is False
        assert parse(pos + ["--devicecache", "--batchaugment"]).devicecache is True
        capsys.readouterr()
        with pytest.raises(SystemExit):
            parse(pos + ["--devicecache"])
        assert "--devicecache needs --batchaugment" in capsys.readouterr().err


def test_cae_script_refuses_devicecache_without_batchaugment():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "stroke-prediction_amd", "train_shape_reconstruction.py"), "--devicecache"],
                       capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode != 0 and "--devicecache needs --batchaugment" in r.stderr
