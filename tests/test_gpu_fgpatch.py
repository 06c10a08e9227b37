"""Foreground-oversampled patch origins on the device (csrc/sp_fgpatch.hip: sp_fg_row_index, sp_patch_origins_fg; common/data.py:
DeviceCaseCache.foreground_index, ForegroundOversample, CachedBatchLoader(foreground=...)) against the numpy restatement
(tests/fgpatch_ref.py).  Every comparison is exact integer (or bit) equality."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import stroke_prediction_amd  # noqa: F401
import fgpatch_ref as R
from gather_ref import gather_group

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "stroke-prediction_amd")
DEV = "cuda:0"
SHAPES = [(3, 5, 70),       # two lane chunks, the second partial
          (2, 3, 7),        # less than one chunk, X no multiple of 4
          (2, 2, 128),      # two full chunks
          (5, 67, 8)]       # Z * Y = 335: no multiple of 64 or 256, two chunks of the scan


def _i3(v):
    return (ctypes.c_int32 * 3)(*[int(a) for a in v])


def _i32(u):
    return u - (1 << 32) if u >= (1 << 31) else u


def _random_case(rs, C1, zyx):
    """values 0, 0.5 and 1: density 0.3 above the threshold 0.5, and values exactly AT the thresholds 0.5 and 0.0"""
    return rs.choice(np.array([0.0, 0.5, 1.0], dtype=np.float32), size=(C1,) + tuple(zyx), p=[0.5, 0.2, 0.3])


def _labels(zyx, planted, seed=0, C1=2):
    """N = 3: one random case and two planted ones"""
    rs = np.random.RandomState(seed)
    Z, Y, X = zyx
    lab = np.zeros((3, C1) + tuple(zyx), dtype=np.float32)
    lab[0] = _random_case(rs, C1, zyx)
    if planted == "empty_full":
        lab[2] = 1.0
    else:
        lab[1, 0, 0, 0, 0] = 1.0                      # its only voxel is (0, 0, 0), in channel 0
        lab[2, 1, Z - 1, Y - 1, X - 1] = 1.0          # its only voxel is the last one, in channel 1
    return lab


def _index(lab_dev, chanmask, thr):
    from stroke_prediction_amd.runtime import lib as L, ops as O
    N, C1, Z, Y, X = lab_dev.shape
    prefix = torch.full((N, Z * Y + 1), -7, dtype=torch.int32, device=DEV)
    rc = L.load().sp_fg_row_index(O.ptr(lab_dev), N, C1, Z, Y, X, _i32(chanmask), thr, O.ptr(prefix), O.stream())
    assert rc == 0, L.last_error()
    return prefix


def _resolve(lab, table, draws, ext1, omax, chanmask, thr, lab_dev=None, prefix=None):
    """one sp_patch_origins_fg launch -> (table, picked) as int64 numpy"""
    from stroke_prediction_amd.runtime import lib as L, ops as O
    lab_dev = torch.from_numpy(lab).to(DEV) if lab_dev is None else lab_dev
    N, C1, Z, Y, X = lab_dev.shape
    prefix = _index(lab_dev, chanmask, thr) if prefix is None else prefix
    tab = torch.tensor(table, dtype=torch.int32).reshape(-1, 5).to(DEV)
    drw = torch.tensor([[f, _i32(u & 0xFFFFFFFF), jx, jy, jz] for f, u, jx, jy, jz in draws], dtype=torch.int32).to(DEV)
    B = tab.shape[0]
    picked = torch.full((B, 4), -9, dtype=torch.int32, device=DEV)
    rc = L.load().sp_patch_origins_fg(O.ptr(lab_dev), O.ptr(prefix), N, C1, Z, Y, X, _i32(chanmask), thr, O.ptr(drw), _i3(ext1), _i3(omax),
                                      O.ptr(tab), O.ptr(picked), B, O.stream())
    assert rc == 0, L.last_error()
    torch.cuda.synchronize()
    return tab.cpu().numpy().astype(np.int64), picked.cpu().numpy().astype(np.int64)


def _gather_labels(lab, table, ext1):
    """the label group of sp_patch_gather_batch (pad1 = 0) at the table's origins"""
    from stroke_prediction_amd.runtime import lib as L, ops as O
    N, C1, Z, Y, X = lab.shape
    src = torch.from_numpy(lab).to(DEV)
    tab = torch.tensor(np.asarray(table), dtype=torch.int32).reshape(-1, 5).to(DEV)
    B = tab.shape[0]
    dst = torch.full((B, C1, ext1[2], ext1[1], ext1[0]), float("nan"), dtype=torch.float32, device=DEV)
    rc = L.load().sp_patch_gather_batch(None, None, 0, None, None, 0.0, O.ptr(src), O.ptr(dst), C1, _i3(ext1), _i3((0, 0, 0)), 0.0, O.ptr(tab),
                                        N, B, Z, Y, X, O.stream())
    assert rc == 0, L.last_error()
    torch.cuda.synchronize()
    return dst.cpu().numpy()


# ------------------------------------------------------------------------------------------------ the index

@pytest.mark.parametrize("planted", ["empty_full", "corners"])
@pytest.mark.parametrize("zyx", SHAPES)
def test_row_index_equals_the_cumsum(zyx, planted):
    lab = _labels(zyx, planted)
    lab_dev = torch.from_numpy(lab).to(DEV)
    for chanmask in (1, 2, 3):
        for thr in (0.5, 0.0):
            got = _index(lab_dev, chanmask, thr).cpu().numpy()
            want = R.row_prefix(lab, chanmask, thr)
            assert got.dtype == want.dtype and np.array_equal(got, want), (chanmask, thr)
    # at threshold 0.5 the 0.5s do not count, at 0.0 they do and the zeros do not
    assert R.row_prefix(lab, 3, 0.0)[0, -1] > R.row_prefix(lab, 3, 0.5)[0, -1] > 0
    assert R.row_prefix(lab, 3, 0.0)[0, -1] < lab[0, 0].size


def test_row_index_rejects_bad_arguments():
    from stroke_prediction_amd.runtime import lib as L, ops as O
    lab = torch.zeros((1, 2, 2, 2, 4), dtype=torch.float32, device=DEV)
    prefix = torch.zeros((1, 5), dtype=torch.int32, device=DEV)
    call = lambda C1, mask: L.load().sp_fg_row_index(O.ptr(lab), 1, C1, 2, 2, 4, mask, 0.5, O.ptr(prefix), O.stream())
    assert call(2, 4) == L.CONSTS["SP_EINVAL"] and "selects no channel" in L.last_error()      # bit 2 with two channels
    assert call(2, 0) == L.CONSTS["SP_EINVAL"]
    assert call(33, 1) == L.CONSTS["SP_EINVAL"] and call(0, 1) == L.CONSTS["SP_EINVAL"]
    assert call(2, 5) == 0                                                                        # bit 0 counts, bit 2 is ignored
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ resolving a voxel

PAD, EXT0 = (3, 2, 1), (30, 7, 3)
EXT1 = tuple(e - 2 * p for e, p in zip(EXT0, PAD))      # (24, 3, 1)


def _omax(zyx, pad=PAD, ext0=EXT0):
    Z, Y, X = zyx
    return tuple(n + 2 * p - e for n, p, e in zip((X, Y, Z), pad, ext0))


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("chanmask", [1, 3])
def test_every_k_resolves_to_flatnonzero_order(chanmask, flip):
    zyx = (3, 5, 70)
    lab = _labels(zyx, "empty_full", seed=1)
    Z, Y, X = zyx
    flat = np.flatnonzero(R.fg_mask(lab, chanmask, 0.5)[0])
    total = flat.size
    assert 200 < total < 800
    rs = np.random.RandomState(5)
    us = [R.u_for(k, total) for k in range(total)] + [0, (1 << 32) - 1]
    B = len(us)
    table = [[0, 40, 1, 1, flip] for _ in range(B)]
    draws = [[1, u, rs.randint(EXT1[0]), rs.randint(EXT1[1]), rs.randint(EXT1[2])] for u in us]
    got_table, got_picked = _resolve(lab, table, draws, EXT1, _omax(zyx), chanmask, 0.5)
    want_table, want_picked = R.resolve(lab, table, draws, EXT1, _omax(zyx), chanmask, 0.5)
    assert np.array_equal(got_picked, want_picked) and np.array_equal(got_table, want_table)
    assert got_picked[:, 0].tolist() == list(range(total)) + [0, total - 1]
    assert ((got_picked[:total, 3] * Y + got_picked[:total, 2]) * X + got_picked[:total, 1]).tolist() == flat.tolist()
    assert (got_picked[:total, 1] == 63).any() and (got_picked[:total, 1] == 64).any() and (got_picked[:total, 1] == 69).any()


@pytest.mark.parametrize("zyx", SHAPES)
def test_origins_clamp_and_keep_the_voxel_in_the_label_patch(zyx):
    """single voxels in opposite corners: j = 0 drives the origin into the upper clamp, j = ext1 - 1 into the lower one, on every
    axis (with the mirror swapping the two along x); an out-of-range j is clamped by the kernel"""
    Z, Y, X = zyx
    pad = (2, 1, 1)
    ext0 = (min(X + 2, 11), min(Y + 2, 5), 4)
    ext1 = tuple(e - 2 * p for e, p in zip(ext0, pad))
    omax = _omax(zyx, pad, ext0)
    assert min(ext1) >= 1 and min(omax) >= 0
    lab = _labels(zyx, "corners", seed=2)
    far = (1000, 1000, 1000)
    js = [(0, 0, 0), tuple(e - 1 for e in ext1), far, (-5, -5, -5), (far[0], -5, 0), (-5, far[1], far[2])]
    table = [[slot, 1, 0, 1, flip] for slot in (1, 2, 0) for flip in (0, 1) for _ in js]
    draws = [[1, 0x9E3779B9 * (b + 1), *js[b % len(js)]] for b in range(len(table))]
    got_table, got_picked = _resolve(lab, table, draws, ext1, omax, 3, 0.5)
    want_table, want_picked = R.resolve(lab, table, draws, ext1, omax, 3, 0.5)
    assert np.array_equal(got_table, want_table) and np.array_equal(got_picked, want_picked)
    assert np.all(got_picked[:, 0] >= 0)
    o = got_table[:, 1:4]
    for axis in range(3):      # both clamps act on every axis
        assert (o[:2 * len(js), axis] == 0).any() and (o[:4 * len(js), axis] == omax[axis]).any()
    # patch pad <= image pad: the gathered label patch shows the picked voxel, at f - o
    patches = _gather_labels(lab, got_table, ext1)
    assert not np.isnan(patches).any()
    for b, (slot, ox, oy, oz, flip) in enumerate(got_table.tolist()):
        k, fx, fy, fz = got_picked[b].tolist()
        p = ((X - 1 - fx if flip else fx) - ox, fy - oy, fz - oz)
        assert all(0 <= a < e for a, e in zip(p, ext1)), b
        assert patches[b, :, p[2], p[1], p[0]].max() == 1.0, b
        if slot in (1, 2):
            assert patches[b].sum() == 1.0
    assert np.array_equal(patches, gather_group(lab, got_table, ext1, (0, 0, 0), 0.0))


def test_untouched_rows_come_back_bit_identical():
    zyx = (3, 5, 70)
    lab = _labels(zyx, "empty_full", seed=3)          # case 1 is empty
    N = lab.shape[0]
    table = [[0, 11, 1, 0, 0],      # forced
             [0, 12, 2, 1, 1],      # not forced
             [1, 13, 0, 2, 0],      # forced, empty case
             [2, 14, 1, 1, 1],      # forced
             [-1, 15, 2, 0, 0],     # forced, slot below the cache
             [N, 16, 0, 1, 1],      # forced, slot behind the cache
             [0, 17, 1, 2, 1],      # forced
             [2, 18, 2, 2, 0]]      # not forced
    draws = [[1, 123456789, 3, 1, 0], [0, 5, 1, 1, 0], [1, 6, 2, 2, 0], [1, 4000000000, 0, 0, 0], [1, 7, 1, 0, 0], [1, 8, 2, 1, 0],
             [1, 99, 23, 2, 0], [0, 9, 0, 0, 0]]
    got_table, got_picked = _resolve(lab, table, draws, EXT1, _omax(zyx), 3, 0.5)
    want_table, want_picked = R.resolve(lab, table, draws, EXT1, _omax(zyx), 3, 0.5)
    assert np.array_equal(got_table, want_table) and np.array_equal(got_picked, want_picked)
    for b in (1, 2, 4, 5, 7):
        assert got_table[b].tolist() == table[b] and got_picked[b].tolist() == [-1] * 4
    for b in (0, 3, 6):
        assert got_picked[b, 0] >= 0 and got_table[b, 1:4].tolist() != table[b][1:4]
        assert got_table[b, 0] == table[b][0] and got_table[b, 4] == table[b][4]


def test_stale_index_leaves_the_row_untouched():
    zyx = (3, 5, 70)
    lab = _labels(zyx, "empty_full", seed=4)
    lab_dev = torch.from_numpy(lab).to(DEV)
    prefix = _index(lab_dev, 3, 0.5)
    lab_dev[0].zero_()                                   # the labels change under the index
    total = int(R.row_prefix(lab, 3, 0.5)[0, -1])
    table = [[0, 9, 1, 1, b & 1] for b in range(8)] + [[2, 9, 1, 1, 0]]
    draws = [[1, R.u_for(k, total), 2, 1, 0] for k in np.linspace(0, total - 1, 8).astype(int)] + [[1, 77, 2, 1, 0]]
    got_table, got_picked = _resolve(lab, table, draws, EXT1, _omax(zyx), 3, 0.5, lab_dev=lab_dev, prefix=prefix)      # asserts rc == 0
    assert got_table[:8].tolist() == table[:8] and np.all(got_picked[:8] == -1)
    assert got_picked[8, 0] >= 0                          # the neighbour whose case did not change is resolved


# ------------------------------------------------------------------------------------------------ the loader

LPAD, LPATCH = (4, 4, 2), (12, 12, 6)
LEXT1 = tuple(e - 2 * p for e, p in zip(LPATCH, LPAD))      # (4, 4, 2)
LOMAX = (16 + 2 * 4 - 12, 16 + 2 * 4 - 12, 6 + 2 * 2 - 6)      # padded - patch = (12, 12, 4)


def _chain(D):
    return [D.ResamplePlaneXY(0.5), D.HemisphericFlipFixedToCaseId(split_id=2), D.PadImages(*LPAD, pad_value=0),
            D.RandomPatch(*LPATCH, *LPAD), D.ToTensor()]


@pytest.fixture(scope="module")
def small_cache():
    """four synthetic cases of 16 x 16 x 6 (32 x 32 resampled by 0.5), two image and two label channels"""
    from stroke_prediction_amd.common import data as D
    ds = D.SyntheticStrokeDataset3D(modalities=["a", "b"], labels=["x", "y"], transform=D.Compose([D.ResamplePlaneXY(0.5)], device=DEV),
                                    xy=32, z=6, n_cases=4)
    cache = D.DeviceCaseCache(ds, DEV)
    lab = cache.labels.cpu().numpy()
    assert lab.shape == (4, 2, 6, 16, 16) and all(R.fg_mask(lab, 3, 0.5)[n].any() for n in range(4))
    return D, cache, lab


def _augment(D, route):
    return D.PatchAugment(p_affine=0, p_elastic=0, p_intensity=0, label_threshold=None, seed=3) if route == "sample" else None


def _batches(loader, n, seed):
    """n batches of four random items under a fixed ``random`` state -> (batches, host tables, device tables as int64 numpy)"""
    random.seed(seed)
    out = []
    for _ in range(n):
        items = [random.randrange(4) for _ in range(4)]
        batch = loader.make_batch(items)
        out.append((batch, loader.last_table.clone(), loader.last_table_device.cpu().numpy().astype(np.int64)))
    return out


@pytest.mark.parametrize("route", ["gather", "sample"])
def test_loader_fraction_one_puts_foreground_into_every_patch(small_cache, route):
    D, cache, lab = small_cache
    loader = D.CachedBatchLoader(cache, [0, 1, 2, 3], 4, _chain(D), patch_augment=_augment(D, route),
                                 foreground=D.ForegroundOversample(1.0, seed=8))
    assert loader._ext1 == LEXT1 and loader._omax == LOMAX
    twin = D.ForegroundOversample(1.0, seed=8)
    at_j = 0
    for batch, host, dev in _batches(loader, 20, seed=1):
        draws = twin.draw(4, LEXT1)
        want, picked = R.resolve(lab, host.numpy(), draws, LEXT1, LOMAX, 3, 0.5)
        assert np.array_equal(dev, want) and np.all(picked[:, 0] >= 0)
        assert not np.array_equal(dev, host.numpy())                 # last_table stays as drawn
        labels = batch["labels"].cpu().numpy()
        assert labels.shape == (4, 2, LEXT1[2], LEXT1[1], LEXT1[0])
        assert np.array_equal(labels, gather_group(lab, dev, LEXT1, (0, 0, 0), 0.0))
        for b in range(4):
            assert labels[b].max() > 0.5, b
            fx, fy, fz = picked[b, 1:]
            f = np.array([15 - fx if dev[b, 4] else fx, fy, fz])
            j = draws[b, 2:5]
            if np.array_equal(f - j, dev[b, 1:4]):                   # nothing clamped: the voxel sits at j
                at_j += 1
                assert labels[b, :, j[2], j[1], j[0]].max() > 0.5
        assert batch["case_id"].tolist() == [cache.case_ids[s] for s in host[:, 0].tolist()]
    assert at_j > 20


@pytest.mark.parametrize("route", ["gather", "sample"])
def test_loader_fraction_zero_equals_the_plain_loader(small_cache, route):
    D, cache, lab = small_cache
    plain = D.CachedBatchLoader(cache, [0, 1, 2, 3], 4, _chain(D))
    loader = D.CachedBatchLoader(cache, [0, 1, 2, 3], 4, _chain(D), patch_augment=_augment(D, route),
                                 foreground=D.ForegroundOversample(0.0, seed=8))
    for (got, host, dev), (want, host0, dev0) in zip(_batches(loader, 5, seed=2), _batches(plain, 5, seed=2)):
        assert torch.equal(host, host0) and np.array_equal(dev, dev0) and np.array_equal(dev, host.numpy())
        assert sorted(got) == sorted(want)
        for key in ("images", "labels", "clinical", "case_id", "clinical_idx"):
            assert got[key].dtype == want[key].dtype and torch.equal(got[key], want[key]), key


@pytest.mark.parametrize("route", ["gather", "sample"])
def test_loader_fraction_half_forces_some_rows_and_is_reproducible(small_cache, route):
    D, cache, lab = small_cache
    plain = D.CachedBatchLoader(cache, [0, 1, 2, 3], 4, _chain(D))
    make = lambda: D.CachedBatchLoader(cache, [0, 1, 2, 3], 4, _chain(D), patch_augment=_augment(D, route),
                                       foreground=D.ForegroundOversample(0.5, seed=9))
    first, second, base = _batches(make(), 10, seed=3), _batches(make(), 10, seed=3), _batches(plain, 10, seed=3)
    twin = D.ForegroundOversample(0.5, seed=9)
    forced = 0
    for (got, host, dev), (_, _, dev2), (want, host0, _) in zip(first, second, base):
        draws = twin.draw(4, LEXT1)
        assert torch.equal(host, host0) and np.array_equal(dev, dev2)
        assert np.array_equal(dev, R.resolve(lab, host.numpy(), draws, LEXT1, LOMAX, 3, 0.5)[0])
        for b in range(4):
            if draws[b, 0]:
                forced += 1
                assert got["labels"][b].max() > 0.5
            else:
                assert dev[b].tolist() == host[b].tolist()
                assert torch.equal(got["images"][b], want["images"][b]) and torch.equal(got["labels"][b], want["labels"][b])
    assert 8 <= forced <= 32


def test_foreground_index_is_built_once_per_key(small_cache):
    D, cache, lab = small_cache
    a = cache.foreground_index()
    assert a is cache.foreground_index(None, 0.5) and a is cache.foreground_index([0, 1]) and a is cache.foreground_index((1, 0), 0.5)
    b = cache.foreground_index([1])
    assert b is not a and b is cache.foreground_index([1])
    assert np.array_equal(a.cpu().numpy(), R.row_prefix(lab, 3, 0.5)) and np.array_equal(b.cpu().numpy(), R.row_prefix(lab, 2, 0.5))
    assert np.array_equal(cache.foreground_index([0], 0.0).cpu().numpy(), R.row_prefix(lab, 1, 0.0))
    with pytest.raises(ValueError, match="channel 2 of 2"):
        cache.foreground_index([2])


# ------------------------------------------------------------------------------------------------ the script

def test_train_unet_segmentation_script_with_fgfraction(tmp_path):
    base = str(tmp_path / "unet")
    unetpath = str(tmp_path / "unet.model")
    env = dict(os.environ, SP_SYNTHETIC_DATA="1", MPLBACKEND="Agg")
    r = subprocess.run([sys.executable, os.path.join(PKG, "train_unet_segmentation.py"), unetpath, "--devicecache", "--fgfraction", "0.5",
                        "--graph", "--fusedadam", "--epochs", "1", "--batchsize", "2", "--fold"] + [str(i) for i in range(8)] +
                       ["--outbasepath", base], capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "fgfraction=0.5" in r.stdout and "Epoch 1/1 training loss" in r.stdout
    for f in (base + "_unet.model", base + "_unet_final.model", unetpath):
        assert os.path.exists(f), f
