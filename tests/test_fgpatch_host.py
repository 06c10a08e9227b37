"""Foreground-oversampled patch origins (common/data.py: ForegroundOversample, csrc/sp_fgpatch.hip), the parts that need no GPU: the
C ABI, the numpy restatement against ``np.flatnonzero``, the sampler's draws, the loader's and the factories' argument checks and
the command-line flags."""
import inspect
import random

import numpy as np
import pytest
import torch

import stroke_prediction_amd  # noqa: F401
import fgpatch_ref as R


def test_header_declares_both_entry_points():
    import os
    from stroke_prediction_amd.runtime import lib as L
    with open(L.HEADER) as f:
        _, sigs, _ = L.parse_header(f.read())
    i32, f32, vp = L.i32, L.f32, L.vp
    assert sigs["sp_fg_row_index"] == ([vp, i32, i32, i32, i32, i32, i32, f32, vp, vp], i32)
    assert sigs["sp_patch_origins_fg"] == ([vp, vp, i32, i32, i32, i32, i32, i32, f32, vp, vp, vp, vp, vp, i32, vp], i32)
    assert "sp_fgpatch.hip" in L.SOURCES and os.path.isfile(os.path.join(L.CSRC_DIR, "sp_fgpatch.hip"))


def test_ref_picks_flatnonzero_k_and_places_it_at_j():
    rs = np.random.RandomState(3)
    N, C1, Z, Y, X = 2, 2, 4, 9, 11
    labels = (rs.rand(N, C1, Z, Y, X) < 0.2).astype(np.float32)
    ext1, omax = (5, 4, 2), (X + 6 - 11, Y + 6 - 10, Z + 2 - 4)      # pad (3, 3, 1), patch (11, 10, 4): crop = pad
    for chanmask in (1, 2, 3):
        mask = R.fg_mask(labels, chanmask, 0.5)
        prefix = R.row_prefix(labels, chanmask, 0.5)
        assert prefix.dtype == np.int32 and prefix.shape == (N, Z * Y + 1) and np.all(prefix[:, 0] == 0)
        assert prefix[:, -1].tolist() == [int(mask[n].sum()) for n in range(N)]
        for slot in range(N):
            flat = np.flatnonzero(mask[slot])
            total = flat.size
            for flip in (0, 1):
                table = [[slot, 99, 98, 97, flip]] * total
                draws = [[1, R.u_for(k, total), rs.randint(ext1[0]), rs.randint(ext1[1]), rs.randint(ext1[2])] for k in range(total)]
                got, picked = R.resolve(labels, table, draws, ext1, omax, chanmask, 0.5)
                assert picked[:, 0].tolist() == list(range(total))
                assert ((picked[:, 3] * Y + picked[:, 2]) * X + picked[:, 1]).tolist() == flat.tolist()
                # the row of the prefix that holds k
                rows = picked[:, 3] * Y + picked[:, 2]
                assert np.all(prefix[slot][rows] <= picked[:, 0]) and np.all(picked[:, 0] < prefix[slot][rows + 1])
                unclamped = 0
                for b in range(total):
                    f = np.array([X - 1 - picked[b, 1] if flip else picked[b, 1], picked[b, 2], picked[b, 3]])
                    j, o = np.array(draws[b][2:]), got[b, 1:4]
                    assert np.all(o >= 0) and np.all(o <= omax)
                    assert np.all(f - o >= 0) and np.all(f - o < ext1)      # inside the label patch, clamped or not
                    if np.all(f - j >= 0) and np.all(f - j <= omax):
                        unclamped += 1
                        assert np.array_equal(f - o, j)
                    assert got[b, 0] == slot and got[b, 4] == flip
                assert unclamped > 0
    # untouched rows: not forced, an empty case, a slot outside the cache
    labels[1] = 0
    table = [[0, 1, 2, 3, 0], [1, 1, 2, 3, 1], [-1, 1, 2, 3, 0], [N, 1, 2, 3, 0], [0, 1, 2, 3, 0]]
    draws = [[0, 5, 0, 0, 0], [1, 5, 0, 0, 0], [1, 5, 0, 0, 0], [1, 5, 0, 0, 0], [1, 0, 0, 0, 0]]
    got, picked = R.resolve(labels, table, draws, ext1, omax, 3, 0.5)
    assert got[:4].tolist() == table[:4] and np.all(picked[:4] == -1) and picked[4, 0] == 0
    # strictly above the threshold
    assert R.row_prefix(np.full((1, 1, 1, 1, 3), 0.5, np.float32), 1, 0.5)[0].tolist() == [0, 0]
    assert R.row_prefix(np.full((1, 1, 1, 1, 3), 0.5, np.float32), 1, 0.0)[0].tolist() == [0, 3]


@pytest.mark.parametrize("total", [1, 7, 1000])
def test_u_for_round_trips(total):
    for k in range(total):
        u = R.u_for(k, total)
        assert 0 <= u < 1 << 32 and (u * total) >> 32 == k
        assert u == 0 or ((u - 1) * total) >> 32 == k - 1      # the smallest such u
    assert (((1 << 32) - 1) * total) >> 32 == total - 1


def test_foreground_oversample_validation():
    from stroke_prediction_amd.common import data as D
    fg = D.ForegroundOversample()
    assert abs(fg.fraction - 1 / 3) < 1e-12 and fg.channels is None and fg.threshold == 0.5
    assert D.ForegroundOversample(0).fraction == 0 and D.ForegroundOversample(1, channels=(1, 0)).channels == [1, 0]
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="fraction"):
            D.ForegroundOversample(bad)
    with pytest.raises(ValueError, match="channels"):
        D.ForegroundOversample(0.5, channels=[0, -1])
    with pytest.raises(ValueError, match="channels"):
        D.ForegroundOversample(0.5, channels=[1, 1])


def test_draws_are_the_objects_own():
    from stroke_prediction_amd.common import data as D
    a, b = D.ForegroundOversample(0.5, seed=11), D.ForegroundOversample(0.5, seed=11)
    random.seed(2)
    state = random.getstate()
    ext1 = (8, 4, 2)
    da = [a.draw(64, ext1) for _ in range(3)]
    assert random.getstate() == state
    db = [b.draw(64, ext1) for _ in range(3)]
    for x, y in zip(da, db):
        assert x.dtype == np.int32 and x.shape == (64, 5) and np.array_equal(x, y)
    assert not np.array_equal(da[0], da[1])
    d = np.concatenate(da)
    assert set(d[:, 0].tolist()) == {0, 1}
    for axis, e in enumerate(ext1):
        assert d[:, 2 + axis].min() == 0 and d[:, 2 + axis].max() == e - 1
    u = d[:, 1].astype(np.int64) & 0xFFFFFFFF
    assert u.max() >= 1 << 31 and u.min() < 1 << 31      # the whole 32-bit range, carried as int32 bits
    # the same number of draws whatever the tosses say: fractions 0 and 1 leave the generator in the same state
    lo, hi = D.ForegroundOversample(0.0, seed=5), D.ForegroundOversample(1.0, seed=5)
    x, y = lo.draw(9, ext1), hi.draw(9, ext1)
    assert not x[:, 0].any() and y[:, 0].all() and np.array_equal(x[:, 1:], y[:, 1:])
    assert np.array_equal(lo.draw(9, ext1)[:, 1:], hi.draw(9, ext1)[:, 1:])


@pytest.fixture()
def host_cache():
    from stroke_prediction_amd.common import data as D
    ds = D.SyntheticStrokeDataset3D(modalities=["a", "b"], labels=["x", "y"], transform=D.Compose([D.ResamplePlaneXY(0.5)]),
                                    xy=32, z=6, n_cases=3)
    return D, D.DeviceCaseCache(ds, device=None)


def test_loader_argument_errors(host_cache):
    D, cache = host_cache
    chain = lambda pad, crop: [D.ResamplePlaneXY(0.5), D.PadImages(*pad), D.RandomPatch(12, 12, 6, *crop), D.ToTensor()]
    fg = D.ForegroundOversample(0.5, seed=1)
    loader = D.CachedBatchLoader(cache, [0, 1, 2], 2, chain((4, 4, 2), (4, 4, 2)), foreground=fg)
    assert loader.foreground is fg and loader.last_table_device is None
    assert D.CachedBatchLoader(cache, [0, 1, 2], 2, chain((4, 4, 2), (4, 4, 2))).foreground is None
    D.CachedBatchLoader(cache, [0, 1, 2], 2, chain((4, 4, 2), (3, 4, 0)), foreground=fg)           # crop below the padding: fine
    with pytest.raises(ValueError, match="RandomPatch"):
        D.CachedBatchLoader(cache, [0, 1, 2], 2, [D.ResamplePlaneXY(0.5), D.ToTensor()], foreground=fg)
    with pytest.raises(ValueError, match="channel 2 of 2"):
        D.CachedBatchLoader(cache, [0, 1, 2], 2, chain((4, 4, 2), (4, 4, 2)), foreground=D.ForegroundOversample(0.5, channels=[0, 2]))
    with pytest.raises(ValueError, match="PadImages' pad"):
        D.CachedBatchLoader(cache, [0, 1, 2], 2, chain((4, 4, 1), (4, 4, 2)), foreground=fg)
    with pytest.raises(ValueError, match="PadImages' pad"):
        D.CachedBatchLoader(cache, [0, 1, 2], 2, [D.RandomPatch(12, 12, 6, 1, 0, 0), D.ToTensor()], foreground=fg)
    no_labels = D.DeviceCaseCache(D.SyntheticStrokeDataset3D(modalities=["a"], labels=[], xy=16, z=6, n_cases=2), device=None)
    with pytest.raises(ValueError, match="labels"):
        D.CachedBatchLoader(no_labels, [0, 1], 2, [D.PadImages(4, 4, 2), D.RandomPatch(12, 12, 6, 4, 4, 2), D.ToTensor()], foreground=fg)
    with pytest.raises(ValueError, match="no labels"):
        no_labels.foreground_index()
    with pytest.raises(RuntimeError):      # the index is built by a kernel: no CPU path
        cache.foreground_index()


def test_factories_take_foreground(monkeypatch):
    from stroke_prediction_amd.common import data as D
    monkeypatch.setenv("SP_SYNTHETIC_DATA", "1")
    for fn in (D.split_data_loader3D, D.single_data_loader3D, D.get_stroke_shape_training_data, D.get_stroke_prediction_training_data):
        assert inspect.signature(fn).parameters["foreground"].default is None
    assert inspect.signature(D.CachedBatchLoader.__init__).parameters["foreground"].default is None
    tf = [D.ToTensor()]
    fg = D.ForegroundOversample(0.5, seed=1)
    with pytest.raises(ValueError, match="foreground needs device_cache=True"):
        D.get_stroke_shape_training_data([], ["a", "b"], tf, tf, [0, 1, 2, 3], 0.5, batchsize=2, foreground=fg)
    with pytest.raises(ValueError, match="foreground needs device_cache=True"):
        D.get_stroke_shape_training_data([], ["a", "b"], tf, None, [0, 1, 2, 3], 0.5, batchsize=2, split=False, foreground=fg)
    with pytest.raises(ValueError, match="foreground needs device_cache=True"):
        D.single_data_loader3D([], ["a"], [0, 1], 2, train_transform=tf, foreground=fg)
    with pytest.raises(ValueError, match="foreground needs device_cache=True"):
        D.split_data_loader3D([], ["a"], [0, 1], 2, train_transform=tf, valid_transform=tf, foreground=fg)


def test_parsers(capsys):
    from common import util
    ns = util.get_args_unet_training(["/tmp/unet.model"])
    assert ns.fgfraction == 0.0 and ns.fgchannels is None
    ns = util.get_args_unet_training(["/tmp/unet.model", "--devicecache", "--fgfraction", "0.33", "--fgchannels", "0", "1"])
    assert ns.fgfraction == 0.33 and ns.fgchannels == [0, 1]
    assert util.get_args_unet_training(["/tmp/unet.model", "--fgfraction", "0"]).fgfraction == 0.0      # off needs no cache
    capsys.readouterr()
    with pytest.raises(SystemExit):
        util.get_args_unet_training(["/tmp/unet.model", "--fgfraction", "0.5"])
    assert "--fgfraction needs --devicecache" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        util.get_args_unet_training(["/tmp/unet.model", "--devicecache", "--fgfraction", "1.5"])
    capsys.readouterr()
    # the CAE scripts gather whole volumes: no such flag
    for parse, pos in ((util.get_args_shape_training, []), (util.get_args_step_training, ["/tmp/cae.model"]),
                       (util.get_args_shape_prediction_training, ["/tmp/cae.model"])):
        assert not hasattr(parse(pos), "fgfraction")
        with pytest.raises(SystemExit):
            parse(pos + ["--fgfraction", "0.5"])
        assert "unrecognized arguments" in capsys.readouterr().err
