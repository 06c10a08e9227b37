"""Batch-level augmentation on the device (csrc/sp_augment.hip, common/data.py:BatchElasticDeform): the generator against its
numpy restatement, the batched filter against the per-volume kernel (bit for bit) and scipy, the warp and the whole transform
against the per-sample device chain and against scipy, the seeded mode, and the loaders / training script end to end."""
import importlib.util
import os
import random

import numpy as np
import pytest
import torch

import stroke_prediction_amd  # noqa: F401
from augment_ref import uniform_pm1
from oracle import transforms as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "stroke-prediction_amd")


def _rng(nfields, per_field, seed, call):
    from stroke_prediction_amd.runtime import lib as L, ops as O
    dst = torch.full((nfields * per_field + 5,), 7.0, dtype=torch.float32, device="cuda")
    L.call("sp_rng_uniform_pm1", O.ptr(dst), nfields, per_field, seed, call, O.stream())
    out = dst.cpu().numpy()
    assert np.all(out[nfields * per_field:] == 7.0)          # nothing written past the last field
    return out[:nfields * per_field].reshape(nfields, per_field)


def test_rng_matches_numpy_restatement():
    seed = 2 ** 40 + 12345
    got = [_rng(3, 1003, seed, call) for call in (0, 2 ** 32 + 7)]        # 1003: no multiple of 4 (ragged last block) or 256
    for g, call in zip(got, (0, 2 ** 32 + 7)):
        assert np.array_equal(g, uniform_pm1(3, 1003, seed, call))
    assert not np.array_equal(got[0], got[1])
    # the float4 path (per_field a multiple of 4) writes the same values
    assert np.array_equal(_rng(2, 1000, seed, 0), uniform_pm1(2, 1000, seed, 0))


@pytest.mark.parametrize("shape, sigma", [((7, 20, 20), 2.0), ((9, 40, 40), 4.0), ((3, 5, 7), 4.0), ((4, 128, 128), 4.0)])
def test_batched_filter_equals_per_volume_kernel_and_scipy(shape, sigma):
    from stroke_prediction_amd.runtime import lib as L, ops as O
    Z, Y, X = shape
    nf = 6
    noise = (np.random.RandomState(3).rand(nf, Z, Y, X) * 2 - 1).astype(np.float32)
    src = torch.from_numpy(noise).cuda()
    dst, tmp = torch.empty_like(src), torch.empty_like(src)
    L.call("sp_gaussian_filter3d_batch", O.ptr(src), O.ptr(dst), O.ptr(tmp), nf, Z, Y, X, sigma, 4.0, O.stream())
    got = dst.cpu().numpy()
    for f in range(nf):
        vol = np.ascontiguousarray(noise[f].transpose(2, 1, 0))                 # (n0, n1, n2) = (x, y, z)
        v = torch.from_numpy(vol).cuda()
        d1, t1 = torch.empty_like(v), torch.empty_like(v)
        L.call("sp_gaussian_filter3d", O.ptr(v), O.ptr(d1), O.ptr(t1), X, Y, Z, sigma, 4.0, O.stream())
        assert np.array_equal(got[f].transpose(2, 1, 0), d1.cpu().numpy()), f
        want = T.gaussian_filter(noise[f].astype(np.float64), sigma, mode="constant", cval=0)
        np.testing.assert_allclose(got[f], want, rtol=0, atol=2e-6)


def _close_but_for_edge_flips(got, want, atol, frac):
    """fp32 coordinates: a sampling point next to a volume face can land on its other side (0 instead of an interpolated
    value) -- the bound of tests/test_transforms.py: at most a share `frac` of the voxels may differ by more than atol"""
    bad = np.abs(got - want) > atol
    print("max |diff| %.3g, voxels above %g: %d of %d (%.3g, allowed %g)" % (float(np.abs(got - want).max()), atol, bad.sum(), bad.size,
                                                                            bad.mean(), frac))
    assert bad.mean() <= frac, (bad.sum(), bad.size, float(np.abs(got - want).max()))


def _samples(B, xyz, n_labels, n_images, seed):
    """numpy samples in the reference's (x, y, z, c) layout: binary labels, smooth images"""
    rs = np.random.RandomState(seed)
    out = []
    for b in range(B):
        s = {"case_id": 10 + b, "clinical_idx": b, "labels": (rs.rand(*xyz, n_labels) > 0.5).astype(np.float32),
             "images": [], "clinical": rs.rand(1, 1, 1, 5).astype(np.float32)}
        if n_images:
            s["images"] = np.stack([T.gaussian_filter(rs.rand(*xyz), 1.5) for _ in range(n_images)], axis=3).astype(np.float32)
        out.append(s)
    return out


def _collate(samples):
    """what the loader hands to a batch transform: ToTensor-layout samples stacked, on the device"""
    batch = {"case_id": torch.tensor([s["case_id"] for s in samples]),
             "labels": torch.stack([torch.from_numpy(T.to_tensor_layout(s["labels"]).copy()) for s in samples]).cuda(),
             "clinical": torch.stack([torch.from_numpy(T.to_tensor_layout(s["clinical"]).copy()) for s in samples]).cuda(), "images": []}
    if len(samples[0]["images"]):
        batch["images"] = torch.stack([torch.from_numpy(T.to_tensor_layout(s["images"]).copy()) for s in samples]).cuda()
    return batch


@pytest.mark.parametrize("xyz, alpha, sigma", [((20, 20, 7), 20, 2), ((128, 128, 4), 100, 4)])
def test_batch_transform_equals_per_sample_device_chain(xyz, alpha, sigma):
    import stroke_prediction_amd.common.data as D
    samples, flips, seeds = _samples(2, xyz, 3, 2, seed=4), [True, False], [21, 22]
    batch = _collate(samples)
    before = {k: batch[k].clone() for k in ("labels", "images")}
    got = D.BatchElasticDeform(alpha, sigma, apply_to_images=True, noise="host")(
        batch, random_states=[np.random.RandomState(s) for s in seeds], flips=flips)
    assert all(torch.equal(batch[k], before[k]) for k in before)                      # no in-place edit of the input
    assert got["clinical"] is batch["clinical"] and got["case_id"] is batch["case_id"]
    # the per-sample chain of the existing classes on the same generator states
    real = D.np.random.RandomState
    want = {"labels": [], "images": []}
    try:
        for s, flip, seed in zip(samples, flips, seeds):
            D.np.random.RandomState = lambda _=None, seed=seed: real(seed)            # ElasticDeform seeds a fresh state from the clock
            dev = D.to_device(s)
            dev = D._flip(dev) if flip else dev
            dev = D.ToTensor()(D.ElasticDeform(alpha, sigma, apply_to_images=True)(dev))
            for k in want:
                want[k].append(dev[k])
    finally:
        D.np.random.RandomState = real
    for k in want:
        w = torch.stack(want[k]).cpu().numpy()
        assert got[k].shape == w.shape and got[k].dtype == torch.float32
        _close_but_for_edge_flips(got[k].cpu().numpy(), w, 1e-5, 2e-4)


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("xyz, alpha, sigma", [((20, 20, 7), 20, 2), ((40, 40, 9), 100, 4)])
def test_batch_transform_matches_scipy(xyz, alpha, sigma, seed):
    import stroke_prediction_amd.common.data as D
    samples, flips = _samples(2, xyz, 3, 0, seed=100 + seed), [False, True]
    seeds = [2 * seed + 50, 2 * seed + 51]
    got = D.BatchElasticDeform(alpha, sigma, noise="host")(_collate(samples), random_states=[np.random.RandomState(s) for s in seeds],
                                                           flips=flips)
    want = []
    for s, flip, sd in zip(samples, flips, seeds):
        s64 = {k: (v.astype(np.float64) if isinstance(v, np.ndarray) else v) for k, v in s.items()}
        r = T.elastic_deform(T.hemispheric_flip(s64, flip), alpha, sigma, False, np.random.RandomState(sd))
        want.append(T.to_tensor_layout(r["labels"]))
    _close_but_for_edge_flips(got["labels"].cpu().numpy().astype(np.float64), np.stack(want), 2e-4, 1e-3)


def test_flip_modes_and_flip_only_images():
    """the three values of `flip`, and images that are flipped but not deformed (apply_to_images=False)"""
    import stroke_prediction_amd.common.data as D
    samples = _samples(3, (12, 12, 5), 1, 2, seed=8)                         # case ids 10, 11, 12
    batch = _collate(samples)
    states = lambda: [np.random.RandomState(s) for s in (1, 2, 3)]
    fixed = D.BatchElasticDeform(10, 2, flip=10, noise="host")(batch, random_states=states())
    explicit = D.BatchElasticDeform(10, 2, noise="host")(batch, random_states=states(), flips=[False, True, True])
    assert torch.equal(fixed["labels"], explicit["labels"]) and torch.equal(fixed["images"], explicit["images"])
    assert torch.equal(fixed["images"][0], batch["images"][0]) and torch.equal(fixed["images"][1:], torch.flip(batch["images"][1:], (-1,)))
    random.seed(6)
    tosses = [random.random() > 0.5 for _ in range(3)]
    random.seed(6)
    tossed = D.BatchElasticDeform(10, 2, flip="random", noise="host")(batch, random_states=states())
    again = D.BatchElasticDeform(10, 2, noise="host")(batch, random_states=states(), flips=tosses)
    assert torch.equal(tossed["labels"], again["labels"]) and torch.equal(tossed["images"], again["images"])
    none = D.BatchElasticDeform(10, 2, noise="host")(batch, random_states=states())
    assert none["images"] is batch["images"] and not torch.equal(none["labels"], fixed["labels"])
    with pytest.raises(ValueError):
        D.BatchElasticDeform()({"labels": torch.zeros(1, 1, 3, 4, 5, device="cuda"), "images": []})        # X != Y


def test_philox_mode_is_reproducible_from_the_seed():
    import stroke_prediction_amd.common.data as D
    batch = _collate(_samples(2, (24, 24, 6), 3, 0, seed=9))
    a, b = D.BatchElasticDeform(20, 2, seed=11), D.BatchElasticDeform(20, 2, seed=11)
    a1, b1, a2 = a(batch)["labels"], b(batch)["labels"], a(batch)["labels"]
    assert torch.equal(a1, b1) and not torch.equal(a1, a2)                  # the call counter advances per batch
    assert not torch.equal(a1, D.BatchElasticDeform(20, 2, seed=12)(batch)["labels"])
    for t in (a1, a2):
        assert float(t.min()) >= 0.0 and float(t.max()) <= 1.0 and bool(torch.isfinite(t).all())      # binary labels interpolate inside [0, 1]
    assert 0.05 < float(a1.mean()) < 0.95 and not torch.equal(a1, batch["labels"])


def test_loader_with_batch_transform(monkeypatch):
    from common import data
    monkeypatch.setenv("SP_SYNTHETIC_DATA", "1")
    labels = ["l0", "l1", "l2"]
    chain = lambda: [data.ResamplePlaneXY(0.25), data.ToTensor()]
    plain = data.get_stroke_shape_training_data([], labels, chain(), chain(), [0, 1, 2, 3, 4, 5], 0.5, batchsize=3)
    aug = data.get_stroke_shape_training_data([], labels, chain(), chain(), [0, 1, 2, 3, 4, 5], 0.5, batchsize=3,
                                              batch_transform=data.BatchElasticDeform(flip="random", seed=5))
    assert len(aug[0].sampler.indices) == len(plain[0].sampler.indices) == 3 and len(aug[0]) == len(plain[0]) == 1
    (p,), (a,) = list(plain[0]), list(aug[0])
    assert set(a) == set(p)
    for k in ("labels", "clinical", "case_id"):
        assert a[k].shape == p[k].shape and a[k].dtype == p[k].dtype and a[k].device == p[k].device, k
    assert tuple(a["labels"].shape) == (3, 3, 28, 64, 64) and a["labels"].is_cuda
    assert sorted(a["case_id"].tolist()) == sorted(p["case_id"].tolist())
    # the validation loader is the same with and without the keyword
    (vp,), (va,) = list(plain[1]), list(aug[1])
    order_p, order_a = np.argsort(vp["case_id"].numpy()), np.argsort(va["case_id"].numpy())
    assert np.array_equal(vp["case_id"].numpy()[order_p], va["case_id"].numpy()[order_a])
    assert torch.equal(vp["labels"][order_p], va["labels"][order_a]) and torch.equal(vp["clinical"][order_p], va["clinical"][order_a])


def test_training_script_with_batchaugment(tmp_path, monkeypatch, capsys):
    """train_shape_reconstruction.py --batchaugment --epochs 1 --graph on synthetic cases: one epoch, a finite loss"""
    monkeypatch.setenv("SP_SYNTHETIC_DATA", "1")
    from common import data, util
    spec = importlib.util.spec_from_file_location("train_shape_reconstruction_batchaugment", os.path.join(PKG, "train_shape_reconstruction.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    args = util.get_args_shape_training(["--batchaugment", "--epochs", "1", "--graph", "--batchsize", "2", "--fold", "0", "1", "2", "3",
                                         "--outbasepath", str(tmp_path / "cae")])
    train_loader, _ = script.build_loaders(args)
    assert isinstance(train_loader.collate_fn.batch_transform, data.BatchElasticDeform)
    assert not any(isinstance(t, (data.ElasticDeform, data.HemisphericFlip)) for t in train_loader.dataset._transform.transforms)
    learner = script.train(args)
    losses = [m.loss for m in learner._metric_dtos["training"]]
    assert len(losses) == 1 and np.isfinite(float(losses[0]))
    assert "Epoch 1/1 training loss" in capsys.readouterr().out
