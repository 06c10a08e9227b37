"""Intensity augmentation on the GPU (csrc/sp_intensity.hip; ``data.IntensityAugment``): ``sp_blur3d_reflect_batch``,
``sp_intensity_stats_partials`` and ``sp_intensity_apply_batch`` against their numpy restatement (tests/intensity_ref.py) -- bit for
bit where the semantics say so, within a derived tolerance of the float64 evaluation elsewhere -- and the transform through the
cached loader.  B = 2, C0 = 2 throughout: four fields per launch."""
import random

import numpy as np
import pytest
import torch

import stroke_prediction_amd  # noqa: F401
import intensity_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD, GUARD_VALUE = 64, 777.0
B, C0 = 2, 2
NF = B * C0
# The largest |fp32 evaluation - float64 evaluation| of tests/intensity_ref.py on the very inputs used below (R.smooth_volumes(NF,
# shape, R.INPUT_SEED), R.SEED, R.CALL), over the three shapes, measured on the CPU and rounded up: 4.293e-07 for "single" and
# 7.734e-07 for "chained" (tests/test_intensity_host.py re-measures them).  The device gets four times that: its logf, cosf and
# powf may differ from numpy's by a few ulp, and t^gamma near t = 0 amplifies that.
MEASURED = {"single": 4.30e-07, "chained": 7.74e-07}
TOL = {name: 4 * v for name, v in MEASURED.items()}
BLUR_RTOL = 2e-6      # times max |x|: the project's bound for the Gaussian filter (tests/test_transforms.py)
# blur: the three common shapes, one extent just above the tile length on each axis in turn (x tile 128, y and z tiles 32), and
# one extent equal to the largest radius (sigma 1.0: radius 4)
BLUR_SHAPES = R.SHAPES + [(7, 10, 130), (7, 34, 13), (34, 10, 13), (4, 10, 13)]
SIGMAS = [0.5, 1.0, None, 0.75]      # radius 2, 4, the delta kernel, 3: rows zero-padded to radius 4


def _guarded(x, lead=0):
    """a device copy of `x` behind `lead` guard words (lead = 1: a view that is not 16-byte aligned) and in front of a guard tail,
    neither of which the kernels may touch -> (buffer, view)"""
    x = np.array(x, dtype=np.float32, order="C")      # a copy: the shared inputs are read-only
    buf = torch.full((lead + x.size + GUARD,), GUARD_VALUE, dtype=torch.float32, device=DEV)
    buf[lead:lead + x.size] = torch.from_numpy(x.reshape(-1)).to(DEV)
    buf.lead = lead
    return buf, buf[lead:lead + x.size].view(x.shape)


def _check_guard(*bufs):
    for buf in bufs:
        assert bool((buf[-GUARD:] == GUARD_VALUE).all()) and bool((buf[:buf.lead] == GUARD_VALUE).all()), "a kernel wrote outside its buffer"


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32, order="C")).to(DEV)


def _stats(x, params, seed=R.SEED, call=R.CALL):
    """sp_intensity_stats_partials on (nf, ...) fields -> partials (nf, 64, 4) as numpy"""
    from stroke_prediction_amd.runtime import lib as L, ops as O
    nf, per_field = len(x), int(np.prod(x.shape[1:]))
    xbuf, xd = _guarded(x)
    pbuf, pd = _guarded(np.full((nf, 64, 4), np.nan))
    par = _dev(params)
    L.call("sp_intensity_stats_partials", O.ptr(xd), O.ptr(par), O.ptr(pd), nf, per_field, seed, call, O.stream())
    torch.cuda.synchronize()
    _check_guard(xbuf, pbuf)
    assert np.array_equal(xd.cpu().numpy(), x)      # the source is only read
    return pd.cpu().numpy()


def _apply(x, params, seed=R.SEED, call=R.CALL, inplace=False, lead=(0, 0)):
    """statistics + apply on (nf, ...) fields -> the output as numpy; the output starts as NaN: an element left out shows"""
    from stroke_prediction_amd.runtime import lib as L, ops as O
    nf, per_field = len(x), int(np.prod(x.shape[1:]))
    xbuf, xd = _guarded(x, lead[0])
    ybuf, yd = (xbuf, xd) if inplace else _guarded(np.full(x.shape, np.nan), lead[1])
    pbuf, pd = _guarded(np.full((nf, 64, 4), np.nan))
    par = _dev(params)
    L.call("sp_intensity_stats_partials", O.ptr(xd), O.ptr(par), O.ptr(pd), nf, per_field, seed, call, O.stream())
    L.call("sp_intensity_apply_batch", O.ptr(xd), O.ptr(yd), O.ptr(par), O.ptr(pd), nf, per_field, seed, call, O.stream())
    torch.cuda.synchronize()
    _check_guard(xbuf, ybuf, pbuf)
    if not inplace:
        assert np.array_equal(xd.cpu().numpy(), x)
    return yd.cpu().numpy()


def _blur(x, weights):
    from stroke_prediction_amd.runtime import lib as L, ops as O
    nf, (Z, Y, X) = len(x), x.shape[1:]
    xbuf, xd = _guarded(x)
    ybuf, yd = _guarded(np.full(x.shape, np.nan))
    tbuf, td = _guarded(np.full(x.shape, np.nan))
    w = _dev(weights)
    L.call("sp_blur3d_reflect_batch", O.ptr(xd), O.ptr(yd), O.ptr(td), O.ptr(w), nf, Z, Y, X, (weights.shape[1] - 1) // 2, O.stream())
    torch.cuda.synchronize()
    _check_guard(xbuf, ybuf, tbuf)
    assert np.array_equal(xd.cpu().numpy(), x)
    return yd.cpu().numpy()


_INPUTS = {}


def _inputs(shape):
    """the smooth unit-scale fields of one shape, computed once and never changed"""
    if shape not in _INPUTS:
        _INPUTS[shape] = R.smooth_volumes(NF, shape, R.INPUT_SEED)
        _INPUTS[shape].setflags(write=False)
    return _INPUTS[shape]


def _same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


NEUTRAL = np.tile(np.array(R.NEUTRAL, np.float32), (NF, 1))


# ------------------------------------------------------------------------------------------------ exactness

@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("shape", R.SHAPES)
def test_neutral_rows_are_bit_equal(shape, inplace):
    x = _inputs(shape)
    _same(_apply(x, NEUTRAL, inplace=inplace), x)


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("shape", R.SHAPES)
def test_gain_only_rows_are_the_fp32_product(shape, inplace):
    x = _inputs(shape)
    params = NEUTRAL.copy()
    params[:, 1] = (0.75, 0.9, 1.1, 1.25)
    _same(_apply(x, params, inplace=inplace), params[:, 1, None, None, None] * x)


@pytest.mark.parametrize("shape", BLUR_SHAPES)
def test_delta_weights_blur_is_bit_equal(shape):
    x = R.smooth_volumes(NF, shape, R.INPUT_SEED)
    x[0, 0, 0, :2] = (-0.0, 0.0)      # the sign of a zero survives too
    for radius in (0, 4):
        w = np.zeros((NF, 2 * radius + 1), np.float32)
        w[:, radius] = 1
        if min(shape) >= radius:
            _same(_blur(x, w), x)


@pytest.mark.parametrize("shape", R.SHAPES)
def test_statistics(shape):
    x = _inputs(shape)
    params = NEUTRAL.copy()
    params[2:, 0] = (0.3, 0.05)      # two fields without noise, two with
    part = _stats(x, params)
    assert not np.isnan(part).any() and not part[:, :, 3].any()
    y1 = x.reshape(NF, -1).copy()
    noisy = np.repeat(NEUTRAL[:1], NF, 0)
    noisy[:, 0] = params[:, 0]
    y1[2:] = _apply(x, noisy).reshape(NF, -1)[2:]      # the device's own y1: the apply launch regenerates the very noise
    ref = R.noisy(x, params, R.SEED, R.CALL)
    assert np.abs(y1 - ref).max() < TOL["single"]
    c = R.chunk_length(y1.shape[1])
    for f in range(NF):
        for i in range(64):
            chunk = y1[f, i * c:(i + 1) * c]
            if len(chunk):
                assert part[f, i, 0] == chunk.min() and part[f, i, 1] == chunk.max()
            else:
                assert part[f, i, 0] == np.inf and part[f, i, 1] == -np.inf and part[f, i, 2] == 0
        assert part[f, :, 0].min() == y1[f].min() and part[f, :, 1].max() == y1[f].max()      # exactly numpy's
        mean = part[f, :, 2].astype(np.float64).sum() / y1.shape[1]
        want = y1[f].astype(np.float64).mean()
        bound = 2.0 ** -19 * np.abs(y1[f]).astype(np.float64).mean()      # at most 32 roundings of 2^-24 on any path of the sum
        print("field %d: mean %.9g, float64 %.9g, |diff| %.3g, bound %.3g" % (f, mean, want, abs(mean - want), bound))
        assert abs(mean - want) <= bound


def test_noise_has_the_reference_sign_pattern_and_moments():
    shape, n, sn = R.SHAPES[2], 1 << 16, np.float32(0.3)
    x = _inputs(shape)
    params = NEUTRAL.copy()
    params[:, 0] = sn
    got = _apply(x, params).reshape(NF, -1)
    for f in (0, 3):
        d = ((got[f].astype(np.float64) - x[f].reshape(-1)) / np.float64(sn))[:n]
        ref = R.normals(f, got.shape[1], R.SEED, R.CALL)[:n]
        sure = np.abs(ref) > 1e-3      # the sum is rounded at 2^-24 of a unit-scale value: only a smaller normal can lose its sign
        assert sure.mean() > 0.99 and np.array_equal(np.sign(d[sure]), np.sign(ref[sure]))
        print("field %d: mean %.4g var %.4g (reference %.4g %.4g)" % (f, d.mean(), d.var(), ref.mean(), ref.var()))
        assert abs(d.mean()) < 5 / np.sqrt(n) and abs(d.var() - 1) < 5 * np.sqrt(2.0 / n)
        # an element differs from the reference by less than 2e-6: the rounding of the sum, 2^-24 of a value below 2, over sigma_n,
        # plus a few ulp of a normal below 5; so does the mean, and the variance by less than 2 E|n| 2e-6
        assert abs(d.mean() - ref.mean()) < 2e-6 and abs(d.var() - ref.var()) < 4e-6
    assert not np.array_equal(got[0] - x[0].reshape(-1), got[1] - x[1].reshape(-1))      # a stream per field


# ------------------------------------------------------------------------------------------------ determinism

@pytest.mark.parametrize("shape", R.SHAPES)
def test_two_calls_are_bit_identical(shape):
    x = _inputs(shape)
    table = R.TABLES["chained"]
    _same(_apply(x, table), _apply(x, table))
    _same(_stats(x, table), _stats(x, table))
    _same(_apply(x, table, inplace=True), _apply(x, table))
    for lead in ((1, 0), (0, 1), (1, 1)):      # a source or a destination that is not 16-byte aligned: element-wise, the same bits
        _same(_apply(x, table, lead=lead), _apply(x, table))
    _same(_apply(x, table, inplace=True, lead=(1, 1)), _apply(x, table))
    w = R.weights_table(SIGMAS)
    _same(_blur(x, w), _blur(x, w))
    assert not np.array_equal(_apply(x, table, call=R.CALL + 1), _apply(x, table))
    assert not np.array_equal(_apply(x, table, seed=R.SEED + (1 << 32)), _apply(x, table))      # the high word of the seed counts


@pytest.mark.parametrize("shape", R.SHAPES)
def test_a_field_does_not_depend_on_the_batch_around_it(shape):
    x = _inputs(shape)
    table = R.TABLES["chained"]
    # field word 0, alone and in front of three others: noise and every later stage
    _same(_apply(x[:1], table[:1]), _apply(x, table)[:1])
    _same(_stats(x[:1], table[:1]), _stats(x, table)[:1])
    # without noise the position does not count either: one volume and one row in every slot
    quiet = np.tile(np.array([R.row(gain=1.1, contrast=0.8, gamma=1.3)], np.float32), (NF, 1))
    out = _apply(np.repeat(x[1:2], NF, 0), quiet)
    for f in range(1, NF):
        _same(out[f], out[0])
    w = R.weights_table(SIGMAS)
    _same(_blur(x[:1], w[:1]), _blur(x, w)[:1])
    _same(_blur(np.repeat(x[1:2], NF, 0), np.repeat(w[1:2], NF, 0))[3], _blur(x[1:2], w[1:2])[0])


# ------------------------------------------------------------------------------------------------ against the float64 reference

@pytest.mark.parametrize("shape", BLUR_SHAPES)
def test_blur_matches_the_reference(shape):
    x = R.smooth_volumes(NF, shape, R.INPUT_SEED)
    w = R.weights_table(SIGMAS)
    got, want = _blur(x, w), R.blur(x, w)
    err = np.abs(got - want).max()
    print("max |blur - float64| %.3g, bound %.3g" % (err, BLUR_RTOL * np.abs(x).max()))
    assert err <= BLUR_RTOL * np.abs(x).max()
    _same(got[2], x[2])      # the delta row among blurring ones
    assert np.abs(got[1] - x[1]).max() > 1e-3


def test_blur_refuses_an_extent_below_the_radius():
    from stroke_prediction_amd.runtime import lib as L, ops as O
    x = _dev(np.zeros((NF, 3, 10, 13)))
    y, t, w = torch.empty_like(x), torch.empty_like(x), _dev(R.weights_table(SIGMAS))
    rc = L.load().sp_blur3d_reflect_batch(O.ptr(x), O.ptr(y), O.ptr(t), O.ptr(w), NF, 3, 10, 13, 4, O.stream())
    assert rc == L.CONSTS["SP_EINVAL"] and "radius" in L.last_error()


@pytest.mark.parametrize("name", sorted(R.TABLES))
@pytest.mark.parametrize("shape", R.SHAPES)
def test_noise_contrast_and_gamma_match_the_reference(shape, name):
    x = _inputs(shape)
    table = R.TABLES[name]
    want = R.apply(x, table, R.SEED, R.CALL)
    for inplace in (False, True):
        got = _apply(x, table, inplace=inplace)
        err = np.abs(got - want).reshape(NF, -1).max(1)
        print("%s %r: max |device - float64| per field %s, bound %.4g" % (name, shape, err, TOL[name]))
        assert np.isfinite(got).all() and err.max() <= TOL[name]


# ------------------------------------------------------------------------------------------------ the transform and the loader

def test_transform_on_a_batch_dict():
    from stroke_prediction_amd.common import data as D
    shape = R.SHAPES[1]
    x = _inputs(shape).reshape((B, C0) + shape)
    batch = {D.KEY_CASE_ID: torch.tensor([3, 4]), D.KEY_IMAGES: _dev(x), D.KEY_LABELS: _dev(x > 0.2), D.KEY_GLOBAL: _dev(np.ones((B, 5)))}
    on = dict(p_noise=1, p_blur=1, p_blur_channel=1, p_gain=1, p_contrast=1, p_gamma=1)
    a, b = D.IntensityAugment(seed=R.SEED, **on), D.IntensityAugment(seed=R.SEED, **on)
    ref = D.IntensityAugment(seed=R.SEED, **on)
    for call in range(2):
        out, again = a(batch), b(batch)
        assert sorted(out) == sorted(batch)
        for k in batch:
            if k != D.KEY_IMAGES:
                assert out[k] is batch[k]
        assert np.array_equal(batch[D.KEY_IMAGES].cpu().numpy(), x)      # the input stays as it was
        assert torch.equal(out[D.KEY_IMAGES], again[D.KEY_IMAGES]) and out[D.KEY_IMAGES].shape == batch[D.KEY_IMAGES].shape
        draws = ref.draw(B, C0)
        assert draws["call"] == call and draws["weights"] is not None
        flat = np.ascontiguousarray(x.reshape((NF,) + shape))
        # the transform is the three entry points on its own table, weights, seed and call: the same bits
        want = _apply(_blur(flat, draws["weights"]), draws["params"], seed=R.SEED, call=call)
        _same(out[D.KEY_IMAGES].cpu().numpy().reshape(want.shape), want)
        assert not np.array_equal(want, flat)
    off = D.IntensityAugment(p_noise=0, p_blur=0, p_gain=0, p_contrast=0, p_gamma=0, p_gamma_invert=0, seed=1)(batch)
    assert torch.equal(off[D.KEY_IMAGES], batch[D.KEY_IMAGES]) and off[D.KEY_IMAGES] is not batch[D.KEY_IMAGES]
    with pytest.raises(RuntimeError, match="no CPU path"):
        a(dict(batch, images=batch[D.KEY_IMAGES].double()))
    with pytest.raises(RuntimeError, match="no CPU path"):
        a(dict(batch, images=batch[D.KEY_IMAGES].cpu()))


def test_loader_is_reproducible_from_the_seed():
    from stroke_prediction_amd.common import data as D
    chain = [D.ResamplePlaneXY(0.5), D.HemisphericFlip(), D.PadImages(4, 4, 2, pad_value=0), D.RandomPatch(16, 12, 6, 4, 4, 2), D.ToTensor()]
    kw = dict(modalities=["a", "b"], labels=["x", "y"], xy=32, z=6, n_cases=6)
    cache = D.DeviceCaseCache(D.SyntheticStrokeDataset3D(transform=D.Compose(D._cache_prefix([chain]), device=DEV), **kw), DEV)
    make = lambda bt, **more: D.CachedBatchLoader(cache, list(range(6)), 4, chain, batch_transform=bt, **more)
    on = dict(p_noise=1, p_blur=1, p_blur_channel=0.5, p_gain=1, p_contrast=1, p_gamma=1)
    a, b, other, plain = make(D.IntensityAugment(seed=4, **on)), make(D.IntensityAugment(seed=4, **on)), make(D.IntensityAugment(seed=5, **on)), make(None)
    mixed_a, mixed_b = make(D.IntensityAugment(seed=6)), make(D.IntensityAugment(seed=6))      # the default tosses
    both = make(D.IntensityAugment(seed=4, **on), patch_augment=D.PatchAugment(seed=4, alpha=20, sigma=2),
                foreground=D.ForegroundOversample(0.5, seed=4))
    for n, items in enumerate(([5, 0, 3, 3], [1, 2, 4, 0], [2, 2])):
        batches = []
        for loader in (a, b, other, plain, mixed_a, mixed_b, both):
            random.seed(30 + n)
            batches.append(loader.make_batch(items))
        got, again, seed5, want = batches[:4]
        assert sorted(got) == sorted(want)
        assert torch.equal(got["images"], again["images"]) and not torch.equal(got["images"], seed5["images"])
        assert not torch.equal(got["images"], want["images"]) and got["images"].shape == want["images"].shape
        assert torch.equal(batches[4]["images"], batches[5]["images"])
        for b_ in (got, again, seed5, batches[4]):      # labels, clinical and the rest equal the loader's without the transform
            assert torch.equal(b_["labels"], want["labels"]) and torch.equal(b_["clinical"], want["clinical"])
            assert torch.equal(b_["case_id"], want["case_id"])
        for b_ in batches:
            assert bool(torch.isfinite(b_["images"]).all())
        assert batches[6]["images"].shape == want["images"].shape      # composes with the augmenting sampler and the oversampling
