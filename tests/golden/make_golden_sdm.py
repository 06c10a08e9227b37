#!/usr/bin/env python3
"""Generate ``sdm.npz`` by running the REAL reference ``test_sdm_resampling.sdm_interpolate_numpy`` /
``get_normalized_time`` on CPU (same environment as ``make_golden.py``; no test runs this file):

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_sdm.py

Inputs come from seeded numpy generators; binary masks are stored with ``packbits``.  The reference's fields are stored in
two lossless-or-bounded encodings that keep the file small (decoded by ``decode`` below, which the tests import):
  * "sq:" signed squared distances (int32): a full-resolution field is sign(s) * sqrt(|s|) -- checked BIT-EQUAL to the
    reference's array here;
  * "q:"  every other field quantised to multiples of 2^-QBITS, delta-coded ":qo" times along the last axis (the order that
    compresses best; the zoomed fields are piecewise cubic there) -- the largest decoding error is checked here and stored
    (``qerr``); it is below 2^-(QBITS+1).
Keys: ``<case>/in_core``, ``<case>/in_penu`` (packbits or float32), ``<case>/<setting>/<field>``.  Every case also satisfies
the cap that the sign-mask comparison relies on: at most 0.1 % of the voxels of each reference field lie within 1e-8 of 0
without being exactly 0 (``near_zero``).
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

QBITS = 34
ORDERS = (0, 1, 2, 3, 4)
INPUT_STEP = 4096               # the float inputs are multiples of 1/4096 in [0, 1]: stored as uint16 counts
NEAR_ZERO, CAP = 1e-8, 1e-3
FIELDS = ("recon_core", "recon_intp", "recon_penu", "latent_core", "latent_intp", "latent_penu")


def decode(fx, key):
    """the stored field ``key`` as float64 (works on any mapping of the npz keys)"""
    if key + ":sq" in fx:
        s = np.asarray(fx[key + ":sq"]).astype(np.int64)
        return np.sign(s) * np.sqrt(np.abs(s).astype(np.float64))
    e = np.asarray(fx[key + ":q"]).astype(np.int64)
    for _ in range(int(fx[key + ":qo"])):
        e = np.cumsum(e, axis=-1)
    return e.astype(np.float64) * 2.0 ** -QBITS


def load_input(fx, key, shape):
    """a stored input volume as the float32 array the reference was given"""
    if key + ":u" in fx:
        return (np.asarray(fx[key + ":u"]).astype(np.float64) / INPUT_STEP).astype(np.float32).reshape(shape)
    return np.unpackbits(np.asarray(fx[key]))[:int(np.prod(shape))].reshape(shape).astype(np.float32)


def _narrow(a):
    for t in (np.int8, np.int16, np.int32):
        if a.min() >= np.iinfo(t).min and a.max() <= np.iinfo(t).max:
            return a.astype(t)
    return a


def encode(fx, key, x, exact_sq=False):
    x = np.asarray(x, dtype=np.float64)
    if exact_sq:
        s = np.rint(np.sign(x) * x * x).astype(np.int64)
        fx[key + ":sq"] = _narrow(s)
        assert np.array_equal(decode(fx, key), x), key
        return
    import zlib
    q = np.rint(x * 2.0 ** QBITS).astype(np.int64)
    best = None
    for order in ORDERS:
        e = q
        for _ in range(order):
            e = np.diff(e, axis=-1, prepend=0)
        e = _narrow(e)
        size = len(zlib.compress(e.tobytes()))
        if best is None or size < best[0]:
            best = (size, order, e)
    fx[key + ":q"], fx[key + ":qo"] = best[2], np.array(best[1])
    err = float(np.abs(decode(fx, key) - x).max())
    assert err <= 2.0 ** -(QBITS + 1), (key, err)
    fx["qerr"] = np.float64(max(float(fx.get("qerr", 0.0)), err))


def blobs(rng, shape, sigma):
    from scipy.ndimage import gaussian_filter
    f = gaussian_filter(rng.rand(*shape), sigma, mode="wrap")
    f -= f.min()
    return f / f.max()


def nested(seed, shape, sigma, qcore=0.92, qpenu=0.75):
    f = blobs(np.random.RandomState(seed), shape, sigma)
    core = (f > np.quantile(f, qcore)).astype(np.float32)
    penu = (f > np.quantile(f, qpenu)).astype(np.float32)
    return core, penu


def near_zero(x):
    """the voxels the sign-mask comparison leaves out: 0 < |x| <= 1e-8.  Exact zeros are compared (both sides compute them
    exactly: a voxel where both transforms vanish, e.g. inside an artificial core -- whose >= 20 voxels alone exceed 0.1 % of a
    12 x 40 x 36 volume)"""
    return (np.abs(x) <= NEAR_ZERO) & (x != 0)


def check_cap(name, x):
    frac = float(near_zero(x).mean())
    assert frac <= CAP, (name, frac)


def run(ref, core, penu, t, resample):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = ref.sdm_interpolate_numpy(core[None, None], penu[None, None], t, resample=resample)
    return dict(zip(FIELDS, out)), buf.getvalue()


def store_case(fx, ref, name, core, penu, ts, settings, binary=True, latents_only=False):
    if binary:
        fx[name + "/in_core"] = np.packbits(core.astype(bool).reshape(-1))
        fx[name + "/in_penu"] = np.packbits(penu.astype(bool).reshape(-1))
    else:
        for k, v in (("in_core", core), ("in_penu", penu)):
            u = np.rint(v.astype(np.float64) * INPUT_STEP).astype(np.uint16)
            assert np.array_equal((u / INPUT_STEP).astype(np.float32), v), k
            fx["%s/%s:u" % (name, k)] = u
    fx[name + "/shape"] = np.array(core.shape)
    fx[name + "/t"] = np.array(ts, dtype=np.float64)
    for resample in settings:
        s = "%s/%s" % (name, "resample" if resample else "full")
        for i, t in enumerate(ts):
            r, printed = run(ref, core, penu, t, resample)
            fx[s + "/printed"] = np.array(printed)
            for k, v in r.items():
                check_cap("%s/%s/t%d" % (s, k, i), v)
            for k in ("latent_core", "latent_intp", "latent_penu"):
                if k == "latent_intp" or i == 0:
                    encode(fx, "%s/%s%s" % (s, k, "/t%d" % i if k == "latent_intp" else ""), r[k])
            if latents_only:
                continue
            full = not resample
            if i == 0:
                encode(fx, s + "/recon_core", r["recon_core"], exact_sq=full)
                encode(fx, s + "/recon_penu", r["recon_penu"], exact_sq=full)
            if t == 0.0 and not full:       # zoom is odd and linear: the t = 0 / t = 1 blends are -core / penu bit for bit
                assert np.array_equal(r["recon_intp"], -r["recon_core"]), s
            elif t == 1.0 and not full:
                assert np.array_equal(r["recon_intp"], r["recon_penu"]), s
            else:
                encode(fx, "%s/recon_intp/t%d" % (s, i), r["recon_intp"])


def main():
    from make_golden import import_reference
    import scipy
    import torch
    import_reference()
    import test_sdm_resampling as ref
    fx = {"scipy_version": np.array(scipy.__version__), "qbits": np.array(QBITS),
          "generator": np.array("reference test_sdm_resampling.sdm_interpolate_numpy / get_normalized_time, tests/golden/make_golden_sdm.py")}
    c, p = nested(101, (4, 128, 128), (1.0, 6.0, 6.0))
    store_case(fx, ref, "bin128_d4", c, p, [0.0, 0.35, 1.0], [True])
    c, p = nested(202, (28, 128, 128), (2.0, 6.0, 6.0))
    store_case(fx, ref, "bin128_d28", c, p, [0.6], [True], latents_only=True)
    c, p = nested(303, (12, 40, 36), (1.5, 3.0, 3.0))
    store_case(fx, ref, "odd", c, p, [0.35], [True, False])
    _, p = nested(404, (12, 40, 36), (1.5, 3.0, 3.0), qpenu=0.85)
    store_case(fx, ref, "artificial", np.zeros_like(p), p, [0.6], [True, False])
    f = blobs(np.random.RandomState(505), (12, 40, 36), (1.5, 3.0, 3.0))
    g = blobs(np.random.RandomState(506), (12, 40, 36), (1.5, 3.0, 3.0))
    penu = np.clip(np.rint((f * 1.6 - 0.3) * 4096) / 4096, 0, 1).astype(np.float32)
    core = np.clip(np.rint((f * g * 2.0 - 0.25) * 4096) / 4096, 0, 1).astype(np.float32)
    penu[penu == 0.5] = 0.5 + 1.0 / 4096
    rng = np.random.RandomState(507)
    for i in rng.choice(penu.size, 6, replace=False):      # a few voxels exactly at the threshold: background in both masks
        penu.reshape(-1)[i] = 0.5
    core.reshape(-1)[rng.choice(core.size, 6, replace=False)] = 0.5
    store_case(fx, ref, "prob", core, penu, [0.55], [False], binary=False)
    # time normalisation: four clinical vectors (B, 5, 1, 1, 1)
    clinical = torch.from_numpy(np.random.RandomState(606).uniform(0.2, 6.0, (4, 5, 1, 1, 1)))
    batch = {"clinical": clinical}
    to_to_ta, norm = ref.get_normalized_time(batch, 10)
    ta_to_tr = batch["clinical"][:, 1, :, :, :].squeeze().unsqueeze(1)          # test_sdm_resampling.py:110-111
    fx["time/clinical"] = clinical.numpy()
    fx["time/to_to_ta"] = to_to_ta.numpy()
    fx["time/normalization"] = norm.numpy()
    fx["time/time_to_treatment"] = (ta_to_tr.type(torch.FloatTensor) / norm).numpy()
    np.savez_compressed(os.path.join(HERE, "sdm.npz"), **fx)
    print("wrote sdm.npz: %d keys, %d bytes, qerr %.3g" % (len(fx), os.path.getsize(os.path.join(HERE, "sdm.npz")), float(fx["qerr"])))


if __name__ == "__main__":
    main()
