"""``--patchaugment`` at the defaults of train_unet_segmentation.py (pad 20, patches 104 x 104 x 68, --xyresample 0.5, batch size 6, all
29 cases): the cached training loader without an augmenter, with ``data.PatchAugment`` and the elastic part off, and with the elastic
part on for every sample, in ONE process, alternated in windows of whole epochs with a device synchronise around each window.
In the same windows the kernels alone on one table: ``sp_patch_sample_batch`` (identity transform; a rotation + scale; rotation +
scale + fields + intensity) against ``sp_patch_gather_batch`` and against ``dst.copy_(src)`` of the same OUTPUT byte count.  Reported:
the median over the windows and the window spread ((max - min) / median).  Second leg: train_unet_segmentation.py --devicecache
--graph --fusedadam end to end with and without --patchaugment: the wall time of a run of 1 epoch and of a run of 1 + K epochs,
K epochs = the difference (start-up and graph capture cancel).

    SP_SYNTHETIC_DATA=1 python tools/bench_patchaugment.py [--windows 5] [--window-seconds 0.3] [--train-epochs 3] [--no-train]
"""
import argparse
import contextlib
import ctypes
import io
import json
import os
import random
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "stroke-prediction_amd")
sys.path.insert(0, ROOT)
sys.path.insert(0, PKG)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import stroke_prediction_amd  # noqa: E402,F401
from stroke_prediction_amd.common import data as D, util  # noqa: E402


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def summary(v):
    med = float(np.median(v))
    return dict(median_ms=med, min_ms=min(v), max_ms=max(v), spread=(max(v) - min(v)) / med)


def measure(windows, window_seconds):
    import train_unet_segmentation as S
    from stroke_prediction_amd.runtime import lib as L, ops as O
    with contextlib.redirect_stdout(io.StringIO()):      # the parser prints its namespace, the script its set sizes
        args = util.get_args_unet_training(["/tmp/unet.model", "--devicecache"])
        plain = S.build_loaders(args)[0]
    cache = plain.cache
    chain = [plain._stages[k] for k in D._CHAIN_ORDER if k in plain._stages]
    items = list(plain.sampler.indices)
    make = lambda aug: D.CachedBatchLoader(cache, items, plain.batch_size, chain, patch_augment=aug)
    loaders = {"plain": plain,
               "augment, elastic off": make(D.PatchAugment(p_elastic=0, seed=args.seed)),
               "augment, elastic on": make(D.PatchAugment(p_elastic=1, seed=args.seed))}
    epoch = {k: (lambda ld=ld: [None for _ in ld]) for k, ld in loaders.items()}
    nb = len(plain)
    reps = {}
    for k, fn in epoch.items():          # warm-up, then size the windows in whole epochs
        timed(fn, 1)
        reps[k] = max(1, int(window_seconds / timed(fn, 1)))
    # the kernels alone on the table of one FULL batch (an epoch's last batch may be short)
    plain.make_batch(items[:plain.batch_size])
    table = plain.last_table.to("cuda")
    B = table.shape[0]
    C0, C1 = cache.images.shape[1], cache.labels.shape[1]
    i3 = lambda v: (ctypes.c_int32 * 3)(*[int(a) for a in v])
    dst0 = torch.empty((B, C0) + tuple(plain._ext0[::-1]), dtype=torch.float32, device="cuda")
    dst1 = torch.empty((B, C1) + tuple(plain._ext1[::-1]), dtype=torch.float32, device="cuda")
    Z, Y, X = cache.shape_zyx
    groups = lambda s1: (O.ptr(cache.images), O.ptr(dst0), C0, i3(plain._ext0), i3(plain._pad0), plain._padval0, O.ptr(cache.labels),
                         O.ptr(dst1), C1, i3(plain._ext1), i3((0, 0, 0)), s1, O.ptr(table))
    dims = (len(cache), B, Z, Y, X)
    full = D.PatchAugment(p_affine=1, p_elastic=1, p_intensity=1, seed=args.seed)
    draws = full.draw(B, C0)
    ident = np.zeros((B, 16), dtype=np.float32)
    ident[:, 0] = ident[:, 4] = ident[:, 8] = 1.0
    affine = draws["xform"].copy()
    affine[:, 12:14] = 0
    up = lambda a: torch.from_numpy(a).to("cuda")
    x_ident, x_affine, x_full, inten = up(ident), up(affine), up(draws["xform"]), up(draws["intensity"])
    fields = full.make_fields(draws, B, plain._ext0[::-1], "cuda")
    sample = lambda xf, f, it, th: (lambda: L.call("sp_patch_sample_batch", *groups(th), O.ptr(xf), O.ptr(f) if f is not None else None,
                                                   O.ptr(it) if it is not None else None, *dims, O.stream()))
    out_bytes = 4 * (dst0.numel() + dst1.numel())
    src, dst = torch.rand(out_bytes // 4, device="cuda"), torch.empty(out_bytes // 4, device="cuda")
    kern = {"copy": lambda: dst.copy_(src),
            "gather": lambda: L.call("sp_patch_gather_batch", *groups(0.0), *dims, O.stream()),
            "sample, identity": sample(x_ident, None, None, -1.0),
            "sample, rotation + scale": sample(x_affine, None, None, 0.5),
            "sample, rotation + scale + fields + intensity": sample(x_full, fields, inten, 0.5),
            "fields (rng + 3 filter passes)": lambda: full.make_fields(draws, B, plain._ext0[::-1], "cuda")}
    kreps = {k: max(10, int(window_seconds / timed(fn, 20))) for k, fn in kern.items()}
    times, ktimes = {k: [] for k in epoch}, {k: [] for k in kern}
    for _ in range(windows):
        for k, fn in epoch.items():      # alternate: a drift of the machine hits all alike
            times[k].append(timed(fn, reps[k]) / nb * 1e3)
        for k, fn in kern.items():
            ktimes[k].append(timed(fn, kreps[k]) * 1e3)
    return dict(batch_size=plain.batch_size, batches_per_epoch=nb, cases=len(cache), output_bytes=out_bytes,
                loaders={k: dict(epochs_per_window=reps[k], **summary(v)) for k, v in times.items()},
                kernel={k: dict(launches_per_window=kreps[k], **summary(v)) for k, v in ktimes.items()})


def measure_training(k_epochs):
    out = {}
    env = dict(os.environ, MPLBACKEND="Agg")
    with tempfile.TemporaryDirectory() as tmp:
        for name, extra in (("cached", []), ("cached + patchaugment", ["--patchaugment"])):
            wall = {}
            for n in (1, 1 + k_epochs):
                cmd = [sys.executable, os.path.join(PKG, "train_unet_segmentation.py"), os.path.join(tmp, "unet.model"), "--devicecache", "--graph",
                       "--fusedadam", "--epochs", str(n), "--outbasepath", os.path.join(tmp, "unet")] + extra
                t0 = time.perf_counter()
                subprocess.run(cmd, check=True, cwd=ROOT, env=env, stdout=subprocess.DEVNULL, timeout=1500)
                wall[n] = time.perf_counter() - t0
            out[name] = dict(wall_1_epoch_s=wall[1], wall_all_epochs_s=wall[1 + k_epochs], epochs=k_epochs,
                             seconds_per_epoch=(wall[1 + k_epochs] - wall[1]) / k_epochs)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-seconds", type=float, default=0.3)
    ap.add_argument("--train-epochs", type=int, default=3, help="K of the end-to-end leg")
    ap.add_argument("--no-train", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_patchaugment: needs the GPU (no CPU path, no CPU timing)")
    random.seed(0)
    torch.manual_seed(0)
    res = measure(args.windows, args.window_seconds)
    print("U-Net chain, batch %d, %d batches per epoch, %d cached cases, %.1f MB written per batch" %
          (res["batch_size"], res["batches_per_epoch"], res["cases"], res["output_bytes"] / 1e6))
    for k, r in res["loaders"].items():
        print("loader %-22s %9.3f ms per batch  (windows %.3f .. %.3f, spread %.1f %%, %d epochs per window)" %
              (k, r["median_ms"], r["min_ms"], r["max_ms"], 100 * r["spread"], r["epochs_per_window"]))
    g, c = res["kernel"]["gather"]["median_ms"], res["kernel"]["copy"]["median_ms"]
    for k, r in res["kernel"].items():
        print("kernel %-46s %8.1f us  (windows %.1f .. %.1f, spread %.1f %%): %.2fx the gather, %.2fx the copy" %
              (k, 1e3 * r["median_ms"], 1e3 * r["min_ms"], 1e3 * r["max_ms"], 100 * r["spread"], r["median_ms"] / g, r["median_ms"] / c))
    if not args.no_train:
        res["training"] = measure_training(args.train_epochs)
        for name, r in res["training"].items():
            print("train_unet_segmentation.py --devicecache --graph --fusedadam, %-21s: %.2f s per epoch (%d epochs: %.1f s - %.1f s)" %
                  (name, r["seconds_per_epoch"], r["epochs"], r["wall_all_epochs_s"], r["wall_1_epoch_s"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
