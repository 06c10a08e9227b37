"""Input pipeline of train_unet_segmentation.py at its defaults (pad 20, patches 104 x 104 x 68, --xyresample 0.5, the script's batch
size, all 29 cases), two loaders in ONE process, alternated in windows with a device synchronise around each window:

  1  per sample   data.get_stroke_shape_training_data(...)                      decode / synthesise, upload, resample, flip, pad, cut, stack
  2  cached       data.get_stroke_shape_training_data(..., device_cache=True)   one table upload + one sp_patch_gather_batch launch

A window is whole epochs of the training loader; reported: the median time per batch over the windows and the window spread
((max - min) / median).  In the same windows the gather kernel alone is timed against ``dst.copy_(src)`` of the same OUTPUT byte count
-- the yardstick for a pure gather.  Second leg: train_unet_segmentation.py --graph --fusedadam end to end, with and without
--devicecache: the wall time of a run of 1 epoch and of a run of 1 + K epochs, K epochs = the difference (start-up and graph capture
cancel).

    python tools/bench_loader.py [--windows 5] [--window-seconds 0.3] [--train-epochs 3] [--no-train]
"""
import argparse
import ctypes
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

NAMES = {1: "per sample", 2: "cached"}


def script_args(extra=()):
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):      # the parser prints its namespace
        return util.get_args_unet_training(["/tmp/unet.model"] + list(extra))


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


def measure_loaders(windows, window_seconds):
    import train_unet_segmentation as S
    import contextlib
    import io
    loaders = {}
    with contextlib.redirect_stdout(io.StringIO()):
        loaders[1] = S.build_loaders(script_args())[0]
        t0 = time.perf_counter()
        loaders[2] = S.build_loaders(script_args(["--devicecache"]))[0]
        torch.cuda.synchronize()
        fill_s = time.perf_counter() - t0
    cache = loaders[2].cache
    epoch = {k: (lambda ld=ld: [None for _ in ld]) for k, ld in loaders.items()}
    nb = len(loaders[1])
    assert len(loaders[2]) == nb
    reps = {}
    for k, fn in epoch.items():          # warm-up, then size the windows in whole epochs
        timed(fn, 1)
        reps[k] = max(1, int(window_seconds / timed(fn, 1)))
    # the kernel alone on the last batch's table, against a copy of the same output byte count
    from stroke_prediction_amd.runtime import lib as L, ops as O
    ld = loaders[2]
    table = ld.last_table.to("cuda")
    B = table.shape[0]
    i3 = lambda v: (ctypes.c_int32 * 3)(*[int(a) for a in v])
    dst0 = torch.empty((B, cache.images.shape[1]) + tuple(ld._ext0[::-1]), dtype=torch.float32, device="cuda")
    dst1 = torch.empty((B, cache.labels.shape[1]) + tuple(ld._ext1[::-1]), dtype=torch.float32, device="cuda")
    Z, Y, X = cache.shape_zyx
    a = (O.ptr(cache.images), O.ptr(dst0), cache.images.shape[1], i3(ld._ext0), i3(ld._pad0), ld._padval0, O.ptr(cache.labels), O.ptr(dst1),
         cache.labels.shape[1], i3(ld._ext1), i3((0, 0, 0)), 0.0, O.ptr(table), len(cache), B, Z, Y, X)
    gather = lambda: L.call("sp_patch_gather_batch", *a, O.stream())
    out_bytes = 4 * (dst0.numel() + dst1.numel())
    src, dst = torch.rand(out_bytes // 4, device="cuda"), torch.empty(out_bytes // 4, device="cuda")
    copy = lambda: dst.copy_(src)
    kern = {"gather": gather, "copy": copy}
    kreps = {k: max(10, int(window_seconds / timed(fn, 20))) for k, fn in kern.items()}
    times = {k: [] for k in epoch}
    ktimes = {k: [] for k in kern}
    for _ in range(windows):
        for k, fn in epoch.items():      # alternate: a drift of the machine hits both alike
            times[k].append(timed(fn, reps[k]) / nb * 1e3)
        for k, fn in kern.items():
            ktimes[k].append(timed(fn, kreps[k]) * 1e3)
    res = {str(k): dict(path=NAMES[k], epochs_per_window=reps[k], **summary(v)) for k, v in times.items()}
    kres = {k: dict(launches_per_window=kreps[k], **summary(v)) for k, v in ktimes.items()}
    return dict(batch_size=loaders[1].batch_size, batches_per_epoch=nb, cases=len(cache), cache_bytes=cache.nbytes, cache_fill_seconds=fill_s,
                gather_output_bytes=out_bytes, loaders=res, kernel=kres)


def measure_training(k_epochs):
    out = {}
    env = dict(os.environ, MPLBACKEND="Agg")
    with tempfile.TemporaryDirectory() as tmp:
        for name, extra in (("per sample", []), ("cached", ["--devicecache"])):
            wall = {}
            for n in (1, 1 + k_epochs):
                cmd = [sys.executable, os.path.join(PKG, "train_unet_segmentation.py"), os.path.join(tmp, "unet.model"), "--graph", "--fusedadam",
                       "--epochs", str(n), "--outbasepath", os.path.join(tmp, "unet")] + extra
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
        raise SystemExit("bench_loader: needs the GPU (no CPU path, no CPU timing)")
    random.seed(0)
    torch.manual_seed(0)
    res = measure_loaders(args.windows, args.window_seconds)
    print("U-Net chain, batch %d, %d batches per epoch; cache: %d cases, %.1f MB, filled in %.2f s" %
          (res["batch_size"], res["batches_per_epoch"], res["cases"], res["cache_bytes"] / 1e6, res["cache_fill_seconds"]))
    for k, r in res["loaders"].items():
        print("path %s  %-11s %9.3f ms per batch  (windows %.3f .. %.3f, spread %.1f %%, %d epochs per window)" %
              (k, r["path"], r["median_ms"], r["min_ms"], r["max_ms"], 100 * r["spread"], r["epochs_per_window"]))
    one, two = res["loaders"]["1"], res["loaders"]["2"]
    print("cached against per sample: %.1fx, %.3f ms per batch saved" % (one["median_ms"] / two["median_ms"], one["median_ms"] - two["median_ms"]))
    g, c = res["kernel"]["gather"], res["kernel"]["copy"]
    print("sp_patch_gather_batch alone %.1f us (windows %.1f .. %.1f), copy_ of the same %.1f MB %.1f us (%.1f .. %.1f): %.2fx the copy" %
          (1e3 * g["median_ms"], 1e3 * g["min_ms"], 1e3 * g["max_ms"], res["gather_output_bytes"] / 1e6, 1e3 * c["median_ms"], 1e3 * c["min_ms"],
           1e3 * c["max_ms"], g["median_ms"] / c["median_ms"]))
    if not args.no_train:
        res["training"] = measure_training(args.train_epochs)
        for name, r in res["training"].items():
            print("train_unet_segmentation.py --graph --fusedadam, %-10s: %.2f s per epoch (%d epochs: %.1f s - %.1f s)" %
                  (name, r["seconds_per_epoch"], r["epochs"], r["wall_all_epochs_s"], r["wall_1_epoch_s"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
