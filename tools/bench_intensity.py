"""``--intensityaugment`` at the defaults of train_unet_segmentation.py (pad 20, patches 104 x 104 x 68, --xyresample 0.5, batch size 6, all
29 cases): the cached training loader without the transform, with ``data.IntensityAugment`` at its default probabilities and with every
stage on for every sample, in ONE process, alternated in windows of whole epochs with a device synchronise around each window.  In the
same windows the kernels alone on the images of one full batch: ``sp_intensity_stats_partials``, ``sp_intensity_apply_batch`` (all-neutral
rows; gain only; every stage) and the three passes of ``sp_blur3d_reflect_batch``, each against ``dst.copy_(src)`` of the same bytes.
Reported: the median over the windows and the window spread ((max - min) / median).

    SP_SYNTHETIC_DATA=1 python tools/bench_intensity.py [--windows 5] [--window-seconds 0.3]
"""
import argparse
import contextlib
import io
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "stroke-prediction_amd")
sys.path.insert(0, ROOT)
sys.path.insert(0, PKG)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import stroke_prediction_amd  # noqa: E402,F401
from stroke_prediction_amd.common import data as D, util  # noqa: E402

ALL_ON = dict(p_noise=1, p_blur=1, p_blur_channel=1, p_gain=1, p_contrast=1, p_gamma=1)


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
    make = lambda bt: D.CachedBatchLoader(cache, items, plain.batch_size, chain, batch_transform=bt)
    loaders = {"plain": plain,
               "intensity, default probabilities": make(D.IntensityAugment(seed=args.seed)),
               "intensity, every stage on": make(D.IntensityAugment(seed=args.seed, **ALL_ON))}
    epoch = {k: (lambda ld=ld: [None for _ in ld]) for k, ld in loaders.items()}
    nb = len(plain)
    reps = {}
    for k, fn in epoch.items():          # warm-up, then size the windows in whole epochs
        timed(fn, 1)
        reps[k] = max(1, int(window_seconds / timed(fn, 1)))
    # the kernels alone on the images of one FULL batch (an epoch's last batch may be short)
    src = plain.make_batch(items[:plain.batch_size])[D.KEY_IMAGES]
    B, C0, Z, Y, X = src.shape
    nf, per_field = B * C0, Z * Y * X
    dst, tmp = torch.empty_like(src), torch.empty_like(src)
    partials = torch.empty((nf, 64, 4), dtype=torch.float32, device="cuda")
    draws = D.IntensityAugment(seed=args.seed, **ALL_ON).draw(B, C0)
    neutral = np.zeros((nf, 8), dtype=np.float32)
    neutral[:, 1:4] = 1
    gain = neutral.copy()
    gain[:, 1] = 1.1
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    p_neutral, p_gain, p_full, weights = up(neutral), up(gain), up(draws["params"]), up(draws["weights"])
    seed, call = args.seed, 0
    stats = lambda p: (lambda: L.call("sp_intensity_stats_partials", O.ptr(src), O.ptr(p), O.ptr(partials), nf, per_field, seed, call, O.stream()))
    apply = lambda p: (lambda: L.call("sp_intensity_apply_batch", O.ptr(src), O.ptr(dst), O.ptr(p), O.ptr(partials), nf, per_field, seed, call,
                                      O.stream()))
    stats(p_full)()      # the partials the apply rows read
    kern = {"copy": lambda: dst.copy_(src),
            "stats, no noise": stats(p_neutral),
            "stats, noise": stats(p_full),
            "apply, all-neutral rows": apply(p_neutral),
            "apply, gain only": apply(p_gain),
            "apply, every stage": apply(p_full),
            "blur (3 passes, radius %d)" % draws["radius"]: lambda: L.call("sp_blur3d_reflect_batch", O.ptr(src), O.ptr(dst), O.ptr(tmp),
                                                                           O.ptr(weights), nf, Z, Y, X, draws["radius"], O.stream())}
    kreps = {k: max(10, int(window_seconds / timed(fn, 20))) for k, fn in kern.items()}
    times, ktimes = {k: [] for k in epoch}, {k: [] for k in kern}
    for _ in range(windows):
        for k, fn in epoch.items():      # alternate: a drift of the machine hits all alike
            times[k].append(timed(fn, reps[k]) / nb * 1e3)
        for k, fn in kern.items():
            ktimes[k].append(timed(fn, kreps[k]) * 1e3)
    return dict(batch_size=plain.batch_size, batches_per_epoch=nb, cases=len(cache), image_bytes=4 * src.numel(),
                loaders={k: dict(epochs_per_window=reps[k], **summary(v)) for k, v in times.items()},
                kernel={k: dict(launches_per_window=kreps[k], **summary(v)) for k, v in ktimes.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-seconds", type=float, default=0.3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_intensity: needs the GPU (no CPU path, no CPU timing)")
    random.seed(0)
    torch.manual_seed(0)
    res = measure(args.windows, args.window_seconds)
    print("U-Net chain, batch %d, %d batches per epoch, %d cached cases, images of a batch: %.1f MB" %
          (res["batch_size"], res["batches_per_epoch"], res["cases"], res["image_bytes"] / 1e6))
    for k, r in res["loaders"].items():
        print("loader %-34s %9.3f ms per batch  (windows %.3f .. %.3f, spread %.1f %%, %d epochs per window)" %
              (k, r["median_ms"], r["min_ms"], r["max_ms"], 100 * r["spread"], r["epochs_per_window"]))
    c = res["kernel"]["copy"]["median_ms"]
    for k, r in res["kernel"].items():
        print("kernel %-28s %8.1f us  (windows %.1f .. %.1f, spread %.1f %%): %.2fx the copy" %
              (k, 1e3 * r["median_ms"], 1e3 * r["min_ms"], 1e3 * r["max_ms"], 100 * r["spread"], r["median_ms"] / c))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
