"""Foreground-oversampled patch origins (data.ForegroundOversample, csrc/sp_fgpatch.hip) at the shapes of train_unet_segmentation.py:
the synthetic set, 2 + 2 channels of 28 x 128 x 128, batch 6, patches 104 x 104 x 68, pad 20.  One process, one shared case cache:

  (a)  time per batch of CachedBatchLoader without ``foreground`` (the path of the commit before the feature, in this build: the
       baseline row) and with fractions 1/3 and 1, alternated in windows of whole epochs with a device synchronise around each window;
       median over the windows and the window spread ((max - min) / median)
  (b)  the one-off time of the index build (DeviceCaseCache.foreground_index): the first call, which also loads the kernels, and the
       median of rebuilds
  (c)  over --batches batches per setting: the share of label patches that hold at least one foreground voxel and the mean
       foreground share of a label patch, for fractions 0, 1/3 and 1 -- once with every label channel as foreground (the default)
       and once with channel 0 alone (the core: the rare class of the set)

    SP_SYNTHETIC_DATA=1 python tools/bench_fgpatch.py [--windows 5] [--window-seconds 0.3] [--batches 200] [--out profiles/fg_patch.md]
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

FRACTIONS = (("none", None), ("1/3", 1.0 / 3.0), ("1", 1.0))


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


def build(seed):
    """the script's training loader over the device cache, and loaders with ``foreground`` over the SAME cache, items and chain"""
    import train_unet_segmentation as S
    with contextlib.redirect_stdout(io.StringIO()):      # the parser prints its namespace, the script its set sizes
        args = util.get_args_unet_training(["/tmp/unet.model", "--devicecache"])
        base = S.build_loaders(args)[0]
    pad = args.padding
    chain = [D.ResamplePlaneXY(args.xyresample), D.HemisphericFlipFixedToCaseId(split_id=args.hemisflipid),
             D.PadImages(pad[0], pad[1], pad[2], pad_value=0), D.RandomPatch(*S.PATCH, pad[0], pad[1], pad[2]), D.ToTensor()]
    make = lambda f, channels=None: D.CachedBatchLoader(base.cache, list(base.sampler.indices), base.batch_size, chain,
                                                        foreground=D.ForegroundOversample(f, channels, seed=seed) if f is not None else None)
    return base, make


def measure_index(cache, rebuilds):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cache.foreground_index()
    torch.cuda.synchronize()
    first = time.perf_counter() - t0
    again = []
    for _ in range(rebuilds):
        cache._fg_index.clear()
        again.append(timed(cache.foreground_index, 1) * 1e3)
    return dict(first_call_ms=first * 1e3, rebuild=summary(again), rebuilds=rebuilds, bytes=int(cache.foreground_index().numel()) * 4)


def measure_time(make, windows, window_seconds):
    loaders = {name: make(f) for name, f in FRACTIONS}
    epoch = {k: (lambda ld=ld: [None for _ in ld]) for k, ld in loaders.items()}
    nb = len(loaders["none"])
    reps = {}
    for k, fn in epoch.items():          # warm-up, then size the windows in whole epochs
        timed(fn, 1)
        reps[k] = max(1, int(window_seconds / timed(fn, 1)))
    times = {k: [] for k in epoch}
    for _ in range(windows):
        for k, fn in epoch.items():      # alternate: a drift of the machine hits all alike
            times[k].append(timed(fn, reps[k]) / nb * 1e3)
    return dict(batches_per_epoch=nb, loaders={k: dict(epochs_per_window=reps[k], **summary(v)) for k, v in times.items()})


def measure_content(make, batches, channels=None):
    """per setting: the label patches of ``batches`` batches, reduced on the device, one read at the end; foreground = ``channels``"""
    out = {}
    for name, f in (("0", 0.0),) + FRACTIONS[1:]:
        loader = make(f, channels)
        random.seed(1)
        torch.manual_seed(1)
        share, n = [], 0
        while n < batches:
            for batch in loader:
                lab = batch[D.KEY_LABELS] if channels is None else batch[D.KEY_LABELS][:, list(channels)]
                fg = (lab > 0.5).any(dim=1).flatten(1).float().mean(dim=1)      # (B,): foreground share per patch
                share.append(fg)
                n += 1
                if n == batches:
                    break
        share = torch.cat(share).cpu().numpy()
        out[name] = dict(patches=int(share.size), with_foreground=float((share > 0).mean()), mean_foreground_share=float(share.mean()))
    return out


def report(res):
    t, ix, c = res["time"], res["index"], res["content"]
    base = t["loaders"]["none"]["median_ms"]
    lines = ["# Foreground-oversampled patch origins: `tools/bench_fgpatch.py`", "",
             "Chain of `train_unet_segmentation.py` at its defaults (`ResamplePlaneXY(0.5)` → `HemisphericFlipFixedToCaseId(15)` →",
             "`PadImages(20, 20, 20)` → `RandomPatch(104, 104, 68, 20, 20, 20)` → `ToTensor`), the synthetic set, 2 + 2 channels of",
             "28×128×128, batch %d, %d training cases, %d batches per epoch; the label patch is 64×64×28.  One process, one shared" %
             (res["batch_size"], res["train_cases"], t["batches_per_epoch"]),
             "`DeviceCaseCache` of %d cases; foreground = any label channel above 0.5.  Measured on %s." % (res["cases"], res["device"]), "",
             "## (a) Time per batch", "",
             "The loaders alternated in windows of whole epochs, a device synchronise around every window; median over %d windows," % res["windows"],
             "spread = (max − min) / median.  The first row is `CachedBatchLoader` without `foreground`: the path of the commit before the",
             "feature, in the same build.", "",
             "| `foreground` | ms per batch | windows (min .. max) | spread | against the baseline |", "|---|---|---|---|---|"]
    for name, _ in FRACTIONS:
        r = t["loaders"][name]
        lines.append("| %s | %.3f | %.3f .. %.3f | %.1f %% | %+.3f ms |" % ("none (baseline)" if name == "none" else "fraction " + name, r["median_ms"],
                                                                        r["min_ms"], r["max_ms"], 100 * r["spread"], r["median_ms"] - base))
    lines += ["", "## (b) Index build (one-off)", "",
              "`DeviceCaseCache.foreground_index()`: two launches of `sp_fg_row_index` over %d cases, %d bytes of prefix sums." %
              (res["cases"], ix["bytes"]), "",
              "| | ms |", "|---|---|",
              "| first call (loads the kernels) | %.3f |" % ix["first_call_ms"],
              "| rebuild, median of %d (min .. max) | %.3f (%.3f .. %.3f) |" % (ix["rebuilds"], ix["rebuild"]["median_ms"], ix["rebuild"]["min_ms"],
                                                                             ix["rebuild"]["max_ms"]), "",
              "## (c) What the patches hold", "",
              "%d batches per setting, `random.seed(1)`, `ForegroundOversample(seed=%d)`." % (res["batches"], res["seed"]), "",
              "| fraction | label patches | with at least one foreground voxel | mean foreground share of a label patch |", "|---|---|---|---|"]
    for name in ("0", "1/3", "1"):
        r = c[name]
        lines.append("| %s | %d | %.1f %% | %.2f %% |" % (name, r["patches"], 100 * r["with_foreground"], 100 * r["mean_foreground_share"]))
    lines += ["", "The same with channel 0 alone (the core) as foreground, `ForegroundOversample(channels=[0])`, counting channel 0:", "",
              "| fraction | label patches | with at least one core voxel | mean core share of a label patch |", "|---|---|---|---|"]
    for name in ("0", "1/3", "1"):
        r = res["content_core"][name]
        lines.append("| %s | %d | %.1f %% | %.2f %% |" % (name, r["patches"], 100 * r["with_foreground"], 100 * r["mean_foreground_share"]))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-seconds", type=float, default=0.3)
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--rebuilds", type=int, default=9)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "fg_patch.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fgpatch: needs the GPU (no CPU path, no CPU timing)")
    random.seed(0)
    torch.manual_seed(0)
    base, make = build(args.seed)
    res = dict(device="%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]), batch_size=base.batch_size, cases=len(base.cache), train_cases=len(base.sampler.indices),
               windows=args.windows, batches=args.batches, seed=args.seed)
    res["index"] = measure_index(base.cache, args.rebuilds)
    res["time"] = measure_time(make, args.windows, args.window_seconds)
    res["content"] = measure_content(make, args.batches)
    res["content_core"] = measure_content(make, args.batches, channels=[0])
    text = report(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
