"""Augmentation of one CAE training batch (B = 4 samples, 3 label channels of 128 x 128 x 28: HemisphericFlip + ElasticDeform),
three paths in ONE process, alternated in windows with a device synchronise around each window:

  1  per sample, host noise     data.HemisphericFlip -> data.ElasticDeform()                     (what the scripts do by default)
  2  per sample, device noise   data.HemisphericFlip -> data.ElasticDeform(device_noise=True)
  3  per batch                  data.BatchElasticDeform(flip="random", noise="philox")           (--batchaugment)

Paths 1 and 2 end in ToTensor + stack (the collate step), so all three deliver a (B, 3, 28, 128, 128) device batch.  Reports the
median time per batch over the windows and the window spread ((max - min) / median), and -- from one
`rocprofv3 --kernel-trace --stats` run of its own (no counters) -- the kernel dispatches per batch and the device time of each
kernel.  In that run one batch of each path is traced after a warm-up batch; a one-element sp_rng_uniform_pm1 launch marks the
boundaries between the sections in the trace.

    python tools/bench_augment.py [--windows 7] [--window-seconds 0.3] [--out DIR] [--no-trace]
"""
import argparse
import csv
import glob
import json
import os
import random
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import stroke_prediction_amd  # noqa: E402,F401
from stroke_prediction_amd.common import data as D  # noqa: E402

B, C, XY, Z = 4, 3, 128, 28
NAMES = {1: "per-sample, host noise", 2: "per-sample, device noise", 3: "per-batch, philox"}
MARK = "rng_uniform_pm1_kernel"


def make_paths():
    samples = [D.to_device(D.synthetic_sample(b + 1, xy=XY, z=Z, n_modalities=0)) for b in range(B)]
    batch = {D.KEY_CASE_ID: torch.arange(1, B + 1), D.KEY_IMAGES: [], D.KEY_GLOBAL: torch.stack([s[D.KEY_GLOBAL] for s in samples]),
             D.KEY_LABELS: torch.stack([D.ToTensor()(s)[D.KEY_LABELS] for s in samples]).contiguous()}

    def per_sample(noise):
        chain = D.Compose([D.HemisphericFlip(), D.ElasticDeform(device_noise=noise), D.ToTensor()])

        def run():
            # ElasticDeform writes into its sample: every batch starts from fresh copies, as a loader's samples are fresh uploads
            out = [chain(dict(s, labels=s[D.KEY_LABELS].clone()))[D.KEY_LABELS] for s in samples]
            return torch.stack(out)
        return run
    bed = D.BatchElasticDeform(flip="random", noise="philox", seed=1)
    return {1: per_sample(False), 2: per_sample(True), 3: lambda: bed(batch)[D.KEY_LABELS]}


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def measure(windows, window_seconds):
    paths = make_paths()
    reps = {}
    for k, fn in paths.items():          # warm-up (code objects, allocator), then size the windows
        timed(fn, 2)
        reps[k] = max(2, int(window_seconds / timed(fn, 3)) + 1)
    times = {k: [] for k in paths}
    for _ in range(windows):
        for k, fn in paths.items():      # alternate: a drift of the machine hits all three alike
            times[k].append(timed(fn, reps[k]) * 1e3)
    res = {}
    for k, v in times.items():
        med = float(np.median(v))
        res[k] = dict(path=NAMES[k], median_ms=med, min_ms=min(v), max_ms=max(v), spread=(max(v) - min(v)) / med, batches_per_window=reps[k])
    return res


def trace_child():
    """the traced program: warm-up, then marker | path 1 | marker | path 2 | marker | path 3 | marker"""
    from stroke_prediction_amd.runtime import lib as L, ops as O
    paths = make_paths()
    for fn in paths.values():
        fn()
    torch.cuda.synchronize()
    one = torch.empty(4, dtype=torch.float32, device="cuda")
    mark = lambda: (torch.cuda.synchronize(), L.call("sp_rng_uniform_pm1", O.ptr(one), 1, 1, 0, 0, O.stream()), torch.cuda.synchronize())
    mark()
    for k in (1, 2, 3):
        paths[k]()
        mark()


def trace(outdir):
    tdir = os.path.join(outdir, "augment_trace")
    cmd = [shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tdir, "-o", "augment", "--",
           sys.executable, os.path.abspath(__file__), "--trace-child"]
    subprocess.run(cmd, check=True, cwd=ROOT, timeout=600)
    files = glob.glob(os.path.join(tdir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise RuntimeError("rocprofv3 left no kernel trace under %s" % tdir)
    with open(files[0]) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    # the generator kernel runs five times after the warm-up: marker, marker, marker, path 3's own launch, marker
    rng = [i for i, r in enumerate(rows) if MARK in r["Kernel_Name"]]
    if len(rng) < 5:
        raise RuntimeError("expected 4 section markers and path 3's launch in the trace, found %d generator launches" % len(rng))
    marks = rng[-5:-2] + rng[-1:]
    out = {}
    for k, (a, b) in zip((1, 2, 3), zip(marks[:-1], marks[1:])):
        per = {}
        for r in rows[a + 1:b]:
            name = r["Kernel_Name"].split("(")[0][:70]
            n, t = per.get(name, (0, 0))
            per[name] = (n + 1, t + int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
        out[k] = dict(dispatches=b - a - 1, kernel_us=sum(t for _, t in per.values()) / 1e3,
                      kernels=sorted(([n, c, t / 1e3] for n, (c, t) in per.items()), key=lambda e: -e[2]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-seconds", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "augment"), help="directory for the kernel trace")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment: needs the GPU (no CPU path, no CPU timing)")
    random.seed(0)
    if args.trace_child:
        return trace_child()
    res = measure(args.windows, args.window_seconds)
    for k, r in res.items():
        print("path %d  %-26s %8.3f ms per batch  (windows %.3f .. %.3f, spread %.1f %%, %d batches per window)" %
              (k, r["path"], r["median_ms"], r["min_ms"], r["max_ms"], 100 * r["spread"], r["batches_per_window"]))
    gain = res[2]["median_ms"] - res[3]["median_ms"]
    noise = max(res[2]["max_ms"] - res[2]["min_ms"], res[3]["max_ms"] - res[3]["min_ms"])
    print("path 3 against path 2: %.2fx, %.3f ms per batch saved; largest window spread of the two %.3f ms -> %s" %
          (res[2]["median_ms"] / res[3]["median_ms"], gain, noise, "beats it" if gain > noise else "NOT outside the spread"))
    tr = None
    if not args.no_trace:
        os.makedirs(args.out, exist_ok=True)
        tr = trace(args.out)
        for k, t in tr.items():
            print("path %d: %d kernel dispatches per batch, %.1f us of kernel time" % (k, t["dispatches"], t["kernel_us"]))
            for name, n, us in t["kernels"][:8]:
                print("    %-70s x%-4d %9.1f us" % (name, n, us))
    print(json.dumps(dict(batch=[B, C, Z, XY, XY], paths={str(k): r for k, r in res.items()}, trace={str(k): t for k, t in (tr or {}).items()})))


if __name__ == "__main__":
    main()
