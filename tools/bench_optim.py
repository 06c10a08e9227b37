"""The fused optimiser step (``optim.FusedAdam`` / ``FusedAdamW`` / ``FusedSGD``) of every kind, with and without gradient
clipping, launched eagerly and inside a captured graph, at two sizes: the flat parameter buffer of the headline U-Net
(2 16 32 64 32 16 32 2) and of the CAE of BASELINE configs[2] (1 16 24 32 100 800 1).

The baseline is ``FusedAdam(capturable=True)`` without clipping (``sp_adam_step_flat_hyp``, the step of every ``--graph`` training
so far).  One process; every path has a parameter, gradient and state of its own, is warmed up, then the paths are timed
alternately in windows, the device synchronised before every clock read.  Eager: microseconds per ``step()`` call (Python and
launch overhead included).  Captured: one graph of ``--chain`` consecutive steps per path, microseconds per step of a replay --
what the step adds to a captured training step.  Median, min and max over the windows.

    python tools/bench_optim.py [--reps N] [--windows K] [--chain C] [--out table.md]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import stroke_prediction_amd  # noqa: E402,F401
from stroke_prediction_amd import optim  # noqa: E402

DEV = "cuda:0"


def flat_sizes():
    from stroke_prediction_amd.common.model.Unet3D import Unet3D
    from stroke_prediction_amd.common.model.Cae3D import Cae3D, Dec3D, Enc3D
    unet = Unet3D([2, 16, 32, 64, 32, 16, 32, 2], dtype="bf16")
    ch = [1, 16, 24, 32, 100, 800, 1]
    cae = Cae3D(Enc3D(128, 28, ch, 5, 1.0, dtype="bf16"), Dec3D(128, 28, ch, 5, 1.0, dtype="bf16"))
    return (("U-Net 2 16 32 64 32 16 32 2", sum(p.numel() for p in unet.parameters() if p.requires_grad)),
            ("CAE 1 16 24 32 100 800 1", sum(p.numel() for p in cae.parameters() if p.requires_grad)))


def make_paths(n, gen):
    p0 = torch.randn(n, generator=gen)
    g0 = torch.randn(n, generator=gen) * 1e-3
    norm = float(g0.double().norm())
    adam = dict(lr=1e-3, betas=(0.99, 0.999), weight_decay=1e-5)
    sgd = dict(lr=1e-2, momentum=0.99, weight_decay=1e-5)
    paths = []
    for name, cls, kw in (("adam (baseline)", optim.FusedAdam, adam), ("adamw", optim.FusedAdamW, adam), ("sgd", optim.FusedSGD, dict(sgd, nesterov=False)),
                          ("sgd-nesterov", optim.FusedSGD, dict(sgd, nesterov=True))):
        for clip in (None, 0.5 * norm):      # half the actual norm: the clipped path really scales
            p = torch.nn.Parameter(p0.to(DEV).clone())
            p.grad = g0.to(DEV).clone()
            opt = cls([p], capturable=True, max_grad_norm=clip, **kw)
            label = name if clip is None else name.replace(" (baseline)", "") + " + clip"
            paths.append((label, opt))
    return paths


def timed(paths, reps, windows, per_call):
    sync = torch.cuda.synchronize
    us = {n: [] for n, _ in paths}
    for _ in range(windows):
        for n, f in paths:      # alternate the paths window by window
            sync()
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            sync()
            us[n].append((time.perf_counter() - t0) / reps / per_call * 1e6)
    return {n: (statistics.median(v), min(v), max(v)) for n, v in us.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200, help="calls per timing window")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--chain", type=int, default=20, help="optimiser steps per captured graph")
    ap.add_argument("--out", type=str, default=None, help="also write the tables (markdown) to this file")
    args = ap.parse_args()
    gen = torch.Generator().manual_seed(0)
    lines = ["device: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__), ""]
    for title, n in flat_sizes():
        paths = make_paths(n, gen)
        for _, opt in paths:      # warm-up: flat groups, the hyper-parameter block, the norm's buffers, code objects
            opt.step(); opt.step()
        torch.cuda.synchronize()
        eager = timed([(name, opt.step) for name, opt in paths], args.reps, args.windows, 1)
        graphs = []
        for name, opt in paths:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(args.chain):
                    opt.step()
            opt.push_hyper()
            g.replay()
            graphs.append((name, g.replay))
        torch.cuda.synchronize()
        captured = timed(graphs, max(1, args.reps // 4), args.windows, args.chain)
        # the algorithm's traffic: p, g and the state read, p and the state written (+ g once more for the norm)
        lines += ["### %s: %d parameters (%.1f MB per fp32 buffer)" % (title, n, 4 * n / 1e6), "",
                  "| step | eager us (median, min - max) | captured us per step (median, min - max) | launches | MB moved |", "|---|---|---|---|---|"]
        for name, opt in paths:
            clip = name.endswith("+ clip")
            bufs = (5 if "sgd" in name else 7) + (1 if clip else 0)
            e, c = eager[name], captured[name]
            lines.append("| %s | %.1f (%.1f - %.1f) | %.2f (%.2f - %.2f) | %d | %.1f |"
                         % (name, e[0], e[1], e[2], c[0], c[1], c[2], (1 if "sgd" in name else 2) + (1 if clip else 0), bufs * 4 * n / 1e6))
        lines.append("")
    lines += ["launches: the update kernel, the step counter's increment of the Adams (an ``add_`` on the device scalar), and with clipping",
              "the norm's first stage (``sp_grad_sqnorm_partials``).", ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
