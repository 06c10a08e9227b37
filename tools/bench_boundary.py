"""The boundary (signed-distance) criterion on the device (``--criterion diceboundary``) against ``--criterion dice``: what a training
step pays for it.

Two shapes: the headline label shape 4 x 2 x 88^3 and the U-Net patch shape 6 x 2 x 28 x 64 x 64.  Per shape, three paths:

* ``dice``: ``BatchDiceLoss([1, 1])`` forward + backward (``sp_dice_*``) -- what every step pays without the flag;
* ``diceboundary``: ``DiceBoundaryLoss([1, 1])`` forward + backward (``sp_signed_distance_batch`` + ``sp_bloss_*``);
* ``signed distance``: the ``sp_signed_distance_batch`` launches alone (seed, one scan per axis, roots).

One process; every path is warmed up, then the paths are timed alternately in windows, the device synchronised before every clock
read; microseconds per call (median over the windows, min, max).  The number to report is diceboundary - dice: the added time per
training step.

    python tools/bench_boundary.py [--reps N] [--windows K] [--once]

``--once``: one call per path after the warm-up, no timing -- the run to put under ``rocprofv3 --kernel-trace --stats`` for the launch
counts (markers on stdout say which path ran)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import stroke_prediction_amd  # noqa: E402,F401
from common import metrics  # noqa: E402


def timed(paths, reps, windows, once):
    sync = torch.cuda.synchronize
    for _, f in paths:      # warm-up: accumulators, cached weights, code objects, the allocator's blocks
        f(); f()
    sync()
    if once:
        for n, f in paths:
            f()
            sync()
            print("ran %s once" % n)
        return {}
    us = {n: [] for n, _ in paths}
    for _ in range(windows):
        for n, f in paths:      # alternate the paths window by window
            sync()
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            sync()
            us[n].append((time.perf_counter() - t0) / reps * 1e6)
    med = {}
    for n, v in us.items():
        med[n] = statistics.median(v)
        print("%-34s per call: median %8.1f us, min %8.1f, max %8.1f" % (n, med[n], min(v), max(v)))
        print("%-34s windows: %s" % ("", " ".join("%.1f" % x for x in v)))
    return med


def lesion_labels(shape, g):
    """labels like the workload's: one ellipsoid per volume taking a few percent of it (a thresholded noise field would make every
    distance 1 or 2 and says nothing about the scan, whose cost does not depend on the mask anyway)"""
    B, C, D, H, W = shape
    z, y, x = torch.meshgrid(torch.arange(D), torch.arange(H), torch.arange(W), indexing="ij")
    lab = torch.zeros(shape)
    for b in range(B):
        for c in range(C):
            cz, cy, cx = (torch.rand(3, generator=g) * torch.tensor([D, H, W]) * 0.5 + torch.tensor([D, H, W]) * 0.25).tolist()
            r = (0.1 + 0.15 * float(torch.rand(1, generator=g))) * (c + 1)
            lab[b, c] = ((((z - cz) / (r * D)) ** 2 + ((y - cy) / (r * H)) ** 2 + ((x - cx) / (r * W)) ** 2) <= 1.0).float()
    return lab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50, help="calls per timing window")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    for shape in ((4, 2, 88, 88, 88), (6, 2, 28, 64, 64)):
        seg = torch.rand(*shape, generator=g).to(dev).requires_grad_(True)
        lab = lesion_labels(shape, g).to(dev)

        def fwd_bwd(crit):
            def f():
                seg.grad = None
                crit(seg, lab).backward()
            return f
        paths = [("dice (sp_dice_*)", fwd_bwd(metrics.BatchDiceLoss([1.0, 1.0]))),
                 ("diceboundary (sdf + sp_bloss_*)", fwd_bwd(metrics.DiceBoundaryLoss([1.0, 1.0]))),
                 ("signed distance alone", lambda: metrics.signed_distance_batch(lab))]
        print("labels %s fp32, mask fraction %.3f" % ("x".join(map(str, shape)), float(lab.mean())))
        med = timed(paths, args.reps, args.windows, args.once)
        if med:
            print("added per training step over --criterion dice: %.1f us (signed distance alone %.1f us)"
                  % (med[paths[1][0]] - med[paths[0][0]], med[paths[2][0]]))


if __name__ == "__main__":
    main()
