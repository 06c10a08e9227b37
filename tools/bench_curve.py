"""The time-to-treatment curve of one case (tester/CaeReconstructionTesterCurve.py): the literal loop -- one ``inference_step`` and
one ``batch_metrics_step`` per point, the reference's flow -- against the batched path (one ``inference_curve`` call, the T
predictions measured by ``sp_binary_measures_many``).  One case of 1 x 1 x 28 x 128 x 128 through a CAE with the
BASELINE.json configs[2] channels in eval mode, 27 and 32 points.  Both paths are warmed up, then timed alternately in this one
process, the device synchronised before every clock read; per-case milliseconds and their spread over the windows are printed.

    python tools/bench_curve.py [--reps N] [--windows K] [--points 27 32] [--once]

``--once``: one case per path and point count after the warm-up, no timing -- the run to put under
``rocprofv3 --kernel-trace --stats`` for the launch counts (markers on stdout say which path ran how often)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import stroke_prediction_amd  # noqa: E402,F401
from common import data  # noqa: E402
from tester.CaeReconstructionTesterCurve import CaeReconstructionTesterCurve  # noqa: E402
from common.model.Cae3D import Cae3D, Enc3D, Dec3D  # noqa: E402
from oracle import weights as W  # noqa: E402


class _OneCase:
    batch_size = 1

    def __init__(self, batch):
        self._batch = batch

    def __iter__(self):
        return iter([self._batch])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=4, help="cases per timing window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--points", type=int, nargs="+", default=[27, 32])
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--path", choices=["both", "literal", "batched"], default="both")
    args = ap.parse_args()
    channels = [1, 16, 24, 32, 100, 800, 1]      # BASELINE.json configs[2]: --channelscae 1 16 24 32 100 800 1
    torch.manual_seed(0)
    cae = Cae3D(Enc3D(128, 28, channels, 5, 1.0), Dec3D(128, 28, channels, 5, 1.0)).cuda()
    labels, clinical = W.cae_inputs(1, 28, 128, 0)
    batch = {data.KEY_CASE_ID: torch.tensor([1]), data.KEY_LABELS: labels.cuda(), data.KEY_GLOBAL: clinical.float(), data.KEY_IMAGES: []}
    sync = torch.cuda.synchronize
    print("channels %s, case 1x1x28x128x128, eval mode, bf16" % channels)
    for npts in args.points:
        fixed = {27: range(6), 32: range(11)}.get(npts)
        if fixed is None:
            raise SystemExit("--points: 27 (range(6)) or 32 (range(11))")
        tester = CaeReconstructionTesterCurve(_OneCase(batch), cae, None, 10, fixed)
        points = tester.schedule(batch)
        assert len(points) == npts

        def literal():
            return [tester.infer_batch(batch, step) for step, _ in points]

        def batched():
            return tester.infer_curve(batch, points)
        run = [(n, f) for n, f in (("literal", literal), ("batched", batched)) if args.path in ("both", n)]
        for _, f in run:      # warm-up: contexts, workspaces, weight packs
            f(); f()
        sync()
        if args.path == "both":
            a, b = literal(), batched()
            worst = max(abs(x[0].lesion.dc - y[0].lesion.dc) for x, y in zip(a, b))
            print("T=%d: max |DC literal - DC batched| over the points %.2e" % (npts, worst))
        if args.once:
            for n, f in run:
                f()
                sync()
                print("T=%d: ran %s once" % (npts, n))
            continue
        ms = {n: [] for n, _ in run}
        for _ in range(args.windows):
            for n, f in run:      # alternate the paths window by window
                sync()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    f()
                sync()
                ms[n].append((time.perf_counter() - t0) / args.reps * 1e3)
        for n, v in ms.items():
            print("T=%d %-8s per case: median %.1f ms, min %.1f, max %.1f (windows of %d cases: %s)"
                  % (npts, n, statistics.median(v), min(v), max(v), args.reps, " ".join("%.1f" % x for x in v)))
        if len(ms) == 2:
            print("T=%d: literal / batched = %.2f (medians); slowest batched window %.1f ms vs fastest literal window %.1f ms"
                  % (npts, statistics.median(ms["literal"]) / statistics.median(ms["batched"]), max(ms["batched"]), min(ms["literal"])))


if __name__ == "__main__":
    main()
