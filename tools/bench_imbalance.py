"""The class-imbalance criteria on the device (``--criterion {tversky,focaltversky,focalbce,tverskyfocalbce}``) against ``dice`` and
``dicebce``, measured in one process.

1. The entry points alone at the headline label shape 4 x 2 x 88^3: ``sp_tloss_sums`` / ``_finalize_clear`` / ``_bwd`` (both terms, focal
   exponent 2 and 2.5) beside ``sp_vloss_sums`` / ``_finalize_clear`` / ``_bwd`` (Dice + BCE), which read and write the same bytes;
   device time per call between two events.
2. Loss forward + backward per criterion on the same tensors, as ``tools/bench_criteria.py`` times it.
3. The headline training step -- U-Net 2 16 32 64 32 16 32 2, bf16, batch 4 of 128^3, ``Learner(graph=True).train_batch`` on the
   step's own input buffers, as ``bench.py`` sets it up -- under each criterion.

Every path is warmed up, then the paths are timed alternately in windows, the device synchronised before every clock read; the median
over the windows, min and max are printed, and the ratio of every criterion to ``dicebce``.

    python tools/bench_imbalance.py [--criteria NAME ...] [--reps N] [--windows K] [--steps N] [--skip-step]

``--criteria`` restricts parts 2 and 3 (``dice dicebce`` runs on a checkout from before the new criteria, part 1 left out)."""
import argparse
import contextlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import stroke_prediction_amd  # noqa: E402,F401
from common import metrics  # noqa: E402

ALL = ["dice", "dicebce", "tversky", "focaltversky", "focalbce", "tverskyfocalbce"]
CHANNELS = [2, 16, 32, 64, 32, 16, 32, 2]


def report(us, unit, yardstick):
    med = {n: statistics.median(v) for n, v in us.items()}
    for n, v in us.items():
        ratio = "   %.3f x %s" % (med[n] / med[yardstick], yardstick) if yardstick in med and n != yardstick else ""
        print("%-52s median %9.3f %s, min %9.3f, max %9.3f%s" % (n, med[n], unit, min(v), max(v), ratio))
    return med


def timed(paths, reps, windows, unit_scale, unit, yardstick):
    """wall time per call of each path: warmed up, alternated window by window"""
    sync = torch.cuda.synchronize
    for _, f in paths:
        f(); f()
    us = {n: [] for n, _ in paths}
    for _ in range(windows):
        for n, f in paths:
            sync()
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            sync()
            us[n].append((time.perf_counter() - t0) / reps * unit_scale)
    return report(us, unit, yardstick)


def entry_points(seg, lab, reps, windows):
    """device time of each of the three launches, between two events around ``reps`` back-to-back calls"""
    from stroke_prediction_amd.runtime import lib as L, ops as O
    B, C = seg.shape[:2]
    dhw = seg[0, 0].numel()
    dev = seg.device
    sums = torch.zeros(L.SP_REDUCE_ROWS, L.SP_VLOSS_PITCH(C), dtype=torch.float64, device=dev)
    w = torch.full((C,), 0.5, device=dev)
    loss, coef, up = torch.empty((), device=dev), torch.empty(3 * C, device=dev), torch.ones((), device=dev)
    d = torch.empty_like(seg)
    o, t, s = O.ptr(seg), O.ptr(lab), O.ptr(sums)
    bs = seg.stride(0)
    count = float(B * dhw)
    paths = [("sp_vloss_sums (dice + bce)", lambda: L.call("sp_vloss_sums", o, bs, t, bs, B, C, dhw, 3, s, O.stream())),
             ("sp_vloss_finalize_clear", lambda: L.call("sp_vloss_finalize_clear", s, O.ptr(w), O.ptr(w), 1e-7, count, C, O.ptr(loss), O.ptr(coef), O.stream())),
             ("sp_vloss_bwd", lambda: L.call("sp_vloss_bwd", o, bs, t, bs, O.ptr(coef), O.ptr(up), B, C, dhw, O.ptr(d), O.stream()))]
    for gamma in (2.0, 2.5):
        tag = " (tversky + focal, gamma %g)" % gamma
        paths += [("sp_tloss_sums" + tag, lambda g=gamma: L.call("sp_tloss_sums", o, bs, t, bs, B, C, dhw, 3, g, 0.25, s, O.stream())),
                  ("sp_tloss_finalize_clear" + tag, lambda: L.call("sp_tloss_finalize_clear", s, O.ptr(w), O.ptr(w), 0.3, 0.7, 4.0 / 3.0, 1e-7, count,
                                                                   C, O.ptr(loss), O.ptr(coef), O.stream())),
                  ("sp_tloss_bwd" + tag, lambda g=gamma: L.call("sp_tloss_bwd", o, bs, t, bs, O.ptr(coef), O.ptr(up), g, 0.25, B, C, dhw, O.ptr(d), O.stream()))]
    for _, f in paths:      # in order: every backward reads coefficients a finalize wrote
        f(); f()
    torch.cuda.synchronize()
    us = {n: [] for n, _ in paths}
    for _ in range(windows):
        for n, f in paths:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            us[n].append(e0.elapsed_time(e1) * 1e3 / reps)
    med = report(us, "us", "")
    for stage in ("sums", "finalize_clear", "bwd"):
        base = med[[n for n in med if n.startswith("sp_vloss_" + stage)][0]]
        for n in med:
            if n.startswith("sp_tloss_" + stage):
                print("%-58s %.3f x sp_vloss_%s" % (n, med[n] / base, stage))


class _LoaderStub:
    def __init__(self, batch_size):
        self.batch_size = batch_size


def step_under(name, dev, batch_size=4, size=128):
    """the headline step as bench.py builds it, under make_criterion(name) -> the step function"""
    from stroke_prediction_amd.common.model.Unet3D import Unet3D
    from stroke_prediction_amd.learner.UnetSegmentationLearner import UnetSegmentationLearner
    from stroke_prediction_amd.optim import FusedAdam, attach_flat_grads
    torch.manual_seed(1234)
    model = Unet3D(CHANNELS, dtype="bf16").to(dev).train()
    out = model.output_size((size,) * 3)
    opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-5, betas=(0.99, 0.999), capturable=True)
    attach_flat_grads(model)
    with contextlib.redirect_stdout(sys.stderr):
        learner = UnetSegmentationLearner(_LoaderStub(batch_size), None, model, opt, None, 1, metrics.make_criterion(name), None,
                                          "/tmp/_bench_imbalance", graph=True, batch_metrics=False, sync_loss=False)
    g = torch.Generator(device=dev).manual_seed(1234)
    images = torch.randn((batch_size, 2) + (size,) * 3, generator=g, device=dev)
    labels = (torch.rand((batch_size, 2) + tuple(out), generator=g, device=dev) > 0.7).float()
    batch = learner.static_batch({"case_id": list(range(batch_size)), "images": images, "labels": labels, "clinical": None}, 0)

    def step():
        return learner.train_batch(batch, 0)
    for _ in range(learner.GRAPH_WARMUP + 1):      # eager warm-ups and the capture
        step()
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--criteria", nargs="+", default=ALL, choices=ALL)
    ap.add_argument("--reps", type=int, default=100, help="calls per timing window (parts 1 and 2)")
    ap.add_argument("--steps", type=int, default=20, help="training steps per timing window (part 3)")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    shape = (4, 2, 88, 88, 88)
    seg = torch.rand(*shape, generator=g).to(dev).requires_grad_(True)
    lab = (torch.rand(*shape, generator=g) > 0.7).float().to(dev)
    two = {"dice": lambda: metrics.BatchDiceLoss([1.0, 1.0]), "dicebce": lambda: metrics.DiceBCELoss([1.0, 1.0]),
           "tversky": lambda: metrics.TverskyLoss([1.0, 1.0]), "focaltversky": lambda: metrics.TverskyLoss([1.0, 1.0], gamma=4.0 / 3.0),
           "focalbce": lambda: metrics.FocalBCELoss(), "tverskyfocalbce": lambda: metrics.TverskyFocalBCELoss([1.0, 1.0])}

    if "tverskyfocalbce" in args.criteria:
        print("1. entry points alone, %s fp32 (device time per launch)" % "x".join(map(str, shape)))
        entry_points(seg.detach(), lab, args.reps, args.windows)

    def fwd_bwd(crit):
        def f():
            seg.grad = None
            crit(seg, lab).backward()
        return f
    print("2. loss forward + backward, segmentation %s fp32 (wall time per call)" % "x".join(map(str, shape)))
    with contextlib.redirect_stdout(sys.stderr):
        paths = [(n, fwd_bwd(two[n]())) for n in args.criteria]
    timed(paths, args.reps, args.windows, 1e6, "us", "dicebce")

    if not args.skip_step:
        print("3. headline training step: U-Net %s bf16, batch 4 x 128^3, Learner(graph=True).train_batch (wall time per step)" % " ".join(map(str, CHANNELS)))
        timed([(n, step_under(n, dev)) for n in args.criteria], args.steps, args.windows, 1e3, "ms", "dicebce")


if __name__ == "__main__":
    main()
