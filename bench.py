#!/usr/bin/env python3
"""Headline benchmark: train-step voxels/sec of the 3-D U-Net (BASELINE.json configs[1]):
channels 2 16 32 64 32 16 32 2, batch 4 per GPU, 2x128^3 synthetic volumes, bf16 storage / MFMA.

A step = ``Learner.train_batch`` (learner/Learner.py:116-130 of the reference): forward + (Dice+Dice)/2 + zero_grad +
backward + [RCCL all-reduce, bucketed, overlapped with backward] + Adam, without the CPU-side medpy metrics
(excluded on both sides).  The product's own ``Learner(graph=True)`` replays the step as one hipGraph.
Prints ONE JSON line on rank 0 (contract in the task statement).  A plain run sets up, warms up, times ``--steps`` steps
and prints the line; ``--full`` adds what takes runs of its own: ``roofline`` / ``kernels`` (dominant kernel family,
HIP-event timed eager steps), ``parity`` (the other precision modes against the f32 mode), ``cpu_baseline`` (the CPU
oracle on the host cores; all cores and 8 threads), ``secondary`` (the other workloads) and the
input-copy time.  ``--dump-outputs DIR`` writes what the last timed step computed as ``DIR/<name>.npy``.

``--gpus N`` with no WORLD_SIZE in the environment launches its own N ranks (``python -m torch.distributed.run``)
BEFORE anything touches the GPU, forwards rank 0's JSON line and exits with the children's status.

Other workloads: ``--workload cae`` (configs[2]), ``--workload unet4`` (configs[4] topology: 4-scale U-Net),
``--workload unet-infer``.
"""
import argparse
import contextlib
import json
import os
import platform
import socket
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

CHANNELS = [2, 16, 32, 64, 32, 16, 32, 2]
CHANNELS4 = [2, 32, 64, 128, 256, 128, 64, 32, 32, 2]       # configs[4] with ch_bC = 32
CAE_CHANNELS = [1, 16, 24, 32, 100, 800, 1]
# dense MFMA peaks (MI355X_MICROARCH.md): bf16 2.5 PFLOP/s; f32 mode = 3 bf16 MFMAs per product; fp8 (MX-scaled) 5 PFLOP/s
PEAK_TFLOPS = {"bf16": 2500.0, "f16": 2500.0, "f32": 2500.0 / 3.0, "fp8": 5000.0, "fp8b": 5000.0, "bf16x3": 2500.0, "f16x3": 2500.0}      # bf16x3: forward convolutions run 3 MFMAs per product (priced in its own line), backward = bf16
DTYPES = ["bf16", "f32", "fp8", "fp8b", "f16", "bf16x3", "f16x3"]      # precision modes the models accept (fp8: bf16 storage + e4m3 / e5m2 MFMA operands, runtime/f8.py)
HBM_PEAK_GBS = 8000.0
TRAIN_GFLOP_PER_SAMPLE_128 = 345.7                        # SURVEY.md 8d (fwd + dgrad + wgrad)
CAE_TRAIN_GFLOP_PER_SAMPLE = {28: 305.5, 124: 1431.0}     # SURVEY.md 8d (3 enc + 4 dec passes)


# ------------------------------------------------------------------------------------------------ CPU baselines
def _cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or "unknown"


def _usable_cpus():
    """host cores this process may actually use: the affinity mask capped by the cgroup CPU quota (a GPU box hands one
    job a share of a large host: timing 256 threads on a 16-core share measures oversubscription, not the CPU)"""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except (AttributeError, OSError):
        pass
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            with open(path) as f:
                parts = f.read().split()
            if path.endswith("cpu.max"):
                if parts[0] != "max":
                    n = min(n, max(1, int(int(parts[0]) / int(parts[1]))))
            else:
                q = int(parts[0])
                if q > 0:
                    with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                        n = min(n, max(1, q // int(f.read())))
            break
        except (OSError, ValueError, IndexError):
            continue
    return n


def _timed_cpu_steps(step, threads, steps):
    torch.set_num_threads(threads)
    times = []
    for i in range(steps + 1):          # 1 warm-up + `steps` timed, median
        t0 = time.perf_counter()
        step(i)
        times.append(time.perf_counter() - t0)
    return sorted(times[1:])[len(times[1:]) // 2]


def _cpu_report(vox, make_step, desc, steps):
    ncpu = _usable_cpus()
    prev = torch.get_num_threads()
    t_all = _timed_cpu_steps(make_step(), ncpu, steps)
    res = {"value": vox / t_all, "unit": "voxels/s", "cores": ncpu, "kind": "port",
           "os_cpu_count": os.cpu_count(), "cpu_model": _cpu_model(), "s_per_step": t_all,
           "sample": "%s, 1 warm-up + %d timed steps, median; all %d usable host cores (affinity / cgroup quota; the host "
                     "reports %s)" % (desc, steps, ncpu, os.cpu_count())}
    if ncpu != 8:
        t8 = _timed_cpu_steps(make_step(), 8, steps)
        res["threads_8"] = {"value": vox / t8, "s_per_step": t8, "cores": 8}
    torch.set_num_threads(prev)
    return res


def cpu_baseline_unet(size, steps=3, batch=2, channels=CHANNELS):
    """The CPU oracle (fp32 restatement of the reference path, oracle/nets.py) timed on the host cores."""
    from oracle import nets, weights as W

    def make_step():
        sd = W.make_state_dict(W.unet_spec(channels), 1234)
        names = nets.trainable(sd)
        for k in names:
            sd[k].requires_grad_(True)
        x, y = W.unet_inputs(batch, size, 1234, scales=(len(channels) - 2) // 2)
        m = [torch.zeros_like(sd[k]) for k in names]
        v = [torch.zeros_like(sd[k]) for k in names]

        def step(i):
            seg = nets.unet_forward(sd, x, training=True)
            loss = nets.unet_loss(seg, y)
            grads = torch.autograd.grad(loss, [sd[k] for k in names])
            with torch.no_grad():
                nets.adam_step([sd[k] for k in names], grads, m, v, i + 1, lr=1e-3, betas=(0.99, 0.999), weight_decay=1e-5)
        return step
    return _cpu_report(batch * size[0] * size[1] * size[2], make_step,
                       "CPU oracle (fp32), U-Net train step, batch %d x 2x%dx%dx%d" % ((batch,) + tuple(size)), steps)


def cpu_baseline_cae(d, hw, steps=3, batch=2):
    from oracle import nets, weights as W

    def make_step():
        sd = W.make_state_dict(W.cae_spec(CAE_CHANNELS), 1234)
        names = nets.trainable(sd)
        for k in names:
            sd[k].requires_grad_(True)
        labels, clinical = W.cae_inputs(batch, d, hw, 1234)
        ttt = nets.time_to_treatment(clinical)
        core, penu, lesion = labels[:, 0:1], labels[:, 1:2], labels[:, 2:3]
        m = [torch.zeros_like(sd[k]) for k in names]
        v = [torch.zeros_like(sd[k]) for k in names]

        def step(i):
            lat, rec = nets.cae_forward(sd, core, penu, lesion, ttt, alpha=1.0, training=True)
            loss = nets.cae_loss(lat, rec, core, penu, lesion, 30)
            grads = torch.autograd.grad(loss, [sd[k] for k in names])
            with torch.no_grad():
                nets.adam_step([sd[k] for k in names], grads, m, v, i + 1, lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-5)
        return step
    return _cpu_report(batch * d * hw * hw, make_step,
                       "CPU oracle (fp32), CAE train step (3 enc + 4 dec passes), batch %d x 1x%dx%dx%d" % (batch, d, hw, hw), steps)


def torch_gpu_baseline(size, batch, steps=3, bf16=True):
    """Optional extra leg (--torch-gpu-baseline): the same torch restatement run by stock PyTorch-ROCm (MIOpen
    convolutions, bf16 autocast, eager autograd, torch-style Adam) on this GPU.  A reference point for what the
    reference code base itself would reach on an MI355X; never the thing shipped or the headline value."""
    from oracle import nets, weights as W
    dev = "cuda:0"
    sd = {k: v.to(dev) for k, v in W.make_state_dict(W.unet_spec(CHANNELS), 1234).items()}
    names = nets.trainable(sd)
    for k in names:
        sd[k].requires_grad_(True)
    x, y = W.unet_inputs(batch, size, 1234)
    x, y = x.to(dev), y.to(dev)
    opt = torch.optim.Adam([sd[k] for k in names], lr=1e-3, weight_decay=1e-5, betas=(0.99, 0.999))
    times = []
    for step in range(steps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
            seg = nets.unet_forward(sd, x, training=True)
        loss = nets.unet_loss(seg.float(), y)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    t = sorted(times[2:])[len(times[2:]) // 2]
    vox = batch * size[0] * size[1] * size[2]
    return {"value": vox / t, "unit": "voxels/s", "ms_per_step": 1e3 * t, "kind": "torch restatement on the same GPU (MIOpen, %s, eager)"
            % ("bf16 autocast" if bf16 else "fp32"), "batch": batch}


# ------------------------------------------------------------------------------------------------ launcher
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def self_launch(args):
    """No WORLD_SIZE and --gpus N > 1: start N ranks of this script with torch.distributed.run.  This process has not
    touched the GPU (and never will): it only relays the children's output and exit status."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // max(1, args.gpus))))
    proc = subprocess.run(cmd, env=env)
    return proc.returncode


def dryrun(args, world, rank):
    """SP_BENCH_DRYRUN (tests/test_parallel_gloo.py): ranks rendezvous, all-reduce one value, rank 0 prints a skeleton
    line.  No GPU, no workload: exercises the launcher and the env plumbing only; never a measurement."""
    import torch.distributed as dist
    seen = torch.ones(1)
    if world > 1:
        dist.init_process_group(os.environ.get("SP_BENCH_BACKEND", "gloo"))
        dist.all_reduce(seen)
        dist.barrier()
    if rank == 0:
        emit_line({"metric": "train-step voxels/sec, 3D U-Net Bx2x128^3", "value": 0.0, "unit": "voxels/s", "n_gpus": world,
                   "steps": args.steps, "warmup": args.warmup, "dryrun": True, "ranks_seen": int(seen.item())})
    if world > 1:
        dist.destroy_process_group()
    return 0


# ------------------------------------------------------------------------------------------------ timing harness
class _LoaderStub:
    """Learner only asks a loader for its batch size before training starts (Learner.py:40)"""

    def __init__(self, batch_size):
        self.batch_size = batch_size


def timed_steps(step, args, world, dev):
    """W untimed steps, then EXACTLY K steps bracketed by barrier + synchronize on both sides; MAX over ranks."""
    import torch.distributed as dist

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    fence()
    dt = time.perf_counter() - t0
    if world > 1:
        tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax)
    return dt, out


DUMP_BYTES = 60 * 1000 * 1000     # --dump-outputs writes at most this much (a larger set: a seeded sample of every array)


def keep_last_dto(learner):
    """--dump-outputs: remember the DTO of the learner's latest forward (in graph mode the captured one, whose tensors every
    replay rewrites).  Installed only when dumping, so a plain run's step is untouched."""
    seen = {}
    inner = learner.inference_step

    def inference_step(batch):
        seen["dto"] = inner(batch)
        return seen["dto"]
    learner.inference_step = inference_step
    return seen


def dto_tensors(dto, prefix):
    """{"<prefix>_<field>[_<field>...]": tensor} of every tensor leaf under a DTO"""
    from stroke_prediction_amd.common.dto.Dto import Dto
    out = {}
    for key, value in dto:
        name = "%s_%s" % (prefix, key)
        if isinstance(value, Dto):
            out.update(dto_tensors(value, name))
        elif torch.is_tensor(value):
            out[name] = value
    return out


def model_state(model):
    """every floating-point entry of the state dict (parameters and BatchNorm buffers), flattened in key order"""
    return torch.cat([v.detach().reshape(-1).float() for v in model.state_dict().values() if v.is_floating_point()])


def dump_outputs(path, arrays):
    """``path/<name>.npy`` for every array: float64 stays float64, everything else becomes float32.  When the whole set is
    larger than DUMP_BYTES, every array is cut to the same fraction of its elements (at least one): flat indices drawn by a
    generator seeded from the array's name, so that two runs with the same arguments sample the same elements."""
    import numpy as np
    import zlib
    os.makedirs(path, exist_ok=True)
    arrays = {k: v.detach() for k, v in arrays.items()}
    total = sum(8 * v.numel() if v.dtype == torch.float64 else 4 * v.numel() for v in arrays.values())
    for name, v in arrays.items():
        v = v.cpu().to(torch.float64 if v.dtype == torch.float64 else torch.float32)
        if total > DUMP_BYTES:
            keep = max(1, v.numel() * DUMP_BYTES // total)
            if keep < v.numel():
                g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
                v = v.reshape(-1)[torch.randint(v.numel(), (keep,), generator=g).sort().values]
        np.save(os.path.join(path, name + ".npy"), v.numpy())
    print("bench.py: %d arrays written to %s" % (len(arrays), path), file=sys.stderr)


def kernel_profile(eager_step, nsteps, world):
    """Per-launch HIP-event timing of the conv / weight-gradient kernels (ops._Timed) over `nsteps` EAGER steps on the
    launch stream: per-kernel events cannot live inside a replayed graph.  Returns {tag: [seconds, flops, launches]} and
    the per-layer table."""
    import torch.distributed as dist
    from stroke_prediction_amd.runtime import ops as O
    O.PROFILE = []
    for _ in range(nsteps):
        eager_step()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    prof, O.PROFILE = O.PROFILE, None
    if os.environ.get("SP_LAYER_ORDER"):      # tools/layer_table.py: (tag, detail, flops) of ONE step's launches, in order
        n1 = len(prof) // nsteps
        with open(os.environ["SP_LAYER_ORDER"], "w") as f:
            json.dump([[tag, detail, flops] for tag, flops, _, _, detail in prof[:n1]], f)
    agg, per_layer = {}, {}
    for tag, flops, e0, e1, detail in prof:
        ms = e0.elapsed_time(e1)
        for d, k in ((agg, tag), (per_layer, (tag, detail))):
            a = d.setdefault(k, [0.0, 0.0, 0])
            a[0] += ms * 1e-3
            a[1] += flops
            a[2] += 1
    return agg, per_layer


def roofline_from(agg, per_layer, nsteps, ms_per_step, dtype, layers_to=None, traffic_key=None):
    if not agg:
        return None, None
    if layers_to is not None:
        for (tag, detail), (tt, ff, nn) in sorted(per_layer.items(), key=lambda kv: -kv[1][0]):
            print("  %-11s %-40s %7.1f us/launch  %6.1f TFLOP/s  x%d/step" % (tag, detail, 1e6 * tt / nn, ff / tt / 1e12, nn // nsteps),
                  file=layers_to)
    dom = max(agg, key=lambda k: agg[k][0])
    t, fl, n = agg[dom]
    peak = PEAK_TFLOPS[dtype]
    traffic, traffic_source = None, None
    if traffic_key:     # HBM bytes per launch from the committed rocprofv3 --pmc passes of THIS workload (FETCH_SIZE x2 + WRITE_SIZE,
        try:            # profiles/*_pmc_traffic.md; regenerated by tools/profile_round.sh) -- null for workloads without such a pass
            tj = os.path.join(ROOT, "profiles", "traffic.json")
            with open(tj) as f:
                d = json.load(f)
            traffic = d[traffic_key]["bytes_per_launch"]
            traffic_source = {"file": "profiles/traffic.json", "mtime": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime(os.path.getmtime(tj))),
                              "passes": d.get("_source" + ("_cae" if traffic_key.startswith("cae_") else ""), "")[:160]}
        except Exception:
            pass
    roof = {"bound": "mfma", "kernel": dom, "achieved": fl / t / 1e12, "peak": peak, "unit": "TFLOP/s",
            "frac": fl / t / 1e12 / peak, "traffic": traffic, "traffic_source": traffic_source, "launches": n, "avg_launch_us": 1e6 * t / n,
            "share_of_step": (t / nsteps) / (ms_per_step * 1e-3),
            "flops": "algorithmic: 2 x taps x Cin x Cout per output voxel of the convolution (data gradients: the forward's output voxels)",
            "timing": "HIP events on the launch stream around every launch, %d eager steps" % nsteps}
    if traffic:
        gbps = traffic / (t / n) / 1e9
        roof["hbm"] = {"achieved": gbps, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbps / HBM_PEAK_GBS}
    kernels = {k: {"time_s_per_step": v[0] / nsteps, "tflops": v[1] / v[0] / 1e12, "launches_per_step": v[2] / nsteps}
               for k, v in agg.items()}
    return roof, kernels


def conv_roofline_unet(size, channels, batch, peak_tflops, kernels):
    """the tighter per-layer bound  sum over the 3x3x3 layers and the three passes (forward, data gradient --
    none for the first layer --, weight gradient) of  max(FLOP / MFMA peak, ideal bytes / HBM peak)  with every operand read
    once and every result written once in bf16 (the weight-gradient output is negligible), against the measured time of the
    same kernels (conv_igemm + conv_wgrad families).  3-scale topology of Unet3D.py:31-79."""
    c = channels
    d = size
    layers = []
    skips = []
    for blk in range(3):                                   # block1..3 (valid convolutions, pool between)
        cin, cout = c[blk], c[blk + 1]
        layers += [(cin, cout, d), (cout, cout, d - 2)]
        d -= 4
        if blk < 2:
            skips.append((cout, d))
            d //= 2
    for up, (cs, _) in zip((4, 5), reversed(skips)):       # block4, block5: upsample x2, concat with the cropped skip
        d *= 2
        cin, cout = c[up - 1] + cs, c[up]
        layers += [(cin, cout, d), (cout, cout, d - 2)]
        d -= 4
    ideal = 0.0
    for i, (cin, cout, din) in enumerate(layers):
        vin, vout = batch * din ** 3, batch * (din - 2) ** 3
        t = max(2.0 * 27 * cin * cout * vout / (peak_tflops * 1e12), (vin * cin + vout * cout) * 2 / (HBM_PEAK_GBS * 1e9))
        ideal += t * (2 if i == 0 else 3)
    measured = sum(kernels[k]["time_s_per_step"] for k in ("conv_igemm", "conv_wgrad") if k in kernels)
    return {"ideal_ms": 1e3 * ideal, "measured_ms": 1e3 * measured, "frac": ideal / measured if measured else None,
            "definition": "sum over the ten 3x3x3 layers x (fwd, dgrad, wgrad) of max(FLOP / %.0f TFLOP/s, bf16 operand bytes / %.0f GB/s)"
                          % (peak_tflops, HBM_PEAK_GBS)}


def step_roofline_unet(size, channels, batch, peak_tflops, ms_per_step):
    """The WHOLE training step against its module-level roofline (VERDICT r4 "next" 5): sum over every module of the step of
    max(FLOP / MFMA peak, algorithmic bytes / HBM peak), every module reading each input once and writing each output once --
    the ten 3x3x3 layers x (forward, data gradient, weight gradient) as in conv_roofline, plus the passes the reference runs as
    modules of their own (Unet3D.py:56-79, metrics.py:16-28): input statistics, 2 max-pools, 2 upsample + crop + concat, the
    pointwise head, the Dice sums, and in the backward the head, one (read g, read y, write dz) pass per convolution output
    (BatchNorm + LeakyReLU backward, carrying the pool / upsample / skip transposes) and Adam.  A fused implementation may beat
    single terms (the pooling pass is gone since round 5); the sum is the yardstick, not a bound on what fusion can reach.
    bytes_measured: rocprofv3 FETCH_SIZE x2 + WRITE_SIZE over every kernel of a step (profiles/traffic.json "step")."""
    c, d, B = channels, size, batch
    E = 2.0                                                   # bf16 bytes per activation element
    items = []                                                # (name, flop, bytes)
    conv_layers, skips = [], []
    for blk in range(3):
        cin, cout = c[blk], c[blk + 1]
        conv_layers += [(cin, cout, d), (cout, cout, d - 2)]
        d -= 4
        if blk < 2:
            skips.append((cout, d))
            items.append(("maxpool", 0.0, B * cout * (d ** 3 + (d // 2) ** 3) * E))
            d //= 2
    for up, (cs, ds) in zip((4, 5), reversed(skips)):
        lowc = c[up - 1]
        items.append(("upsample+crop+cat", 0.0, B * (lowc * d ** 3 + cs * (2 * d) ** 3 + (lowc + cs) * (2 * d) ** 3) * E))
        d *= 2
        conv_layers += [(lowc + cs, c[up], d), (c[up], c[up], d - 2)]
        d -= 4
    nout = B * d ** 3
    items.append(("input statistics", 0.0, B * c[0] * size ** 3 * 4.0))
    for i, (cin, cout, din) in enumerate(conv_layers):
        vin, vout = B * din ** 3, B * (din - 2) ** 3
        fl = 2.0 * 27 * cin * cout * vout
        by = vin * cin * (4.0 if i == 0 else E) + vout * cout * E
        for p in (("fwd", "wgrad") if i == 0 else ("fwd", "dgrad", "wgrad")):
            items.append(("conv %d->%d @%d %s" % (cin, cout, din, p), fl, by))
        if i + 1 < len(conv_layers) or True:
            items.append(("dz of conv %d->%d @%d" % (cin, cout, din), 0.0, 3 * vout * cout * E))      # read g, read y, write dz
    items.pop()                                               # (the last convolution's dz is the head's backward below)
    items.append(("head fwd", 2.0 * nout * (c[5] * c[6] + c[6] * c[7]), nout * (c[5] * E + c[7] * 4.0)))
    items.append(("dice sums + backward", 0.0, nout * c[7] * 4.0 * 4))
    items.append(("head bwd", 6.0 * nout * (c[5] * c[6] + c[6] * c[7]), nout * (2 * c[5] * E + 2 * c[7] * 4.0)))
    nparam = sum(27 * a * b + b + 2 * a for a, b, _ in conv_layers) + c[5] * c[6] + c[6] + c[6] * c[7] + c[7]
    items.append(("adam", 0.0, 28.0 * nparam))
    ideal = sum(max(fl / (peak_tflops * 1e12), by / (HBM_PEAK_GBS * 1e9)) for _, fl, by in items)
    out = {"ideal_ms": 1e3 * ideal, "measured_ms": ms_per_step, "frac": 1e3 * ideal / ms_per_step,
           "flops_algorithmic": sum(fl for _, fl, _ in items), "bytes_algorithmic": sum(by for _, _, by in items), "bytes_measured": None}
    try:
        with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
            out["bytes_measured"] = json.load(f)["step"]["bytes_per_step"]
    except Exception:
        pass
    return out


def conv_roofline_cae(d, hw, batch, peak_tflops, kernels, channels=None):
    """The per-layer bound of SURVEY 8(d) for the CAE (VERDICT r3 missing 4): sum over the 10 encoder layers x 3 passes and the
    12 decoder layers x 4 passes (Cae3D.py:39-76,105-107,176-220,230-233) and over forward, data gradient (none for the encoder's
    first layer) and weight gradient of  max(FLOP / MFMA peak, bf16 operand bytes / HBM peak)  -- most of this network is 1 / 16 /
    24-channel layers at full resolution, i.e. HBM-bound by construction -- against the measured time of the conv_igemm +
    conv_wgrad kernel families."""
    from stroke_prediction_amd.runtime.cae_engine import ENC_LAYERS, DEC_LAYERS, channel_map
    from stroke_prediction_amd.runtime import plan as P
    cm = channel_map(channels or CAE_CHANNELS)
    ideal, flop_total, bytes_total = 0.0, 0.0, 0.0
    for table, dims, passes in ((ENC_LAYERS, (d, hw, hw), 3), (DEC_LAYERS, None, 4)):
        if dims is None:
            dims = enc_out
        for i, (kind, ci, co, k, s_, p_) in enumerate(table):
            cin, cout = cm[ci], cm[co]
            mk = P.conv_fwd_op if kind == "conv" else P.convT_fwd_op
            op = mk(cin, cout, k, s_, p_, dims, -(-cin // 8) * 8, -(-cout // 8) * 8, 0)
            vin, vout = batch * dims[0] * dims[1] * dims[2], batch * op.y_dims[0] * op.y_dims[1] * op.y_dims[2]
            flop = 2.0 * batch * op.algo_macs * cin * cout
            byt = (vin * cin + vout * cout) * 2.0
            t = max(flop / (peak_tflops * 1e12), byt / (HBM_PEAK_GBS * 1e9))
            n = 2 if (table is ENC_LAYERS and i == 0) else 3
            ideal += passes * n * t
            flop_total += passes * n * flop
            bytes_total += passes * n * byt
            dims = tuple(op.y_dims)
        enc_out = dims
    measured = sum(kernels[k]["time_s_per_step"] for k in ("conv_igemm", "conv_wgrad") if k in kernels)
    return {"ideal_ms": 1e3 * ideal, "measured_ms": 1e3 * measured, "frac": ideal / measured if measured else None,
            "algorithmic_gflop": flop_total / 1e9, "ideal_bf16_operand_mb": bytes_total / 1e6,
            "definition": "sum over 10 encoder layers x 3 passes + 12 decoder layers x 4 passes x (fwd, dgrad, wgrad) of "
                          "max(FLOP / %.0f TFLOP/s, bf16 operand bytes / %.0f GB/s)" % (peak_tflops, HBM_PEAK_GBS)}


def rccl_proof(sync, world, dev):
    """{ranks, backend, direct, two_shot} for the bench line of an N-rank run: `ranks` is the result of all-reducing a one over the
    process group (and over the DirectComm communicator when the gradient exchange runs on it) -- N only if N ranks took part."""
    import torch.distributed as dist
    out = {"ranks": None, "backend": None, "direct": None, "two_shot": None}
    if not dist.is_initialized():
        return out
    one = torch.ones(1, device=dev)
    dist.all_reduce(one)
    out["ranks"], out["backend"] = int(one.item()), dist.get_backend()
    d = getattr(sync, "direct", None)
    out["direct"] = d is not None
    if d is not None:
        t = torch.ones(1, device=dev)
        d.all_reduce_async(t)
        d.wait()
        torch.cuda.synchronize()
        out["ranks_direct"] = int(t.item())
        out["two_shot"] = bool(getattr(d, "two_shot", False))
    return out


def init_dist(world, dev):
    import torch.distributed as dist
    if world > 1 or os.environ.get("SP_FORCE_SYNC"):      # SP_FORCE_SYNC: 1-rank RCCL group, rehearses capture on one GPU
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        if os.environ.get("SP_BENCH_BACKEND"):
            dist.init_process_group(os.environ["SP_BENCH_BACKEND"])
        else:
            dist.init_process_group("nccl", device_id=dev)


_STDOUT_FD = None


def emit_line(res):
    """the ONE JSON line, on the real stdout (main() parks file descriptor 1 on stderr for everything else)"""
    sys.stdout.flush()
    if _STDOUT_FD is not None:
        os.dup2(_STDOUT_FD, 1)
    print(json.dumps(res))
    sys.stdout.flush()
    if _STDOUT_FD is not None:
        os.dup2(2, 1)                           # communicator teardown may print as well


def finish(res, rank):
    import torch.distributed as dist
    if rank == 0:
        emit_line(res)
    if dist.is_initialized():
        dist.destroy_process_group()
    return 0


def use_graph_for(args, world):
    # N = 1: the step is replayed as one hipGraph (Learner(graph=True)).  N > 1, fast mode: forward + loss + backward are one
    # graph, the gradient all-reduce and the fused Adam launch follow eagerly (no collective inside a capture -- the one thing
    # that cannot be rehearsed with several ranks on a 1-GPU box; SP_DIST_GRAPH=1 captures it too).  Exact mode (collectives
    # inside forward and backward): eager.  SP_DIST_EAGER=1: eager launches for N > 1 as in round 1.
    if args.no_graph:
        return False
    return world == 1 or (args.dp_mode == "fast" and not os.environ.get("SP_DIST_EAGER"))


# ------------------------------------------------------------------------------------------------ workloads
def bench_unet(args, world, rank, dev, four_scale=False):
    import torch.distributed as dist
    from stroke_prediction_amd.common.model.Unet3D import Unet3D
    from stroke_prediction_amd.common.metrics import BatchDiceLoss
    from stroke_prediction_amd.learner.UnetSegmentationLearner import UnetSegmentationLearner
    from stroke_prediction_amd.optim import FusedAdam, attach_flat_grads
    from stroke_prediction_amd.parallel import DataParallelSync
    size = (args.size,) * 3
    torch.manual_seed(1234)                      # identical random-init weights on every rank
    if four_scale:
        from stroke_prediction_amd.common.model.Unet3D import LargeUnet3D
        model = LargeUnet3D(CHANNELS4, dtype=args.dtype).to(dev).train()
        channels = CHANNELS4
    else:
        model = Unet3D(CHANNELS, dtype=args.dtype).to(dev).train()
        channels = CHANNELS
    out = model.output_size(size)
    sync = DataParallelSync(model, mode=args.dp_mode, bucketed=not args.no_buckets)
    use_graph = use_graph_for(args, world)
    opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-5,
                    betas=(0.99, 0.999), grad_scale=sync.grad_scale, capturable=True)   # train_unet_segmentation.py:13-14,32
    attach_flat_grads(model)
    with contextlib.redirect_stdout(sys.stderr):      # stdout carries the JSON line only
        learner = UnetSegmentationLearner(_LoaderStub(args.batch), None, model, opt, None, 1, BatchDiceLoss([1.0]),
                                          None, "/tmp/_bench_unet", graph=use_graph, batch_metrics=False, sync_loss=False)
    g = torch.Generator(device=dev).manual_seed(1234 + rank)
    images = torch.randn((args.batch, 2) + size, generator=g, device=dev)
    labels = (torch.rand((args.batch, 2) + tuple(out), generator=g, device=dev) > 0.7).float()
    batch = {"case_id": list(range(args.batch)), "images": images, "labels": labels, "clinical": None}
    # the synthetic batch lives in the captured step's own input buffers (what a loader that writes into Learner.static_batch()'s
    # tensors does): no device-to-device copy of resident inputs inside the step
    if not os.environ.get("SP_BENCH_COPY_INPUTS"):      # (A/B knob: the per-step copy of the batch into the step's buffers)
        batch = learner.static_batch(batch, 0)

    def step():
        return learner.train_batch(batch, 0)

    seen = keep_last_dto(learner) if args.dump_outputs else None
    for _ in range(learner.GRAPH_WARMUP + 1 if use_graph else 0):      # eager warm-ups + capture happen before the timed region
        step()
    dt, last = timed_steps(step, args, world, dev)
    ms = 1e3 * dt / args.steps
    if args.dump_outputs and rank == 0:      # the last timed step's loss, segmentation and the model it left behind
        dump_outputs(args.dump_outputs, dict(dto_tensors(seen["dto"].outputs, "outputs"), loss=last.loss, state=model_state(model)))
    # what a loader pays that does NOT write into the step's own buffers: the device-to-device copy of one batch (outside the timed
    # region; reported next to the line so that the resident-input number can be read either way)
    copy_us = None
    if args.full and use_graph and not os.environ.get("SP_BENCH_COPY_INPUTS") and batch["images"].data_ptr() != images.data_ptr():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            batch["images"].copy_(images)
            batch["labels"].copy_(labels)
        e1.record()
        torch.cuda.synchronize()
        copy_us = e0.elapsed_time(e1) * 1e3 / 20
    vox = world * args.batch * size[0] * size[1] * size[2] * args.steps
    rccl = rccl_proof(sync, world, dev)
    launch_mode = ("hipGraph (Learner(graph=True))" if world == 1 or os.environ.get("SP_DIST_GRAPH") else
                   "hipGraph of forward + loss + backward, then all-reduce and Adam (Learner(graph=True))") if use_graph else "eager"
    name = ("4-scale U-Net %s" % " ".join(map(str, CHANNELS4))) if four_scale else "U-Net 2 16 32 64 32 16 32 2"
    res = {
        "metric": "train-step voxels/sec, 3D U-Net Bx2x%d^3" % args.size, "value": vox / dt, "unit": "voxels/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
        "config": {"workload": "%s: %s, B=%d/GPU, 2x%d^3 -> 2x%d^3, train_batch = fwd+Dice+bwd+Adam"
                               % ("configs[4] net" if four_scale else "configs[1]", name, args.batch, args.size, out[0]),
                   "global_batch": world * args.batch, "parallelism": "dp%d" % world, "loss": float(last.loss),
                   "launch": launch_mode, "input": "resident in the step's input buffers (Learner.static_batch)" if (use_graph and not os.environ.get("SP_BENCH_COPY_INPUTS")) else "resident device tensors",
                   "input_copy_us": copy_us,      # device-to-device copy of one batch into those buffers, NOT in ms_per_step
                   "dp_mode": args.dp_mode if world > 1 else None,
                   # VERDICT r4 "next" 8: which fp8 recipe is which (cosines of the weight gradients against the f32 mode)
                   "precision_note": {"fp8b": "configs[4] TRAINING mode: bf16 forward, fp8 data/weight gradients; gradient cosines of the bf16 mode (0.89 whole-gradient vs f32)",
                                      "fp8": "THROUGHPUT mode: e4m3 forward flips LeakyReLU branches (whole-gradient cosine 0.39 vs f32 at random init on random targets); trains like f32/bf16/fp8b on a learnable target (profiles/r05_f8_train_curve.txt); fp8b keeps the bf16 gradient directions"
                                      }.get(args.dtype),
                   # proof that the collectives saw N ranks: the sum of an all-reduce of ones over the group the gradients travel on
                   "rccl_ranks": rccl["ranks"], "rccl_backend": rccl["backend"], "rccl_direct": rccl["direct"], "rccl_two_shot": rccl["two_shot"],
                   "grad_exchange": (("one all-reduce of the flat gradient buffer between the backward graph and Adam"
                                      if (use_graph and not os.environ.get("SP_DIST_GRAPH")) else
                                      "%d buckets, reverse layer order, async on the RCCL stream" % sync.nbuckets_last)
                                     if not args.no_buckets else "one blocking all-reduce") if world > 1 else None},
    }
    if not args.no_kernel_timing:
        nprof = min(args.steps, 3)
        agg, per_layer = kernel_profile(lambda: learner._optimise(batch, 0), nprof, world)
        tkey = "conv_igemm" if (not four_scale and args.dtype == "bf16" and args.size == 128 and args.batch == 4) else None
        roof, kernels = roofline_from(agg, per_layer, nprof, ms, args.dtype, sys.stderr if args.layers else None, traffic_key=tkey)
        if roof:
            res["roofline"], res["kernels"] = roof, kernels
            if not four_scale and args.dtype in ("bf16", "f16", "bf16x3", "f16x3"):
                cr = roof["conv_roofline"] = conv_roofline_unet(args.size, channels, args.batch, PEAK_TFLOPS[args.dtype], kernels)
                # flat copies: the driver's record keeps the scalar entries of `roofline` only
                roof.update({"conv_ideal_ms": cr["ideal_ms"], "conv_measured_ms": cr["measured_ms"], "conv_frac": cr["frac"]})
                if args.dtype in ("bf16", "f16"):
                    sr = roof["step"] = step_roofline_unet(args.size, channels, args.batch, PEAK_TFLOPS[args.dtype], ms)
                    roof.update({"step_ideal_ms": sr["ideal_ms"], "step_measured_ms": sr["measured_ms"], "step_frac": sr["frac"],
                                 "step_bytes_algorithmic": sr["bytes_algorithmic"], "step_bytes_measured": sr["bytes_measured"],
                                 "step_flops_algorithmic": sr["flops_algorithmic"]})
        if args.size == 128 and not four_scale:
            res["train_step_tflops"] = TRAIN_GFLOP_PER_SAMPLE_128 * 1e9 * world * args.batch * args.steps / dt / 1e12
    if rank == 0 and world == 1 and not args.no_parity and not four_scale and args.dtype in ("bf16", "f16"):
        res["parity"] = parity_vs_f32(model, images)
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        # bounded CPU sample (about 10-30 s): the headline size for the 3-scale net; for the 4-scale net one 2x128^3 volume
        # (a 256^3 oracle step is minutes) -- same network, same per-voxel work up to the valid-convolution border share
        res["cpu_baseline"] = cpu_baseline_unet(size, channels=channels, steps=getattr(args, "cpu_steps", 3)) if not four_scale else \
            cpu_baseline_unet((128, 128, 128), steps=1, batch=1, channels=channels)
    if rank == 0 and world == 1 and args.torch_gpu_baseline and not four_scale:
        try:
            res["torch_gpu_baseline"] = torch_gpu_baseline(size, args.batch, bf16=(args.dtype == "bf16"))
        except Exception as e:
            res["torch_gpu_baseline"] = {"error": str(e).splitlines()[0][:200]}
    return res


def parity_vs_f32(model, images):
    """What the fast modes cost in accuracy at the headline size: the SAME weights and inputs through the bf16 path, the f16
    path (IEEE-half storage), the bf16x3 path (forward on bf16 pairs, three MFMAs per product) and the f32 path (fp32 storage,
    split-bf16 x3: the mode the tests hold to the 1e-3 logit tolerance against the CPU oracle, tests/test_gpu_unet.py).
    Four cases per mode: the weights the timed steps left behind ("trained": ~30 Adam steps from the seeded initialisation) and
    freshly initialised ones, each in eval mode (running BatchNorm statistics, batch 1) and in train mode (batch statistics,
    batch 2).  logits = logit(probability)."""
    import copy
    from stroke_prediction_amd.common.model.Unet3D import Unet3D
    import stroke_prediction_amd.common.dto.UnetDto as UnetDtoUtil
    try:
        with torch.no_grad():
            torch.manual_seed(1234)
            fresh = Unet3D(model.channels, dtype="bf16").to(images.device).state_dict()
            weights = {"trained": copy.deepcopy(model.state_dict()), "random_init": fresh}
            out = {}
            for wname, sd in weights.items():
                for phase in ("eval", "train"):
                    x = (images[:1] if phase == "eval" else images[:2]).contiguous()
                    probs = {}
                    for mode in ("f32", "bf16", "f16", "bf16x3", "f16x3"):
                        m = Unet3D(model.channels, dtype=mode).to(images.device)
                        m.load_state_dict(copy.deepcopy(sd))
                        m.train(phase == "train")
                        dto = m(UnetDtoUtil.init_dto(x, None, None))
                        probs[mode] = torch.cat((dto.outputs.core, dto.outputs.penu), 1).double().clamp(1e-7, 1 - 1e-7)
                        del m
                    l32 = torch.log(probs["f32"] / (1 - probs["f32"]))
                    case = {"max_abs_logit_f32_mode": float(l32.abs().max())}
                    for mode in ("bf16", "f16", "bf16x3", "f16x3"):
                        lm = torch.log(probs[mode] / (1 - probs[mode]))
                        case[mode] = {"max_abs_prob": float((probs[mode] - probs["f32"]).abs().max()),
                                      "max_rel_logit": float(((lm - l32).abs() / l32.abs().clamp_min(1.0)).max()),
                                      "max_abs_logit_over_max_logit": float((lm - l32).abs().max() / l32.abs().max()),
                                      "rms_logit": float((lm - l32).pow(2).mean().sqrt())}
                    out["%s_%s" % (wname, phase)] = case
            out["note"] = ("distance of each fast mode from the f32 mode (same weights, same input, 128^3): max_rel_logit = max over voxels of "
                           "|dlogit| / max(|logit|, 1); max_abs_logit_over_max_logit = the tests' form of the north-star tolerance (1e-3).  "
                           "bf16 / f16 storage (8 / 11 significand bits per activation) does not reach it; the pair modes (forward on hi + lo 16-bit "
                           "tensors, three MFMAs per product: bf16x3 ~17 bits, f16x3 ~22 bits) do -- secondary.unet_f16x3 / .unet_bf16x3 time them")
            return out
    except Exception as e:      # the parity leg must never take the measurement down
        return {"error": str(e).splitlines()[0][:200]}


def bench_unet_infer(args, world, rank, dev):
    """Tester.infer_batch / Learner.validate_batch -- eval-mode forward (running BatchNorm statistics),
    torch.no_grad, reference call path model(dto) (Tester.py:16-28, Learner.py:132-142)."""
    from stroke_prediction_amd.common.model.Unet3D import Unet3D
    import stroke_prediction_amd.common.dto.UnetDto as UnetDtoUtil
    size = (args.size,) * 3
    torch.manual_seed(1234)
    model = Unet3D(CHANNELS, dtype=args.dtype).to(dev).eval()
    out = model.output_size(size)
    model.freeze(True)
    g = torch.Generator(device=dev).manual_seed(1234 + rank)
    images = torch.randn((args.batch, 2) + size, generator=g, device=dev)
    labels = torch.zeros((args.batch, 2) + tuple(out), device=dev)

    def step():
        with torch.no_grad():
            dto = model(UnetDtoUtil.init_dto(images, labels[:, 0:1], labels[:, 1:2]))
        return dto.outputs

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    graph = None
    if not args.no_graph and world == 1:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = step()
    dt, last = timed_steps((lambda: graph.replay()) if graph is not None else step, args, world, dev)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, dto_tensors(captured if graph is not None else last, "outputs"))
    vox = world * args.batch * size[0] * size[1] * size[2] * args.steps
    res = {"metric": "inference voxels/sec, 3D U-Net Bx2x%d^3 (eval forward)" % args.size, "value": vox / dt, "unit": "voxels/s",
           "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps,
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
           "config": {"workload": "3D U-Net --channels 2 16 32 64 32 16 32 2, batch %d/GPU, 2x%d^3 -> 2x%d^3, eval forward "
                                  "(SURVEY 8 row N1)" % (args.batch, args.size, out[0]),
                      "launch": "hipGraph" if graph is not None else "eager"}}
    return res


def bench_cae(args, world, rank, dev):
    """BASELINE configs[2]: CAE --channelscae 1 16 24 32 100 800 1, batch 4, 1 x D x 128 x 128 (D = 28 native; the
    reference cannot close the loss at D = 128), one Learner.train_batch without the CPU metrics."""
    from stroke_prediction_amd.common.model.Cae3D import Cae3D, Enc3D, Dec3D
    from stroke_prediction_amd.common.metrics import BatchDiceLoss
    from stroke_prediction_amd.learner.CaeReconstructionLearner import CaeReconstructionLearner
    from stroke_prediction_amd.optim import FusedAdam, attach_flat_grads
    from stroke_prediction_amd.parallel import DataParallelSync
    from stroke_prediction_amd.common import data as D
    ch = CAE_CHANNELS
    d, hw = args.cae_depth, 128
    torch.manual_seed(1234)
    cae = Cae3D(Enc3D(hw, d, ch, 5, 1.0, dtype=args.dtype), Dec3D(hw, d, ch, 5, 1.0, dtype=args.dtype)).to(dev).train()
    use_graph = use_graph_for(args, world)
    opt = FusedAdam([p for p in cae.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-5, betas=(0.9, 0.999),
                    grad_scale=1.0 / world, capturable=True)          # train_shape_reconstruction.py:11-13,40
    sync = DataParallelSync(cae, optimizer=opt, bucketed=not args.no_buckets)
    attach_flat_grads(cae)
    with contextlib.redirect_stdout(sys.stderr):
        learner = CaeReconstructionLearner(_LoaderStub(args.batch), None, cae, opt, None, 1, None, "/tmp/_bench_cae",
                                           BatchDiceLoss([1.0]), verbose=False, graph=use_graph, batch_metrics=False,
                                           sync_loss=False)
    labels, clinical = D.synthetic_shape_batch(args.batch, d, hw, 1234 + rank)
    batch = {"case_id": list(range(args.batch)), "images": None, "labels": labels.to(dev), "clinical": clinical.to(dev)}
    epoch = 30                                                          # latent-loss ramp factor 0.2
    batch = learner.static_batch(batch, epoch)                          # (see the U-Net workload)

    def step():
        return learner.train_batch(batch, epoch)

    seen = keep_last_dto(learner) if args.dump_outputs else None
    for _ in range(learner.GRAPH_WARMUP + 1 if use_graph else 0):
        step()
    dt, last = timed_steps(step, args, world, dev)
    ms = 1e3 * dt / args.steps
    if args.dump_outputs and rank == 0:
        dto = seen["dto"]
        dump_outputs(args.dump_outputs, dict(dto_tensors(dto.latents, "latents"), **dto_tensors(dto.reconstructions, "reconstructions"),
                                             loss=last.loss, state=model_state(cae)))
    vox = world * args.batch * d * hw * hw * args.steps
    res = {"metric": "train-step voxels/sec, CAE Bx1xDx128x128 (3 encoder + 4 decoder passes)", "value": vox / dt,
           "unit": "voxels/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms,
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
           "config": {"workload": "CAE shape reconstruction --channelscae 1 16 24 32 100 800 1, batch %d/GPU, 1x%dx128x128, "
                                  "Learner.train_batch (configs[2]; 128^3 itself does not close the reference's loss, SURVEY 8d)"
                                  % (args.batch, d),
                      "global_batch": world * args.batch, "parallelism": "dp%d" % world, "loss": float(last.loss),
                      "launch": "hipGraph (Learner(graph=True))" if use_graph else "eager"}}
    if not args.no_kernel_timing:
        nprof = min(args.steps, 3)
        agg, per_layer = kernel_profile(lambda: learner._optimise(batch, epoch), nprof, world)
        roof, kernels = roofline_from(agg, per_layer, nprof, ms, args.dtype, sys.stderr if args.layers else None,
                                      traffic_key="cae_conv_igemm" if (d == 28 and args.batch == 4 and args.dtype == "bf16") else None)
        if roof:
            res["roofline"], res["kernels"] = roof, kernels
            if args.dtype == "bf16":
                roof["conv_roofline"] = conv_roofline_cae(d, hw, args.batch, PEAK_TFLOPS[args.dtype], kernels)
        if d in CAE_TRAIN_GFLOP_PER_SAMPLE:
            res["train_step_tflops"] = CAE_TRAIN_GFLOP_PER_SAMPLE[d] * 1e9 * world * args.batch * args.steps / dt / 1e12
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        res["cpu_baseline"] = cpu_baseline_cae(d, hw, steps=min(getattr(args, "cpu_steps", 3), 3 if d <= 28 else 1))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=None, help="per-GPU batch (default 4; unet4: 2 -- BatchNorm training needs more than one sample, as Learner asserts)")
    ap.add_argument("--size", type=int, default=None, help="cubic input size (default 128; unet4: 256)")
    ap.add_argument("--dtype", default="bf16", choices=DTYPES)
    ap.add_argument("--no-secondary", action="store_true", help="--full run of the default workload only: skip the compact results of the other workloads")
    ap.add_argument("--workload", default="unet", choices=["unet", "cae", "unet-infer", "unet4"],
                    help="unet = BASELINE configs[1] (headline); cae = configs[2]: CAE 1 16 24 32 100 800 1, 3 enc + 4 dec passes; "
                         "unet4 = configs[4] topology (4-scale U-Net 2 32 64 128 256 128 64 32 [32] 2, default 256^3); "
                         "unet-infer = SURVEY 8 row N1: eval-mode forward only (Tester / validate_batch), no gradients")
    ap.add_argument("--cae-depth", type=int, default=28, help="CAE volume depth (28 native, 124 = closest closed size to 128)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-kernel-timing", action="store_true")
    ap.add_argument("--no-parity", action="store_true", help="skip the bf16-vs-f32-mode logit comparison leg")
    ap.add_argument("--torch-gpu-baseline", action="store_true",
                    help="also time the torch restatement (MIOpen, bf16 autocast) on this GPU; reported beside cpu_baseline")
    ap.add_argument("--dp-mode", default="fast", choices=["fast", "exact"],
                    help="multi-GPU: fast = local BatchNorm/Dice + gradient mean; exact = global-batch BatchNorm and Dice sums")
    ap.add_argument("--no-buckets", action="store_true", help="multi-GPU: one blocking all-reduce after backward instead of overlapped buckets")
    ap.add_argument("--layers", action="store_true", help="print per-layer conv kernel timings to stderr")
    ap.add_argument("--no-graph", action="store_true", help="launch every kernel from Python instead of replaying a hipGraph")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run what the headline figure does not need: kernel timing and rooflines, the "
                         "precision parity leg, the CPU baseline, the secondary workloads and the input-copy time (each still "
                         "subject to its --no-* option)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (outputs, loss, model state) as DIR/<name>.npy, float32 / float64, "
                         "at most 60 MB in all (a larger set: the same seeded sample fraction of every array)")
    args = ap.parse_args()
    if args.layers and not args.full:
        ap.error("--layers prints the kernel timing of --full")
    if not args.full:      # a plain run: set up, warm up, time the steps, print the line
        args.no_kernel_timing = args.no_parity = args.no_cpu_baseline = args.no_secondary = True
    if args.batch is None:
        args.batch = 2 if args.workload == "unet4" else 4
    if args.size is None:
        args.size = 256 if args.workload == "unet4" else 128

    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:
        return self_launch(args)              # nothing below runs in the launcher process: it never touches the GPU
    world = int(env_world or "1")
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d (launch N ranks with --gpus N, or unset WORLD_SIZE and let "
                         "bench.py start them)" % (args.gpus, world))
    if rank != 0:
        sys.stdout = open(os.devnull, "w")
    # stdout carries the JSON line only: libraries that write to file descriptor 1 themselves (RCCL prints a banner --
    # "ROCm version / Hostname / Librccl path" -- when a communicator is created) go to stderr until finish() prints
    global _STDOUT_FD
    sys.stdout.flush()
    _STDOUT_FD = os.dup(1)
    os.dup2(2, 1)
    if os.environ.get("SP_BENCH_DRYRUN"):
        return dryrun(args, world, rank)
    # SP_BENCH_DEVICE / SP_BENCH_BACKEND: rehearsal of the multi-rank code path on a one-GPU box (all ranks on one
    # device, gloo instead of RCCL, which refuses two ranks per device); never set in a measured run
    if os.environ.get("SP_BENCH_DEVICE") is not None:
        local_rank = int(os.environ["SP_BENCH_DEVICE"])
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    init_dist(world, dev)
    import stroke_prediction_amd  # noqa: F401  (puts the drop-in packages on sys.path)
    res = run_workload(args, world, rank, dev)
    if args.workload == "unet" and world == 1 and rank == 0 and not args.no_secondary and args.dtype == "bf16" and args.size == 128:
        res["secondary"] = secondary_workloads(args, dev)
        tolerance_mode_into_config(res)
    return finish(res, rank)


def tolerance_mode_into_config(res, mode="bf16x3"):
    """The co-headline (VERDICT r4 "next" 4): BASELINE configs[1] names bf16, north_star a 1e-3 logit tolerance that bf16 storage
    cannot meet; `bf16x3` (forward on bf16 pairs) is the fast mode that does.  Its step time, conv roofline and distance from the
    f32 mode go into `config` as flat scalars (the driver's record keeps those), next to the full objects in `secondary`."""
    sec = res.get("secondary", {}).get("unet_" + mode)
    if not sec or "ms_per_step" not in sec:
        return
    c = res["config"]
    c["tolerance_mode"] = mode
    c["tolerance_mode_ms_per_step"] = sec["ms_per_step"]
    c["tolerance_mode_voxels_per_s"] = sec["value"]
    rf = sec.get("roofline") or {}
    c["tolerance_mode_mfma_frac"] = rf.get("frac")
    c["tolerance_mode_conv_frac"] = (rf.get("conv_roofline") or {}).get("frac")
    par = res.get("parity") or {}
    worst = [v[mode]["max_abs_logit_over_max_logit"] for v in par.values() if isinstance(v, dict) and mode in v]
    c["tolerance_mode_max_rel_logit"] = max(worst) if worst else None      # vs the f32 mode, worst of trained / random-init x eval / train
    worst = [v[res["dtype"]]["max_abs_logit_over_max_logit"] for v in par.values() if isinstance(v, dict) and res["dtype"] in v]
    c["headline_mode_max_rel_logit"] = max(worst) if worst else None


def run_workload(args, world, rank, dev):
    if args.workload == "cae":
        return bench_cae(args, world, rank, dev)
    if args.workload == "unet-infer":
        return bench_unet_infer(args, world, rank, dev)
    return bench_unet(args, world, rank, dev, four_scale=(args.workload == "unet4"))


def secondary_workloads(args, dev):
    """The other workloads of BASELINE.json / SURVEY 8 under the same clock as the headline line (``--full`` runs of the
    default command): each with its own model, warm-up and timed region, AFTER the headline's timed region has closed;
    compact results (the full line of each is what `bench.py --workload ... ` prints).  Bounded: 10 timed steps each, one
    timed CPU-oracle step where a CPU leg is given."""
    import copy
    import gc
    out = {}
    t_all = time.perf_counter()
    plan = [("cae_d28", dict(workload="cae", cae_depth=28, dtype="bf16"), True),
            ("cae_d124", dict(workload="cae", cae_depth=124, dtype="bf16"), False),
            ("unet4_bf16", dict(workload="unet4", dtype="bf16", batch=2, size=256), True),
            ("unet4_fp8", dict(workload="unet4", dtype="fp8", batch=2, size=256), True),
            ("unet4_fp8b", dict(workload="unet4", dtype="fp8b", batch=2, size=256), False),
            ("unet_f16x3", dict(workload="unet", dtype="f16x3"), False),
            ("unet_bf16x3", dict(workload="unet", dtype="bf16x3"), False),
            ("unet_f16", dict(workload="unet", dtype="f16"), False),
            ("unet_f32", dict(workload="unet", dtype="f32"), False),
            ("unet_infer", dict(workload="unet-infer", dtype="bf16"), False)]
    for name, over, cpu in plan:
        if over["dtype"] not in DTYPES:
            continue
        a = copy.copy(args)
        a.steps, a.warmup, a.layers, a.no_parity, a.torch_gpu_baseline, a.dump_outputs = 10, 3, False, True, False, None
        a.no_cpu_baseline = not cpu or args.no_cpu_baseline
        a.cpu_steps = 1
        for k, v in over.items():
            setattr(a, k, v)
        t0 = time.perf_counter()
        try:
            r = run_workload(a, 1, 0, dev)
            c = {"metric": r["metric"], "workload": r["config"]["workload"], "dtype": r["dtype"], "ms_per_step": r["ms_per_step"],
                 "value": r["value"], "unit": r["unit"], "steps": r["steps"], "warmup": r["warmup"]}
            if r.get("roofline"):
                c["roofline"] = {k: r["roofline"][k] for k in ("kernel", "achieved", "peak", "unit", "frac", "avg_launch_us")}
                if r["roofline"].get("conv_roofline"):
                    c["roofline"]["conv_roofline"] = {k: r["roofline"]["conv_roofline"][k] for k in ("ideal_ms", "measured_ms", "frac")}
            if r.get("train_step_tflops") is not None:
                c["train_step_tflops"] = r["train_step_tflops"]
            if r.get("parity"):
                c["parity"] = r["parity"]
            if r.get("cpu_baseline"):
                c["cpu_baseline"] = {k: r["cpu_baseline"][k] for k in ("value", "unit", "cores", "kind", "s_per_step", "sample")}
            out[name] = c
        except Exception as e:      # a secondary leg must never take the headline line down
            out[name] = {"error": "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:300] if str(e) else "")}
        out[name]["wall_s"] = time.perf_counter() - t0
        gc.collect()
        torch.cuda.empty_cache()
    out["wall_s"] = time.perf_counter() - t_all
    return out


if __name__ == "__main__":
    sys.exit(main())
