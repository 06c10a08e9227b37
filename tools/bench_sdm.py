#!/usr/bin/env python3
"""Device vs host time of the signed-distance-map baseline (reference test_sdm_resampling.py) per case, 28 x 128 x 128
synthetic nested blobs (common.data.synthetic_sample), in one process (profiles/sdm_baseline.md):

  * device: ``sdm_interpolate_torch`` (masks for the measures) + the four (2, 2, 1) export zooms, timed with device events
    after warm-up, for resample True / False and T = 1 / 32 (the curve length of CaeReconstructionTesterCurve);
  * host: the scipy.ndimage calls the reference makes for one case -- four distance_transform_edt, center_of_mass (timed
    separately: it only runs for an empty core), the two down-zooms, the three up-zooms (resample), the four export zooms.

    python tools/bench_sdm.py [--reps 20] [--host-reps 2] [--device-only] [--only RESAMPLE,T]

``--device-only`` is the form to run under ``rocprofv3 --kernel-trace --stats`` (launches per call, us per kernel).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def case_volumes(case_id=3):
    from stroke_prediction_amd.common import data
    s = data.synthetic_sample(case_id, xy=128, z=28, n_modalities=0)
    lab = s[data.KEY_LABELS].transpose(3, 2, 1, 0)          # (x, y, z, C) -> (C, z, y, x)
    return np.ascontiguousarray(lab[0]), np.ascontiguousarray(lab[1]), np.ascontiguousarray(lab[2])


def device_case(sdm, core, penu, lesion, t, resample):
    out = sdm.sdm_interpolate_torch(core, penu, t, resample=resample, masks=True)
    recon_core, recon_intp, recon_penu = out[0], out[1], out[2]
    intp = recon_intp if recon_intp.dim() == 3 else recon_intp[0]
    return (sdm.zoom_torch(intp, (1, 2, 2), out="gt0"), sdm.zoom_torch(lesion, (1, 2, 2), out="i8", src_as_int8=True),
            sdm.zoom_torch(recon_core, (1, 2, 2), out="lt0"), sdm.zoom_torch(recon_penu, (1, 2, 2), out="gt0"))


def time_device(core_np, penu_np, lesion_np, reps, T, resample):
    import torch
    from stroke_prediction_amd.common import sdm
    core, penu, lesion = (torch.from_numpy(a).cuda() for a in (core_np, penu_np, lesion_np))
    t = 0.4 if T == 1 else torch.linspace(0, 1, T, dtype=torch.float64)
    for _ in range(3):
        device_case(sdm, core, penu, lesion, t, resample)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        device_case(sdm, core, penu, lesion, t, resample)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times))


def time_host(core, penu, lesion, reps, t=0.4):
    from scipy import ndimage as ndi
    core, penu, lesion = core.astype(np.float64), penu.astype(np.float64), lesion
    parts = {}

    def clock(name, fn):
        t0 = time.perf_counter()
        r = fn()
        parts[name] = parts.get(name, 0.0) + time.perf_counter() - t0
        return r

    for _ in range(reps):
        pb = penu > 0.5
        e0 = clock("edt x4", lambda: ndi.distance_transform_edt(pb))
        e1 = clock("edt x4", lambda: ndi.distance_transform_edt(penu < 0.5))
        cb = core > 0.5
        clock("center_of_mass", lambda: ndi.center_of_mass(pb))
        e2 = clock("edt x4", lambda: ndi.distance_transform_edt(1 - cb))
        e3 = clock("edt x4", lambda: ndi.distance_transform_edt(cb))
        pd, cd = e0 - e1, e2 - e3
        lp = clock("down zoom x2", lambda: ndi.zoom(pd, (1, 1 / 12, 1 / 12)))
        lc = clock("down zoom x2", lambda: ndi.zoom(cd, (1, 1 / 12, 1 / 12)))
        rc = clock("up zoom x3", lambda: ndi.zoom(lc, (1, 12, 12))[:, 2:130, 2:130])
        rp = clock("up zoom x3", lambda: ndi.zoom(lp, (1, 12, 12))[:, 2:130, 2:130])
        ri = clock("up zoom x3", lambda: ndi.zoom(lp * t - lc * (1 - t), (1, 12, 12))[:, 2:130, 2:130])
        for v in (ri, rc, rp):
            clock("export zoom x4", lambda: ndi.zoom(v.transpose((2, 1, 0)), (2, 2, 1)))
        clock("export zoom x4", lambda: ndi.zoom(lesion.astype(np.int8).transpose((2, 1, 0)), (2, 2, 1)))
    parts = {k: v / reps * 1e3 for k, v in parts.items()}
    total = sum(v for k, v in parts.items() if k != "center_of_mass")
    return total, parts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--only", type=str, default=None, help="RESAMPLE,T: time that one device configuration (for the profiler)")
    a = ap.parse_args()
    import torch
    core, penu, lesion = case_volumes()
    res = {"shape": list(core.shape), "device": torch.cuda.get_device_name(0)}
    configs = [(r, T) for r in (True, False) for T in (1, 32)]
    if a.only:
        r, T = (int(v) for v in a.only.split(","))
        configs = [(bool(r), T)]
    for resample, T in configs:
        med, mn = time_device(core, penu, lesion, a.reps, T, resample)
        res["device_ms/resample=%d/T=%d" % (resample, T)] = round(med, 4)
        print("device  resample=%-5s T=%-2d  median %.3f ms  min %.3f ms" % (resample, T, med, mn), flush=True)
    if not a.device_only:
        total, parts = time_host(core, penu, lesion, a.host_reps)
        res["host_ms/resample=1/T=1"] = round(total, 1)
        res["host_parts_ms"] = {k: round(v, 1) for k, v in parts.items()}
        print("host    resample=True  T=1   %.1f ms  (%s)" % (total, ", ".join("%s %.1f" % kv for kv in parts.items())), flush=True)
        res["speedup/resample=1/T=1"] = round(total / res["device_ms/resample=1/T=1"], 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
