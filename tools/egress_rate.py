#!/usr/bin/env python3
"""Egress of one step's semi-dense cloud: what it costs a batch caller to get the points that pass the writers' filter
(PM.cc:100-132: !(sigma > 0.01) && rho > 1e-6, rho = checked plane) out of the engine.

Builds bench.py's workload (default configs[1]: 640x480, 64 keyframes x 20 neighbours, seeded synthetic scene), runs one
step and times, end to end and per step:
  (a) today's path: sdm_download_depth + _checked + _pointset per keyframe, then the filter in NumPy
  (b) sdm_extract_points into pageable NumPy arrays
  (c) sdm_extract_points into sdm_host_alloc (pinned) arrays
  (d) sdm_extract_points into torch device tensors
each producing xyz, pixel code and {rho, sigma} of every point (the results of (a)-(d) are checked equal), plus the
device time of the extraction (HIP events around the call with a device destination: its kernels, the offsets' read-back
and the one host round trip).  Prints one JSON line.

  python tools/egress_rate.py                      # configs[1]
  python tools/egress_rate.py --res 720p --kfs 256 --nbrs 7   # configs[2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIELDS = ("xyz", "pixel", "rho_sigma")


def host_path(eng, slots, W, max_sigma):
    xyz, pix, rs = [], [], []
    offs = [0]
    for s in slots:
        rho_d, sigma = eng.download_depth(s)
        rho = eng.download_checked(s)
        pts = eng.download_pointset(s)
        keep = ~(sigma.astype(np.float64) > max_sigma) & (rho.astype(np.float64) > 0.000001)
        flat = np.flatnonzero(keep)
        xyz.append(pts.reshape(-1, 3)[flat])
        pix.append(((flat // W).astype(np.uint32) << 16) | (flat % W).astype(np.uint32))
        rs.append(np.stack([rho.reshape(-1)[flat], sigma.reshape(-1)[flat]], 1))
        offs.append(offs[-1] + len(flat))
    return {"xyz": np.concatenate(xyz), "pixel": np.concatenate(pix), "rho_sigma": np.concatenate(rs),
            "offsets": np.asarray(offs, np.int64)}


def same(a, b):
    for f in FIELDS + ("offsets",):
        x, y = np.asarray(a[f]), np.asarray(b[f])
        if x.shape != y.shape or x.tobytes() != y.tobytes():
            return False
    return True


def timed(fn, reps):
    fn()  # warm: allocations, code objects
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", default="480p", choices=["480p", "720p", "1080p"])
    ap.add_argument("--kfs", type=int, default=64)
    ap.add_argument("--nbrs", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-sigma", type=float, default=0.01,
                    help="the filter's sigma gate (PM.cc:120: 0.01; the synthetic scenes' sigmas lie mostly above it)")
    args = ap.parse_args()

    import torch
    import bench
    import sdm_pkg
    pkg = sdm_pkg.load()
    wl = bench.Workload(pkg, torch, args.res, args.kfs, args.nbrs, 2.6, 1, 0, 0)
    wl.step("allgather", "torch")
    torch.cuda.synchronize()
    eng, slots, W, H = wl.eng, list(wl.pl["own_slots"]), wl.W, wl.H
    n, P = len(slots), wl.W * wl.H
    ms = args.max_sigma

    ms_a, ref = timed(lambda: host_path(eng, slots, W, ms), args.reps)
    total = int(ref["offsets"][-1])
    m = max(total, 1)  # (an empty tensor has no address: the call would see no field)
    shapes = {"xyz": (m, 3), "pixel": (m,), "rho_sigma": (m, 2)}
    dtypes = {"xyz": np.float32, "pixel": np.uint32, "rho_sigma": np.float32}

    page = {f: np.empty(shapes[f], dtypes[f]) for f in FIELDS}
    ms_b, got_b = timed(lambda: eng.extract_points(slots, max_sigma=ms, out=page), args.reps)
    pinned = {f: eng.host_alloc(shapes[f], dtypes[f]) for f in FIELDS}
    ms_c, got_c = timed(lambda: eng.extract_points(slots, max_sigma=ms, out=pinned), args.reps)
    tdt = {"xyz": torch.float32, "pixel": torch.int32, "rho_sigma": torch.float32}
    dev = {f: torch.empty(shapes[f], dtype=tdt[f], device="cuda") for f in FIELDS}
    ms_d, got_d = timed(lambda: eng.extract_points(slots, max_sigma=ms, out=dev), args.reps)
    got_d = {f: (got_d[f].cpu().numpy().view(np.uint32) if f == "pixel" else got_d[f].cpu().numpy()) for f in FIELDS}
    got_d["offsets"] = ref["offsets"]

    # device time: HIP events on the engine's stream (torch's current stream) around the call, device destination
    ev = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.extract_points(slots, max_sigma=ms, out=dev)
        b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    dev_ms = float(np.median([a.elapsed_time(b) for a, b in ev]))
    ok = same(got_b, ref) and same(got_c, ref) and same(got_d, ref)
    for a in pinned.values():
        eng.host_free(a)

    bytes_a = n * P * (8 + 4 + 12)
    bytes_b = total * (12 + 4 + 8) + 8 * (n + 1)
    out = {
        "metric": "egress of one step's filtered semi-dense cloud (xyz, pixel, rho/sigma)",
        "workload": bench.workload_name(W, H, args.kfs, args.nbrs, args.res),
        "keyframes": n,
        "max_sigma": ms,
        "points": total,
        "points_per_keyframe": round(total / n, 1),
        "pass_fraction": float("%.4g" % (total / (n * P))),
        "extract_device_ms": round(dev_ms, 4),
        "ms_a_download3_numpy": round(ms_a, 3),
        "ms_b_extract_pageable": round(ms_b, 3),
        "ms_c_extract_pinned": round(ms_c, 3),
        "ms_d_extract_device": round(ms_d, 3),
        "speedup_b_over_a": round(ms_a / ms_b, 2),
        "bytes_link_a": bytes_a,
        "bytes_link_b": bytes_b,
        "link_GBs_a": round(bytes_a / ms_a / 1e6, 2),
        "identical": ok,
        "reps": args.reps,
        "arch": eng.arch(),
    }
    print(json.dumps(out))
    wl.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
