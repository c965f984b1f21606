#!/usr/bin/env python3
"""Per-point visibility lists of one step's semi-dense cloud: what sdm_extract_points_support costs on top of
sdm_extract_points, next to the inter-keyframe check whose per-neighbour statement it repeats, and next to the host route
it replaces.

Builds bench.py's workload for each configuration (default: configs[1], 640x480 x 64 keyframes x 20 neighbours, and
1280x720 x 256 x 7; sigma gate 0.1, the line egress_rate.py uses), runs one step and, in one process, takes medians of
--reps runs after --warmup runs, device time from HIP events, device destinations:
  (a) extract_points                      xyz, pixel (events around the call, which ends with a stream synchronise)
  (b) extract_points_support              xyz, pixel, support (likewise)
  (c) inter_check on the same references  (commit = 0: rewrites the checked planes with the values they hold; the call
                                          does not wait, so the engine's stage events around its launches are read)
  (d) the host route: download the {rho, sigma} planes of a 4-keyframe sample and of their neighbours and run the NumPy
      restatement (tests/support_np.py); wall time, scaled to all keyframes and labelled as such
The words of (b) and (d) are checked equal on the sample.  Expectation to check, not a gate: the support pass does a
subset of K4's per-pixel work on a subset of its pixels, so (b) - (a) should not exceed (c).
Writes profiles/visibility_mi355x.json and prints it.

  python tools/visibility_rate.py
  python tools/visibility_rate.py --only 480p:64:20
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIGS = ["480p:64:20", "720p:256:7"]
SAMPLE = 4


def device_ms(torch, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ev = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def stage_ms(eng, fn, stage, warmup, reps):
    """a call that does not wait for its kernels: the engine's own HIP events around the stage's launches"""
    for _ in range(warmup):
        fn()
    eng.enable_timing(True)
    ts = []
    for _ in range(reps):
        eng.get_timing(reset=True)
        fn()
        eng.synchronize()
        ts.append(eng.get_timing()[stage][0])
    eng.enable_timing(False)
    return float(np.median(ts))


def host_route(eng, wl, sample, max_sigma):
    """today's route to the lists: the planes over the link, projection and four-tap test on the host"""
    import support_np as sn
    pl = wl.pl
    t0 = time.perf_counter()
    need = sorted(set(k for i in sample for k in [pl["own"][i]] + list(pl["nbrs"][i])))
    maps = {k: eng.download_depth(pl["slot"][k]) for k in need}
    kfs = {k: sn.keyframe(wl.K, wl.scene.Tcw(k), wl.H, wl.W) for k in need}
    words = []
    for i in sample:
        k, row = pl["own"][i], list(pl["nbrs"][i])
        _, w = sn.inter_support(kfs[k], maps[k][0], [kfs[j] for j in row], [maps[j][0] for j in row],
                                  [maps[j][1] for j in row])
        chk = eng.download_checked(pl["slot"][k])  # the plane the filter reads (source 1)
        with np.errstate(invalid="ignore"):
            keep = ~(maps[k][1].astype(np.float64) > max_sigma) & (chk.astype(np.float64) > 0.000001)
        words.append(w[keep])
    return (time.perf_counter() - t0) * 1e3, words


def run(pkg, torch, bench, res, kfs, nbrs, args):
    wl = bench.Workload(pkg, torch, res, kfs, nbrs, 2.6, 1, 0, 0)
    wl.step("allgather", "torch")
    torch.cuda.synchronize()
    eng, pl = wl.eng, wl.pl
    slots, rows = list(pl["own_slots"]), np.asarray(pl["nbr_slots"], np.int32)
    n, ms = len(slots), args.max_sigma
    cap = max(eng.extract_bound(slots), 1)
    dev = {"xyz": torch.empty((cap, 3), dtype=torch.float32, device="cuda"),
           "pixel": torch.empty(cap, dtype=torch.int32, device="cuda")}
    dev_s = dict(dev, support=torch.empty(cap, dtype=torch.int64, device="cuda"))
    ms_a = device_ms(torch, lambda: eng.extract_points(slots, max_sigma=ms, out=dev), args.warmup, args.reps)
    ms_b = device_ms(torch, lambda: eng.extract_points_support(slots, rows, max_sigma=ms, out=dev_s), args.warmup, args.reps)
    ms_c = stage_ms(eng, lambda: eng.inter_check(slots, rows), "inter", args.warmup, args.reps)
    got = eng.extract_points_support(slots, rows, max_sigma=ms, out=dev_s)
    offs = got["offsets"]
    total = int(offs[-1])
    sup = got["support"].cpu().numpy().view(np.uint64)
    sample = [int(i) for i in np.linspace(0, n - 1, min(SAMPLE, n)).astype(int)]
    ms_d, words = host_route(eng, wl, sample, ms)
    ok = all(np.array_equal(sup[offs[i]:offs[i + 1]], w) for i, w in zip(sample, words))
    pc = np.unpackbits(sup.view(np.uint8).reshape(-1, 8), axis=1).sum(1) if total else np.zeros(0, np.int64)
    out = {
        "workload": bench.workload_name(wl.W, wl.H, kfs, nbrs, res),
        "keyframes": n,
        "neighbours": nbrs,
        "max_sigma": ms,
        "points": total,
        "listed_pixels": int(sum(eng.active_count(s) for s in slots)),
        "popcount_min_mean_max": [int(pc.min()), round(float(pc.mean()), 2), int(pc.max())] if total else None,
        "ms_a_extract_points": round(ms_a, 4),
        "ms_b_extract_points_support": round(ms_b, 4),
        "ms_b_minus_a": round(ms_b - ms_a, 4),
        "ms_c_inter_check": round(ms_c, 4),
        "b_minus_a_not_above_c": bool(ms_b - ms_a <= ms_c),
        "ms_d_host_route_sample": round(ms_d, 2),
        "host_route_sample_keyframes": len(sample),
        "ms_d_host_route_scaled_to_all_keyframes": round(ms_d * n / len(sample), 1),
        "b_equals_d_on_sample": bool(ok),
        "link_bytes_host_route_all_keyframes": n * wl.W * wl.H * 8,
        "link_bytes_support": total * 8,
    }
    wl.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", action="append", help="res:keyframes:neighbours (repeatable; default: %s)" % ", ".join(CONFIGS))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-sigma", type=float, default=0.1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "visibility_mi355x.json"))
    args = ap.parse_args()

    import torch
    import bench
    import sdm_pkg
    pkg = sdm_pkg.load()
    runs = []
    for cfg in args.only or CONFIGS:
        res, kfs, nbrs = cfg.split(":")
        runs.append(run(pkg, torch, bench, res, int(kfs), int(nbrs), args))
        print(json.dumps(runs[-1]), flush=True)
    doc = {"metric": "per-point visibility lists of one step's filtered cloud: device ms (HIP events, median), device "
                     "destinations; (d) is host wall time on a sample, scaled",
           "reps": args.reps, "warmup": args.warmup, "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "runs": runs}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0 if all(r["b_equals_d_on_sample"] for r in runs) else 1


if __name__ == "__main__":
    sys.exit(main())
