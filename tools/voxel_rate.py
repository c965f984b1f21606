#!/usr/bin/env python3
"""One point per voxel of one step's semi-dense cloud: what sdm_extract_points_voxel costs next to sdm_extract_points, and
next to the host route it replaces (the plain cloud over the link, then the merge in NumPy).

Builds bench.py's workload for each configuration (default: configs[1], 640x480 x 64 keyframes x 20 neighbours, and
1280x720 x 256 x 7; sigma gate 0.1), runs one step and, in one process, for each voxel size (default 0.005 and 0.02) and
each destination kind (torch device tensors, pageable NumPy) takes the median wall time of --reps calls after --warmup
calls (every call ends with a stream synchronise):
  (a) extract_points        fields xyz, rho_sigma
  (b) extract_points_voxel  the same fields, multiplicity and source_index
  (c) the host route: (a) into pageable memory plus tests/voxel_np.py on this machine's CPU (median of --host-reps),
      its result checked equal to (b)'s
  (d) M / T, kept over plain points
Expectation to check, not a gate: (b) into pageable memory takes less wall time than (c).  (b) - (a) is reported.
  (e) the integer atomics of k_voxel_insert (three per mergeable point) over its device time needs a kernel trace:
        rocprofv3 --kernel-trace --stats -d DIR -o voxel --output-format csv -- python tools/voxel_rate.py --out DIR/run.json
        python tools/voxel_rate.py --kernel-stats DIR/.../voxel_kernel_stats.csv --profiled DIR/run.json
      The first writes, beside the timings (inflated by the tracer and not kept), the number of points its calls
      inserted; the second divides by the kernel's total time and adds the figure to --out.
Writes profiles/voxel_mi355x.json and prints it.

  python tools/voxel_rate.py
  python tools/voxel_rate.py --only 480p:64:20
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIGS = ["480p:64:20", "720p:256:7"]
VOXELS = [0.005, 0.02]
FIELDS = ("xyz", "rho_sigma")
OUT = os.path.join(ROOT, "profiles", "voxel_mi355x.json")


def wall_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def run(pkg, torch, bench, res, kfs, nbrs, args, counts):
    import voxel_np
    wl = bench.Workload(pkg, torch, res, kfs, nbrs, 2.6, 1, 0, 0)
    wl.step("allgather", "torch")
    torch.cuda.synchronize()
    eng, slots, ms = wl.eng, list(wl.pl["own_slots"]), args.max_sigma
    cap = max(eng.extract_bound(slots), 1)

    def buffers(kind, vox):
        if kind == "device":
            out = {"xyz": torch.empty((cap, 3), dtype=torch.float32, device="cuda"),
                   "rho_sigma": torch.empty((cap, 2), dtype=torch.float32, device="cuda")}
            if vox:
                out.update(multiplicity=torch.empty(cap, dtype=torch.int32, device="cuda"),
                           source_index=torch.empty(cap, dtype=torch.int32, device="cuda"))
        else:
            out = {"xyz": np.empty((cap, 3), np.float32), "rho_sigma": np.empty((cap, 2), np.float32)}
            if vox:
                out.update(multiplicity=np.empty(cap, np.uint32), source_index=np.empty(cap, np.uint32))
        return out

    plain = {k: np.array(v) for k, v in eng.extract_points(slots, max_sigma=ms, fields=FIELDS).items()}
    T = int(plain["offsets"][-1])
    doc = {"workload": bench.workload_name(wl.W, wl.H, kfs, nbrs, res), "keyframes": len(slots), "max_sigma": ms,
           "plain_points_T": T, "link_bytes_plain": T * 20, "ms_a_extract_points": {}, "voxels": []}
    for kind in ("device", "pageable"):
        out = buffers(kind, False)
        doc["ms_a_extract_points"][kind] = round(wall_ms(lambda: eng.extract_points(slots, max_sigma=ms, out=out),
                                                         args.warmup, args.reps), 4)
    out_a = buffers("pageable", False)
    for voxel in args.voxel or VOXELS:
        row = {"voxel_size": voxel}
        for kind in ("device", "pageable"):
            out = buffers(kind, True)
            row["ms_b_extract_points_voxel_" + kind] = round(
                wall_ms(lambda: eng.extract_points_voxel(slots, voxel, max_sigma=ms, out=out), args.warmup, args.reps), 4)
            row["ms_b_minus_a_" + kind] = round(row["ms_b_extract_points_voxel_" + kind] - doc["ms_a_extract_points"][kind], 4)
            counts["calls"] += args.warmup + args.reps
            counts["points"] += (args.warmup + args.reps) * T
        got = eng.extract_points_voxel(slots, voxel, max_sigma=ms, out=buffers("pageable", True))
        counts["calls"] += 1
        counts["points"] += T
        host = {}

        def route():
            p = eng.extract_points(slots, max_sigma=ms, out=out_a)
            host["r"] = (p, voxel_np.voxel_merge(p["xyz"], p["rho_sigma"][:, 1], voxel, p["offsets"]))

        row["ms_c_host_route"] = round(wall_ms(route, 1, args.host_reps), 2)
        p, (kept, mult, _, offs) = host["r"]
        M = len(kept)
        row["kept_points_M"] = M
        row["d_M_over_T"] = round(M / max(T, 1), 5)
        row["link_bytes_voxel"] = M * 28
        row["b_equals_c"] = bool(int(got["plain_total"]) == T and np.array_equal(got["offsets"], offs) and
                                 np.array_equal(got["source_index"], kept) and np.array_equal(got["multiplicity"], mult) and
                                 np.array_equal(got["xyz"].view(np.uint32), p["xyz"][kept].view(np.uint32)) and
                                 np.array_equal(got["rho_sigma"].view(np.uint32), p["rho_sigma"][kept].view(np.uint32)))
        row["b_pageable_below_c"] = bool(row["ms_b_extract_points_voxel_pageable"] < row["ms_c_host_route"])
        doc["voxels"].append(row)
    wl.close()
    return doc


def add_kernel_stats(args):
    """(e): 3 atomics per inserted point over k_voxel_insert's total device time in the profiled run"""
    prof = json.load(open(args.profiled))
    total_ns = calls = 0
    for r in csv.DictReader(open(args.kernel_stats)):
        if "k_voxel_insert" in r["Name"]:
            total_ns += float(r["TotalDurationNs"])
            calls += int(r["Calls"])
    pts = prof["insert"]["points"]
    doc = json.load(open(args.out))
    doc["e_insert_atomics"] = {
        "calls": calls, "calls_expected": prof["insert"]["calls"], "points_inserted": pts,
        "k_voxel_insert_total_ms": round(total_ns / 1e6, 3),
        "ns_per_point": round(total_ns / max(pts, 1), 4),
        "atomics_per_second": round(3 * pts / max(total_ns, 1) * 1e9, -6),
        "note": "three integer atomics per point (64-bit compare-and-swap, 64-bit min, 32-bit add) over the kernel's total "
                "time in one rocprofv3 --kernel-trace --stats run of this script; the time also covers the kernel's loads",
    }
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["e_insert_atomics"]))
    return 0 if calls == prof["insert"]["calls"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", action="append", help="res:keyframes:neighbours (repeatable; default: %s)" % ", ".join(CONFIGS))
    ap.add_argument("--voxel", action="append", type=float, help="voxel size (repeatable; default: 0.005, 0.02)")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--max-sigma", type=float, default=0.1)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--kernel-stats", help="rocprofv3 kernel stats CSV of a profiled run of this script: add (e) to --out")
    ap.add_argument("--profiled", help="the JSON that profiled run wrote")
    args = ap.parse_args()
    if args.kernel_stats:
        return add_kernel_stats(args)

    import torch
    import bench
    import sdm_pkg
    pkg = sdm_pkg.load()
    runs, counts = [], {"calls": 0, "points": 0}
    for cfg in args.only or CONFIGS:
        res, kfs, nbrs = cfg.split(":")
        runs.append(run(pkg, torch, bench, res, int(kfs), int(nbrs), args, counts))
        print(json.dumps(runs[-1]), flush=True)
    doc = {"metric": "one point per voxel of one step's filtered cloud: wall ms per call (median; every call ends with a "
                     "stream synchronise), fields xyz + rho_sigma; (c) is extract_points into pageable memory plus the "
                     "NumPy merge on the host",
           "reps": args.reps, "warmup": args.warmup, "host_reps": args.host_reps,
           "arch": torch.cuda.get_device_properties(0).gcnArchName, "runs": runs, "insert": counts}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0 if all(v["b_equals_c"] for r in runs for v in r["voxels"]) else 1


if __name__ == "__main__":
    sys.exit(main())
