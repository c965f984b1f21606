#!/usr/bin/env python3
"""Free-space counts for the merged cloud: what sdm_extract_points_voxel_freespace costs next to
sdm_extract_points_voxel_cameras, and next to the route it replaces (the lists and the kept points over the link, the ray
walk in NumPy on the host).

Builds bench.py's workload for each configuration (default: configs[1], 640x480 x 64 keyframes x 20 neighbours, and
1280x720 x 256 x 7; sigma gate 0.1, source 1), runs one step and, in one process, for each voxel size (default 0.005 and
0.02), end_margin 1 and a max_steps that skips nothing (SDM_FREESPACE_MAX_STEPS; rays_skipped is reported), for each
destination kind (torch device tensors, pageable NumPy) takes the median wall time of --reps calls after --warmup calls
(every call ends with a stream synchronise):
  (a) extract_points_voxel_cameras    fields xyz, multiplicity, source_index, cam_offsets and cam_slots
  (b) extract_points_voxel_freespace  the same plus crossings
  (c) today's route: (a) into pageable memory + tests/carve_np.py on this machine's CPU (--host-reps runs), its counts and
      totals checked equal to (b)'s.  Rows whose walk has more than --host-max-cells counted cells skip (c): the NumPy walk
      of such a row takes minutes.
Expectation to check, not a gate: (b) into pageable memory takes less wall time than (c).
Nanoseconds per visited cell come from a separate run of this tool under `rocprofv3 --kernel-trace --stats` (writing its own
--out); `--trace-csv STATS --trace-json THAT_OUT` then merges k_voxel_carve's time per counted cell into the JSON (no GPU).
Writes profiles/voxel_freespace_mi355x.json and prints it.

  python tools/voxel_freespace_rate.py
  python tools/voxel_freespace_rate.py --only 480p:64:20
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
VOXELS = [0.005, 0.02]
OUT = os.path.join(ROOT, "profiles", "voxel_freespace_mi355x.json")
MAX_STEPS = 65536  # SDM_FREESPACE_MAX_STEPS


def wall_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def run(pkg, torch, bench, res, kfs, nbrs, args):
    import carve_np
    wl = bench.Workload(pkg, torch, res, kfs, nbrs, 2.6, 1, 0, 0)
    wl.step("allgather", "torch")
    torch.cuda.synchronize()
    eng, slots, ms = wl.eng, list(wl.pl["own_slots"]), args.max_sigma
    rows = np.ascontiguousarray(np.asarray(wl.pl["nbr_slots"], np.int32).reshape(len(slots), -1))
    centres = {int(wl.pl["slot"][k]): carve_np.camera_centre(wl.scene.Tcw(k)) for k in wl.pl["inputs"]}
    cap = max(eng.extract_bound(slots), 1)
    cam_cap = cap * (1 + rows.shape[1])

    def buffers(kind, crossings):
        if kind == "device":
            out = {"xyz": torch.empty((cap, 3), dtype=torch.float32, device="cuda"),
                   "multiplicity": torch.empty(cap, dtype=torch.int32, device="cuda"),
                   "source_index": torch.empty(cap, dtype=torch.int32, device="cuda"),
                   "cam_offsets": torch.empty(cap + 1, dtype=torch.int64, device="cuda"),
                   "cam_slots": torch.empty(cam_cap, dtype=torch.int32, device="cuda")}
            if crossings:
                out["crossings"] = torch.empty(cap, dtype=torch.int32, device="cuda")
        else:
            out = {"xyz": np.empty((cap, 3), np.float32), "multiplicity": np.empty(cap, np.uint32),
                   "source_index": np.empty(cap, np.uint32), "cam_offsets": np.empty(cap + 1, np.int64),
                   "cam_slots": np.empty(cam_cap, np.int32)}
            if crossings:
                out["crossings"] = np.empty(cap, np.uint32)
        return out

    w, r, margin = args.warmup, args.reps, args.end_margin
    doc = {"workload": bench.workload_name(wl.W, wl.H, kfs, nbrs, res), "keyframes": len(slots), "n_nbr": int(rows.shape[1]),
           "max_sigma": ms, "end_margin": margin, "max_steps": MAX_STEPS, "voxels": []}
    for voxel in args.voxel or VOXELS:
        row = {"voxel_size": voxel}
        for kind in ("device", "pageable"):
            out_a, out_b = buffers(kind, False), buffers(kind, True)
            a = wall_ms(lambda: eng.extract_points_voxel_cameras(slots, rows, voxel, max_sigma=ms, out=out_a), w, r)
            b = wall_ms(lambda: eng.extract_points_voxel_freespace(slots, rows, voxel, margin, MAX_STEPS, max_sigma=ms,
                                                                   out=out_b), w, r)
            row["ms_a_extract_points_voxel_cameras_" + kind] = round(a, 4)
            row["ms_b_extract_points_voxel_freespace_" + kind] = round(b, 4)
            row["ms_b_minus_a_" + kind] = round(b - a, 4)
        got = eng.extract_points_voxel_freespace(slots, rows, voxel, margin, MAX_STEPS, max_sigma=ms, out=buffers("pageable", True))
        M, E, cells = len(got["crossings"]), int(got["rays_total"]), int(got["cells_visited"])
        row.update(kept_points_M=M, rays_E=E, rays_skipped=int(got["rays_skipped"]), cells_visited=cells,
                   mean_counted_cells_per_ray=round(cells / max(E, 1), 2),
                   kept_points_crossed=int((np.asarray(got["crossings"]) > 0).sum()),
                   kept_points_crossed_at_least_their_cameras=int((np.asarray(got["crossings"]) >=
                                                                   np.diff(np.asarray(got["cam_offsets"]))).sum()))
        if cells <= args.host_max_cells:
            out_c = buffers("pageable", False)
            host = {}

            def route():
                v = eng.extract_points_voxel_cameras(slots, rows, voxel, max_sigma=ms, out=out_c)
                host["r"] = carve_np.freespace(v["xyz"], v["cam_offsets"], v["cam_slots"], centres, voxel, margin, MAX_STEPS)

            row["ms_c_host_route"] = round(wall_ms(route, 0, args.host_reps), 2)
            ref = host["r"]
            row["b_equals_c"] = bool(np.array_equal(np.asarray(got["crossings"]), ref["crossings"]) and
                                     (E, int(got["rays_skipped"]), cells) ==
                                     (ref["rays_total"], ref["rays_skipped"], ref["cells_visited"]))
            row["b_pageable_below_c"] = bool(row["ms_b_extract_points_voxel_freespace_pageable"] < row["ms_c_host_route"])
        else:
            row["ms_c_host_route"] = row["b_equals_c"] = row["b_pageable_below_c"] = None
        doc["voxels"].append(row)
    wl.close()
    return doc


def add_trace(out_path, traced_json, stats_csv):
    """no GPU: k_voxel_carve's row of the kernel statistics (columns Name, Calls, TotalDurationNs) of a traced run of this
    tool, divided by the cells the traced run's calls counted (every row of it made the same number of calls), goes into
    the JSON of the untraced run as "k_voxel_carve_trace" """
    import csv
    with open(stats_csv) as f:
        rec = [r for r in csv.DictReader(f) if "k_voxel_carve" in r["Name"]]
    with open(traced_json) as f:
        traced = json.load(f)
    rows = [v for r in traced["runs"] for v in r["voxels"]]
    total_ns, calls = float(rec[0]["TotalDurationNs"]), int(rec[0]["Calls"])
    per_row = calls / len(rows)
    cells = sum(v["cells_visited"] for v in rows) * per_row
    with open(out_path) as f:
        doc = json.load(f)
    doc["k_voxel_carve_trace"] = {"workloads": [r["workload"] for r in traced["runs"]],
                                  "voxels": sorted({v["voxel_size"] for v in rows}), "calls": calls, "total_ns": total_ns,
                                  "mean_us_per_call": round(total_ns / calls / 1e3, 2),
                                  "ns_per_visited_cell": round(total_ns / cells, 5)}
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["k_voxel_carve_trace"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", action="append", help="res:keyframes:neighbours (repeatable; default: %s)" % ", ".join(CONFIGS))
    ap.add_argument("--voxel", action="append", type=float, help="voxel size (repeatable; default: 0.005, 0.02)")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--host-max-cells", type=float, default=3e8, help="skip (c) on rows with more counted cells (about 4 ns each in NumPy)")
    ap.add_argument("--end-margin", type=int, default=1)
    ap.add_argument("--max-sigma", type=float, default=0.1)
    ap.add_argument("--trace-csv", help="kernel statistics of a separate traced run of this tool")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--trace-json", help="with --trace-csv: the JSON the traced run wrote; merges the figure into --out and exits")
    args = ap.parse_args()
    if args.trace_csv:
        add_trace(args.out, args.trace_json, args.trace_csv)
        return 0

    import torch
    import bench
    import sdm_pkg
    pkg = sdm_pkg.load()
    runs = []
    for cfg in args.only or CONFIGS:
        res, kfs, nbrs = cfg.split(":")
        runs.append(run(pkg, torch, bench, res, int(kfs), int(nbrs), args))
        print(json.dumps(runs[-1]), flush=True)
    doc = {"metric": "free-space counts of the merged cloud: wall ms per call (median; every call ends with a stream "
                     "synchronise), fields xyz + multiplicity + source_index + cam_offsets + cam_slots (+ crossings); (c) is "
                     "extract_points_voxel_cameras into pageable memory plus the NumPy ray walk on the host",
           "reps": args.reps, "warmup": args.warmup, "host_reps": args.host_reps,
           "arch": torch.cuda.get_device_properties(0).gcnArchName, "runs": runs}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    ok = all(v["b_equals_c"] is not False for r in runs for v in r["voxels"])
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
