#!/usr/bin/env python3
"""The online route to free-space evidence: what integrating and carving a block of keyframes on the persistent voxel map
(sdm_vmap_integrate + sdm_vmap_carve) costs next to the only route there was, re-merging and re-walking everything
integrated so far (sdm_extract_points_voxel_freespace).

Builds bench.py's configs[1] (640x480 x 64 keyframes x 20 neighbours; sigma gate 0.1, source 1), runs one step and, for
each voxel size (default 0.02 and 0.005), hands the 64 keyframes over in 8 blocks of 8 with their full neighbour rows
(n_nbr 20), end_margin 1.  Per block, wall time (every call ends with a stream synchronise; median of --reps passes over
the 8 blocks after --warmup passes), into pageable memory:
  (a) extract_points_voxel_freespace over all the slots integrated so far: xyz and crossings of the kept points
  (b) vmap_integrate of the block, vmap_carve of the block, then a fetch of the evidence of the created range.  Each
      pass starts from vmap_clear, which keeps the table and the counters' allocation: no pass after the first grows
      anything.
The two routes do not count the same thing -- (a) counts the rays of every slot so far through the merged cloud of the
call, (b) the rays of the block through the entries present -- so no result is compared across them; (b) is checked
against itself: the counters fetched at the end sum to the cells_hit and ends_hit the calls returned, pass after pass.
Expectation to report against, not a gate: (b) per block stays flat while (a) grows with the block index.
Per-kernel device times need a kernel trace of their own (timing only, no counters):
    rocprofv3 --kernel-trace --stats -d DIR -o carve --output-format csv -- python tools/vmap_carve_rate.py --out DIR/run.json
    python tools/vmap_carve_rate.py --kernel-stats DIR/.../carve_kernel_stats.csv
The second adds the k_vmap_* and k_voxel_carve rows of the trace to --out (the wall times of the traced run are inflated
and not kept).  Writes profiles/vmap_carve_mi355x.json and prints it.
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

VOXELS = [0.02, 0.005]
OUT = os.path.join(ROOT, "profiles", "vmap_carve_mi355x.json")
BLOCK = 8
TOTALS = ("plain_total", "rays_total", "rays_skipped", "cells_visited", "cells_hit", "ends_hit")


def run(pkg, torch, bench, args):
    res, kfs, nbrs = "480p", 64, 20
    wl = bench.Workload(pkg, torch, res, kfs, nbrs, 2.6, 1, 0, 0)
    wl.step("allgather", "torch")
    torch.cuda.synchronize()
    eng, slots, ms = wl.eng, list(wl.pl["own_slots"]), args.max_sigma
    rows = np.ascontiguousarray(np.asarray(wl.pl["nbr_slots"], np.int32).reshape(len(slots), -1))
    blocks = [list(range(i, min(i + BLOCK, len(slots)))) for i in range(0, len(slots), BLOCK)]  # indices into slots / rows
    cap = max(eng.extract_bound(slots), 1)
    out_a = {"xyz": np.empty((cap, 3), np.float32), "crossings": np.empty(cap, np.uint32)}
    out_b = {"crossings": np.empty(cap, np.uint64), "ends": np.empty(cap, np.uint64)}
    T = int(eng.extract_points(slots, max_sigma=ms, fields=("pixel",))["offsets"][-1])
    doc = {"workload": bench.workload_name(wl.W, wl.H, kfs, nbrs, res), "keyframes": len(slots), "block": BLOCK,
           "n_nbr": int(rows.shape[1]), "end_margin": args.end_margin, "max_steps": args.max_steps, "max_sigma": ms,
           "plain_points_T": T, "voxels": []}
    kw = dict(max_sigma=ms)
    for voxel in args.voxel or VOXELS:
        ta = [[] for _ in blocks]
        tb = [[] for _ in blocks]
        tb_carve = [[] for _ in blocks]
        rays_a = [0] * len(blocks)
        totals = [None] * len(blocks)
        for rep in range(args.warmup + args.reps):
            for b in range(len(blocks)):
                done = [i for blk in blocks[:b + 1] for i in blk]
                sl = [slots[i] for i in done]
                t0 = time.perf_counter()
                got = eng.extract_points_voxel_freespace(sl, rows[done], voxel, args.end_margin, args.max_steps, out=out_a, **kw)
                if rep >= args.warmup:
                    ta[b].append((time.perf_counter() - t0) * 1e3)
                rays_a[b] = int(got["rays_total"])
        eng.vmap_open(voxel)
        consistent = True
        for rep in range(args.warmup + args.reps):
            eng.vmap_clear()
            for b, blk in enumerate(blocks):
                sl = [slots[i] for i in blk]
                t0 = time.perf_counter()
                d = eng.vmap_integrate(sl, updated=False, **kw)
                t1 = time.perf_counter()
                cv = eng.vmap_carve(sl, rows[blk], args.end_margin, args.max_steps, **kw)
                t2 = time.perf_counter()
                if d["created"]:
                    eng.vmap_fetch_evidence(first=d["first_created"], count=d["created"], out=out_b)
                if rep >= args.warmup:
                    tb[b].append((time.perf_counter() - t0) * 1e3)
                    tb_carve[b].append((t2 - t1) * 1e3)
                totals[b] = dict({f: cv[f] for f in TOTALS}, created=d["created"])
            ev = eng.vmap_fetch_evidence()
            consistent &= int(ev["crossings"].sum()) == sum(t["cells_hit"] for t in totals)
            consistent &= int(ev["ends"].sum()) == sum(t["ends_hit"] for t in totals)
        info = eng.vmap_info()
        eng.vmap_close()
        ma = [round(float(np.median(t)), 4) for t in ta]
        mb = [round(float(np.median(t)), 4) for t in tb]
        mc = [round(float(np.median(t)), 4) for t in tb_carve]
        doc["voxels"].append({"voxel_size": voxel, "ms_a_freespace_over_all_so_far": ma, "rays_a": rays_a,
                              "ms_b_integrate_carve_fetch": mb, "ms_b_carve_call_alone": mc, "b_totals": totals,
                              "final_voxels_M": info["voxels"], "table_slots": info["table_slots"],
                              "b_counters_sum_to_the_returned_totals": bool(consistent),
                              "a_last_over_first": round(ma[-1] / ma[0], 3), "b_last_over_first": round(mb[-1] / mb[0], 3),
                              "ms_a_sum_over_blocks": round(sum(ma), 4), "ms_b_sum_over_blocks": round(sum(mb), 4)})
    wl.close()
    return doc


def add_kernel_stats(args):
    doc = json.load(open(args.out))
    rows = []
    for r in csv.DictReader(open(args.kernel_stats)):
        if "k_vmap_" in r["Name"] or "k_voxel_carve" in r["Name"]:
            rows.append({"kernel": r["Name"].split("(")[0], "calls": int(r["Calls"]),
                         "total_ms": round(float(r["TotalDurationNs"]) / 1e6, 4),
                         "mean_us": round(float(r["TotalDurationNs"]) / max(int(r["Calls"]), 1) / 1e3, 3)})
    doc["kernel_stats"] = {"rows": rows, "note": "one rocprofv3 --kernel-trace --stats run of this script, all voxel sizes and "
                                                  "blocks together"}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["kernel_stats"]))
    return 0 if rows else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel", action="append", type=float, help="voxel size (repeatable; default: 0.02, 0.005)")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-sigma", type=float, default=0.1)
    ap.add_argument("--end-margin", type=int, default=1)
    ap.add_argument("--max-steps", type=int, default=4096)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--kernel-stats", help="rocprofv3 kernel stats CSV of a traced run of this script: add its kernel rows to --out")
    args = ap.parse_args()
    if args.kernel_stats:
        return add_kernel_stats(args)

    import torch
    import bench
    import sdm_pkg
    pkg = sdm_pkg.load()
    doc = {"metric": "free-space evidence, online: wall ms per block of 8 keyframes (median; every call ends with a stream "
                     "synchronise), pageable destinations; (a) re-merges and re-walks every slot integrated so far, (b) "
                     "integrates and carves the block on the persistent map and fetches the evidence of the created range",
           "reps": args.reps, "warmup": args.warmup, "arch": torch.cuda.get_device_properties(0).gcnArchName}
    doc.update(run(pkg, torch, bench, args))
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    return 0 if all(v["b_counters_sum_to_the_returned_totals"] for v in doc["voxels"]) else 1


if __name__ == "__main__":
    sys.exit(main())
