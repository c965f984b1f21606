#!/usr/bin/env python3
"""The online route to one point per voxel: what integrating a block of keyframes into the persistent voxel map
(sdm_vmap_integrate) costs next to the only route there was, re-merging everything integrated so far.

Builds bench.py's configs[1] (640x480 x 64 keyframes x 20 neighbours; sigma gate 0.1, source 1), runs one step and, for
each voxel size (default 0.005 and 0.02), hands the 64 keyframes over in 8 blocks of 8.  Per block, wall time (every call
ends with a stream synchronise; median of --reps passes over the 8 blocks after --warmup passes), into pageable memory:
  (a) extract_points_voxel over all the slots integrated so far: fields xyz, rho_sigma, multiplicity, source_index
  (b) vmap_integrate of the block, then a fetch of the created range, then a fetch of updated_ids: fields xyz, rho_sigma,
      multiplicity.  Each pass starts from vmap_clear, which keeps the table: no pass after the first grows anything.
(b)'s final map is checked against (a)'s last result: the same points, field bits and multiplicities, matched by
(tag, pixel).  Expectation to check, not a gate: (b) per block stays flat while (a) grows with the block index.
Per-kernel device times need a kernel trace of their own:
    rocprofv3 --kernel-trace --stats -d DIR -o vmap --output-format csv -- python tools/vmap_rate.py --out DIR/run.json
    python tools/vmap_rate.py --kernel-stats DIR/.../vmap_kernel_stats.csv
The second adds the k_vmap_* rows of the trace to --out (the wall times of the traced run are inflated and not kept).
Writes profiles/vmap_mi355x.json and prints it.
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

VOXELS = [0.005, 0.02]
OUT = os.path.join(ROOT, "profiles", "vmap_mi355x.json")
BLOCK = 8
FETCH = ("xyz", "rho_sigma", "multiplicity")


def run(pkg, torch, bench, args):
    import voxel_np
    res, kfs, nbrs = "480p", 64, 20
    wl = bench.Workload(pkg, torch, res, kfs, nbrs, 2.6, 1, 0, 0)
    wl.step("allgather", "torch")
    torch.cuda.synchronize()
    eng, slots, ms = wl.eng, list(wl.pl["own_slots"]), args.max_sigma
    blocks = [slots[i:i + BLOCK] for i in range(0, len(slots), BLOCK)]
    cap = max(eng.extract_bound(slots), 1)
    out_a = {"xyz": np.empty((cap, 3), np.float32), "rho_sigma": np.empty((cap, 2), np.float32),
             "multiplicity": np.empty(cap, np.uint32), "source_index": np.empty(cap, np.uint32)}
    out_b = {"xyz": np.empty((cap, 3), np.float32), "rho_sigma": np.empty((cap, 2), np.float32),
             "multiplicity": np.empty(cap, np.uint32)}
    upd = np.empty(cap, np.uint32)
    T = int(eng.extract_points(slots, max_sigma=ms, fields=("pixel",))["offsets"][-1])
    doc = {"workload": bench.workload_name(wl.W, wl.H, kfs, nbrs, res), "keyframes": len(slots), "block": BLOCK,
           "max_sigma": ms, "plain_points_T": T, "voxels": []}
    for voxel in args.voxel or VOXELS:
        ta = [[] for _ in blocks]
        tb = [[] for _ in blocks]
        deltas = [None] * len(blocks)
        for rep in range(args.warmup + args.reps):
            for b in range(len(blocks)):
                done = [s for blk in blocks[:b + 1] for s in blk]
                t0 = time.perf_counter()
                eng.extract_points_voxel(done, voxel, max_sigma=ms, out=out_a)
                if rep >= args.warmup:
                    ta[b].append((time.perf_counter() - t0) * 1e3)
        eng.vmap_open(voxel)
        for rep in range(args.warmup + args.reps):
            eng.vmap_clear()
            for b, blk in enumerate(blocks):
                t0 = time.perf_counter()
                d = eng.vmap_integrate(blk, max_sigma=ms, updated=upd)
                if d["created"]:
                    eng.vmap_fetch(first=d["first_created"], count=d["created"], out=out_b)
                if d["updated"]:
                    eng.vmap_fetch(ids=d["updated_ids"], out=out_b)
                if rep >= args.warmup:
                    tb[b].append((time.perf_counter() - t0) * 1e3)
                deltas[b] = {f: d[f] for f in ("plain_total", "dropped", "created", "updated")}
        # I2: the final map against the per-call merge over all 64 keyframes
        info = eng.vmap_info()
        full = eng.vmap_fetch()
        vox = eng.extract_points_voxel(slots, voxel, max_sigma=ms, fields=("xyz", "pixel", "rho_sigma", "intensity"))
        _, ok = voxel_np.cells(vox["xyz"], voxel)
        tag = np.repeat(np.asarray(slots, np.int32), np.diff(vox["offsets"]))
        o1, o2 = np.lexsort((full["pixel"], full["tag"])), np.lexsort((vox["pixel"][ok], tag[ok]))
        same = info["voxels"] == int(ok.sum()) and info["dropped"] == int((~ok).sum()) and all(
            np.asarray(full[f])[o1].tobytes() == np.asarray(vox[f])[ok][o2].tobytes()
            for f in ("xyz", "pixel", "rho_sigma", "intensity", "multiplicity")) and np.array_equal(full["tag"][o1], tag[ok][o2])
        eng.vmap_close()
        ma = [round(float(np.median(t)), 4) for t in ta]
        mb = [round(float(np.median(t)), 4) for t in tb]
        doc["voxels"].append({"voxel_size": voxel, "ms_a_remerge_all_so_far": ma, "ms_b_integrate_and_fetch_delta": mb,
                              "deltas": deltas, "final_voxels_M": info["voxels"], "table_slots": info["table_slots"],
                              "b_final_map_equals_a_last": bool(same),
                              "a_last_over_first": round(ma[-1] / ma[0], 3), "b_last_over_first": round(mb[-1] / mb[0], 3),
                              "ms_a_sum_over_blocks": round(sum(ma), 4), "ms_b_sum_over_blocks": round(sum(mb), 4)})
    wl.close()
    return doc


def add_kernel_stats(args):
    doc = json.load(open(args.out))
    rows = []
    for r in csv.DictReader(open(args.kernel_stats)):
        if "k_vmap_" in r["Name"]:
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
    ap.add_argument("--voxel", action="append", type=float, help="voxel size (repeatable; default: 0.005, 0.02)")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-sigma", type=float, default=0.1)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--kernel-stats", help="rocprofv3 kernel stats CSV of a traced run of this script: add its k_vmap_* rows to --out")
    args = ap.parse_args()
    if args.kernel_stats:
        return add_kernel_stats(args)

    import torch
    import bench
    import sdm_pkg
    pkg = sdm_pkg.load()
    doc = {"metric": "one point per voxel, online: wall ms per block of 8 keyframes (median; every call ends with a stream "
                     "synchronise), pageable destinations; (a) re-merges every slot integrated so far, (b) integrates the "
                     "block into the persistent map and fetches what changed",
           "reps": args.reps, "warmup": args.warmup, "arch": torch.cuda.get_device_properties(0).gcnArchName}
    doc.update(run(pkg, torch, bench, args))
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    return 0 if all(v["b_final_map_equals_a_last"] for v in doc["voxels"]) else 1


if __name__ == "__main__":
    sys.exit(main())
