#!/usr/bin/env python3
"""Merging the voxel map of another rank: what sdm_vmap_import + sdm_vmap_import_observations cost next to integrating and
observing the same keyframes in place.

Builds bench.py's configs[1] (640x480 x 64 keyframes x 20 neighbours; sigma gate 0.1, source 1) twice -- two engines on one
GPU -- and runs one step in each.  Engine B integrates and observes the second half of the keyframes (one call per
keyframe, full neighbour rows) into its map; its full vmap_fetch and vmap_fetch_observations are taken once, into pageable
host arrays and into torch device tensors.  Then, per voxel size (default 0.02 and 0.005) and pass, engine A starts from
vmap_clear, integrates and observes the FIRST half (untimed) and one of three routes brings in the second half; wall time
(every route ends with a stream synchronise; median of --reps passes after --warmup passes):
  (a) vmap_integrate + vmap_observe of the second half's keyframes, one call each per keyframe -- the route a single map
      takes, and the only one there was before the import
  (b) vmap_import of B's records from host arrays, then vmap_import_observations of B's log with dst_ids as entry_map
  (c) the same from device tensors, dst_ids staying on the device
The three routes must leave the same M, points and E, and (b) and (c) the same records as (a) apart from epoch; the exit
code says so.  No threshold is set: nothing here was measured before.
Writes profiles/vmap_import_mi355x.json and prints it.
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

VOXELS = [0.02, 0.005]
OUT = os.path.join(ROOT, "profiles", "vmap_import_mi355x.json")
RECORD = ("xyz", "pixel", "rho_sigma", "intensity", "tag", "multiplicity")


def fill(eng, slots, rows, idx, kw):
    for i in idx:
        eng.vmap_integrate([slots[i]], updated=False, **kw)
        eng.vmap_observe([slots[i]], rows[[i]], **kw)


def run_voxel(torch, A, B, slots, rows, kw, voxel, args):
    half = len(slots) // 2
    first, second = list(range(half)), list(range(half, len(slots)))
    A.vmap_open(voxel)
    B.vmap_open(voxel)
    fill(B, slots, rows, second, kw)
    host = B.vmap_fetch(fields=RECORD)
    hlog = B.vmap_fetch_observations()
    m1, e1 = len(host["pixel"]), len(hlog["entry"])
    dev = {f: torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a)).cuda()
           for f, a in host.items()}
    dlog = {f: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda() for f, a in hlog.items()}
    B.vmap_close()
    times = {"a_integrate_observe": [], "b_import_host": [], "c_import_device": []}
    ends, recs = {}, {}
    for rep in range(args.warmup + args.reps):
        for route in times:
            A.vmap_clear()
            fill(A, slots, rows, first, kw)
            A.synchronize()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if route == "a_integrate_observe":
                fill(A, slots, rows, second, kw)
            elif route == "b_import_host":
                d = A.vmap_import(host, dst_ids=True, updated=False)
                A.vmap_import_observations(hlog["entry"], hlog["tag"], d["dst_ids"])
            else:
                d = A.vmap_import(dev, dst_ids=True, updated=False)
                A.vmap_import_observations(dlog["entry"], dlog["tag"], d["dst_ids"])
            A.synchronize()
            if rep >= args.warmup:
                times[route].append((time.perf_counter() - t0) * 1e3)
            if rep == 0:
                info = A.vmap_info()
                ends[route] = (info["voxels"], info["points"], A.vmap_obs_info()["observations"])
                full = A.vmap_fetch(fields=RECORD)
                recs[route] = {f: full[f].tobytes() for f in RECORD}
    plain = sum(A.extract_bound([slots[i]]) for i in second)
    A.vmap_close()
    same = ends["a_integrate_observe"] == ends["b_import_host"] == ends["c_import_device"] and \
        recs["a_integrate_observe"] == recs["b_import_host"] == recs["c_import_device"]
    one = {"voxel_size": voxel, "records_R": m1, "pairs_P": e1, "merged_M_points_E": list(ends["a_integrate_observe"]),
           "plain_point_bound_of_the_second_half": int(plain), "routes_agree": bool(same)}
    for route, t in times.items():
        one["ms_" + route] = round(float(np.median(t)), 4)
    one["bytes_b_over_the_link"] = 33 * m1 + 4 * m1 + 8 * e1 + 4 * m1
    return one


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel", action="append", type=float, help="voxel size (repeatable; default: 0.02, 0.005)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-sigma", type=float, default=0.1)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()

    import torch
    import bench
    import sdm_pkg
    pkg = sdm_pkg.load()
    res, kfs, nbrs = "480p", 64, 20
    wls = [bench.Workload(pkg, torch, res, kfs, nbrs, 2.6, 1, 0, 0) for _ in range(2)]
    for wl in wls:
        wl.step("allgather", "torch")
    torch.cuda.synchronize()
    A, B = wls[0].eng, wls[1].eng
    slots = list(wls[0].pl["own_slots"])
    rows = np.ascontiguousarray(np.asarray(wls[0].pl["nbr_slots"], np.int32).reshape(len(slots), -1))
    kw = dict(max_sigma=args.max_sigma)
    doc = {"metric": "bringing the second half of the keyframes into a voxel map that holds the first half: wall ms (median; "
                     "every route ends with a stream synchronise); (a) integrates and observes them in place, one call each per "
                     "keyframe, (b) imports another engine's fetched map and log from pageable host arrays, (c) from device tensors",
           "reps": args.reps, "warmup": args.warmup, "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "workload": bench.workload_name(wls[0].W, wls[0].H, kfs, nbrs, res), "keyframes": len(slots),
           "n_nbr": int(rows.shape[1]), "max_sigma": args.max_sigma, "voxels": []}
    for voxel in args.voxel or VOXELS:
        doc["voxels"].append(run_voxel(torch, A, B, slots, rows, kw, voxel, args))
    for wl in wls:
        wl.close()
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    return 0 if all(v["routes_agree"] for v in doc["voxels"]) else 1


if __name__ == "__main__":
    sys.exit(main())
