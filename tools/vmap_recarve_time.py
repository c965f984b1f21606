#!/usr/bin/env python3
"""Rebuilding a voxel map's free-space evidence from its observation log: what sdm_vmap_recarve costs.

The workload is tools/vmap_repose_time.py's: by vmap_import and vmap_import_observations, a map of about --entries entries
(default 10^6 records) seen by --keyframes keyframes and a log of three pairs per entry; every entry's xyz is its pixel and
rho under its keyframe's pose.  The table holds the poses of all keyframes, so every pair is a ray.  Per pass one
vmap_recarve(reset=True) over the whole log; wall time ending in a stream synchronise.  --warmup passes are dropped;
median, minimum and maximum of --reps passes are reported, with the returned rays_total and cells_visited, so that rays/s
and cells/s can be read off.  Every pass must return the same outs and leave the same counters; the exit code says so.
There is no earlier device route to compare against (the counters cannot be imported, so a host round trip does not
exist) and no threshold is set.
Writes profiles/vmap_recarve_mi355x.json and prints it."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

OUT = os.path.join(ROOT, "profiles", "vmap_recarve_mi355x.json")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=1000000)
    ap.add_argument("--keyframes", type=int, default=200)
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--end-margin", type=int, default=1)
    ap.add_argument("--max-steps", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()

    import torch
    import sdm_pkg
    import vmap_repose_np as vr
    import vmap_repose_time as workload
    pkg = sdm_pkg.load()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    rng = np.random.default_rng(2026)
    rec, poses = workload.make_map(vr, rng, args.entries, args.keyframes)
    eng = pkg.Engine(64, 48, 1)
    eng.vmap_open(args.voxel, len(rec["pixel"]))
    d = eng.vmap_import(rec, updated=False)
    M = eng.vmap_info()["voxels"]
    eng.vmap_import_observations(rng.integers(0, M, 3 * M).astype(np.uint32), rng.integers(0, args.keyframes, 3 * M).astype(np.int32))
    E = eng.vmap_obs_info()["observations"]
    tags = np.arange(args.keyframes, dtype=np.int32)[::-1].copy()
    Tcw = np.ascontiguousarray(poses[tags])

    times, outs, sums = [], [], []
    for rep in range(args.warmup + args.reps):
        eng.synchronize()
        t0 = time.perf_counter()
        got = eng.vmap_recarve(tags, Tcw, args.end_margin, args.max_steps, reset=True)
        eng.synchronize()
        t = (time.perf_counter() - t0) * 1e3
        if rep >= args.warmup:
            times.append(t)
        outs.append(got)
        if rep in (0, args.warmup + args.reps - 1):
            ev = eng.vmap_fetch_evidence()
            sums.append(hashlib.sha256(ev["crossings"].tobytes() + ev["ends"].tobytes()).hexdigest())
    same = all(o == outs[0] for o in outs) and sums[0] == sums[-1]
    eng.close()
    med = float(np.median(times))
    doc = {"metric": "rebuilding the free-space evidence of a voxel map from its observation log: wall ms per "
                     "sdm_vmap_recarve(reset = 1) over the whole log, ending with a stream synchronise",
           "reps": args.reps, "warmup": args.warmup, "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "entries_M": int(M), "records_imported": int(d["total"]), "observations_E": int(E), "keyframes": args.keyframes,
           "poses_in_table": int(len(tags)), "voxel_size": args.voxel, "end_margin": args.end_margin, "max_steps": args.max_steps,
           "outs": outs[0], "passes_agree": bool(same),
           "ms_recarve": {"median": round(med, 3), "min": round(float(np.min(times)), 3), "max": round(float(np.max(times)), 3)},
           "rays_per_s_at_median": round(outs[0]["rays_total"] / (med * 1e-3)),
           "cells_per_s_at_median": round(outs[0]["cells_visited"] / (med * 1e-3))}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
