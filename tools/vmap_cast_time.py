#!/usr/bin/env python3
"""Ray queries on the voxel map: what sdm_vmap_render and sdm_vmap_cast_segments cost.

The workload is tools/vmap_repose_time.py's, as tools/vmap_recarve_time.py sets it up: by vmap_import and
vmap_import_observations, a map of about --entries entries (default 10^6 records) seen by --keyframes keyframes and a log of
three pairs per entry.  Three measurements, each the wall time of one call ending in a stream synchronise, sources and
destinations on the device:
  render   a 640 x 480 view from the pose of the middle keyframe, rays to inverse depth --rho-far.  That camera stands inside
           the cloud -- its own cell holds an entry -- so with start_margin 0 every pixel stops at once: the figure is the
           call's fixed cost.  The second render skips the first --near-clip cells of every ray (0.5 m at the defaults), as
           a viewer's near plane would, and walks (render_near_clip)
  cast     one segment per pair of the log, from the camera centre of the pair's keyframe to the xyz of the pair's entry --
           sdm_vmap_recarve's rays -- with end_margin = recarve's + 1 (the same cells) and no filter: the occlusion question
           asked of every (entry, camera) pair, beside profiles/vmap_recarve_mi355x.json's walk of the same rays to their ends
--warmup passes are dropped; median, minimum and maximum of --reps passes are reported with the returned totals, so that
rays/s and cells/s can be read off.  Every pass must return the same bits; the exit code says so.  The lane mapping is the
raster one (ray i on lane i); no tile mapping has been measured.  No device route existed before: no threshold is set.
Writes profiles/vmap_cast_mi355x.json and prints it."""
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

OUT = os.path.join(ROOT, "profiles", "vmap_cast_mi355x.json")


def timed(eng, call, warmup, reps, digest):
    times, outs, sums = [], [], []
    for rep in range(warmup + reps):
        eng.synchronize()
        t0 = time.perf_counter()
        got = call()
        eng.synchronize()
        t = (time.perf_counter() - t0) * 1e3
        if rep >= warmup:
            times.append(t)
        outs.append({f: v for f, v in got.items() if isinstance(v, int)})
        sums.append(digest(got))
    same = all(o == outs[0] for o in outs) and all(s == sums[0] for s in sums)
    med = float(np.median(times))
    return {"outs": outs[0], "passes_agree": bool(same),
            "ms": {"median": round(med, 3), "min": round(float(np.min(times)), 3), "max": round(float(np.max(times)), 3)},
            "rays_per_s_at_median": round(outs[0]["rays_total"] / (med * 1e-3)),
            "cells_per_s_at_median": round(outs[0]["cells_visited"] / (med * 1e-3))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=1000000)
    ap.add_argument("--keyframes", type=int, default=200)
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--end-margin", type=int, default=2)
    ap.add_argument("--max-steps", type=int, default=4096)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--rho-far", type=float, default=0.2)
    ap.add_argument("--near-clip", type=int, default=25)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()

    import torch
    import sdm_pkg
    import vmap_recarve_np as vrc
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
    log = eng.vmap_fetch_observations()
    E = len(log["entry"])
    xyz = np.array(eng.vmap_fetch(fields=("xyz",))["xyz"]).reshape(-1, 3)
    origins = torch.from_numpy(vrc.centres_of(poses)[log["tag"]]).cuda()
    ends = torch.from_numpy(xyz[log["entry"].astype(np.int64)]).cuda()
    n_px = args.width * args.height
    dst = {f: torch.empty(max(E, n_px), dtype=torch.float32 if f == "rho" else torch.int32, device="cuda") for f in ("ids", "steps", "rho")}

    def digest(n):
        return lambda got: hashlib.sha256(b"".join(got[f].reshape(-1)[:n].cpu().numpy().tobytes() for f in sorted(got)
                                                   if not isinstance(got[f], int))).hexdigest()

    mid = args.keyframes // 2
    render = timed(eng, lambda: eng.vmap_render(workload.K_CAM, poses[mid], args.width, args.height, args.rho_far,
                                                max_steps=args.max_steps, **dst), args.warmup, args.reps, digest(n_px))
    clipped = timed(eng, lambda: eng.vmap_render(workload.K_CAM, poses[mid], args.width, args.height, args.rho_far,
                                                 start_margin=args.near_clip, max_steps=args.max_steps, **dst),
                    args.warmup, args.reps, digest(n_px))
    cast = timed(eng, lambda: eng.vmap_cast_segments(origins, ends, end_margin=args.end_margin, max_steps=args.max_steps,
                                                     ids=dst["ids"], steps=dst["steps"]), args.warmup, args.reps, digest(E))
    eng.close()
    doc = {"metric": "ray queries on a voxel map: wall ms per sdm_vmap_render and per sdm_vmap_cast_segments over the log's (entry, "
                     "camera) segments, sources and destinations on the device, each ending with a stream synchronise",
           "reps": args.reps, "warmup": args.warmup, "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "entries_M": int(M), "records_imported": int(d["total"]), "observations_E": int(E), "keyframes": args.keyframes,
           "voxel_size": args.voxel, "max_steps": args.max_steps, "lane_mapping": "raster: ray i on lane i (no tile mapping measured)",
           "render": dict(render, width=args.width, height=args.height, rho_far=args.rho_far, pose_of_keyframe=mid, start_margin=0,
                          end_margin=0),
           "render_near_clip": dict(clipped, width=args.width, height=args.height, rho_far=args.rho_far, pose_of_keyframe=mid,
                                    start_margin=args.near_clip, end_margin=0),
           "cast_log_segments": dict(cast, start_margin=0, end_margin=args.end_margin)}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    return 0 if render["passes_agree"] and clipped["passes_agree"] and cast["passes_agree"] else 1


if __name__ == "__main__":
    sys.exit(main())
