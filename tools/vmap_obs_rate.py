#!/usr/bin/env python3
"""The online route to the camera lists of the voxel map: what observing a block of keyframes (sdm_vmap_observe) and
fetching the created range of the observation log costs next to the only route there was, re-merging everything
integrated so far with its camera lists.

Builds bench.py's configs[1] (640x480 x 64 keyframes x 20 neighbours; sigma gate 0.1, source 1), runs one step and, for
each voxel size (default 0.02 and 0.005), hands the 64 keyframes over in 8 blocks of 8 with their full neighbour rows.
Per block, wall time (every call ends with a stream synchronise; median of --reps passes over the 8 blocks after --warmup
passes), into pageable memory:
  (a) extract_points_voxel_cameras over all the slots integrated so far: cam_offsets and cam_slots only
  (b) vmap_observe of the block, then a fetch of the created range of the log (entry and tag).  The block's
      vmap_integrate runs before it, untimed (tools/vmap_rate.py times that).  Each pass starts from vmap_clear, which
      keeps the set, the log and the per-entry arrays: no pass after the first grows anything.
(b)'s final lists are checked against (a)'s last result by O3 of include/sdm_c.h: the list of every entry equals the
cam_slots list of the kept point with the same (tag, pixel).  Expectation to report against, not a gate: (b) per block
stays flat while (a) grows with the block index.
Writes profiles/vmap_obs_mi355x.json and prints it.
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
OUT = os.path.join(ROOT, "profiles", "vmap_obs_mi355x.json")
BLOCK = 8


def run(pkg, torch, bench, args):
    import voxel_np
    res, kfs, nbrs = "480p", 64, 20
    wl = bench.Workload(pkg, torch, res, kfs, nbrs, 2.6, 1, 0, 0)
    wl.step("allgather", "torch")
    torch.cuda.synchronize()
    eng, slots, ms = wl.eng, list(wl.pl["own_slots"]), args.max_sigma
    rows = np.ascontiguousarray(np.asarray(wl.pl["nbr_slots"], np.int32).reshape(len(slots), -1))
    blocks = [list(range(i, min(i + BLOCK, len(slots)))) for i in range(0, len(slots), BLOCK)]  # indices into slots / rows
    kw = dict(max_sigma=ms)
    cap = max(eng.extract_bound(slots), 1)
    T = int(eng.extract_points(slots, fields=("pixel",), **kw)["offsets"][-1])
    out_a = {"cam_offsets": np.empty(cap + 1, np.int64), "cam_slots": np.empty(cap * (rows.shape[1] + 1), np.int32)}
    out_b = {"entry": np.empty(cap * (rows.shape[1] + 1), np.uint32), "tag": np.empty(cap * (rows.shape[1] + 1), np.int32)}
    doc = {"workload": bench.workload_name(wl.W, wl.H, kfs, nbrs, res), "keyframes": len(slots), "block": BLOCK,
           "n_nbr": int(rows.shape[1]), "max_sigma": ms, "plain_points_T": T, "voxels": []}
    for voxel in args.voxel or VOXELS:
        ta = [[] for _ in blocks]
        tb = [[] for _ in blocks]
        deltas = [None] * len(blocks)
        for rep in range(args.warmup + args.reps):
            for b in range(len(blocks)):
                done = [i for blk in blocks[:b + 1] for i in blk]
                t0 = time.perf_counter()
                eng.extract_points_voxel_cameras([slots[i] for i in done], rows[done], voxel, fields=(), out=out_a, **kw)
                if rep >= args.warmup:
                    ta[b].append((time.perf_counter() - t0) * 1e3)
        eng.vmap_open(voxel)
        for rep in range(args.warmup + args.reps):
            eng.vmap_clear()
            for b, blk in enumerate(blocks):
                sl = [slots[i] for i in blk]
                eng.vmap_integrate(sl, updated=False, **kw)
                t0 = time.perf_counter()
                d = eng.vmap_observe(sl, rows[blk], **kw)
                if d["created"]:
                    eng.vmap_fetch_observations(first=d["first_created"], count=d["created"], out=out_b)
                if rep >= args.warmup:
                    tb[b].append((time.perf_counter() - t0) * 1e3)
                deltas[b] = d
        # O3 holds for one integrate of everything; the lists are independent of how the integrates and observes were cut
        # only through the ids, so match by (tag, pixel) as O3 does
        info, oinfo = eng.vmap_info(), eng.vmap_obs_info()
        rec = eng.vmap_fetch(fields=("tag", "pixel"))
        cams = eng.vmap_fetch_cameras()
        vox = eng.extract_points_voxel_cameras(slots, rows, voxel, fields=("xyz", "pixel"), **kw)
        _, ok = voxel_np.cells(vox["xyz"], voxel)
        tag = np.repeat(np.asarray(slots, np.int32), np.diff(vox["offsets"]))
        want = {}
        for k in np.flatnonzero(ok):
            want[(int(tag[k]), int(vox["pixel"][k]))] = vox["cam_slots"][vox["cam_offsets"][k]:vox["cam_offsets"][k + 1]].tobytes()
        same = len(want) == info["voxels"] and all(
            cams["cam_tags"][cams["cam_offsets"][e]:cams["cam_offsets"][e + 1]].tobytes() == want.get((int(rec["tag"][e]), int(rec["pixel"][e])))
            for e in range(info["voxels"]))
        eng.vmap_close()
        ma = [round(float(np.median(t)), 4) for t in ta]
        mb = [round(float(np.median(t)), 4) for t in tb]
        doc["voxels"].append({"voxel_size": voxel, "ms_a_remerge_all_so_far_with_cameras": ma, "ms_b_observe_and_fetch_created": mb,
                              "deltas": deltas, "final_voxels_M": info["voxels"], "observations_E": oinfo["observations"],
                              "obs_table_slots": oinfo["table_slots"], "b_final_lists_equal_a_last": bool(same),
                              "a_last_over_first": round(ma[-1] / ma[0], 3), "b_last_over_first": round(mb[-1] / mb[0], 3),
                              "ms_a_sum_over_blocks": round(sum(ma), 4), "ms_b_sum_over_blocks": round(sum(mb), 4)})
    wl.close()
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel", action="append", type=float, help="voxel size (repeatable; default: 0.02, 0.005)")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-sigma", type=float, default=0.1)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()

    import torch
    import bench
    import sdm_pkg
    pkg = sdm_pkg.load()
    doc = {"metric": "camera lists of the voxel map, online: wall ms per block of 8 keyframes (median; every call ends with a "
                     "stream synchronise), pageable destinations; (a) re-merges every slot integrated so far with its camera "
                     "lists, (b) observes the block on the persistent map and fetches the created range of the log",
           "reps": args.reps, "warmup": args.warmup, "arch": torch.cuda.get_device_properties(0).gcnArchName}
    doc.update(run(pkg, torch, bench, args))
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    return 0 if all(v["b_final_lists_equal_a_last"] for v in doc["voxels"]) else 1


if __name__ == "__main__":
    sys.exit(main())
