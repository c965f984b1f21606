#!/usr/bin/env python3
"""Deciding which entries of the voxel map are surface, online: what sdm_vmap_classify costs per block next to the route it
replaces, fetching the per-entry state of ALL entries and filtering on the host.

Builds bench.py's configs[1] (640x480 x 64 keyframes x 20 neighbours; sigma gate 0.1, source 1), runs one step and, for
each voxel size (default 0.02 and 0.005), hands the 64 keyframes over in 8 blocks of 8 with their full neighbour rows:
integrate, observe, carve (untimed; tools/vmap_rate.py, vmap_obs_rate.py and vmap_carve_rate.py time those), then, per
block, wall time (every route ends with a stream synchronise; median of --reps passes over the 8 blocks after --warmup
passes):
  (a) vmap_fetch(multiplicity, rho_sigma) + vmap_fetch_evidence + vmap_fetch_cameras (offsets only) of all M entries into
      pageable memory, and the LOCAL tests in NumPy (no neighbour test: a host would have to rebuild the table for it)
  (b) vmap_classify, committing, with host id lists -- once per pass series with the rule's min_neighbours (2), once with 0,
      which prices the probes.  Each pass starts from vmap_clear, which keeps every capacity.
The flags of the min_neighbours 0 series are checked against (a)'s filter.  Expectation to report against, not a gate: the
bytes over the link of (b) follow the delta while those of (a) grow with M.
Writes profiles/vmap_classify_mi355x.json and prints it.
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
OUT = os.path.join(ROOT, "profiles", "vmap_classify_mi355x.json")
BLOCK = 8
RULE = dict(min_multiplicity=2, min_cameras=2, min_ends=2, ratio_num=1, ratio_den=2, max_sigma=0.05, min_neighbours=2)


def host_filter(state, offs, rule):
    """the LOCAL tests on fetched arrays (the counters of this workload are far below 2^32: uint64 products are exact)"""
    import voxel_np
    skey = voxel_np.sigma_key(state["rho_sigma"][:, 1])
    mkey = voxel_np.sigma_key(np.array([rule["max_sigma"]], np.float32))[0]
    return ((state["multiplicity"] >= rule["min_multiplicity"]) & (np.diff(offs) >= rule["min_cameras"]) &
            (state["ends"] >= rule["min_ends"]) &
            (state["crossings"] * np.uint64(rule["ratio_den"]) <= state["ends"] * np.uint64(rule["ratio_num"])) & (skey <= mkey))


def run(pkg, torch, bench, args):
    res, kfs, nbrs = "480p", 64, 20
    wl = bench.Workload(pkg, torch, res, kfs, nbrs, 2.6, 1, 0, 0)
    wl.step("allgather", "torch")
    torch.cuda.synchronize()
    eng, slots, ms = wl.eng, list(wl.pl["own_slots"]), args.max_sigma
    rows = np.ascontiguousarray(np.asarray(wl.pl["nbr_slots"], np.int32).reshape(len(slots), -1))
    blocks = [list(range(i, min(i + BLOCK, len(slots)))) for i in range(0, len(slots), BLOCK)]  # indices into slots / rows
    kw = dict(max_sigma=ms)
    cap = max(eng.extract_bound(slots), 1)
    out_rec = {"multiplicity": np.empty(cap, np.uint32), "rho_sigma": np.empty((cap, 2), np.float32)}
    out_ev = {"crossings": np.empty(cap, np.uint64), "ends": np.empty(cap, np.uint64)}
    out_cam = {"cam_offsets": np.empty(cap + 1, np.int64)}
    out_ids = {"accepted_ids": np.empty(cap, np.uint32), "retracted_ids": np.empty(cap, np.uint32)}
    doc = {"workload": bench.workload_name(wl.W, wl.H, kfs, nbrs, res), "keyframes": len(slots), "block": BLOCK,
           "n_nbr": int(rows.shape[1]), "max_sigma": ms, "rule": RULE, "voxels": []}
    for voxel in args.voxel or VOXELS:
        doc["voxels"].append(run_voxel(eng, slots, rows, blocks, kw, voxel, args, out_rec, out_ev, out_cam, out_ids))
    wl.close()
    return doc


def run_voxel(eng, slots, rows, blocks, kw, voxel, args, out_rec, out_ev, out_cam, out_ids):
    eng.vmap_open(voxel)
    series = {"voxel_size": voxel}
    for name, rule, with_a in (("min_neighbours_2", RULE, True), ("min_neighbours_0", dict(RULE, min_neighbours=0), False)):
        ta = [[] for _ in blocks]
        tb = [[] for _ in blocks]
        deltas, entries, keep = [None] * len(blocks), [0] * len(blocks), None
        for rep in range(args.warmup + args.reps):
            eng.vmap_clear()
            for b, blk in enumerate(blocks):
                sl = [slots[i] for i in blk]
                eng.vmap_integrate(sl, updated=False, **kw)
                eng.vmap_observe(sl, rows[blk], **kw)
                eng.vmap_carve(sl, rows[blk], **kw)
                M = eng.vmap_info()["voxels"]
                entries[b] = M
                if with_a:
                    t0 = time.perf_counter()
                    st = eng.vmap_fetch(first=0, count=M, out=out_rec)
                    st.update(eng.vmap_fetch_evidence(first=0, count=M, out=out_ev))
                    offs = eng.vmap_fetch_cameras(first=0, count=M, out=out_cam)["cam_offsets"]
                    keep = host_filter(st, offs, rule)
                    if rep >= args.warmup:
                        ta[b].append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                d = eng.vmap_classify(rule, commit=True, ids=out_ids)
                if rep >= args.warmup:
                    tb[b].append((time.perf_counter() - t0) * 1e3)
                deltas[b] = {f: d[f] for f in ("examined", "accepted", "retracted", "published_total")}
        one = {"ms_b_classify": [round(float(np.median(t)), 4) for t in tb], "deltas": deltas, "entries_M": entries,
               "bytes_b_over_the_link": [4 * (d["accepted"] + d["retracted"]) for d in deltas]}
        if with_a:
            one["ms_a_fetch_all_and_filter"] = [round(float(np.median(t)), 4) for t in ta]
            one["bytes_a_over_the_link"] = [(4 + 8 + 16) * m + 8 * (m + 1) for m in entries]
        else:  # no neighbour test: the flags are (a)'s filter
            M = entries[-1]
            st = eng.vmap_fetch(first=0, count=M, out=out_rec)
            st.update(eng.vmap_fetch_evidence(first=0, count=M, out=out_ev))
            offs = eng.vmap_fetch_cameras(first=0, count=M, out=out_cam)["cam_offsets"]
            one["b_flags_equal_a_filter"] = bool(np.array_equal(eng.vmap_fetch_published().astype(bool), host_filter(st, offs, rule)))
        series[name] = one
    eng.vmap_close()
    return series


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
    doc = {"metric": "classifying the voxel map's entries, online: wall ms per block of 8 keyframes (median; every route ends "
                     "with a stream synchronise), pageable destinations; (a) fetches multiplicity, rho_sigma, both counters and "
                     "the camera-list offsets of all M entries and filters on the host, (b) classifies on the device and returns "
                     "the accepted and retracted ids",
           "reps": args.reps, "warmup": args.warmup, "arch": torch.cuda.get_device_properties(0).gcnArchName}
    doc.update(run(pkg, torch, bench, args))
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    return 0 if all(v["min_neighbours_0"]["b_flags_equal_a_filter"] for v in doc["voxels"]) else 1


if __name__ == "__main__":
    sys.exit(main())
