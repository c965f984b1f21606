#!/usr/bin/env python3
"""Retiring keyframes from a voxel map: what sdm_vmap_retire costs next to the only route a caller had before it.

Builds tools/vmap_repose_time.py's map: about --entries entries (default 10^6) of --keyframes keyframes, a log of three pairs
per entry.  --retired of the keyframes' tags are then retired, per mode.  Per pass the map is rebuilt (untimed) and one of
two routes retires the tags; wall time, every route ending with a stream synchronise:
  (a) vmap_retire, carry = 0, remap and the four lists to host arrays made once and sized for the map
  (b) the round trip on the same engine: full vmap_fetch and vmap_fetch_observations to the host, the filter in NumPy
      (tests/vmap_retire_np.plan), vmap_clear, vmap_import of the survivors, vmap_import_observations of the pairs that
      stay with dst_ids as entry_map
The routes alternate within a pass; --warmup passes are dropped; median, minimum and maximum of --reps passes are
reported, and for (b) the NumPy share on its own.  Both routes must leave the same records (apart from epoch), ids, log
and lists; the exit code says so.  No threshold is set: nothing here was measured before.
Writes profiles/vmap_retire_mi355x.json and prints it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from vmap_repose_time import RECORD, make_map, rebuild, state  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "vmap_retire_mi355x.json")
NOID = 0xFFFFFFFF
OUTS = ("examined", "dropped", "orphaned", "voxels", "observations_before", "observations", "removed")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=1000000)
    ap.add_argument("--keyframes", type=int, default=200)
    ap.add_argument("--retired", type=int, default=50)
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()

    import torch
    import sdm_pkg
    import vmap_repose_np as vr
    import vmap_retire_np as vt
    pkg = sdm_pkg.load()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    rng = np.random.default_rng(2026)
    rec, _ = make_map(vr, rng, args.entries, args.keyframes)
    eng = pkg.Engine(64, 48, 1)
    eng.vmap_open(args.voxel, len(rec["pixel"]))
    d = eng.vmap_import(rec, updated=False)
    M = eng.vmap_info()["voxels"]
    ent = rng.integers(0, M, 3 * M).astype(np.uint32)
    pairs = {"entry": ent, "tag": rng.integers(0, args.keyframes, 3 * M).astype(np.int32)}
    eng.vmap_import_observations(pairs["entry"], pairs["tag"])
    E = eng.vmap_obs_info()["observations"]
    tags = np.sort(rng.choice(args.keyframes, args.retired, replace=False)).astype(np.int32)[::-1].copy()
    dest = dict(remap=np.empty(M, np.uint32),
                dropped={"dropped_ids": np.empty(M, np.uint32), "dropped_published": np.empty(M, np.uint8)},
                removed={"removed_entry": np.empty(E, np.uint32), "removed_tag": np.empty(E, np.int32)})

    doc = {"metric": "retiring keyframe tags from a voxel map: wall ms per call sequence, every route ending with a stream "
                     "synchronise; (a) sdm_vmap_retire, carry 0, remap and the four lists to host arrays; (b) full fetch to the "
                     "host, the filter in NumPy, clear, import, import_observations on the same engine",
           "reps": args.reps, "warmup": args.warmup, "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "entries_M": int(M), "records_imported": int(d["total"]), "observations_E": int(E), "keyframes": args.keyframes,
           "retired_tags": int(len(tags)), "voxel_size": args.voxel, "modes": {}}
    ok = True
    for mode in ("winner", "unobserved"):
        times = {"a_retire": [], "b_round_trip": [], "b_numpy_share": []}
        ends, outs = {}, {}
        for rep in range(args.warmup + args.reps):
            for route in (("a_retire", "b_round_trip") if rep % 2 == 0 else ("b_round_trip", "a_retire")):
                rebuild(eng, rec, pairs)
                t0 = time.perf_counter()
                if route == "a_retire":
                    outs = eng.vmap_retire(tags, mode=mode, carry=False, **dest)
                    eng.synchronize()
                    t = [(time.perf_counter() - t0) * 1e3]
                else:
                    full = eng.vmap_fetch()
                    log = eng.vmap_fetch_observations()
                    t1 = time.perf_counter()
                    p = vt.plan(full["tag"], log["entry"], log["tag"], tags, mode)
                    surv = p["remap"] != NOID
                    src = {f: full[f][surv] for f in RECORD}
                    le, lt = log["entry"][p["keep"]], log["tag"][p["keep"]]
                    t2 = time.perf_counter()
                    eng.vmap_clear()
                    di = eng.vmap_import(src, dst_ids=True, updated=False)
                    emap = np.full(len(surv), NOID, np.uint32)
                    emap[surv] = di["dst_ids"]
                    eng.vmap_import_observations(le, lt, emap)
                    eng.synchronize()
                    t = [(time.perf_counter() - t0) * 1e3, (t2 - t1) * 1e3]
                if rep >= args.warmup:
                    times[route].append(t[0])
                    if route == "b_round_trip":
                        times["b_numpy_share"].append(t[1])
                if rep == 0:
                    ends[route] = state(eng)
        same = ends["a_retire"] == ends["b_round_trip"]
        ok = ok and same
        res = {"delta": {f: int(outs[f]) for f in OUTS}, "routes_agree": bool(same)}
        for route, t in times.items():
            res["ms_" + route] = {"median": round(float(np.median(t)), 3), "min": round(float(np.min(t)), 3),
                                  "max": round(float(np.max(t)), 3)}
        doc["modes"][mode] = res
    eng.close()
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
