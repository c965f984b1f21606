#!/usr/bin/env python3
"""Connected components of the voxel map's entries: what sdm_vmap_components costs.

The workload is tools/vmap_repose_time.py's, as tools/vmap_cast_time.py sets it up: by vmap_import, a map of about --entries
entries (default 10^6 records) seen by --keyframes keyframes.  Each measurement is the wall time of one call ending in a
stream synchronise, destinations on the device:
  c6, c26         connectivity 6 and 26, no filter, label and size
  c26_published   connectivity 26 with require_published, after a committing classify under min_neighbours = --neighbours
  c26_small       connectivity 26 with min_size = --min-size and the list of small members beside label and size
  c26_totals      connectivity 26 with min_size, no destination: the six totals alone
  host_fetch      what the host route cannot avoid before any flood fill: vmap_fetch of xyz and multiplicity and
                  vmap_fetch_published of the whole map into host memory
--warmup passes are dropped; median, minimum and maximum of --reps passes are reported with the returned totals.  Every pass
must return the same bits; the exit code says so.  No device route existed before: no threshold is set.
The find of the linking pass halves its paths.  The plain walk is timed on a variant library:
  python tools/build_variants.py plainwalk=-DSDM_VCOMP_HALVE=false
  SDM_LIB_PATH=.../lib/variants/libsdm_hip_plainwalk.so python tools/vmap_comp_time.py --out profiles/vmap_comp_plainwalk_mi355x.json
Writes profiles/vmap_comp_mi355x.json (or --out) and prints it; "library" names the library that was timed."""
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

OUT = os.path.join(ROOT, "profiles", "vmap_comp_mi355x.json")


def digest(got):
    return hashlib.sha256(b"".join(np.ascontiguousarray(got[f].cpu().numpy() if hasattr(got[f], "cpu") else got[f]).tobytes()
                                   for f in sorted(got) if not isinstance(got[f], int))).hexdigest()


def timed(eng, call, warmup, reps):
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
    return {"outs": outs[0], "passes_agree": bool(same),
            "ms": {"median": round(float(np.median(times)), 3), "min": round(float(np.min(times)), 3),
                   "max": round(float(np.max(times)), 3)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=1000000)
    ap.add_argument("--keyframes", type=int, default=200)
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--min-size", type=int, default=8)
    ap.add_argument("--neighbours", type=int, default=2)
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
    rec, _ = workload.make_map(vr, rng, args.entries, args.keyframes)
    eng = pkg.Engine(64, 48, 1)
    eng.vmap_open(args.voxel, len(rec["pixel"]))
    d = eng.vmap_import(rec, updated=False)
    M = eng.vmap_info()["voxels"]
    dst = {f: torch.empty(M, dtype=torch.int32, device="cuda") for f in ("labels", "sizes", "small_ids")}
    two = dict(labels=dst["labels"], sizes=dst["sizes"], small_ids=False)

    res = {}
    res["c6"] = timed(eng, lambda: eng.vmap_components(connectivity=6, **two), args.warmup, args.reps)
    res["c26"] = timed(eng, lambda: eng.vmap_components(connectivity=26, **two), args.warmup, args.reps)
    res["c26_small"] = timed(eng, lambda: eng.vmap_components(connectivity=26, min_size=args.min_size, **dst), args.warmup, args.reps)
    res["c26_totals"] = timed(eng, lambda: eng.vmap_components(connectivity=26, min_size=args.min_size, labels=False, sizes=False,
                                                               small_ids=False), args.warmup, args.reps)
    host = {"xyz": np.empty((M, 3), np.float32), "multiplicity": np.empty(M, np.uint32)}
    flags = np.empty(M, np.uint8)

    def fetch():
        eng.vmap_fetch(fields=("xyz", "multiplicity"), out=host)
        eng.vmap_fetch_published(out=flags)
        return {"xyz": host["xyz"], "multiplicity": host["multiplicity"], "published": flags, "entries": int(M)}

    res["host_fetch"] = timed(eng, fetch, args.warmup, args.reps)
    pub = eng.vmap_classify(dict(min_neighbours=args.neighbours), True, ids=False)["published_total"]
    res["c26_published"] = timed(eng, lambda: eng.vmap_components(connectivity=26, require_published=True, **two),
                                 args.warmup, args.reps)
    eng.close()
    doc = {"metric": "connected components of a voxel map's entries: wall ms per sdm_vmap_components, destinations on the device, "
                     "each ending with a stream synchronise; host_fetch: the whole map's xyz, multiplicity and flags to host memory",
           "reps": args.reps, "warmup": args.warmup, "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "entries_M": int(M), "records_imported": int(d["total"]), "keyframes": args.keyframes, "voxel_size": args.voxel,
           "min_size": args.min_size, "classify_min_neighbours": args.neighbours, "published": int(pub),
           "library": os.path.basename(os.environ.get("SDM_LIB_PATH") or "libsdm_hip.so")}
    doc.update(res)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    return 0 if all(r["passes_agree"] for r in res.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
