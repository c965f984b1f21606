#!/usr/bin/env python3
"""Per-entry surface normals of the voxel map: what sdm_vmap_normals costs.

The workload is tools/vmap_repose_time.py's, as tools/vmap_comp_time.py sets it up: by vmap_import, a map of about --entries
entries (default 10^6 records) seen by --keyframes keyframes, each record carrying its keyframe's tag.  Each measurement is the
wall time of one call ending in a stream synchronise, the three destinations on the device:
  r1, r2              radius 1 and 2 over the whole map, no pose table
  r1_poses, r2_poses  the same with the table of every keyframe's pose: every estimated entry is oriented
  host_fetch          what the host route cannot avoid before any PCA: vmap_fetch of xyz, multiplicity and tag and
                      vmap_fetch_published of the whole map into host memory
  host_restatement    tests/vmap_normals_np.py (NumPy, vectorised over the entries) on the fetched records: radius 1 and 2 with
                      the table, one pass each
--warmup passes are dropped; median, minimum and maximum of --reps passes are reported with the returned totals.  Every pass
must return the same bits, and the restatement's bits are the device's; the exit code says so.  No device route existed
before: no threshold is set.
Writes profiles/vmap_normals_mi355x.json (or --out) and prints it; "library" names the library that was timed."""
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

OUT = os.path.join(ROOT, "profiles", "vmap_normals_mi355x.json")
ARRAYS = ("normal", "variation", "points")


def digest(got):
    return hashlib.sha256(b"".join(np.ascontiguousarray(got[f].cpu().numpy() if hasattr(got[f], "cpu") else got[f]).tobytes()
                                   for f in ARRAYS if f in got)).hexdigest()


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
    return {"outs": outs[0], "passes_agree": bool(same), "sha256": sums[0],
            "ms": {"median": round(float(np.median(times)), 3), "min": round(float(np.min(times)), 3),
                   "max": round(float(np.max(times)), 3)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=1000000)
    ap.add_argument("--keyframes", type=int, default=200)
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--min-points", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-restatement", action="store_true", help="skip the NumPy route (minutes at 10^6 records)")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()

    import torch
    import sdm_pkg
    import vmap_normals_np as vn
    import vmap_repose_np as vr
    import vmap_repose_time as workload
    pkg = sdm_pkg.load()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    rng = np.random.default_rng(2026)
    rec, poses = workload.make_map(vr, rng, args.entries, args.keyframes)
    tags = np.arange(args.keyframes, dtype=np.int32)
    Tcw = np.ascontiguousarray(poses, np.float32).reshape(-1, 12)
    eng = pkg.Engine(64, 48, 1)
    eng.vmap_open(args.voxel, len(rec["pixel"]))
    d = eng.vmap_import(rec, updated=False)
    M = eng.vmap_info()["voxels"]
    dst = dict(normals=torch.empty((M, 3), dtype=torch.float32, device="cuda"),
               variations=torch.empty(M, dtype=torch.float32, device="cuda"), counts=torch.empty(M, dtype=torch.int32, device="cuda"))
    kw = dict(min_points=args.min_points, **dst)

    res = {}
    for r in (1, 2):
        res["r%d" % r] = timed(eng, lambda: eng.vmap_normals(radius=r, **kw), args.warmup, args.reps)
        res["r%d_poses" % r] = timed(eng, lambda: eng.vmap_normals(tags, Tcw, radius=r, **kw), args.warmup, args.reps)
    host = {"xyz": np.empty((M, 3), np.float32), "multiplicity": np.empty(M, np.uint32), "tag": np.empty(M, np.int32)}
    flags = np.empty(M, np.uint8)

    def fetch():
        eng.vmap_fetch(fields=("xyz", "multiplicity", "tag"), out=host)
        eng.vmap_fetch_published(out=flags)
        return {"entries": int(M)}

    res["host_fetch"] = timed(eng, fetch, args.warmup, args.reps)
    res["host_fetch"].pop("sha256")
    ok = all(r["passes_agree"] for r in res.values())
    if not args.no_restatement:
        res["host_restatement"] = {}
        for r in (1, 2):
            t0 = time.perf_counter()
            exp = vn.normals(host, None, args.voxel, tags, Tcw, radius=r, min_points=args.min_points)
            ms = (time.perf_counter() - t0) * 1e3
            same = digest(exp) == res["r%d_poses" % r]["sha256"] and \
                {f: exp[f] for f in vn.OUTS} == res["r%d_poses" % r]["outs"]
            res["host_restatement"]["r%d_poses" % r] = {"ms": round(ms, 1), "equals_device": bool(same)}
            ok = ok and same
    eng.close()
    doc = {"metric": "per-entry surface normals of a voxel map: wall ms per sdm_vmap_normals over the whole map, destinations on the "
                     "device, each ending with a stream synchronise; host_fetch: the whole map's xyz, multiplicity, tag and flags to "
                     "host memory; host_restatement: the NumPy restatement on them, one pass",
           "reps": args.reps, "warmup": args.warmup, "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "entries_M": int(M), "records_imported": int(d["total"]), "keyframes": args.keyframes, "voxel_size": args.voxel,
           "min_points": args.min_points, "library": os.path.basename(os.environ.get("SDM_LIB_PATH") or "libsdm_hip.so")}
    doc.update(res)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
