#!/usr/bin/env python3
"""The triangle mesh of the voxel map: what sdm_vmap_mesh costs.

The workload is tools/vmap_normals_time.py's: by vmap_import, a map of about --entries entries (default 10^6 records) seen by
--keyframes keyframes at --voxel, and its normals at radius 2 turned towards every keyframe's pose, left on the device.  Each
measurement is the wall time of one call ending in a stream synchronise, normals and destinations on the device:
  mesh                the whole map: triangles, owner_tris and vertex_used, the list sized by a call for the totals before
  totals              the same call without a destination: everything up to the first wait
  normals_and_mesh    sdm_vmap_normals at radius 2 with the pose table, then sdm_vmap_mesh: what an update costs
  host_fetch          what the host route cannot avoid: vmap_fetch of xyz and multiplicity, vmap_fetch_published, and the
                      normals copied to host memory
  host_restatement    tests/vmap_mesh_np.py (NumPy, vectorised over the owners) on the fetched records and normals, one pass
--warmup passes are dropped; median, minimum and maximum of --reps passes are reported with the returned totals.  Every pass
must return the same bits, and the restatement's bits are the device's on the full map; the exit code says so.  No device
route existed before: no threshold is set.
Writes profiles/vmap_mesh_mi355x.json (or --out) and prints it; "library" names the library that was timed."""
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

OUT = os.path.join(ROOT, "profiles", "vmap_mesh_mi355x.json")
ARRAYS = ("tri", "owner_tris", "vertex_used")


def digest(got):
    h = hashlib.sha256()
    for f in ARRAYS:
        if f in got:
            a = got[f].cpu().numpy() if hasattr(got[f], "cpu") else got[f]
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


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
    ap.add_argument("--no-restatement", action="store_true", help="skip the NumPy route")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()

    import torch
    import sdm_pkg
    import vmap_mesh_np as vm
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
    normal = torch.empty((M, 3), dtype=torch.float32, device="cuda")
    nkw = dict(radius=2, min_points=args.min_points, normals=normal, variations=False, counts=False)
    eng.vmap_normals(tags, Tcw, **nkw)
    T = eng.vmap_mesh(normal, tri=False, owner_tris=False, vertex_used=False)["triangles"]
    dst = dict(tri=torch.empty((max(T, 1), 3), dtype=torch.int32, device="cuda"),
               owner_tris=torch.empty(M, dtype=torch.uint8, device="cuda"), vertex_used=torch.empty(M, dtype=torch.uint8, device="cuda"))

    def update():
        eng.vmap_normals(tags, Tcw, **nkw)
        return eng.vmap_mesh(normal, **dst)

    res = {"mesh": timed(eng, lambda: eng.vmap_mesh(normal, **dst), args.warmup, args.reps),
           "totals": timed(eng, lambda: eng.vmap_mesh(normal, tri=False, owner_tris=False, vertex_used=False), args.warmup, args.reps),
           "normals_and_mesh": timed(eng, update, args.warmup, args.reps)}
    host = {"xyz": np.empty((M, 3), np.float32), "multiplicity": np.empty(M, np.uint32)}
    flags = np.empty(M, np.uint8)
    host_normal = torch.empty((M, 3), dtype=torch.float32).pin_memory()

    def fetch():
        eng.vmap_fetch(fields=("xyz", "multiplicity"), out=host)
        eng.vmap_fetch_published(out=flags)
        host_normal.copy_(normal)
        torch.cuda.synchronize()
        return {"entries": int(M)}

    res["host_fetch"] = timed(eng, fetch, args.warmup, args.reps)
    res["host_fetch"].pop("sha256")
    ok = all(r["passes_agree"] for r in res.values()) and res["mesh"]["outs"] == res["totals"]["outs"]
    if not args.no_restatement:
        t0 = time.perf_counter()
        exp = vm.mesh(host, None, args.voxel, host_normal.numpy())
        ms = (time.perf_counter() - t0) * 1e3
        same = digest(exp) == res["mesh"]["sha256"] and {f: exp[f] for f in vm.OUTS} == res["mesh"]["outs"]
        res["host_restatement"] = {"ms": round(ms, 1), "equals_device": bool(same), "stats": exp["stats"]}
        ok = ok and same
    eng.close()
    doc = {"metric": "triangle mesh of a voxel map: wall ms per sdm_vmap_mesh over the whole map, normals and destinations on the "
                     "device, each ending with a stream synchronise; host_fetch: the whole map's xyz, multiplicity, flags and "
                     "normals to host memory; host_restatement: the NumPy restatement on them, one pass",
           "reps": args.reps, "warmup": args.warmup, "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "entries_M": int(M), "records_imported": int(d["total"]), "keyframes": args.keyframes, "voxel_size": args.voxel,
           "normals": {"radius": 2, "min_points": args.min_points, "oriented_by": "every keyframe's pose"},
           "library": os.path.basename(os.environ.get("SDM_LIB_PATH") or "libsdm_hip.so")}
    doc.update(res)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
