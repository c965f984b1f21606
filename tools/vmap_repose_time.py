#!/usr/bin/env python3
"""Re-placing a voxel map under adjusted poses: what sdm_vmap_repose costs next to the only route a caller had before it.

Builds, by vmap_import and vmap_import_observations, a map of about --entries entries (default 10^6) seen by --keyframes
keyframes and a log of three pairs per entry: every entry's xyz is its pixel and rho under its keyframe's pose, so the map
is one a pipeline could have made.  --adjusted of the keyframes then get a slightly different pose.  Per pass the map is
rebuilt (untimed) and one of two routes re-places it; wall time, every route ending with a stream synchronise:
  (a) vmap_repose with the adjusted keyframes' table, remap to a host array, carry = 0
  (b) the round trip on the same engine: full vmap_fetch and vmap_fetch_observations to the host, the new xyz in NumPy
      (tests/vmap_repose_np.new_xyz), vmap_clear, vmap_import, vmap_import_observations with dst_ids as entry_map
The routes alternate within a pass; --warmup passes are dropped; median, minimum and maximum of --reps passes are
reported, and for (b) the NumPy share on its own.  Both routes must leave the same records (apart from epoch), ids, log
and lists; the exit code says so.  No threshold is set: nothing here was measured before.
Writes profiles/vmap_repose_mi355x.json and prints it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUT = os.path.join(ROOT, "profiles", "vmap_repose_mi355x.json")
RECORD = ("xyz", "pixel", "rho_sigma", "intensity", "tag", "multiplicity")
F = np.float32
W, H = 640, 480
K_CAM = np.array([520.0, 520.0, 319.5, 239.5], F)


def pose(rng, k, jitter=0.0):
    """keyframe k of a camera walking along x and turning slowly; jitter: the adjustment"""
    ry = 0.01 * k + jitter * rng.normal()
    rx = jitter * rng.normal()
    cx, sx, cy, sy = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry)
    R = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    t = -R @ (np.array([0.05 * k, 0, 0]) + jitter * rng.normal(size=3))
    return np.concatenate([R, t.reshape(3, 1)], axis=1).astype(F).reshape(12)


def make_map(vr, rng, entries, keyframes):
    per = entries // keyframes
    n = per * keyframes
    tag = np.repeat(np.arange(keyframes, dtype=np.int32), per)
    pixel = (rng.integers(2, W - 2, n) | (rng.integers(2, H - 2, n) << 16)).astype(np.uint32)
    rho = rng.uniform(0.2, 1.0, n).astype(F)
    rec = {"pixel": pixel, "rho_sigma": np.stack([rho, rng.uniform(0.005, 0.1, n).astype(F)], axis=1),
           "intensity": rng.integers(0, 256, n).astype(np.uint8), "tag": tag, "multiplicity": rng.integers(1, 5, n).astype(np.uint32),
           "xyz": np.zeros((n, 3), F)}
    poses = np.array([pose(rng, k) for k in range(keyframes)], F)
    Ks = np.tile(K_CAM, (keyframes, 1))
    rec["xyz"], _ = vr.new_xyz(rec, np.arange(keyframes), Ks, poses)
    return rec, poses


def rebuild(eng, rec, pairs):
    eng.vmap_clear()
    eng.vmap_import(rec, dst_ids=False, updated=False)
    eng.vmap_import_observations(pairs["entry"], pairs["tag"])
    eng.synchronize()


def state(eng):
    full = eng.vmap_fetch(fields=RECORD)
    log = eng.vmap_fetch_observations()
    cams = eng.vmap_fetch_cameras()
    return [full[f].tobytes() for f in RECORD] + [log[f].tobytes() for f in ("entry", "tag")] + \
        [np.asarray(cams[f]).tobytes() for f in ("cam_offsets", "cam_tags")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=1000000)
    ap.add_argument("--keyframes", type=int, default=200)
    ap.add_argument("--adjusted", type=int, default=50)
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()

    import torch
    import sdm_pkg
    import vmap_repose_np as vr
    pkg = sdm_pkg.load()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    rng = np.random.default_rng(2026)
    rec, poses = make_map(vr, rng, args.entries, args.keyframes)
    eng = pkg.Engine(64, 48, 1)
    eng.vmap_open(args.voxel, len(rec["pixel"]))
    d = eng.vmap_import(rec, updated=False)
    M = eng.vmap_info()["voxels"]
    ent = rng.integers(0, M, 3 * M).astype(np.uint32)
    pairs = {"entry": ent, "tag": rng.integers(0, args.keyframes, 3 * M).astype(np.int32)}
    eng.vmap_import_observations(pairs["entry"], pairs["tag"])
    E = eng.vmap_obs_info()["observations"]
    adj = np.sort(rng.choice(args.keyframes, args.adjusted, replace=False)).astype(np.int32)[::-1].copy()
    Ka = np.tile(K_CAM, (len(adj), 1))
    Ta = np.array([pose(rng, int(k), 0.002) for k in adj], F)

    times = {"a_repose": [], "b_round_trip": [], "b_numpy_share": []}
    ends, outs = {}, {}
    for rep in range(args.warmup + args.reps):
        for route in (("a_repose", "b_round_trip") if rep % 2 == 0 else ("b_round_trip", "a_repose")):
            rebuild(eng, rec, pairs)
            t0 = time.perf_counter()
            if route == "a_repose":
                outs = eng.vmap_repose(adj, Ka, Ta, carry=False, remap=True)
                eng.synchronize()
                t = [(time.perf_counter() - t0) * 1e3]
            else:
                full = eng.vmap_fetch()
                log = eng.vmap_fetch_observations()
                t1 = time.perf_counter()
                full["xyz"], _ = vr.new_xyz(full, adj, Ka, Ta)
                t2 = time.perf_counter()
                eng.vmap_clear()
                di = eng.vmap_import({f: full[f] for f in RECORD}, dst_ids=True, updated=False)
                eng.vmap_import_observations(log["entry"], log["tag"], di["dst_ids"])
                eng.synchronize()
                t = [(time.perf_counter() - t0) * 1e3, (t2 - t1) * 1e3]
            if rep >= args.warmup:
                times[route].append(t[0])
                if route == "b_round_trip":
                    times["b_numpy_share"].append(t[1])
            if rep == 0:
                ends[route] = state(eng)
    same = ends["a_repose"] == ends["b_round_trip"]
    eng.close()
    doc = {"metric": "re-placing a voxel map under adjusted poses: wall ms per call sequence, every route ending with a stream "
                     "synchronise; (a) sdm_vmap_repose, remap to a host array, carry 0; (b) full fetch to the host, new xyz in "
                     "NumPy, clear, import, import_observations on the same engine",
           "reps": args.reps, "warmup": args.warmup, "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "entries_M": int(M), "records_imported": int(d["total"]), "observations_E": int(E), "keyframes": args.keyframes,
           "adjusted_keyframes": int(len(adj)), "voxel_size": args.voxel,
           "delta": {f: int(outs[f]) for f in ("examined", "reposed", "moved", "dropped", "merged", "voxels", "observations")},
           "routes_agree": bool(same)}
    for route, t in times.items():
        doc["ms_" + route] = {"median": round(float(np.median(t)), 3), "min": round(float(np.min(t)), 3),
                              "max": round(float(np.max(t)), 3)}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
