#!/usr/bin/env python3
"""The merged cloud with its camera lists: what sdm_extract_points_voxel_cameras costs next to sdm_extract_points_voxel,
and next to the route it replaces (every support word and the representative array over the link, the union in NumPy).

Builds bench.py's workload for each configuration (default: configs[1], 640x480 x 64 keyframes x 20 neighbours, and
1280x720 x 256 x 7; sigma gate 0.1, source 1), runs one step and, in one process, for each voxel size (default 0.005 and
0.02) and each destination kind (torch device tensors, pageable NumPy) takes the median wall time of --reps calls after
--warmup calls (every call ends with a stream synchronise):
  (a) extract_points_voxel          fields xyz, rho_sigma, multiplicity and source_index
  (b) extract_points_voxel_cameras  the same plus cam_offsets and cam_slots; also with SDM_VOXCAM_PLAIN_OR set (one
      atomicOr per lane and word instead of one per run of equal rank), its result checked equal
  (c) today's route into pageable memory: extract_points_support (no field) + extract_points_voxel(representative=True)
      + tests/voxcam_np.py on this machine's CPU (median of --host-reps), its lists checked equal to (b)'s
Expectation to check, not a gate: (b) into pageable memory takes less wall time than (c).  (b) - (a) is reported next to
extract_points_support's own time minus extract_points'.
Writes profiles/voxel_cameras_mi355x.json and prints it.

  python tools/voxel_cameras_rate.py
  python tools/voxel_cameras_rate.py --only 480p:64:20
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

CONFIGS = ["480p:64:20", "720p:256:7"]
VOXELS = [0.005, 0.02]
OUT = os.path.join(ROOT, "profiles", "voxel_cameras_mi355x.json")
PLAIN_OR = "SDM_VOXCAM_PLAIN_OR"


def wall_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def run(pkg, torch, bench, res, kfs, nbrs, args):
    import voxcam_np
    wl = bench.Workload(pkg, torch, res, kfs, nbrs, 2.6, 1, 0, 0)
    wl.step("allgather", "torch")
    torch.cuda.synchronize()
    eng, slots, ms = wl.eng, list(wl.pl["own_slots"]), args.max_sigma
    rows = np.ascontiguousarray(np.asarray(wl.pl["nbr_slots"], np.int32).reshape(len(slots), -1))
    cap = max(eng.extract_bound(slots), 1)
    cam_cap = cap * (1 + rows.shape[1])

    def buffers(kind, cams):
        if kind == "device":
            out = {"xyz": torch.empty((cap, 3), dtype=torch.float32, device="cuda"),
                   "rho_sigma": torch.empty((cap, 2), dtype=torch.float32, device="cuda"),
                   "multiplicity": torch.empty(cap, dtype=torch.int32, device="cuda"),
                   "source_index": torch.empty(cap, dtype=torch.int32, device="cuda")}
            if cams:
                out.update(cam_offsets=torch.empty(cap + 1, dtype=torch.int64, device="cuda"),
                           cam_slots=torch.empty(cam_cap, dtype=torch.int32, device="cuda"))
        else:
            out = {"xyz": np.empty((cap, 3), np.float32), "rho_sigma": np.empty((cap, 2), np.float32),
                   "multiplicity": np.empty(cap, np.uint32), "source_index": np.empty(cap, np.uint32)}
            if cams:
                out.update(cam_offsets=np.empty(cap + 1, np.int64), cam_slots=np.empty(cam_cap, np.int32))
        return out

    w, r = args.warmup, args.reps
    T = int(eng.extract_points(slots, max_sigma=ms, fields=("pixel",))["offsets"][-1])
    pix, sup = np.empty(cap, np.uint32), np.empty(cap, np.uint64)
    ms_plain = wall_ms(lambda: eng.extract_points(slots, max_sigma=ms, out={"pixel": pix}), w, r)
    ms_sup = wall_ms(lambda: eng.extract_points_support(slots, rows, max_sigma=ms, out={"pixel": pix, "support": sup}), w, r)
    doc = {"workload": bench.workload_name(wl.W, wl.H, kfs, nbrs, res), "keyframes": len(slots), "n_nbr": int(rows.shape[1]),
           "distinct_slots_Cn": int(len(voxcam_np.camera_table(slots, rows))), "max_sigma": ms, "plain_points_T": T,
           "ms_extract_points_support_minus_extract_points_pageable": round(ms_sup - ms_plain, 4), "voxels": []}
    for voxel in args.voxel or VOXELS:
        row = {"voxel_size": voxel}
        for kind in ("device", "pageable"):
            out_a, out_b = buffers(kind, False), buffers(kind, True)
            a = wall_ms(lambda: eng.extract_points_voxel(slots, voxel, max_sigma=ms, out=out_a), w, r)
            b = wall_ms(lambda: eng.extract_points_voxel_cameras(slots, rows, voxel, max_sigma=ms, out=out_b), w, r)
            os.environ[PLAIN_OR] = "1"
            p = wall_ms(lambda: eng.extract_points_voxel_cameras(slots, rows, voxel, max_sigma=ms, out=out_b), w, r)
            del os.environ[PLAIN_OR]
            row["ms_a_extract_points_voxel_" + kind] = round(a, 4)
            row["ms_b_extract_points_voxel_cameras_" + kind] = round(b, 4)
            row["ms_b_plain_atomic_or_" + kind] = round(p, 4)
            row["ms_b_minus_a_" + kind] = round(b - a, 4)
        got = {k: np.array(v) for k, v in eng.extract_points_voxel_cameras(slots, rows, voxel, max_sigma=ms,
                                                                             out=buffers("pageable", True)).items()}
        os.environ[PLAIN_OR] = "1"
        alt = eng.extract_points_voxel_cameras(slots, rows, voxel, max_sigma=ms, out=buffers("pageable", True))
        del os.environ[PLAIN_OR]
        out_c = buffers("pageable", False)
        out_c["representative"] = np.empty(cap, np.uint32)
        host = {}

        def route():
            s = eng.extract_points_support(slots, rows, max_sigma=ms, fields=(), out={"support": sup})
            v = eng.extract_points_voxel(slots, voxel, max_sigma=ms, out=out_c, representative=True)
            host["r"] = (v, voxcam_np.voxel_cameras(s["support"], s["offsets"], slots, rows, v["representative"],
                                                    len(v["source_index"])))

        row["ms_c_host_route"] = round(wall_ms(route, 1, args.host_reps), 2)
        v, (offs, cs) = host["r"]
        M, E = len(v["source_index"]), len(cs)
        row.update(kept_points_M=M, list_entries_E=E, M_over_T=round(M / max(T, 1), 5),
                   mean_cameras_per_kept_point=round(E / max(M, 1), 3),
                   link_bytes_cameras=8 * (M + 1) + 4 * E, link_bytes_host_route=12 * T)
        row["b_equals_c"] = bool(np.array_equal(got["cam_offsets"], offs) and np.array_equal(got["cam_slots"], cs) and
                                 np.array_equal(got["source_index"], v["source_index"]) and
                                 np.array_equal(got["xyz"].view(np.uint32), v["xyz"].view(np.uint32)))
        row["combined_equals_plain_or"] = bool(all(np.array_equal(got[f], np.asarray(alt[f])) for f in
                                                   ("cam_offsets", "cam_slots", "source_index", "multiplicity")))
        row["b_pageable_below_c"] = bool(row["ms_b_extract_points_voxel_cameras_pageable"] < row["ms_c_host_route"])
        doc["voxels"].append(row)
    wl.close()
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", action="append", help="res:keyframes:neighbours (repeatable; default: %s)" % ", ".join(CONFIGS))
    ap.add_argument("--voxel", action="append", type=float, help="voxel size (repeatable; default: 0.005, 0.02)")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--max-sigma", type=float, default=0.1)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()

    import torch
    import bench
    import sdm_pkg
    pkg = sdm_pkg.load()
    runs = []
    for cfg in args.only or CONFIGS:
        res, kfs, nbrs = cfg.split(":")
        runs.append(run(pkg, torch, bench, res, int(kfs), int(nbrs), args))
        print(json.dumps(runs[-1]), flush=True)
    doc = {"metric": "the merged cloud with one camera list per kept point: wall ms per call (median; every call ends with "
                     "a stream synchronise), fields xyz + rho_sigma + multiplicity + source_index; (c) is "
                     "extract_points_support + extract_points_voxel(representative) into pageable memory plus the NumPy "
                     "union on the host",
           "reps": args.reps, "warmup": args.warmup, "host_reps": args.host_reps,
           "arch": torch.cuda.get_device_properties(0).gcnArchName, "runs": runs}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    ok = all(v["b_equals_c"] and v["combined_equals_plain_or"] for r in runs for v in r["voxels"])
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
