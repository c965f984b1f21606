#!/usr/bin/env python3
"""What SemiDenseRecon's search priors cost when the engine derives them from resident ORB observations
(sdm_upload_observations_batch + sdm_search_priors), against the host helpers the class used to call once per pair
(sdm_median_rot_in_plane, sdm_stereo_search_constraints) on the same data.

Keyframes: n_kp keypoints each, 60 % of them carrying a map point drawn from a pool of 2 * n_kp shared points, 5 % without
an angle, 0.6 * n_kp point depths.  Measured, per keypoint count (1000: TUM / EuRoC / 720p configs, 2000: KITTI):
  - device time (HIP events on the engine's stream around the call: slot tables in, kernel, priors out) of one
    sdm_search_priors for 64 references x 20 neighbours;
  - wall time of upload_observations_batch (84 keyframes) + search_priors (64 x 20);
  - wall time of one online keyframe: upload_observations_batch (1 + 7 keyframes) + search_priors (1 x 7);
  - wall time of the host helpers over the same 64 x 20 block and the same keyframe (this machine's CPU, one thread).
The device results are checked equal to the host helpers'.  Writes one JSON object (--out) and prints it.

  python tools/priors_rate.py --out profiles/priors_mi355x.json
"""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def keyframes(rng, n_kf, n_kp):
    out = []
    for _ in range(n_kf):
        ids = rng.choice(2 * n_kp, n_kp, replace=False).astype(np.int32)
        ids[rng.uniform(0, 1, n_kp) >= 0.6] = -1
        ang = rng.uniform(0.0, 360.0, n_kp).astype(np.float32)
        ang[rng.uniform(0, 1, n_kp) < 0.05] = -1.0
        dep = rng.uniform(0.5, 3.0, int((ids >= 0).sum())).astype(np.float32)
        out.append((ids, ang, dep))
    return out


def stats(xs):
    xs = sorted(xs)
    return {"median_ms": round(xs[len(xs) // 2], 4), "min_ms": round(xs[0], 4), "max_ms": round(xs[-1], 4), "runs": len(xs)}


def host_priors(binding, kfs, refs, nbrs):
    rot = np.empty(nbrs.shape, np.float32)
    mn = np.empty(len(refs), np.float32)
    mx = np.empty(len(refs), np.float32)
    for a, r in enumerate(refs):
        mn[a], mx[a] = binding.stereo_search_constraints(kfs[r][2])
        for j, s in enumerate(nbrs[a]):
            rot[a, j] = binding.median_rot_in_plane(kfs[r][0], kfs[r][1], kfs[s][0], kfs[s][1])
    return rot, mn, mx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kps", default="1000,2000")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import sdm_pkg
    pkg = sdm_pkg.load()
    lib = pkg.load_library()
    if lib.sdm_device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("priors_rate measures on the GPU: no device visible")
    stream = torch.cuda.Stream()
    n_kf, n_ref, n = 84, 64, 20
    res = {"gpu": torch.cuda.get_device_name(0), "cpu": platform.processor() or platform.machine(), "n_kf": n_kf,
           "block": [n_ref, n], "online": [1, 7], "per_kp": {}}
    for n_kp in [int(x) for x in args.kps.split(",")]:
        rng = np.random.default_rng(n_kp)
        kfs = keyframes(rng, n_kf, n_kp)
        eng = pkg.Engine(64, 48, n_kf, max_neighbours=n, stream=stream.cuda_stream)
        refs = np.arange(n_ref, dtype=np.int32)
        nbrs = np.array([[(r + 1 + j) % n_kf for j in range(n)] for r in refs], np.int32)
        slots = list(range(n_kf))
        up = lambda ss: eng.upload_observations_batch(ss, [kfs[s][0] for s in ss], [kfs[s][1] for s in ss],
                                                      [kfs[s][2] for s in ss])
        up(slots)
        rot, mn, mx = eng.search_priors(refs, nbrs)
        h_rot, h_mn, h_mx = host_priors(pkg.binding, kfs, refs, nbrs)
        same = bool((rot == h_rot).all() and (mn.view(np.uint32) == h_mn.view(np.uint32)).all()
                    and (mx.view(np.uint32) == h_mx.view(np.uint32)).all())
        # device time of one 64 x 20 search_priors
        dev = []
        for i in range(args.reps + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            eng.search_priors(refs, nbrs)
            e1.record(stream)
            e1.synchronize()
            if i >= 3:
                dev.append(e0.elapsed_time(e1))
        # wall: 84-keyframe upload + 64 x 20 priors; one keyframe with 7 neighbours
        wall_block, wall_up, wall_one = [], [], []
        one_nbrs = np.array([[1, 2, 3, 4, 5, 6, 7]], np.int32)
        for i in range(args.reps + 3):
            t0 = time.perf_counter()
            up(slots)
            t1 = time.perf_counter()
            eng.search_priors(refs, nbrs)
            t2 = time.perf_counter()
            up(list(range(8)))
            eng.search_priors([0], one_nbrs)
            t3 = time.perf_counter()
            if i >= 3:
                wall_block.append(1e3 * (t2 - t0))
                wall_up.append(1e3 * (t1 - t0))
                wall_one.append(1e3 * (t3 - t2))
        host_block, host_one = [], []
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            host_priors(pkg.binding, kfs, refs, nbrs)
            t1 = time.perf_counter()
            host_priors(pkg.binding, kfs, [0], one_nbrs)
            t2 = time.perf_counter()
            host_block.append(1e3 * (t1 - t0))
            host_one.append(1e3 * (t2 - t1))
        res["per_kp"][str(n_kp)] = {
            "device_equals_host_helpers": same,
            "search_priors_64x20_device": stats(dev),
            "upload_84kf_plus_search_priors_64x20_wall": stats(wall_block),
            "upload_84kf_wall": stats(wall_up),
            "online_1x7_upload_plus_priors_wall": stats(wall_one),
            "host_helpers_64x20_wall": stats(host_block),
            "host_helpers_1x7_wall": stats(host_one),
        }
        eng.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
