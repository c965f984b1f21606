#!/usr/bin/env python3
"""What choosing SemiDenseRecon's neighbours costs when the engine derives them from resident ORB observations
(sdm_covisible_neighbours: k_covis_weights + k_covis_select), against the host building the same table through an inverted
index (map point id -> observers) in NumPy, and against sdm_search_priors on the same references.

Keyframes: tools/priors_rate.py's generator (n_kp keypoints each, 60 % of them carrying a map point drawn from a pool of
2 * n_kp shared points, 5 % without an angle).  Measured, per keypoint count (1000, 2000), medians of --reps runs after 3
warm-up runs:
  (a) 64 references x 84 candidates, n = 20: device time (HIP events on the engine's stream around the call: slot lists
      in, two kernels, neighbour lists out) and wall time;
  (b) 1 reference x 8 candidates, n = 7: the online case;
  (c) 512 references x 512 candidates, n = 20 (the 84 keyframes repeated over 512 slots): how the pair count scales;
  (d) the host's inverted index for (a) and (b) (this machine's CPU, one thread), and sdm_search_priors 64 x 20 on the
      neighbours (a) chose.
The kernels' split comes from a run of its own: rocprofv3 --kernel-trace --stats -- python tools/covis_rate.py --reps 10.
The device results are checked equal to the host's.  Writes one JSON object (--out) and prints it.

  python tools/covis_rate.py --out profiles/covis_mi355x.json
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from priors_rate import keyframes, stats  # noqa: E402


def host_neighbours(ids, refs, cands, n, min_weight):
    """the same table on the host: an inverted index map point -> candidate positions, one bincount per reference, a stable
    sort on (-weight, position), the threshold and the single-candidate rule of KeyFrame.cc:348-352"""
    pos = np.concatenate([np.full(int((ids[c] >= 0).sum()), p, np.int32) for p, c in enumerate(cands)])
    mps = np.concatenate([ids[c][ids[c] >= 0] for c in cands])
    order = np.argsort(mps, kind="stable")
    mps, pos = mps[order], pos[order]
    slot_pos = {c: p for p, c in enumerate(cands)}
    nbrs = np.full((len(refs), n), -1, np.int32)
    w_out = np.zeros((len(refs), n), np.int32)
    cnt = np.zeros(len(refs), np.int32)
    cands = np.asarray(cands)
    for a, r in enumerate(refs):
        mine = ids[r][ids[r] >= 0]
        lo = np.searchsorted(mps, mine, "left")
        hi = np.searchsorted(mps, mine, "right")
        take = np.concatenate([pos[l:h] for l, h in zip(lo, hi)]) if len(mine) else np.zeros(0, np.int32)
        w = np.bincount(take, minlength=len(cands))
        if r in slot_pos:
            w[slot_pos[r]] = 0
        rank = np.lexsort((np.arange(len(cands)), -w))
        keep = rank[w[rank] >= min_weight]
        if keep.size == 0 and w.max() >= 1:
            keep = rank[:1]
        keep = keep[:n]
        cnt[a] = keep.size
        nbrs[a, :keep.size] = cands[keep]
        w_out[a, :keep.size] = w[keep]
    return nbrs, w_out, cnt


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
        raise SystemExit("covis_rate measures on the GPU: no device visible")
    stream = torch.cuda.Stream()
    n_kf, big = 84, 512
    res = {"gpu": torch.cuda.get_device_name(0), "cpu": platform.processor() or platform.machine(), "n_kf": n_kf,
           "min_weight": 15, "cases": {"a": [64, 84, 20], "b": [1, 8, 7], "c": [big, big, 20]}, "per_kp": {}}

    def timed(eng, fn):
        dev, wall = [], []
        for i in range(args.reps + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            e1.record(stream)
            e1.synchronize()
            if i >= 3:
                dev.append(e0.elapsed_time(e1))
                wall.append(1e3 * (t1 - t0))
        return {"device": stats(dev), "wall": stats(wall)}

    for n_kp in [int(x) for x in args.kps.split(",")]:
        rng = np.random.default_rng(n_kp)
        kfs = keyframes(rng, n_kf, n_kp)
        eng = pkg.Engine(64, 48, big, max_neighbours=20, stream=stream.cuda_stream)
        slots = list(range(big))
        ids = [kfs[s % n_kf][0] for s in slots]
        for s0 in range(0, big, 64):  # (64 keyframes per packed copy)
            ss = slots[s0:s0 + 64]
            eng.upload_observations_batch(ss, [kfs[s % n_kf][0] for s in ss], [kfs[s % n_kf][1] for s in ss],
                                          [kfs[s % n_kf][2] for s in ss])
        cases = {"a": (list(range(64)), list(range(n_kf)), 20), "b": ([0], list(range(1, 9)), 7), "c": (slots, slots, 20)}
        out = {}
        same = True
        for name, (refs, cands, n) in cases.items():
            got = eng.covisible_neighbours(refs, cands, n, 15)
            want = host_neighbours(ids, refs, cands, n, 15)
            same = same and all(np.array_equal(g, w) for g, w in zip(got, want))
            out["covisible_neighbours_%s_%dx%d_n%d" % (name, len(refs), len(cands), n)] = timed(
                eng, lambda: eng.covisible_neighbours(refs, cands, n, 15))
            out["covisibility_%s_%dx%d" % (name, len(refs), len(cands))] = timed(eng, lambda: eng.covisibility(refs, cands))
        out["device_equals_host"] = bool(same)
        refs, cands, n = cases["a"]
        nbrs, _, cnt = eng.covisible_neighbours(refs, cands, n, 15)
        out["a_references_with_n_neighbours"] = int((cnt == n).sum())
        if (cnt == n).all():
            out["search_priors_64x20"] = timed(eng, lambda: eng.search_priors(refs, nbrs))
        for name in ("a", "b"):
            refs, cands, n = cases[name]
            ts = []
            for _ in range(args.host_reps):
                t0 = time.perf_counter()
                host_neighbours(ids, refs, cands, n, 15)
                ts.append(1e3 * (time.perf_counter() - t0))
            out["host_inverted_index_%s_wall" % name] = stats(ts)
        res["per_kp"][str(n_kp)] = out
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
