"""Worker for tests/test_gpu_vmap_import.py: one rank of a sharded voxel map.  Launched by torch.distributed.run with every
rank on GPU 0 and a gloo group.  Every rank runs the golden fixture through the pipeline, integrates and observes only the
keyframes of its block into its own map, and then calls shard.vmap_allgather_merge; it saves its merged map, log size and
camera lists.

usage: vmap_merge_worker.py OUT_DIR FIXTURE VOXEL_SIZE"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import golden_util as gu  # noqa: E402
import sdm_pkg  # noqa: E402


def main():
    out_dir, name, voxel = sys.argv[1], sys.argv[2], float(sys.argv[3])
    pkg = sdm_pkg.load()
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    g = gu.load(name)
    n = g["n_kf"]
    eng = pkg.Engine(g["W"], g["H"], n, max_neighbours=g["n"])
    for k in range(n):
        eng.upload_image(k, g["im"][k], g["K"], g["Tcw"][k])
    refs = list(range(n))
    lo, hi = float(g["min_depth"]), float(g["max_depth"])
    eng.search_fuse(refs, g["nbrs"], lo, hi, rot=gu.rots(g))
    eng.recon(refs, g["nbrs"], lo, hi, rot=gu.rots(g))
    eng.inter_check(refs, g["nbrs"])
    eng.pointset(refs, source=1)
    eng.vmap_open(voxel)
    for k in range((n * rank) // world, (n * (rank + 1)) // world):  # this rank's block
        eng.vmap_integrate([k], max_sigma=0.3)
        eng.vmap_observe([k], g["nbrs"][[k]], max_sigma=0.3)
    before = eng.vmap_info()["voxels"]
    merged = pkg.shard.vmap_allgather_merge(eng)
    assert [m["rank"] for m in merged] == [r for r in range(world) if r != rank]
    out = dict(eng.vmap_fetch())
    out.update(eng.vmap_fetch_cameras())
    out["before"] = np.array([before])
    out["points"] = np.array([eng.vmap_info()["points"]])
    out["observations"] = np.array([eng.vmap_obs_info()["observations"]])
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
    dist.barrier()
    eng.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
