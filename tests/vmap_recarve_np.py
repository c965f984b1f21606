"""NumPy restatement of sdm_vmap_recarve (include/sdm_c.h): the free-space evidence of the persistent voxel map made
again from its observation log.

  pairs   pair k of the range first .. first + count - 1 of the log is (e, t) = (entry[k], tag[k]); a pair whose tag is not
          in the table is UNPOSED and contributes nothing
  rays    one per posed pair: from O, the camera centre of the table's pose of t (carve_np.camera_centre), to P, the xyz of
          record e as it stands
  walk    vmap_carve_np.carve's, unchanged: the posed pairs are handed to it as plain points g with P as their xyz, the
          pair's pose index as their slot, no neighbour table, and the table's centres -- there is no second walker
  count   crossings and ends per entry, added to the counters (reset: after both are put to 0 for every entry)
The map is only read: its keys and ids come from vmap_np.VoxelMap.keys / .ids, or from map_index(record xyz)."""
import numpy as np

import carve_np
import vmap_carve_np as vc
import voxel_np

OUTS = ("pairs_total", "pairs_unposed", "rays_total", "rays_skipped", "cells_visited", "cells_hit", "ends_hit")


def map_index(rec_xyz, voxel_size):
    """(keys int64[M] sorted, ids int64[M]) of a map from its records' xyz (every record lies in its own entry's voxel)"""
    xyz = np.ascontiguousarray(rec_xyz, np.float32).reshape(-1, 3)
    cell, ok = voxel_np.cells(xyz, voxel_size)
    assert ok.all(), "a record of the map is mergeable"
    keys = carve_np.pack(cell)
    order = np.argsort(keys, kind="stable")
    return keys[order], order.astype(np.int64)


def centres_of(Tcw):
    return np.array([carve_np.camera_centre(T) for T in np.asarray(Tcw, np.float32).reshape(-1, 12)], np.float32).reshape(-1, 3)


def accumulate(ev, M, add, reset):
    """the counters {"crossings", "ends"} (any length up to M: entries created later read 0) after a call that adds `add`"""
    out = {}
    for f in ("crossings", "ends"):
        old = np.zeros(M, np.uint64)
        if not reset:
            old[:len(ev[f])] = ev[f]
        out[f] = old + add[f]
    return out


def recarve(map_keys_ids, rec_xyz, log_entry, log_tag, tags, Tcw, voxel_size, end_margin=1, max_steps=4096, first=0,
            count=None):
    """map_keys_ids: (keys int64[M] sorted, ids int64[M]); rec_xyz float32[M, 3]; log_entry uint32[E], log_tag int32[E];
    tags int[n] (distinct), Tcw float32[n, 12]
    -> dict(crossings uint64[M], ends uint64[M]: what the call ADDS, the seven outs, steps int64[rays] (N, or -1 for a
    skipped ray), ray_pair int64[rays]: the log index of each ray)"""
    xyz = np.ascontiguousarray(rec_xyz, np.float32).reshape(-1, 3)
    entry = np.asarray(log_entry, np.int64).reshape(-1)
    ltag = np.asarray(log_tag, np.int64).reshape(-1)
    tags = np.asarray(tags, np.int64).reshape(-1)
    n, E = len(tags), len(entry)
    assert len(set(tags.tolist())) == n and len(ltag) == E
    count = E - first if count is None else count
    assert 0 <= first and 0 <= count and first + count <= E
    k = np.arange(first, first + count)
    pose = np.full(count, -1, np.int64)
    if n:
        order = np.argsort(tags)
        at = np.minimum(np.searchsorted(tags[order], ltag[k]), n - 1)
        pose = np.where(tags[order][at] == ltag[k], order[at], -1)
    posed = pose >= 0
    got = vc.carve(map_keys_ids, xyz[entry[k[posed]]], pose[posed], None, np.arange(n), None, centres_of(Tcw), voxel_size,
                   end_margin, max_steps)
    assert got["rays_total"] == int(posed.sum()) and (got["ray_g"] == np.arange(got["rays_total"])).all()
    out = {f: got[f] for f in ("crossings", "ends", "rays_total", "rays_skipped", "cells_visited", "cells_hit", "ends_hit", "steps")}
    out.update(pairs_total=int(count), pairs_unposed=int(count - posed.sum()), ray_pair=k[posed])
    return out
