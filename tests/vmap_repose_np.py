"""NumPy restatement of sdm_vmap_repose (include/sdm_c.h): re-placing a persistent voxel map under new keyframe poses.
Built on the mirrors of the calls it is defined by -- vmap_np.VoxelMap, vmap_import_np.import_records /
import_observations, vmap_obs_np.ObservationLog -- and on np_pointset_pixel of tests/test_oracle_crosscheck.py, the
float32 statement of UpdateSemiDensePointSet's one pixel.

  new xyz   entry i whose tag is tags[p]: np_pointset_pixel(K[p], Tcw[p], pixel & 0xffff, pixel >> 16, rho) -- float32
            operations in the device's order, (double)rho < 1e-6 -> (0, 0, 0); any other entry keeps its bits
  re-bin    the old entries i = 0 .. M-1, at their new xyz and with m = their multiplicity, imported in increasing i into
            an empty map of the same voxel size; the surviving record keeps its OLD epoch; remap = the import's dst_ids
  info      calls += 1; points and dropped stay
  log       the old log, in log order, imported through remap into an empty log; the log's calls stay
  carry     0: counters and flags restart at 0; 1: 64-bit sums (wrapping) and the OR over the old entries mapped to each

pointset_pixels is np_pointset_pixel over arrays (the same operations in the same order; tests/test_vmap_repose_cpu.py
holds the two against each other bit for bit)."""
import numpy as np

import vmap_import_np as vi
import vmap_np
import vmap_obs_np as vo
import voxel_np

f32 = np.float32
NOID = vi.NOID
DELTA = ("examined", "reposed", "moved", "dropped", "merged", "voxels", "observations_before", "observations")


def pointset_pixels(K, Tcw, x, y, inv_d):
    """np_pointset_pixel for arrays x, y, inv_d -> float32[n, 3]"""
    K = np.asarray(K, f32).reshape(4)
    T = np.asarray(Tcw, f32).reshape(3, 4)
    fx, fy, cx, cy = K
    inv_d = np.asarray(inv_d, f32).reshape(-1)
    x = np.asarray(x).reshape(-1).astype(f32)
    y = np.asarray(y).reshape(-1).astype(f32)
    with np.errstate(all="ignore"):
        Rwc = T[:, :3].T.copy()
        t = T[:, 3]
        Ow = np.array([(Rwc[i, 0] * t[0] + Rwc[i, 1] * t[1]) + Rwc[i, 2] * t[2] for i in range(3)], f32)
        Z = f32(1) / inv_d
        X = Z * (x - cx) / fx
        Y = Z * (y - cy) / fy
        out = np.stack([((Rwc[i, 0] * X + Rwc[i, 1] * Y) + Rwc[i, 2] * Z) + (-Ow[i]) * f32(1) for i in range(3)], axis=1)
    out = out.astype(f32)
    out[inv_d.astype(np.float64) < 0.000001] = 0
    return out


def new_xyz(rec, tags, K, Tcw):
    """(xyz float32[M, 3], hit bool[M]): the entries' xyz under the pose table, and which entries the table names"""
    tags = np.asarray([] if tags is None else tags, np.int64).reshape(-1)
    assert len(set(tags.tolist())) == len(tags) and (tags >= 0).all() and (tags < (1 << 31)).all()
    xyz = np.array(rec["xyz"], f32).reshape(-1, 3)
    hit = np.zeros(len(xyz), bool)
    if len(tags):
        K = np.asarray(K, f32).reshape(-1, 4)
        Tcw = np.asarray(Tcw, f32).reshape(-1, 12)
        assert len(K) == len(tags) == len(Tcw)
    pixel = np.asarray(rec["pixel"], np.uint32)
    for p, t in enumerate(tags):
        sel = np.flatnonzero(np.asarray(rec["tag"]) == t)
        if len(sel):
            hit[sel] = True
            xyz[sel] = pointset_pixels(K[p], Tcw[p], pixel[sel] & 0xffff, pixel[sel] >> 16, rec["rho_sigma"][sel, 0])
    return xyz, hit


def repose(vm, ol, tags, K, Tcw, carry=False, ev=None, flags=None):
    """Re-places the vmap_np.VoxelMap `vm` and the vmap_obs_np.ObservationLog `ol` (or None) in place.  ev: {"crossings",
    "ends"} uint64[M] or None; flags: uint8[M] or None.  Returns (delta, ev, flags): the delta {"examined", "reposed",
    "moved", "dropped", "merged", "voxels", "observations_before", "observations", "remap"} and the new counters and
    flags (None where None came in)."""
    M = vm.M
    old = {f: vm.rec[f] for f in vmap_np.FIELDS}
    xyz, hit = new_xyz(old, tags, K, Tcw)
    moved = hit & (xyz.view(np.uint32) != np.ascontiguousarray(old["xyz"], f32).reshape(-1, 3).view(np.uint32)).any(axis=1)
    fresh = vmap_np.VoxelMap(vm.voxel_size)
    src = {f: old[f] for f in ("pixel", "rho_sigma", "intensity", "tag", "multiplicity")}
    src["xyz"] = xyz
    d = vi.import_records(fresh, src)
    remap = d["dst_ids"]
    # the epoch rule: each new entry's winner is the old entry with the smallest (key(sigma), old id) among those mapped to it
    surv = np.flatnonzero(remap != NOID)
    if len(surv):
        skey = voxel_np.sigma_key(old["rho_sigma"][surv, 1]).astype(np.uint64)
        o = np.lexsort((surv, skey, remap[surv]))
        e_sorted, i_sorted = remap[surv][o], surv[o]
        first = np.append(True, e_sorted[1:] != e_sorted[:-1])
        win = i_sorted[first]
        assert (e_sorted[first] == np.arange(fresh.M)).all()
        for f in ("pixel", "tag", "intensity"):  # (the import picked the same winners)
            assert (fresh.rec[f] == old[f][win]).all(), f
        fresh.rec["epoch"] = old["epoch"][win].astype(np.uint32)
    vm.rec, vm.keys, vm.ids = fresh.rec, fresh.keys, fresh.ids
    vm.calls += 1
    E0 = 0 if ol is None else ol.E
    if ol is not None and ol.E:
        nl = vo.ObservationLog()
        vi.import_observations(nl, vm.M, ol.entry, ol.tag, remap)
        ol.entry, ol.tag, ol.pairs = nl.entry, nl.tag, nl.pairs
    M2 = vm.M
    ev2 = flags2 = None
    if ev is not None:
        ev2 = {f: np.zeros(M2, np.uint64) for f in ev}
        if carry:
            for f in ev:
                np.add.at(ev2[f], remap[surv].astype(np.int64), np.asarray(ev[f], np.uint64)[surv])
    if flags is not None:
        flags2 = np.zeros(M2, np.uint8)
        if carry:
            np.maximum.at(flags2, remap[surv].astype(np.int64), (np.asarray(flags)[surv] != 0).astype(np.uint8))
    delta = {"examined": M, "reposed": int(hit.sum()), "moved": int(moved.sum()), "dropped": d["dropped"],
             "merged": M - d["dropped"] - M2, "voxels": M2, "observations_before": E0,
             "observations": 0 if ol is None else ol.E, "remap": remap}
    return delta, ev2, flags2
