"""NumPy restatement of sdm_vmap_import and sdm_vmap_import_observations (include/sdm_c.h): merging externally supplied
records, and the (entry, tag) pairs that go with them, into a persistent voxel map and its observation log.  Both work on
the mirrors of the calls they extend -- vmap_np.VoxelMap and vmap_obs_np.ObservationLog -- and change them in place.

  records  {"xyz", "rho_sigma"} required; "pixel", "intensity", "tag" default to 0, "multiplicity" to 1, "epoch" is ignored.
           Processing r = 0 .. R-1 in order: a record that is unmergeable (voxel_np's cells, the DESTINATION's voxel size)
           or has multiplicity 0 is dropped; a record of a voxel without an entry appends entry id = M with its bits, its
           multiplicity and epoch c; any other adds its multiplicity (saturating at 2^32 - 1) and replaces the record iff
           its key is STRICTLY below the stored one (epoch c).  c counts integrates and imports alike.
  pairs    k = 0 .. P-1 in order: the entry is entry[k], or entry_map[entry[k]] (entry[k] >= len(entry_map): rejected); an
           entry >= M or a tag < 0 is rejected; a pair not yet stored is appended at index E.
Done per call with one sort instead of a loop, as vmap_np.integrate and vmap_obs_np.observe are."""
import numpy as np

import vmap_np
import voxel_np

SAT = vmap_np.SAT
NOID = 0xFFFFFFFF
DELTA = ("total", "dropped", "first_created", "created", "updated")
OBS_DELTA = ("total", "rejected", "first_created", "created")


def sources(records):
    """the six source arrays of `records` with the defaults filled in"""
    xyz = np.ascontiguousarray(records["xyz"], np.float32).reshape(-1, 3)
    R = len(xyz)
    src = {"xyz": xyz, "rho_sigma": np.ascontiguousarray(records["rho_sigma"], np.float32).reshape(-1, 2)}
    for f, dt in (("pixel", np.uint32), ("intensity", np.uint8), ("tag", np.int32)):
        src[f] = np.zeros(R, dt) if records.get(f) is None else np.asarray(records[f], dt).reshape(-1)
    src["multiplicity"] = np.ones(R, np.uint32) if records.get("multiplicity") is None else \
        np.asarray(records["multiplicity"], np.uint32).reshape(-1)
    assert all(len(v) == R for v in src.values())
    return src


def import_records(vm, records):
    """merges the records into the vmap_np.VoxelMap `vm`; returns the delta {"total", "dropped", "first_created",
    "created", "updated", "updated_ids", "dst_ids"}"""
    src = sources(records)
    xyz, mult_r = src["xyz"], src["multiplicity"].astype(np.int64)
    R, M0 = len(xyz), vm.M
    vm.calls += 1
    c = vm.calls
    cell, ok = voxel_np.cells(xyz, vm.voxel_size)
    ok = ok & (mult_r > 0)
    dropped = int(R - ok.sum())
    vm.points += int(mult_r[ok].sum())
    vm.dropped += dropped
    delta = {"total": R, "dropped": dropped, "first_created": M0, "created": 0, "updated": 0,
             "updated_ids": np.zeros(0, np.uint32), "dst_ids": np.full(R, NOID, np.uint32)}
    if dropped == R:
        return delta
    rm = np.flatnonzero(ok)
    ci = cell[ok].astype(np.int64) + (1 << 20)
    vox = (ci[:, 0] << 42) | (ci[:, 1] << 21) | ci[:, 2]
    skey = voxel_np.sigma_key(src["rho_sigma"][ok, 1]).astype(np.uint64)
    order = np.lexsort(((skey << np.uint64(32)) | rm.astype(np.uint64), vox))
    vs, rs, ks = vox[order], rm[order], skey[order]
    first = np.append(True, vs[1:] != vs[:-1])
    start = np.flatnonzero(first)
    uv = vs[start]                            # the call's voxels, ascending key
    win_r, win_key = rs[start], ks[start]     # (each voxel's first sorted record minimises (key, r))
    add = np.add.reduceat(mult_r[rs], start)  # (R <= 2^30 records of < 2^32: no int64 sum overflows)
    first_r = np.minimum.reduceat(rs, start)
    pos = np.searchsorted(vm.keys, uv)
    found = pos < len(vm.keys)
    found[found] = vm.keys[pos[found]] == uv[found]
    eid = np.full(len(uv), -1, np.int64)
    eid[found] = vm.ids[pos[found]]
    new = np.flatnonzero(~found)
    new = new[np.argsort(first_r[new], kind="stable")]  # ids in the order of the voxels' first records
    eid[new] = M0 + np.arange(len(new))
    old = np.flatnonzero(found)
    beats = win_key[old] < voxel_np.sigma_key(vm.rec["rho_sigma"][eid[old], 1]).astype(np.uint64)
    upd = old[beats]
    upd = upd[np.argsort(win_r[upd], kind="stable")]
    mult = np.concatenate([vm.rec["multiplicity"].astype(np.int64), np.zeros(len(new), np.int64)])
    mult[eid] = np.minimum(mult[eid] + np.minimum(add, SAT), SAT)
    for f in vmap_np.FIELDS:
        vm.rec[f] = np.concatenate([vm.rec[f], vmap_np._empty(f, len(new))])
    vm.rec["multiplicity"] = mult.astype(np.uint32)
    write = np.concatenate([new, upd])
    for f in vmap_np.RECORD:
        vm.rec[f][eid[write]] = src[f][win_r[write]]
    vm.rec["epoch"][eid[write]] = c
    keys = np.concatenate([vm.keys, uv[new]])
    ids = np.concatenate([vm.ids, eid[new]])
    o = np.argsort(keys, kind="stable")
    vm.keys, vm.ids = keys[o], ids[o]
    delta["dst_ids"][rs] = eid[np.cumsum(first) - 1].astype(np.uint32)
    delta.update(created=len(new), updated=len(upd), updated_ids=eid[upd].astype(np.uint32))
    return delta


def import_observations(ol, M, entry, tag, entry_map=None):
    """merges the pairs into the vmap_obs_np.ObservationLog `ol` of a map with M entries; returns {"total", "rejected",
    "first_created", "created"}"""
    ent = np.asarray(entry, np.uint32).reshape(-1).astype(np.int64)
    tg = np.asarray(tag, np.int32).reshape(-1).astype(np.int64)
    assert len(ent) == len(tg)
    if entry_map is not None:
        emap = np.asarray(entry_map, np.uint32).reshape(-1).astype(np.int64)
        inside = ent < len(emap)
        res = np.full(len(ent), NOID, np.int64)
        res[inside] = emap[ent[inside]]
        ent = res
    good = (ent < M) & (tg >= 0)
    delta = {"total": len(ent), "rejected": int((~good).sum()), "first_created": ol.E, "created": 0}
    ol.calls += 1
    pair = (ent[good] << 32) | tg[good]
    order = np.flatnonzero(good)
    fresh = ~np.isin(pair, ol.pairs)
    pair, order = pair[fresh], order[fresh]
    if len(pair):
        o = np.lexsort((order, pair))
        pair, order = pair[o], order[o]
        first = np.append(True, pair[1:] != pair[:-1])  # each new pair's first index
        pair, order = pair[first], order[first]
        pair = pair[np.argsort(order, kind="stable")]
        ol.entry = np.concatenate([ol.entry, (pair >> 32).astype(np.uint32)])
        ol.tag = np.concatenate([ol.tag, (pair & 0xffffffff).astype(np.int32)])
        ol.pairs = np.sort(np.concatenate([ol.pairs, pair]))
        delta["created"] = len(pair)
    return delta
