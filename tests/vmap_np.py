"""NumPy restatement of the persistent voxel map's semantics (sdm_vmap_*, include/sdm_c.h) over explicit plain clouds.

  A cloud is {"xyz": f32[T,3], "pixel": u32[T], "rho_sigma": f32[T,2], "intensity": u8[T]} in plain order -- what
  sdm_extract_points returns -- plus one tag per point.  Cells, mergeability and key(sigma) are voxel_np's.  Processing
  the points in increasing g: an unmergeable point is dropped; a point of a voxel without an entry appends entry id = M
  (multiplicity 1, epoch c); any other adds 1 to the multiplicity (saturating at 2^32 - 1) and replaces the record iff its
  key is STRICTLY below the stored one (epoch c).  Done here per call with one sort instead of a loop: per voxel of the
  call, its first point, its count and the minimum of (key(sigma), g)."""
import numpy as np

import voxel_np

RECORD = ("xyz", "pixel", "rho_sigma", "intensity", "tag")
FIELDS = RECORD + ("multiplicity", "epoch")
_DT = {"xyz": (np.float32, 3), "pixel": (np.uint32, 1), "rho_sigma": (np.float32, 2), "intensity": (np.uint8, 1),
       "tag": (np.int32, 1), "multiplicity": (np.uint32, 1), "epoch": (np.uint32, 1)}
SAT = (1 << 32) - 1


def point_tags(offsets, slots, tags=None):
    """the tag of every plain point: tags[i] (default: slots[i]) for the points offsets[i] .. offsets[i + 1] - 1"""
    per = np.asarray(slots if tags is None else tags, np.int32).reshape(-1)
    return np.repeat(per, np.diff(np.asarray(offsets, np.int64)))


def _empty(f, n=0):
    dt, per = _DT[f]
    return np.zeros((n, per) if per > 1 else (n,), dt)


class VoxelMap:
    def __init__(self, voxel_size):
        self.voxel_size = voxel_size
        self.clear()

    def clear(self):
        self.rec = {f: _empty(f) for f in FIELDS}
        self.keys = np.zeros(0, np.int64)   # the cell keys of the entries, sorted
        self.ids = np.zeros(0, np.int64)    # the entry of each key
        self.points = self.dropped = self.calls = 0

    @property
    def M(self):
        return len(self.rec["pixel"])

    def info(self):
        return {"voxels": self.M, "points": self.points, "dropped": self.dropped, "calls": self.calls}

    def integrate(self, cloud, tag):
        """merges one plain cloud; returns the delta {"plain_total", "dropped", "first_created", "created", "updated",
        "updated_ids"}"""
        xyz = np.ascontiguousarray(cloud["xyz"], np.float32).reshape(-1, 3)
        sigma = np.ascontiguousarray(np.asarray(cloud["rho_sigma"], np.float32).reshape(-1, 2)[:, 1])
        T, M0 = len(xyz), self.M
        self.calls += 1
        c = self.calls
        cell, ok = voxel_np.cells(xyz, self.voxel_size)
        dropped = int(T - ok.sum())
        self.points += T - dropped
        self.dropped += dropped
        delta = {"plain_total": T, "dropped": dropped, "first_created": M0, "created": 0, "updated": 0,
                 "updated_ids": np.zeros(0, np.uint32)}
        if dropped == T:
            return delta
        gm = np.flatnonzero(ok)
        ci = cell[ok].astype(np.int64) + (1 << 20)
        vox = (ci[:, 0] << 42) | (ci[:, 1] << 21) | ci[:, 2]
        skey = voxel_np.sigma_key(sigma[ok]).astype(np.uint64)
        order = np.lexsort(((skey << np.uint64(32)) | gm.astype(np.uint64), vox))
        vs, gs, ks = vox[order], gm[order], skey[order]
        start = np.flatnonzero(np.append(True, vs[1:] != vs[:-1]))
        uv = vs[start]                            # the call's voxels, ascending key
        win_g, win_key = gs[start], ks[start]     # (each voxel's first sorted entry minimises (key, g))
        count = np.diff(np.append(start, len(vs)))
        first_g = np.minimum.reduceat(gs, start)
        # which of them have an entry
        pos = np.searchsorted(self.keys, uv)
        found = pos < len(self.keys)
        found[found] = self.keys[pos[found]] == uv[found]
        eid = np.full(len(uv), -1, np.int64)
        eid[found] = self.ids[pos[found]]
        # created: ids in the order of the voxels' first points
        new = np.flatnonzero(~found)
        new = new[np.argsort(first_g[new], kind="stable")]
        eid[new] = M0 + np.arange(len(new))
        # updated: the call's winner strictly beats the stored sigma
        old = np.flatnonzero(found)
        beats = win_key[old] < voxel_np.sigma_key(self.rec["rho_sigma"][eid[old], 1]).astype(np.uint64)
        upd = old[beats]
        upd = upd[np.argsort(win_g[upd], kind="stable")]
        # multiplicities
        mult = np.concatenate([self.rec["multiplicity"].astype(np.int64), np.zeros(len(new), np.int64)])
        mult[eid] = np.minimum(mult[eid] + count, SAT)
        # records
        for f in FIELDS:
            self.rec[f] = np.concatenate([self.rec[f], _empty(f, len(new))])
        self.rec["multiplicity"] = mult.astype(np.uint32)
        write = np.concatenate([new, upd])
        src = {"xyz": xyz, "pixel": np.asarray(cloud["pixel"], np.uint32).reshape(-1),
               "rho_sigma": np.asarray(cloud["rho_sigma"], np.float32).reshape(-1, 2),
               "intensity": np.asarray(cloud["intensity"], np.uint8).reshape(-1), "tag": np.asarray(tag, np.int32).reshape(-1)}
        for f in RECORD:
            self.rec[f][eid[write]] = src[f][win_g[write]]
        self.rec["epoch"][eid[write]] = c
        # the key index
        keys = np.concatenate([self.keys, uv[new]])
        ids = np.concatenate([self.ids, eid[new]])
        o = np.argsort(keys, kind="stable")
        self.keys, self.ids = keys[o], ids[o]
        delta.update(created=len(new), updated=len(upd), updated_ids=eid[upd].astype(np.uint32))
        return delta

    def fetch(self, ids=None, first=0, count=None):
        """entries first .. first + count - 1, or the entries ids[...]: {field: array}"""
        if ids is None:
            count = self.M - first if count is None else count
            if first < 0 or count < 0 or first + count > self.M:
                raise IndexError("range beyond the map's entries")
            sel = np.arange(first, first + count)
        else:
            sel = np.asarray(ids, np.int64).reshape(-1)
            if first != 0 or (sel >= self.M).any():
                raise IndexError("id beyond the map's entries")
        return {f: self.rec[f][sel] for f in FIELDS}
