"""NumPy restatement of the classification on the persistent voxel map (sdm_vmap_classify, include/sdm_c.h).

  Inputs: (keys, ids) and the records of a vmap_np.VoxelMap, the two free-space counters, ncam (the lengths of
  vmap_obs_np.ObservationLog.cameras' lists), a rule and the published flags.  The ratio test runs on Python integers, so
  no product wraps; the neighbour lookup is a searchsorted on the sorted cell keys.  Cells and key(sigma) are voxel_np's."""
import numpy as np

import voxel_np

RULE_DEFAULTS = {"min_multiplicity": 0, "min_cameras": 0, "min_ends": 0, "ratio_num": 1, "ratio_den": 1,
                 "max_sigma": float("inf"), "min_neighbours": 0}
LIM = 1 << 20


def rule_of(**kw):
    r = dict(RULE_DEFAULTS)
    for f in kw:
        if f not in r:
            raise KeyError(f)
    r.update(kw)
    if r["ratio_den"] < 1 or not 0 <= r["min_neighbours"] <= 26:
        raise ValueError("ratio_den must be >= 1 and min_neighbours in 0 .. 26")
    return r


def _pad(a, M, dt):
    """a per-entry input that may be missing (None) or shorter than M (entries created after it was taken): zeros"""
    out = np.zeros(M, dt)
    if a is not None:
        a = np.asarray(a).reshape(-1)
        out[:len(a)] = a[:M]
    return out


def local(rec, crossings, ends, ncam, rule):
    """bool[M]: the LOCAL tests of every entry"""
    M = len(rec["multiplicity"])
    cr, en, nc = _pad(crossings, M, np.uint64), _pad(ends, M, np.uint64), _pad(ncam, M, np.int64)
    num, den = int(rule["ratio_num"]), int(rule["ratio_den"])
    if M and (int(cr.max()) * den >= 1 << 64 or int(en.max()) * num >= 1 << 64):  # Python integers: nothing wraps
        ratio = np.fromiter((c * den <= e * num for c, e in zip(cr.tolist(), en.tolist())), bool, M)
    else:  # (no product reaches 2^64: uint64 is exact)
        ratio = cr * np.uint64(den) <= en * np.uint64(num)
    skey = voxel_np.sigma_key(np.asarray(rec["rho_sigma"], np.float32).reshape(-1, 2)[:, 1])
    mkey = voxel_np.sigma_key(np.array([rule["max_sigma"]], np.float32))[0]
    return ((rec["multiplicity"].astype(np.int64) >= int(rule["min_multiplicity"])) & (nc >= int(rule["min_cameras"])) &
            (en >= np.uint64(rule["min_ends"])) & ratio & (skey <= mkey))


def neighbours(keys_ids, rec, voxel_size, loc, only=None):
    """int[M]: nb(id), the adjacent cells that hold a LOCAL-passing entry (all 26 are looked up).  only: bool[M], the
    entries to count for; the others read 0"""
    keys = np.asarray(keys_ids[0], np.int64).reshape(-1)
    ids = np.asarray(keys_ids[1], np.int64).reshape(-1)
    M = len(loc)
    out = np.zeros(M, np.int64)
    sel = np.arange(M) if only is None else np.flatnonzero(only)
    if len(sel) == 0:
        return out
    cell, ok = voxel_np.cells(np.asarray(rec["xyz"], np.float32).reshape(-1, 3)[sel], voxel_size)
    assert ok.all()  # an entry's record is mergeable
    c = cell.astype(np.int64)
    nb = np.zeros(len(sel), np.int64)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                if dx == dy == dz == 0:
                    continue
                n = c + np.array([dx, dy, dz])
                inside = ((n >= -LIM) & (n < LIM)).all(1)
                b = n + LIM
                key = (b[:, 0] << 42) | (b[:, 1] << 21) | b[:, 2]
                pos = np.minimum(np.searchsorted(keys, key), len(keys) - 1)
                hit = inside & (keys[pos] == key)
                nb[hit] += loc[ids[pos[hit]]]
    out[sel] = nb
    return out


def passing(keys_ids, rec, voxel_size, crossings, ends, ncam, rule):
    """(passing bool[M], LOCAL bool[M])"""
    loc = local(rec, crossings, ends, ncam, rule)
    if rule["min_neighbours"] == 0:
        return loc.copy(), loc
    return loc & (neighbours(keys_ids, rec, voxel_size, loc, only=loc) >= rule["min_neighbours"]), loc


class Classifier:
    """the published flags and the committing calls since open / clear"""

    def __init__(self):
        self.clear()

    def clear(self):
        self.published = np.zeros(0, np.uint8)
        self.calls = 0

    def info(self):
        return {"published": int(self.published.sum()), "calls": self.calls}

    def flags(self, M):
        """uint8[M]: entries created after the last committing call read 0"""
        return _pad(self.published, M, np.uint8)

    def classify(self, vm, crossings, ends, ncam, rule, commit=True):
        """vm: a vmap_np.VoxelMap -> {"examined", "accepted", "retracted", "published_total", "accepted_ids",
        "retracted_ids", "local"} (local: the LOCAL-passing entries, for the tests)"""
        M = vm.M
        ok, loc = passing((vm.keys, vm.ids), vm.rec, vm.voxel_size, crossings, ends, ncam, rule)
        pub = self.flags(M).astype(bool)
        acc, ret = np.flatnonzero(ok & ~pub), np.flatnonzero(~ok & pub)
        if commit:
            self.published = ok.astype(np.uint8)
            self.calls += 1
        return {"examined": M, "accepted": len(acc), "retracted": len(ret),
                "published_total": int(ok.sum()) if commit else int(pub.sum()),
                "accepted_ids": acc.astype(np.uint32), "retracted_ids": ret.astype(np.uint32), "local": int(loc.sum())}
