"""NumPy restatement of the observation log on the persistent voxel map (sdm_vmap_observe, sdm_vmap_fetch_observations,
sdm_vmap_fetch_cameras; include/sdm_c.h): per ENTRY of the map, the set of keyframe tags that saw any point of its voxel,
kept as an append-only log of (entry, tag) pairs.

  tags     the tag of row i is own_tags[i]; the tag of column j of row i is nbr_tags[i][j]
  cameras  C(g) = {own tag of i(g)} U {tag of column j : bit j of support[g]} -- a SET of tags: equal tags collapse and a
           column that carries the point's own tag falls out; without a neighbour table C(g) is the own tag alone
  entry    id(g) = the entry of the voxel of the point's xyz (voxel_np's cells and mergeability); a point that is
           unmergeable or whose voxel has no entry is UNMAPPED and contributes nothing
  result   as if the mapped points were processed in increasing g and within a point its tags in ascending order: a pair
           not yet stored is appended with index E
The map is only read: its keys and ids come from vmap_np.VoxelMap.keys / .ids.

Vectorised: one candidate per (g, position d in the row's ascending distinct tag list), ordered by g * Lmax + d; the new
pairs are the first candidates of the pair keys the log does not hold, in that order."""
import numpy as np

import voxel_np
from vmap_carve_np import _lookup

DELTA = ("plain_total", "unmapped", "candidates", "first_created", "created")
TAG_LIM = 1 << 31


def row_lists(own_tags, nbr_tags):
    """per row: (its distinct tags ascending, the mask of the columns that name each), own tag included (mask: the
    columns equal to it)"""
    own = np.asarray(own_tags, np.int64).reshape(-1)
    n = len(own)
    nb = np.zeros((n, 0), np.int64) if nbr_tags is None or n == 0 else np.asarray(nbr_tags, np.int64).reshape(n, -1)
    assert nb.shape[1] <= 64 and (own >= 0).all() and (own < TAG_LIM).all() and (nb >= 0).all() and (nb < TAG_LIM).all()
    out = []
    for i in range(n):
        tags = np.unique(np.append(nb[i], own[i]))
        masks = [sum(1 << j for j in range(nb.shape[1]) if nb[i, j] == t) for t in tags]
        out.append((tags, np.array(masks, np.uint64)))
    return out


def entries_of(map_keys_ids, plain_xyz, voxel_size):
    """id(g) int64[T], -1 for an unmapped point"""
    keys = np.asarray(map_keys_ids[0], np.int64).reshape(-1)
    ids = np.asarray(map_keys_ids[1], np.int64).reshape(-1)
    xyz = np.ascontiguousarray(plain_xyz, np.float32).reshape(-1, 3)
    cell, ok = voxel_np.cells(xyz, voxel_size)
    eid = np.full(len(xyz), -1, np.int64)
    if ok.any():
        ci = cell[ok].astype(np.int64) + (1 << 20)
        eid[ok] = _lookup(keys, ids, (ci[:, 0] << 42) | (ci[:, 1] << 21) | ci[:, 2])
    return eid


class ObservationLog:
    def __init__(self):
        self.clear()

    def clear(self):
        self.entry = np.zeros(0, np.uint32)
        self.tag = np.zeros(0, np.int32)
        self.pairs = np.zeros(0, np.int64)  # (entry << 32 | tag) of the log, sorted
        self.calls = 0

    @property
    def E(self):
        return len(self.entry)

    def info(self):
        return {"observations": self.E, "calls": self.calls}

    def observe(self, map_keys_ids, voxel_size, plain_xyz, slot_index_of_g, support_words, own_tags, nbr_tags):
        """map_keys_ids: (keys int64[M] sorted, ids int64[M]); plain_xyz float32[T, 3]; slot_index_of_g int[T]: i(g);
        support_words uint64[T] (ignored when nbr_tags is None); own_tags int[n]; nbr_tags int[n, n_nbr] or None
        -> the delta {"plain_total", "unmapped", "candidates", "first_created", "created"}"""
        row = np.asarray(slot_index_of_g, np.int64).reshape(-1)
        T = len(row)
        eid = entries_of(map_keys_ids, plain_xyz, voxel_size)
        assert len(eid) == T
        lists = row_lists(own_tags, nbr_tags)
        own = np.asarray(own_tags, np.int64).reshape(-1)
        sup = np.zeros(T, np.uint64) if nbr_tags is None else np.asarray(support_words, np.uint64).reshape(-1)
        assert len(sup) == T
        Lmax = max([len(t) for t, _ in lists] + [1])
        g_of, t_of, d_of = [], [], []
        for i, (tags, masks) in enumerate(lists):
            mine = np.flatnonzero(row == i)
            for d, (t, m) in enumerate(zip(tags, masks)):
                seen = mine if t == own[i] else mine[(sup[mine] & m) != 0]
                g_of.append(seen)
                t_of.append(np.full(len(seen), t, np.int64))
                d_of.append(np.full(len(seen), d, np.int64))
        g_of = np.concatenate(g_of) if g_of else np.zeros(0, np.int64)
        t_of = np.concatenate(t_of) if t_of else np.zeros(0, np.int64)
        d_of = np.concatenate(d_of) if d_of else np.zeros(0, np.int64)
        mapped = eid[g_of] >= 0
        delta = {"plain_total": T, "unmapped": int((eid < 0).sum()), "candidates": int(mapped.sum()),
                 "first_created": self.E, "created": 0}
        self.calls += 1
        pair = (eid[g_of[mapped]] << 32) | t_of[mapped]
        order = g_of[mapped] * Lmax + d_of[mapped]
        fresh = ~np.isin(pair, self.pairs)
        pair, order = pair[fresh], order[fresh]
        if len(pair):
            o = np.lexsort((order, pair))
            pair, order = pair[o], order[o]
            first = np.append(True, pair[1:] != pair[:-1])  # each new pair's smallest order key
            pair, order = pair[first], order[first]
            pair = pair[np.argsort(order, kind="stable")]
            self.entry = np.concatenate([self.entry, (pair >> 32).astype(np.uint32)])
            self.tag = np.concatenate([self.tag, (pair & 0xffffffff).astype(np.int32)])
            self.pairs = np.sort(np.concatenate([self.pairs, pair]))
            delta["created"] = len(pair)
        return delta

    def fetch(self, first=0, count=None):
        count = self.E - first if count is None else count
        if first < 0 or count < 0 or first + count > self.E:
            raise IndexError("range beyond the log's observations")
        return {"entry": self.entry[first:first + count], "tag": self.tag[first:first + count]}

    def cameras(self, M, ids=None, first=0, count=None):
        """(cam_offsets int64[count + 1], cam_tags int32[total]): per requested entry its tags in ascending order"""
        if ids is None:
            count = M - first if count is None else count
            if first < 0 or count < 0 or first + count > M:
                raise IndexError("range beyond the map's entries")
            sel = np.arange(first, first + count)
        else:
            sel = np.asarray(ids, np.int64).reshape(-1)
            if first != 0 or (sel >= M).any():
                raise IndexError("id beyond the map's entries")
        lo = np.searchsorted(self.pairs, sel << 32)
        hi = np.searchsorted(self.pairs, (sel + 1) << 32)
        offs = np.concatenate([[0], np.cumsum(hi - lo)]).astype(np.int64)
        tags = [self.pairs[a:b] & 0xffffffff for a, b in zip(lo, hi)]
        return offs, (np.concatenate(tags) if tags else np.zeros(0, np.int64)).astype(np.int32)


def lists(cam_offsets, cam_tags):
    return [cam_tags[a:b].tolist() for a, b in zip(cam_offsets[:-1], cam_offsets[1:])]
