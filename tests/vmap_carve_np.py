"""NumPy restatement of sdm_vmap_carve's free-space evidence on the persistent voxel map (include/sdm_c.h): per ENTRY of
the map, the (camera, plain point) rays of a call that pass through its voxel (crossings) and that end in it (ends).

  state   two 64-bit counters per entry, 0 when the entry is created and after clear
  cameras C(g) = {slots[i(g)]} U {nbr_slots[i(g)][j] : bit j of support[g]} -- a SET: a repeated neighbour and a neighbour
          equal to the point's own slot fall out; without a neighbour table C(g) is the observing slot alone
  rays    one per (g, s in C(g)): from O, the camera centre of slot s, to P, the plain point's own xyz
  cells   cO = floor(O * inv), cP = floor(P * inv) in float32, inv = float32(1) / float32(voxel_size); a ray with a cell
          outside [-2^20, 2^20) (NaN, +-Inf) or with N = sum |cP - cO| > max_steps is skipped
  walk    exactly N steps: per step the axis with steps left and the smallest tMax (x, y, z in turn, replaced only by a
          strictly smaller value), tMax += tDel; the cells of index s <= N - 1 - end_margin are counted
  count   every counted cell whose key has an entry adds 1 to crossings[id]; every walked ray whose end cell cP has an
          entry adds 1 to ends[id], whatever end_margin
The map is only read: its keys and ids come from vmap_np.VoxelMap.keys / .ids.

All arithmetic is float32 (NumPy never fuses).  Vectorised over the rays; the one Python loop runs over the steps."""
import numpy as np

from carve_np import LIM, MAX_STEPS, pack

TOTALS = ("plain_total", "rays_total", "rays_skipped", "cells_visited", "cells_hit", "ends_hit")


def rays_of(slot_index_of_g, support_words, slots, nbr_slots):
    """the rays (g, camera slot) of the call: (g int64[R], slot int64[R]), one per member of C(g)"""
    row = np.asarray(slot_index_of_g, np.int64).reshape(-1)
    T = len(row)
    slots = np.asarray(slots, np.int64).reshape(-1)
    g_of, s_of = [np.arange(T)], [slots[row]]
    if nbr_slots is not None:
        nb = np.asarray(nbr_slots, np.int64).reshape(len(slots), -1)
        sup = np.asarray(support_words, np.uint64).reshape(-1)
        assert len(sup) == T
        for i in range(len(slots)):
            mine = np.flatnonzero(row == i)
            for s in dict.fromkeys(int(v) for v in nb[i]):  # the distinct neighbours of slot i
                if s == slots[i]:
                    continue
                mask = np.uint64(sum(1 << j for j in range(nb.shape[1]) if nb[i, j] == s))
                seen = mine[(sup[mine] & mask) != 0]
                g_of.append(seen)
                s_of.append(np.full(len(seen), s, np.int64))
    return np.concatenate(g_of), np.concatenate(s_of)


def _lookup(keys, ids, key):
    """the entry of each key, or -1"""
    if not len(keys):
        return np.full(len(key), -1, np.int64)
    at = np.minimum(np.searchsorted(keys, key), len(keys) - 1)
    return np.where(keys[at] == key, ids[at], -1)


def carve(map_keys_ids, plain_xyz, slot_index_of_g, support_words, slots, nbr_slots, centres, voxel_size, end_margin=1,
          max_steps=4096):
    """map_keys_ids: (keys int64[M] sorted, ids int64[M]) of the entries present; plain_xyz float32[T, 3];
    slot_index_of_g int[T]: i(g); support_words uint64[T] (ignored when nbr_slots is None); slots int[n];
    nbr_slots int[n, n_nbr] or None; centres {slot: float32[3]} or an array indexed by slot
    -> dict(crossings uint64[M], ends uint64[M], the six totals, steps int64[R] (N, or -1 for a skipped ray))"""
    assert end_margin >= 0 and 1 <= max_steps <= MAX_STEPS
    keys = np.asarray(map_keys_ids[0], np.int64).reshape(-1)
    ids = np.asarray(map_keys_ids[1], np.int64).reshape(-1)
    M = len(ids)
    assert (keys[1:] > keys[:-1]).all() and (M == 0 or sorted(ids.tolist()) == list(range(M)))
    xyz = np.ascontiguousarray(plain_xyz, np.float32).reshape(-1, 3)
    T = len(xyz)
    g_of, s_of = rays_of(slot_index_of_g, support_words, slots, nbr_slots)
    R = len(g_of)
    voxel = np.float32(voxel_size)
    inv = np.float32(1.0) / voxel
    P = xyz[g_of]
    O = np.zeros((R, 3), np.float32)
    for s in np.unique(s_of):
        O[s_of == s] = np.asarray(centres[int(s)], np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        fO, fP = np.floor(O * inv), np.floor(P * inv)
        ok = ((fO >= -LIM) & (fO < LIM) & (fP >= -LIM) & (fP < LIM)).all(axis=1)
    cO = np.where(ok[:, None], fO, 0).astype(np.int64)
    cP = np.where(ok[:, None], fP, 0).astype(np.int64)
    N = np.abs(cP - cO).sum(axis=1)
    walk = np.flatnonzero(ok & (N <= max_steps))
    steps = np.full(R, -1, np.int64)
    steps[walk] = N[walk]
    crossings, ends = np.zeros(M, np.int64), np.zeros(M, np.int64)

    cur, tgt, n_of = cO[walk].copy(), cP[walk], N[walk]
    step = np.sign(tgt - cur)
    r = np.abs(tgt - cur)
    o, p = O[walk], P[walk]
    with np.errstate(all="ignore"):
        d = p - o
        bnd = (cur + (step > 0)).astype(np.float32) * voxel
        tMax = (bnd - o) / d
        tDel = voxel / np.abs(d)
    assert tMax.dtype == np.float32 and tDel.dtype == np.float32
    counted = np.maximum(n_of - end_margin, 0)
    hit = 0
    for s in range(int(n_of.max()) if len(walk) else 0):
        live = np.flatnonzero(s < n_of)
        cnt = live[s < counted[live]]
        if len(cnt):
            e = _lookup(keys, ids, pack(cur[cnt]))
            np.add.at(crossings, e[e >= 0], 1)
            hit += int((e >= 0).sum())
        a = np.full(len(live), -1)
        best = np.zeros(len(live), np.float32)
        for ax in range(3):
            take = (r[live, ax] > 0) & ((a < 0) | (tMax[live, ax] < best))  # (a NaN compares false)
            a[take] = ax
            best[take] = tMax[live[take], ax]
        assert (a >= 0).all()
        cur[live, a] += step[live, a]
        r[live, a] -= 1
        with np.errstate(all="ignore"):
            tMax[live, a] = tMax[live, a] + tDel[live, a]
    assert (cur == tgt).all()  # every walked ray stops in cP
    e = _lookup(keys, ids, pack(tgt)) if len(walk) else np.zeros(0, np.int64)
    np.add.at(ends, e[e >= 0], 1)
    return {"crossings": crossings.astype(np.uint64), "ends": ends.astype(np.uint64), "plain_total": T, "rays_total": R,
            "rays_skipped": R - len(walk), "cells_visited": int(counted.sum()), "cells_hit": hit,
            "ends_hit": int((e >= 0).sum()), "steps": steps, "ray_g": g_of, "ray_slot": s_of}
