"""NumPy restatement of sdm_extract_points_voxel_freespace's free-space counts (include/sdm_c.h): per kept point of the
merged cloud, the (camera, kept point) rays of the call that pass through its voxel on their way to another point.

  one ray per entry e of the camera lists: from O, the camera centre of slot cam_slots[e], to P, the kept point's xyz
  cells cO = floor(O * inv), cP = floor(P * inv) in float32, inv = float32(1) / float32(voxel_size); a ray with a cell
  outside [-2^20, 2^20) (NaN, +-Inf) or with N = sum |cP - cO| > max_steps is skipped
  the walk takes exactly N steps: per step the axis with steps left and the smallest tMax (x, y, z in turn, replaced only
  by a strictly smaller value), tMax += tDel; the cells of index s <= N - 1 - end_margin are counted

All arithmetic is float32 (NumPy never fuses).  Vectorised over the rays; the one Python loop runs over the steps."""
import numpy as np

LIM = np.float32(2.0 ** 20)
MAX_STEPS = 65536  # SDM_FREESPACE_MAX_STEPS


def camera_centre(Tcw):
    """O = -(Rwc * tcw) of a [3, 4] (or 12) float32 pose, in the order of the point-set pass"""
    T = np.asarray(Tcw, np.float32).reshape(3, 4)
    t = T[:, 3]
    O = np.empty(3, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(3):  # Rwc[i][j] = Tcw[j][i]
            O[i] = -((T[0, i] * t[0] + T[1, i] * t[1]) + T[2, i] * t[2])
    return O


def pack(cell):
    """int64 cells [R, 3] in [-2^20, 2^20) -> the 63-bit voxel key"""
    c = cell.astype(np.int64) + (1 << 20)
    return (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]


def freespace(xyz, cam_offsets, cam_slots, centres, voxel_size, end_margin=1, max_steps=4096):
    """xyz float32[M, 3] kept points, cam_offsets int64[M + 1], cam_slots int32[E], centres {slot: float32[3]} or an array
    indexed by slot -> dict(crossings uint32[M], rays_total, rays_skipped, cells_visited, steps int64[E] (N, or -1 for a
    skipped ray), end int64[E, 3] (the cell each walked ray stops in), end_cell int64[E, 3] (cP of each walked ray))"""
    assert end_margin >= 0 and 1 <= max_steps <= MAX_STEPS
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    M = len(xyz)
    offs = np.asarray(cam_offsets, np.int64).reshape(-1)
    slots = np.asarray(cam_slots, np.int64).reshape(-1)
    E = len(slots)
    assert len(offs) == M + 1 and offs[0] == 0 and offs[-1] == E
    voxel = np.float32(voxel_size)
    inv = np.float32(1.0) / voxel
    k_of = np.repeat(np.arange(M), np.diff(offs))  # k(e)
    P = xyz[k_of]
    uniq = np.unique(slots)
    O_of = np.zeros((int(uniq.max()) + 1 if E else 1, 3), np.float32)
    for s in uniq:
        O_of[s] = np.asarray(centres[int(s)], np.float32)
    O = O_of[slots]
    with np.errstate(invalid="ignore", over="ignore"):
        fO, fP = np.floor(O * inv), np.floor(P * inv)
        ok = ((fO >= -LIM) & (fO < LIM) & (fP >= -LIM) & (fP < LIM)).all(axis=1)
        # the table: voxel key -> kept point, over the mergeable kept points (one per voxel in a merged cloud)
        fK = np.floor(xyz * inv)
        merge = ((fK >= -LIM) & (fK < LIM)).all(axis=1)
    keys = pack(fK[merge])
    order = np.argsort(keys, kind="stable")
    keys, owner = keys[order], np.flatnonzero(merge)[order]
    assert (keys[1:] != keys[:-1]).all(), "two mergeable kept points share a voxel"

    steps = np.full(E, -1, np.int64)
    end = np.zeros((E, 3), np.int64)
    end_cell = np.zeros((E, 3), np.int64)
    cO = np.where(ok[:, None], fO, 0).astype(np.int64)
    cP = np.where(ok[:, None], fP, 0).astype(np.int64)
    N = np.abs(cP - cO).sum(axis=1)
    walk = np.flatnonzero(ok & (N <= max_steps))
    steps[walk] = N[walk]
    crossings = np.zeros(M, np.int64)

    cur, tgt, n_of = cO[walk].copy(), cP[walk], N[walk]
    end_cell[walk] = tgt
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
    for s in range(int(n_of.max()) if len(walk) else 0):
        live = np.flatnonzero(s < n_of)
        cnt = live[s < counted[live]]
        if len(cnt) and len(keys):
            key = pack(cur[cnt])
            at = np.minimum(np.searchsorted(keys, key), len(keys) - 1)
            np.add.at(crossings, owner[at[keys[at] == key]], 1)
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
    end[walk] = cur
    return {"crossings": crossings.astype(np.uint32), "rays_total": E, "rays_skipped": E - len(walk),
            "cells_visited": int(counted.sum()), "steps": steps, "end": end, "end_cell": end_cell}
