"""NumPy restatement of sdm_vmap_cast_segments and sdm_vmap_render (include/sdm_c.h): the first entry of the persistent
voxel map along a segment, and the view the map predicts for a camera.

  ray       a segment from O to P; cO = floor(O * inv), cP = floor(P * inv) in float32, inv = float32(1) / float32(voxel_size);
            a ray with a cell outside [-2^20, 2^20) (NaN, +-Inf) or with N = sum |cP - cO| > max_steps is SKIPPED
  walk      vmap_carve_np.carve's, stated once more with the early exit: per step the axis with steps left and the smallest
            tMax (x, y, z in turn, replaced only by a strictly smaller value), tMax += tDel; cur at index s = 0 .. N
  examined  the cells start_margin <= s <= N - end_margin, in increasing s
  filter    an examined cell stops the ray iff its key has an entry id with multiplicity[id] >= min_multiplicity and, with
            require_published, published[id] != 0 (flags None: every flag reads 0)
  per ray   hit_id, hit_step of the first stopping cell; (NO_HIT, 0) for none; (SKIPPED, 0) for a skipped ray
  totals    rays_total, rays_skipped, rays_hit, cells_visited = examined cells up to and including the stopping one
  render    ray i = y * W + x from carve_np.camera_centre(Tcw) to vmap_repose_np.pointset_pixels(K, Tcw, x, y, rho_far);
            hit_rho = 1 / (((Tcw[8] X + Tcw[9] Y) + Tcw[10] Z) + Tcw[11]) of the hit entry's record xyz, +0 otherwise
The map is only read: its keys and ids come from vmap_recarve_np.map_index(record xyz).

All arithmetic is float32 (NumPy never fuses).  Vectorised over the rays; the one Python loop runs over the steps."""
import numpy as np

import carve_np
import vmap_recarve_np as vr
from carve_np import LIM, MAX_STEPS, pack
from vmap_carve_np import _lookup
from vmap_repose_np import pointset_pixels

f32 = np.float32
NO_HIT, SKIPPED = 0xFFFFFFFF, 0xFFFFFFFE
OUTS = ("rays_total", "rays_skipped", "rays_hit", "cells_visited")


def stops(rec, flags, min_multiplicity=0, require_published=False):
    """bool[M]: the entries that pass the filter"""
    mult = np.asarray(rec["multiplicity"], np.int64).reshape(-1)
    ok = mult >= int(min_multiplicity)
    if require_published:
        ok &= (np.zeros(len(mult), bool) if flags is None else np.asarray(flags).reshape(-1)[:len(mult)] != 0)
    return ok


def cast_segments(rec, flags, origins, ends, voxel_size, start_margin=0, end_margin=0, max_steps=4096, min_multiplicity=0,
                  require_published=False):
    """rec: the map's records {"xyz" float32[M, 3], "multiplicity" uint32[M]}; flags: uint8[M] or None; origins, ends
    float32[n, 3] -> dict(hit_id uint32[n], hit_step int32[n], the four totals, steps int64[n]: N, or -1 for a skipped ray)"""
    assert start_margin >= 0 and end_margin >= 0 and 1 <= max_steps <= MAX_STEPS
    xyz = np.ascontiguousarray(rec["xyz"], f32).reshape(-1, 3)
    keys, ids = vr.map_index(xyz, voxel_size)
    passes = stops(rec, flags, min_multiplicity, require_published)
    O = np.ascontiguousarray(origins, f32).reshape(-1, 3)
    P = np.ascontiguousarray(ends, f32).reshape(-1, 3)
    n = len(O)
    assert len(P) == n
    voxel = f32(voxel_size)
    inv = f32(1.0) / voxel
    with np.errstate(invalid="ignore", over="ignore"):
        fO, fP = np.floor(O * inv), np.floor(P * inv)
        ok = ((fO >= -LIM) & (fO < LIM) & (fP >= -LIM) & (fP < LIM)).all(axis=1)
    cO = np.where(ok[:, None], fO, 0).astype(np.int64)
    cP = np.where(ok[:, None], fP, 0).astype(np.int64)
    N = np.abs(cP - cO).sum(axis=1)
    walk = np.flatnonzero(ok & (N <= max_steps))
    steps = np.full(n, -1, np.int64)
    steps[walk] = N[walk]
    hit_id = np.full(n, SKIPPED, np.uint32)
    hit_id[walk] = NO_HIT
    hit_step = np.zeros(n, np.int32)

    cur, tgt, n_of = cO[walk].copy(), cP[walk], N[walk]
    step = np.sign(tgt - cur)
    r = np.abs(tgt - cur)
    o, p = O[walk], P[walk]
    with np.errstate(all="ignore"):
        d = p - o
        bnd = (cur + (step > 0)).astype(f32) * voxel
        tMax = (bnd - o) / d
        tDel = voxel / np.abs(d)
    assert tMax.dtype == f32 and tDel.dtype == f32
    last = n_of - end_margin                      # the examined cells are start_margin .. last
    going = np.ones(len(walk), bool)              # walked rays that have not stopped
    visited = 0
    for s in range(int(last.max()) + 1 if len(walk) else 0):
        live = np.flatnonzero(going & (s <= last))
        if not len(live):
            break
        if s >= start_margin:
            visited += len(live)
            e = _lookup(keys, ids, pack(cur[live]))
            stop = e >= 0
            stop[stop] = passes[e[stop]]
            hit_id[walk[live[stop]]] = e[stop].astype(np.uint32)
            hit_step[walk[live[stop]]] = s
            going[live[stop]] = False
            live = live[~stop]
        live = live[s < last[live]]               # (a ray at s == last has been examined for the last time)
        if not len(live):
            continue
        a = np.full(len(live), -1)
        best = np.zeros(len(live), f32)
        for ax in range(3):
            take = (r[live, ax] > 0) & ((a < 0) | (tMax[live, ax] < best))  # (a NaN compares false)
            a[take] = ax
            best[take] = tMax[live[take], ax]
        assert (a >= 0).all()
        cur[live, a] += step[live, a]
        r[live, a] -= 1
        with np.errstate(all="ignore"):
            tMax[live, a] = tMax[live, a] + tDel[live, a]
    hit = (hit_id != NO_HIT) & (hit_id != SKIPPED)
    return {"hit_id": hit_id, "hit_step": hit_step, "rays_total": n, "rays_skipped": n - len(walk), "rays_hit": int(hit.sum()),
            "cells_visited": int(visited), "steps": steps}


def render_segments(K, Tcw, W, H, rho_far):
    """(origins, ends) float32[W * H, 3] of sdm_vmap_render's rays, ray i = y * W + x"""
    assert 1 <= W <= 65535 and 1 <= H <= 65535 and float(f32(rho_far)) >= 0.000001
    i = np.arange(W * H)
    ends = pointset_pixels(K, Tcw, i % W, i // W, np.full(W * H, rho_far, f32))
    return np.tile(carve_np.camera_centre(Tcw), (W * H, 1)).astype(f32), ends


def render(rec, flags, K, Tcw, W, H, rho_far, voxel_size, **kw):
    """-> cast_segments' dict over the pixels' rays with hit_id, hit_step shaped [H, W], plus hit_rho float32[H, W]"""
    origins, ends = render_segments(K, Tcw, W, H, rho_far)
    got = cast_segments(rec, flags, origins, ends, voxel_size, **kw)
    got["hit_rho"] = hit_rho(rec, Tcw, got["hit_id"]).reshape(H, W)
    for f in ("hit_id", "hit_step"):
        got[f] = got[f].reshape(H, W)
    return got


def hit_rho(rec, Tcw, hit_id):
    """1 / z of each hit entry's record xyz in the camera Tcw, float32, +0 where nothing was hit"""
    T = np.asarray(Tcw, f32).reshape(12)
    hit_id = np.asarray(hit_id, np.uint32).reshape(-1)
    hit = (hit_id != NO_HIT) & (hit_id != SKIPPED)
    out = np.zeros(len(hit_id), f32)
    p = np.ascontiguousarray(rec["xyz"], f32).reshape(-1, 3)[hit_id[hit].astype(np.int64)]
    with np.errstate(all="ignore"):
        z = ((T[8] * p[:, 0] + T[9] * p[:, 1]) + T[10] * p[:, 2]) + T[11]
        out[hit] = f32(1.0) / z
    assert out.dtype == f32
    return out
