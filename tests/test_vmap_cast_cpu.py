"""CPU: tests/vmap_cast_np.py (the NumPy statement of sdm_vmap_cast_segments and sdm_vmap_render) -- tied to a scalar loop,
one ray and one cell at a time as include/sdm_c.h words it, on crafted rays and on synthetic maps; its properties (a
stricter filter never brings a hit closer, the log's rays against sdm_vmap_recarve's statement on the golden fixtures, the
render against the segments it defines); and the fixture totals the GPU test relies on.  The synthetic inputs of
tests/test_gpu_vmap_cast.py are defined here."""
import numpy as np
import pytest

import carve_np
import golden_util as gu
import vmap_cast_np as vk
import vmap_recarve_np as vr
from test_vmap_carve_cpu import cloud_of
from test_vmap_recarve_cpu import EQ_MARGIN, EQ_STEPS, EQ_VOXEL, VOXEL, fixture_kf0, synthetic_case
from test_vmap_recarve_cpu import PINNED as RECARVE_PINNED
from test_vmap_repose_cpu import pose

F = np.float32
LIM = 1 << 20
ARRAYS = ("hit_id", "hit_step")
KINDS = ("hit at start_margin", "hit in the end cell", "miss", "range skip", "max_steps skip", "through a filtered entry to a hit",
         "through a filtered entry to a miss")
SYN_M = (0, 1, 65, 2049)
SYN_RAYS = (0, 1, 63, 64, 65, 257, 1025)
# a camera in front of the synthetic maps' cube of cells, looking along +z at it; the same camera turned round; no pose at all
RENDER_K = np.array([30.0, 30.0, 16.0, 8.0], F)
POSE_AT = pose(0.0, 0.0, (-0.3, -0.3, 1.0))
POSE_AWAY = pose(0.0, np.pi, (0.3, -0.3, -1.0))
POSE_NAN = np.full(12, np.nan, F)
RENDER_SIZES = ((1, 1), (64, 1), (33, 17))
RHO_FAR = 0.5


def scalar_cast(rec, flags, origins, ends, voxel_size, start_margin=0, end_margin=0, max_steps=4096, min_multiplicity=0,
                require_published=False):
    """the semantics of include/sdm_c.h, ray by ray, cell by cell (tests/test_vmap_carve_cpu.scalar_carve's pattern).  Beside
    vmap_cast_np's outputs: kind[i], the names of KINDS that ray i is an example of"""
    voxel = F(voxel_size)
    inv = F(1.0) / voxel
    xyz = np.asarray(rec["xyz"], F).reshape(-1, 3)
    mult = np.asarray(rec["multiplicity"]).reshape(-1)
    entry = {}
    for e, p in enumerate(xyz):
        cell = tuple(int(np.floor(p[a] * inv)) for a in range(3))
        assert cell not in entry
        entry[cell] = e
    O_all, P_all = np.asarray(origins, F).reshape(-1, 3), np.asarray(ends, F).reshape(-1, 3)
    n = len(O_all)
    hit_id, hit_step = np.full(n, vk.SKIPPED, np.uint32), np.zeros(n, np.int32)
    steps = np.full(n, -1, np.int64)
    tot = dict.fromkeys(vk.OUTS, 0)
    kind = [set() for _ in range(n)]
    for i in range(n):
        O, P = O_all[i], P_all[i]
        tot["rays_total"] += 1
        with np.errstate(all="ignore"):
            fO = [np.floor(O[a] * inv) for a in range(3)]
            fP = [np.floor(P[a] * inv) for a in range(3)]
            if not all(-LIM <= v < LIM for v in fO + fP):
                tot["rays_skipped"] += 1
                kind[i].add("range skip")
                continue
            cO, cP = [int(v) for v in fO], [int(v) for v in fP]
            r = [abs(cP[a] - cO[a]) for a in range(3)]
            N = sum(r)
            if N > max_steps:
                tot["rays_skipped"] += 1
                kind[i].add("max_steps skip")
                continue
            steps[i] = N
            hit_id[i] = vk.NO_HIT
            step = [(cP[a] > cO[a]) - (cP[a] < cO[a]) for a in range(3)]
            tMax, tDel = [None] * 3, [None] * 3
            for a in range(3):
                if r[a] > 0:
                    d = P[a] - O[a]
                    bnd = F(cO[a] + (1 if step[a] > 0 else 0)) * voxel
                    tMax[a] = (bnd - O[a]) / d
                    tDel[a] = voxel / abs(d)
            cur = list(cO)
            filtered = False
            for s in range(N + 1):  # cur is the ray's cell of index s
                if start_margin <= s <= N - end_margin:
                    tot["cells_visited"] += 1
                    e = entry.get(tuple(cur))
                    if e is not None:
                        if mult[e] >= min_multiplicity and (not require_published or (flags is not None and flags[e] != 0)):
                            hit_id[i], hit_step[i] = e, s
                            tot["rays_hit"] += 1
                            if s == start_margin:
                                kind[i].add("hit at start_margin")
                            if s == N:
                                kind[i].add("hit in the end cell")
                            if filtered:
                                kind[i].add("through a filtered entry to a hit")
                            break
                        filtered = True
                if s == N:
                    assert cur == cP
                    break
                best = None
                for a in range(3):  # never reads an axis with r = 0
                    if r[a] > 0 and (best is None or tMax[a] < tMax[best]):
                        best = a
                cur[best] += step[best]
                r[best] -= 1
                tMax[best] = tMax[best] + tDel[best]
            else:
                raise AssertionError("unreachable")
            if hit_id[i] == vk.NO_HIT:
                kind[i].add("miss")
                if filtered:
                    kind[i].add("through a filtered entry to a miss")
    return dict(tot, hit_id=hit_id, hit_step=hit_step, steps=steps, kind=kind)


def both(rec, flags, origins, ends, voxel, **kw):
    got = vk.cast_segments(rec, flags, origins, ends, voxel, **kw)
    exp = scalar_cast(rec, flags, origins, ends, voxel, **kw)
    assert got["hit_id"].dtype == np.uint32 and got["hit_step"].dtype == np.int32
    for f in ARRAYS + ("steps",):
        np.testing.assert_array_equal(got[f], exp[f], err_msg="%s %s" % (f, kw))
    assert {f: got[f] for f in vk.OUTS} == {f: exp[f] for f in vk.OUTS}, kw
    # the consequences sdm_c.h states
    hit = got["hit_id"] < (1 << 30)
    assert got["rays_hit"] == int(hit.sum()) and got["rays_skipped"] == int((got["hit_id"] == vk.SKIPPED).sum())
    assert not got["hit_step"][~hit].any() and (got["hit_id"][got["steps"] < 0] == vk.SKIPPED).all()
    return got, exp["kind"]


def crafted_case():
    """tests/test_vmap_carve_cpu.py's crafted points at voxel 1 as a map -- one entry per point, id = g; entry 8 lies in the
    cell of the origin (0.5, 0.5, 0.5); entry 11 on the long diagonal; entries 12 and 13 in the last cells of the range -- and
    segments: the eleven rays of that test (steps [6, 1, 2, 3, 4, 5, 4, 1, 0, 4, 5]), the three-axis tie to (7.5, 7.5, 7.5),
    a ray into empty space, rays along the edges of the cell range and one cell beyond them, and NaN and Inf coordinates"""
    e = 1048575.5   # the centre of cell 2^20 - 1; -e - 0.0 is the centre of cell -2^20
    pts = np.array([[2.5, 2.5, 2.5], [1.5, 0.5, 0.5], [1.5, 1.5, 0.5], [1.5, 1.5, 1.5], [2.5, 1.5, 1.5], [2.5, 2.5, 1.5],
                    [2.5, 2.5, 0.5], [0.5, 1.5, 0.5], [0.75, 0.25, 0.5], [-3.5, 0.5, 0.5], [0.5, 0.5, 5.5], [7.5, 7.5, 7.5],
                    [e, 0.5, 0.5], [0.5, -e, 0.5]], F)
    rec = dict(cloud_of(pts), tag=np.zeros(len(pts), np.int32))
    rec["multiplicity"] = np.array([2, 1, 3, 2, 2, 2, 2, 2, 1, 2, 2, 5, 2, 2], np.uint32)
    flags = (np.arange(len(pts)) % 2 == 1).astype(np.uint8)
    O0 = [0.5, 0.5, 0.5]
    segs = [(O0, p) for p in pts[:12].tolist()]
    segs += [(O0, [0.5, 0.5, -5.5]),                                   # 12: into empty space
             ([e - 3, 0.5, 0.5], [e, 0.5, 0.5]),                       # 13: ends in cell 2^20 - 1
             ([e - 3, 0.5, 0.5], [e + 1, 0.5, 0.5]),                   # 14: ends one cell beyond
             ([0.5, -e + 2, 0.5], [0.5, -e, 0.5]),                     # 15: ends in cell -2^20
             ([0.5, -e + 2, 0.5], [0.5, -e - 1, 0.5]),                 # 16: one cell beyond
             ([e, 0.5, 0.5], [e - 2, 0.5, 0.5]),                       # 17: starts in the last cell, which holds entry 12
             ([np.nan, 0.5, 0.5], [2.5, 2.5, 2.5]), (O0, [2.5, np.nan, 2.5]),
             (O0, [np.inf, 0.5, 0.5]), ([0.5, -np.inf, 0.5], O0),
             ([7.5, 7.5, 7.5], O0)]                                    # 22: the tie ray backwards
    return rec, flags, np.array([s[0] for s in segs], F), np.array([s[1] for s in segs], F)


CRAFTED_COMBOS = (dict(max_steps=64), dict(max_steps=64, start_margin=1), dict(max_steps=64, start_margin=1, end_margin=1),
                  dict(max_steps=21), dict(max_steps=20), dict(max_steps=6, start_margin=1), dict(max_steps=5, start_margin=1),
                  dict(max_steps=64, min_multiplicity=2), dict(max_steps=64, min_multiplicity=2, end_margin=1),
                  dict(max_steps=64, min_multiplicity=3), dict(max_steps=64, require_published=True),
                  dict(max_steps=64, require_published=True, min_multiplicity=2, start_margin=1),
                  dict(max_steps=64, min_multiplicity=6), dict(max_steps=64, min_multiplicity=0xFFFFFFFF),
                  dict(max_steps=64, start_margin=2, end_margin=3), dict(max_steps=64, start_margin=22),
                  dict(max_steps=64, end_margin=22), dict(max_steps=64, start_margin=1000, end_margin=1000))


def test_crafted_rays_against_the_scalar_loop():
    rec, flags, O, P = crafted_case()
    got, _ = both(rec, flags, O, P, 1.0, max_steps=64)
    assert got["steps"].tolist() == [6, 1, 2, 3, 4, 5, 4, 1, 0, 4, 5, 21, 6, 3, -1, 2, -1, 2, -1, -1, -1, -1, 21]
    # every ray from the origin's cell stops in it at once: it holds entry 8 (the ray to entry 8 itself has N = 0)
    assert got["hit_id"][:13].tolist() == [8] * 13 and not got["hit_step"][:13].any()
    assert got["hit_id"][13:18].tolist() == [12, vk.SKIPPED, 13, vk.SKIPPED, 12] and got["hit_step"][13:18].tolist() == [3, 0, 2, 0, 0]
    assert got["hit_id"][22] == 11 and got["hit_step"][22] == 0
    assert got["cells_visited"] == 13 + 4 + 3 + 1 + 1
    seen = set()
    combos = CRAFTED_COMBOS
    res = {}
    for kw in combos:
        got, kind = both(rec, flags, O, P, 1.0, **kw)
        res[tuple(sorted(kw.items()))] = got
        seen |= set().union(*kind)
    assert seen == set(KINDS), set(KINDS) - seen
    r = res[(("max_steps", 64), ("start_margin", 1))]
    # start_margin 1: the walk of ray 0 is (0,0,0) (1,0,0) (1,1,0) (1,1,1) (2,1,1) (2,2,1) (2,2,2): entry 1 at s = 1; the ray to
    # entry 9 meets nothing before its end cell; N = 0 examines nothing; the three-axis tie goes x, y, z: (1,0,0) first
    assert r["hit_id"][[0, 9, 8, 11]].tolist() == [1, 9, vk.NO_HIT, 1] and r["hit_step"][[0, 9, 8, 11]].tolist() == [1, 4, 0, 1]
    assert r["hit_id"][12] == vk.NO_HIT and r["cells_visited"] > 0
    r = res[(("end_margin", 1), ("max_steps", 64), ("start_margin", 1))]
    assert r["hit_id"][[9, 1, 7]].tolist() == [vk.NO_HIT] * 3            # the end cell is not examined; N = 1 examines nothing
    assert res[(("max_steps", 21),)]["rays_skipped"] == 6 and res[(("max_steps", 20),)]["rays_skipped"] == 8   # N == max_steps walks
    assert res[(("max_steps", 6), ("start_margin", 1))]["hit_id"][0] == 1 and res[(("max_steps", 5), ("start_margin", 1))]["hit_id"][0] == vk.SKIPPED
    r = res[(("max_steps", 64), ("min_multiplicity", 2))]
    # entries 8 and 1 (multiplicity 1) are transparent: ray 0 stops at entry 2 in (1,1,0), s = 2; the ray to entry 1 misses
    assert r["hit_id"][[0, 1, 8]].tolist() == [2, vk.NO_HIT, vk.NO_HIT] and r["hit_step"][0] == 2
    r = res[(("max_steps", 64), ("require_published", True))]
    assert r["hit_id"][0] == 1 and r["hit_id"][2] == 1 and r["hit_id"][10] == vk.NO_HIT    # the odd ids are published
    for key in ((("max_steps", 64), ("min_multiplicity", 6)), (("max_steps", 64), ("min_multiplicity", 0xFFFFFFFF))):
        assert res[key]["rays_hit"] == 0 and res[key]["cells_visited"] == int((res[key]["steps"][res[key]["steps"] >= 0] + 1).sum())
    for key in ((("max_steps", 64), ("start_margin", 22)), (("end_margin", 22), ("max_steps", 64)),
                (("end_margin", 1000), ("max_steps", 64), ("start_margin", 1000))):
        assert res[key]["rays_hit"] == 0 and res[key]["cells_visited"] == 0 and res[key]["rays_skipped"] == 6
    # flags never allocated: every entry reads 0
    got, _ = both(rec, None, O, P, 1.0, max_steps=64, require_published=True)
    assert got["rays_hit"] == 0 and got["cells_visited"] > 0


def synthetic_rays(rec, n, seed=0):
    """(origins, ends) float32[n, 3] for a map of test_vmap_recarve_cpu.synthetic_case: the origins around the cube of cells
    beside the world's origin; the ends at entries' points, at random points in and around the cube, 240 cells away, and
    -- one ray in sixteen -- NaN, Inf or a point beyond the cell range"""
    rng = np.random.default_rng(1700 + n + seed)
    M = len(rec["pixel"])
    O = rng.uniform(-0.6, 1.2, (n, 3)).astype(F)
    P = rng.uniform(-0.3, 0.9, (n, 3)).astype(F)
    if M:
        at = rng.random(n) < 0.6
        P[at] = rec["xyz"][rng.integers(0, M, int(at.sum()))]
    far = rng.random(n) < 0.1
    P[far] = (rng.uniform(0, 3, (int(far.sum()), 3)) + [0, 0, 12]).astype(F)
    bad = np.flatnonzero(np.arange(n) % 16 == 5)
    for j, i in enumerate(bad):
        (P if j % 2 else O)[i, j % 3] = (np.nan, np.inf, -np.inf, 3e6)[j % 4]
    return O, P


def synthetic_flags(M, seed=0):
    return (np.random.default_rng(77 + M + seed).random(M) < 0.5).astype(np.uint8)


FILTERS = (dict(), dict(min_multiplicity=2), dict(require_published=True), dict(min_multiplicity=3, require_published=True))


def test_synthetic_map_against_the_scalar_loop():
    rec, _ = synthetic_case(65, 65)
    flags = synthetic_flags(65)
    O, P = synthetic_rays(rec, 257)
    seen = set()
    for kw in (dict(), dict(start_margin=1, end_margin=1), dict(max_steps=200, min_multiplicity=2),
               dict(require_published=True, start_margin=3), dict(min_multiplicity=3, require_published=True, end_margin=2)):
        got, kind = both(rec, flags, O, P, VOXEL, **kw)
        seen |= set().union(*kind)
        assert got["rays_hit"] > 0 and got["rays_skipped"] >= 16 and got["rays_hit"] + got["rays_skipped"] < 257
    assert seen == set(KINDS), set(KINDS) - seen


@pytest.mark.parametrize("M", SYN_M)
def test_synthetic_inputs_cover_what_the_gpu_test_is_for(M):
    rec, _ = synthetic_case(M, 0)
    flags = synthetic_flags(M)
    O, P = synthetic_rays(rec, 1025)
    base = vk.cast_segments(rec, None, O, P, VOXEL)
    assert base["rays_skipped"] >= 64 and base["steps"].max() > 200     # long rays beside short ones in one wave
    if M == 0:
        assert base["rays_hit"] == 0
        return
    assert base["rays_hit"] > 0
    if M >= 65:
        # P1: a stricter filter never brings a hit closer; with a filter that nothing passes every walked ray is a miss
        hit0 = base["hit_id"] < (1 << 30)
        for kw in FILTERS[1:]:
            got = vk.cast_segments(rec, flags, O, P, VOXEL, **kw)
            hit = got["hit_id"] < (1 << 30)
            assert 0 < hit.sum() < hit0.sum() and not (hit & ~hit0).any()
            assert (got["hit_step"][hit] >= base["hit_step"][hit]).all() and (got["hit_step"][hit] > base["hit_step"][hit]).any()
            assert got["cells_visited"] > base["cells_visited"]
        for kw in (dict(min_multiplicity=4), dict(require_published=True)):
            got = vk.cast_segments(rec, np.zeros(M, np.uint8), O, P, VOXEL, **kw)
            assert got["rays_hit"] == 0 and (got["hit_id"][got["steps"] >= 0] == vk.NO_HIT).all()
            assert got["cells_visited"] == int((got["steps"][got["steps"] >= 0] + 1).sum())
        # the views: the camera that looks at the cube sees it, the one turned round sees nothing, no pose skips every ray
        at = vk.render(rec, flags, RENDER_K, POSE_AT, 33, 17, RHO_FAR, VOXEL)
        assert at["rays_hit"] > (33 * 17 // 8 if M > 65 else 8) and at["rays_skipped"] == 0 and (at["hit_rho"][at["hit_id"] < (1 << 30)] > 0).all()
        away = vk.render(rec, flags, RENDER_K, POSE_AWAY, 33, 17, RHO_FAR, VOXEL)
        assert away["rays_hit"] == 0 and away["rays_skipped"] == 0 and away["cells_visited"] > 0
        none = vk.render(rec, flags, RENDER_K, POSE_NAN, 33, 17, RHO_FAR, VOXEL)
        assert none["rays_skipped"] == 33 * 17 and (none["hit_id"] == vk.SKIPPED).all() and not none["hit_rho"].any()


# ---- P3: the render is the cast of the segments it defines, and hit_rho is the header's formula ---------------------------
@pytest.mark.parametrize("W,H", RENDER_SIZES)
def test_render_is_the_cast_of_its_segments(W, H):
    rec, _ = synthetic_case(2049, 0)
    flags = synthetic_flags(2049)
    for T in (POSE_AT, POSE_AWAY, POSE_NAN):
        for kw in (dict(), dict(min_multiplicity=2, require_published=True, start_margin=2)):
            got = vk.render(rec, flags, RENDER_K, T, W, H, RHO_FAR, VOXEL, **kw)
            # the segments, pixel by pixel: the centre, and np_pointset_pixel's statement written out for one pixel
            O, P = np.zeros((W * H, 3), F), np.zeros((W * H, 3), F)
            t = T.reshape(3, 4)
            with np.errstate(all="ignore"):
                for y in range(H):
                    for x in range(W):
                        Z = F(1) / F(RHO_FAR)
                        X, Y = Z * (F(x) - RENDER_K[2]) / RENDER_K[0], Z * (F(y) - RENDER_K[3]) / RENDER_K[1]
                        c = carve_np.camera_centre(T)
                        O[y * W + x] = c
                        P[y * W + x] = [((t[0, i] * X + t[1, i] * Y) + t[2, i] * Z) + c[i] * F(1) for i in range(3)]
            exp = scalar_cast(rec, flags, O, P, VOXEL, **kw)
            for f in ARRAYS:
                np.testing.assert_array_equal(got[f].reshape(-1), exp[f])
            assert {f: got[f] for f in vk.OUTS} == {f: exp[f] for f in vk.OUTS}
            rho = np.zeros(W * H, F)
            with np.errstate(all="ignore"):
                for i, e in enumerate(exp["hit_id"]):
                    if e < (1 << 30):
                        X, Y, Z = rec["xyz"][e]
                        rho[i] = F(1) / (((T[8] * X + T[9] * Y) + T[10] * Z) + T[11])
            assert got["hit_rho"].dtype == F and got["hit_rho"].tobytes() == rho.reshape(H, W).tobytes()
            assert got["hit_id"].shape == got["hit_step"].shape == got["hit_rho"].shape == (H, W)


# ---- P2: the log's rays on the golden fixtures, against sdm_vmap_recarve's statement ---------------------------------------
def log_rays(vm, ol, tags, Tcw):
    """(origins, ends, entry) of the log's pairs: from the centre of the pair's pose to the xyz of the pair's entry"""
    centre = {int(t): carve_np.camera_centre(T) for t, T in zip(tags, np.asarray(Tcw, F).reshape(-1, 12))}
    O = np.array([centre[int(t)] for t in ol.tag], F).reshape(-1, 3)
    return O, vm.rec["xyz"][ol.entry.astype(np.int64)], ol.entry.astype(np.int64)


# (rays_hit, cells_visited) at end_margin m + 1, then at end_margin 0: what the restatement gives on the CPU
PINNED = {"plane_160x120_n7": (0, 2572636, 8824, 2590284), "plane_64x48_n7": (0, 841822, 2880, 847582),
          "plane_96x80_n20": (0, 800897, 2704, 806305), "strip_roll_160x120_n7": (25, 2576889, 8937, 2594683)}


@pytest.mark.parametrize("name", gu.fixture_names())
def test_log_rays_against_the_recarve(name):
    vm, ol, carved, (tags, Tcw), T = fixture_kf0(name)
    rec = vm.rec
    O, P, entry = log_rays(vm, ol, tags, Tcw)
    re = vr.recarve((vm.keys, vm.ids), rec["xyz"], ol.entry, ol.tag, tags, Tcw, EQ_VOXEL, EQ_MARGIN, EQ_STEPS)
    assert (re["rays_total"], re["cells_visited"], re["cells_hit"]) == RECARVE_PINNED[name][1:4]
    inner = vk.cast_segments(rec, None, O, P, EQ_VOXEL, 0, EQ_MARGIN + 1, EQ_STEPS)
    whole = vk.cast_segments(rec, None, O, P, EQ_VOXEL, 0, 0, EQ_STEPS)
    print(name, {f: inner[f] for f in vk.OUTS}, {f: whole[f] for f in vk.OUTS})
    assert inner["rays_total"] == re["rays_total"] and inner["rays_skipped"] == re["rays_skipped"] == 0
    assert (inner["rays_hit"] == 0) == (re["cells_hit"] == 0) and inner["rays_hit"] <= re["cells_hit"]
    assert inner["cells_visited"] <= re["cells_visited"]
    if re["cells_hit"] == 0:
        assert inner["cells_visited"] == re["cells_visited"]    # no early exit: the same cells
    # end_margin 0: every walked ray hits, and it hits its own entry exactly if nothing stood before the end cell
    assert whole["rays_hit"] == whole["rays_total"]
    early = inner["hit_id"] != vk.NO_HIT
    np.testing.assert_array_equal(whole["hit_id"] == entry, whole["hit_step"] == whole["steps"])
    assert (whole["hit_step"][~early] >= whole["steps"][~early] - EQ_MARGIN).all()   # (the cells that only end_margin 0 examines)
    for f in ARRAYS:
        np.testing.assert_array_equal(whole[f][early], inner[f][early])
    assert (inner["rays_hit"], inner["cells_visited"], whole["rays_hit"], whole["cells_visited"]) == PINNED[name]
    # the scalar loop agrees with the pinned totals: every ray of the smallest fixture, every eighth of the others
    pick = np.arange(len(O)) if name == "plane_64x48_n7" else np.arange(0, len(O), 8)
    for got, em in ((inner, EQ_MARGIN + 1), (whole, 0)):
        exp = scalar_cast(rec, None, O[pick], P[pick], EQ_VOXEL, 0, em, EQ_STEPS)
        for f in ARRAYS:
            np.testing.assert_array_equal(got[f][pick], exp[f])
        if len(pick) == len(O):
            assert {f: got[f] for f in vk.OUTS} == {f: exp[f] for f in vk.OUTS}
