"""CPU: tests/vmap_carve_np.py (the NumPy statement of sdm_vmap_carve's evidence) against three references -- a scalar
Python walk, ray by ray, exactly as include/sdm_c.h words it; tests/carve_np.py (the merged statement of
sdm_extract_points_voxel_freespace) in the one case where both are defined alike; and additivity over splits and orders on
a fixed map -- plus the totals of the golden fixtures the GPU test relies on (computed on the CPU)."""
import numpy as np
import pytest

import carve_np
import golden_util as gu
import vmap_carve_np as vc
import vmap_np
import voxel_np
from test_carve_cpu import one_per_voxel
from test_voxcam_cpu import fixture_case

F = np.float32
LIM = 1 << 20
SLOTS = [3, 5, 9]
# repeated neighbours, a neighbour equal to the row's own slot, a slot that is nobody's own (7)
NBRS = np.array([[5, 5, 3, 9], [3, 9, 9, 7], [9, 3, 5, 3]], np.int32)


def cloud_of(xyz):
    T = len(xyz)
    return {"xyz": np.asarray(xyz, F), "pixel": np.arange(T, dtype=np.uint32),
            "rho_sigma": np.stack([np.ones(T, F), np.full(T, 0.01, F)], 1), "intensity": np.zeros(T, np.uint8)}


def map_of(xyz, voxel):
    vm = vmap_np.VoxelMap(voxel)
    vm.integrate(cloud_of(xyz), np.zeros(len(xyz), np.int32))
    return vm


def scalar_carve(vm, xyz, row, support, slots, nbrs, centres, voxel_size, end_margin, max_steps):
    """the semantics of include/sdm_c.h, point by point, camera by camera, cell by cell"""
    voxel = F(voxel_size)
    inv = F(1.0) / voxel
    entry = {}
    for key, e in zip(vm.keys.tolist(), vm.ids.tolist()):
        entry[((key >> 42) - LIM, ((key >> 21) & (2 * LIM - 1)) - LIM, (key & (2 * LIM - 1)) - LIM)] = e
    crossings, ends = np.zeros(vm.M, np.uint64), np.zeros(vm.M, np.uint64)
    tot = dict.fromkeys(vc.TOTALS, 0)
    tot["plain_total"] = len(xyz)
    for g, P in enumerate(np.asarray(xyz, F).reshape(-1, 3)):
        i = int(row[g])
        cams = {int(slots[i])}
        if nbrs is not None:
            cams |= {int(nbrs[i][j]) for j in range(len(nbrs[i])) if (int(support[g]) >> j) & 1}
        for s in sorted(cams):
            tot["rays_total"] += 1
            O = np.asarray(centres[s], F)
            with np.errstate(all="ignore"):
                fO = [np.floor(O[a] * inv) for a in range(3)]
                fP = [np.floor(P[a] * inv) for a in range(3)]
                if not all(-LIM <= v < LIM for v in fO + fP):
                    tot["rays_skipped"] += 1
                    continue
                cO, cP = [int(v) for v in fO], [int(v) for v in fP]
                r = [abs(cP[a] - cO[a]) for a in range(3)]
                N = sum(r)
                if N > max_steps:
                    tot["rays_skipped"] += 1
                    continue
                step = [(cP[a] > cO[a]) - (cP[a] < cO[a]) for a in range(3)]
                tMax, tDel = [None] * 3, [None] * 3
                for a in range(3):
                    if r[a] > 0:
                        d = P[a] - O[a]
                        bnd = F(cO[a] + (1 if step[a] > 0 else 0)) * voxel
                        tMax[a] = (bnd - O[a]) / d
                        tDel[a] = voxel / abs(d)
                cur = list(cO)
                for k in range(N):
                    if k <= N - 1 - end_margin:
                        tot["cells_visited"] += 1
                        e = entry.get(tuple(cur))
                        if e is not None:
                            crossings[e] += 1
                            tot["cells_hit"] += 1
                    best = None
                    for a in range(3):  # never reads an axis with r = 0
                        if r[a] > 0 and (best is None or tMax[a] < tMax[best]):
                            best = a
                    cur[best] += step[best]
                    r[best] -= 1
                    tMax[best] = tMax[best] + tDel[best]
                assert cur == cP
                e = entry.get(tuple(cP))
                if e is not None:
                    ends[e] += 1
                    tot["ends_hit"] += 1
    return crossings, ends, tot


def both(vm, xyz, row, support, slots, nbrs, centres, voxel, end_margin, max_steps):
    got = vc.carve((vm.keys, vm.ids), xyz, row, support, slots, nbrs, centres, voxel, end_margin, max_steps)
    cr, en, tot = scalar_carve(vm, xyz, row, support, slots, nbrs, centres, voxel, end_margin, max_steps)
    assert got["crossings"].dtype == np.uint64 and got["ends"].dtype == np.uint64 and len(got["crossings"]) == vm.M
    np.testing.assert_array_equal(got["crossings"], cr)
    np.testing.assert_array_equal(got["ends"], en)
    assert {f: got[f] for f in vc.TOTALS} == tot
    assert got["cells_hit"] == int(cr.sum()) and got["ends_hit"] == int(en.sum())
    return got


def random_case(seed, voxel):
    """(map, xyz, row, support, centres): random points plus points on cell faces, on both sides of zero, non-finite and
    out-of-range ones; rays along the axes and along exact diagonals from camera 3 (tMax ties)"""
    rng = np.random.default_rng(seed)
    v = F(voxel)
    centres = {3: np.array([0.5, 0.5, 0.5], F) * v, 5: rng.uniform(-1, 1, 3).astype(F), 7: rng.uniform(-1, 1, 3).astype(F),
               9: np.array([-2.5, 1.5, -0.5], F) * v}
    pts = rng.uniform(-1, 1, (90, 3)).astype(F)
    pts[:20] = np.round(pts[:20] / v) * v                      # on cell faces (corners), both signs
    k = np.arange(1, 11, dtype=F)[:, None]
    diag = centres[3] + k * v * np.array([[1, 1, 1]], F)       # exact three-axis ties from camera 3
    diag2 = centres[3] + k * v * np.array([[-1, 1, 0]], F)     # two-axis ties, towards negative x
    axis = centres[3] + k * v * np.array([[0, 0, -1]], F)      # axis-parallel, towards negative z
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [3e7, 0, 0]], F)
    xyz = np.concatenate([diag, diag2, axis, pts, bad]).astype(F)
    T = len(xyz)
    row = rng.integers(0, 3, T)
    row[:30] = 0  # the crafted rays belong to slot 3: its own camera is the one they are exact from
    order = np.argsort(row, kind="stable")  # plain order: slot by slot
    support = rng.integers(0, 16, T).astype(np.uint64)
    dense = rng.uniform(-1.2, 1.2, (900, 3)).astype(F)  # the map: most cells of the region, the carved points' among them
    vm = map_of(np.concatenate([dense, xyz[:60]]), voxel)
    return vm, xyz[order], row[order], support, centres


@pytest.mark.parametrize("seed", range(3))
def test_random_clouds_against_the_scalar_walk(seed):
    voxel = (0.25, 0.11, 0.5)[seed]
    vm, xyz, row, support, centres = random_case(seed, voxel)
    seen_skip = False
    for end_margin, max_steps in ((0, 4096), (1, 4096), (2, 9), (1000, 4096)):
        got = both(vm, xyz, row, support, SLOTS, NBRS, centres, voxel, end_margin, max_steps)
        assert got["rays_skipped"] >= 4  # the non-finite and out-of-range points
        assert got["ends_hit"] > 0
        if end_margin == 0:
            assert got["cells_hit"] > 100
        if end_margin == 1000:
            assert got["cells_visited"] == 0 and got["crossings"].sum() == 0 and got["ends_hit"] > 0
        seen_skip |= max_steps == 9 and got["rays_skipped"] > 4
    assert seen_skip or voxel == 0.5
    # C(g) is a set: the rays are those of the distinct cameras
    g_of, s_of = vc.rays_of(row, support, SLOTS, NBRS)
    assert len(set(zip(g_of.tolist(), s_of.tolist()))) == len(g_of)
    # no neighbour table: the observing camera alone
    own = both(vm, xyz, row, None, SLOTS, None, centres, voxel, 1, 4096)
    assert own["rays_total"] == len(xyz)
    # a non-finite centre skips every ray of that camera, the others are walked
    broken = dict(centres)
    broken[5] = np.array([np.nan, 0, 0], F)
    got = both(vm, xyz, row, support, SLOTS, NBRS, broken, voxel, 1, 4096)
    assert got["rays_skipped"] >= int((got["ray_slot"] == 5).sum()) > 0 and got["rays_skipped"] < got["rays_total"]
    broken[5] = np.array([0, -np.inf, 0], F)
    both(vm, xyz, row, support, SLOTS, NBRS, broken, voxel, 0, 4096)


def test_crafted_rays():
    """ties, axis-parallel rays, N = 0, N == max_steps and max_steps + 1, end_margin beyond N, the camera's own cell"""
    O0 = np.array([0.5, 0.5, 0.5], F)
    pts = np.array([[2.5, 2.5, 2.5], [1.5, 0.5, 0.5], [1.5, 1.5, 0.5], [1.5, 1.5, 1.5], [2.5, 1.5, 1.5], [2.5, 2.5, 1.5],
                    [2.5, 2.5, 0.5], [0.5, 1.5, 0.5], [0.75, 0.25, 0.5], [-3.5, 0.5, 0.5], [0.5, 0.5, 5.5]], F)
    vm = map_of(pts, 1.0)  # one entry per point: id = g
    assert vm.M == len(pts)
    row = np.zeros(len(pts), np.int64)
    got = both(vm, pts, row, None, [0], None, {0: O0}, 1.0, 0, 64)
    # the walks are tests/test_carve_cpu.py's: the ray to point 0 visits (0,0,0) (1,0,0) (1,1,0) (1,1,1) (2,1,1) (2,2,1), ...
    # and every ray of the camera counts its own cell s = 0, which holds entry 8 -- except the ray to entry 8 itself (N = 0)
    assert got["steps"].tolist() == [6, 1, 2, 3, 4, 5, 4, 1, 0, 4, 5]
    assert got["crossings"].tolist() == [0, 6, 5, 3, 2, 1, 0, 0, 10, 0, 0]
    assert got["ends"].tolist() == [1] * len(pts) and got["ends_hit"] == len(pts)
    got = both(vm, pts, row, None, [0], None, {0: O0}, 1.0, 1, 64)
    assert got["crossings"].tolist() == [0, 5, 4, 2, 1, 0, 0, 0, 8, 0, 0]  # (the two N = 1 rays count nothing now)
    assert both(vm, pts, row, None, [0], None, {0: O0}, 1.0, 0, 6)["rays_skipped"] == 0      # N == max_steps walks
    got = both(vm, pts, row, None, [0], None, {0: O0}, 1.0, 0, 5)                             # N == max_steps + 1 skips
    assert got["rays_skipped"] == 1 and got["steps"][0] == -1 and got["ends"][0] == 0
    for margin in (6, 7, 1000):  # beyond every N: nothing is crossed, every walked ray still ends
        got = both(vm, pts, row, None, [0], None, {0: O0}, 1.0, margin, 64)
        assert got["cells_visited"] == 0 and got["crossings"].sum() == 0 and got["ends_hit"] == len(pts)
    # a self neighbour and a repeated one add nothing; a real one adds its rays
    nb = np.array([[0, 0, 4, 4]], np.int32)
    sup = np.full(len(pts), 0b0011, np.uint64)
    cen = {0: O0, 4: np.array([0.5, 4.5, 0.5], F)}
    same = both(vm, pts, row, sup, [0], nb, cen, 1.0, 0, 64)
    assert same["rays_total"] == len(pts)
    sup[:] = 0b1100
    more = both(vm, pts, row, sup, [0], nb, cen, 1.0, 0, 64)
    assert more["rays_total"] == 2 * len(pts) and more["ends"].tolist() == [2] * len(pts)
    sup[:] = 0b0100
    assert both(vm, pts, row, sup, [0], nb, cen, 1.0, 0, 64)["crossings"].tolist() == more["crossings"].tolist()


@pytest.mark.parametrize("seed", range(3))
def test_against_the_merged_statement(seed):
    """one plain point per voxel, a map from one integrate of it, camera lists equal to C(g): crossings entry for entry"""
    rng = np.random.default_rng(40 + seed)
    voxel = (0.05, 0.11, 0.3)[seed]
    pts = rng.uniform(-1, 1, (150, 3)).astype(F)
    pts[:40] = (rng.uniform(0.2, 0.9, (40, 1)) * np.array([[0.9, 0.7, 0.8]])).astype(F)  # a line the rays run along
    xyz = one_per_voxel(pts, voxel)
    T = len(xyz)
    vm = map_of(xyz, voxel)
    assert vm.M == T  # every point is mergeable and alone in its voxel: entry id = g
    row = np.sort(rng.integers(0, 3, T))
    support = rng.integers(0, 16, T).astype(np.uint64)
    centres = {s: rng.uniform(-1.2, 1.2, 3).astype(F) for s in (3, 5, 7, 9)}
    centres[3] = np.zeros(3, F)  # (the line passes through it)
    g_of, s_of = vc.rays_of(row, support, SLOTS, NBRS)
    order = np.lexsort((s_of, g_of))
    offs = np.concatenate([[0], np.cumsum(np.bincount(g_of, minlength=T))]).astype(np.int64)
    for end_margin, max_steps in ((0, 4096), (1, 4096), (2, 30)):
        got = vc.carve((vm.keys, vm.ids), xyz, row, support, SLOTS, NBRS, centres, voxel, end_margin, max_steps)
        ref = carve_np.freespace(xyz, offs, s_of[order].astype(np.int32), centres, voxel, end_margin, max_steps)
        np.testing.assert_array_equal(got["crossings"], ref["crossings"].astype(np.uint64))
        assert (got["rays_total"], got["rays_skipped"], got["cells_visited"]) == \
            (ref["rays_total"], ref["rays_skipped"], ref["cells_visited"])
        assert got["cells_hit"] == int(ref["crossings"].sum())
        np.testing.assert_array_equal(got["ends"], np.bincount(g_of[order][ref["steps"] >= 0], minlength=T))
        if end_margin == 0:
            assert got["crossings"].sum() > 0


def test_additivity_over_splits_and_orders():
    vm, xyz, row, support, centres = random_case(7, 0.25)

    def call(rows):
        sel = np.isin(row, rows)
        remap = np.cumsum(np.isin(np.arange(3), rows)) - 1
        return vc.carve((vm.keys, vm.ids), xyz[sel], remap[row[sel]], support[sel], [SLOTS[i] for i in rows], NBRS[rows], centres,
                        0.25, 1, 4096)

    def total(calls):
        out = {"crossings": np.zeros(vm.M, np.uint64), "ends": np.zeros(vm.M, np.uint64), **dict.fromkeys(vc.TOTALS, 0)}
        for c in calls:
            for f in out:
                out[f] = out[f] + c[f]
        return out

    whole = total([call([0, 1, 2])])
    assert whole["cells_hit"] > 100
    for split in ([[0, 1], [2]], [[2], [0, 1]], [[1], [2], [0]], [[0], [1, 2]]):
        got = total([call(rows) for rows in split])
        for f in whole:
            assert np.array_equal(got[f], whole[f]), (split, f)


def fixture_sequence(name, voxel=0.02, end_margin=1, max_steps=4096):
    """one integrate-then-carve per keyframe (sigma gate 0.3, the checked rho, the fixtures' short neighbour rows):
    the summed totals, and the counters over the final entries"""
    g, xyz, sigma, offs, support, rows = fixture_case(name)
    T = len(xyz)
    cloud = {"xyz": xyz, "pixel": np.arange(T, dtype=np.uint32), "rho_sigma": np.stack([np.ones(T, F), sigma], 1),
             "intensity": np.zeros(T, np.uint8)}
    centres = {k: carve_np.camera_centre(g["Tcw"][k]) for k in range(g["n_kf"])}
    vm = vmap_np.VoxelMap(voxel)
    tot = dict.fromkeys(vc.TOTALS, 0)
    crossings, ends = np.zeros(0, np.uint64), np.zeros(0, np.uint64)
    for k in range(g["n_kf"]):
        a, b = offs[k], offs[k + 1]
        vm.integrate({f: v[a:b] for f, v in cloud.items()}, np.full(b - a, k, np.int32))
        got = vc.carve((vm.keys, vm.ids), xyz[a:b], np.zeros(b - a, np.int64), support[a:b], [k], rows[k:k + 1], centres, voxel,
                       end_margin, max_steps)
        grow = vm.M - len(crossings)
        crossings = np.concatenate([crossings, np.zeros(grow, np.uint64)]) + got["crossings"]
        ends = np.concatenate([ends, np.zeros(grow, np.uint64)]) + got["ends"]
        for f in vc.TOTALS:
            tot[f] += got[f]
    return tot, crossings, ends


# (plain_total, rays_total, cells_visited, cells_hit = crossings.sum(), ends_hit): what the restatement gives on the CPU
PINNED = {"plane_160x120_n7": (14150, 56313, 4178452, 2609, 56313), "plane_64x48_n7": (4535, 17979, 1279018, 755, 17979),
          "plane_96x80_n20": (16287, 64275, 4835126, 2050, 64275), "strip_roll_160x120_n7": (16441, 64420, 4512342, 12955, 64420)}


@pytest.mark.parametrize("name", gu.fixture_names())
def test_golden_fixtures_are_not_vacuous(name):
    tot, crossings, ends = fixture_sequence(name)
    print(name, tot, "entries crossed", int((crossings > 0).sum()))
    assert tot["rays_skipped"] == 0 and tot["cells_hit"] > 0
    assert int(crossings.sum()) == tot["cells_hit"] and int(ends.sum()) == tot["ends_hit"]
    assert tot["ends_hit"] == tot["rays_total"] > tot["plain_total"]  # a carve after its integrate: every end cell has an entry
    assert (tot["plain_total"], tot["rays_total"], tot["cells_visited"], tot["cells_hit"], tot["ends_hit"]) == PINNED[name]
