"""CPU: tests/carve_np.py (the NumPy statement of sdm_extract_points_voxel_freespace's counts) against a second
formulation -- a scalar Python walk, ray by ray -- on random clouds and on crafted rays, and how many kept points of the
golden fixtures another camera sees through (computed on the CPU: support_np, voxel_np, voxcam_np, the fixture cloud)."""
import numpy as np
import pytest

import carve_np
import golden_util as gu
import voxcam_np
import voxel_np
from test_voxcam_cpu import fixture_case

F = np.float32
LIM = 1 << 20


def scalar_freespace(xyz, cam_offsets, cam_slots, centres, voxel_size, end_margin, max_steps):
    """the semantics of include/sdm_c.h, ray by ray, cell by cell -> (crossings, skipped, visited, per-ray end cells)"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    voxel = F(voxel_size)
    inv = F(1.0) / voxel
    table = {}
    with np.errstate(all="ignore"):
        for j, p in enumerate(xyz):
            c = [np.floor(p[a] * inv) for a in range(3)]
            if all(-LIM <= v < LIM for v in c):
                assert tuple(int(v) for v in c) not in table
                table[tuple(int(v) for v in c)] = j
    crossings = np.zeros(len(xyz), np.uint32)
    skipped = visited = 0
    ends = []
    for k in range(len(xyz)):
        for e in range(int(cam_offsets[k]), int(cam_offsets[k + 1])):
            O, P = np.asarray(centres[int(cam_slots[e])], np.float32), xyz[k]
            with np.errstate(all="ignore"):
                fO = [np.floor(O[a] * inv) for a in range(3)]
                fP = [np.floor(P[a] * inv) for a in range(3)]
                if not all(-LIM <= v < LIM for v in fO + fP):
                    skipped += 1
                    ends.append(None)
                    continue
                cO, cP = [int(v) for v in fO], [int(v) for v in fP]
                r = [abs(cP[a] - cO[a]) for a in range(3)]
                N = sum(r)
                if N > max_steps:
                    skipped += 1
                    ends.append(None)
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
                for s in range(N):
                    if s <= N - 1 - end_margin:
                        visited += 1
                        j = table.get(tuple(cur))
                        if j is not None:
                            crossings[j] += 1
                    best = None
                    for a in range(3):  # never reads an axis with r = 0
                        if r[a] > 0 and (best is None or tMax[a] < tMax[best]):
                            best = a
                    cur[best] += step[best]
                    r[best] -= 1
                    tMax[best] = tMax[best] + tDel[best]
                ends.append((tuple(cur), tuple(cP)))
    return crossings, skipped, visited, ends


def both(xyz, offs, cs, centres, voxel, end_margin, max_steps):
    got = carve_np.freespace(xyz, offs, cs, centres, voxel, end_margin, max_steps)
    cr, sk, vis, ends = scalar_freespace(xyz, offs, cs, centres, voxel, end_margin, max_steps)
    assert got["crossings"].dtype == np.uint32 and len(got["crossings"]) == len(np.asarray(xyz).reshape(-1, 3))
    np.testing.assert_array_equal(got["crossings"], cr)
    assert (got["rays_total"], got["rays_skipped"], got["cells_visited"]) == (len(cs), sk, vis)
    walked = got["steps"] >= 0
    assert int((~walked).sum()) == sk
    np.testing.assert_array_equal(got["end"][walked], got["end_cell"][walked])  # every walked ray ends in cP
    for e, pair in enumerate(ends):
        assert (pair is None) == (not walked[e])
        if pair is not None:
            assert pair[0] == pair[1] == tuple(got["end"][e])
    return got


def one_per_voxel(xyz, voxel):
    """a cloud thinned to one mergeable point per voxel (what a merged cloud is)"""
    c, ok = voxel_np.cells(xyz, voxel)
    key = carve_np.pack(np.where(ok[:, None], c, 0))
    _, first = np.unique(key, return_index=True)
    keep = np.zeros(len(xyz), bool)
    keep[first] = True
    return xyz[keep | ~ok]


@pytest.mark.parametrize("seed", range(4))
def test_random_clouds(seed):
    rng = np.random.default_rng(seed)
    voxel = (0.05, 0.11, 0.02, 0.3)[seed]
    n_cam = 5
    pts = rng.uniform(-1, 1, (150, 3)).astype(np.float32)
    pts[:40] = (rng.uniform(0.2, 0.9, (40, 1)) * np.array([[0.9, 0.7, 0.8]])).astype(np.float32)  # a line the rays run along
    if seed == 1:
        pts[50] = np.nan  # unmergeable kept points: their rays are skipped, their counter stays 0
        pts[51] = [np.inf, 0, 0]
        pts[52] = [3e7, 0, 0]
    xyz = one_per_voxel(pts, voxel)
    M = len(xyz)
    centres = {7 * s + 3: rng.uniform(-1.2, 1.2, 3).astype(np.float32) for s in range(n_cam)}
    centres[3] = np.zeros(3, np.float32)
    ids = np.array(sorted(centres))
    lens = rng.integers(1, n_cam + 1, M)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cs = np.concatenate([np.sort(rng.permutation(ids)[:ln]) for ln in lens]).astype(np.int32)
    for end_margin, max_steps in ((0, 4096), (1, 4096), (2, 30), (50, 4096)):
        got = both(xyz, offs, cs, centres, voxel, end_margin, max_steps)
        if end_margin == 0 and max_steps == 4096:
            assert got["crossings"].sum() > 0
        if max_steps == 30 and voxel < 0.1:
            assert 0 < got["rays_skipped"] < len(cs)
    if seed == 1:
        bad = ~voxel_np.cells(xyz, voxel)[1]
        assert bad.sum() == 3 and got["rays_skipped"] >= np.diff(offs)[bad].sum() and (got["crossings"][bad] == 0).all()


def lists(per_point):
    offs = np.concatenate([[0], np.cumsum([len(c) for c in per_point])]).astype(np.int64)
    return offs, np.array([s for c in per_point for s in c], np.int32)


def test_crafted_rays():
    O0 = np.array([0.5, 0.5, 0.5], F)
    # exact three- and two-axis ties (d = (2, 2, 2) and (2, 2, 0), voxel 1): x first, then y, then z
    xyz = np.array([[2.5, 2.5, 2.5], [1.5, 0.5, 0.5], [1.5, 1.5, 0.5], [1.5, 1.5, 1.5], [2.5, 1.5, 1.5], [2.5, 2.5, 1.5],
                    [2.5, 2.5, 0.5], [0.5, 1.5, 0.5]], F)
    offs, cs = lists([[0]] * len(xyz))
    got = both(xyz, offs, cs, {0: O0}, 1.0, 0, 64)
    # the ray to point 0 visits (0,0,0) (1,0,0) (1,1,0) (1,1,1) (2,1,1) (2,2,1); the one to point 6 (0,0,0) (1,0,0) (1,1,0)
    # (2,1,0); to point 4 (0,0,0) (1,0,0) (1,1,0) (1,1,1); to point 5 (0,0,0) (1,0,0) (1,1,0) (1,1,1) (2,1,1); points 2 and 3
    # are reached through (1,0,0) and (1,0,0) (1,1,0)
    np.testing.assert_array_equal(got["crossings"], [0, 6, 5, 3, 2, 1, 0, 0])
    assert got["steps"].tolist() == [6, 1, 2, 3, 4, 5, 4, 1] and got["cells_visited"] == 26
    assert both(xyz, offs, cs, {0: O0}, 1.0, 1, 64)["crossings"].tolist() == [0, 5, 4, 2, 1, 0, 0, 0]
    # axis-parallel rays, on both sides of zero, towards negative cells
    xyz = np.array([[-3.5, 0.5, 0.5], [-1.5, 0.5, 0.5], [0.5, -2.5, 0.5], [0.5, -0.5, 0.5], [0.5, 0.5, 3.5], [0.5, 0.5, 1.5]], F)
    offs, cs = lists([[0]] * len(xyz))
    got = both(xyz, offs, cs, {0: O0}, 1.0, 0, 64)
    assert got["crossings"].tolist() == [0, 1, 0, 1, 0, 1] and got["steps"].tolist() == [4, 2, 3, 1, 3, 1]
    # origin and end in one cell (N = 0): walked, nothing counted
    xyz = np.array([[0.75, 0.25, 0.5], [5.5, 0.5, 0.5]], F)
    offs, cs = lists([[0], [0]])
    got = both(xyz, offs, cs, {0: O0}, 1.0, 0, 64)
    assert got["steps"].tolist() == [0, 5] and got["rays_skipped"] == 0 and got["cells_visited"] == 5
    assert got["crossings"].tolist() == [1, 0]  # the second ray starts in the first point's voxel
    # N == max_steps walks, max_steps + 1 skips
    assert both(xyz, offs, cs, {0: O0}, 1.0, 0, 5)["rays_skipped"] == 0
    got = both(xyz, offs, cs, {0: O0}, 1.0, 0, 4)
    assert got["rays_skipped"] == 1 and got["crossings"].tolist() == [0, 0] and got["cells_visited"] == 0
    # end_margin >= N: nothing counted, the ray still walked
    for margin in (5, 6, 1000):
        got = both(xyz, offs, cs, {0: O0}, 1.0, margin, 64)
        assert got["rays_skipped"] == 0 and got["cells_visited"] == 0 and got["crossings"].sum() == 0
    # an origin cell out of range, NaN and +-Inf poses: skipped
    bad = {0: O0, 1: np.array([3e6, 0, 0], F), 2: np.array([np.nan, 0, 0], F), 3: np.array([0, np.inf, 0], F),
           4: np.array([0, 0, -np.inf], F), 5: np.array([-1048576.5, 0, 0], F), 6: np.array([-1048576.0, 0.5, 0.5], F)}
    offs, cs = lists([[0, 1, 2, 3, 4, 5, 6], [0]])
    got = both(xyz, offs, cs, bad, 1.0, 0, MAXS)
    assert got["rays_skipped"] == 6 and got["steps"].tolist() == [0, -1, -1, -1, -1, -1, -1, 5]
    assert both(xyz, offs, cs, bad, 1.0, 0, carve_np.MAX_STEPS)["rays_skipped"] == 6  # (camera 6 is 2^20 steps away)
    edge = np.array([[-1048572.5, 0.5, 0.5], [-1048574.5, 0.5, 0.5]], F)  # the cell -2^20 itself is in range
    offs, cs = lists([[5, 6], [6]])
    got = both(edge, offs, cs, bad, 1.0, 0, MAXS)
    assert got["steps"].tolist() == [-1, 3, 1] and got["crossings"].tolist() == [0, 1]
    # a |d_a| so small that tDel overflows: two cells apart in x by 1e-42 (voxel 1, the boundary between them), and a d_a
    # whose tMax is Inf / NaN: the integers still drive the walk into cP
    tiny = np.array([[1.0, 7.5, 0.5], [1.0, 0.5, 0.5], [np.float32(1e-42) + F(1.0), 0.5, 3.5]], F)
    org = {0: np.array([np.nextafter(F(1.0), F(0.0)), 0.5, 0.5], F)}
    offs, cs = lists([[0], [0], [0]])
    with np.errstate(all="ignore"):
        assert np.isinf(F(1.0) / abs(tiny[0, 0] - org[0][0]) * F(1e35))
    both(tiny, offs, cs, org, 1.0, 0, 64)
    both(tiny * F(1e-3), offs, cs, {0: org[0] * F(1e-3)}, 1e-3, 0, 64)
    den = {0: np.array([F(1e-45), 0.5, 0.5], F)}  # d_x denormal-sized: tDel = voxel / |d| = Inf
    pts = np.array([[-1e-45, 3.5, 0.5], [0.0, 1.5, 0.5]], F)
    offs, cs = lists([[0], [0]])
    got = both(pts, offs, cs, den, 1.0, 0, 64)
    assert got["steps"].tolist() == [4, 1]


MAXS = 4096


def fixture_rays(name, voxel=0.02):
    g, xyz, sigma, offs, support, rows = fixture_case(name)
    refs = np.arange(g["n_kf"])
    kept, _, rep, _ = voxel_np.voxel_merge(xyz, sigma, voxel, offs)
    co, cs = voxcam_np.voxel_cameras(support, offs, refs, rows, rep, len(kept))
    centres = {int(k): carve_np.camera_centre(g["Tcw"][k]) for k in refs}
    return xyz[kept], co, cs, centres


@pytest.mark.parametrize("name", gu.fixture_names())
def test_golden_fixtures_are_seen_through(name):
    pts, co, cs, centres = fixture_rays(name)
    crossed = []
    for margin in (0, 1, 2):
        got = carve_np.freespace(pts, co, cs, centres, 0.02, margin, MAXS)
        walked = got["steps"] >= 0
        np.testing.assert_array_equal(got["end"][walked], got["end_cell"][walked])
        assert got["rays_skipped"] == 0 and got["rays_total"] == len(cs)
        assert got["cells_visited"] == int(np.maximum(got["steps"] - margin, 0).sum())
        crossed.append(int((got["crossings"] > 0).sum()))
        if margin == 0:
            print("%s: E %d, longest N %d, mean N %.1f" % (name, len(cs), got["steps"].max(), got["steps"].mean()))
    print("%s: kept points with crossings > 0 at end_margin 0 / 1 / 2: %s" % (name, crossed))
    assert crossed[0] >= 100
    if name.startswith("strip"):
        assert crossed[1] >= 100
    assert crossed[0] > crossed[1] > crossed[2]


def test_fixture_subset_against_the_scalar_walk():
    """the two formulations on real geometry: the first rays of one fixture"""
    pts, co, cs, centres = fixture_rays("plane_64x48_n7")
    m = 60
    both(pts[:m], co[:m + 1], cs[:co[m]], centres, 0.02, 1, MAXS)
