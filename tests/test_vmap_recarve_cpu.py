"""CPU: tests/vmap_recarve_np.py (the NumPy statement of sdm_vmap_recarve) -- tied to a scalar loop over the (entry, tag)
pairs on small hand-made maps, its properties (additivity over log splits and orders, reset, the empty table, every walked
ray ends in its own entry), the hostile poses and rays, and the equivalence with sdm_vmap_carve's statement where every
multiplicity is 1: keyframe 0 of every golden fixture, integrated, observed and carved alone at voxel 0.005.  The synthetic
inputs of tests/test_gpu_vmap_recarve.py are defined here."""
import functools

import numpy as np
import pytest

import carve_np
import golden_util as gu
import vmap_carve_np as vc
import vmap_import_np as vi
import vmap_np
import vmap_obs_np as vo
import vmap_recarve_np as vr
from test_vmap_carve_cpu import cloud_of, scalar_carve
from test_vmap_repose_cpu import VOXEL, pose
from test_voxcam_cpu import fixture_case

F = np.float32
LOG_TAGS = 12                       # the log's tags are 0 .. 11; 10 and 11 are in no table
TAG_GOOD, TAG_NAN, TAG_INF, TAG_FAR = 5, 7, 8, 9
# (entries, pairs) of the synthetic maps: the wave edges, one pair, nothing, several workgroups
SYN_CASES = ((0, 0), (1, 1), (63, 63), (64, 64), (65, 65), (2049, 5000), (2049, 64), (65, 700))
SYN_POSES = (0, 1, 2, 37)
COUNTERS = ("crossings", "ends")


def table(n_poses, seed=0):
    """(tags int32[n], Tcw float32[n, 12]) in unsorted tag order: a good pose; then a NaN pose; then the other log tags below
    10, with an infinite and a far pose among them, and tags that no pair carries"""
    rng = np.random.default_rng(300 + n_poses + seed)

    def good():
        return pose(*rng.uniform(-0.3, 0.3, 2), rng.uniform(-0.6, 0.6, 3))

    rows = []
    if n_poses >= 1:
        rows.append((TAG_GOOD, good()))
    if n_poses >= 2:
        rows.append((TAG_NAN, np.full(12, np.nan, F)))
    if n_poses >= 3:
        inf = good()
        inf[7] = np.inf
        rows.append((TAG_INF, inf))
        rows.append((TAG_FAR, pose(0.1, 0.2, (1e6, -1e6, 3e6))))     # a centre beyond +-2^20 cells of 0.05
        for t in [0, 1, 2, 3, 4, 6, (1 << 31) - 1] + list(range(200, 260)):
            if len(rows) < n_poses:
                rows.append((t, good()))
    assert len(rows) == n_poses
    order = rng.permutation(n_poses)
    if n_poses > 1 and (np.diff([rows[i][0] for i in order]) > 0).all():
        order = order[::-1]
    return np.array([rows[i][0] for i in order], np.int32), np.array([rows[i][1] for i in order], F).reshape(-1, 12)


def synthetic_case(M, E, seed=0):
    """(records of a map of exactly M entries, every record in a voxel of its own; the E distinct pairs of its log in a random
    order).  Four fifths of the entries fill a cube of cells beside the origin, where the cameras of table() stand, so a
    ray to one crosses others; the rest lie on a lattice a thousand cells away: long rays beside short ones"""
    rng = np.random.default_rng(900 + M + E + seed)
    near = M - M // 5
    side = max(int(np.ceil(near ** (1.0 / 3.0))), 1)
    i = np.arange(near)
    j = np.arange(M - near)
    cell = np.concatenate([np.stack([i % side, (i // side) % side, i // (side * side)], 1),
                           np.stack([j % 64, j // 64, np.full(len(j), 1000)], 1)]).astype(np.float64)
    xyz = ((cell + rng.uniform(0.1, 0.9, (M, 3))) * VOXEL).astype(F)
    rec = {"xyz": xyz, "pixel": rng.integers(0, 1 << 20, M).astype(np.uint32),
           "rho_sigma": np.stack([rng.uniform(0.2, 2.0, M), rng.uniform(0.01, 0.2, M)], 1).astype(F),
           "intensity": rng.integers(0, 256, M).astype(np.uint8), "tag": rng.integers(0, LOG_TAGS, M).astype(np.int32),
           "multiplicity": rng.integers(1, 4, M).astype(np.uint32)}
    assert E <= M * LOG_TAGS
    pick = rng.choice(M * LOG_TAGS, E, replace=False) if E else np.zeros(0, np.int64)
    return rec, {"entry": (pick // LOG_TAGS).astype(np.uint32), "tag": (pick % LOG_TAGS).astype(np.int32)}


def crafted_case():
    """tests/test_vmap_carve_cpu.py's crafted rays at voxel 1: one entry per point (id = g), one pair per entry, and the pose
    whose centre is exactly (0.5, 0.5, 0.5).  The steps are [6, 1, 2, 3, 4, 5, 4, 1, 0, 4, 5]; entry 8 lies in the camera's
    own cell; entry 11 has no pair"""
    pts = np.array([[2.5, 2.5, 2.5], [1.5, 0.5, 0.5], [1.5, 1.5, 0.5], [1.5, 1.5, 1.5], [2.5, 1.5, 1.5], [2.5, 2.5, 1.5],
                    [2.5, 2.5, 0.5], [0.5, 1.5, 0.5], [0.75, 0.25, 0.5], [-3.5, 0.5, 0.5], [0.5, 0.5, 5.5], [7.5, 7.5, 7.5]], F)
    rec = dict(cloud_of(pts), tag=np.zeros(len(pts), np.int32), multiplicity=np.ones(len(pts), np.uint32))
    pairs = {"entry": np.arange(len(pts) - 1, dtype=np.uint32), "tag": np.zeros(len(pts) - 1, np.int32)}
    Tcw = np.array([[1, 0, 0, -0.5, 0, 1, 0, -0.5, 0, 0, 1, -0.5]], F)
    assert carve_np.camera_centre(Tcw[0]).tolist() == [0.5, 0.5, 0.5]
    return rec, pairs, np.zeros(1, np.int32), Tcw


def build(rec, pairs, voxel):
    """the map and the log as the restatements make them from imported records and pairs"""
    vm, ol = vmap_np.VoxelMap(voxel), vo.ObservationLog()
    d = vi.import_records(vm, rec)
    M = len(rec["pixel"])
    assert d["created"] == M == vm.M and (d["dst_ids"] == np.arange(M)).all()
    if len(pairs["entry"]):
        vi.import_observations(ol, vm.M, pairs["entry"], pairs["tag"])
    assert np.array_equal(ol.entry, pairs["entry"]) and np.array_equal(ol.tag, pairs["tag"])
    return vm, ol


def call(vm, ol, tags, Tcw, end_margin=1, max_steps=4096, first=0, count=None):
    got = vr.recarve((vm.keys, vm.ids), vm.rec["xyz"], ol.entry, ol.tag, tags, Tcw, vm.voxel_size, end_margin, max_steps, first, count)
    assert got["crossings"].dtype == np.uint64 and got["ends"].dtype == np.uint64 and len(got["crossings"]) == vm.M
    # the consequences sdm_c.h states
    assert got["rays_total"] == got["pairs_total"] - got["pairs_unposed"]
    assert got["cells_hit"] == int(got["crossings"].sum()) and got["ends_hit"] == int(got["ends"].sum())
    assert got["ends_hit"] == got["rays_total"] - got["rays_skipped"]
    walked = ol.entry[got["ray_pair"][got["steps"] >= 0]]
    np.testing.assert_array_equal(got["ends"], np.bincount(walked, minlength=vm.M).astype(np.uint64))
    # the map index made from the records alone is the map's
    keys, ids = vr.map_index(vm.rec["xyz"], vm.voxel_size)
    assert np.array_equal(keys, vm.keys) and np.array_equal(ids, vm.ids)
    return got


def scalar_recarve(vm, ol, tags, Tcw, end_margin, max_steps, first=0, count=None):
    """the semantics of include/sdm_c.h, pair by pair: test_vmap_carve_cpu's scalar walk of one ray at a time"""
    centre = {int(t): carve_np.camera_centre(T) for t, T in zip(tags, np.asarray(Tcw, F).reshape(-1, 12))}
    count = ol.E - first if count is None else count
    cr, en = np.zeros(vm.M, np.uint64), np.zeros(vm.M, np.uint64)
    tot = dict.fromkeys(vr.OUTS, 0)
    for k in range(first, first + count):
        e, t = int(ol.entry[k]), int(ol.tag[k])
        tot["pairs_total"] += 1
        if t not in centre:
            tot["pairs_unposed"] += 1
            continue
        c1, e1, t1 = scalar_carve(vm, vm.rec["xyz"][e][None], [0], None, [0], None, {0: centre[t]}, vm.voxel_size, end_margin, max_steps)
        cr, en = cr + c1, en + e1
        for f in vr.OUTS[2:]:
            tot[f] += t1[f]
    return cr, en, tot


def both(vm, ol, tags, Tcw, end_margin=1, max_steps=4096, first=0, count=None):
    got = call(vm, ol, tags, Tcw, end_margin, max_steps, first, count)
    cr, en, tot = scalar_recarve(vm, ol, tags, Tcw, end_margin, max_steps, first, count)
    np.testing.assert_array_equal(got["crossings"], cr)
    np.testing.assert_array_equal(got["ends"], en)
    assert {f: got[f] for f in vr.OUTS} == tot
    return got


def test_crafted_rays_against_the_scalar_loop():
    """N == max_steps and max_steps + 1, end_margin 0, 1 and beyond N, a centre in the point's own cell, an entry with no
    pairs, a tag absent from the table"""
    rec, pairs, tags, Tcw = crafted_case()
    vm, ol = build(rec, pairs, 1.0)
    got = both(vm, ol, tags, Tcw, 0, 64)
    assert got["steps"].tolist() == [6, 1, 2, 3, 4, 5, 4, 1, 0, 4, 5]
    # every ray counts the camera's own cell, which holds entry 8 -- except the ray to entry 8 itself (N = 0: nothing
    # counted, one end); entry 11 has no pair: no end, and no ray reaches its voxel
    assert got["crossings"].tolist() == [0, 6, 5, 3, 2, 1, 0, 0, 10, 0, 0, 0]
    assert got["ends"].tolist() == [1] * 11 + [0]
    assert both(vm, ol, tags, Tcw, 1, 64)["crossings"].tolist() == [0, 5, 4, 2, 1, 0, 0, 0, 8, 0, 0, 0]
    assert both(vm, ol, tags, Tcw, 0, 6)["rays_skipped"] == 0                        # N == max_steps walks
    got = both(vm, ol, tags, Tcw, 0, 5)                                              # N == max_steps + 1 skips
    assert got["rays_skipped"] == 1 and got["steps"][0] == -1 and got["ends"][0] == 0
    for margin in (6, 7, 1000):  # beyond every N: nothing is crossed, every walked ray still ends
        got = both(vm, ol, tags, Tcw, margin, 64)
        assert got["cells_visited"] == 0 and got["crossings"].sum() == 0 and got["ends_hit"] == 11
    # a table that does not name the log's tag: no ray
    got = both(vm, ol, [3], Tcw, 0, 64)
    assert (got["pairs_total"], got["pairs_unposed"], got["rays_total"]) == (11, 11, 0) and not got["crossings"].any()
    # a range: the pairs 3 .. 6 alone
    got = both(vm, ol, tags, Tcw, 0, 64, 3, 4)
    assert got["steps"].tolist() == [3, 4, 5, 4] and got["ends"].tolist() == [0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("n_poses", SYN_POSES)
def test_synthetic_map_against_the_scalar_loop(n_poses):
    """65 entries, 65 pairs: the hostile poses (NaN, Inf, a centre beyond +-2^20 cells), the tags in no table, the entries
    without pairs"""
    rec, pairs = synthetic_case(65, 65)
    vm, ol = build(rec, pairs, VOXEL)
    tags, Tcw = table(n_poses)
    for end_margin, max_steps in ((0, 4096), (1, 4096), (2, 900)):
        got = both(vm, ol, tags, Tcw, end_margin, max_steps)
        posed = np.isin(ol.tag, tags)
        assert got["pairs_unposed"] == int((~posed).sum())
        if n_poses == 0:
            assert got["pairs_unposed"] == got["pairs_total"] == 65 and not got["crossings"].any() and not got["ends"].any()
        bad = np.isin(ol.tag, [t for t in (TAG_NAN, TAG_INF, TAG_FAR) if t in tags])
        assert got["rays_skipped"] >= int(bad.sum())
        if n_poses == 37:
            assert bad.sum() >= 3 and 0 < got["pairs_unposed"] < 65 and got["ends_hit"] > 0
            assert (np.bincount(ol.entry, minlength=vm.M) == 0).any()   # entries without pairs
            if max_steps == 900:
                assert got["rays_skipped"] > int(bad.sum())             # the far lattice is beyond 900 steps


def test_additivity_over_splits_and_orders_and_reset():
    rec, pairs = synthetic_case(65, 700)
    vm, ol = build(rec, pairs, VOXEL)
    tags, Tcw = table(37)
    whole = call(vm, ol, tags, Tcw)
    assert whole["cells_hit"] > 0 and whole["rays_skipped"] > 0 and whole["pairs_unposed"] > 0
    E = ol.E
    for cuts in ([0, 63, E], [0, 64, 65, E], [0, 1, 128, 129, 640, E], [0, 0, E, E]):
        ranges = list(zip(cuts[:-1], cuts[1:]))
        for order in (ranges, ranges[::-1]):
            ev = {f: np.zeros(0, np.uint64) for f in COUNTERS}
            tot = dict.fromkeys(vr.OUTS, 0)
            for i, (a, b) in enumerate(order):
                got = call(vm, ol, tags, Tcw, first=a, count=b - a)
                ev = vr.accumulate(ev, vm.M, got, reset=(i == 0))
                for f in vr.OUTS:
                    tot[f] += got[f]
            for f in COUNTERS:
                np.testing.assert_array_equal(ev[f], whole[f], err_msg=str(cuts))
            assert tot == {f: whole[f] for f in vr.OUTS}, cuts
    # reset is idempotent; without it a second call counts twice
    once = vr.accumulate({f: np.full(vm.M, 9, np.uint64) for f in COUNTERS}, vm.M, whole, True)
    twice = vr.accumulate(once, vm.M, call(vm, ol, tags, Tcw), True)
    added = vr.accumulate(once, vm.M, whole, False)
    for f in COUNTERS:
        np.testing.assert_array_equal(once[f], whole[f])
        np.testing.assert_array_equal(twice[f], whole[f])
        np.testing.assert_array_equal(added[f], 2 * whole[f])
    # an empty range and an empty log
    got = call(vm, ol, tags, Tcw, first=E, count=0)
    assert [got[f] for f in vr.OUTS] == [0] * 7
    got = call(vm, vo.ObservationLog(), tags, Tcw)
    assert [got[f] for f in vr.OUTS] == [0] * 7 and not got["ends"].any()


@pytest.mark.parametrize("M,E", SYN_CASES)
def test_synthetic_inputs_cover_what_the_gpu_test_is_for(M, E):
    rec, pairs = synthetic_case(M, E)
    vm, ol = build(rec, pairs, VOXEL)
    assert vm.M == M and ol.E == E
    got = call(vm, ol, *table(37))
    if E >= 63:
        assert got["cells_hit"] > 0 and got["rays_skipped"] > 0 and 0 < got["pairs_unposed"] < E
        assert got["steps"].max() > 1000     # the far lattice: long rays beside short ones in one wave
    tags, _ = table(37)
    assert len(tags) == 37 and len(set(tags.tolist())) == 37 and (np.diff(tags) < 0).any() and (1 << 31) - 1 in tags


# ---- where every multiplicity is 1, a recarve of the whole log is the carve ----------------------------------------------
EQ_VOXEL, EQ_MARGIN, EQ_STEPS = 0.005, 1, 4096


@functools.lru_cache(maxsize=None)
def fixture_kf0(name):
    """keyframe 0 of a golden fixture, integrated, observed and carved alone with its neighbour row (sigma gate 0.3, the
    checked rho): (the map, the log, the carve's result, the table of keyframe 0 and its neighbours at the fixture's poses)"""
    g, xyz, sigma, offs, support, rows = fixture_case(name)
    a, b = int(offs[0]), int(offs[1])
    T = b - a
    cloud = {"xyz": xyz[a:b], "pixel": np.arange(T, dtype=np.uint32), "rho_sigma": np.stack([np.ones(T, F), sigma[a:b]], 1),
             "intensity": np.zeros(T, np.uint8)}
    vm, ol = vmap_np.VoxelMap(EQ_VOXEL), vo.ObservationLog()
    vm.integrate(cloud, np.zeros(T, np.int32))
    row = np.zeros(T, np.int64)
    ol.observe((vm.keys, vm.ids), EQ_VOXEL, xyz[a:b], row, support[a:b], [0], rows[0:1])
    centres = {k: carve_np.camera_centre(g["Tcw"][k]) for k in range(g["n_kf"])}
    carved = vc.carve((vm.keys, vm.ids), xyz[a:b], row, support[a:b], [0], rows[0:1], centres, EQ_VOXEL, EQ_MARGIN, EQ_STEPS)
    tags = np.unique(np.append(rows[0], 0)).astype(np.int32)[::-1]
    return vm, ol, carved, (tags, np.array([g["Tcw"][k] for k in tags], F).reshape(-1, 12)), T


# M = T of keyframe 0 at voxel 0.005, then (rays_total, cells_visited, cells_hit, ends_hit): what the restatement gives on
# the CPU.  At this voxel a plane's rays pass through no other entry's voxel: only the strip has crossings; the counters
# compared entry for entry are the ends on every fixture and the crossings on the strip
PINNED = {"plane_160x120_n7": (2209, 8824, 2572636, 0, 8824), "plane_64x48_n7": (720, 2880, 841822, 0, 2880),
          "plane_96x80_n20": (678, 2704, 800897, 0, 2704), "strip_roll_160x120_n7": (2255, 8937, 2576915, 25, 8937)}


@pytest.mark.parametrize("name", gu.fixture_names())
def test_recarve_of_the_whole_log_is_the_carve(name):
    vm, ol, carved, (tags, Tcw), T = fixture_kf0(name)
    assert vm.M == T and (vm.rec["multiplicity"] == 1).all()   # every multiplicity is 1: the equivalence is not vacuous
    got = call(vm, ol, tags, Tcw, EQ_MARGIN, EQ_STEPS)
    print(name, T, {f: got[f] for f in vr.OUTS}, "longest ray", int(got["steps"].max()))
    for f in COUNTERS:
        np.testing.assert_array_equal(got[f], carved[f], err_msg=f)
    for f in ("rays_total", "rays_skipped", "cells_visited", "cells_hit", "ends_hit"):
        assert got[f] == carved[f], f
    assert got["pairs_unposed"] == 0 and got["rays_skipped"] == 0 and got["rays_total"] == ol.E > T and got["cells_visited"] > 0
    assert (T, got["rays_total"], got["cells_visited"], got["cells_hit"], got["ends_hit"]) == PINNED[name]
