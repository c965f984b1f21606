"""CPU: tests/vmap_class_np.py (the NumPy statement of sdm_vmap_classify) against an independent scalar dict loop on
random and crafted maps, the invariants C1 .. C3 of include/sdm_c.h on the statement itself, and the pinned figures of
the golden fixtures' integrate-observe-carve-classify sequences."""
import functools
import struct

import numpy as np
import pytest

import carve_np
import golden_util as gu
import vmap_carve_np as vc
import vmap_class_np as vcl
import vmap_np
import vmap_obs_np as vo
from test_voxcam_cpu import fixture_case
from test_vmap_obs_cpu import scalar_key

F = np.float32
TOP64 = (1 << 64) - 1
RULE = vcl.rule_of(min_multiplicity=2, min_cameras=2, min_ends=2, ratio_num=1, ratio_den=2, max_sigma=0.2, min_neighbours=2)


def float_key(x):
    """key() of one float32, through its bytes"""
    b = struct.unpack("<I", struct.pack("<f", x))[0]
    return (~b) & 0xFFFFFFFF if b >> 31 else b | 0x80000000


def scalar_classify(vm, crossings, ends, ncam, rule, published, wrap=False):
    """the semantics of include/sdm_c.h, entry by entry: (passing, LOCAL, nb) as lists.  wrap: the ratio products are
    taken modulo 2^64 -- the mistake the statement must not make"""
    M = vm.M
    cell_of = [scalar_key(vm.rec["xyz"][e], vm.voxel_size) for e in range(M)]
    entry_at = {c: e for e, c in enumerate(cell_of)}
    assert len(entry_at) == M and None not in entry_at
    mod = (1 << 64) if wrap else (1 << 200)
    loc = []
    for e in range(M):
        cr, en = int(crossings[e]), int(ends[e])
        loc.append(int(vm.rec["multiplicity"][e]) >= rule["min_multiplicity"] and int(ncam[e]) >= rule["min_cameras"] and
                   en >= rule["min_ends"] and (cr * rule["ratio_den"]) % mod <= (en * rule["ratio_num"]) % mod and
                   float_key(vm.rec["rho_sigma"][e][1]) <= float_key(rule["max_sigma"]))
    nb = []
    for e in range(M):
        cx, cy, cz = cell_of[e]
        n = 0
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    c = (cx + dx, cy + dy, cz + dz)
                    if c == cell_of[e] or not all(-(1 << 20) <= v < (1 << 20) for v in c):
                        continue
                    o = entry_at.get(c)
                    n += o is not None and loc[o]
        nb.append(n)
    ok = [loc[e] and nb[e] >= rule["min_neighbours"] for e in range(M)]
    return ok, loc, nb


def cloud_of(xyz, sigma):
    T = len(xyz)
    return {"xyz": xyz, "pixel": np.arange(T, dtype=np.uint32), "rho_sigma": np.stack([np.ones(T, F), sigma.astype(F)], 1),
            "intensity": np.zeros(T, np.uint8)}


SIGMAS = np.array([0.05, 0.1, 0.19999, 0.2, 0.2000001, 0.5, 0.0, -0.0, np.nan, -np.nan, np.inf, -np.inf, -1.0, 1e-30], F)


def random_map(seed, voxel=0.25, T=1500, edge=True):
    """a dense random map on both sides of zero, two clusters at the ends of the cell range, every special sigma"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-1, 1, (T, 3)).astype(F)
    if edge:  # cells 2^20 - 1, 2^20 - 2 and -2^20, -2^20 + 1: some of their neighbours lie outside the range
        top = F((1 << 20) - 0.5) * F(voxel)
        corner = np.array([[top, top, top], [-top, -top, -top], [top, -top, 0.1]], F)
        c = corner[rng.integers(0, 3, 120)]
        near = c - rng.integers(0, 2, (120, 3)).astype(F) * np.sign(c) * F(voxel)  # one cell inwards, or none, per axis
        xyz = np.concatenate([xyz, corner, near.astype(F)])
    sigma = SIGMAS[rng.integers(0, len(SIGMAS), len(xyz))]
    vm = vmap_np.VoxelMap(voxel)
    for part in np.array_split(rng.permutation(len(xyz)), 3):  # three calls: records get replaced, multiplicities add
        vm.integrate(cloud_of(xyz[part], sigma[part]), np.zeros(len(part), np.int32))
    M = vm.M
    crossings = rng.integers(0, 6, M).astype(np.uint64)
    ends = rng.integers(0, 6, M).astype(np.uint64)
    huge = rng.random(M) < 0.15  # counters near 2^64 - 1: a product that wraps gives another answer
    crossings[huge] = np.uint64(TOP64) - rng.integers(0, 4, int(huge.sum())).astype(np.uint64)
    ends[huge] = np.uint64(TOP64) - rng.integers(0, 4, int(huge.sum())).astype(np.uint64)
    half = rng.random(M) < 0.1
    crossings[half] = np.uint64(1 << 63) + rng.integers(0, 3, int(half.sum())).astype(np.uint64)
    ncam = rng.integers(0, 4, M)
    return vm, crossings, ends, ncam


RULES = [dict(min_multiplicity=2, min_cameras=1, min_ends=1, ratio_num=1, ratio_den=2, max_sigma=0.2, min_neighbours=1),
         dict(ratio_num=3, ratio_den=2, max_sigma=float("nan"), min_neighbours=0),
         dict(ratio_num=0xFFFFFFFF, ratio_den=0xFFFFFFFF, max_sigma=float("inf"), min_neighbours=26),
         dict(min_ends=TOP64 - 2, ratio_num=2, ratio_den=3, max_sigma=float("-inf"), min_neighbours=0),
         dict(ratio_num=0, ratio_den=1, max_sigma=-0.0, min_neighbours=1),
         dict(min_multiplicity=1, ratio_num=1, ratio_den=4, max_sigma=0.0, min_neighbours=2),
         dict(ratio_num=2, ratio_den=2, max_sigma=-float("nan"), min_neighbours=0)]


@pytest.mark.parametrize("voxel", [0.25, 1.0])
@pytest.mark.parametrize("seed", range(3))
def test_random_maps_against_the_dict_loop(seed, voxel):
    vm, crossings, ends, ncam = random_map(seed, voxel)
    M = vm.M
    cells = np.array([scalar_key(vm.rec["xyz"][e], voxel) for e in range(M)])
    assert (cells < 0).any() and (cells > 0).any()  # both sides of zero
    assert (cells == (1 << 20) - 1).any() and (cells == -(1 << 20)).any()  # the ends of the cell range
    wrapped_differs = False
    seen_nb = set()
    for r in RULES:
        rule = vcl.rule_of(**r)
        ok, loc = vcl.passing((vm.keys, vm.ids), vm.rec, voxel, crossings, ends, ncam, rule)
        s_ok, s_loc, s_nb = scalar_classify(vm, crossings, ends, ncam, rule, None)
        assert loc.tolist() == s_loc, r
        assert ok.tolist() == s_ok, r
        assert vcl.neighbours((vm.keys, vm.ids), vm.rec, voxel, loc).tolist() == s_nb, r
        wrapped_differs |= scalar_classify(vm, crossings, ends, ncam, rule, None, wrap=True)[1] != s_loc
        seen_nb |= set(s_nb)
    assert wrapped_differs  # the counters are large enough for a wrapping product to show
    assert max(seen_nb) >= 3 and 0 in seen_nb


def test_special_sigmas_and_thresholds():
    """every (sigma, max_sigma) pair of the special values, one entry each: the verdict is key(sigma) <= key(max_sigma)"""
    order = [-np.nan, -np.inf, -1.0, -0.0, 0.0, 1e-30, 0.05, 0.2, np.inf, np.nan]  # ascending under key()
    keys = [float_key(F(v)) for v in order]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    xyz = (np.arange(len(order))[:, None] * np.array([[3.0, 0, 0]]) + 0.5).astype(F)  # no two entries adjacent
    vm = vmap_np.VoxelMap(1.0)
    vm.integrate(cloud_of(xyz, np.array(order, F)), np.zeros(len(order), np.int32))
    assert vm.M == len(order)
    z = np.zeros(vm.M, np.uint64)
    for j, ms in enumerate(order):
        ok, _ = vcl.passing((vm.keys, vm.ids), vm.rec, 1.0, z, z, z, vcl.rule_of(max_sigma=ms))
        assert ok.tolist() == [i <= j for i in range(len(order))], ms
        assert ok.tolist() == scalar_classify(vm, z, z, z, vcl.rule_of(max_sigma=ms), None)[0]


def test_full_block_with_a_failing_centre():
    """a 3 x 3 x 3 block of entries whose centre fails LOCAL: it does not pass though all 26 neighbours do, and it is not
    counted as anybody's neighbour"""
    g = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij"), -1).reshape(-1, 3)
    xyz = (g + 0.5).astype(F) * F(0.5)
    sigma = np.where((g == 0).all(1), 0.9, 0.1).astype(F)
    vm = vmap_np.VoxelMap(0.5)
    vm.integrate(cloud_of(xyz, sigma), np.zeros(27, np.int32))
    assert vm.M == 27
    z = np.zeros(27, np.uint64)
    centre = int(np.flatnonzero((g == 0).all(1))[0])
    in_block = np.array([np.prod(3 - np.abs(c)) for c in g]) - 1  # the other cells of the block adjacent to each cell
    for want in (0, 1, 7, 10, 16, 17, 25, 26):
        rule = vcl.rule_of(max_sigma=0.2, min_neighbours=want)
        ok, loc = vcl.passing((vm.keys, vm.ids), vm.rec, 0.5, z, z, z, rule)
        s_ok, s_loc, s_nb = scalar_classify(vm, z, z, z, rule, None)
        assert ok.tolist() == s_ok and loc.tolist() == s_loc
        assert not ok[centre] and s_nb[centre] == 26 and int(loc.sum()) == 26
        assert [s_nb[e] for e in range(27) if e != centre] == [int(in_block[e]) - 1 for e in range(27) if e != centre]
        assert int(ok.sum()) == sum(in_block[e] - 1 >= want for e in range(27) if e != centre)
    # with a centre that passes, min_neighbours 26 accepts exactly the centre
    ok, _ = vcl.passing((vm.keys, vm.ids), vm.rec, 0.5, z, z, z, vcl.rule_of(max_sigma=1.0, min_neighbours=26))
    assert np.flatnonzero(ok).tolist() == [centre]


def test_invariants_c1_c2_c3():
    vm, crossings, ends, ncam = random_map(11, 0.25, edge=False)
    A = vcl.rule_of(min_multiplicity=2, ratio_num=1, ratio_den=1, max_sigma=0.2, min_neighbours=1)
    B = vcl.rule_of(min_multiplicity=1, min_cameras=1, ratio_num=2, ratio_den=1, max_sigma=0.5, min_neighbours=2)
    pa = vcl.passing((vm.keys, vm.ids), vm.rec, 0.25, crossings, ends, ncam, A)[0]
    pb = vcl.passing((vm.keys, vm.ids), vm.rec, 0.25, crossings, ends, ncam, B)[0]
    assert (pa & ~pb).any() and (pb & ~pa).any() and (pa & pb).any()
    cl = vcl.Classifier()
    dry = cl.classify(vm, crossings, ends, ncam, A, commit=False)
    assert cl.info() == {"published": 0, "calls": 0} and dry["published_total"] == 0 and dry["accepted"] == int(pa.sum())
    a = cl.classify(vm, crossings, ends, ncam, A)
    assert a["accepted_ids"].tolist() == np.flatnonzero(pa).tolist() == dry["accepted_ids"].tolist() and a["retracted"] == 0
    again = cl.classify(vm, crossings, ends, ncam, A)  # C1
    assert again["accepted"] == again["retracted"] == 0 and again["published_total"] == a["published_total"] == int(pa.sum())
    b = cl.classify(vm, crossings, ends, ncam, B)  # C2
    assert b["accepted_ids"].tolist() == np.flatnonzero(pb & ~pa).tolist()
    assert b["retracted_ids"].tolist() == np.flatnonzero(pa & ~pb).tolist()
    assert np.array_equal(cl.flags(vm.M), pb.astype(np.uint8))  # C3
    assert cl.info() == {"published": int(pb.sum()), "calls": 3}
    # entries created after the call read 0, and a later call judges them like any other
    more = np.random.default_rng(5).uniform(1.5, 2.5, (300, 3)).astype(F)
    m0 = vm.M
    vm.integrate(cloud_of(more, np.full(300, 0.1, F)), np.zeros(300, np.int32))
    assert vm.M > m0 and not cl.flags(vm.M)[m0:].any() and np.array_equal(cl.flags(vm.M)[:m0], pb.astype(np.uint8))
    c = cl.classify(vm, None, None, None, vcl.rule_of(max_sigma=float("nan")))  # no evidence, no log: everything passes
    assert c["published_total"] == vm.M and c["retracted"] == 0 and c["accepted"] == vm.M - int(pb.sum())
    none = cl.classify(vm, crossings, ends, ncam, vcl.rule_of(min_multiplicity=1 << 31, min_neighbours=0))
    assert none["retracted"] == vm.M and none["published_total"] == 0 and not cl.flags(vm.M).any()


@functools.lru_cache(maxsize=None)
def fixture_sequence(name, voxel=0.02, end_margin=1, max_steps=4096):
    """test_vmap_obs_cpu.fixture_sequence's recipe with test_vmap_carve_cpu.fixture_sequence's carve, and a committing
    classify with RULE after every keyframe: (the map, the flags, per call (delta of the statement, the scalar loop's
    (passing, LOCAL, nb)))"""
    g, xyz, sigma, offs, support, rows = fixture_case(name)
    cloud = cloud_of(xyz, sigma)
    centres = {k: carve_np.camera_centre(g["Tcw"][k]) for k in range(g["n_kf"])}
    vm, ol, cl, calls = vmap_np.VoxelMap(voxel), vo.ObservationLog(), vcl.Classifier(), []
    crossings, ends = np.zeros(0, np.uint64), np.zeros(0, np.uint64)
    for k in range(g["n_kf"]):
        a, b = offs[k], offs[k + 1]
        vm.integrate({f: v[a:b] for f, v in cloud.items()}, np.full(b - a, k, np.int32))
        ol.observe((vm.keys, vm.ids), voxel, xyz[a:b], np.zeros(b - a, np.int64), support[a:b], [k], rows[k:k + 1])
        got = vc.carve((vm.keys, vm.ids), xyz[a:b], np.zeros(b - a, np.int64), support[a:b], [k], rows[k:k + 1], centres, voxel,
                       end_margin, max_steps)
        grow = vm.M - len(crossings)
        crossings = np.concatenate([crossings, np.zeros(grow, np.uint64)]) + got["crossings"]
        ends = np.concatenate([ends, np.zeros(grow, np.uint64)]) + got["ends"]
        ncam = np.diff(ol.cameras(vm.M)[0])
        before = cl.flags(vm.M).astype(bool)
        scalar = scalar_classify(vm, crossings, ends, ncam, RULE, None)
        d = cl.classify(vm, crossings, ends, ncam, RULE)
        calls.append((d, scalar, before))
    return vm, cl, calls


# (summed accepted, summed retracted, final published): what the statement and the scalar loop agree on
PINNED = {"plane_160x120_n7": (436, 8, 428), "plane_64x48_n7": (573, 8, 565), "plane_96x80_n20": (622, 20, 602),
          "strip_roll_160x120_n7": (592, 24, 568)}


@pytest.mark.parametrize("name", gu.fixture_names())
def test_golden_fixtures_are_not_vacuous(name):
    vm, cl, calls = fixture_sequence(name)
    rejected_by_neighbours = 0
    for d, (s_ok, s_loc, s_nb), before in calls:
        ok = np.array(s_ok, bool)
        assert d["accepted_ids"].tolist() == np.flatnonzero(ok & ~before).tolist()
        assert d["retracted_ids"].tolist() == np.flatnonzero(~ok & before).tolist()
        assert d["local"] == sum(s_loc) and d["published_total"] == int(ok.sum())
        rejected_by_neighbours += sum(s_loc) - int(ok.sum())
    got = (sum(d["accepted"] for d, _, _ in calls), sum(d["retracted"] for d, _, _ in calls), calls[-1][0]["published_total"])
    print(name, "M", vm.M, got, "LOCAL-passing entries the neighbour test rejected, summed:", rejected_by_neighbours)
    assert any(d["retracted"] > 0 for d, _, _ in calls) and got[0] > 0 and rejected_by_neighbours > 0
    assert got == PINNED[name]
    assert cl.info() == {"published": got[2], "calls": len(calls)} and got[0] - got[1] == got[2]
    if name == "plane_160x120_n7":
        d = calls[0][0]
        assert (d["examined"], d["local"], d["accepted"]) == (516, 313, 310)
