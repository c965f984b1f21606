"""CPU: tests/vmap_obs_np.py (the NumPy statement of sdm_vmap_observe's observation log) against a scalar dict loop on
random clouds, the invariants O1 .. O4 of include/sdm_c.h on the statement itself, and the pinned figures of the golden
fixtures' integrate-then-observe sequences."""
import functools

import numpy as np
import pytest

import golden_util as gu
import vmap_np
import vmap_obs_np as vo
import voxcam_np
import voxel_np
from test_voxcam_cpu import fixture_case

F = np.float32
TOP = (1 << 31) - 1


def cloud_of(xyz):
    T = len(xyz)
    return {"xyz": xyz, "pixel": np.arange(T, dtype=np.uint32), "rho_sigma": np.stack([np.ones(T, F), np.full(T, 0.1, F)], 1),
            "intensity": np.zeros(T, np.uint8)}


def map_of(xyz, voxel):
    vm = vmap_np.VoxelMap(voxel)
    vm.integrate(cloud_of(xyz), np.zeros(len(xyz), np.int32))
    return vm


def scalar_key(p, voxel):
    """the voxel of one point as a tuple of cells, or None (float32 throughout, as voxel_np.cells)"""
    inv = F(1.0) / F(voxel)
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.floor(p.astype(F) * inv)
    if not all(-(2.0 ** 20) <= v < 2.0 ** 20 for v in c):  # (False for a NaN)
        return None
    return tuple(int(v) for v in c)


class DictLog:
    """the semantics of include/sdm_c.h, point by point"""

    def __init__(self):
        self.log, self.have = [], set()

    def observe(self, entry_of_cell, voxel, xyz, row, support, own, nbr):
        d = {"plain_total": len(xyz), "unmapped": 0, "candidates": 0, "first_created": len(self.log), "created": 0}
        for g in range(len(xyz)):
            i = int(row[g])
            key = scalar_key(xyz[g], voxel)
            eid = entry_of_cell.get(key) if key is not None else None
            if eid is None:
                d["unmapped"] += 1
                continue
            cams = {int(own[i])}
            if nbr is not None:
                cams |= {int(nbr[i][j]) for j in range(len(nbr[i])) if int(support[g]) >> j & 1}
            d["candidates"] += len(cams)
            for t in sorted(cams):
                if (eid, t) not in self.have:
                    self.have.add((eid, t))
                    self.log.append((eid, t))
                    d["created"] += 1
        return d

    def lists(self, M):
        out = [[] for _ in range(M)]
        for e, t in sorted(self.have):
            out[e].append(t)
        return out


def cells_of_map(vm, voxel):
    """{cell tuple: entry id} of a vmap_np map, through its records' own xyz"""
    return {scalar_key(vm.rec["xyz"][e], voxel): e for e in range(vm.M)}


def same_log(ol, dl, M, what=""):
    assert list(zip(ol.entry.tolist(), ol.tag.tolist())) == dl.log, what
    offs, tags = ol.cameras(M)
    assert offs.dtype == np.int64 and tags.dtype == np.int32
    got = vo.lists(offs, tags)
    assert got == dl.lists(M), what
    assert all(a < b for c in got for a, b in zip(c, c[1:])), what


def random_case(seed, voxel, n=4, n_nbr=5, T=900, tag_pool=None):
    """a map built from two thirds of a random cloud (so that some points have no entry), nasty points included"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-1, 1, (T, 3)).astype(F)
    bad = rng.permutation(T)[:30]
    xyz[bad[:10], rng.integers(0, 3, 10)] = np.nan
    xyz[bad[10:20], rng.integers(0, 3, 10)] = np.inf
    xyz[bad[20:30], rng.integers(0, 3, 10)] = F(2.0 ** 21) * F(voxel) * F(2)  # beyond the cell range
    vm = map_of(xyz[rng.random(T) < 0.66], voxel)
    row = np.sort(rng.integers(0, n, T))
    pool = np.array(tag_pool if tag_pool is not None else [0, 3, 3, 7, 11, TOP, 12, 5])
    own = rng.choice(pool, n)
    nbr = rng.choice(pool, (n, n_nbr))
    nbr[0, 0] = own[0]  # a column that carries the own tag
    nbr[1, 1] = nbr[1, 0]  # equal tags on different columns
    if n > 2:
        own[2] = own[1]  # equal tags on different slots
    support = rng.integers(0, 1 << n_nbr, T, dtype=np.uint64) if n_nbr < 64 else \
        rng.integers(0, 1 << 63, T, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, T, dtype=np.uint64)
    support[rng.random(T) < 0.2] = 0
    return vm, xyz, row, support, own, nbr


@pytest.mark.parametrize("voxel", [0.25, 0.02, 1000.0])
@pytest.mark.parametrize("seed", range(3))
def test_random_clouds_against_the_dict_loop(seed, voxel):
    vm, xyz, row, support, own, nbr = random_case(seed, voxel)
    cells = cells_of_map(vm, voxel)
    ol, dl = vo.ObservationLog(), DictLog()
    for rep in range(2):  # the second pass creates nothing (O2)
        a = ol.observe((vm.keys, vm.ids), voxel, xyz, row, support, own, nbr)
        b = dl.observe(cells, voxel, xyz, row, support, own, nbr)
        assert a == b, (rep, a, b)
        assert a["unmapped"] >= 30 and (rep == 0) == (a["created"] > 0)
        same_log(ol, dl, vm.M, rep)
    assert ol.info() == {"observations": len(dl.log), "calls": 2}
    tags = set(ol.tag.tolist())
    assert 0 in tags and TOP in tags  # the ends of the tag range


def test_crafted_cases():
    voxel = 0.5
    xyz = np.array([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [0.9, 0.1, 0.1], [np.nan, 0, 0], [5, 5, 5], [0.3, 0.1, 0.2]], F)
    vm = map_of(xyz[:3], voxel)  # entries 0 (three points) and 1; (5, 5, 5) is not in the map
    assert vm.M == 2
    cells = cells_of_map(vm, voxel)
    row = np.array([0, 0, 0, 1, 1, 1])
    own, nbr = np.array([4, 9]), np.array([[9, 4, 9, 2], [2, 2, 9, 0]])
    support = np.array([0b0001, 0b0110, 0b1000, 0b1111, 0b1111, 0b0011], np.uint64)
    ol, dl = vo.ObservationLog(), DictLog()
    d = ol.observe((vm.keys, vm.ids), voxel, xyz, row, support, own, nbr)
    assert d == dl.observe(cells, voxel, xyz, row, support, own, nbr)
    # g0 {4, 9} -> (0,4) (0,9); g1 {4, 9}: the self column falls out, nothing new; g2 {4, 2} on entry 1 -> (1,2) (1,4);
    # g3 NaN, g4 no entry: unmapped; g5 {9, 2}: two columns, one tag -> (0,2)
    assert list(zip(ol.entry.tolist(), ol.tag.tolist())) == [(0, 4), (0, 9), (1, 2), (1, 4), (0, 2)]
    assert d == {"plain_total": 6, "unmapped": 2, "candidates": 8, "first_created": 0, "created": 5}
    assert vo.lists(*ol.cameras(vm.M)) == [[2, 4, 9], [2, 4]]
    assert vo.lists(*ol.cameras(vm.M, ids=[1, 1, 0])) == [[2, 4], [2, 4], [2, 4, 9]]
    assert vo.lists(*ol.cameras(vm.M, first=1, count=1)) == [[2, 4]]
    # an empty call, and one without a neighbour table: the own tag alone
    e = ol.observe((vm.keys, vm.ids), voxel, xyz[:0], row[:0], support[:0], own, nbr)
    assert e == {"plain_total": 0, "unmapped": 0, "candidates": 0, "first_created": 5, "created": 0}
    z = ol.observe((vm.keys, vm.ids), voxel, xyz, row, None, np.array([6, 4]), None)
    assert z == dl.observe(cells, voxel, xyz, row, None, [6, 4], None)
    assert z["candidates"] == 4 and z["created"] == 2 and ol.fetch(5)["tag"].tolist() == [6, 6]
    same_log(ol, dl, vm.M)
    # before any integrate everything is unmapped
    none = vo.ObservationLog()
    empty = vmap_np.VoxelMap(voxel)
    d0 = none.observe((empty.keys, empty.ids), voxel, xyz, row, support, own, nbr)
    assert d0 == {"plain_total": 6, "unmapped": 6, "candidates": 0, "first_created": 0, "created": 0}


def test_bit_63_of_a_64_column_row():
    vm, xyz, row, support, own, nbr = random_case(5, 0.25, n=2, n_nbr=64, T=300, tag_pool=np.arange(100, 164))
    nbr[0] = np.arange(200, 264)  # all distinct: column 63 is the only one that names tag 263
    support[row == 0] &= np.uint64((1 << 63) - 1)
    first = np.flatnonzero((row == 0) & (vo.entries_of((vm.keys, vm.ids), xyz, 0.25) >= 0))[0]
    support[first] = np.uint64(1 << 63)
    ol, dl = vo.ObservationLog(), DictLog()
    a = ol.observe((vm.keys, vm.ids), 0.25, xyz, row, support, own, nbr)
    assert a == dl.observe(cells_of_map(vm, 0.25), 0.25, xyz, row, support, own, nbr)
    same_log(ol, dl, vm.M)
    assert (ol.tag == 263).sum() == 1


def observe_rows(ol, vm, voxel, case, rows):
    _, xyz, row, support, own, nbr = case
    sel = np.isin(row, rows)
    remap = np.cumsum(np.isin(np.arange(len(own)), rows)) - 1
    return ol.observe((vm.keys, vm.ids), voxel, xyz[sel], remap[row[sel]], support[sel], own[rows], nbr[rows])


@pytest.mark.parametrize("seed", range(3))
def test_split_and_order_invariance(seed):
    voxel = 0.25
    case = random_case(seed + 10, voxel, n=6)
    vm = case[0]
    whole = vo.ObservationLog()
    observe_rows(whole, vm, voxel, case, list(range(6)))
    assert whole.E > 200
    rng = np.random.default_rng(seed)
    cuts = [[0, 6], [0, 1, 2, 3, 4, 5, 6], [0, 0, 6, 6], [0, 3, 3, 6]]  # fixed, degenerate (empty groups) ...
    cuts += [sorted({0, 6} | set(rng.integers(1, 6, 2).tolist())) for _ in range(3)]  # ... and random cuts
    for cut in cuts:  # O1: consecutive groups leave a byte-identical log
        ol = vo.ObservationLog()
        made = sum(observe_rows(ol, vm, voxel, case, list(range(a, b)))["created"] for a, b in zip(cut[:-1], cut[1:]))
        assert made == whole.E
        assert np.array_equal(ol.entry, whole.entry) and np.array_equal(ol.tag, whole.tag), cut
    again = observe_rows(whole, vm, voxel, case, list(range(6)))  # O2
    assert again["created"] == 0 and again["first_created"] == whole.E and again["candidates"] > 0
    for order in ([5, 4, 3, 2, 1, 0], rng.permutation(6).tolist()):  # O4: the lists, not the log order
        ol = vo.ObservationLog()
        for i in order:
            observe_rows(ol, vm, voxel, case, [i])
        assert np.array_equal(ol.pairs, whole.pairs)
        for a, b in zip(ol.cameras(vm.M), whole.cameras(vm.M)):
            assert np.array_equal(a, b)
    assert not np.array_equal(ol.entry, whole.entry)  # (the order of the calls does show in the log)


@pytest.mark.parametrize("voxel", [0.02, 1000.0, 1e-7])
@pytest.mark.parametrize("name", ["plane_64x48_n7", "plane_96x80_n20"])
def test_o3_against_the_per_call_camera_lists(name, voxel):
    """one integrate into an empty map, one observe of the same arguments, tags = slots: every entry's list is the
    cam_slots list of the kept point with the same (tag, pixel)"""
    g, xyz, sigma, offs, support, rows = fixture_case(name)
    T, n = len(xyz), g["n_kf"]
    cloud = cloud_of(xyz)
    cloud["rho_sigma"] = np.stack([np.ones(T, F), sigma], 1)
    row = np.searchsorted(offs[1:], np.arange(T), side="right")
    vm = vmap_np.VoxelMap(voxel)
    vm.integrate(cloud, row.astype(np.int32))
    ol = vo.ObservationLog()
    d = ol.observe((vm.keys, vm.ids), voxel, xyz, row, support, np.arange(n), rows)
    kept, _, rep, _ = voxel_np.voxel_merge(xyz, sigma, voxel, offs)
    ok = voxel_np.cells(xyz, voxel)[1]
    assert d["unmapped"] == int((~ok).sum()) and d["created"] == ol.E
    want = voxcam_np.lists(*voxcam_np.voxel_cameras(support, offs, np.arange(n), rows, rep, len(kept)))
    got = vo.lists(*ol.cameras(vm.M))
    by_pixel = {(int(row[q]), int(q)): want[k] for k, q in enumerate(kept) if ok[q]}  # (pixel = g in cloud_of)
    assert len(by_pixel) == vm.M
    for e in range(vm.M):
        assert got[e] == by_pixel[(int(vm.rec["tag"][e]), int(vm.rec["pixel"][e]))], e


@functools.lru_cache(maxsize=None)
def fixture_sequence(name, voxel=0.02):
    """one integrate-then-observe per keyframe (sigma gate 0.3, the checked rho, the fixtures' short neighbour rows,
    tags = keyframe index): (the map, the log, per call (delta, entries before the call's integrate))"""
    g, xyz, sigma, offs, support, rows = fixture_case(name)
    T = len(xyz)
    cloud = cloud_of(xyz)
    cloud["rho_sigma"] = np.stack([np.ones(T, F), sigma], 1)
    vm, ol, calls = vmap_np.VoxelMap(voxel), vo.ObservationLog(), []
    for k in range(g["n_kf"]):
        a, b = offs[k], offs[k + 1]
        m0 = vm.M
        vm.integrate({f: v[a:b] for f, v in cloud.items()}, np.full(b - a, k, np.int32))
        d = ol.observe((vm.keys, vm.ids), voxel, xyz[a:b], np.zeros(b - a, np.int64), support[a:b], [k], rows[k:k + 1])
        calls.append((d, m0))
    return vm, ol, calls


# voxel 0.02: (E, observations created on entries older than their call summed over the calls, created by the last call,
# of those on older entries, longest list), from an independent dict loop; and E at voxel 0.005
PINNED = {"plane_160x120_n7": (4933, 2256, 485, 317, 8), "plane_64x48_n7": (6879, 2897, 674, 345, 8),
          "plane_96x80_n20": (10204, 7573, 86, 62, 21), "strip_roll_160x120_n7": (6382, 2531, 305, 120, 8)}
PINNED_E_FINE = {"plane_160x120_n7": 37210, "plane_64x48_n7": 16061, "plane_96x80_n20": 50397, "strip_roll_160x120_n7": 39944}
FINAL_M = {"plane_160x120_n7": 686, "plane_64x48_n7": 1008, "plane_96x80_n20": 691, "strip_roll_160x120_n7": 996}


@pytest.mark.parametrize("name", gu.fixture_names())
def test_golden_fixture_pins(name):
    vm, ol, calls = fixture_sequence(name)
    older = [int((ol.entry[d["first_created"]:d["first_created"] + d["created"]] < m0).sum()) for d, m0 in calls]
    offs, _ = ol.cameras(vm.M)
    got = (ol.E, sum(older), calls[-1][0]["created"], older[-1], int(np.diff(offs).max()))
    print(name, "M", vm.M, got)
    assert vm.M == FINAL_M[name]
    assert got == PINNED[name]
    assert all(d["unmapped"] == 0 for d, _ in calls)  # an observe after its integrate: every point has an entry
    assert sum(d["created"] for d, _ in calls) == ol.E


@pytest.mark.parametrize("name", gu.fixture_names())
def test_golden_fixture_pins_fine_voxels(name):
    _, ol, _ = fixture_sequence(name, 0.005)
    assert ol.E == PINNED_E_FINE[name]
