"""CPU: tests/vmap_import_np.py (the NumPy statement of sdm_vmap_import and sdm_vmap_import_observations) against a second
formulation -- a scalar dict loop over the records and the pairs, exactly as include/sdm_c.h words them -- on random and
crafted sources; the invariants I1 .. I3 and the observation invariants; and the pinned figures of merging the golden
fixtures' two- and three-rank splits, which must reproduce the one-map run."""
import functools

import numpy as np
import pytest

import golden_util as gu
import vmap_import_np as vi
import vmap_np
import vmap_obs_np as vo
from test_vmap_cpu import DictMap, make_cloud, part, same_maps
from test_vmap_obs_cpu import FINAL_M, PINNED, PINNED_E_FINE, cloud_of, fixture_sequence
from test_voxcam_cpu import fixture_case
from test_voxel_cpu import _key

F = np.float32
SAT = (1 << 32) - 1
NOID = 0xFFFFFFFF


class DictImport(DictMap):
    """sdm_vmap_import record by record, on the dict map of test_vmap_cpu"""

    def import_records(self, records):
        xyz = np.asarray(records["xyz"], F).reshape(-1, 3)
        R = len(xyz)
        src = {"xyz": xyz, "rho_sigma": np.asarray(records["rho_sigma"], F).reshape(-1, 2)}
        for f in ("pixel", "intensity", "tag"):  # an absent source reads 0 ...
            src[f] = [0] * R if records.get(f) is None else records[f]
        src["multiplicity"] = [1] * R if records.get("multiplicity") is None else records["multiplicity"]  # ... and this one 1
        self.calls += 1
        c, M0 = self.calls, len(self.rec)
        sig_bits = np.ascontiguousarray(src["rho_sigma"][:, 1]).view(np.uint32)
        dropped, winner, dst = 0, {}, []
        for r in range(len(src["xyz"])):
            m = int(src["multiplicity"][r])
            cell = self._cell(src["xyz"][r]) if m else None
            if cell is None:
                dropped += 1
                dst.append(NOID)
                continue
            self.points += m
            record = (src["xyz"][r].tobytes(), int(src["pixel"][r]), src["rho_sigma"][r].tobytes(), int(src["intensity"][r]),
                      int(src["tag"][r]))  # (the same tuple same_as_dict forms from a fetch)
            k = _key(int(sig_bits[r]))
            if cell not in self.entry:
                self.entry[cell] = len(self.rec)
                self.rec.append([record, m, c, k])
                dst.append(self.entry[cell])
                continue
            i = self.entry[cell]
            dst.append(i)
            e = self.rec[i]
            e[1] = min(e[1] + m, SAT)
            if k < e[3]:
                e[0], e[2], e[3] = record, c, k
                winner[i] = r
        self.dropped += dropped
        upd = sorted((r, i) for i, r in winner.items() if i < M0)
        return {"total": len(dst), "dropped": dropped, "first_created": M0, "created": len(self.rec) - M0, "updated": len(upd),
                "updated_ids": [i for _, i in upd], "dst_ids": dst}


class DictPairs:
    """sdm_vmap_import_observations pair by pair"""

    def __init__(self):
        self.log, self.have = [], set()

    def import_observations(self, M, entry, tag, entry_map=None):
        d = {"total": len(entry), "rejected": 0, "first_created": len(self.log), "created": 0}
        for k in range(len(entry)):
            e, t = int(entry[k]), int(tag[k])
            if entry_map is not None:
                e = int(entry_map[e]) if e < len(entry_map) else NOID
            if e >= M or t < 0:
                d["rejected"] += 1
            elif (e, t) not in self.have:
                self.have.add((e, t))
                self.log.append((e, t))
                d["created"] += 1
        return d


def same_import(a, b, what=""):
    for f in vi.DELTA:
        assert int(a[f]) == int(b[f]), (what, f, a[f], b[f])
    for f in ("updated_ids", "dst_ids"):
        assert [int(i) for i in a[f]] == [int(i) for i in b[f]], (what, f)


def same_as_dict(vm, dm, what=""):
    assert vm.info() == dm.info(), what
    got = vm.fetch()
    for i, (record, mult, epoch, _) in enumerate(dm.rec):
        mine = (got["xyz"][i].tobytes(), int(got["pixel"][i]), got["rho_sigma"][i].tobytes(), int(got["intensity"][i]),
                int(got["tag"][i]))
        assert mine == record and int(got["multiplicity"][i]) == mult and int(got["epoch"][i]) == epoch, (what, i)


def make_records(rng, R, nasty=True, spread=1.0):
    """a cloud of test_vmap_cpu with tags of both signs and multiplicities 0, 1 and large"""
    rec = make_cloud(rng, R, spread=spread, nasty=nasty)
    rec["tag"] = rng.integers(-5, 40, R).astype(np.int32)
    rec["multiplicity"] = rng.choice(np.array([0, 1, 1, 1, 2, 77, 1 << 20, (1 << 31) + 1, SAT], np.uint32), R)
    if R >= 8:  # duplicate voxels inside one import, with a tie and a strict win among them
        rec["xyz"][1] = rec["xyz"][0]
        rec["xyz"][5] = rec["xyz"][0]
        rec["rho_sigma"][1, 1] = rec["rho_sigma"][0, 1]
        rec["multiplicity"][[0, 1, 5]] = (3, 4, 5)
    return rec


@pytest.mark.parametrize("voxel", [0.25, 0.05, 1e-7, 1000.0])
@pytest.mark.parametrize("seed", range(3))
def test_random_records_against_the_dict_loop(seed, voxel):
    rng = np.random.default_rng(100 + seed)
    vm, dm = vmap_np.VoxelMap(voxel), DictImport(voxel)
    seen_drop = seen_upd = 0
    for call in range(4):
        if call == 1:  # an integrate between the imports: the call number counts both
            cloud = make_cloud(rng, 300, nasty=True)
            tag = rng.integers(0, 9, 300).astype(np.int32)
            vm.integrate(cloud, tag), dm.integrate(cloud, tag)
            continue
        rec = make_records(rng, 700)
        if call == 2:  # optional sources absent: zeros, and multiplicity 1
            rec = {"xyz": rec["xyz"], "rho_sigma": rec["rho_sigma"]}
        a, b = vi.import_records(vm, rec), dm.import_records(rec)
        same_import(a, b, (seed, voxel, call))
        same_as_dict(vm, dm, (seed, voxel, call))
        seen_drop += a["dropped"]
        seen_upd += a["updated"]
        assert ((a["dst_ids"] == NOID).sum()) == a["dropped"]
    assert seen_drop > 0 and vm.calls == 4
    if voxel != 1e-7:
        assert seen_upd > 0
    empty = vi.import_records(vm, {"xyz": np.zeros((0, 3), F), "rho_sigma": np.zeros((0, 2), F)})
    same_import(empty, dm.import_records({"xyz": np.zeros((0, 3), F), "rho_sigma": np.zeros((0, 2), F)}))
    assert empty["total"] == 0 and vm.calls == 5


def test_saturation_within_one_call_and_across_calls():
    big = (1 << 31) + 1
    rec = {"xyz": np.array([[0.1, 0.1, 0.1], [0.12, 0.1, 0.1], [0.9, 0.9, 0.9]], F), "rho_sigma": np.array([[1, 0.1]] * 3, F),
           "multiplicity": np.array([big, big, 5], np.uint32)}
    vm, dm = vmap_np.VoxelMap(0.25), DictImport(0.25)
    same_import(vi.import_records(vm, rec), dm.import_records(rec))
    same_as_dict(vm, dm)
    wrapped = (big + big) & SAT
    assert wrapped == 2 and wrapped != SAT  # what a wrapping 32-bit per-call count would have given
    assert vm.fetch()["multiplicity"].tolist() == [SAT, 5]
    assert vm.points == 2 * big + 5  # the 64-bit sum does not saturate
    same_import(vi.import_records(vm, rec), dm.import_records(rec))  # a saturated entry stays saturated
    assert vm.fetch()["multiplicity"].tolist() == [SAT, 10]
    one = {"xyz": rec["xyz"][2:], "rho_sigma": rec["rho_sigma"][2:], "multiplicity": np.array([SAT - 9], np.uint32)}
    vi.import_records(vm, one)
    assert vm.fetch()["multiplicity"].tolist() == [SAT, SAT]  # 10 + (SAT - 9) clamps, and does not wrap to 0


@pytest.mark.parametrize("seed", range(3))
def test_i1_split_invariance(seed):
    rng = np.random.default_rng(200 + seed)
    rec = make_records(rng, 900)
    base = make_cloud(rng, 400, nasty=True)
    whole = vmap_np.VoxelMap(0.25)
    whole.integrate(base, np.zeros(400, np.int32))
    d = vi.import_records(whole, rec)
    assert d["created"] > 0 and d["updated"] > 0
    for cuts in ([450], [1, 899], sorted(rng.choice(np.arange(1, 900), 5, replace=False).tolist()), [0, 0, 900]):
        vm = vmap_np.VoxelMap(0.25)
        vm.integrate(base, np.zeros(400, np.int32))
        dst = []
        for a, b in zip([0] + cuts, cuts + [900]):
            dst.append(vi.import_records(vm, part(rec, a, b))["dst_ids"])
        same_maps(vm, whole, epoch=False, what=cuts)
        assert np.array_equal(np.concatenate(dst), d["dst_ids"]), cuts


@pytest.mark.parametrize("voxel", [0.25, 0.05])
@pytest.mark.parametrize("seed", range(3))
def test_i2_importing_a_fetched_map_is_integrating_its_clouds(seed, voxel):
    rng = np.random.default_rng(300 + seed)
    P = [make_cloud(rng, 500, nasty=True) for _ in range(2)]
    Q = [make_cloud(rng, 500, nasty=True) for _ in range(3)]
    A, B, both = vmap_np.VoxelMap(voxel), vmap_np.VoxelMap(voxel), vmap_np.VoxelMap(voxel)
    for i, cl in enumerate(P):
        A.integrate(cl, np.full(500, i, np.int32)), both.integrate(cl, np.full(500, i, np.int32))
    for i, cl in enumerate(Q):
        B.integrate(cl, np.full(500, 10 + i, np.int32)), both.integrate(cl, np.full(500, 10 + i, np.int32))
    d = vi.import_records(A, B.fetch())
    assert d["dropped"] == 0 and d["total"] == B.M and d["created"] > 0 and d["updated"] > 0
    fa, fb = A.fetch(), both.fetch()
    for f in vmap_np.FIELDS:
        if f != "epoch":
            assert fa[f].tobytes() == fb[f].tobytes(), f
    assert (A.M, A.points) == (both.M, both.points)
    assert np.array_equal(A.keys, both.keys) and np.array_equal(A.ids, both.ids)


@pytest.mark.parametrize("seed", range(2))
def test_i3_round_trip_reproduces_the_map(seed):
    rng = np.random.default_rng(400 + seed)
    vm = vmap_np.VoxelMap(0.05)
    for i in range(3):
        vm.integrate(make_cloud(rng, 600, nasty=True), np.full(600, i, np.int32))
    back = vmap_np.VoxelMap(0.05)
    d = vi.import_records(back, vm.fetch())
    assert d["created"] == vm.M and d["dropped"] == 0 and np.array_equal(d["dst_ids"], np.arange(vm.M))
    fa, fb = back.fetch(), vm.fetch()
    for f in vmap_np.FIELDS:
        if f != "epoch":
            assert fa[f].tobytes() == fb[f].tobytes(), f
    assert back.points == vm.points and (back.fetch()["epoch"] == 1).all()
    # another voxel size re-bins: the coarser map has fewer entries and the same number of points
    coarse = vmap_np.VoxelMap(0.5)
    vi.import_records(coarse, vm.fetch())
    assert 0 < coarse.M < vm.M and coarse.points == vm.points


@pytest.mark.parametrize("seed", range(3))
def test_random_pairs_against_the_dict_loop(seed):
    rng = np.random.default_rng(500 + seed)
    M, P = 50, 1500
    ol, dl = vo.ObservationLog(), DictPairs()
    for call in range(3):
        entry = rng.integers(0, 70, P).astype(np.uint32)  # some >= M
        tag = rng.integers(-3, 12, P).astype(np.int32)    # some < 0
        tag[rng.integers(0, P, 5)] = (1 << 31) - 1
        emap = None
        if call == 1:  # through a map that carries dropped records and is shorter than some entries
            emap = rng.integers(0, 60, 64).astype(np.uint32)
            emap[rng.integers(0, 64, 8)] = NOID
        a, b = vi.import_observations(ol, M, entry, tag, emap), dl.import_observations(M, entry, tag, emap)
        assert a == b, (call, a, b)
        assert a["rejected"] > 0 and a["created"] > 0
        assert list(zip(ol.entry.tolist(), ol.tag.tolist())) == dl.log
    again = vi.import_observations(ol, M, entry, tag)  # the same pairs again create nothing
    assert again["created"] == 0 and again["first_created"] == ol.E and ol.calls == 4
    assert vi.import_observations(ol, M, np.zeros(0, np.uint32), np.zeros(0, np.int32)) == \
        {"total": 0, "rejected": 0, "first_created": ol.E, "created": 0}


def test_pairs_split_invariance_and_order_independent_lists():
    rng = np.random.default_rng(7)
    M, P = 40, 2000
    entry, tag = rng.integers(0, 45, P).astype(np.uint32), rng.integers(-1, 9, P).astype(np.int32)
    whole = vo.ObservationLog()
    vi.import_observations(whole, M, entry, tag)
    for cuts in ([1000], [1, 2, 1999], [0, 2000]):
        ol = vo.ObservationLog()
        for a, b in zip([0] + cuts, cuts + [P]):
            vi.import_observations(ol, M, entry[a:b], tag[a:b])
        assert np.array_equal(ol.entry, whole.entry) and np.array_equal(ol.tag, whole.tag), cuts
    rev = vo.ObservationLog()
    for a, b in ((1000, 2000), (0, 1000)):
        vi.import_observations(rev, M, entry[a:b], tag[a:b])
    assert np.array_equal(rev.pairs, whole.pairs) and not np.array_equal(rev.entry, whole.entry)
    for x, y in zip(rev.cameras(M), whole.cameras(M)):
        assert np.array_equal(x, y)


# ---- the golden fixtures: keyframes split over ranks, rank r + 1 imported into rank 0 in rank order ------------------------
@functools.lru_cache(maxsize=None)
def rank_sequence(name, voxel, lo, hi):
    """fixture_sequence's recipe for the keyframes lo .. hi - 1 alone: (the map, the log)"""
    g, xyz, sigma, offs, support, rows = fixture_case(name)
    cloud = cloud_of(xyz)
    cloud["rho_sigma"] = np.stack([np.ones(len(xyz), F), sigma], 1)
    vm, ol = vmap_np.VoxelMap(voxel), vo.ObservationLog()
    for k in range(lo, hi):
        a, b = offs[k], offs[k + 1]
        vm.integrate({f: v[a:b] for f, v in cloud.items()}, np.full(b - a, k, np.int32))
        ol.observe((vm.keys, vm.ids), voxel, xyz[a:b], np.zeros(b - a, np.int64), support[a:b], [k], rows[k:k + 1])
    return vm, ol


def merged(name, voxel, world, importer=None):
    """rank 0's map and log after importing ranks 1 .. world - 1 in rank order; the figures of every import"""
    n = gu.load(name)["n_kf"]
    maps = [rank_sequence(name, voxel, (n * r) // world, (n * (r + 1)) // world) for r in range(world)]
    vm0, ol0 = maps[0]
    vm, ol = vmap_np.VoxelMap(voxel), vo.ObservationLog()
    vm.rec = {f: v.copy() for f, v in vm0.rec.items()}
    vm.keys, vm.ids, vm.points, vm.dropped, vm.calls = vm0.keys.copy(), vm0.ids.copy(), vm0.points, vm0.dropped, vm0.calls
    ol.entry, ol.tag, ol.pairs, ol.calls = ol0.entry.copy(), ol0.tag.copy(), ol0.pairs.copy(), ol0.calls
    figures = []
    for vr, lr in maps[1:]:
        d = vi.import_records(vm, vr.fetch())
        o = vi.import_observations(ol, vm.M, lr.entry, lr.tag, d["dst_ids"])
        assert d["dropped"] == 0 and o["rejected"] == 0
        figures.append((vr.M, d["created"], d["updated"], lr.E, o["created"]))
    return vm, ol, figures


def same_as_one_map(name, voxel, vm, ol):
    one_vm, one_ol, _ = fixture_sequence(name, voxel)
    fa, fb = vm.fetch(), one_vm.fetch()
    for f in vmap_np.FIELDS:
        if f != "epoch":
            assert fa[f].tobytes() == fb[f].tobytes(), (name, f)
    assert (vm.M, vm.points) == (one_vm.M, one_vm.points)
    assert ol.E == one_ol.E and np.array_equal(ol.pairs, one_ol.pairs)
    for x, y in zip(ol.cameras(vm.M), one_ol.cameras(one_vm.M)):
        assert np.array_equal(x, y)


# (rank 1's M, import created, import updated, rank 1's E, pairs created) of the two-rank merge at voxel 0.02
PINNED_MERGE = {"plane_160x120_n7": (645, 73, 421, 2788, 1987), "plane_64x48_n7": (893, 129, 194, 3824, 2542),
                "plane_96x80_n20": (637, 115, 283, 5920, 4759), "strip_roll_160x120_n7": (855, 174, 211, 3715, 2235)}


def scalar_merge_figures(name, voxel=0.02):
    """the same figures from the dict loops alone"""
    n = gu.load(name)["n_kf"]
    vm0, ol0 = rank_sequence(name, voxel, 0, n // 2)
    vm1, ol1 = rank_sequence(name, voxel, n // 2, n)
    dm = DictImport(voxel)
    d0 = dm.import_records(vm0.fetch())  # (I3: rank 0's map, rebuilt record by record)
    assert d0["created"] == vm0.M
    dp = DictPairs()
    dp.import_observations(vm0.M, ol0.entry, ol0.tag)
    d = dm.import_records(vm1.fetch())
    o = dp.import_observations(len(dm.rec), ol1.entry, ol1.tag, d["dst_ids"])
    return (vm1.M, d["created"], d["updated"], ol1.E, o["created"]), len(dm.rec), len(dp.log)


@pytest.mark.parametrize("name", gu.fixture_names())
def test_golden_two_rank_merge_pins(name):
    vm, ol, figures = merged(name, 0.02, 2)
    scalar, m, e = scalar_merge_figures(name)
    print(name, "numpy", figures[0], "scalar", scalar, "M", vm.M, "E", ol.E)
    assert figures[0] == PINNED_MERGE[name]
    assert scalar == PINNED_MERGE[name]
    assert vm.M == m == FINAL_M[name] and ol.E == e == PINNED[name][0]
    same_as_one_map(name, 0.02, vm, ol)


@pytest.mark.parametrize("name", gu.fixture_names())
def test_golden_three_rank_merge_and_fine_voxels(name):
    vm, ol, _ = merged(name, 0.02, 3)
    assert vm.M == FINAL_M[name] and ol.E == PINNED[name][0]
    same_as_one_map(name, 0.02, vm, ol)
    for world in (2, 3):
        vm, ol, _ = merged(name, 0.005, world)
        assert ol.E == PINNED_E_FINE[name]
        same_as_one_map(name, 0.005, vm, ol)
