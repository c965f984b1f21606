"""CPU: tests/vmap_np.py (the NumPy statement of the persistent voxel map's semantics, sdm_vmap_*) against a second
formulation -- a plain Python dict loop over the points, exactly as include/sdm_c.h words it -- on random and crafted
clouds; the three invariants of the header (split invariance, agreement with the per-call merge, re-integration); and the
non-vacuity of the golden fixtures the GPU test relies on."""
import math

import numpy as np
import pytest

import golden_util as gu
import vmap_np
import voxel_np
from test_voxel_cpu import _fixture_cloud, _key

f32 = np.float32
SAT = (1 << 32) - 1


class DictMap:
    """the semantics of include/sdm_c.h, point by point"""

    def __init__(self, voxel_size):
        self.inv = f32(1.0) / f32(voxel_size)
        self.entry = {}   # cell -> id
        self.rec = []     # id -> [record tuple, multiplicity, epoch, key of the stored sigma]
        self.points = self.dropped = self.calls = 0

    def _cell(self, p):
        cell = []
        for v in p:
            with np.errstate(invalid="ignore", over="ignore"):
                c = float(f32(v) * self.inv)  # one float32 multiply
            if math.isnan(c) or math.isinf(c) or not (-2.0 ** 20 <= math.floor(c) < 2.0 ** 20):
                return None
            cell.append(math.floor(c))
        return tuple(cell)

    def integrate(self, cloud, tag):
        self.calls += 1
        c, M0 = self.calls, len(self.rec)
        sig_bits = np.ascontiguousarray(cloud["rho_sigma"], f32).reshape(-1, 2)[:, 1].copy().view(np.uint32)
        xyz = np.asarray(cloud["xyz"], f32).reshape(-1, 3)
        dropped, winner = 0, {}
        for g in range(len(xyz)):
            cell = self._cell(xyz[g])
            if cell is None:
                dropped += 1
                continue
            self.points += 1
            record = (xyz[g].tobytes(), int(cloud["pixel"][g]), np.asarray(cloud["rho_sigma"][g], f32).tobytes(),
                      int(cloud["intensity"][g]), int(tag[g]))
            k = _key(int(sig_bits[g]))
            if cell not in self.entry:
                self.entry[cell] = len(self.rec)
                self.rec.append([record, 1, c, k])
                continue
            e = self.rec[self.entry[cell]]
            e[1] = min(e[1] + 1, SAT)
            if k < e[3]:
                e[0], e[2], e[3] = record, c, k
                winner[self.entry[cell]] = g
        self.dropped += dropped
        upd = sorted((g, i) for i, g in winner.items() if i < M0)
        return {"plain_total": len(xyz), "dropped": dropped, "first_created": M0, "created": len(self.rec) - M0,
                "updated": len(upd), "updated_ids": [i for _, i in upd]}

    def info(self):
        return {"voxels": len(self.rec), "points": self.points, "dropped": self.dropped, "calls": self.calls}


def same_delta(a, b, what=""):
    for f in ("plain_total", "dropped", "first_created", "created", "updated"):
        assert int(a[f]) == int(b[f]), (what, f, a[f], b[f])
    assert [int(i) for i in a["updated_ids"]] == [int(i) for i in b["updated_ids"]], what


def same_as_dict(vm, dm, what=""):
    assert vm.info() == dm.info(), what
    got = vm.fetch()
    for i, (record, mult, epoch, _) in enumerate(dm.rec):
        mine = (got["xyz"][i].tobytes(), int(got["pixel"][i]), got["rho_sigma"][i].tobytes(), int(got["intensity"][i]),
                int(got["tag"][i]))
        assert mine == record and int(got["multiplicity"][i]) == mult and int(got["epoch"][i]) == epoch, (what, i)


def same_maps(a, b, epoch=True, what=""):
    """two vmap_np maps byte for byte (epoch and calls optional)"""
    ia, ib = a.info(), b.info()
    if not epoch:
        ia.pop("calls"), ib.pop("calls")
    assert ia == ib, what
    fa, fb = a.fetch(), b.fetch()
    for f in vmap_np.FIELDS:
        if f == "epoch" and not epoch:
            continue
        assert fa[f].tobytes() == fb[f].tobytes(), (what, f)


def make_cloud(rng, T, spread=1.0, nasty=False):
    xyz = rng.uniform(-spread, spread, (T, 3)).astype(f32)
    sigma = rng.choice(np.array([0.01, 0.02, 0.05, 0.011], f32), T)  # many ties, within and across calls
    if nasty:
        big = f32(2.0 ** 20 * 0.25)
        special = [(np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf), (-big, 0, 0), (np.nextafter(-big, f32(-np.inf)), 0, 0),
                   (np.nextafter(big, f32(0)), 0, 0), (big, 0, 0), (-1e-30, 0.1, 0.1), (1e-30, 0.1, 0.1), (-0.0, 0.0, 0.3),
                   (0.0, -0.0, 0.26), (-0.25, 0.0, 0.25)]
        at = rng.choice(T, 3 * len(special), replace=False)
        xyz[at] = np.array(special * 3, f32)
        sigma[rng.choice(T, T // 10, replace=False)] = rng.choice(
            np.array([0.0, -0.0, np.nan, -np.nan, np.inf, 1e-45], f32), T // 10)
    return {"xyz": xyz, "pixel": rng.integers(0, 1 << 26, T).astype(np.uint32),
            "rho_sigma": np.stack([rng.uniform(0.5, 2, T).astype(f32), sigma], 1),
            "intensity": rng.integers(0, 256, T).astype(np.uint8)}


def part(cloud, a, b):
    return {f: v[a:b] for f, v in cloud.items()}


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("voxel", (0.25, 0.3, 0.05, 1e-7, 1000.0))
def test_random_clouds_against_the_dict_loop(seed, voxel):
    rng = np.random.default_rng(seed)
    vm, dm = vmap_np.VoxelMap(voxel), DictMap(voxel)
    seen_update = seen_create = seen_drop = 0
    for call in range(5):
        T = 0 if call == 2 else int(rng.integers(150, 400))  # (an empty call too)
        cloud = make_cloud(rng, T, nasty=T > 0)
        tag = rng.integers(-5, 1000, T).astype(np.int32)
        d1, d2 = vm.integrate(cloud, tag), dm.integrate(cloud, tag)
        same_delta(d1, d2, "call %d" % call)
        same_as_dict(vm, dm, "call %d" % call)
        if call:
            seen_update += d1["updated"]
            seen_create += d1["created"]
        seen_drop += d1["dropped"]
    assert seen_drop > 0
    if voxel in (0.25, 0.3):
        assert seen_update > 0 and seen_create > 0
    if voxel == 1000.0:
        assert seen_update > 0  # (eight voxels around the origin hold nearly every point)
    info = vm.info()
    assert int(vm.fetch()["multiplicity"].astype(np.int64).sum()) == info["points"]


def test_crafted_order_ties_and_signed_zero():
    """the earlier call keeps a tie; -0 beats +0; a NaN sigma with the sign clear loses to everything, with it set wins"""
    xyz = np.full((1, 3), 0.1, f32)

    def one(sigma, pixel):
        return {"xyz": xyz, "pixel": np.array([pixel], np.uint32), "rho_sigma": np.array([[1.0, sigma]], f32),
                "intensity": np.array([pixel], np.uint8)}

    nan_neg = np.array([0xFFC00000], np.uint32).view(f32)[0]
    steps = [(np.nan, 1), (0.02, 1), (0.02, 0), (0.0, 1), (0.0, 0), (-0.0, 1), (-0.0, 0), (nan_neg, 1)]
    vm, dm = vmap_np.VoxelMap(1.0), DictMap(1.0)
    for call, (sigma, upd) in enumerate(steps):
        d = vm.integrate(one(sigma, call), [call])
        same_delta(d, dm.integrate(one(sigma, call), [call]))
        assert d["created"] == (call == 0) and d["updated"] == (upd if call else 0), call
        assert list(d["updated_ids"]) == ([0] if call and upd else [])
    got = vm.fetch()
    assert int(got["multiplicity"][0]) == len(steps) and int(got["epoch"][0]) == len(steps) and int(got["tag"][0]) == len(steps) - 1
    same_as_dict(vm, dm)


def test_multiplicity_saturates():
    vm = vmap_np.VoxelMap(1.0)
    cloud = make_cloud(np.random.default_rng(0), 3, spread=0.1)
    cloud["xyz"] = np.abs(cloud["xyz"])
    vm.integrate(cloud, [0, 0, 0])
    vm.rec["multiplicity"][:] = SAT - 4
    d = vm.integrate(cloud, [1, 1, 1])
    assert int(vm.fetch()["multiplicity"][0]) == SAT - 1 and d["updated"] == 0
    vm.integrate(cloud, [2, 2, 2])
    assert int(vm.fetch()["multiplicity"][0]) == SAT


# I1: any split into consecutive groups leaves the same map except epoch and calls
@pytest.mark.parametrize("seed", range(3))
def test_split_invariance(seed):
    rng = np.random.default_rng(100 + seed)
    T = 900
    cloud = make_cloud(rng, T, nasty=True)
    tag = rng.integers(0, 9, T).astype(np.int32)
    for voxel in (0.25, 0.05, 1000.0):
        whole = vmap_np.VoxelMap(voxel)
        whole.integrate(cloud, tag)
        for cuts in ([0, 300, 600, T], [0, 1, T - 1, T], sorted({0, T} | set(rng.integers(0, T + 1, 6).tolist())), list(range(0, T + 1, 100))):
            split = vmap_np.VoxelMap(voxel)
            created = 0
            for a, b in zip(cuts[:-1], cuts[1:]):
                d = split.integrate(part(cloud, a, b), tag[a:b])
                assert d["first_created"] == created
                created += d["created"]
            same_maps(whole, split, epoch=False, what="voxel %r cuts %r" % (voxel, cuts))


# I2: one call into an empty map = the mergeable kept points of the per-call merge
@pytest.mark.parametrize("seed", range(3))
def test_agreement_with_the_per_call_merge(seed):
    rng = np.random.default_rng(200 + seed)
    T = 800
    cloud = make_cloud(rng, T, nasty=True)
    cloud["pixel"] = rng.permutation(T).astype(np.uint32)  # (tag, pixel) identifies a point
    tag = np.zeros(T, np.int32)
    for voxel in (0.25, 0.05, 1e-7, 1000.0):
        vm = vmap_np.VoxelMap(voxel)
        d = vm.integrate(cloud, tag)
        kept, mult, _, _ = voxel_np.voxel_merge(cloud["xyz"], cloud["rho_sigma"][:, 1], voxel, [0, T])
        _, ok = voxel_np.cells(cloud["xyz"], voxel)
        keep_ok = ok[kept]
        assert d["dropped"] == int((~keep_ok).sum()) and d["created"] == int(keep_ok.sum()) and d["updated"] == 0
        got = vm.fetch()
        o1, o2 = np.argsort(got["pixel"]), np.argsort(cloud["pixel"][kept[keep_ok]])
        for f in ("xyz", "pixel", "rho_sigma", "intensity"):
            assert got[f][o1].tobytes() == cloud[f][kept[keep_ok]][o2].tobytes(), f
        np.testing.assert_array_equal(got["multiplicity"][o1], mult[keep_ok][o2])
        # and the ids are the order of the voxels' first points
        first = {}
        c, _ = voxel_np.cells(cloud["xyz"], voxel)
        for g in np.flatnonzero(ok):
            first.setdefault(tuple(c[g]), g)
        of_entry = [first[tuple(e)] for e in voxel_np.cells(got["xyz"], voxel)[0]]
        assert of_entry == sorted(of_entry) and len(set(of_entry)) == vm.M


# I3: the same cloud again creates and updates nothing and doubles every multiplicity
def test_reintegration():
    rng = np.random.default_rng(300)
    cloud = make_cloud(rng, 700, nasty=True)
    tag = rng.integers(0, 5, 700).astype(np.int32)
    for voxel in (0.25, 0.05):
        vm = vmap_np.VoxelMap(voxel)
        d1 = vm.integrate(cloud, tag)
        before = vm.fetch()
        d2 = vm.integrate(cloud, tag + 100)
        assert d2["created"] == 0 and d2["updated"] == 0 and d2["dropped"] == d1["dropped"] and d2["first_created"] == d1["created"]
        after = vm.fetch()
        for f in vmap_np.FIELDS:
            if f != "multiplicity":
                assert before[f].tobytes() == after[f].tobytes(), f
        np.testing.assert_array_equal(after["multiplicity"], 2 * before["multiplicity"])


def test_fetch_forms():
    rng = np.random.default_rng(5)
    vm = vmap_np.VoxelMap(0.25)
    vm.integrate(make_cloud(rng, 300), np.zeros(300, np.int32))
    full = vm.fetch()
    ids = rng.integers(0, vm.M, 40)
    a, b = vm.fetch(ids=ids), vm.fetch(first=7, count=11)
    for f in vmap_np.FIELDS:
        assert a[f].tobytes() == full[f][ids].tobytes() and b[f].tobytes() == full[f][7:18].tobytes()
    for bad in (dict(first=1, count=vm.M), dict(ids=[vm.M]), dict(first=-1, count=1)):
        with pytest.raises(IndexError):
            vm.fetch(**bad)
    assert list(vmap_np.point_tags([0, 2, 2, 5], [4, 9, 1])) == [4, 4, 1, 1, 1]
    assert list(vmap_np.point_tags([0, 2, 2, 5], [4, 9, 1], [70, 80, 90])) == [70, 70, 90, 90, 90]


# the golden fixtures, one call per keyframe: the last call still creates and still improves entries at 0.02
FINAL_M = {0.02: (686, 1008, 691, 996), 0.005: (6236, 3601, 5960, 7330)}


@pytest.mark.parametrize("idx,name", list(enumerate(gu.fixture_names())))
def test_golden_fixtures_are_not_vacuous(idx, name):
    g = gu.load(name)
    xyz, sigma, slot = _fixture_cloud(g)
    T = len(xyz)
    cloud = {"xyz": xyz, "pixel": np.arange(T, dtype=np.uint32), "rho_sigma": np.stack([np.ones(T, f32), sigma], 1),
             "intensity": np.zeros(T, np.uint8)}
    offs = np.searchsorted(slot, np.arange(g["n_kf"] + 1))
    for voxel in (0.02, 0.005):
        vm = vmap_np.VoxelMap(voxel)
        for k in range(g["n_kf"]):
            d = vm.integrate(part(cloud, offs[k], offs[k + 1]), slot[offs[k]:offs[k + 1]])
            assert d["dropped"] == 0
        print(name, voxel, "M", vm.M, "last call created", d["created"], "updated", d["updated"])
        assert vm.M == FINAL_M[voxel][idx]
        if voxel == 0.02:
            assert d["created"] > 0 and d["updated"] > 0
            assert d["created"] >= 7 and d["updated"] >= 195
        whole = vmap_np.VoxelMap(voxel)
        whole.integrate(cloud, slot)
        same_maps(whole, vm, epoch=False, what=name)
