"""GPU: the observation log on the persistent voxel map (sdm_vmap_observe, sdm_vmap_get_obs_info,
sdm_vmap_fetch_observations, sdm_vmap_fetch_cameras / Engine.vmap_observe, .vmap_obs_info, .vmap_fetch_observations,
.vmap_fetch_cameras) against tests/vmap_obs_np.py fed the engine's own extract_points_support(fields=ALL) and the entries
of tests/vmap_np.py -- after every call the delta, the info, a full fetch of the log and a full fetch of the camera lists.
Everything is an integer: every comparison is for equality.

Not run here: the refusals E + B > 2^30 and T x Lmax > 2^40, which no image a test can afford reaches."""
import ctypes
import sys

import numpy as np
import pytest

import golden_util as gu
import vmap_np
import vmap_obs_np as vo
import voxel_np
from test_gpu_extract import ALL, EINVAL, ESTATE, _state, pipeline
from test_gpu_vmap import _crafted_engine, same_fetch, same_info, snapshot, unchanged

pytestmark = pytest.mark.gpu

TOP = (1 << 31) - 1


@pytest.fixture(scope="module")
def engines(pkg, gpu_ok):
    """the golden fixtures run through the pipeline once each; shared by the tests that change no plane"""
    made = {}

    def get(name):
        if name not in made:
            g = gu.load(name)
            made[name] = (g, pipeline(pkg, g))
        return made[name]

    yield get
    for _, eng in made.values():
        eng.close()


class Mirror:
    """tests/vmap_np.py's map plus tests/vmap_obs_np.py's log"""

    def __init__(self, voxel):
        self.voxel = voxel
        self.vm = vmap_np.VoxelMap(voxel)
        self.ol = vo.ObservationLog()

    def clear(self):
        self.vm.clear()
        self.ol.clear()

    def integrate(self, eng, slots, tags=None, **kw):
        plain = eng.extract_points(slots, fields=ALL, **kw)
        return self.vm.integrate(plain, vmap_np.point_tags(plain["offsets"], slots, tags))

    def observe(self, eng, slots, nbrs=None, tags=None, nbr_tags=None, **kw):
        if len(slots) == 0:
            plain, sup = {"xyz": np.zeros((0, 3), np.float32), "offsets": np.zeros(1, np.int64)}, np.zeros(0, np.uint64)
        elif nbrs is None:
            plain, sup = eng.extract_points(slots, fields=ALL, **kw), None
        else:
            plain = eng.extract_points_support(slots, nbrs, fields=ALL, **kw)
            sup = plain["support"]
        row = np.repeat(np.arange(len(slots)), np.diff(plain["offsets"]))
        own = slots if tags is None else tags
        cols = None if nbrs is None else (nbrs if nbr_tags is None else nbr_tags)
        return self.ol.observe((self.vm.keys, self.vm.ids), self.voxel, plain["xyz"], row, sup, own, cols)


def obs_snapshot(eng):
    cams = eng.vmap_fetch_cameras()
    return eng.vmap_obs_info(), {f: np.array(a) for f, a in eng.vmap_fetch_observations().items()}, \
        {f: np.array(a) for f, a in cams.items()}


def obs_unchanged(eng, snap, what=""):
    info, log, cams = snap
    assert eng.vmap_obs_info() == info, what
    same_fetch(eng.vmap_fetch_observations(), log, what)
    same_fetch(eng.vmap_fetch_cameras(), cams, what)


def same_obs(eng, ref, what=""):
    """the info, a full fetch of the log and a full fetch of the lists, as bits"""
    info = eng.vmap_obs_info()
    assert {f: info[f] for f in ("observations", "calls")} == ref.ol.info(), (what, info, ref.ol.info())
    if info["table_slots"]:
        assert info["table_slots"] >= max(1024, 2 * info["observations"]) and info["table_slots"] & (info["table_slots"] - 1) == 0
    log = eng.vmap_fetch_observations()
    assert log["entry"].dtype == np.uint32 and log["tag"].dtype == np.int32
    same_fetch(log, ref.ol.fetch(), what + " log")
    offs, tags = ref.ol.cameras(ref.vm.M)
    cams = eng.vmap_fetch_cameras()
    same_fetch(cams, {"cam_offsets": offs, "cam_tags": tags}, what + " lists")
    return info, log, cams


def step(eng, ref, slots, nbrs=None, tags=None, nbr_tags=None, what="", **kw):
    """one observe against the restatement"""
    exp = ref.observe(eng, slots, nbrs, tags, nbr_tags, **kw)
    got = eng.vmap_observe(slots, nbrs, tags, nbr_tags, **kw)
    assert got == exp, (what, got, exp)
    same_obs(eng, ref, what)
    return got


def both(eng, ref, slots, tags=None, **kw):
    exp = ref.integrate(eng, slots, tags, **kw)
    got = eng.vmap_integrate(slots, tags, **kw)
    assert (got["created"], got["updated"]) == (exp["created"], exp["updated"])
    return got


# 1. the golden fixtures, one integrate-then-observe per keyframe with the fixture's full neighbour rows
@pytest.mark.parametrize("src", (1, 0))
@pytest.mark.parametrize("name,voxel", [("plane_64x48_n7", 0.02), ("plane_64x48_n7", 0.005), ("plane_96x80_n20", 0.02)])
def test_golden_fixtures(engines, name, voxel, src):
    g, eng = engines(name)
    refs = list(range(g["n_kf"]))
    kw = dict(source=src, max_sigma=0.3)
    eng.vmap_open(voxel)
    try:
        ref = Mirror(voxel)
        same_obs(eng, ref, "empty map")
        assert eng.vmap_obs_info() == {"observations": 0, "calls": 0, "table_slots": 0, "rehashes": 0}
        older, first = 0, None
        for k in refs:
            what = "%s src %d voxel %r keyframe %d" % (name, src, voxel, k)
            m0 = ref.vm.M
            both(eng, ref, [k], **kw)
            same_obs(eng, ref, what + " integrated")  # the lists survive growth; new entries read empty
            got = step(eng, ref, [k], g["nbrs"][[k]], what=what, **kw)
            assert got["unmapped"] == 0  # observed after its integrate: every point has an entry
            older += int((ref.ol.entry[got["first_created"]:] < m0).sum())
            first = first or got
        info, fin = eng.vmap_obs_info(), eng.vmap_info()
        print("%s src %d voxel %r: E %d on M %d, %d on older entries, %s" % (name, src, voxel, info["observations"], fin["voxels"],
                                                                          older, info))
        assert info["observations"] > fin["voxels"] > 500 and older > 0
        same_info(eng, ref.vm, name)  # the map is read, not changed
        same_fetch(eng.vmap_fetch(), ref.vm.fetch(), name)
        if voxel == 0.005:
            assert info["rehashes"] >= 2
            # the log outgrew what the first call reserved (E + B = its plain points x its row's tags), and the entries
            # outgrew the records the first integrate made: log and per-entry arrays were copied
            assert info["observations"] > first["plain_total"] * (g["n"] + 1)
            assert fin["voxels"] > first["plain_total"]
    finally:
        eng.vmap_close()


# 2. crafted maps
@pytest.mark.parametrize("W,H", [(32, 24), (64, 48)])
def test_crafted_maps(pkg, gpu_ok, W, H):
    rng = np.random.default_rng(W)
    eng, rho, sigma = _crafted_engine(pkg, W, H, rng)
    for s in range(3):
        eng.upload_depth(s, rho, sigma)  # (the third slot's K: non-finite and out of range)
    pose = np.eye(4, dtype=np.float32)[:3].copy()
    pose[:, 3] = (-500.0, -500.0, -500.0)  # the centre at (500, 500, 500): one cell of edge 1000 holds every finite point
    for s in (0, 1):
        eng.set_pose(s, pose)
    eng.pointset([0, 1, 2], source=0)
    kw = dict(source=0, max_sigma=0.01, min_rho=-1.0)
    slots = [0, 1, 2]
    table = np.array([[1, 1, 0, 2], [1, 0, 0, 2], [2, 2, 2, 2]], np.int32)  # repeated and self columns
    far = ~voxel_np.cells(eng.extract_points([2], fields=("xyz",), **kw)["xyz"], 1000.0)[1]
    assert 0 < int(far.sum())
    for voxel in (1000.0, 0.01):
        what = "crafted %dx%d voxel %r" % (W, H, voxel)
        eng.vmap_open(voxel)
        ref = Mirror(voxel)
        # observe BEFORE integrate: everything is unmapped and nothing is created
        got = step(eng, ref, slots, table, what=what + " empty map", **kw)
        assert got == {"plain_total": 3 * W * H, "unmapped": 3 * W * H, "candidates": 0, "first_created": 0, "created": 0}
        for s in slots:
            both(eng, ref, [s], **kw)
        snap = snapshot(eng)
        M = snap[0]["voxels"]
        got = step(eng, ref, slots, table, what=what + " table", **kw)
        assert got["candidates"] > got["plain_total"] - got["unmapped"] > 0  # neighbours confirm points
        if voxel == 1000.0:
            # every lane of every wave hits the same few pairs
            assert M <= 2 and got["unmapped"] >= int(far.sum()) and got["created"] <= 3 * M
            assert sorted(set(ref.ol.tag.tolist())) == [0, 1, 2]
            lists = vo.lists(*ref.ol.cameras(M))
            assert lists[0] == [0, 1, 2] and got["created"] == sum(len(c) for c in lists)
        else:
            assert M > W * H // 8  # nearly every distinct point is an entry of its own
        assert step(eng, ref, slots, table, what=what + " again", **kw)["created"] == 0
        # two slots sharing one tag, the ends of the tag range, columns renamed so that two carry one tag
        nt = np.array([[7, 8, 7, TOP], [TOP, TOP, 0, 7], [5, 5, 5, 5]], np.int32)
        got = step(eng, ref, slots, table, [TOP, TOP, 0], nt, what=what + " tags", **kw)
        assert got["created"] > 0 and TOP in ref.ol.tag and 0 in ref.ol.tag
        # no neighbour table: the own tag alone
        got = step(eng, ref, [1, 0], None, [11, 12], what=what + " no table", **kw)
        assert got["candidates"] == got["plain_total"] - got["unmapped"] and got["created"] > 0
        # a call without a point and a call without a slot
        got = step(eng, ref, slots, table, what=what + " T = 0", source=0, max_sigma=0.01, min_rho=1e30)
        assert got["plain_total"] == 0 and got["first_created"] == ref.ol.E
        got = step(eng, ref, [], None, what=what + " n = 0", **kw)
        assert got["plain_total"] == 0 and eng.vmap_obs_info()["calls"] == ref.ol.calls
        unchanged(eng, snap, what)  # the map is read, not changed
        eng.vmap_close()
    eng.close()


def test_bit_63_of_a_64_column_row(pkg, gpu_ok):
    W, H = 32, 24
    rng = np.random.default_rng(63)
    f = np.float32
    eng = pkg.Engine(W, H, 3, max_neighbours=64)  # (_crafted_engine's scene with room for a full row)
    im = rng.integers(0, 256, (H, W)).astype(np.uint8)
    pose = np.eye(4, dtype=f)[:3].copy()
    pose[:, 3] = (8.0, 6.0, 1.0)
    for s in range(3):
        eng.upload_image(s, im, np.array([1, 1, 2, 2], f), pose)
    rho = rng.choice(np.array([1, 1, 2, 4], f), (H, W))
    sigma = np.full((H, W), 0.004, f)
    for s in range(3):
        eng.upload_depth(s, rho, sigma)
    eng.pointset([0, 1, 2], source=0)
    kw = dict(source=0, max_sigma=0.01, min_rho=-1.0)
    nbrs = np.zeros((2, 64), np.int32)  # column 63 alone names the slot that confirms
    nbrs[0, 63], nbrs[1, 63] = 1, 0
    nbrs[0, :63], nbrs[1, :63] = 0, 1  # (self columns, which nbr_tags gives tags of their own)
    nt = np.arange(100, 228, dtype=np.int32).reshape(2, 64)
    eng.vmap_open(0.25)
    ref = Mirror(0.25)
    both(eng, ref, [0, 1], [50, 60], **kw)
    sup = eng.extract_points_support([0, 1], nbrs, fields=(), **kw)["support"]
    assert (sup >> np.uint64(63)).any()
    step(eng, ref, [0, 1], nbrs, [50, 60], nt, what="64 columns", **kw)
    assert 163 in ref.ol.tag and 227 in ref.ol.tag
    eng.vmap_close()
    eng.close()


# 3. the invariants on the device
def test_invariants(engines):
    g, eng = engines("plane_96x80_n20")
    refs = list(range(g["n_kf"]))
    rows = np.ascontiguousarray(g["nbrs"][:, :3])
    kw = dict(max_sigma=0.3)
    voxel = 0.02
    eng.vmap_open(voxel)
    try:
        ref = Mirror(voxel)
        both(eng, ref, refs, **kw)
        M = ref.vm.M
        whole = step(eng, ref, refs, rows, what="one call", **kw)
        assert whole["created"] > 2 * M
        one = obs_snapshot(eng)
        # O2: again, nothing
        again = eng.vmap_observe(refs, rows, **kw)
        assert again == dict(whole, first_created=whole["created"], created=0)
        assert eng.vmap_fetch_observations()["entry"].tobytes() == one[1]["entry"].tobytes()
        # O1: any split into consecutive groups leaves a byte-identical log
        rng = np.random.default_rng(4)
        n = len(refs)
        for cut in (list(range(n + 1)), [0, 0, 9, 9, n], sorted({0, n} | set(rng.integers(1, n, 3).tolist()))):
            eng.vmap_clear()
            eng.vmap_integrate(refs, updated=False, **kw)
            made = 0
            for a, b in zip(cut[:-1], cut[1:]):
                made += eng.vmap_observe(refs[a:b], rows[a:b], **kw)["created"]
            assert made == whole["created"]
            same_fetch(eng.vmap_fetch_observations(), one[1], "cut %r" % (cut,))
            same_fetch(eng.vmap_fetch_cameras(), one[2], "cut %r" % (cut,))
        # O4: the order of the calls changes the log's order, not the lists
        eng.vmap_clear()
        eng.vmap_integrate(refs, updated=False, **kw)
        for blk in (refs[13:], refs[5:13], refs[:5]):
            eng.vmap_observe(blk, rows[blk], **kw)
        same_fetch(eng.vmap_fetch_cameras(), one[2], "order")
        log = eng.vmap_fetch_observations()
        assert log["entry"].tobytes() != one[1]["entry"].tobytes()
        key = lambda l: np.sort((l["entry"].astype(np.int64) << 32) | l["tag"])
        np.testing.assert_array_equal(key(log), key(one[1]))
        # O3: every entry's list is the per-call merge's list of the kept point with the same (tag, pixel)
        vox = eng.extract_points_voxel_cameras(refs, rows, voxel, fields=ALL, **kw)
        ok = voxel_np.cells(vox["xyz"], voxel)[1]
        tag = vmap_np.point_tags(vox["offsets"], refs)
        want = vo.lists(vox["cam_offsets"], vox["cam_slots"])
        by = {(int(tag[k]), int(vox["pixel"][k])): want[k] for k in np.flatnonzero(ok)}
        rec = eng.vmap_fetch(fields=("tag", "pixel"))
        got = vo.lists(one[2]["cam_offsets"], one[2]["cam_tags"])
        assert len(by) == M == len(got)
        for e in range(M):
            assert got[e] == by[(int(rec["tag"][e]), int(rec["pixel"][e]))], e
        plain = eng.extract_points(refs, fields=("xyz",), **kw)
        assert whole["unmapped"] == int((~voxel_np.cells(plain["xyz"], voxel)[1]).sum())
    finally:
        eng.vmap_close()


# 4. growth: the lists survive record growth and rehashes, new entries read empty; clear; the same sequence again
def test_growth_and_clear(engines):
    g, eng = engines("plane_64x48_n7")
    refs = list(range(g["n_kf"]))
    rows = np.ascontiguousarray(g["nbrs"][:, :3])
    kw = dict(max_sigma=0.3)
    eng.vmap_open(0.005)
    try:
        ref = Mirror(0.005)

        def sequence():
            both(eng, ref, [0, 1], **kw)
            step(eng, ref, [0, 1], rows[[0, 1]], what="first observe", **kw)
            M0, slots0 = eng.vmap_info()["voxels"], eng.vmap_obs_info()["table_slots"]
            old = eng.vmap_fetch_cameras()
            assert old["cam_offsets"][-1] > M0
            for k in refs[2:]:
                both(eng, ref, [k], **kw)
            _, _, got = same_obs(eng, ref, "grown")  # records (and the per-entry arrays with them) grew between observes
            assert got["cam_offsets"][:M0 + 1].tobytes() == old["cam_offsets"].tobytes()
            assert got["cam_tags"].tobytes() == old["cam_tags"].tobytes()
            assert (got["cam_offsets"][M0:] == got["cam_offsets"][M0]).all()  # entries created later read empty
            for k in refs[2:]:
                step(eng, ref, [k], rows[[k]], [100 + k], rows[[k]] + 100, what="observe after growth", **kw)
            return M0, slots0, eng.vmap_info(), obs_snapshot(eng)

        M0, slots0, info, first = sequence()
        assert info["voxels"] > 2 * M0 and first[0]["table_slots"] > slots0 and first[0]["rehashes"] >= 1
        eng.vmap_clear()
        ref.clear()
        assert eng.vmap_obs_info() == dict(first[0], observations=0, calls=0, rehashes=0)  # the capacity kept
        assert len(eng.vmap_fetch_observations()["entry"]) == 0
        both(eng, ref, refs, **kw)
        same_obs(eng, ref, "after clear")  # every list empty
        eng.vmap_clear()
        ref.clear()
        _, _, _, second = sequence()
        assert second[0] == dict(first[0], rehashes=0)  # (the set kept is large enough)
        for a, b in zip(first[1:], second[1:]):
            same_fetch(a, b, "the same sequence again")
    finally:
        eng.vmap_close()


# 5. fetches: pageable, pinned, device; range and ids; repeated ids; single fields; exact and short capacities
def test_destinations_and_capacity(pkg, engines):
    torch = pytest.importorskip("torch")
    g, eng = engines("plane_96x80_n20")
    kw = dict(max_sigma=0.3)
    slots = [7, 1, 12, 0]
    rows = np.ascontiguousarray(g["nbrs"][slots][:, :3])
    eng.vmap_open(0.02)
    try:
        eng.vmap_integrate(slots, updated=False, **kw)
        M = eng.vmap_info()["voxels"]
        assert M > 300
        ids = np.concatenate([np.random.default_rng(1).integers(0, M, 500), [M - 1, 0, 0]]).astype(np.uint32)
        dev_ids = torch.from_numpy(ids.view(np.int32)).cuda()

        def pick(offs, tags, sel):
            ls = [tags[offs[e]:offs[e + 1]] for e in sel]
            return {"cam_offsets": np.concatenate([[0], np.cumsum([len(c) for c in ls])]).astype(np.int64),
                    "cam_tags": (np.concatenate(ls) if ls else np.zeros(0)).astype(np.int32)}

        def forms(log, offs, tags, what):
            E, total = len(log["entry"]), len(tags)
            # the log
            same_fetch(eng.vmap_fetch_observations(), log, what)
            same_fetch(eng.vmap_fetch_observations(first=E, count=0), {f: a[E:] for f, a in log.items()}, what + " empty range")
            for f in log:
                same_fetch(eng.vmap_fetch_observations(fields=(f,)), {f: log[f]}, what + " " + f)
            if E:
                same_fetch(eng.vmap_fetch_observations(first=5, count=E - 9), {f: a[5:E - 4] for f, a in log.items()}, what + " range")
                pinned = {"entry": eng.host_alloc((E,), np.uint32), "tag": eng.host_alloc((E,), np.int32)}  # exactly enough
                same_fetch({f: np.array(a) for f, a in eng.vmap_fetch_observations(out=pinned).items()}, log, what + " pinned")
                for a in pinned.values():
                    eng.host_free(a)
                out = {f: torch.full((E + 7,), -1, dtype=torch.int32, device="cuda") for f in log}
                got = eng.vmap_fetch_observations(first=3, count=E - 3, out=out)
                same_fetch({f: t.cpu().numpy().view(log[f].dtype) for f, t in got.items()}, {f: a[3:] for f, a in log.items()},
                           what + " device")
                assert all(bool((t[E - 3:] == -1).all()) for t in out.values())
                out = {"entry": np.full(E - 1, 77, np.uint32), "tag": np.full(E, 77, np.int32)}  # one short: nothing written
                with pytest.raises(pkg.SdmError) as e:
                    eng.vmap_fetch_observations(count=E, out=out)
                assert e.value.code == EINVAL and all((a == 77).all() for a in out.values())
            # the lists
            full = {"cam_offsets": offs, "cam_tags": tags}
            same_fetch(eng.vmap_fetch_cameras(), full, what + " lists")
            same_fetch(eng.vmap_fetch_cameras(first=5, count=M - 9), pick(offs, tags, range(5, M - 4)), what + " lists range")
            same_fetch(eng.vmap_fetch_cameras(first=M, count=0), pick(offs, tags, []), what + " lists empty range")
            same_fetch(eng.vmap_fetch_cameras(ids=ids), pick(offs, tags, ids), what + " lists ids (repeated)")
            want = pick(offs, tags, ids)
            # cam_tags == NULL: the offsets only; exact capacities, pageable and pinned
            got = eng.vmap_fetch_cameras(out={"cam_offsets": np.full(M + 1, -1, np.int64)})
            assert got["cam_total"] == total and got["cam_offsets"].tobytes() == offs.tobytes()
            got = eng.vmap_fetch_cameras(out={"cam_tags": np.full(max(total, 1), -1, np.int32)[:total]})
            assert got["cam_total"] == total and got["cam_tags"].tobytes() == tags.tobytes()
            pinned = {"cam_offsets": eng.host_alloc((len(ids) + 1,), np.int64), "cam_tags": eng.host_alloc((max(len(want["cam_tags"]), 1),), np.int32)}
            got = eng.vmap_fetch_cameras(ids=ids, out=pinned)
            same_fetch({f: np.array(got[f]) for f in want}, want, what + " lists pinned ids")
            for a in pinned.values():
                eng.host_free(a)
            # device destinations, range and device ids
            out = {"cam_offsets": torch.full((M + 1,), -1, dtype=torch.int64, device="cuda"),
                   "cam_tags": torch.full((total + 5,), -1, dtype=torch.int32, device="cuda")}
            got = eng.vmap_fetch_cameras(out=out)
            same_fetch({f: got[f].cpu().numpy() for f in full}, full, what + " lists device")
            assert bool((out["cam_tags"][total:] == -1).all())
            out = {"cam_offsets": torch.full((len(ids) + 1,), -1, dtype=torch.int64, device="cuda"),
                   "cam_tags": torch.full((len(want["cam_tags"]) + 1,), -1, dtype=torch.int32, device="cuda")}
            got = eng.vmap_fetch_cameras(ids=dev_ids, out=out)
            same_fetch({f: got[f].cpu().numpy() for f in want}, want, what + " lists device ids")
            got = eng.vmap_fetch_cameras(ids=dev_ids, out={"cam_offsets": out["cam_offsets"]})
            assert got["cam_offsets"].cpu().numpy().tobytes() == want["cam_offsets"].tobytes()
            if total:  # one short: EINVAL with the total, neither array written
                for mk in (lambda m, dt: np.full(m, 77, dt), lambda m, dt: torch.full((m,), 77, dtype=getattr(torch, np.dtype(dt).name), device="cuda")):
                    out = {"cam_offsets": mk(M + 1, np.int64), "cam_tags": mk(total - 1, np.int32)}
                    with pytest.raises(pkg.SdmError) as e:
                        eng.vmap_fetch_cameras(out=out)
                    assert e.value.code == EINVAL and e.value.cam_total == total
                    assert all(bool((a == 77).all()) for a in out.values())

        none = {"entry": np.zeros(0, np.uint32), "tag": np.zeros(0, np.int32)}
        forms(none, np.zeros(M + 1, np.int64), np.zeros(0, np.int32), "before any observe")  # every list is empty
        got = eng.vmap_observe(slots, rows, **kw)
        assert got["created"] > M
        log = {f: np.array(a) for f, a in eng.vmap_fetch_observations().items()}
        cams = eng.vmap_fetch_cameras()
        assert len(log["entry"]) == got["created"] == cams["cam_offsets"][-1] == len(cams["cam_tags"])
        o = np.lexsort((log["tag"], log["entry"]))  # the lists are the log, grouped by entry and sorted
        assert cams["cam_tags"].tobytes() == log["tag"][o].tobytes()
        np.testing.assert_array_equal(np.diff(cams["cam_offsets"]), np.bincount(log["entry"], minlength=M))
        forms(log, np.array(cams["cam_offsets"]), np.array(cams["cam_tags"]), "observed")
    finally:
        eng.vmap_close()


# 6. refusals: each leaves the log, both infos and full fetches as they were
def test_refusals(pkg, gpu_ok):
    torch = pytest.importorskip("torch")
    b = sys.modules[pkg.__name__ + ".binding"]
    g = gu.load("plane_64x48_n7")
    eng = pipeline(pkg, g, extra_slots=2)
    lib, ctx = eng.lib, eng.ctx
    spare, empty = g["n_kf"], g["n_kf"] + 1
    eng.upload_image(spare, g["im"][0], g["K"], g["Tcw"][0])
    eng.upload_depth(spare, *eng.download_depth(0))  # a depth map never inter-keyframe checked
    kw = dict(max_sigma=0.3)
    rows = np.ascontiguousarray(g["nbrs"][:, :3])

    def refused(code, fn, *a, **k):
        with pytest.raises(pkg.SdmError) as e:
            fn(*a, **k)
        assert e.value.code == code, (e.value, a, k)
        return e.value

    refused(ESTATE, eng.vmap_observe, [0], rows[[0]], **kw)  # no open map
    refused(ESTATE, eng.vmap_obs_info)
    refused(ESTATE, eng.vmap_fetch_observations, first=0, count=0)
    refused(ESTATE, eng.vmap_fetch_cameras, first=0, count=0)
    eng.vmap_open(0.02)
    eng.vmap_integrate([0, 1, 2], updated=False, **kw)
    eng.vmap_observe([0, 1, 2], rows[[0, 1, 2]], **kw)
    snap, osnap = snapshot(eng), obs_snapshot(eng)
    M, E = snap[0]["voxels"], osnap[0]["observations"]
    assert M > 100 and E > M

    def check(code, fn, *a, **k):
        err = refused(code, fn, *a, **k)
        unchanged(eng, snap, "%r %r" % (a, k))
        obs_unchanged(eng, osnap, "%r %r" % (a, k))
        return err

    # the slot and neighbour states and the argument errors of sdm_extract_points and sdm_extract_points_support
    check(ESTATE, eng.vmap_observe, [3, empty], rows[[3, 4]], **kw)             # a slot without a depth map
    check(ESTATE, eng.vmap_observe, [3, spare], rows[[3, 4]], source=1, **kw)   # never inter-keyframe checked
    check(ESTATE, eng.vmap_observe, [3], np.array([[4, empty]], np.int32), **kw)  # a neighbour without a depth map
    check(EINVAL, eng.vmap_observe, [3, 4, 3], rows[[3, 4, 3]], **kw)           # a repeated slot
    check(EINVAL, eng.vmap_observe, [3, 99], rows[[3, 4]], **kw)                # a slot out of range
    check(EINVAL, eng.vmap_observe, [3], np.array([[4, 99]], np.int32), **kw)   # a neighbour out of range
    check(EINVAL, eng.vmap_observe, [3], np.array([[4, -1]], np.int32), **kw)
    check(EINVAL, eng.vmap_observe, [3], rows[[3]], source=2, **kw)
    check(EINVAL, eng.vmap_observe, [3], np.zeros((1, g["n"] + 1), np.int32), **kw)  # n_nbr > max_neighbours
    # tags outside [0, 2^31)
    check(EINVAL, eng.vmap_observe, [3, 4], rows[[3, 4]], [7, -1], **kw)
    check(EINVAL, eng.vmap_observe, [3, 4], rows[[3, 4]], [-(1 << 31), 7], **kw)
    err = check(EINVAL, eng.vmap_observe, [3, 4], rows[[3, 4]], None, np.array([[1, 2, 3], [4, -1, 6]], np.int32), **kw)
    assert err.plain_total == 0
    sl = (ctypes.c_int * 2)(3, 4)
    nb = (ctypes.c_int * 6)(*[int(v) for v in rows[[3, 4]].reshape(-1)])

    def raw(n, slots, tags, n_nbr, nbrs, nbr_tags, ob):
        return lib.sdm_vmap_observe(ctx, n, slots, tags, n_nbr, nbrs, nbr_tags, 1, 0.3, 1e-6, ctypes.byref(ob) if ob is not None else None)

    for n, slots, n_nbr, nbrs, nbr_tags in ((2, sl, 3, nb, "null ob"), (-1, sl, 3, nb, None), (2, None, 3, nb, None), (2, sl, -1, nb, None),
                                            (2, sl, 0, nb, None), (2, sl, 3, None, None), (2, sl, 0, None, nb)):
        ob = None if nbr_tags == "null ob" else b.VmapObserveDelta()
        if ob is not None:
            ob.plain_total = ob.unmapped = ob.candidates = ob.first_created = ob.created = 9
        assert raw(n, slots, None, n_nbr, nbrs, None if nbr_tags == "null ob" else nbr_tags, ob) == EINVAL, (n, n_nbr)
        if ob is not None:
            assert [getattr(ob, f) for f in b.VMAP_OBSERVE_OUTS] == [0] * 5
    unchanged(eng, snap, "raw observes")
    obs_unchanged(eng, osnap, "raw observes")
    # the fetches: exactly sdm_vmap_fetch's errors
    check(EINVAL, eng.vmap_fetch_observations, first=0, count=-1)
    check(EINVAL, eng.vmap_fetch_observations, first=1, count=E)                 # a range beyond E
    check(EINVAL, eng.vmap_fetch_observations, first=E + 1, count=0)
    check(EINVAL, eng.vmap_fetch_observations, first=-1, count=1)
    check(EINVAL, eng.vmap_fetch_observations, first=0, count=10, out={"tag": np.zeros(9, np.int32)})  # count > capacity
    check(EINVAL, eng.vmap_fetch_observations, fields=())                        # no destination
    check(EINVAL, eng.vmap_fetch_cameras, first=0, count=-1)
    check(EINVAL, eng.vmap_fetch_cameras, first=1, count=M)                      # a range beyond M
    check(EINVAL, eng.vmap_fetch_cameras, first=M + 1, count=0)
    check(EINVAL, eng.vmap_fetch_cameras, first=-1, count=1)
    check(EINVAL, eng.vmap_fetch_cameras, first=0, count=10, out={"cam_offsets": np.zeros(10, np.int64)})  # count > capacity
    check(EINVAL, eng.vmap_fetch_cameras, ids=np.array([0, M, 1], np.uint32))    # an id beyond M, host ids
    check(EINVAL, eng.vmap_fetch_cameras, ids=np.array([0, 1], np.uint32), first=1)
    check(EINVAL, eng.vmap_fetch_cameras, out={})                                # no destination
    dev_ids = torch.tensor([0, 1, M, 2], dtype=torch.int32, device="cuda")
    offs = torch.full((5,), -1, dtype=torch.int64, device="cuda")
    check(EINVAL, eng.vmap_fetch_cameras, ids=dev_ids, out={"cam_offsets": offs})  # the flag; nothing written
    assert bool((offs == -1).all())
    buf = torch.full((8192,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    for where in ("entry", "tag"):
        v = b.VmapObservations()
        v.capacity, v.on_device = 1024, 1
        setattr(v, where, buf.data_ptr() + 2)
        assert lib.sdm_vmap_fetch_observations(ctx, 0, 16, ctypes.byref(v)) == EINVAL, where
    for where in ("cam_offsets", "cam_tags", "ids"):
        v = b.VmapCameras()
        v.capacity, v.cam_capacity, v.on_device = 64, 1024, 1
        ids_ptr = None
        if where == "ids":
            v.cam_offsets, ids_ptr = buf.data_ptr() + 16384, buf.data_ptr() + 2
        else:
            setattr(v, where, buf.data_ptr() + (4 if where == "cam_offsets" else 2))
        assert lib.sdm_vmap_fetch_cameras(ctx, ids_ptr, 0, 16, ctypes.byref(v)) == EINVAL, where
    v = b.VmapCameras()
    v.capacity, v.cam_capacity, v.cam_tags = 64, -1, buf.data_ptr()
    assert lib.sdm_vmap_fetch_cameras(ctx, None, 0, 16, ctypes.byref(v)) == EINVAL  # a negative cam_capacity
    assert lib.sdm_vmap_fetch_cameras(ctx, None, 0, 16, None) == EINVAL
    assert lib.sdm_vmap_fetch_observations(ctx, 0, 16, None) == EINVAL
    assert lib.sdm_vmap_get_obs_info(ctx, None) == EINVAL
    assert bool((buf == 0x5A5A5A5A).all())
    unchanged(eng, snap, "raw fetches")
    obs_unchanged(eng, osnap, "raw fetches")
    # the log still works, and as the restatement says
    ref = Mirror(0.02)
    ref.integrate(eng, [0, 1, 2], **kw)
    ref.observe(eng, [0, 1, 2], rows[[0, 1, 2]], **kw)
    same_obs(eng, ref, "the mirror of the state so far")
    step(eng, ref, [3, 4], rows[[3, 4]], [TOP, 0], what="after the refusals", **kw)
    eng.vmap_close()
    eng.close()


# 7. determinism on two engines, no side effects, and a map that was observed between integrates against one that was not
def test_determinism_and_no_side_effects(pkg, gpu_ok):
    g = gu.load("plane_96x80_n20")
    refs = list(range(g["n_kf"]))
    nbrs = g["nbrs"][refs]
    short = np.ascontiguousarray(nbrs[:, :3])
    kw = dict(max_sigma=0.3)
    engs = [pipeline(pkg, g), pipeline(pkg, g)]
    eng, other = engs
    for e in engs:
        e.enable_stats(True)
    before = _state(eng, refs)
    stats0 = eng.get_stats(reset=False)

    def views():
        return (eng.extract_points(refs, fields=ALL, **kw),
                eng.extract_points_voxel_freespace(refs, short, 0.02, fields=ALL, **kw))

    def same_views(a, b, what):
        for x, y in zip(a, b):
            assert set(x) == set(y)
            for f in x:
                assert np.asarray(x[f]).tobytes() == np.asarray(y[f]).tobytes(), (what, f)

    v0 = views()
    stats1 = eng.get_stats(reset=False)
    blocks = (refs[:8], refs[8:9], refs[9:])

    def run(e, observe):
        deltas, obs, carved = [], [], []
        for blk in blocks:
            tags = [1000 + s for s in blk]
            deltas.append(e.vmap_integrate(blk, tags, **kw))
            if observe:
                obs.append(e.vmap_observe(blk, nbrs[blk], tags, nbrs[blk] + 1000, **kw))
                if e is eng:
                    same_views(v0, views(), "between the map calls")
            carved.append(e.vmap_carve(blk, nbrs[blk], **kw))
        return deltas, obs, carved, e.vmap_fetch(), e.vmap_info(), e.vmap_fetch_evidence(), obs_snapshot(e)

    eng.vmap_open(0.02)
    other.vmap_open(0.02)
    d0, o0, c0, f0, i0, e0, s0 = run(eng, True)
    d1, _, c1, f1, i1, e1, z1 = run(other, False)   # never observed: the same deltas, records and evidence, an empty log
    assert i0 == i1 and i0["voxels"] > 100 and c0 == c1
    for a, b2 in zip(d0, d1):
        assert {f: a[f] for f in a if f != "updated_ids"} == {f: b2[f] for f in b2 if f != "updated_ids"}
        assert a["updated_ids"].tobytes() == b2["updated_ids"].tobytes()
    same_fetch(f0, f1, "observed between integrates / never observed")
    same_fetch(e0, e1, "evidence, observed / never observed")
    assert z1[0]["observations"] == 0 and z1[2]["cam_offsets"][-1] == 0
    other.vmap_clear()
    _, o1, _, _, _, _, s1 = run(other, True)        # the second engine, the same interleaving: the same bits
    assert o0 == o1 and sum(o["created"] for o in o0) == s0[0]["observations"] > i0["voxels"]
    assert {f: s0[0][f] for f in ("observations", "calls")} == {f: s1[0][f] for f in ("observations", "calls")}
    same_fetch(s0[1], s1[1], "two engines, the log")
    same_fetch(s0[2], s1[2], "two engines, the lists")
    assert int(s0[1]["tag"].min()) >= 1000
    # no side effects: planes, views; the stats move only as sdm_extract_points_support moves table_stagings
    same_views(v0, views(), "after the map calls")
    for x, y in zip(before, _state(eng, refs)):
        np.testing.assert_array_equal(x, y)
    a0 = eng.get_stats(reset=False)
    b0 = other.get_stats(reset=False)
    blk, rows = [5, 2, 11], np.array([[2, 2, 11], [5, 11, 5], [4, 4, 4]], np.int32)  # lists no call has staged
    eng.vmap_observe(blk, rows, **kw)
    other.extract_points_support(blk, rows, fields=(), **kw)
    a1, b1 = eng.get_stats(reset=False), other.get_stats(reset=False)
    assert a1["table_stagings"] - a0["table_stagings"] == b1["table_stagings"] - b0["table_stagings"]
    assert {f: v for f, v in a1.items() if f != "table_stagings"} == {f: v for f, v in stats1.items() if f != "table_stagings"}
    assert {f: v for f, v in stats1.items() if f != "table_stagings"} == {f: v for f, v in stats0.items() if f != "table_stagings"}
    eng.vmap_observe(blk, None, **kw)  # no table: no support pass, nothing staged
    assert eng.get_stats(reset=False) == a1
    eng.vmap_fetch_cameras()
    eng.vmap_fetch_observations()
    assert eng.get_stats(reset=False) == a1
    eng.vmap_close()  # the second engine's map is freed by sdm_destroy
    for e in engs:
        e.close()
