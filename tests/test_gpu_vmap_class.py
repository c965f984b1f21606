"""GPU: classification on the persistent voxel map (sdm_vmap_classify, sdm_vmap_get_class_info, sdm_vmap_fetch_published /
Engine.vmap_classify, .vmap_class_info, .vmap_fetch_published) against tests/vmap_class_np.py fed the engine's own
extract_points_support(fields=ALL), the poses, and the map, log and counters of tests/vmap_np.py, vmap_obs_np.py and
vmap_carve_np.py -- after every call the delta, both id lists, the info and a full fetch of the flags.  Everything is an
integer or a comparison under key(): every comparison is for equality."""
import ctypes
import sys

import numpy as np
import pytest

import carve_np
import golden_util as gu
import vmap_carve_np as vc
import vmap_class_np as vcl
import vmap_np
import vmap_obs_np as vo
from test_gpu_extract import ALL, EINVAL, ESTATE, _state, pipeline
from test_gpu_vmap import _crafted_engine, same_fetch, snapshot, unchanged

pytestmark = pytest.mark.gpu

EXT_TILE = 2048
TOP64 = (1 << 64) - 1
RULE = dict(min_multiplicity=2, min_cameras=2, min_ends=2, ratio_num=1, ratio_den=2, max_sigma=0.2, min_neighbours=2)
NOTHING = dict(min_multiplicity=0xFFFFFFFF, min_ends=TOP64)  # a rule nothing passes
COUNTS = ("examined", "accepted", "retracted", "published_total")


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


def centres_of(poses):
    return {int(s): carve_np.camera_centre(T) for s, T in poses.items()}


class Mirror:
    """tests/vmap_np.py's map, tests/vmap_obs_np.py's log, the two counters of tests/vmap_carve_np.py and the flags of
    tests/vmap_class_np.py"""

    def __init__(self, voxel):
        self.voxel = voxel
        self.vm, self.ol, self.cl = vmap_np.VoxelMap(voxel), vo.ObservationLog(), vcl.Classifier()
        self.clear()

    def clear(self):
        self.vm.clear()
        self.ol.clear()
        self.cl.clear()
        self.ev = {f: np.zeros(0, np.uint64) for f in ("crossings", "ends")}

    def block(self, eng, slots, nbrs, centres, tags=None, observe=True, carve=True, **kw):
        """integrate, observe and carve one block from one extraction of the engine's"""
        if nbrs is None:
            plain, sup = eng.extract_points(slots, fields=ALL, **kw), None
        else:
            plain = eng.extract_points_support(slots, nbrs, fields=ALL, **kw)
            sup = plain["support"]
        self.vm.integrate(plain, vmap_np.point_tags(plain["offsets"], slots, tags))
        for f in self.ev:  # entries created later start at 0
            self.ev[f] = np.concatenate([self.ev[f], np.zeros(self.vm.M - len(self.ev[f]), np.uint64)])
        row = np.repeat(np.arange(len(slots)), np.diff(plain["offsets"]))
        if observe:
            own = slots if tags is None else tags
            self.ol.observe((self.vm.keys, self.vm.ids), self.voxel, plain["xyz"], row, sup, own, nbrs)
        if carve:
            exp = vc.carve((self.vm.keys, self.vm.ids), plain["xyz"], row, sup, slots, nbrs, centres, self.voxel, 1, 4096)
            for f in self.ev:
                self.ev[f] = self.ev[f] + exp[f]

    def classify(self, rule, commit=True):
        ncam = np.diff(self.ol.cameras(self.vm.M)[0]) if self.ol.E else None  # (no observation: every length reads 0)
        return self.cl.classify(self.vm, self.ev["crossings"], self.ev["ends"], ncam, vcl.rule_of(**rule), commit)


def feed(eng, ref, slots, nbrs, centres, tags=None, observe=True, carve=True, **kw):
    """one block into the engine's map and the mirror"""
    ref.block(eng, slots, nbrs, centres, tags, observe, carve, **kw)
    eng.vmap_integrate(slots, tags, updated=False, **kw)
    if observe:
        eng.vmap_observe(slots, nbrs, tags, **kw)
    if carve:
        eng.vmap_carve(slots, nbrs, 1, 4096, **kw)
    assert eng.vmap_info()["voxels"] == ref.vm.M


def same_flags(eng, ref, what=""):
    got = eng.vmap_fetch_published()
    exp = ref.cl.flags(ref.vm.M)
    assert got.dtype == np.uint8 and got.shape == exp.shape, (what, got.shape, exp.shape)
    np.testing.assert_array_equal(got, exp, err_msg=what + " published")
    assert eng.vmap_class_info() == ref.cl.info(), (what, eng.vmap_class_info(), ref.cl.info())
    return got


def step(eng, ref, rule, commit=True, what=""):
    """one classify against the restatement: the counts, both id lists, the info and a full fetch of the flags"""
    exp = ref.classify(rule, commit)
    got = eng.vmap_classify(rule, commit)
    print(what, {f: got[f] for f in COUNTS}, "LOCAL", exp["local"])
    assert {f: got[f] for f in COUNTS} == {f: exp[f] for f in COUNTS}, (what, got, exp)
    for f in ("accepted_ids", "retracted_ids"):
        assert got[f].dtype == np.uint32 and got[f].shape == exp[f].shape, (what, f)
        np.testing.assert_array_equal(got[f], exp[f], err_msg="%s %s" % (what, f))
    same_flags(eng, ref, what)
    return got, exp


def class_snapshot(eng):
    return eng.vmap_class_info(), np.array(eng.vmap_fetch_published())


def class_unchanged(eng, snap, what=""):
    assert eng.vmap_class_info() == snap[0], what
    assert eng.vmap_fetch_published().tobytes() == snap[1].tobytes(), what


def full_state(eng):
    """everything a classify must leave alone (C4) and everything a refusal must: the map, the log, the lists, the
    counters, the flags"""
    return (snapshot(eng), eng.vmap_obs_info(), {f: np.array(a) for f, a in eng.vmap_fetch_observations().items()},
            {f: np.array(a) for f, a in eng.vmap_fetch_cameras().items()},
            {f: np.array(a) for f, a in eng.vmap_fetch_evidence().items()}, class_snapshot(eng))


def state_unchanged(eng, st, what="", flags=True):
    unchanged(eng, st[0], what)
    assert eng.vmap_obs_info() == st[1], what
    same_fetch(eng.vmap_fetch_observations(), st[2], what)
    same_fetch(eng.vmap_fetch_cameras(), st[3], what)
    same_fetch(eng.vmap_fetch_evidence(), st[4], what)
    if flags:
        class_unchanged(eng, st[5], what)


# 1. the golden fixtures: integrate, observe, carve, classify per keyframe
@pytest.mark.parametrize("src", (1, 0))
@pytest.mark.parametrize("name", ["plane_64x48_n7", "plane_96x80_n20"])
def test_golden_fixtures(engines, name, src):
    g, eng = engines(name)
    refs = list(range(g["n_kf"]))
    centres = centres_of({k: g["Tcw"][k] for k in refs})
    rows = np.ascontiguousarray(g["nbrs"][:, :3])
    kw = dict(source=src, max_sigma=0.3)
    eng.vmap_open(0.02)
    try:
        ref = Mirror(0.02)
        same_flags(eng, ref, "empty map")
        acc = ret = rejected = 0
        for k in refs:
            what = "%s src %d keyframe %d" % (name, src, k)
            feed(eng, ref, [k], rows[[k]], centres, **kw)
            same_flags(eng, ref, what + " fed")  # the flags survive growth; new entries read 0
            st = full_state(eng)
            got, exp = step(eng, ref, RULE, True, what)
            state_unchanged(eng, st, what, flags=False)  # C4
            acc, ret = acc + got["accepted"], ret + got["retracted"]
            rejected += exp["local"] - got["published_total"]
            again, _ = step(eng, ref, RULE, True, what + " again")  # C1
            assert again["accepted"] == again["retracted"] == 0
        print("%s src %d: accepted %d retracted %d published %d, the neighbour test rejected %d" %
              (name, src, acc, ret, got["published_total"], rejected))
        assert acc > 0 and rejected > 0 and acc - ret == got["published_total"]
        if src == 1:  # (the checked maps are what tests/test_vmap_class_cpu.py pins: some call retracts)
            assert ret > 0
        assert eng.vmap_class_info()["calls"] == 2 * len(refs)
    finally:
        eng.vmap_close()


# 2. rule changes on a fixed map (C2, C3), a rule nothing passes, and commit = 0
def test_rule_changes_on_a_fixed_map(engines):
    g, eng = engines("plane_96x80_n20")
    refs = list(range(g["n_kf"]))
    centres = centres_of({k: g["Tcw"][k] for k in refs})
    rows = np.ascontiguousarray(g["nbrs"][:, :3])
    kw = dict(max_sigma=0.3)
    eng.vmap_open(0.02)
    try:
        ref = Mirror(0.02)
        for blk in (refs[:8], refs[8:]):
            feed(eng, ref, blk, rows[blk], centres, **kw)
        a, _ = step(eng, ref, RULE, True, "rule A")
        pa = ref.cl.flags(ref.vm.M).astype(bool)
        assert a["accepted"] == int(pa.sum()) > 100 and a["retracted"] == 0
        b, _ = step(eng, ref, dict(RULE, min_multiplicity=3), True, "rule B")
        pb = ref.cl.flags(ref.vm.M).astype(bool)
        assert b["retracted"] > 0 and b["accepted"] == 0  # (B is stricter)
        np.testing.assert_array_equal(b["retracted_ids"], np.flatnonzero(pa & ~pb))
        c, _ = step(eng, ref, dict(RULE, min_multiplicity=1, min_neighbours=0, ratio_num=3), True, "rule C, laxer")
        pc = ref.cl.flags(ref.vm.M).astype(bool)
        np.testing.assert_array_equal(c["accepted_ids"], np.flatnonzero(pc & ~pb))
        np.testing.assert_array_equal(c["retracted_ids"], np.flatnonzero(pb & ~pc))
        assert c["accepted"] > 0
        d, _ = step(eng, ref, RULE, True, "rule A again")  # both lists at once
        assert d["accepted"] + d["retracted"] > 0
        np.testing.assert_array_equal(eng.vmap_fetch_published(), pa.astype(np.uint8))  # C3
        snap = class_snapshot(eng)
        for rep in range(2):  # commit = 0: the lists, and no state changes
            dry, _ = step(eng, ref, dict(RULE, min_multiplicity=3), False, "dry %d" % rep)
            np.testing.assert_array_equal(dry["retracted_ids"], b["retracted_ids"])
            assert dry["published_total"] == a["published_total"]
            class_unchanged(eng, snap, "dry")
        none, _ = step(eng, ref, NOTHING, True, "nothing passes")
        assert none["retracted"] == a["published_total"] and none["published_total"] == 0
        np.testing.assert_array_equal(none["retracted_ids"], np.flatnonzero(pa))
        assert not eng.vmap_fetch_published().any()
    finally:
        eng.vmap_close()


# 3. before any observe or carve: ncam and the counters read 0
def test_before_any_observe_or_carve(engines):
    g, eng = engines("plane_64x48_n7")
    kw = dict(max_sigma=0.3)
    eng.vmap_open(0.02)
    try:
        ref = Mirror(0.02)
        feed(eng, ref, [0, 1, 2], None, None, observe=False, carve=False, **kw)
        assert eng.vmap_obs_info()["table_slots"] == 0 and not eng.vmap_fetch_published().any()
        got, _ = step(eng, ref, dict(min_cameras=1), True, "min_cameras 1")
        assert got["accepted"] == 0 and got["examined"] == ref.vm.M > 100
        got, _ = step(eng, ref, dict(min_ends=1), True, "min_ends 1")
        assert got["accepted"] == 0
        got, exp = step(eng, ref, dict(min_multiplicity=2, min_cameras=0, min_ends=0, min_neighbours=4), True, "by multiplicity")
        assert 0 < got["accepted"] < exp["local"] < ref.vm.M
        mult = eng.vmap_fetch(fields=("multiplicity",))["multiplicity"]
        assert (mult[got["accepted_ids"]] >= 2).all()
    finally:
        eng.vmap_close()


# 4. crafted maps: cell faces, both signs, NaN and signed-zero sigmas; thresholds of every kind
@pytest.mark.parametrize("W,H", [(32, 24), (64, 48)])
def test_crafted_maps(pkg, gpu_ok, W, H):
    rng = np.random.default_rng(W)
    eng, rho, sigma = _crafted_engine(pkg, W, H, rng)
    for s in range(3):
        eng.upload_depth(s, rho, rng.permutation(sigma.reshape(-1)).reshape(H, W))
    eng.pointset([0, 1, 2], source=0)
    pose = np.eye(4, dtype=np.float32)[:3].copy()
    pose[:, 3] = (8.0, 6.0, 1.0)
    centres = centres_of({s: pose for s in range(3)})
    kw = dict(source=0, max_sigma=0.01, min_rho=-1.0)
    table = np.array([[1, 1, 0, 2], [1, 0, 0, 2], [2, 2, 2, 2]], np.int32)
    for voxel in (1.0, 0.25):
        eng.vmap_open(voxel)
        ref = Mirror(voxel)
        feed(eng, ref, [0, 1, 2], table, centres, **kw)
        sig = eng.vmap_fetch(fields=("rho_sigma",))["rho_sigma"][:, 1]
        xyz = eng.vmap_fetch(fields=("xyz",))["xyz"]
        assert (xyz < 0).any() and (xyz > 0).any()
        what = "crafted %dx%d voxel %r" % (W, H, voxel)
        seen = set()
        for ms in (0.003, 0.0, -0.0, float("nan"), float("inf"), float("-inf"), 0.002):
            for nb in (0, 1, 3, 26):
                got, exp = step(eng, ref, dict(max_sigma=ms, ratio_num=0xFFFFFFFF, min_neighbours=nb), True, "%s max_sigma %r nb %d" % (what, ms, nb))
                seen.add((exp["local"], got["published_total"]))
        assert len(seen) >= 6  # the thresholds and the neighbour counts tell entries apart
        got, exp = step(eng, ref, dict(min_cameras=2, min_ends=2, ratio_num=1, ratio_den=3, max_sigma=float("nan"), min_neighbours=2),
                        True, what + " evidence")
        assert 0 < exp["local"] < ref.vm.M and got["published_total"] < exp["local"]  # the neighbour test rejects some
        if voxel == 1.0:  # (at 0.25 few entries or none have two LOCAL-passing neighbours)
            assert got["published_total"] > 0
        step(eng, ref, dict(ratio_num=0, max_sigma=float("nan")), True, what + " ratio 0: crossings must be 0")
        eng.vmap_close()
    eng.close()


def _sheet_engine(pkg, W=64, H=48):
    """one slot, identity pose, K = (1, 1, 2, 2): a pixel with rho 1 sits alone in its cell at voxel 1; rho 0 sits at the origin"""
    eng = pkg.Engine(W, H, 1)
    eng.upload_image(0, np.zeros((H, W), np.uint8), np.array([1, 1, 2, 2], np.float32), np.eye(4, dtype=np.float32)[:3])
    return eng


# 5. entry counts around one tile, an empty map and a one-entry map
def test_entry_counts_around_one_tile(pkg, gpu_ok):
    W, H = 64, 48
    eng = _sheet_engine(pkg, W, H)
    rng = np.random.default_rng(2)
    centres = centres_of({0: np.eye(4, dtype=np.float32)[:3]})
    kw = dict(source=0, max_sigma=0.01, min_rho=-1.0)
    inner = np.zeros((H, W), bool)
    inner[2:-2, 2:-2] = True
    order = np.flatnonzero(inner.reshape(-1))
    sigma = rng.choice(np.array([0.001, 0.002, 0.004, 0.006], np.float32), (H, W))
    seen = set()
    for K in (0, EXT_TILE - 2, EXT_TILE - 1, EXT_TILE, EXT_TILE + 1):
        rho = np.zeros(H * W, np.float32)
        rho[order[:K]] = 1
        eng.upload_depth(0, rho.reshape(H, W), sigma)
        eng.pointset([0], source=0)
        eng.vmap_open(1.0)
        ref = Mirror(1.0)
        if K == 0:  # the empty map first
            got, _ = step(eng, ref, RULE, True, "empty map")
            assert [got[f] for f in COUNTS] == [0] * 4
            assert eng.vmap_class_info() == {"published": 0, "calls": 1}
        feed(eng, ref, [0], None, centres, **kw)
        M = ref.vm.M
        seen.add(M)
        what = "M %d" % M
        for rule in (dict(max_sigma=0.004, min_neighbours=3), dict(max_sigma=0.002, min_neighbours=1), dict(max_sigma=0.001),
                     dict(max_sigma=0.006, min_neighbours=8), NOTHING, dict(min_cameras=1, min_ends=1, ratio_num=0xFFFFFFFF)):
            got, _ = step(eng, ref, rule, True, "%s %r" % (what, rule))
        assert got["published_total"] == M  # every entry was seen by its camera and ends one ray
        if K == 0:
            assert M == 1
        eng.vmap_close()
    eng.close()
    print("entry counts", sorted(seen))
    assert {1, EXT_TILE - 1, EXT_TILE, EXT_TILE + 1} <= seen


# 6. M beyond 2048 x 2048: the second scan level of both counts
def test_1080p_second_scan_level(pkg, gpu_ok):
    W, H = 1920, 1080
    eng = pkg.Engine(W, H, 3)
    rng = np.random.default_rng(11)
    im = np.zeros((H, W), np.uint8)
    eye = np.eye(4, dtype=np.float32)[:3]
    for s in range(3):
        eng.upload_image(s, im, np.array([1000, 1000, W / 2, H / 2], np.float32), eye)
        rho = np.where(rng.random((H, W)) < 0.9, rng.uniform(0.5, 2.0, (H, W)), 0).astype(np.float32)
        eng.upload_depth(s, rho, rng.uniform(0.001, 0.009, (H, W)).astype(np.float32))
    eng.pointset([0, 1, 2], source=0)
    kw = dict(source=0, min_rho=-1.0)
    eng.vmap_open(0.002)
    ref = Mirror(0.002)
    feed(eng, ref, [0, 1, 2], None, None, observe=False, carve=False, **kw)
    M = ref.vm.M
    assert M > EXT_TILE * EXT_TILE
    a, exp = step(eng, ref, dict(max_sigma=0.0012, min_neighbours=1), True, "1080p first")
    assert 0 < a["accepted"] < exp["local"]
    c, _ = step(eng, ref, dict(max_sigma=0.0012, min_neighbours=0), True, "1080p no probe")
    assert c["accepted"] > 100000 and c["accepted_ids"][-1] > EXT_TILE * EXT_TILE
    d, _ = step(eng, ref, NOTHING, True, "1080p retract all")
    assert d["retracted"] == c["published_total"] > 100000 and d["retracted_ids"][-1] > EXT_TILE * EXT_TILE
    eng.vmap_close()
    eng.close()


# 7. destinations and capacities: host, pinned and device id arrays, a NULL list, one short, the exact size; the fetch forms
def test_destinations_and_capacity(pkg, engines):
    torch = pytest.importorskip("torch")
    g, eng = engines("plane_96x80_n20")
    refs = list(range(g["n_kf"]))
    centres = centres_of({k: g["Tcw"][k] for k in refs})
    rows = np.ascontiguousarray(g["nbrs"][:, :3])
    kw = dict(max_sigma=0.3)
    eng.vmap_open(0.02)
    try:
        ref = Mirror(0.02)
        feed(eng, ref, refs, rows, centres, **kw)
        M = ref.vm.M
        step(eng, ref, dict(RULE, min_multiplicity=3), True, "seed")  # some published, so that the next rule lists both ways
        rule = dict(RULE, min_multiplicity=1, min_neighbours=0, ratio_num=3, max_sigma=0.1)
        exp = ref.classify(rule, commit=False)
        na, nr = exp["accepted"], exp["retracted"]
        assert na > 5 and nr > 5
        snap = class_snapshot(eng)

        def check(got, lists):
            assert {f: got[f] for f in COUNTS} == {f: exp[f] for f in COUNTS}
            for f in lists:
                a = got[f].cpu().numpy().view(np.uint32) if hasattr(got[f], "cpu") else np.asarray(got[f])
                np.testing.assert_array_equal(a, exp[f], err_msg=f)
            class_unchanged(eng, snap, "dry")

        both = ("accepted_ids", "retracted_ids")
        check(eng.vmap_classify(rule, commit=False), both)
        check(eng.vmap_classify(rule, commit=False, ids=False), ())  # counts only: two NULL lists
        for f, n in (("accepted_ids", na), ("retracted_ids", nr)):  # one NULL list
            out = np.full(n + 3, 0xABCD, np.uint32)
            got = eng.vmap_classify(rule, commit=False, ids={f: out})
            check(got, (f,))
            assert set(got) == set(COUNTS) | {f} and (out[n:] == 0xABCD).all()
        exact = {"accepted_ids": np.empty(na, np.uint32), "retracted_ids": np.empty(nr, np.uint32)}
        check(eng.vmap_classify(rule, commit=False, ids=exact), both)
        pinned = {"accepted_ids": eng.host_alloc((na,), np.uint32), "retracted_ids": eng.host_alloc((nr,), np.uint32)}
        check(eng.vmap_classify(rule, commit=False, ids=pinned), both)
        for a in pinned.values():
            eng.host_free(a)
        dev = {"accepted_ids": torch.full((na,), -1, dtype=torch.int32, device="cuda"),
               "retracted_ids": torch.full((nr + 7,), -1, dtype=torch.int32, device="cuda")}
        check(eng.vmap_classify(rule, commit=False, ids=dev), both)
        assert bool((dev["retracted_ids"][nr:] == -1).all())
        with pytest.raises(ValueError):
            eng.vmap_classify(rule, commit=False, ids={"accepted_ids": dev["accepted_ids"], "retracted_ids": exact["retracted_ids"]})
        # one short: EINVAL with the counts filled, neither array written, no flag changed -- committing or not
        for commit in (True, False):
            for short in both:
                for kind in ("host", "device"):
                    if kind == "host":
                        out = {f: np.full((na if f == "accepted_ids" else nr) - (f == short), 77, np.uint32) for f in both}
                    else:
                        out = {f: torch.full(((na if f == "accepted_ids" else nr) - (f == short),), 77, dtype=torch.int32, device="cuda")
                               for f in both}
                    with pytest.raises(pkg.SdmError) as e:
                        eng.vmap_classify(rule, commit=commit, ids=out)
                    assert e.value.code == EINVAL and (e.value.accepted, e.value.retracted) == (na, nr)
                    assert all(bool((a == 77).all()) for a in out.values())
                    class_unchanged(eng, snap, "short %s %s" % (short, kind))
        # then the exact size, committing, into device arrays
        dev = {"accepted_ids": torch.full((na,), -1, dtype=torch.int32, device="cuda"),
               "retracted_ids": torch.full((nr,), -1, dtype=torch.int32, device="cuda")}
        got = eng.vmap_classify(rule, commit=True, ids=dev)
        exp = ref.classify(rule, commit=True)
        for f in both:
            np.testing.assert_array_equal(got[f].cpu().numpy().view(np.uint32), exp[f])
        full = same_flags(eng, ref, "committed into device arrays")
        assert full.any() and not full.all()
        # the fetch forms
        ids = np.concatenate([np.random.default_rng(1).integers(0, M, 500), [M - 1, 0, 0]]).astype(np.uint32)
        dev_ids = torch.from_numpy(ids.view(np.int32)).cuda()
        np.testing.assert_array_equal(eng.vmap_fetch_published(first=5, count=M - 9), full[5:M - 4])
        assert len(eng.vmap_fetch_published(first=M, count=0)) == 0
        np.testing.assert_array_equal(eng.vmap_fetch_published(ids=ids), full[ids])
        pin = eng.host_alloc((M,), np.uint8)
        pin[:] = 9
        np.testing.assert_array_equal(np.array(eng.vmap_fetch_published(out=pin)), full)
        eng.host_free(pin)
        out = torch.full((M + 5,), 9, dtype=torch.uint8, device="cuda")
        np.testing.assert_array_equal(eng.vmap_fetch_published(out=out).cpu().numpy(), full)
        assert bool((out[M:] == 9).all())
        out = torch.full((len(ids),), 9, dtype=torch.uint8, device="cuda")
        np.testing.assert_array_equal(eng.vmap_fetch_published(ids=dev_ids, out=out).cpu().numpy(), full[ids])
        out = np.full(M - 1, 9, np.uint8)
        with pytest.raises(pkg.SdmError) as e:
            eng.vmap_fetch_published(count=M, out=out)
        assert e.value.code == EINVAL and (out == 9).all()
    finally:
        eng.vmap_close()


# 8. refusals: each leaves the map, the log, the counters and the flags as they were
def test_refusals(pkg, engines):
    torch = pytest.importorskip("torch")
    b = sys.modules[pkg.__name__ + ".binding"]
    g, eng = engines("plane_64x48_n7")
    lib, ctx = eng.lib, eng.ctx
    refs = list(range(g["n_kf"]))
    centres = centres_of({k: g["Tcw"][k] for k in refs})
    rows = np.ascontiguousarray(g["nbrs"][:, :3])
    kw = dict(max_sigma=0.3)

    def refused(code, fn, *a, **k):
        with pytest.raises(pkg.SdmError) as e:
            fn(*a, **k)
        assert e.value.code == code, (e.value, a, k)
        return e.value

    refused(ESTATE, eng.vmap_classify, RULE)  # no open map
    refused(ESTATE, eng.vmap_classify, RULE, True, False)
    refused(ESTATE, eng.vmap_class_info)
    refused(ESTATE, eng.vmap_fetch_published, first=0, count=0)
    eng.vmap_open(0.02)
    try:
        ref = Mirror(0.02)
        feed(eng, ref, refs[:4], rows[:4], centres, **kw)
        first, _ = step(eng, ref, RULE, True, "before the refusals")
        assert first["accepted"] > 50
        feed(eng, ref, refs[4:], rows[4:], centres, **kw)  # so that the next classify has work to do
        st = full_state(eng)
        M = ref.vm.M

        def check(code, fn, *a, **k):
            err = refused(code, fn, *a, **k)
            state_unchanged(eng, st, "%r %r" % (a, k))
            return err

        for commit in (True, False):
            check(EINVAL, eng.vmap_classify, dict(RULE, ratio_den=0), commit)
            check(EINVAL, eng.vmap_classify, dict(RULE, min_neighbours=-1), commit)
            check(EINVAL, eng.vmap_classify, dict(RULE, min_neighbours=27), commit)
            err = check(EINVAL, eng.vmap_classify, RULE, commit, {"accepted_ids": np.zeros(1, np.uint32)})  # the capacity case
            assert err.accepted > 1
        with pytest.raises(ValueError):
            eng.vmap_classify(dict(RULE, min_sigma=1))

        def raw(rule, delta, commit=1, c=ctx):
            return lib.sdm_vmap_classify(c, ctypes.byref(rule) if rule is not None else None, commit,
                                         ctypes.byref(delta) if delta is not None else None)

        def rule_of(**kw2):
            r = b.VmapRule()
            for f, v in dict(b.VMAP_RULE_DEFAULTS, **RULE, **kw2).items():
                setattr(r, f, v)
            return r

        def delta_of(**kw2):
            d = b.VmapClassDelta()
            d.examined = d.accepted = d.retracted = d.published_total = 9
            for f, v in kw2.items():
                setattr(d, f, v)
            return d

        host = np.full(M, 0x5A5A, np.uint32)
        buf = torch.full((M + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        assert raw(None, delta_of()) == EINVAL and raw(rule_of(), None) == EINVAL and raw(rule_of(), delta_of(), c=None) == EINVAL
        cases = [delta_of(accepted_ids=host.ctypes.data, accepted_capacity=-1),
                 delta_of(retracted_ids=host.ctypes.data, retracted_capacity=-5),
                 delta_of(accepted_ids=buf.data_ptr() + 2, accepted_capacity=M, on_device=1),
                 delta_of(retracted_ids=buf.data_ptr() + 1, retracted_capacity=M, on_device=1)]
        for d in cases:
            assert raw(rule_of(), d) == EINVAL
            assert [getattr(d, f) for f in COUNTS] == [0] * 4
        d = delta_of(accepted_ids=None, accepted_capacity=-1, retracted_ids=None, retracted_capacity=-1)
        assert raw(rule_of(), d, commit=0) == 0 and d.examined == M  # a NULL list's capacity is ignored
        assert (host == 0x5A5A).all() and bool((buf == 0x5A5A5A5A).all())
        state_unchanged(eng, st, "raw classifies")
        # fetch: exactly sdm_vmap_fetch's errors
        check(EINVAL, eng.vmap_fetch_published, first=0, count=-1)
        check(EINVAL, eng.vmap_fetch_published, first=1, count=M)                   # a range beyond M
        check(EINVAL, eng.vmap_fetch_published, first=M + 1, count=0)
        check(EINVAL, eng.vmap_fetch_published, first=-1, count=1)
        check(EINVAL, eng.vmap_fetch_published, first=0, count=10, out=np.zeros(9, np.uint8))  # count > capacity
        check(EINVAL, eng.vmap_fetch_published, ids=np.array([0, M, 1], np.uint32))  # an id beyond M, host ids
        check(EINVAL, eng.vmap_fetch_published, ids=np.array([0, 1], np.uint32), first=1)
        dev_ids = torch.tensor([0, 1, M, 2], dtype=torch.int32, device="cuda")
        check(EINVAL, eng.vmap_fetch_published, ids=dev_ids, out=torch.zeros(4, dtype=torch.uint8, device="cuda"))  # the flag
        p = b.VmapPublished()
        p.published, p.capacity, p.on_device = buf.data_ptr(), 16, 1
        assert lib.sdm_vmap_fetch_published(ctx, buf.data_ptr() + 4096 + 2, 0, 16, ctypes.byref(p)) == EINVAL  # misaligned ids
        assert lib.sdm_vmap_fetch_published(ctx, None, 0, 16, None) == EINVAL
        p = b.VmapPublished()
        p.capacity = 16
        assert lib.sdm_vmap_fetch_published(ctx, None, 0, 16, ctypes.byref(p)) == EINVAL  # no destination
        assert lib.sdm_vmap_get_class_info(ctx, None) == EINVAL and lib.sdm_vmap_get_class_info(None, None) == EINVAL
        assert bool((buf == 0x5A5A5A5A).all())
        state_unchanged(eng, st, "raw fetches")
        got, _ = step(eng, ref, RULE, True, "after the refusals")  # the map still works, and as the restatement says
        assert got["accepted"] > 0
    finally:
        eng.vmap_close()


# 9. survival: a rehash and record growth, clear, close and reopen
def test_survival(engines):
    g, eng = engines("plane_64x48_n7")
    refs = list(range(g["n_kf"]))
    centres = centres_of({k: g["Tcw"][k] for k in refs})
    rows = np.ascontiguousarray(g["nbrs"][:, :3])
    kw = dict(max_sigma=0.3)
    lax = dict(min_multiplicity=1, min_cameras=1, min_ends=1, ratio_num=4, max_sigma=0.25, min_neighbours=0)
    eng.vmap_open(0.005, 16)  # a small reserve: the first block fits the minimum table, the rest outgrows table and records
    try:
        ref = Mirror(0.005)
        feed(eng, ref, [0], rows[[0]], centres, **kw)
        info0 = eng.vmap_info()
        a, _ = step(eng, ref, lax, True, "small")
        old = np.array(eng.vmap_fetch_published())
        assert a["accepted"] > 50 and old.any() and not old.all()
        feed(eng, ref, refs[1:], rows[1:], centres, **kw)
        info = eng.vmap_info()
        assert info["rehashes"] > info0["rehashes"] and info["voxels"] > 2 * info0["voxels"]  # table and records grew
        got = same_flags(eng, ref, "grown")
        assert got[:len(old)].tobytes() == old.tobytes() and not got[len(old):].any()
        b, _ = step(eng, ref, lax, True, "after growth")
        assert b["accepted"] > a["accepted"]
        first = np.array(eng.vmap_fetch_published())
        eng.vmap_clear()
        ref.clear()
        assert eng.vmap_class_info() == {"published": 0, "calls": 0} and len(eng.vmap_fetch_published()) == 0
        feed(eng, ref, refs, rows, centres, **kw)
        assert not same_flags(eng, ref, "after clear").any()  # zeros, though the array kept its capacity
        step(eng, ref, lax, True, "after clear")
        eng.vmap_close()
        eng.vmap_open(0.005, 16)
        ref = Mirror(0.005)
        assert eng.vmap_class_info() == {"published": 0, "calls": 0}
        feed(eng, ref, [0], rows[[0]], centres, **kw)
        step(eng, ref, lax, True, "reopened small")
        feed(eng, ref, refs[1:], rows[1:], centres, **kw)
        step(eng, ref, lax, True, "reopened grown")
        assert eng.vmap_fetch_published().tobytes() == first.tobytes()  # the same sequence, the same bits
    finally:
        eng.vmap_close()


# 10. determinism on two engines (C5) and no side effects (C4)
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

    def views():
        return (eng.extract_points(refs, fields=ALL, **kw),
                eng.extract_points_voxel(refs, 0.02, fields=ALL, **kw),
                eng.extract_points_voxel_freespace(refs, short, 0.02, fields=ALL, **kw))

    def same_views(a, b, what):
        for x, y in zip(a, b):
            assert set(x) == set(y)
            for f in x:
                assert np.asarray(x[f]).tobytes() == np.asarray(y[f]).tobytes(), (what, f)

    v0 = views()
    stats0 = eng.get_stats(reset=False)
    blocks = (refs[:8], refs[8:9], refs[9:])
    rules = (RULE, dict(RULE, min_multiplicity=3), dict(RULE, min_neighbours=0, ratio_num=5))

    def run(e, classify):
        out = []
        for blk, rule in zip(blocks, rules):
            d = e.vmap_integrate(blk, [1000 + s for s in blk], **kw)
            o = e.vmap_observe(blk, nbrs[blk], [1000 + s for s in blk], 1000 + nbrs[blk], **kw)
            c = e.vmap_carve(blk, nbrs[blk], **kw)
            out.append(({f: v for f, v in d.items() if f != "updated_ids"}, d["updated_ids"].tobytes(), o, c))
            if classify:
                stats = e.get_stats(reset=False)
                r = e.vmap_classify(rule)
                assert e.get_stats(reset=False) == stats  # no counter of the engine moves
                out.append(({f: r[f] for f in COUNTS}, r["accepted_ids"].tobytes(), r["retracted_ids"].tobytes()))
                if e is eng:
                    same_views(v0, views(), "between the map calls")
        state = (e.vmap_fetch(), e.vmap_info(), e.vmap_fetch_evidence(), e.vmap_fetch_observations(), e.vmap_fetch_cameras(),
                 e.vmap_obs_info())
        return out, state, np.array(e.vmap_fetch_published()), e.vmap_class_info()

    eng.vmap_open(0.02)
    other.vmap_open(0.02)
    o0, s0, p0, i0 = run(eng, True)
    o1, s1, p1, i1 = run(other, False)  # never classified: the same map, log and counters; every flag 0
    assert [x for x in o0 if len(x) == 4] == o1
    for a, b2 in zip(s0, s1):
        if isinstance(a, dict) and not isinstance(next(iter(a.values())), (int, float)):
            same_fetch(a, b2, "classified between the calls / never classified")
        else:
            assert a == b2
    assert not p1.any() and i1 == {"published": 0, "calls": 0} and p0.any() and i0["calls"] == 3
    other.vmap_clear()
    o2, _, p2, i2 = run(other, True)  # the second engine, the same sequence: the same bits
    assert o0 == o2 and p0.tobytes() == p2.tobytes() and i0 == i2
    assert sum(x[0]["retracted"] for x in o0 if len(x) == 3) > 0
    same_views(v0, views(), "after the map calls")
    for x, y in zip(before, _state(eng, refs)):
        np.testing.assert_array_equal(x, y)
    s = eng.get_stats(reset=False)
    assert {f: v for f, v in s.items() if f != "table_stagings"} == {f: v for f, v in stats0.items() if f != "table_stagings"}
    eng.vmap_close()  # the second engine's map, flags included, is freed by sdm_destroy
    for e in engs:
        e.close()
