"""GPU: free-space evidence on the persistent voxel map (sdm_vmap_carve, sdm_vmap_fetch_evidence / Engine.vmap_carve,
Engine.vmap_fetch_evidence) against tests/vmap_carve_np.py fed the engine's own extract_points_support(fields=ALL), the
poses and the entries of tests/vmap_np.py -- the six totals of every call and a full fetch of both counters after every
call.  Everything is an integer: every comparison is for equality."""
import ctypes
import sys

import numpy as np
import pytest

import carve_np
import golden_util as gu
import vmap_carve_np as vc
import vmap_np
import voxel_np
from test_gpu_extract import ALL, EINVAL, ESTATE, _state, pipeline
from test_gpu_vmap import _crafted_engine, same_fetch, same_info, snapshot, unchanged

pytestmark = pytest.mark.gpu

FIELDS = ("crossings", "ends")


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
    """tests/vmap_np.py's map plus the two counters as the header defines them"""

    def __init__(self, voxel):
        self.voxel = voxel
        self.vm = vmap_np.VoxelMap(voxel)
        self.clear()

    def clear(self):
        self.vm.clear()
        self.ev = {f: np.zeros(0, np.uint64) for f in FIELDS}

    def integrate(self, eng, slots, tags=None, **kw):
        plain = eng.extract_points(slots, fields=ALL, **kw)
        d = self.vm.integrate(plain, vmap_np.point_tags(plain["offsets"], slots, tags))
        for f in FIELDS:  # entries created later start at 0
            self.ev[f] = np.concatenate([self.ev[f], np.zeros(self.vm.M - len(self.ev[f]), np.uint64)])
        return d

    def carve(self, eng, slots, nbrs, centres, end_margin, max_steps, **kw):
        if nbrs is None:
            plain, sup = eng.extract_points(slots, fields=ALL, **kw), None
        else:
            plain = eng.extract_points_support(slots, nbrs, fields=ALL, **kw)
            sup = plain["support"]
        row = np.repeat(np.arange(len(slots)), np.diff(plain["offsets"]))
        exp = vc.carve((self.vm.keys, self.vm.ids), plain["xyz"], row, sup, slots, nbrs, centres, self.voxel, end_margin, max_steps)
        for f in FIELDS:
            self.ev[f] = self.ev[f] + exp[f]
        return exp


def same_evidence(eng, ref, what=""):
    got = eng.vmap_fetch_evidence()
    assert set(got) == set(FIELDS)
    for f in FIELDS:
        assert got[f].dtype == np.uint64 and got[f].shape == ref.ev[f].shape, (what, f, got[f].shape, ref.ev[f].shape)
        np.testing.assert_array_equal(got[f], ref.ev[f], err_msg="%s %s" % (what, f))
    return got


def step(eng, ref, slots, nbrs, centres, end_margin=1, max_steps=4096, what="", **kw):
    """one carve against the restatement: the six totals and a full fetch of both counters"""
    exp = ref.carve(eng, slots, nbrs, centres, end_margin, max_steps, **kw)
    got = eng.vmap_carve(slots, nbrs, end_margin, max_steps, **kw)
    assert got == {f: exp[f] for f in vc.TOTALS}, (what, got, {f: exp[f] for f in vc.TOTALS})
    same_evidence(eng, ref, what)
    return got, exp


# 1. the golden fixtures, one integrate-then-carve per keyframe with the fixture's full neighbour rows
@pytest.mark.parametrize("src", (1, 0))
@pytest.mark.parametrize("name,voxel", [("plane_64x48_n7", 0.02), ("plane_64x48_n7", 0.005), ("plane_96x80_n20", 0.02)])
def test_golden_fixtures(engines, name, voxel, src):
    g, eng = engines(name)
    refs = list(range(g["n_kf"]))
    centres = centres_of({k: g["Tcw"][k] for k in refs})
    kw = dict(source=src, max_sigma=0.3)
    eng.vmap_open(voxel)
    try:
        ref = Mirror(voxel)
        same_evidence(eng, ref, "empty map")
        tot = dict.fromkeys(vc.TOTALS, 0)
        for k in refs:
            what = "%s src %d voxel %r keyframe %d" % (name, src, voxel, k)
            exp = ref.integrate(eng, [k], **kw)
            got = eng.vmap_integrate([k], **kw)
            assert (got["created"], got["updated"]) == (exp["created"], exp["updated"]), what
            same_evidence(eng, ref, what + " integrated")  # the counters survive growth; new entries read 0
            got, _ = step(eng, ref, [k], g["nbrs"][[k]], centres, 1, 4096, what, **kw)
            for f in tot:
                tot[f] += got[f]
        print("%s src %d voxel %r: %s, %d entries crossed" % (name, src, voxel, tot, int((ref.ev["crossings"] > 0).sum())))
        assert tot["rays_skipped"] == 0 and tot["cells_hit"] > 0 and tot["rays_total"] > tot["plain_total"] > 1000
        assert tot["ends_hit"] == tot["rays_total"]  # carved after its integrate: every end cell has an entry
        assert int(ref.ev["crossings"].sum()) == tot["cells_hit"] and int(ref.ev["ends"].sum()) == tot["ends_hit"]
        # the map is read, not changed
        same_info(eng, ref.vm, name)
        same_fetch(eng.vmap_fetch(), ref.vm.fetch(), name)
        if voxel == 0.005:
            assert eng.vmap_info()["rehashes"] >= 2
    finally:
        eng.vmap_close()


# 2. crafted maps: the centre inside an entry's voxel, ties, axis-parallel rays, non-finite points, a NaN pose, max_steps at
# the longest N and one below, end_margin 0 and huge, no table against tables of repeated and self neighbours
@pytest.mark.parametrize("W,H", [(32, 24), (64, 48)])
def test_crafted_maps(pkg, gpu_ok, W, H):
    rng = np.random.default_rng(W)
    eng, rho, sigma = _crafted_engine(pkg, W, H, rng)
    rho[2, 2] = 4   # Z = 0.25 straight ahead: axis-parallel, and in the camera's own cell at voxel 1
    rho[3, 3] = 1   # d = (1, 1, 1): an exact three-axis tie
    rho[2, 6] = 1   # d = (4, 0, 1)
    for s in range(3):
        eng.upload_depth(s, rho, sigma)  # (the third slot's K: non-finite and out of range)
    eng.pointset([0, 1, 2], source=0)
    pose = np.eye(4, dtype=np.float32)[:3].copy()
    pose[:, 3] = (8.0, 6.0, 1.0)
    centres = centres_of({s: pose for s in range(3)})
    assert centres[0].tolist() == [-8.0, -6.0, -1.0]
    kw = dict(source=0, max_sigma=0.01, min_rho=-1.0)
    slots = [0, 1, 2]
    table = np.array([[1, 1, 0, 2], [1, 0, 0, 2], [2, 2, 2, 2]], np.int32)  # repeated and self neighbours
    selfs = np.array([[0, 0], [1, 1], [2, 2]], np.int32)                    # nothing but the own camera
    for voxel in (1.0, 0.25):
        eng.vmap_open(voxel)
        ref = Mirror(voxel)
        for s in slots:
            ref.integrate(eng, [s], **kw)
            eng.vmap_integrate([s], **kw)
        snap = snapshot(eng)
        what = "crafted %dx%d voxel %r" % (W, H, voxel)
        got0, exp0 = step(eng, ref, slots, None, centres, 0, 4096, what + " own camera", **kw)
        assert got0["rays_total"] == got0["plain_total"] == 3 * W * H
        bad = got0["rays_skipped"]
        far = ~voxel_np.cells(eng.extract_points([2], fields=("xyz",), **kw)["xyz"], voxel)[1]
        assert bad == int(far.sum()) > 0  # the third slot's non-finite and out-of-range points, and nothing else
        steps = exp0["steps"]
        if voxel == 1.0:
            assert (steps == 0).any()  # a point in its camera's cell
            home = carve_np.pack(np.floor(centres[0][None] * (np.float32(1) / np.float32(voxel))).astype(np.int64))
            at = np.searchsorted(ref.vm.keys, home)[0]
            assert ref.vm.keys[at] == home[0]  # the camera centre lies in a voxel that holds an entry: cell s = 0 counts
            assert ref.ev["crossings"][ref.vm.ids[at]] >= int((steps > 0).sum()) > 500
        # the same through tables that add no camera
        before = {f: a.copy() for f, a in ref.ev.items()}
        got1, _ = step(eng, ref, slots, selfs, centres, 0, 4096, what + " self neighbours", **kw)
        assert got1 == got0
        for f in FIELDS:
            np.testing.assert_array_equal(ref.ev[f], 2 * before[f])
        got2, exp2 = step(eng, ref, slots, table, centres, 0, 4096, what + " table", **kw)
        assert got2["rays_total"] > got0["rays_total"]  # neighbours confirm points
        assert len(set(zip(exp2["ray_g"].tolist(), exp2["ray_slot"].tolist()))) == got2["rays_total"]
        if voxel != 1.0:  # (walks four times as long: the variants below stay at voxel 1)
            unchanged(eng, snap, what)
            eng.vmap_close()
            continue
        # max_steps at the longest N and one below
        longest = int(steps.max())
        assert longest > 8
        got, _ = step(eng, ref, slots, table, centres, 1, longest, what + " longest", **kw)
        assert got["rays_skipped"] == got2["rays_skipped"]
        got, _ = step(eng, ref, slots, table, centres, 1, longest - 1, what + " longest - 1", **kw)
        assert got["rays_skipped"] > got2["rays_skipped"]
        got, _ = step(eng, ref, slots, table, centres, 1 << 30, 65536, what + " huge margin", **kw)
        assert got["cells_visited"] == 0 and got["cells_hit"] == 0 and got["ends_hit"] > 0
        step(eng, ref, [1, 0], table[[1, 0]], centres, 2, 4096, what + " two slots", **kw)
        # a NaN pose: every ray of that camera is skipped, the planes stay
        nan_pose = pose.copy()
        nan_pose[0, 3] = np.nan
        eng.set_pose(0, nan_pose)
        moved = dict(centres)
        moved[0] = carve_np.camera_centre(nan_pose)
        got, _ = step(eng, ref, [0], None, moved, 0, 4096, what + " NaN pose", **kw)
        assert got["rays_skipped"] == got["rays_total"] == W * H and got["ends_hit"] == 0
        eng.set_pose(0, pose)
        step(eng, ref, [0], None, centres, 0, 4096, what + " pose back", **kw)
        unchanged(eng, snap, what)
        eng.vmap_close()
    eng.close()


# 3. growth: the counters survive rehashes and record growth, new entries read 0; clear; the same sequence again
def test_growth_and_clear(engines):
    g, eng = engines("plane_64x48_n7")
    refs = list(range(g["n_kf"]))
    centres = centres_of({k: g["Tcw"][k] for k in refs})
    rows = np.ascontiguousarray(g["nbrs"][:, :3])
    kw = dict(max_sigma=0.3)
    eng.vmap_open(0.005)
    try:
        ref = Mirror(0.005)

        def sequence():
            ref.integrate(eng, [0, 1], **kw)
            eng.vmap_integrate([0, 1], **kw)
            step(eng, ref, [0, 1], rows[[0, 1]], centres, 0, 4096, what="first carve", **kw)
            M0, slots0 = eng.vmap_info()["voxels"], eng.vmap_info()["table_slots"]
            old = {f: a.copy() for f, a in eng.vmap_fetch_evidence().items()}
            assert old["crossings"].sum() > 0 and old["ends"].sum() > 0
            for k in refs[2:]:
                ref.integrate(eng, [k], **kw)
                eng.vmap_integrate([k], **kw)
            info = eng.vmap_info()
            got = same_evidence(eng, ref, "grown")
            for f in FIELDS:
                assert got[f][:M0].tobytes() == old[f].tobytes() and not got[f][M0:].any()
            step(eng, ref, [3, 4], rows[[3, 4]], centres, what="carve after growth", **kw)
            return M0, slots0, info, {f: a.copy() for f, a in eng.vmap_fetch_evidence().items()}

        M0, slots0, info, first = sequence()
        assert info["rehashes"] >= 2 and info["table_slots"] > slots0 and info["voxels"] > 2 * M0  # table and records grew
        eng.vmap_clear()
        ref.clear()
        assert all(len(a) == 0 for a in eng.vmap_fetch_evidence().values())
        ref.integrate(eng, refs, **kw)
        eng.vmap_integrate(refs, **kw)
        same_evidence(eng, ref, "after clear")  # all zeros
        assert not eng.vmap_fetch_evidence()["ends"].any()
        eng.vmap_clear()
        ref.clear()
        _, _, info2, second = sequence()
        assert info2["rehashes"] == 0  # (the table kept is large enough)
        for f in FIELDS:
            assert first[f].tobytes() == second[f].tobytes(), f
    finally:
        eng.vmap_close()


# 4. additivity and order on a fixed map
def test_additivity_and_order(engines):
    g, eng = engines("plane_96x80_n20")
    refs = list(range(g["n_kf"]))
    centres = centres_of({k: g["Tcw"][k] for k in refs})
    rows = np.ascontiguousarray(g["nbrs"][:, :3])
    kw = dict(max_sigma=0.3)
    A, B = refs[:9], refs[9:]
    eng.vmap_open(0.02)
    try:
        seen = {}
        for how, calls in (("A then B", (A, B)), ("B then A", (B, A)), ("A u B", (B[3:] + A + B[:3],))):
            eng.vmap_clear()
            eng.vmap_integrate(refs, updated=False, **kw)
            tot = dict.fromkeys(vc.TOTALS, 0)
            for c in calls:
                got = eng.vmap_carve(c, rows[c], **kw)
                for f in tot:
                    tot[f] += got[f]
            seen[how] = (tot, eng.vmap_fetch_evidence())
        ref = Mirror(0.02)
        ref.integrate(eng, refs, **kw)
        exp = ref.carve(eng, refs, rows, centres, 1, 4096, **kw)
        assert exp["cells_hit"] > 1000
        for how, (tot, ev) in seen.items():
            assert tot == {f: exp[f] for f in vc.TOTALS}, how
            for f in FIELDS:
                np.testing.assert_array_equal(ev[f], ref.ev[f], err_msg="%s %s" % (how, f))
    finally:
        eng.vmap_close()


# 5. destinations: pageable, pinned, device; range and ids; single fields; exact and short capacities; before any carve
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

        def forms(full, what):
            same_fetch(eng.vmap_fetch_evidence(), full, what)
            same_fetch(eng.vmap_fetch_evidence(first=5, count=M - 9), {f: a[5:M - 4] for f, a in full.items()}, what + " range")
            same_fetch(eng.vmap_fetch_evidence(first=M, count=0), {f: a[M:] for f, a in full.items()}, what + " empty range")
            same_fetch(eng.vmap_fetch_evidence(ids=ids), {f: a[ids] for f, a in full.items()}, what + " ids")
            for f in FIELDS:  # single fields
                same_fetch(eng.vmap_fetch_evidence(fields=(f,)), {f: full[f]}, what + " " + f)
                same_fetch(eng.vmap_fetch_evidence(ids=ids, fields=(f,)), {f: full[f][ids]}, what + " ids " + f)
            pinned = {f: eng.host_alloc((M,), np.uint64) for f in FIELDS}  # exactly enough
            for a in pinned.values():
                a[:] = 0xABCD
            same_fetch({f: np.array(a) for f, a in eng.vmap_fetch_evidence(out=pinned).items()}, full, what + " pinned")
            same_fetch({f: np.array(a) for f, a in eng.vmap_fetch_evidence(ids=ids[:M], out=pinned).items()},
                       {f: a[ids[:M]] for f, a in full.items()}, what + " pinned ids")
            for a in pinned.values():
                eng.host_free(a)

            def device_out(m, fields=FIELDS):
                return {f: torch.full((m,), -1, dtype=torch.int64, device="cuda") for f in fields}

            def to_host(res):
                return {f: t.cpu().numpy().view(np.uint64) for f, t in res.items()}

            same_fetch(to_host(eng.vmap_fetch_evidence(out=device_out(M))), full, what + " device")
            out = device_out(64)
            same_fetch(to_host(eng.vmap_fetch_evidence(first=3, count=50, out=out)), {f: a[3:53] for f, a in full.items()},
                       what + " device range")
            assert all(bool((t[50:] == -1).all()) for t in out.values())
            same_fetch(to_host(eng.vmap_fetch_evidence(ids=dev_ids, out=device_out(len(ids)))),
                       {f: a[ids] for f, a in full.items()}, what + " device ids")
            same_fetch(to_host(eng.vmap_fetch_evidence(ids=dev_ids, out=device_out(len(ids), ("ends",)))),
                       {"ends": full["ends"][ids]}, what + " device ids, one field")
            # one short: EINVAL, nothing written
            out = {"crossings": np.full(M - 1, 77, np.uint64), "ends": np.full(M, 77, np.uint64)}
            with pytest.raises(pkg.SdmError) as e:
                eng.vmap_fetch_evidence(count=M, out=out)
            assert e.value.code == EINVAL and all((a == 77).all() for a in out.values())
            out = device_out(M - 1)
            with pytest.raises(pkg.SdmError) as e:
                eng.vmap_fetch_evidence(count=M, out=out)
            assert e.value.code == EINVAL and all(bool((t == -1).all()) for t in out.values())

        zeros = {f: np.zeros(M, np.uint64) for f in FIELDS}
        forms(zeros, "before any carve")  # no counter exists yet: every form returns zeros
        got = eng.vmap_carve(slots, rows, **kw)
        assert got["cells_hit"] > 0 and got["ends_hit"] > 0
        full = {f: np.array(a) for f, a in eng.vmap_fetch_evidence().items()}
        assert int(full["crossings"].sum()) == got["cells_hit"] and int(full["ends"].sum()) == got["ends_hit"]
        forms(full, "carved")
    finally:
        eng.vmap_close()


# 6. refusals: each leaves the counters, the info and a full fetch as they were
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

    refused(ESTATE, eng.vmap_carve, [0], rows[[0]], **kw)  # no open map
    refused(ESTATE, eng.vmap_fetch_evidence, first=0, count=0)
    eng.vmap_open(0.02)
    eng.vmap_integrate([0, 1, 2], updated=False, **kw)
    eng.vmap_carve([0, 1, 2], rows[[0, 1, 2]], **kw)
    snap = snapshot(eng)
    ev = {f: np.array(a) for f, a in eng.vmap_fetch_evidence().items()}
    M = snap[0]["voxels"]
    assert M > 100 and ev["crossings"].any() and ev["ends"].any()

    def check(code, fn, *a, **k):
        err = refused(code, fn, *a, **k)
        unchanged(eng, snap, "%r %r" % (a, k))
        same_fetch(eng.vmap_fetch_evidence(), ev, "%r %r" % (a, k))
        return err

    # the slot and neighbour states and the argument errors of sdm_extract_points and sdm_extract_points_support
    check(ESTATE, eng.vmap_carve, [3, empty], rows[[3, 4]], **kw)             # a slot without a depth map
    check(ESTATE, eng.vmap_carve, [3, spare], rows[[3, 4]], source=1, **kw)   # never inter-keyframe checked
    check(ESTATE, eng.vmap_carve, [3], np.array([[4, empty]], np.int32), **kw)  # a neighbour without a depth map
    check(EINVAL, eng.vmap_carve, [3, 4, 3], rows[[3, 4, 3]], **kw)           # a repeated slot
    check(EINVAL, eng.vmap_carve, [3, 99], rows[[3, 4]], **kw)                # a slot out of range
    check(EINVAL, eng.vmap_carve, [3], np.array([[4, 99]], np.int32), **kw)   # a neighbour out of range
    check(EINVAL, eng.vmap_carve, [3], np.array([[4, -1]], np.int32), **kw)
    check(EINVAL, eng.vmap_carve, [3], rows[[3]], source=2, **kw)
    check(EINVAL, eng.vmap_carve, [3], np.zeros((1, g["n"] + 1), np.int32), **kw)  # n_nbr > max_neighbours
    # the new argument errors
    check(EINVAL, eng.vmap_carve, [3], rows[[3]], end_margin=-1, **kw)
    check(EINVAL, eng.vmap_carve, [3], rows[[3]], max_steps=0, **kw)
    check(EINVAL, eng.vmap_carve, [3], rows[[3]], max_steps=65537, **kw)
    err = check(EINVAL, eng.vmap_carve, [3], rows[[3]], max_steps=-5, **kw)
    assert err.plain_total == 0
    sl = (ctypes.c_int * 2)(3, 4)
    nb = (ctypes.c_int * 6)(*[int(v) for v in rows[[3, 4]].reshape(-1)])

    def raw(n, slots, n_nbr, nbrs, cv):
        return lib.sdm_vmap_carve(ctx, n, slots, n_nbr, nbrs, 1, 0.3, 1e-6, ctypes.byref(cv) if cv is not None else None)

    def args(margin=1, steps=4096):
        cv = b.VmapCarveArgs()
        cv.end_margin, cv.max_steps = margin, steps
        cv.plain_total = cv.rays_total = cv.rays_skipped = cv.cells_visited = cv.cells_hit = cv.ends_hit = 9
        return cv

    for n, slots, n_nbr, nbrs in ((2, sl, 3, nb), (-1, sl, 3, nb), (2, None, 3, nb), (2, sl, -1, nb), (2, sl, 0, nb), (2, sl, 3, None)):
        cv = args() if (n, slots, n_nbr, nbrs) != (2, sl, 3, nb) else None
        assert raw(n, slots, n_nbr, nbrs, cv) == EINVAL, (n, n_nbr)
        if cv is not None:
            assert [getattr(cv, f) for f in b.VMAP_CARVE_OUTS] == [0] * 6
    unchanged(eng, snap, "raw carves")
    same_fetch(eng.vmap_fetch_evidence(), ev, "raw carves")
    # fetch: exactly sdm_vmap_fetch's errors
    check(EINVAL, eng.vmap_fetch_evidence, first=0, count=-1)
    check(EINVAL, eng.vmap_fetch_evidence, first=1, count=M)                   # a range beyond M
    check(EINVAL, eng.vmap_fetch_evidence, first=M + 1, count=0)
    check(EINVAL, eng.vmap_fetch_evidence, first=-1, count=1)
    check(EINVAL, eng.vmap_fetch_evidence, first=0, count=10, out={"ends": np.zeros(9, np.uint64)})  # count > capacity
    check(EINVAL, eng.vmap_fetch_evidence, ids=np.array([0, M, 1], np.uint32))  # an id beyond M, host ids
    check(EINVAL, eng.vmap_fetch_evidence, ids=np.array([0, 1], np.uint32), first=1)
    check(EINVAL, eng.vmap_fetch_evidence, fields=())                          # no destination
    dev_ids = torch.tensor([0, 1, M, 2], dtype=torch.int32, device="cuda")
    check(EINVAL, eng.vmap_fetch_evidence, ids=dev_ids, out={"ends": torch.zeros(4, dtype=torch.int64, device="cuda")})  # the flag
    buf = torch.full((8192,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    for where in ("crossings", "ends", "ids"):
        e = b.VmapEvidence()
        e.capacity, e.on_device = 1024, 1
        ids_ptr = None
        if where == "ids":
            e.ends, ids_ptr = buf.data_ptr() + 16384, buf.data_ptr() + 2
        else:
            setattr(e, where, buf.data_ptr() + 4)
        assert lib.sdm_vmap_fetch_evidence(ctx, ids_ptr, 0, 16, ctypes.byref(e)) == EINVAL, where
    assert lib.sdm_vmap_fetch_evidence(ctx, None, 0, 16, None) == EINVAL
    e = b.VmapEvidence()
    e.capacity = 16
    assert lib.sdm_vmap_fetch_evidence(ctx, None, 0, 16, ctypes.byref(e)) == EINVAL  # no destination
    assert bool((buf == 0x5A5A5A5A).all())
    unchanged(eng, snap, "raw fetches")
    same_fetch(eng.vmap_fetch_evidence(), ev, "raw fetches")
    # the map still works, and as the restatement says; the limits of max_steps and end_margin are accepted
    centres = centres_of({k: g["Tcw"][k] for k in range(g["n_kf"])})
    ref = Mirror(0.02)
    ref.integrate(eng, [0, 1, 2], **kw)
    ref.carve(eng, [0, 1, 2], rows[[0, 1, 2]], centres, 1, 4096, **kw)
    same_evidence(eng, ref, "the mirror of the state so far")
    step(eng, ref, [3, 4], rows[[3, 4]], centres, 0, 65536, "after the refusals", **kw)
    step(eng, ref, [4], None, centres, 1, 1, "max_steps 1", **kw)
    eng.vmap_close()
    eng.close()


# 7. determinism on two engines, no side effects, and a map that was carved between integrates against one that was not
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

    def run(e, carve):
        deltas, totals = [], []
        for blk in blocks:
            deltas.append(e.vmap_integrate(blk, [1000 + s for s in blk], **kw))
            if carve:
                totals.append(e.vmap_carve(blk, nbrs[blk], **kw))
                if e is eng:
                    same_views(v0, views(), "between the map calls")
        return deltas, totals, e.vmap_fetch(), e.vmap_info(), e.vmap_fetch_evidence()

    eng.vmap_open(0.02)
    other.vmap_open(0.02)
    d0, t0, f0, i0, e0 = run(eng, True)
    d1, _, f1, i1, z1 = run(other, False)   # never carved: the same deltas and records, counters all zero
    assert i0 == i1 and i0["voxels"] > 100
    for a, b2 in zip(d0, d1):
        assert {f: a[f] for f in a if f != "updated_ids"} == {f: b2[f] for f in b2 if f != "updated_ids"}
        assert a["updated_ids"].tobytes() == b2["updated_ids"].tobytes()
    same_fetch(f0, f1, "carved between integrates / never carved")
    assert not z1["crossings"].any() and not z1["ends"].any()
    other.vmap_clear()
    _, t1, _, _, e1 = run(other, True)      # the second engine, the same sequence: the same bits
    assert t0 == t1 and sum(t["cells_hit"] for t in t0) > 1000
    same_fetch(e0, e1, "two engines")
    assert int(e0["crossings"].sum()) == sum(t["cells_hit"] for t in t0)
    # no side effects: planes, views; the stats move only as sdm_extract_points_support moves table_stagings
    same_views(v0, views(), "after the map calls")
    for x, y in zip(before, _state(eng, refs)):
        np.testing.assert_array_equal(x, y)
    a0 = eng.get_stats(reset=False)
    b0 = other.get_stats(reset=False)
    blk, rows = [5, 2, 11], np.array([[2, 2, 11], [5, 11, 5], [4, 4, 4]], np.int32)  # lists no call has staged
    eng.vmap_carve(blk, rows, **kw)
    other.extract_points_support(blk, rows, fields=(), **kw)
    a1, b1 = eng.get_stats(reset=False), other.get_stats(reset=False)
    assert a1["table_stagings"] - a0["table_stagings"] == b1["table_stagings"] - b0["table_stagings"]
    assert {f: v for f, v in a1.items() if f != "table_stagings"} == {f: v for f, v in stats1.items() if f != "table_stagings"}
    assert {f: v for f, v in stats1.items() if f != "table_stagings"} == {f: v for f, v in stats0.items() if f != "table_stagings"}
    eng.vmap_carve(blk, None, **kw)  # no table: no support pass, nothing staged
    assert eng.get_stats(reset=False) == a1
    eng.vmap_close()  # the second engine's map is freed by sdm_destroy
    for e in engs:
        e.close()
