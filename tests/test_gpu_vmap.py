"""GPU: the persistent voxel map (sdm_vmap_* / Engine.vmap_*) against tests/vmap_np.py fed the engine's own
extract_points(fields=ALL) for each call -- every delta, updated_ids included, and a full fetch of all fields after every
call compared for equality (floats as bits)."""
import ctypes
import sys

import numpy as np
import pytest

import golden_util as gu
import vmap_np
import voxel_np
from test_gpu_extract import ALL, EINVAL, ESTATE, _state, pipeline

pytestmark = pytest.mark.gpu

VOXELS = (0.005, 0.02, 1000.0, 1e-7)
INFO = ("voxels", "points", "dropped", "calls")
DELTA = ("plain_total", "dropped", "first_created", "created", "updated")


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


def same_fetch(got, exp, what="", skip=()):
    for f in exp:
        if f in skip:
            continue
        g, e = np.asarray(got[f]), np.asarray(exp[f])
        assert g.shape == e.shape and g.dtype == e.dtype, (what, f, g.shape, e.shape, g.dtype, e.dtype)
        assert g.tobytes() == e.tobytes(), (what, f)


def same_info(eng, ref, what=""):
    info, exp = eng.vmap_info(), ref.info()
    assert {f: info[f] for f in INFO} == exp, (what, info, exp)
    assert info["table_slots"] >= max(1024, 2 * info["voxels"]) and info["table_slots"] & (info["table_slots"] - 1) == 0
    return info


def step(eng, ref, slots, tags=None, what="", **kw):
    """one integrate against the restatement: the delta, the info and a full fetch of all fields"""
    plain = eng.extract_points(slots, fields=ALL, **kw)
    exp = ref.integrate(plain, vmap_np.point_tags(plain["offsets"], slots, tags))
    got = eng.vmap_integrate(slots, tags, **kw)
    assert {f: got[f] for f in DELTA} == {f: exp[f] for f in DELTA}, (what, got, exp)
    assert got["updated_ids"].dtype == np.uint32
    np.testing.assert_array_equal(got["updated_ids"], exp["updated_ids"], err_msg=what + " updated_ids")
    same_info(eng, ref, what)
    same_fetch(eng.vmap_fetch(), ref.fetch(), what)
    return got


def snapshot(eng):
    return eng.vmap_info(), {f: np.array(a) for f, a in eng.vmap_fetch().items()}


def unchanged(eng, snap, what=""):
    info, full = snap
    assert eng.vmap_info() == info, what
    same_fetch(eng.vmap_fetch(), full, what)


# 1. the golden fixtures: per keyframe, all at once, two halves
@pytest.mark.parametrize("name", gu.fixture_names())
def test_golden_fixtures(engines, name):
    g, eng = engines(name)
    n_kf = g["n_kf"]
    refs = list(range(n_kf))
    splits = {"each": [[k] for k in refs], "all": [refs], "halves": [refs[:n_kf // 2], refs[n_kf // 2:]]}
    for src in (1, 0):
        kw = dict(source=src, max_sigma=0.3)
        for voxel in VOXELS:
            final = {}
            for how, groups in splits.items():
                what = "%s src %d voxel %r %s" % (name, src, voxel, how)
                eng.vmap_open(voxel, 0)
                try:
                    ref = vmap_np.VoxelMap(voxel)
                    assert eng.vmap_info()["table_slots"] == 1024
                    for grp in groups:
                        d = step(eng, ref, grp, what=what, **kw)
                    info = eng.vmap_info()
                    final[how] = (info, eng.vmap_fetch())
                    assert info["points"] + info["dropped"] > 1000
                    if voxel == 1e-7:  # nearly every cell is out of range: the dropped path
                        assert info["dropped"] > 1000
                    if how == "each" and voxel == 0.005:
                        assert info["rehashes"] >= 2
                    if how == "each" and voxel == 0.02 and src == 1:
                        assert d["created"] > 0 and d["updated"] > 0
                    if how == "all":  # I2: the mergeable kept points of the per-call merge, matched by (tag, pixel)
                        vox = eng.extract_points_voxel(refs, voxel, fields=ALL, **kw)
                        _, ok = voxel_np.cells(vox["xyz"], voxel)
                        assert info["dropped"] == int((~ok).sum()) and info["voxels"] == int(ok.sum())
                        tag = vmap_np.point_tags(vox["offsets"], refs)
                        o1 = np.lexsort((final[how][1]["pixel"], final[how][1]["tag"]))
                        o2 = np.lexsort((vox["pixel"][ok], tag[ok]))
                        for f in ALL + ("multiplicity",):
                            assert np.asarray(final[how][1][f])[o1].tobytes() == np.asarray(vox[f])[ok][o2].tobytes(), (what, f)
                        np.testing.assert_array_equal(final[how][1]["tag"][o1], tag[ok][o2])
                finally:
                    eng.vmap_close()
            for how in ("all", "halves"):  # I1: byte-identical except epoch and calls
                a, b = final["each"], final[how]
                assert {f: a[0][f] for f in INFO[:3]} == {f: b[0][f] for f in INFO[:3]}
                same_fetch(a[1], b[1], "%s src %d voxel %r each / %s" % (name, src, voxel, how), skip=("epoch",))


def _crafted_engine(pkg, W, H, rng):
    """K = (1, 1, 2, 2), identity rotations: pixel (x, y) at rho = 1 / Z is the point O + (Z (x - 2), Z (y - 2), Z) -- on
    cell faces, on both sides of zero; a rho below 1e-6 and the 2-pixel border sit at (0, 0, 0).  The third slot's focal
    length of 2e-38 gives non-finite and out-of-range coordinates."""
    f = np.float32
    eng = pkg.Engine(W, H, 3)
    im = rng.integers(0, 256, (H, W)).astype(np.uint8)
    pose = np.eye(4, dtype=f)[:3].copy()
    pose[:, 3] = (8.0, 6.0, 1.0)  # the camera centre at (-8, -6, -1): the sheets straddle zero on every axis
    for s in range(3):
        eng.upload_image(s, im, np.array([1, 1, 2, 2] if s < 2 else [2e-38, 2e-38, 2, 2], f), pose)
    rho = rng.choice(np.array([0, 1e-39, 1, 1, 2, 4], f), (H, W))
    sigma = rng.choice(np.array([0.0, -0.0, np.nan, 0.004, 0.004, 0.002], f), (H, W))
    return eng, rho, sigma


# 2a. crafted maps: cross-call ties, sigma's total order, cell faces, both signs, dropped points
@pytest.mark.parametrize("W,H", [(32, 24), (64, 48)])
def test_crafted_maps(pkg, gpu_ok, W, H):
    rng = np.random.default_rng(W)
    eng, rho, sigma = _crafted_engine(pkg, W, H, rng)
    sig2 = rng.permutation(sigma.reshape(-1)).reshape(H, W)
    eng.upload_depth(0, rho, sigma)
    eng.upload_depth(1, rho, sig2)   # the same points under other sigmas: -0 against +0, NaN, ties across calls
    eng.upload_depth(2, rho, sigma)  # (through the third slot's K: non-finite and out of range)
    eng.pointset([0, 1, 2], source=0)
    kw = dict(source=0, max_sigma=0.01, min_rho=-1.0)
    for voxel in (1.0, 0.25):
        eng.vmap_open(voxel)
        ref = vmap_np.VoxelMap(voxel)
        d0 = step(eng, ref, [0], [10], "crafted first", **kw)
        assert d0["plain_total"] == W * H and d0["created"] > 10 and d0["dropped"] == 0
        xyz = eng.extract_points([0], fields=("xyz",), **kw)["xyz"]
        inv = np.float32(1) / np.float32(voxel)
        assert (xyz < 0).any() and (xyz > 0).any()
        if voxel == 0.25:
            assert (xyz * inv == np.floor(xyz * inv)).all()  # every point on cell faces
        d1 = step(eng, ref, [1], [11], "crafted other sigmas", **kw)
        assert d1["created"] == 0 and d1["updated"] > 0
        d2 = step(eng, ref, [2], [12], "crafted dropped", **kw)
        assert d2["dropped"] > 0
        with np.errstate(invalid="ignore"):
            assert (~np.isfinite(eng.extract_points([2], fields=("xyz",), **kw)["xyz"])).any()
        before = eng.vmap_fetch()
        d3 = step(eng, ref, [2, 0, 1], None, "crafted again", **kw)  # I3, in another order and with the slots as tags
        assert d3["created"] == 0 and d3["updated"] == 0 and d3["dropped"] == d2["dropped"]
        after = eng.vmap_fetch()
        same_fetch(after, before, "I3", skip=("multiplicity",))
        np.testing.assert_array_equal(after["multiplicity"], 2 * before["multiplicity"])
        d4 = step(eng, ref, [0], [13], "crafted tie", **kw)
        assert d4["created"] == 0 and d4["updated"] == 0  # the earlier call keeps every tie
        assert set(np.unique(eng.vmap_fetch(fields=("tag",))["tag"]).tolist()) <= {10, 11, 12}
        eng.vmap_close()
    eng.close()


# 2b. every pixel in one voxel: every lane of every wave on one table slot; I3; then one sigma lowered
def test_one_hot_voxel(pkg, gpu_ok):
    W, H = 64, 48
    rng = np.random.default_rng(3)
    eng, _, sigma = _crafted_engine(pkg, W, H, rng)
    zero = np.zeros((H, W), np.float32)
    sigma = np.where(np.isnan(sigma), np.float32(0.003), sigma)
    eng.upload_depth(0, zero, sigma)
    eng.pointset([0], source=0)
    kw = dict(source=0, max_sigma=0.01, min_rho=-1.0)
    eng.vmap_open(0.25)
    ref = vmap_np.VoxelMap(0.25)
    d = step(eng, ref, [0], [5], "hot first", **kw)
    assert (d["plain_total"], d["created"], d["updated"], d["dropped"]) == (W * H, 1, 0, 0)
    first = eng.vmap_fetch()
    assert int(first["multiplicity"][0]) == W * H
    d = step(eng, ref, [0], [6], "hot again", **kw)
    assert (d["created"], d["updated"]) == (0, 0) and int(eng.vmap_fetch()["multiplicity"][0]) == 2 * W * H
    lowered = sigma.copy()
    lowered[17, 33] = -1.0  # below every sigma of the map
    eng.upload_depth(0, zero, lowered)
    eng.pointset([0], source=0)
    d = step(eng, ref, [0], [7], "hot lowered", **kw)
    assert (d["created"], d["updated"]) == (0, 1) and list(d["updated_ids"]) == [0]
    got = eng.vmap_fetch()
    assert int(got["pixel"][0]) == (17 << 16) | 33 and int(got["tag"][0]) == 7 and int(got["epoch"][0]) == 3
    assert int(got["multiplicity"][0]) == 3 * W * H
    eng.vmap_close()
    eng.close()


# 3. a recycled slot with a new tag, tags = NULL, and the same slot after a pose change
def test_recycled_slots_and_poses(pkg, gpu_ok):
    g = gu.load("plane_64x48_n7")
    eng = pipeline(pkg, g)
    kw = dict(source=0, max_sigma=0.3)
    eng.vmap_open(0.02)
    ref = vmap_np.VoxelMap(0.02)
    step(eng, ref, [0, 1, 2], [100, 101, 102], "first block", **kw)
    # slot 0 is recycled for a newer keyframe
    eng.upload_image(0, g["im"][5], g["K"], g["Tcw"][5])
    rho, sigma = eng.download_depth(5)
    eng.upload_depth(0, rho, (sigma * np.float32(0.5)).astype(np.float32))
    eng.pointset([0], source=0)
    d = step(eng, ref, [0, 3], [107, 103], "recycled", **kw)
    assert d["updated"] > 0
    tags = eng.vmap_fetch(fields=("tag",))["tag"]
    assert (tags == 107).any() and (tags == 100).any()
    d = step(eng, ref, [4], None, "tags = NULL", **kw)
    assert d["created"] > 0 and (eng.vmap_fetch(fields=("tag",))["tag"][d["first_created"]:] == 4).all()
    # the same slot after a pose change: new xyz, the old entries stay as they are unless beaten
    before = eng.vmap_fetch()
    T = np.array(g["Tcw"][1], np.float32).copy()
    T[:, 3] += np.array([0.3, -0.2, 0.1], np.float32)
    eng.set_pose(1, T)
    eng.pointset([1], source=0)
    d = step(eng, ref, [1], [201], "moved", **kw)
    assert d["created"] > 0
    after = eng.vmap_fetch()
    stay = np.setdiff1d(np.arange(d["first_created"]), d["updated_ids"])
    for f in ("xyz", "pixel", "rho_sigma", "intensity", "tag", "epoch"):
        assert after[f][stay].tobytes() == before[f][stay].tobytes(), f
    eng.vmap_close()
    eng.close()


# 4. a call whose T reaches the second scan level, into a map that already holds entries
def test_1080p_dense_second_scan_level(pkg, gpu_ok):
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
    eng.vmap_open(0.006)
    ref = vmap_np.VoxelMap(0.006)
    d = step(eng, ref, [1], [7], "1080p first", **kw)
    assert d["created"] > 100000
    d = step(eng, ref, [2, 0, 1], [8, 9, 10], "1080p second level", **kw)
    print("1080p: T %d created %d updated %d" % (d["plain_total"], d["created"], d["updated"]))
    assert d["plain_total"] == 3 * W * H > 2048 * 2048 and d["created"] > 100000 and d["updated"] > 1000
    assert eng.vmap_info()["rehashes"] >= 2
    eng.vmap_close()
    eng.close()


# 5. destinations, the ids gather, NULL members, exact and short capacities
def test_destinations_and_capacity(pkg, engines):
    torch = pytest.importorskip("torch")
    g, eng = engines("plane_96x80_n20")
    kw = dict(max_sigma=0.3)
    first, second = [7, 1, 12, 0], [19, 3, 5]
    plain = [eng.extract_points(s, fields=ALL, **kw) for s in (first, second)]
    ref = vmap_np.VoxelMap(0.02)
    ref.integrate(plain[0], vmap_np.point_tags(plain[0]["offsets"], first))
    M0, T = ref.M, len(plain[1]["pixel"])
    exp = ref.integrate(plain[1], vmap_np.point_tags(plain[1]["offsets"], second))
    full = ref.fetch()
    U, M = exp["updated"], ref.M
    assert 0 < U < min(M0, T)

    def again(updated):
        eng.vmap_open(0.02)
        eng.vmap_integrate(first, updated=False, **kw)
        return eng.vmap_integrate(second, updated=updated, **kw)

    try:
        # updated_ids: made by the binding, pageable at the exact bound, pinned, device, not asked for
        got = again(True)
        np.testing.assert_array_equal(got["updated_ids"], exp["updated_ids"])
        eng.vmap_close()
        dest = np.full(min(M0, T), 0xABCD, np.uint32)
        got = again(dest)
        np.testing.assert_array_equal(got["updated_ids"], exp["updated_ids"])
        assert (dest[U:] == 0xABCD).all()
        eng.vmap_close()
        pinned = eng.host_alloc((min(M0, T) + 3,), np.uint32)
        np.testing.assert_array_equal(np.array(again(pinned)["updated_ids"]), exp["updated_ids"])
        eng.host_free(pinned)
        eng.vmap_close()
        dev = torch.full((min(M0, T),), 0x5A5A, dtype=torch.int32, device="cuda")
        got = again(dev)
        np.testing.assert_array_equal(got["updated_ids"].cpu().numpy().view(np.uint32), exp["updated_ids"])
        assert bool((dev[U:] == 0x5A5A).all())
        eng.vmap_close()
        got = again(False)
        assert "updated_ids" not in got and {f: got[f] for f in DELTA} == {f: exp[f] for f in DELTA}
        same_fetch(eng.vmap_fetch(), full, "without updated_ids")
        eng.vmap_close()
        # one short of the a-priori bound: EINVAL before the map changes, plain_total filled
        eng.vmap_open(0.02)
        eng.vmap_integrate(first, updated=False, **kw)
        snap = snapshot(eng)
        dest = np.full(min(M0, T) - 1, 0xABCD, np.uint32)
        with pytest.raises(pkg.SdmError) as e:
            eng.vmap_integrate(second, updated=dest, **kw)
        assert e.value.code == EINVAL and e.value.plain_total == T and e.value.first_created == M0
        assert (dest == 0xABCD).all()
        unchanged(eng, snap, "short updated_capacity")
        eng.vmap_integrate(second, updated=False, **kw)

        # fetch: pageable (above), pinned, device; range and ids; subsets of the fields
        same_fetch(eng.vmap_fetch(first=5, count=M - 9), {f: a[5:M - 4] for f, a in full.items()}, "range")
        same_fetch(eng.vmap_fetch(first=M, count=0), {f: a[M:] for f, a in full.items()}, "empty range at the end")
        ids = np.concatenate([np.random.default_rng(1).integers(0, M, 700), exp["updated_ids"], [M - 1, 0, 0]]).astype(np.uint32)
        same_fetch(eng.vmap_fetch(ids=ids), {f: a[ids] for f, a in full.items()}, "ids")
        rng_ids = np.arange(40, 300, dtype=np.uint32)
        same_fetch(eng.vmap_fetch(ids=rng_ids), eng.vmap_fetch(first=40, count=260), "ids against the range form")
        for fields in (("tag",), ("xyz", "epoch"), ("intensity",), ("rho_sigma", "multiplicity", "pixel")):
            same_fetch(eng.vmap_fetch(fields=fields), {f: full[f] for f in fields}, "fields %r" % (fields,))
            same_fetch(eng.vmap_fetch(ids=ids, fields=fields), {f: full[f][ids] for f in fields}, "ids fields %r" % (fields,))
        dt = {"xyz": (np.float32, (M, 3)), "pixel": (np.uint32, (M,)), "rho_sigma": (np.float32, (M, 2)),
              "intensity": (np.uint8, (M,)), "tag": (np.int32, (M,)), "multiplicity": (np.uint32, (M,)), "epoch": (np.uint32, (M,))}
        pinned = {f: eng.host_alloc(shape, d) for f, (d, shape) in dt.items()}  # exactly enough
        same_fetch({f: np.array(a) for f, a in eng.vmap_fetch(out=pinned).items()}, full, "pinned")
        same_fetch({f: np.array(a) for f, a in eng.vmap_fetch(ids=ids[:M], out=pinned).items()},
                   {f: a[ids[:M]] for f, a in full.items()}, "pinned ids")
        for a in pinned.values():
            eng.host_free(a)
        tdt = {np.float32: torch.float32, np.uint32: torch.int32, np.int32: torch.int32, np.uint8: torch.uint8}

        def device_out(m):
            return {f: torch.zeros((m,) + shape[1:], dtype=tdt[d], device="cuda") for f, (d, shape) in dt.items()}

        def to_host(res):
            return {f: t.cpu().numpy().view(dt[f][0]) for f, t in res.items()}

        same_fetch(to_host(eng.vmap_fetch(out=device_out(M))), full, "device")
        same_fetch(to_host(eng.vmap_fetch(first=3, count=50, out=device_out(64))), {f: a[3:53] for f, a in full.items()}, "device range")
        dev_ids = torch.from_numpy(ids.view(np.int32)).cuda()
        same_fetch(to_host(eng.vmap_fetch(ids=dev_ids, out=device_out(len(ids)))), {f: a[ids] for f, a in full.items()}, "device ids")
        sub = {f: t for f, t in device_out(len(ids)).items() if f in ("xyz", "tag")}
        same_fetch(to_host(eng.vmap_fetch(ids=dev_ids, out=sub)), {f: full[f][ids] for f in sub}, "device ids, two fields")
        # one short: EINVAL, nothing written
        out = {"xyz": np.full((M - 1, 3), 7.0, np.float32), "tag": np.full(M - 1, 77, np.int32)}
        with pytest.raises(pkg.SdmError) as e:
            eng.vmap_fetch(count=M, out=out)
        assert e.value.code == EINVAL and (out["xyz"] == 7.0).all() and (out["tag"] == 77).all()
    finally:
        try:
            eng.vmap_close()
        except pkg.SdmError:
            pass


# 6. refusals: each leaves the info and a full fetch as they were
def test_refusals(pkg, gpu_ok):
    torch = pytest.importorskip("torch")
    b = sys.modules[pkg.__name__ + ".binding"]
    g = gu.load("plane_64x48_n7")
    eng = pipeline(pkg, g, extra_slots=2)
    lib, ctx = eng.lib, eng.ctx
    spare, empty = g["n_kf"], g["n_kf"] + 1
    eng.upload_image(spare, g["im"][0], g["K"], g["Tcw"][0])
    eng.upload_depth(spare, *eng.download_depth(0))  # a depth map never inter-keyframe checked
    kw = dict(max_sigma=0.3, updated=False)

    def refused(code, fn, *a, **k):
        with pytest.raises(pkg.SdmError) as e:
            fn(*a, **k)
        assert e.value.code == code, (e.value, a, k)

    # no open map
    refused(ESTATE, eng.vmap_clear)
    refused(ESTATE, eng.vmap_close)
    refused(ESTATE, eng.vmap_info)
    refused(ESTATE, eng.vmap_integrate, [0], **kw)
    refused(ESTATE, eng.vmap_fetch, first=0, count=0)
    # open
    for voxel in (0.0, -0.02, float("nan"), float("inf"), 1e-45):
        refused(EINVAL, eng.vmap_open, voxel)
    refused(EINVAL, eng.vmap_open, 0.02, -1)
    refused(EINVAL, eng.vmap_open, 0.02, (1 << 30) + 1)
    refused(ESTATE, eng.vmap_info)
    eng2 = pipeline(pkg, g, with_pointset=False)
    refused(ESTATE, eng2.vmap_open, 0.02)
    eng2.close()
    eng.vmap_open(0.02)
    refused(ESTATE, eng.vmap_open, 0.02)
    refused(ESTATE, eng.vmap_open, 0.01, 100)
    eng.vmap_integrate([0, 1, 2], [50, 51, 52], **kw)
    snap = snapshot(eng)
    M = snap[0]["voxels"]
    assert M > 100

    def check(code, fn, *a, **k):
        refused(code, fn, *a, **k)
        unchanged(eng, snap, "%r %r" % (a, k))

    # integrate: the slot states and argument errors of sdm_extract_points
    check(ESTATE, eng.vmap_integrate, [3, empty], **kw)              # a slot without a depth map
    check(ESTATE, eng.vmap_integrate, [3, spare], source=1, **kw)    # never inter-keyframe checked
    check(EINVAL, eng.vmap_integrate, [3, 4, 3], **kw)               # a repeated slot
    check(EINVAL, eng.vmap_integrate, [3, 99], **kw)                 # a slot out of range
    check(EINVAL, eng.vmap_integrate, [3, -1], **kw)
    check(EINVAL, eng.vmap_integrate, [3], source=2, **kw)
    sl = (ctypes.c_int * 2)(3, 4)
    d = b.VmapDelta()
    assert lib.sdm_vmap_integrate(ctx, -1, sl, None, 1, 0.3, 1e-6, ctypes.byref(d)) == EINVAL
    assert lib.sdm_vmap_integrate(ctx, 2, None, None, 1, 0.3, 1e-6, ctypes.byref(d)) == EINVAL
    unchanged(eng, snap, "raw slot lists")
    # updated_ids: a negative or short capacity, a misaligned device pointer
    buf = torch.full((8192,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    host = np.full(8192, 0xABCD, np.uint32)
    T = int(eng.extract_points([3, 4], fields=("pixel",), max_sigma=0.3)["offsets"][-1])
    assert min(M, T) > 1
    for ptr, dev, cap in ((host.ctypes.data, 0, -1), (host.ctypes.data, 0, min(M, T) - 1), (buf.data_ptr() + 2, 1, 8000),
                          (buf.data_ptr(), 1, min(M, T) - 1)):
        d = b.VmapDelta()
        d.updated_ids, d.on_device, d.updated_capacity = ptr, dev, cap
        assert lib.sdm_vmap_integrate(ctx, 2, sl, None, 1, 0.3, 1e-6, ctypes.byref(d)) == EINVAL, (dev, cap)
        if cap == min(M, T) - 1:
            assert d.plain_total == T and d.first_created == M
        assert (d.created, d.updated, d.dropped) == (0, 0, 0)
        unchanged(eng, snap, "updated_ids %d %d" % (dev, cap))
    assert (host == 0xABCD).all() and bool((buf == 0x5A5A5A5A).all())
    # fetch
    check(EINVAL, eng.vmap_fetch, first=0, count=-1)
    check(EINVAL, eng.vmap_fetch, first=1, count=M)                   # a range beyond M
    check(EINVAL, eng.vmap_fetch, first=M + 1, count=0)
    check(EINVAL, eng.vmap_fetch, first=-1, count=1)
    check(EINVAL, eng.vmap_fetch, first=0, count=10, out={"tag": np.zeros(9, np.int32)})  # count > capacity
    check(EINVAL, eng.vmap_fetch, ids=np.array([0, M, 1], np.uint32))  # an id beyond M, host ids
    check(EINVAL, eng.vmap_fetch, ids=np.array([0, 1], np.uint32), first=1)
    check(EINVAL, eng.vmap_fetch, fields=())                          # no destination
    dev_ids = torch.tensor([0, 1, M, 2], dtype=torch.int32, device="cuda")
    check(EINVAL, eng.vmap_fetch, ids=dev_ids, out={"tag": torch.zeros(4, dtype=torch.int32, device="cuda")})  # the kernel's flag
    pb, vf = b.PointBuffers(), b.VmapFields()
    pb.capacity, pb.on_device = 4096, 1
    for where in ("xyz", "pixel", "rho_sigma", "tag", "multiplicity", "epoch", "ids"):
        pb.xyz = pb.pixel = pb.rho_sigma = vf.tag = vf.multiplicity = vf.epoch = None
        ids_ptr = None
        if where == "ids":
            vf.tag, ids_ptr = buf.data_ptr() + 4096, buf.data_ptr() + 2
        else:
            setattr(pb if where in ALL else vf, where, buf.data_ptr() + (4 if where == "rho_sigma" else 2))
        assert lib.sdm_vmap_fetch(ctx, ids_ptr, 0, 16, ctypes.byref(pb), ctypes.byref(vf)) == EINVAL, where
    assert lib.sdm_vmap_fetch(ctx, None, 0, 16, None, None) == EINVAL
    pb = b.PointBuffers()
    pb.capacity = 16
    assert lib.sdm_vmap_fetch(ctx, None, 0, 16, ctypes.byref(pb), None) == EINVAL  # no destination, extra NULL
    assert bool((buf == 0x5A5A5A5A).all())
    unchanged(eng, snap, "raw fetches")
    # the map still works, and as the restatement says
    ref = vmap_np.VoxelMap(0.02)
    plain = eng.extract_points([0, 1, 2], fields=ALL, max_sigma=0.3)
    ref.integrate(plain, vmap_np.point_tags(plain["offsets"], [0, 1, 2], [50, 51, 52]))
    step(eng, ref, [3, 4], None, "after the refusals", max_sigma=0.3)
    eng.vmap_close()
    eng.close()


# 7. clear = a fresh open with the table kept; close and reopen with another voxel size
def test_clear_and_reopen(engines):
    g, eng = engines("plane_160x120_n7")
    refs = list(range(g["n_kf"]))
    kw = dict(max_sigma=0.3)
    eng.vmap_open(0.005)
    try:
        ref = vmap_np.VoxelMap(0.005)
        for k in refs:
            step(eng, ref, [k], what="before clear", **kw)
        slots = eng.vmap_info()["table_slots"]
        assert slots > 1024
        eng.vmap_clear()
        info = eng.vmap_info()
        assert info == {"voxels": 0, "points": 0, "dropped": 0, "calls": 0, "table_slots": slots, "rehashes": 0,
                        "voxel_size": info["voxel_size"]}
        assert np.float32(info["voxel_size"]) == np.float32(0.005)
        assert all(len(a) == 0 for a in eng.vmap_fetch().values())
        ref = vmap_np.VoxelMap(0.005)
        for k in refs:  # (the same sequence: the table kept is large enough for it)
            d = step(eng, ref, [k], what="after clear", **kw)
        assert d["first_created"] > 0 and eng.vmap_info()["table_slots"] == slots and eng.vmap_info()["rehashes"] == 0
        eng.vmap_close()
        eng.vmap_open(0.05, 5000)
        assert eng.vmap_info()["table_slots"] == 16384 and np.float32(eng.vmap_info()["voxel_size"]) == np.float32(0.05)
        ref = vmap_np.VoxelMap(0.05)
        step(eng, ref, refs, what="reopened", **kw)
    finally:
        eng.vmap_close()


# 8. determinism and no side effects
def test_determinism_and_no_side_effects(pkg, gpu_ok):
    g = gu.load("plane_96x80_n20")
    refs = list(range(g["n_kf"]))
    nbrs = g["nbrs"][refs]
    kw = dict(max_sigma=0.3)
    engs = [pipeline(pkg, g), pipeline(pkg, g)]
    eng = engs[0]
    eng.enable_stats(True)
    before = _state(eng, refs)
    stats0 = eng.get_stats(reset=False)

    def views():
        return (eng.extract_points(refs, fields=ALL, **kw), eng.extract_points_voxel_cameras(refs, nbrs, 0.02, fields=ALL, **kw))

    def same_views(a, b, what):
        for x, y in zip(a, b):
            assert set(x) == set(y)
            for f in x:
                assert np.asarray(x[f]).tobytes() == np.asarray(y[f]).tobytes(), (what, f)

    v0 = views()
    fetched = []
    for e in engs:
        e.vmap_open(0.02)
        deltas = []
        for blk in (refs[:8], refs[8:9], refs[9:]):
            deltas.append(e.vmap_integrate(blk, [1000 + s for s in blk], **kw))
            if e is eng:
                same_views(v0, views(), "between the map calls")
        deltas.append(e.vmap_integrate(refs[:5], **kw))
        fetched.append((deltas, e.vmap_fetch(), e.vmap_info()))
    (d0, f0, i0), (d1, f1, i1) = fetched
    assert i0 == i1 and i0["voxels"] > 100
    for a, b2 in zip(d0, d1):
        assert {f: a[f] for f in DELTA} == {f: b2[f] for f in DELTA}
        assert a["updated_ids"].tobytes() == b2["updated_ids"].tobytes()
    assert sum(d["updated"] for d in d0[1:]) > 0
    same_fetch(f0, f1, "two engines")
    same_views(v0, views(), "after the map calls")
    assert eng.get_stats(reset=False) == stats0
    for x, y in zip(before, _state(eng, refs)):
        np.testing.assert_array_equal(x, y)
    eng.vmap_close()  # the second engine's map is freed by sdm_destroy
    for e in engs:
        e.close()


# 9. growth with every optional per-entry array present: what the old entries hold is carried over bit for bit, the new
# entries start empty
def test_growth_carries_every_array(engines):
    g, eng = engines("plane_64x48_n7")
    voxel, kw = 0.02, dict(max_sigma=0.3)
    slots, nbrs = [0, 1], np.ascontiguousarray(g["nbrs"][:2, :3])

    def everything(m):
        got = dict(eng.vmap_fetch(first=0, count=m))
        got.update(eng.vmap_fetch_evidence(first=0, count=m))
        got.update(eng.vmap_fetch_cameras(first=0, count=m))
        got["published"] = eng.vmap_fetch_published(first=0, count=m)
        return {f: np.array(a) for f, a in got.items()}

    eng.vmap_open(voxel, 0)
    try:
        T = eng.vmap_integrate(slots, updated=False, **kw)["plain_total"]
        eng.vmap_carve(slots, nbrs, **kw)
        eng.vmap_observe(slots, nbrs, **kw)
        assert eng.vmap_classify(dict(min_multiplicity=1), commit=True, ids=False)["accepted"] > 0
        info = eng.vmap_info()
        M0, r0 = info["voxels"], info["rehashes"]
        before = everything(M0)
        assert M0 > 100 and before["crossings"].any() and before["ends"].any()
        assert len(before["cam_tags"]) >= M0 and before["published"].any()
        # records at fresh voxels, far from the scene, until the table has rehashed and the records have outgrown both
        # 2 * M0 and the capacity the integrate left (its plain points)
        n = 0
        while info["rehashes"] == r0 or info["voxels"] <= max(2 * M0, T):
            i = np.arange(n, n + 1500)
            n += 1500
            xyz = ((np.stack([i % 64, i // 64, np.full(len(i), 5000)], axis=1) + 0.5) * voxel).astype(np.float32)
            d = eng.vmap_import({"xyz": xyz, "rho_sigma": np.full((len(i), 2), 0.5, np.float32)}, dst_ids=False, updated=False)
            assert d["created"] == len(i)
            info = eng.vmap_info()
        M = info["voxels"]
        assert M == M0 + n
        after = everything(M)
        for f in before:
            m = before["cam_offsets"][-1] if f == "cam_tags" else len(before[f])
            assert after[f][:m].tobytes() == before[f].tobytes(), f
        assert not after["crossings"][M0:].any() and not after["ends"][M0:].any() and not after["published"][M0:].any()
        assert (after["cam_offsets"][M0:] == before["cam_offsets"][-1]).all() and len(after["cam_tags"]) == len(before["cam_tags"])
    finally:
        eng.vmap_close()
