"""GPU: sdm_extract_points_voxel / Engine.extract_points_voxel against tests/voxel_np.py fed the engine's own
extract_points(fields=ALL) for the same arguments -- every returned array compared for equality (floats as uint32)."""
import ctypes
import sys

import numpy as np
import pytest

import golden_util as gu
import voxel_np
from common import bits
from test_gpu_extract import ALL, EINVAL, ESTATE, _state, pipeline

pytestmark = pytest.mark.gpu

VOXELS = (1e-4, 0.005, 0.02, 1000.0, 1e-7)


@pytest.fixture(scope="module")
def engines(pkg, gpu_ok):
    """the golden fixtures run through the pipeline once each; shared by the tests that change no state"""
    made = {}

    def get(name):
        if name not in made:
            g = gu.load(name)
            made[name] = (g, pipeline(pkg, g))
        return made[name]

    yield get
    for _, eng in made.values():
        eng.close()


def expected(plain, voxel):
    """voxel_np over a plain extraction (fields=ALL) -> what extract_points_voxel(representative=True) must return"""
    kept, mult, rep, offs = voxel_np.voxel_merge(plain["xyz"], plain["rho_sigma"][:, 1], voxel, plain["offsets"])
    exp = {f: np.asarray(plain[f])[kept] for f in plain if f != "offsets"}
    exp.update(offsets=offs, multiplicity=mult, source_index=kept, representative=rep, plain_total=len(plain["xyz"]))
    return exp


def assert_same(got, exp, what=""):
    assert int(got["plain_total"]) == exp["plain_total"], what
    np.testing.assert_array_equal(np.asarray(got["offsets"]), exp["offsets"], err_msg=what + " offsets")
    for f, g in got.items():
        if f in ("offsets", "plain_total"):
            continue
        g, e = np.asarray(g), exp[f]
        assert g.shape == e.shape, (what, f, g.shape, e.shape)
        if f in ("xyz", "rho_sigma"):
            np.testing.assert_array_equal(bits(g), bits(e), err_msg="%s %s" % (what, f))
        else:
            np.testing.assert_array_equal(g.astype(np.int64), e.astype(np.int64), err_msg="%s %s" % (what, f))


def run(eng, slots, voxel, what="", **kw):
    """one voxel call with every output against the restatement; returns (got, plain)"""
    plain = eng.extract_points(slots, fields=ALL, **kw)
    got = eng.extract_points_voxel(slots, voxel, fields=ALL, representative=True, **kw)
    assert set(got) == set(ALL) | {"offsets", "multiplicity", "source_index", "representative", "plain_total"}
    assert_same(got, expected(plain, voxel), "%s voxel %r" % (what, voxel))
    return got, plain


def invariants(got, plain):
    T, M = int(got["plain_total"]), len(got["source_index"])
    assert int(got["multiplicity"].astype(np.int64).sum()) == T
    assert (np.diff(got["source_index"].astype(np.int64)) > 0).all()
    np.testing.assert_array_equal(got["representative"][got["source_index"]], np.arange(M))
    slot_of = np.searchsorted(plain["offsets"][1:], got["source_index"], side="right")  # slot index of each kept point
    np.testing.assert_array_equal(got["offsets"], np.searchsorted(slot_of, np.arange(len(plain["offsets"]))))
    return T, M


# 1. the golden fixtures; 4a. a kept count that crosses a tile within a slot and slot boundaries inside tiles
@pytest.mark.parametrize("name", gu.fixture_names())
def test_golden_fixtures(engines, name):
    g, eng = engines(name)
    refs = list(range(g["n_kf"]))
    for src in (1, 0):
        for voxel in VOXELS:
            got, plain = run(eng, refs, voxel, "%s src %d" % (name, src), source=src, max_sigma=0.3)
            T, M = invariants(got, plain)
            assert T > 1000
            if voxel == 0.02:
                assert M < T / 3
                slot_of = np.searchsorted(plain["offsets"][1:], np.arange(T), side="right")
                lo, hi = np.full(M, len(refs)), np.full(M, -1)
                np.minimum.at(lo, got["representative"], slot_of)
                np.maximum.at(hi, got["representative"], slot_of)
                assert int((lo < hi).sum()) >= 100
            if voxel == 1e-7 and src == 1:
                assert M == T and (got["multiplicity"] == 1).all()
            if voxel == 1e-7 and src == 0:
                # the point sets were made from the checked planes: a depth-map rho the check removed sits at the stored
                # (0, 0, 0), and those points share one voxel at any size; every other point stays alone
                zero = (bits(plain["xyz"]) == 0).all(axis=1)
                assert M == T - int(zero.sum()) + int(zero.any())
                assert (got["multiplicity"][got["representative"][~zero]] == 1).all()
            if voxel == 1000.0:
                assert M <= 8
            if voxel == 1e-4 and name != "plane_64x48_n7":
                per_slot = np.diff(got["offsets"])
                assert per_slot.max() > 2048 or M > 2048  # more than one tile of kept points
                assert (np.asarray(plain["offsets"][1:-1]) % 2048 != 0).any()  # a slot boundary inside a tile


# 2. the slot listed first wins ties
def test_slot_order_decides_ties(pkg, gpu_ok):
    g = gu.load("plane_64x48_n7")
    W, H = g["W"], g["H"]
    eng = pkg.Engine(W, H, 2)
    rng = np.random.default_rng(2)
    rho = np.where(rng.random((H, W)) < 0.5, rng.uniform(0.5, 2.0, (H, W)), 0).astype(np.float32)
    sigma = np.where(rho != 0, rng.uniform(0.001, 0.009, (H, W)), 0).astype(np.float32)
    for s in (0, 1):
        eng.upload_image(s, g["im"][0], g["K"], g["Tcw"][0])
        eng.upload_depth(s, rho, sigma)
    eng.pointset([0, 1], source=0)
    for order in ([0, 1], [1, 0]):
        got, plain = run(eng, order, 0.01, "order %r" % (order,), source=0)
        T, _ = invariants(got, plain)
        assert T > 1000 and T % 2 == 0
        assert got["offsets"][1] == got["offsets"][2] > 0  # every kept point is the first-listed slot's
        assert (got["multiplicity"] % 2 == 0).all()
    # a smaller sigma at a few pixels of the second-listed slot: exactly those move to it
    base, _ = run(eng, [0, 1], 0.01, "base", source=0)
    inset = np.zeros((H, W), bool)
    inset[2:H - 2, 2:W - 2] = True  # (outside it the stored xyz is (0, 0, 0) for every pixel: one voxel)
    ys, xs = np.nonzero((rho > 1e-6) & inset)
    pick = rng.choice(len(ys), 5, replace=False)
    sig1 = sigma.copy()
    sig1[ys[pick], xs[pick]] = 0.0005  # below every sigma of the map: wins its voxel whatever else is in it
    eng.upload_depth(1, rho, sig1)
    eng.pointset([1], source=0)
    got, plain = run(eng, [0, 1], 0.01, "lowered", source=0)
    moved = got["pixel"][got["offsets"][1]:]
    assert sorted(moved.tolist()) == sorted(((ys[pick].astype(np.uint32) << 16) | xs[pick].astype(np.uint32)).tolist())
    assert len(got["source_index"]) <= len(base["source_index"]) + 5
    eng.close()


def _crafted(W, H, rng):
    """rho in {0, 1e-39, 1, 2, 4} (xyz on cell faces for the pose and K below), sigma with +0, -0, NaN and ties"""
    f = np.float32
    rho = rng.choice(np.array([0, 1e-39, 1, 1, 2, 4], f), (H, W))
    sigma = rng.choice(np.array([0.0, -0.0, np.nan, 0.004, 0.004, 0.002], f), (H, W))
    return rho, sigma


# 3. crafted maps: cell faces, both sides of zero, unmergeable points, sigma's total order, every lane on one table slot
@pytest.mark.parametrize("W,H", [(32, 24), (64, 48)])
def test_crafted_maps(pkg, gpu_ok, W, H):
    """(A rho below 1e-6 back-projects to (0, 0, 0), PM.cc:345, so no 1 / rho overflows; the non-finite and out-of-range
    coordinates come from the third slot's focal length of 2e-38.)"""
    eng = pkg.Engine(W, H, 3)
    rng = np.random.default_rng(W)
    im = rng.integers(0, 256, (H, W)).astype(np.uint8)
    eye = np.eye(4, dtype=np.float32)[:3]
    K = np.array([16, 16, W / 2, H / 2], np.float32)  # X = Z (x - W/2) / 16: multiples of 1/16 at Z = 1
    for s in range(3):
        eng.upload_image(s, im, K if s < 2 else np.array([2e-38, 2e-38, W / 2, H / 2], np.float32), eye)
        eng.upload_depth(s, *_crafted(W, H, rng))
    eng.pointset([0, 1, 2], source=0)
    for voxel in (0.25, 0.0625, 1.0):
        got, plain = run(eng, [2, 0, 1], voxel, "crafted", source=0, max_sigma=0.01, min_rho=-1.0)
        T, M = invariants(got, plain)
        assert T == 3 * W * H  # NaN, +-0 and every other sigma pass, and so does every rho
        xyz = plain["xyz"]
        assert (~np.isfinite(xyz)).any() and (xyz < 0).any() and (xyz > 0).any()
        zeros = int((bits(xyz) == 0).all(axis=1).sum())
        assert zeros > T // 8 and got["multiplicity"].max() >= zeros  # the zero-rho pixels share one voxel
        _, ok = voxel_np.cells(xyz, voxel)
        assert 0 < int((~ok).sum()) and (got["multiplicity"][got["representative"][~ok]] == 1).all()
        inv = np.float32(1) / np.float32(voxel)
        fin = np.isfinite(xyz)
        with np.errstate(over="ignore"):
            assert (xyz[fin] * inv == np.floor(xyz[fin] * inv)).mean() > 0.5  # points exactly on cell faces
    eng.close()


# 4b. more than 2048 x 2048 plain points: the second scan level of the voxel passes
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
    order = [2, 0, 1]
    plain = eng.extract_points(order, source=0, min_rho=-1.0, fields=("xyz", "rho_sigma"))
    T = len(plain["xyz"])
    assert T == 3 * W * H > 2048 * 2048
    got = eng.extract_points_voxel(order, 0.006, source=0, min_rho=-1.0, fields=("xyz", "rho_sigma"), representative=True)
    exp = expected(plain, 0.006)
    print("1080p: T %d M %d" % (T, len(exp["source_index"])))
    assert 0.3 * T < len(exp["source_index"]) < 0.7 * T  # the voxel keeps about half
    assert_same(got, exp, "1080p")
    eng.close()


# 5. destinations and capacity
def test_destinations_and_capacity(pkg, engines):
    torch = pytest.importorskip("torch")
    g, eng = engines("plane_96x80_n20")
    refs = [7, 1, 12, 0, 19, 3]
    kw = dict(max_sigma=0.3)
    plain = eng.extract_points(refs, fields=ALL, **kw)
    exp = expected(plain, 0.02)
    T, M = exp["plain_total"], len(exp["source_index"])
    assert 1 < M < T
    assert_same(eng.extract_points_voxel(refs, 0.02, fields=ALL, representative=True, **kw), exp, "pageable")
    cap = M + 5
    u32 = ("pixel", "multiplicity", "source_index", "representative")
    dev = {"xyz": torch.empty((cap, 3), dtype=torch.float32, device="cuda"),
           "pixel": torch.empty(cap, dtype=torch.int32, device="cuda"),
           "rho_sigma": torch.empty((cap, 2), dtype=torch.float32, device="cuda"),
           "intensity": torch.empty(cap, dtype=torch.uint8, device="cuda"),
           "multiplicity": torch.empty(cap, dtype=torch.int32, device="cuda"),
           "source_index": torch.empty(cap, dtype=torch.int32, device="cuda"),
           "representative": torch.empty(T + 3, dtype=torch.int32, device="cuda")}
    got = eng.extract_points_voxel(refs, 0.02, out=dev, representative=True, **kw)
    host = {f: (t.cpu().numpy() if hasattr(t, "cpu") else t) for f, t in got.items()}
    for f in u32:
        host[f] = host[f].view(np.uint32)
    assert_same(host, exp, "device")
    pinned = {"xyz": eng.host_alloc((cap, 3), np.float32), "pixel": eng.host_alloc((cap,), np.uint32),
              "rho_sigma": eng.host_alloc((cap, 2), np.float32), "intensity": eng.host_alloc((cap,), np.uint8),
              "multiplicity": eng.host_alloc((cap,), np.uint32), "source_index": eng.host_alloc((cap,), np.uint32),
              "representative": eng.host_alloc((T + 3,), np.uint32)}
    got = eng.extract_points_voxel(refs, 0.02, out=pinned, representative=True, **kw)
    assert_same({k: np.array(v) for k, v in got.items()}, exp, "pinned")
    for a in pinned.values():
        eng.host_free(a)
    # no point field: only the vox outputs
    got = eng.extract_points_voxel(refs, 0.02, fields=(), representative=True, **kw)
    assert set(got) == {"offsets", "multiplicity", "source_index", "representative", "plain_total"}
    assert_same(got, exp, "fields=()")
    got = eng.extract_points_voxel(refs, 0.02, fields=(), **kw)
    assert set(got) == {"offsets", "multiplicity", "source_index", "plain_total"}
    assert_same(got, exp, "fields=() without representative")

    def sentinel(m, t):
        return {"xyz": np.full((m, 3), 7.0, np.float32), "multiplicity": np.full(m, 0xABCD, np.uint32),
                "source_index": np.full(m, 0xABCD, np.uint32), "representative": np.full(t, 0xABCD, np.uint32)}

    out = sentinel(M, T)  # exactly enough
    assert_same(eng.extract_points_voxel(refs, 0.02, out=out, representative=True, **kw), exp, "exact capacity")
    for m, t in ((M - 1, T), (M, T - 1)):  # one short: EINVAL, offsets and plain_total filled, nothing written
        out = sentinel(m, t)
        with pytest.raises(pkg.SdmError) as e:
            eng.extract_points_voxel(refs, 0.02, out=out, representative=True, **kw)
        assert e.value.code == EINVAL
        np.testing.assert_array_equal(e.value.offsets, exp["offsets"])
        assert e.value.plain_total == T
        assert (out["xyz"] == 7.0).all() and all((out[f] == 0xABCD).all() for f in out if f != "xyz")


# 6. errors leave the buffers alone
def test_errors(pkg, engines):
    torch = pytest.importorskip("torch")
    g, eng = engines("plane_64x48_n7")

    def fresh():
        return {"xyz": np.full((4096, 3), 7.0, np.float32), "multiplicity": np.full(4096, 0xABCD, np.uint32),
                "source_index": np.full(4096, 0xABCD, np.uint32), "representative": np.full(8192, 0xABCD, np.uint32)}

    def untouched(out):
        return (out["xyz"] == 7.0).all() and all((out[f] == 0xABCD).all() for f in out if f != "xyz")

    for voxel in (0.0, -0.02, float("nan"), float("inf"), 1e-45):
        out = fresh()
        with pytest.raises(pkg.SdmError) as e:
            eng.extract_points_voxel([0, 1], voxel, max_sigma=0.3, out=out, representative=True)
        assert e.value.code == EINVAL, voxel
        assert untouched(out)
    out = fresh()
    with pytest.raises(pkg.SdmError) as e:
        eng.extract_points_voxel([0, 1, 0], 0.02, max_sigma=0.3, out=out, representative=True)  # a repeated slot
    assert e.value.code == EINVAL and untouched(out)
    # a misaligned device multiplicity
    b = sys.modules[pkg.__name__ + ".binding"]
    buf = torch.full((8192,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    pb, vb = b.PointBuffers(), b.VoxelBuffers()
    pb.capacity, pb.on_device = 4096, 1
    vb.multiplicity = buf.data_ptr() + 2
    offs = (ctypes.c_longlong * 3)()
    sl = (ctypes.c_int * 2)(0, 1)
    rc = eng.lib.sdm_extract_points_voxel(eng.ctx, 2, sl, 1, 0.3, 1e-6, 0.02, ctypes.byref(pb), ctypes.byref(vb), offs)
    assert rc == EINVAL and bool((buf == 0x5A5A5A5A).all())
    vb.multiplicity = None  # no destination at all
    assert eng.lib.sdm_extract_points_voxel(eng.ctx, 2, sl, 1, 0.3, 1e-6, 0.02, ctypes.byref(pb), ctypes.byref(vb), offs) == EINVAL
    assert eng.lib.sdm_extract_points_voxel(eng.ctx, 2, sl, 1, 0.3, 1e-6, 0.02, ctypes.byref(pb), None, offs) == EINVAL
    # a context without the point-set pool: the merge reads the plane even when xyz is not asked for
    eng2 = pipeline(pkg, g, with_pointset=False)
    out = {"pixel": np.full(4096, 0xABCD, np.uint32)}
    with pytest.raises(pkg.SdmError) as e:
        eng2.extract_points_voxel([0, 1], 0.02, max_sigma=0.3, out=out)
    assert e.value.code == ESTATE and (out["pixel"] == 0xABCD).all()
    eng2.close()


# 7. no side effects, determinism, scratch reuse after a larger call
def test_no_side_effects_and_determinism(pkg, gpu_ok):
    g = gu.load("plane_160x120_n7")
    eng = pipeline(pkg, g)
    refs = list(range(g["n_kf"]))
    eng.enable_stats(True)
    before = _state(eng, refs)
    stats0 = eng.get_stats(reset=False)
    plain0 = eng.extract_points(refs, max_sigma=0.3, fields=ALL)
    a, _ = run(eng, refs, 0.02, "first", max_sigma=0.3)
    b = eng.extract_points_voxel(refs, 0.02, max_sigma=0.3, fields=ALL, representative=True)
    for f in a:
        assert np.asarray(a[f]).tobytes() == np.asarray(b[f]).tobytes(), f
    assert eng.get_stats(reset=False) == stats0
    for x, y in zip(before, _state(eng, refs)):
        np.testing.assert_array_equal(x, y)
    plain1 = eng.extract_points(refs, max_sigma=0.3, fields=ALL)
    for f in plain0:
        assert np.asarray(plain0[f]).tobytes() == np.asarray(plain1[f]).tobytes(), f
    # a much smaller call right after (the scratch of the larger one reused, a smaller table inside it)
    got, plain = run(eng, [3], 0.02, "after a larger call", max_sigma=0.3)
    assert 0 < got["plain_total"] < a["plain_total"] // 4
    eng.close()


# 8. composition with the visibility lists
def test_composition_with_support(engines):
    g, eng = engines("plane_96x80_n20")
    refs = [4, 9, 2, 15, 10]
    nbrs = g["nbrs"][refs]
    sup = eng.extract_points_support(refs, nbrs, max_sigma=0.3, fields=("pixel",))
    got = eng.extract_points_voxel(refs, 0.02, max_sigma=0.3, fields=("pixel",), representative=True)
    T, M = int(got["plain_total"]), len(got["source_index"])
    assert T == len(sup["support"]) and 0 < M < T
    np.testing.assert_array_equal(sup["pixel"][got["source_index"]], got["pixel"])
    own = sup["support"][got["source_index"]]  # the words of the kept points
    # the union over each kept point's voxel, in camera indices (bit j names a different keyframe for each slot)
    slot_of = np.searchsorted(sup["offsets"][1:], np.arange(T), side="right")
    cams = [set() for _ in range(M)]
    for gidx in np.flatnonzero(sup["support"]):
        w, k = int(sup["support"][gidx]), int(got["representative"][gidx])
        cams[k].update(int(nbrs[slot_of[gidx]][j]) for j in range(nbrs.shape[1]) if w >> j & 1)
    kept_slot = slot_of[got["source_index"]]
    grew = 0
    for k in range(M):
        mine = {int(nbrs[kept_slot[k]][j]) for j in range(nbrs.shape[1]) if int(own[k]) >> j & 1}
        assert mine <= cams[k]
        grew += mine < cams[k]
    assert grew > 0  # some merged point gained cameras from the points it stands for
