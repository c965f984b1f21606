"""GPU: sdm_extract_points_voxel_cameras / Engine.extract_points_voxel_cameras against the composition it replaces -- the
engine's own extract_points_support and extract_points_voxel(representative=True) for the same arguments, joined by
tests/voxcam_np.py.  Every returned array is compared for equality; there are no tolerances."""
import ctypes
import sys

import numpy as np
import pytest

import golden_util as gu
import voxcam_np
from common import bits
from test_gpu_extract import ALL, EINVAL, ESTATE, _state, pipeline

pytestmark = pytest.mark.gpu

VOXELS = (1e-4, 0.005, 0.02, 1000.0, 1e-7)
VOX_OUT = ("multiplicity", "source_index", "representative")


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


def reference(eng, slots, nbrs, voxel, fields=ALL, **kw):
    """today's route: the support words and the merged cloud from the engine, the lists from voxcam_np"""
    sup = eng.extract_points_support(slots, nbrs, fields=(), **kw)
    vox = eng.extract_points_voxel(slots, voxel, fields=fields, representative=True, **kw)
    M = len(vox["source_index"])
    assert len(sup["support"]) == int(vox["plain_total"])
    offs, cs = voxcam_np.voxel_cameras(sup["support"], sup["offsets"], slots, nbrs, vox["representative"], M)
    exp = {f: np.asarray(v) for f, v in vox.items()}
    exp.update(cam_offsets=offs, cam_slots=cs, cam_total=len(cs))
    return exp, sup


def assert_same(got, exp, what=""):
    """every output of the call: extract_points_voxel's bit for bit, and the lists"""
    assert int(got["plain_total"]) == int(exp["plain_total"]), what
    assert int(got["cam_total"]) == int(exp["cam_total"]), what
    for f, g in got.items():
        if f in ("plain_total", "cam_total"):
            continue
        g, e = np.asarray(g), np.asarray(exp[f])
        assert g.shape == e.shape, (what, f, g.shape, e.shape)
        if f in ("xyz", "rho_sigma"):
            np.testing.assert_array_equal(bits(g), bits(e), err_msg="%s %s" % (what, f))
        else:
            np.testing.assert_array_equal(g.astype(np.int64), e.astype(np.int64), err_msg="%s %s" % (what, f))


def run(eng, slots, nbrs, voxel, what="", fields=ALL, **kw):
    exp, sup = reference(eng, slots, nbrs, voxel, fields=fields, **kw)
    got = eng.extract_points_voxel_cameras(slots, nbrs, voxel, fields=fields, representative=True, **kw)
    assert set(got) == set(fields) | set(VOX_OUT) | {"offsets", "plain_total", "cam_offsets", "cam_slots", "cam_total"}
    assert got["cam_offsets"].dtype == np.int64 and got["cam_slots"].dtype == np.int32
    assert_same(got, exp, "%s voxel %r" % (what, voxel))
    return got, exp, sup


def own_lengths(sup, slots, nbrs, source_index):
    """|C(g)| of the kept points: the list each would carry from its own support word alone"""
    T = len(sup["support"])
    offs, _ = voxcam_np.voxel_cameras(sup["support"], sup["offsets"], slots, nbrs, np.arange(T), T)
    return np.diff(offs)[np.asarray(source_index, np.int64)]


# 1. the golden fixtures: short and full rows, both sources, every voxel size; 4a. M > 2048 with slot boundaries in tiles
@pytest.mark.parametrize("name", gu.fixture_names())
def test_golden_fixtures(engines, name):
    g, eng = engines(name)
    refs = list(range(g["n_kf"]))
    for rows, short in ((g["nbrs"][:, :3], True), (g["nbrs"], False)):
        for src in (1, 0):
            for voxel in VOXELS:
                got, exp, sup = run(eng, refs, rows, voxel, "%s src %d short %d" % (name, src, short), source=src, max_sigma=0.3)
                M, lens = len(got["source_index"]), np.diff(got["cam_offsets"])
                assert (lens >= 1).all() and got["cam_offsets"][0] == 0 and got["cam_offsets"][-1] == got["cam_total"]
                if voxel == 0.02 and short and src == 1:
                    own = own_lengths(sup, refs, rows, got["source_index"])
                    gained, beyond = int((lens > own).sum()), int((lens > rows.shape[1] + 1).sum())
                    print("%s: M %d, %d kept points gain a camera, %d hold more than 4" % (name, M, gained, beyond))
                    assert gained >= 500 and beyond >= 500
                if voxel == 1e-7 and src == 1:
                    assert M == int(got["plain_total"])
                    np.testing.assert_array_equal(lens, own_lengths(sup, refs, rows, got["source_index"]))
                if voxel == 1000.0:
                    assert M <= 8
                if voxel == 1e-4 and name == "plane_160x120_n7":
                    assert M > 2048 and (np.asarray(got["offsets"][1:-1]) % 2048 != 0).any()
    # shuffled slots, and every row permuted on its own: the lists follow the slot ids, not the bit positions
    rng = np.random.default_rng(5)
    order = [int(s) for s in rng.permutation(g["n_kf"])]
    rows = np.stack([g["nbrs"][s][rng.permutation(g["n"])][:3] for s in order])
    run(eng, order, rows, 0.02, name + " shuffled", max_sigma=0.3)


# 2. more than one bitset word: 180 cameras at scattered slot ids, rows of 40 neighbours
def test_three_bitset_words(pkg, gpu_ok):
    g = gu.load("plane_64x48_n7")
    S, n_cam, n_nbr = 208, 180, 40
    eng = pkg.Engine(g["W"], g["H"], S, max_neighbours=n_nbr)
    rng = np.random.default_rng(8)
    ids = [int(s) for s in rng.permutation(S)[:n_cam]]  # slot id != camera index
    for q, s in enumerate(ids):  # the fixture's keyframes and maps, over and over
        k = q % g["n_kf"]
        eng.upload_image(s, g["im"][k], g["K"], g["Tcw"][k])
        eng.upload_depth(s, g["rho"][k], g["sigma"][k])
    eng.pointset(ids, source=0)
    slots = ids[:6]
    deal = [int(s) for s in rng.permutation(ids)]
    rows = np.array([[deal[(i * n_nbr + j) % n_cam] for j in range(n_nbr)] for i in range(6)], np.int32)
    rows[1, 35] = rows[1, 2]   # a repeated neighbour
    rows[2, 33] = slots[2]     # a neighbour equal to the row's own slot
    table = voxcam_np.camera_table(slots, rows)
    assert len(table) > 128 and (table != np.arange(len(table))).any()
    for i in range(6):  # every row spans all three words
        assert set(np.searchsorted(table, rows[i]) >> 6) == {0, 1, 2}
    for voxel in (0.02, 1000.0, 1e-7):
        got, exp, sup = run(eng, slots, rows, voxel, "three words", source=0, max_sigma=0.3)
        assert (sup["support"] >> np.uint64(32)).any()  # bits 32 - 63 used
        used = np.searchsorted(table, got["cam_slots"]) >> 6
        assert set(used.tolist()) == {0, 1, 2}
    eng.close()


# 3. crafted maps: unmergeable points, zero words, every lane of every wave on one bitset word
@pytest.mark.parametrize("W,H", [(32, 24), (64, 48)])
def test_crafted_maps(pkg, gpu_ok, W, H):
    from test_gpu_voxel import _crafted
    import voxel_np
    eng = pkg.Engine(W, H, 3)
    rng = np.random.default_rng(W)
    im = rng.integers(0, 256, (H, W)).astype(np.uint8)
    eye = np.eye(4, dtype=np.float32)[:3]
    K = np.array([16, 16, W / 2, H / 2], np.float32)
    for s in range(3):
        eng.upload_image(s, im, K if s < 2 else np.array([2e-38, 2e-38, W / 2, H / 2], np.float32), eye)
        eng.upload_depth(s, *_crafted(W, H, rng))
    eng.pointset([0, 1, 2], source=0)
    slots, rows = [2, 0, 1], np.array([[0, 1], [1, 2], [2, 0]], np.int32)
    kw = dict(source=0, max_sigma=0.01, min_rho=-1.0)
    for voxel in (1000.0, 0.25):
        got, exp, sup = run(eng, slots, rows, voxel, "crafted", **kw)
        T = int(got["plain_total"])
        assert T == 3 * W * H
        lists = voxcam_np.lists(got["cam_offsets"], got["cam_slots"])
        own_offs, own_cs = voxcam_np.voxel_cameras(sup["support"], sup["offsets"], slots, rows, np.arange(T), T)
        own = voxcam_np.lists(own_offs, own_cs)
        plain = eng.extract_points(slots, fields=("xyz",), **kw)
        _, ok = voxel_np.cells(plain["xyz"], voxel)
        row_of = np.searchsorted(sup["offsets"][1:], np.arange(T), side="right")
        lone = np.flatnonzero(~ok)
        assert len(lone) > 0
        for q in lone:  # an unmergeable point keeps exactly its own C(g)
            assert lists[got["representative"][q]] == own[q]
        lone_zero = [q for q in lone if sup["support"][q] == 0]
        assert lone_zero and all(lists[got["representative"][q]] == [slots[row_of[q]]] for q in lone_zero)
        if voxel == 1000.0:
            zeros = (bits(plain["xyz"]) == 0).all(axis=1)
            assert zeros.sum() > T // 8 and len(set(got["representative"][zeros].tolist())) == 1  # one voxel, one word
            assert lists[got["representative"][np.flatnonzero(zeros)[0]]] == [0, 1, 2]
    eng.close()


# 4b. more than 2048 x 2048 KEPT points: the second scan level of the list pass
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
    order, rows = [2, 0, 1], np.array([[0, 1], [1, 2], [2, 0]], np.int32)
    kw = dict(source=0, min_rho=-1.0)
    exp, sup = reference(eng, order, rows, 0.003, fields=(), **kw)
    T, M = int(exp["plain_total"]), len(exp["source_index"])
    print("1080p: T %d M %d E %d" % (T, M, exp["cam_total"]))
    assert T == 3 * W * H and M > 2048 * 2048
    got = eng.extract_points_voxel_cameras(order, rows, 0.003, fields=(), representative=True, **kw)
    assert_same(got, exp, "1080p")
    assert len(set(np.diff(got["cam_offsets"]).tolist())) >= 2
    eng.close()


def _raw(eng, b, slots, rows, voxel, pb, vb, vc, max_sigma=0.3, source=1):
    """the C call itself -> (rc, offsets)"""
    sl = (ctypes.c_int * len(slots))(*slots)
    flat = [int(v) for v in np.asarray(rows).reshape(-1)]
    nb = (ctypes.c_int * max(len(flat), 1))(*flat)
    offs = (ctypes.c_longlong * (len(slots) + 1))()
    n_nbr = np.asarray(rows).shape[1]
    rc = eng.lib.sdm_extract_points_voxel_cameras(eng.ctx, len(slots), sl, n_nbr, nb, source, max_sigma, 1e-6, voxel,
                                                  ctypes.byref(pb), ctypes.byref(vb) if vb is not None else None,
                                                  ctypes.byref(vc), offs)
    return rc, np.array(offs[:], np.int64)


# 5. destinations and capacities
def test_destinations_and_capacity(pkg, engines):
    torch = pytest.importorskip("torch")
    b = sys.modules[pkg.__name__ + ".binding"]
    g, eng = engines("plane_96x80_n20")
    refs = [7, 1, 12, 0, 19, 3]
    rows = g["nbrs"][refs][:, :3]
    kw = dict(max_sigma=0.3)
    exp, _ = reference(eng, refs, rows, 0.02, **kw)
    T, M, E = int(exp["plain_total"]), len(exp["source_index"]), int(exp["cam_total"])
    assert 1 < M < T and E > M
    assert_same(eng.extract_points_voxel_cameras(refs, rows, 0.02, fields=ALL, representative=True, **kw), exp, "pageable")
    no_rep = eng.extract_points_voxel_cameras(refs, rows, 0.02, fields=("xyz",), **kw)  # ranks in the engine's own scratch
    assert "representative" not in no_rep
    assert_same(no_rep, exp, "without representative")
    cap = M + 5
    i32 = ("pixel",) + VOX_OUT + ("cam_slots",)
    dev = {"xyz": torch.empty((cap, 3), dtype=torch.float32, device="cuda"),
           "pixel": torch.empty(cap, dtype=torch.int32, device="cuda"),
           "rho_sigma": torch.empty((cap, 2), dtype=torch.float32, device="cuda"),
           "intensity": torch.empty(cap, dtype=torch.uint8, device="cuda"),
           "multiplicity": torch.empty(cap, dtype=torch.int32, device="cuda"),
           "source_index": torch.empty(cap, dtype=torch.int32, device="cuda"),
           "representative": torch.empty(T + 3, dtype=torch.int32, device="cuda"),
           "cam_offsets": torch.empty(cap + 1, dtype=torch.int64, device="cuda"),
           "cam_slots": torch.empty(E + 7, dtype=torch.int32, device="cuda")}
    got = eng.extract_points_voxel_cameras(refs, rows, 0.02, out=dev, representative=True, **kw)
    host = {f: (t.cpu().numpy() if hasattr(t, "cpu") else t) for f, t in got.items()}
    for f in i32:
        host[f] = host[f].view(np.uint32 if f != "cam_slots" else np.int32)
    assert_same(host, exp, "device")
    # cam_slots = NULL on the device: the offsets only, and nothing else named
    only = {"cam_offsets": torch.full((cap + 1,), -1, dtype=torch.int64, device="cuda")}
    got = eng.extract_points_voxel_cameras(refs, rows, 0.02, out=only, **kw)
    assert set(got) == {"cam_offsets", "offsets", "plain_total", "cam_total"} and got["cam_total"] == E
    np.testing.assert_array_equal(got["cam_offsets"].cpu().numpy(), exp["cam_offsets"])
    assert bool((only["cam_offsets"][M + 1:] == -1).all())
    only = {"cam_slots": torch.full((E + 2,), -1, dtype=torch.int32, device="cuda")}  # and cam_offsets = NULL
    with pytest.raises(pkg.SdmError) as e:  # out->capacity is 0 then: the kept points do not fit
        eng.extract_points_voxel_cameras(refs, rows, 0.02, out=only, **kw)
    assert e.value.code == EINVAL and e.value.cam_total == 0 and bool((only["cam_slots"] == -1).all())
    pinned = {"xyz": eng.host_alloc((cap, 3), np.float32), "multiplicity": eng.host_alloc((cap,), np.uint32),
              "source_index": eng.host_alloc((cap,), np.uint32), "representative": eng.host_alloc((T + 3,), np.uint32),
              "cam_offsets": eng.host_alloc((cap + 1,), np.int64), "cam_slots": eng.host_alloc((E + 7,), np.int32)}
    got = eng.extract_points_voxel_cameras(refs, rows, 0.02, out=pinned, representative=True, **kw)
    assert_same({k: np.array(v) for k, v in got.items()}, exp, "pinned")
    for a in pinned.values():
        eng.host_free(a)

    # the C call with `out` and `vox` naming nothing; cam_slots = NULL and cam_offsets = NULL in turn
    pb, vc = b.PointBuffers(), b.VoxelCameras()
    pb.capacity = M
    co, cs = np.full(M + 1, -7, np.int64), np.full(E, -7, np.int32)
    vc.cam_offsets = co.ctypes.data
    rc, offs = _raw(eng, b, refs, rows, 0.02, pb, None, vc)
    assert rc == 0 and vc.cam_total == E
    np.testing.assert_array_equal(co, exp["cam_offsets"])
    np.testing.assert_array_equal(offs, exp["offsets"])
    vc = b.VoxelCameras()
    vc.cam_slots, vc.cam_capacity = cs.ctypes.data, E  # exactly enough
    rc, _ = _raw(eng, b, refs, rows, 0.02, pb, b.VoxelBuffers(), vc)
    assert rc == 0 and vc.cam_total == E
    np.testing.assert_array_equal(cs, exp["cam_slots"])

    # cam_capacity = E - 1: EINVAL, the totals filled, both camera arrays untouched
    out = {"cam_offsets": np.full(M + 1, -7, np.int64), "cam_slots": np.full(E - 1, -7, np.int32)}
    with pytest.raises(pkg.SdmError) as e:
        eng.extract_points_voxel_cameras(refs, rows, 0.02, out=out, **kw)
    assert e.value.code == EINVAL and e.value.cam_total == E and e.value.plain_total == T
    np.testing.assert_array_equal(e.value.offsets, exp["offsets"])
    assert (out["cam_offsets"] == -7).all() and (out["cam_slots"] == -7).all()
    out = {"cam_offsets": np.full(M + 1, -7, np.int64), "cam_slots": np.full(E, -7, np.int32)}  # E exactly
    assert_same(eng.extract_points_voxel_cameras(refs, rows, 0.02, out=out, **kw),
                {f: exp[f] for f in ("cam_offsets", "cam_slots", "offsets", "plain_total", "cam_total", "multiplicity",
                                     "source_index")}, "exact cam_capacity")
    # the point capacities come first and keep their contract: nothing written, cam_total 0
    for m, t in ((M - 1, T), (M, T - 1)):
        out = {"xyz": np.full((m, 3), 7.0, np.float32), "representative": np.full(t, 0xABCD, np.uint32),
               "cam_offsets": np.full(m + 1, -7, np.int64), "cam_slots": np.full(E, -7, np.int32)}
        with pytest.raises(pkg.SdmError) as e:
            eng.extract_points_voxel_cameras(refs, rows, 0.02, out=out, representative=True, **kw)
        assert e.value.code == EINVAL and e.value.cam_total == 0 and e.value.plain_total == T
        np.testing.assert_array_equal(e.value.offsets, exp["offsets"])
        assert (out["xyz"] == 7.0).all() and (out["representative"] == 0xABCD).all()
        assert (out["cam_offsets"] == -7).all() and (out["cam_slots"] == -7).all()
    assert_same(eng.extract_points_voxel_cameras(refs, rows, 0.02, **kw), exp, "sized by the binding")


def test_no_plain_point(pkg, engines):
    """nothing passes the filter: every offset is 0, and the lists are the one entry cam_offsets[0] = 0, on the host and on
    the device; nothing else is written"""
    torch = pytest.importorskip("torch")
    g, eng = engines("plane_64x48_n7")
    refs, rows = [0, 1, 2], g["nbrs"][[0, 1, 2]]
    kw = dict(max_sigma=0.3, min_rho=1e30)
    host = {"xyz": np.full((4, 3), 7.0, np.float32), "cam_offsets": np.full(5, -7, np.int64), "cam_slots": np.full(9, -7, np.int32)}
    dev = {"xyz": torch.full((4, 3), 7.0, dtype=torch.float32, device="cuda"),
           "cam_offsets": torch.full((5,), -7, dtype=torch.int64, device="cuda"),
           "cam_slots": torch.full((9,), -7, dtype=torch.int32, device="cuda")}
    for what, out in (("host", host), ("device", dev)):
        got = eng.extract_points_voxel_cameras(refs, rows, 0.02, out=out, **kw)
        assert got["plain_total"] == 0 and got["cam_total"] == 0 and not np.asarray(got["offsets"]).any(), what
        co = out["cam_offsets"].cpu().numpy() if what == "device" else out["cam_offsets"]
        cs = out["cam_slots"].cpu().numpy() if what == "device" else out["cam_slots"]
        xyz = out["xyz"].cpu().numpy() if what == "device" else out["xyz"]
        assert co[0] == 0 and (co[1:] == -7).all() and (cs == -7).all() and (xyz == 7.0).all(), what


def test_binding_retries_once(pkg, engines, monkeypatch):
    """a cam_slots sized by the binding that turns out too small: the call is repeated once with the reported total"""
    g, eng = engines("plane_64x48_n7")
    refs = list(range(g["n_kf"]))
    exp, _ = reference(eng, refs, g["nbrs"], 0.02, fields=("xyz",), max_sigma=0.3)
    M, E = len(exp["source_index"]), int(exp["cam_total"])
    assert E > 1 + g["n"]
    calls = []
    real = eng.lib.sdm_extract_points_voxel_cameras
    monkeypatch.setattr(eng.lib, "sdm_extract_points_voxel_cameras", lambda *a: calls.append(1) or real(*a))
    monkeypatch.setattr(eng, "extract_bound", lambda *a, **k: 1)  # the binding sizes cam_slots to 1 + n_nbr entries
    out = {"xyz": np.empty((M, 3), np.float32), "multiplicity": np.empty(M, np.uint32), "source_index": np.empty(M, np.uint32)}
    got = eng.extract_points_voxel_cameras(refs, g["nbrs"], 0.02, out=out, max_sigma=0.3)
    assert len(calls) == 2
    assert_same(got, {f: exp[f] for f in got}, "retry")
    out["cam_slots"] = np.full(E - 1, -7, np.int32)  # the caller's own array is never replaced
    with pytest.raises(pkg.SdmError) as e:
        eng.extract_points_voxel_cameras(refs, g["nbrs"], 0.02, out=out, max_sigma=0.3)
    assert len(calls) == 3 and e.value.cam_total == E and (out["cam_slots"] == -7).all()


# 5b. every error of the two calls it composes, and its own; nothing is written
def test_errors(pkg, engines):
    torch = pytest.importorskip("torch")
    b = sys.modules[pkg.__name__ + ".binding"]
    g, eng = engines("plane_64x48_n7")
    rows = g["nbrs"][[0, 1]][:, :3]

    def fresh():
        return {"xyz": np.full((4096, 3), 7.0, np.float32), "representative": np.full(8192, 0xABCD, np.uint32),
                "cam_offsets": np.full(4097, -7, np.int64), "cam_slots": np.full(40000, -7, np.int32)}

    def untouched(out):
        return ((out["xyz"] == 7.0).all() and (out["representative"] == 0xABCD).all() and
                (out["cam_offsets"] == -7).all() and (out["cam_slots"] == -7).all())

    def refused(code, slots, nbrs, voxel, engine=eng, **kw):
        out = fresh()
        with pytest.raises(pkg.SdmError) as e:
            engine.extract_points_voxel_cameras(slots, nbrs, voxel, max_sigma=0.3, out=out, representative=True, **kw)
        assert e.value.code == code, (code, e.value)
        assert untouched(out) and e.value.cam_total == 0

    for voxel in (0.0, -0.02, float("nan"), float("inf"), 1e-45):  # sdm_extract_points_voxel's
        refused(EINVAL, [0, 1], rows, voxel)
    refused(EINVAL, [0, 1, 0], g["nbrs"][[0, 1, 0]][:, :3], 0.02)  # a repeated slot
    refused(EINVAL, [0, 99], rows, 0.02)                           # a slot out of range
    refused(EINVAL, [0, 1], rows, 0.02, source=2)
    refused(EINVAL, [0, 1], np.zeros((2, g["n"] + 1), np.int32), 0.02)  # sdm_extract_points_support's: n_nbr > max_neighbours
    refused(EINVAL, [0, 1], np.array([[1, 2, 99], [0, 2, 3]], np.int32), 0.02)  # a neighbour out of range
    refused(EINVAL, [0, 1], np.array([[1, 2, -1], [0, 2, 3]], np.int32), 0.02)
    eng.extract_points_voxel_cameras([0, 1], np.array([[1, 1, 1], [1, 0, 0]], np.int32), 0.02, max_sigma=0.3)  # accepted
    eng3 = pipeline(pkg, g, extra_slots=1)  # slot n_kf holds nothing
    refused(ESTATE, [0, 1], np.array([[1, 2, g["n_kf"]], [0, 2, 3]], np.int32), 0.02, engine=eng3)
    refused(ESTATE, [0, g["n_kf"]], rows, 0.02, engine=eng3)
    eng3.close()
    eng2 = pipeline(pkg, g, with_pointset=False)  # the merge reads the point-set plane
    refused(ESTATE, [0, 1], rows, 0.02, engine=eng2)
    eng2.close()

    # the C call: NULL nbr_slots, no camera pointer, a negative cam_capacity, misaligned device pointers
    pb, vb, vc = b.PointBuffers(), b.VoxelBuffers(), b.VoxelCameras()
    pb.capacity = 4096
    assert _raw(eng, b, [0, 1], rows, 0.02, pb, vb, vc)[0] == EINVAL  # neither cam_offsets nor cam_slots
    co = np.full(4097, -7, np.int64)
    vc.cam_offsets = co.ctypes.data
    assert _raw(eng, b, [0, 1], np.zeros((2, 0), np.int32), 0.02, pb, vb, vc)[0] == EINVAL  # n_nbr < 1
    sl, offs = (ctypes.c_int * 2)(0, 1), (ctypes.c_longlong * 3)()
    fn = eng.lib.sdm_extract_points_voxel_cameras
    assert fn(eng.ctx, 2, sl, 3, None, 1, 0.3, 1e-6, 0.02, ctypes.byref(pb), ctypes.byref(vb), ctypes.byref(vc), offs) == EINVAL
    assert fn(eng.ctx, 2, sl, 3, None, 1, 0.3, 1e-6, 0.02, ctypes.byref(pb), ctypes.byref(vb), None, offs) == EINVAL
    cs = np.full(64, -7, np.int32)
    vc.cam_slots, vc.cam_capacity = cs.ctypes.data, -1
    assert _raw(eng, b, [0, 1], rows, 0.02, pb, vb, vc)[0] == EINVAL
    assert (co == -7).all() and (cs == -7).all()
    buf = torch.full((16384,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    pb.on_device = 1
    for off_at, slots_at in ((4, 0), (0, 2)):  # cam_offsets not 8-byte, cam_slots not 4-byte aligned
        vc = b.VoxelCameras()
        vc.cam_offsets = buf.data_ptr() + off_at
        vc.cam_slots, vc.cam_capacity = buf.data_ptr() + 32768 + slots_at, 4096
        assert _raw(eng, b, [0, 1], rows, 0.02, pb, vb, vc)[0] == EINVAL
    vb.multiplicity = buf.data_ptr() + 2  # sdm_extract_points_voxel's own alignment check still holds
    vc = b.VoxelCameras()
    vc.cam_offsets = buf.data_ptr()
    assert _raw(eng, b, [0, 1], rows, 0.02, pb, vb, vc)[0] == EINVAL
    assert bool((buf == 0x5A5A5A5A).all())


# 6. determinism, no side effects, the staged table set, both forms of the OR pass
def test_determinism_side_effects_and_or_forms(pkg, gpu_ok, monkeypatch):
    g = gu.load("plane_160x120_n7")
    eng = pipeline(pkg, g)
    refs = list(range(g["n_kf"]))
    short = np.ascontiguousarray(g["nbrs"][:, :3])
    eng.enable_stats(True)
    before = _state(eng, refs)
    stats0 = eng.get_stats(reset=False)

    def call(rows, voxel=0.02):
        return eng.extract_points_voxel_cameras(refs, rows, voxel, max_sigma=0.3, fields=ALL, representative=True)

    def no_stagings(st):
        return {k: v for k, v in st.items() if k != "table_stagings"}

    def stagings():
        return eng.get_stats(reset=False)["table_stagings"]

    # table_stagings moves as for extract_points_support: once for a table no cached set holds, not at all otherwise
    other = np.ascontiguousarray(g["nbrs"][:, 1:4])
    s0 = stagings()
    eng.extract_points_support(refs, other, max_sigma=0.3, fields=())
    d_support = stagings() - s0
    a = call(short)
    st1 = eng.get_stats(reset=False)
    assert d_support == 1 and st1["table_stagings"] == s0 + 2 and no_stagings(st1) == no_stagings(stats0)
    call(other)  # the set extract_points_support staged serves this call
    assert stagings() == s0 + 2
    b2 = call(short)
    for f in a:
        assert np.asarray(a[f]).tobytes() == np.asarray(b2[f]).tobytes(), f
    assert eng.get_stats(reset=False) == st1
    for x, y in zip(before, _state(eng, refs)):
        np.testing.assert_array_equal(x, y)
    # one atomic per lane instead of one per run of equal rank: the same bytes
    for voxel in (0.02, 1000.0, 1e-4):
        comb = call(short, voxel)
        monkeypatch.setenv("SDM_VOXCAM_PLAIN_OR", "1")
        plain_form = call(short, voxel)
        monkeypatch.delenv("SDM_VOXCAM_PLAIN_OR")
        for f in comb:
            assert np.asarray(comb[f]).tobytes() == np.asarray(plain_form[f]).tobytes(), (voxel, f)
    # a much smaller call right after (the scratch of the larger one reused)
    run(eng, [3], short[[3]], 0.02, "after a larger call", max_sigma=0.3)
    # a following inter_check over the same lists reuses the set this call staged
    call(short)
    st2 = eng.get_stats(reset=False)
    eng.inter_check(refs, short)
    assert eng.get_stats(reset=False)["table_stagings"] == st2["table_stagings"]
    eng.close()
