"""GPU: sdm_extract_points_support / Engine.extract_points_support -- the per-point visibility words -- against
tests/support_np.py (PM.cc:659-765 in NumPy) over the fixtures' maps or the maps downloaded from the device.  Every
comparison is exact: integers or bit patterns."""
import ctypes

import numpy as np
import pytest

import golden_util as gu
import support_np as sn
from test_gpu_extract import ALL, EINVAL, ESTATE, _random_map, _state, assert_same

pytestmark = pytest.mark.gpu

U64 = np.uint64


def pipeline(pkg, g, extra_slots=0, max_neighbours=None):
    """test_gpu_extract.py's pipeline shape: upload, recon, inter_check, pointset(1)"""
    n_kf = g["n_kf"]
    eng = pkg.Engine(g["W"], g["H"], n_kf + extra_slots, max_neighbours=max_neighbours or g["n"])
    for k in range(n_kf):
        eng.upload_image(k, g["im"][k], g["K"], g["Tcw"][k])
    refs = list(range(n_kf))
    eng.search_fuse(refs, g["nbrs"], float(g["min_depth"]), float(g["max_depth"]), rot=gu.rots(g))
    eng.recon(refs, g["nbrs"], float(g["min_depth"]), float(g["max_depth"]), rot=gu.rots(g))
    eng.inter_check(refs, g["nbrs"])
    eng.pointset(refs, source=1)
    return eng


def at_pixels(plane, codes):
    codes = np.asarray(codes, np.int64)
    return plane[codes >> 16, codes & 0xffff]


def device_maps(eng, slots):
    return {s: eng.download_depth(s) for s in slots}


def expected_words(poses, K, H, W, maps, slot, row):
    """the restatement for `slot` with neighbour row `row` over maps = {slot: (rho, sigma)}, poses = {slot: Tcw}"""
    kfs = {s: sn.keyframe(K, poses[s], H, W) for s in set(row) | {slot}}
    return sn.inter_support(kfs[slot], maps[slot][0], [kfs[j] for j in row], [maps[j][0] for j in row],
                            [maps[j][1] for j in row])[1]


def check_words(got, slots, words_of):
    """got["support"] == words_of(i, slot) at the extracted pixels of every slot"""
    for i, s in enumerate(slots):
        a, b = got["offsets"][i], got["offsets"][i + 1]
        np.testing.assert_array_equal(got["support"][a:b], at_pixels(words_of(i, s), got["pixel"][a:b]),
                                      err_msg="slot %d (position %d)" % (s, i))


def plain(got):
    return {k: v for k, v in got.items() if k != "support"}


@pytest.fixture(scope="module")
def fixture_words():
    """the restatement over each fixture's own rho / sigma, computed once: {name: [words of keyframe k]}"""
    cache = {}

    def get(name):
        if name not in cache:
            g = gu.load(name)
            cache[name] = (g, [sn.fixture_support(g, k)[1] for k in range(g["n_kf"])])
        return cache[name]
    return get


@pytest.mark.parametrize("name", gu.fixture_names())
def test_golden_fixture_support(pkg, gpu_ok, fixture_words, name):
    g, words = fixture_words(name)
    eng = pipeline(pkg, g)
    refs = list(range(g["n_kf"]))
    for max_sigma in (0.3, 0.01):
        got = eng.extract_points_support(refs, g["nbrs"], max_sigma=max_sigma, fields=ALL)
        ref = eng.extract_points(refs, max_sigma=max_sigma, fields=ALL)
        assert_same(plain(got), {k: np.asarray(v) for k, v in ref.items()}, name)
        total = int(got["offsets"][-1])
        assert got["support"].dtype == U64 and got["support"].shape == (total,)
        check_words(got, refs, lambda i, s: words[s])
        pc = sn.popcount(got["support"])
        print(name, max_sigma, "points", total, "popcounts", sorted(set(pc.tolist())))
        assert (pc >= 3).all()  # source 1: the check kept these points, lambdaN = 3
        if max_sigma == 0.3:
            assert len(set(pc.tolist())) >= 2
        else:
            assert total == 0  # the synthetic scenes' sigmas lie above the reference's 0.01: an empty cloud, no failure
    eng.close()


def test_wave_and_slot_boundaries(pkg, gpu_ok, fixture_words):
    name = "strip_roll_160x120_n7"
    g, words = fixture_words(name)
    eng = pipeline(pkg, g)
    rng = np.random.default_rng(21)
    order = [int(s) for s in rng.permutation(g["n_kf"])]
    got = eng.extract_points_support(order, g["nbrs"][order], max_sigma=0.08, fields=("pixel",))
    counts = {s: int(got["offsets"][i + 1] - got["offsets"][i]) for i, s in enumerate(order)}
    assert [counts[k] for k in range(g["n_kf"])] == [147, 139, 117, 74, 33, 56, 75, 99]  # no multiple of 64, two below 64
    check_words(got, order, lambda i, s: words[s])
    # every slot gets its own permutation of its neighbour row: the bits follow it
    perms = [rng.permutation(g["n"]) for _ in order]
    rows = np.stack([g["nbrs"][s][p] for s, p in zip(order, perms)])
    got2 = eng.extract_points_support(order, rows, max_sigma=0.08, fields=("pixel",))
    np.testing.assert_array_equal(got2["pixel"], got["pixel"])
    np.testing.assert_array_equal(got2["offsets"], got["offsets"])
    changed = 0
    for i, (s, p) in enumerate(zip(order, perms)):
        a, b = got["offsets"][i], got["offsets"][i + 1]
        w = got["support"][a:b]
        exp = np.zeros(b - a, U64)
        for j in range(g["n"]):  # position j of the new row holds the neighbour of position p[j]
            exp |= ((w >> U64(p[j])) & U64(1)) << U64(j)
        np.testing.assert_array_equal(got2["support"][a:b], exp, err_msg="slot %d" % s)
        changed += int((exp != w).sum())
    assert changed > 0
    eng.close()


def test_bits_32_to_63(pkg, gpu_ok):
    g = gu.load("plane_96x80_n20")
    eng = pipeline(pkg, g, max_neighbours=40)
    refs = [0, 10, 20]
    rows = np.stack([np.concatenate([g["nbrs"][k], g["nbrs"][k]]) for k in refs])  # neighbour j again at j + 20
    got = eng.extract_points_support(refs, rows, max_sigma=0.3, fields=("pixel",))
    check_words(got, refs, lambda i, s: sn.fixture_support(g, s, nbr_row=rows[i])[1])
    w = got["support"]
    np.testing.assert_array_equal(w >> U64(20), w & U64(0xFFFFF))
    high = [int((w[got["offsets"][i]:got["offsets"][i + 1]] >> U64(32) != 0).sum()) for i in range(3)]
    print("points", np.diff(got["offsets"]).tolist(), "with a bit >= 32", high)
    assert np.diff(got["offsets"]).tolist() == [678, 821, 728] and high == [636, 821, 577]
    eng.close()


def _arbitrary_map(rng, H, W):
    """_random_map's style plus what a pipeline never produces: negative rho, sigma = 0, 1e-20 and 1e20 in both planes,
    non-zero values in the 2-px border"""
    rho, sigma = _random_map(rng, H, W, frac=0.5)
    sigma = (sigma * np.float32(20)).astype(np.float32)  # up to 0.4: neighbours agree and disagree
    for plane in (rho, sigma):
        for v in (1e-20, 1e20, 0.0):
            ys, xs = rng.integers(0, H, 40), rng.integers(0, W, 40)
            plane[ys, xs] = np.float32(v)
    ys, xs = rng.integers(0, H, 40), rng.integers(0, W, 40)
    rho[ys, xs] = np.float32(-0.5)
    rho[:2], rho[-2:], rho[:, :2], rho[:, -2:] = 0.7, 0.9, 1.1, 1.3
    sigma[:2], sigma[-2:], sigma[:, :2], sigma[:, -2:] = 0.005, 0.005, 0.005, 0.005
    return rho, sigma


def test_arbitrary_maps(pkg, gpu_ok):
    g = gu.load("plane_64x48_n7")
    n_kf, H, W = g["n_kf"], g["H"], g["W"]
    eng = pipeline(pkg, g, extra_slots=3)
    rng = np.random.default_rng(33)
    extra = [n_kf, n_kf + 1, n_kf + 2]
    poses = {k: g["Tcw"][k] for k in range(n_kf)}
    for i, s in enumerate(extra):  # the poses of keyframes 1, 3, 5, moved a little: projections land inside the neighbours
        T = g["Tcw"][2 * i + 1].copy()
        T[0, 3] += 0.01 * (i + 1)
        poses[s] = T
        eng.upload_image(s, g["im"][2 * i + 1], g["K"], T)
        eng.upload_depth(s, *_arbitrary_map(rng, H, W))
    eng.pointset(extra, source=0)
    maps = device_maps(eng, list(range(n_kf)) + extra)

    def run(slots, rows, **kw):
        got = eng.extract_points_support(slots, rows, fields=ALL, **kw)
        assert_same(plain(got), {k: np.asarray(v) for k, v in eng.extract_points(slots, fields=ALL, **kw).items()})
        check_words(got, slots, lambda i, s: expected_words(poses, g["K"], H, W, maps, s, list(rows[i])))
        return got

    # the arbitrary maps as references: a dense walk that keeps every pixel (min_rho < 0), neighbours of both kinds
    rows = [[0, extra[1], 2, extra[2]], [extra[0], 1, 3, extra[2]], [4, 5, extra[0], extra[1]]]
    got = run(extra, rows, source=0, max_sigma=float("inf"), min_rho=-1.0)
    assert int(got["offsets"][-1]) == 3 * H * W
    codes = got["pixel"].astype(np.int64)
    y, x = codes >> 16, codes & 0xffff
    border = (x < 2) | (x >= W - 2) | (y < 2) | (y >= H - 2)
    assert border.any() and not got["support"][border].any()  # border points carry 0, whatever their rho
    with np.errstate(invalid="ignore"):
        skipped = got["rho_sigma"][:, 0].astype(np.float64) < 0.000001
    assert skipped.any() and not got["support"][skipped].any()  # and so do the points PM.cc:662 skips
    assert got["support"][~border & ~skipped].any()
    # ... and as neighbours of pipeline slots, filter on the checked plane and on the depth map
    slots = [3, 0, 6]
    rows = [[extra[0], 2, extra[1], 4, extra[2]], [extra[2], extra[1], extra[0], 1, 2], [5, extra[0], 4, extra[2], 3]]
    for src in (1, 0):
        got = run(slots, rows, source=src, max_sigma=0.3)
        assert int(got["offsets"][-1]) > 0 and got["support"].any()
    # both kinds of reference in one call
    run([extra[1], 2, extra[0]], [[0, 1, extra[2]], [extra[0], 1, 3], [2, extra[1], 4]], source=0, max_sigma=0.3)
    eng.close()


def test_after_commit(pkg, gpu_ok):
    g = gu.load("plane_64x48_n7")
    eng = pipeline(pkg, g)
    refs = list(range(g["n_kf"]))
    committed = [2, 5]
    eng.inter_check(committed, g["nbrs"][committed], commit=True)
    maps = device_maps(eng, refs)
    for k in committed:  # the depth map now holds the checked rho
        np.testing.assert_array_equal(maps[k][0].view(np.uint32), eng.download_checked(k).view(np.uint32))
        assert (maps[k][0].view(np.uint32) != g["rho"][k].view(np.uint32)).any()
    poses = {k: g["Tcw"][k] for k in refs}
    slots = [5, 1, 2, 4]  # committed ones as references, and as neighbours of the others
    for src in (1, 0):
        got = eng.extract_points_support(slots, g["nbrs"][slots], source=src, max_sigma=0.3, fields=("pixel",))
        assert int(got["offsets"][-1]) > 0
        check_words(got, slots, lambda i, s: expected_words(poses, g["K"], g["H"], g["W"], maps, s, list(g["nbrs"][s])))
    eng.close()


def test_no_side_effects(pkg, gpu_ok):
    g = gu.load("plane_160x120_n7")
    eng = pipeline(pkg, g)
    refs = list(range(g["n_kf"]))
    before = _state(eng, refs)
    cloud0 = eng.extract_points(refs, max_sigma=0.3, fields=ALL)
    a = eng.extract_points_support(refs, g["nbrs"], max_sigma=0.3, fields=ALL)
    b = eng.extract_points_support(refs, g["nbrs"], max_sigma=0.3, fields=ALL)
    np.testing.assert_array_equal(a["support"], b["support"])
    assert_same(plain(a), {k: np.asarray(v) for k, v in plain(b).items()}, "repeat")
    for x, y in zip(before, _state(eng, refs)):
        np.testing.assert_array_equal(x, y)
    assert_same(eng.extract_points(refs, max_sigma=0.3, fields=ALL), {k: np.asarray(v) for k, v in cloud0.items()}, "cloud")
    eng.inter_check(refs, g["nbrs"])
    for x, y in zip(before, _state(eng, refs)):  # the check gives what it gave before
        np.testing.assert_array_equal(x, y)
    eng.close()


class _Misaligned:
    """an 8-byte-element device tensor view whose address is 4 bytes off (torch refuses to build one itself)"""

    def __init__(self, t):
        self.t = t
        self.is_cuda = True

    def is_contiguous(self):
        return True

    def element_size(self):
        return 8

    def get_device(self):
        return self.t.get_device()

    def data_ptr(self):
        return self.t.data_ptr()

    def numel(self):
        return self.t.numel() // 2


def test_destinations(pkg, gpu_ok):
    torch = pytest.importorskip("torch")
    g = gu.load("plane_96x80_n20")
    eng = pipeline(pkg, g)
    refs = [7, 1, 12, 0, 19, 3]
    rows = g["nbrs"][refs]
    ref = eng.extract_points_support(refs, rows, max_sigma=0.1, fields=ALL)  # pageable arrays sized by the binding
    total = int(ref["offsets"][-1])
    assert total > 0 and ref["support"].any()
    cap = total + 5
    # pageable, preallocated
    out = {"pixel": np.empty(cap, np.uint32), "support": np.full(cap, 0x5A5A, U64)}
    got = eng.extract_points_support(refs, rows, max_sigma=0.1, out=out)
    np.testing.assert_array_equal(got["support"], ref["support"])
    np.testing.assert_array_equal(got["pixel"], ref["pixel"])
    assert (out["support"][total:] == 0x5A5A).all()
    # pinned
    pinned = {"xyz": eng.host_alloc((cap, 3), np.float32), "pixel": eng.host_alloc((cap,), np.uint32),
              "rho_sigma": eng.host_alloc((cap, 2), np.float32), "intensity": eng.host_alloc((cap,), np.uint8),
              "support": eng.host_alloc((cap,), U64)}
    got = eng.extract_points_support(refs, rows, max_sigma=0.1, out=pinned)
    np.testing.assert_array_equal(np.array(got["support"]), ref["support"])
    assert_same({k: np.array(v) for k, v in plain(got).items()}, plain(ref), "pinned")
    for a in pinned.values():
        eng.host_free(a)
    # torch device tensors
    dev = {"xyz": torch.empty((cap, 3), dtype=torch.float32, device="cuda"),
           "pixel": torch.empty(cap, dtype=torch.int32, device="cuda"),
           "rho_sigma": torch.empty((cap, 2), dtype=torch.float32, device="cuda"),
           "intensity": torch.empty(cap, dtype=torch.uint8, device="cuda"),
           "support": torch.empty(cap, dtype=torch.int64, device="cuda")}
    got = eng.extract_points_support(refs, rows, max_sigma=0.1, out=dev)
    host = {f: t.cpu().numpy() for f, t in got.items() if f != "offsets"}
    host["pixel"] = host["pixel"].view(np.uint32)
    host["offsets"] = got["offsets"]
    np.testing.assert_array_equal(host.pop("support").view(U64), ref["support"])
    assert_same(host, plain(ref), "device")
    # support alone: no other field, on the host and on the device
    got = eng.extract_points_support(refs, rows, max_sigma=0.1, fields=())
    assert set(got) == {"support", "offsets"}
    np.testing.assert_array_equal(got["support"], ref["support"])
    np.testing.assert_array_equal(got["offsets"], ref["offsets"])
    alone = torch.zeros(cap, dtype=torch.int64, device="cuda")
    got = eng.extract_points_support(refs, rows, max_sigma=0.1, out={"support": alone})
    np.testing.assert_array_equal(got["support"].cpu().numpy().view(U64), ref["support"])
    # a device support array 4 bytes into a buffer: the 8-byte stores need 8-byte alignment
    buf = torch.empty(2 * cap + 1, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        eng.extract_points_support(refs, rows, max_sigma=0.1, out={"support": _Misaligned(buf[1:])})
    b = __import__("sys").modules[pkg.__name__ + ".binding"]
    pb = b.PointBuffers()
    pb.capacity = cap
    pb.on_device = 1
    offs = (ctypes.c_longlong * (len(refs) + 1))()
    sl = (ctypes.c_int * len(refs))(*refs)
    nb = np.ascontiguousarray(rows, np.int32)
    call = lambda ptr: eng.lib.sdm_extract_points_support(
        eng.ctx, len(refs), sl, nb.shape[1], nb.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 1, 0.1, 1e-6, ctypes.byref(pb),
        ctypes.cast(ptr, ctypes.POINTER(ctypes.c_ulonglong)), offs)
    assert buf[1:].data_ptr() % 8 == 4
    assert call(buf[1:].data_ptr()) == EINVAL
    assert call(buf.data_ptr()) == 0 and offs[len(refs)] == total
    np.testing.assert_array_equal(buf[:2 * total].cpu().numpy().view(U64), ref["support"])
    eng.close()


def test_refusals(pkg, gpu_ok):
    g = gu.load("plane_64x48_n7")
    n_kf = g["n_kf"]
    eng = pipeline(pkg, g, extra_slots=2)
    spare, never = n_kf, n_kf + 1
    eng.upload_image(spare, g["im"][0], g["K"], g["Tcw"][0])  # a keyframe without a depth map
    refs = [0, 1]
    rows = g["nbrs"][refs]

    def code(slots, rows, **kw):
        with pytest.raises(pkg.SdmError) as e:
            eng.extract_points_support(slots, rows, max_sigma=0.3, **kw)
        return e.value

    assert code(refs, np.zeros((2, 0), np.int32)).code == EINVAL               # n_nbr = 0
    assert code(refs, np.tile(rows, (1, 2))[:, :g["n"] + 1]).code == EINVAL    # n_nbr > max_neighbours
    for bad in (-1, n_kf + 2):                                                 # a neighbour slot out of range
        r = rows.copy()
        r[1, 3] = bad
        assert code(refs, r).code == EINVAL
    for bad in (spare, never):                                                 # a neighbour without a depth map
        r = rows.copy()
        r[0, 2] = bad
        assert code(refs, r).code == ESTATE
    assert code([0, 0], rows).code == EINVAL                                   # sdm_extract_points' own checks stay
    assert code([spare], rows[:1], source=0).code == ESTATE
    r = rows.copy()
    r[0, 1] = r[0, 0]                                                          # a repeated neighbour is accepted
    got = eng.extract_points_support(refs, r, max_sigma=0.3, fields=("pixel",))
    w0 = got["support"][:got["offsets"][1]]                                    # the points of refs[0], whose row repeats
    assert len(w0) > 0 and w0.any()
    np.testing.assert_array_equal((w0 >> U64(1)) & U64(1), w0 & U64(1))
    # NULL support, NULL neighbour table
    b = __import__("sys").modules[pkg.__name__ + ".binding"]
    pb = b.PointBuffers()
    pix = np.empty(g["W"] * g["H"] * 2, np.uint32)
    pb.pixel = pix.ctypes.data
    pb.capacity = pix.size
    offs = (ctypes.c_longlong * 3)()
    sl = (ctypes.c_int * 2)(*refs)
    nb = np.ascontiguousarray(rows, np.int32)
    nbp = nb.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    sup = np.empty(pix.size, U64)
    supp = sup.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong))
    f = eng.lib.sdm_extract_points_support
    assert f(eng.ctx, 2, sl, g["n"], nbp, 1, 0.3, 1e-6, ctypes.byref(pb), None, offs) == EINVAL
    assert f(eng.ctx, 2, sl, g["n"], None, 1, 0.3, 1e-6, ctypes.byref(pb), supp, offs) == EINVAL
    assert f(eng.ctx, 2, sl, g["n"], nbp, 1, 0.3, 1e-6, ctypes.byref(pb), supp, offs) == 0
    total = offs[2]
    assert total > 1
    # capacity one short: offsets filled, the sentinels stay
    out = {"pixel": np.full(total - 1, 0xABCD, np.uint32), "support": np.full(total - 1, 0xFEEDFACE, U64)}
    e = code(refs, rows, out=out)
    assert e.code == EINVAL
    assert list(e.offsets) == list(offs)
    assert (out["pixel"] == 0xABCD).all() and (out["support"] == 0xFEEDFACE).all()
    eng.close()
