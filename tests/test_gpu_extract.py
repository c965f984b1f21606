"""GPU: sdm_extract_points / Engine.extract_points against the host filter of the reference's writers (PM.cc:100-132)
applied to the downloaded planes -- bit for bit: floats compared as uint32, pixel codes and offsets equal."""
import ctypes

import numpy as np
import pytest

import golden_util as gu
from common import bits

pytestmark = pytest.mark.gpu

ALL = ("xyz", "pixel", "rho_sigma", "intensity")
EINVAL, ESTATE = 1, 4


def host_filter(rho, sigma, max_sigma=0.01, min_rho=1e-6):
    """(pixel codes, flat indices) of the pixels the host loops keep, raster order"""
    with np.errstate(invalid="ignore"):
        keep = ~(sigma.astype(np.float64) > max_sigma) & (rho.astype(np.float64) > min_rho)
    ys, xs = np.nonzero(keep)
    return ((ys.astype(np.uint32) << 16) | xs.astype(np.uint32)), ys * rho.shape[1] + xs


def expected(eng, slots, source=1, max_sigma=0.01, min_rho=1e-6, fields=ALL):
    """today's path: three downloads per keyframe and the filter on the host"""
    out = {f: [] for f in fields}
    offs = [0]
    for s in slots:
        r, sg = eng.download_depth(s)
        rho = eng.download_checked(s) if source else r
        code, flat = host_filter(rho, sg, max_sigma, min_rho)
        if "pixel" in fields:
            out["pixel"].append(code)
        if "rho_sigma" in fields:
            out["rho_sigma"].append(np.stack([rho.reshape(-1)[flat], sg.reshape(-1)[flat]], 1))
        if "xyz" in fields:
            out["xyz"].append(eng.download_pointset(s).reshape(-1, 3)[flat])
        if "intensity" in fields:
            out["intensity"].append(eng.download_inputs(s)[0].reshape(-1)[flat])
        offs.append(offs[-1] + len(code))
    shapes = {"xyz": (0, 3), "pixel": (0,), "rho_sigma": (0, 2), "intensity": (0,)}
    res = {f: np.concatenate(v) if v else np.zeros(shapes[f]) for f, v in out.items()}
    res["offsets"] = np.asarray(offs, np.int64)
    return res


def assert_same(got, exp, what=""):
    np.testing.assert_array_equal(np.asarray(got["offsets"]), exp["offsets"], err_msg=what + " offsets")
    for f in exp:
        if f == "offsets":
            continue
        g, e = np.asarray(got[f]), exp[f]
        assert g.shape == e.shape, (what, f, g.shape, e.shape)
        if f in ("xyz", "rho_sigma"):
            np.testing.assert_array_equal(bits(g), bits(e), err_msg="%s %s" % (what, f))
        else:
            np.testing.assert_array_equal(g.astype(np.int64), e.astype(np.int64), err_msg="%s %s" % (what, f))


def pipeline(pkg, g, extra_slots=0, **kw):
    """the fixture through upload_image -> recon -> inter_check -> pointset(1), as test_gpu_golden.py runs it"""
    n_kf = g["n_kf"]
    eng = pkg.Engine(g["W"], g["H"], n_kf + extra_slots, max_neighbours=g["n"], **kw)
    for k in range(n_kf):
        eng.upload_image(k, g["im"][k], g["K"], g["Tcw"][k])
    refs = list(range(n_kf))
    eng.search_fuse(refs, g["nbrs"], float(g["min_depth"]), float(g["max_depth"]), rot=gu.rots(g))
    eng.recon(refs, g["nbrs"], float(g["min_depth"]), float(g["max_depth"]), rot=gu.rots(g))
    eng.inter_check(refs, g["nbrs"])
    if kw.get("with_pointset", True):
        eng.pointset(refs, source=1)
    return eng


@pytest.mark.parametrize("name", gu.fixture_names())
def test_golden_fixture_cloud(pkg, gpu_ok, name):
    g = gu.load(name)
    eng = pipeline(pkg, g)
    refs = list(range(g["n_kf"]))
    # the synthetic scenes' sigmas lie mostly above the reference's 0.01: a wider gate as well, so that points pass
    for max_sigma in (0.01, 0.3):
        got = eng.extract_points(refs, max_sigma=max_sigma, fields=ALL)
        # pixel codes and rho / sigma: the filter over the fixture's own checked rho and sigma
        pos = 0
        for k in refs:
            code, flat = host_filter(g["chk"][k], g["sigma"][k], max_sigma)
            a, b = got["offsets"][k], got["offsets"][k + 1]
            assert a == pos and b - a == len(code), (name, k)
            np.testing.assert_array_equal(got["pixel"][a:b], code)
            np.testing.assert_array_equal(bits(got["rho_sigma"][a:b, 0]), bits(g["chk"][k].reshape(-1)[flat]))
            np.testing.assert_array_equal(bits(got["rho_sigma"][a:b, 1]), bits(g["sigma"][k].reshape(-1)[flat]))
            np.testing.assert_array_equal(bits(got["xyz"][a:b]), bits(eng.download_pointset(k).reshape(-1, 3)[flat]))
            np.testing.assert_array_equal(got["intensity"][a:b], g["im"][k].reshape(-1)[flat])
            pos = b
        assert pos > 0 or max_sigma == 0.01
        assert_same(got, expected(eng, refs, max_sigma=max_sigma), name)
    eng.close()


def _random_map(rng, H, W, frac=0.3):
    rho = np.where(rng.random((H, W)) < frac, rng.uniform(-0.2, 2.0, (H, W)), 0).astype(np.float32)
    sigma = np.where(rho != 0, rng.uniform(0, 0.02, (H, W)), 0).astype(np.float32)
    return rho, sigma


def test_list_dense_and_mixed_paths(pkg, gpu_ok):
    g = gu.load("plane_96x80_n20")
    n_kf = g["n_kf"]
    eng = pipeline(pkg, g, extra_slots=3)
    rng = np.random.default_rng(7)
    # dense slots: arbitrary maps (non-zero off the active lists) over uploaded keyframes, then their point sets
    dense = [n_kf, n_kf + 1, n_kf + 2]
    for i, s in enumerate(dense):
        eng.upload_image(s, g["im"][i], g["K"], g["Tcw"][i])
        eng.upload_depth(s, *_random_map(rng, g["H"], g["W"]))
    eng.pointset(dense, source=0)
    listed = [5, 0, 17, 3, 11]
    # list path, sources 1 and 0 (pipeline maps from recon)
    for src in (1, 0):
        for ms in (0.01, 0.1):
            got = eng.extract_points(listed, source=src, max_sigma=ms, fields=ALL)
            assert ms == 0.01 or got["offsets"][-1] > 0
            assert_same(got, expected(eng, listed, source=src, max_sigma=ms), "list src%d" % src)
    # dense path (source 0: checked planes of these slots do not exist yet)
    order = [dense[2], dense[0], dense[1]]
    assert_same(eng.extract_points(order, source=0, fields=ALL), expected(eng, order, source=0), "dense")
    # both kinds in one call, unsorted
    mixed = [dense[1], 9, dense[0], 2, 14]
    assert_same(eng.extract_points(mixed, source=0, fields=ALL), expected(eng, mixed, source=0), "mixed src0")
    # source 1 on the dense slots: the generic inter check writes arbitrary checked planes
    nb = [[j for j in range(n_kf) if j != i][:4] for i in range(3)]
    eng.inter_check(dense, nb)
    eng.pointset(dense, source=1)
    mixed = [19, dense[2], 4, dense[0], dense[1], 8]
    assert_same(eng.extract_points(mixed, source=1, fields=ALL), expected(eng, mixed, source=1), "mixed src1")
    # after a pose update the stored plane is copied as it stands (not recomputed)
    T = g["Tcw"][4].copy()
    T[0, 3] += 0.25
    eng.set_pose(4, T)
    assert_same(eng.extract_points([4, dense[0]], fields=("xyz", "pixel")),
                expected(eng, [4, dense[0]], fields=("xyz", "pixel")), "after set_pose")
    # every point-set plane value equals the download, non-default thresholds too
    assert_same(eng.extract_points(mixed, source=1, max_sigma=0.05, min_rho=0.5, fields=ALL),
                expected(eng, mixed, source=1, max_sigma=0.05, min_rho=0.5), "thresholds")
    # identical from run to run
    a = eng.extract_points(listed + dense, source=0, fields=ALL)
    b = eng.extract_points(listed + dense, source=0, fields=ALL)
    assert_same(a, {k: np.asarray(v) for k, v in b.items()}, "repeat")
    eng.close()


def test_predicate_edges(pkg, gpu_ok):
    W, H = 64, 16
    eng = pkg.Engine(W, H, 2, with_pointset=False)
    f = np.float32
    s01, r6 = f(0.01), f(1e-6)
    sig_vals = [s01, np.nextafter(s01, f(np.inf)), np.nextafter(s01, f(-np.inf)), f(np.nan), f(-0.0), f(0.0), f(0.05),
                np.nextafter(f(0.05), f(np.inf)), f(1e30), f(np.inf), f(-1.0), f(1e-45)]
    rho_vals = [r6, np.nextafter(r6, f(np.inf)), np.nextafter(r6, f(-np.inf)), f(np.nan), f(-0.0), f(0.0), f(1.0),
                f(np.inf), f(-np.inf), f(1e-45), f(2e-6)]
    S, R = np.meshgrid(np.array(sig_vals, f), np.array(rho_vals, f), indexing="ij")
    sigma = np.zeros((H, W), f)
    rho = np.zeros((H, W), f)
    sigma.reshape(-1)[:S.size] = S.reshape(-1)
    rho.reshape(-1)[:R.size] = R.reshape(-1)
    eng.upload_depth(0, rho, sigma)
    eng.upload_depth(1, rho[::-1].copy(), sigma[:, ::-1].copy())
    for ms in (0.01, 0.0, 1e30, 0.05, -0.0, float(np.float32(0.01)), float("inf"), float("nan")):
        for mr in (1e-6, 0.0, float(np.float32(1e-6)), -1.0, float("nan")):
            got = eng.extract_points([1, 0], source=0, max_sigma=ms, min_rho=mr, fields=("pixel", "rho_sigma"))
            assert_same(got, expected(eng, [1, 0], 0, ms, mr, ("pixel", "rho_sigma")), "max_sigma %r min_rho %r" % (ms, mr))
    eng.close()


def test_empty_keyframe_and_many_slots(pkg, gpu_ok):
    W, H, n = 160, 120, 300  # 10 tiles per dense slot: 3000 tiles, more than one scan workgroup covers
    eng = pkg.Engine(W, H, n, with_pointset=False)
    rng = np.random.default_rng(3)
    z = np.zeros((H, W), np.float32)
    for s in range(n):
        if s % 37 == 5:
            eng.upload_depth(s, z, z)  # an empty keyframe
        else:
            eng.upload_depth(s, *_random_map(rng, H, W, frac=0.05 + 0.5 * rng.random()))
    order = list(rng.permutation(n))
    got = eng.extract_points(order, source=0, fields=("pixel", "rho_sigma"))
    exp = expected(eng, order, 0, fields=("pixel", "rho_sigma"))
    assert_same(got, exp, "300 slots")
    empties = [i for i, s in enumerate(order) if s % 37 == 5]
    assert empties and all(exp["offsets"][i] == exp["offsets"][i + 1] for i in empties)
    one = eng.extract_points([5], source=0, fields=("pixel",))
    assert list(one["offsets"]) == [0, 0] and one["pixel"].size == 0
    eng.close()


def test_1080p_dense_second_scan_level(pkg, gpu_ok):
    W, H = 1920, 1080  # 1013 tiles per dense slot: three slots need a second scan workgroup
    eng = pkg.Engine(W, H, 3, with_pointset=False)
    rng = np.random.default_rng(11)
    for s in range(3):
        eng.upload_depth(s, *_random_map(rng, H, W, frac=0.4))
    order = [2, 0, 1]
    assert_same(eng.extract_points(order, source=0, fields=("pixel", "rho_sigma")),
                expected(eng, order, 0, fields=("pixel", "rho_sigma")), "1080p")
    eng.close()


def _state(eng, slots, with_chk=True):
    st = []
    for s in slots:
        r, sg = eng.download_depth(s)
        st += [bits(r), bits(sg), bits(eng.download_pointset(s)), eng.active_count(s)]
        if with_chk:
            st.append(bits(eng.download_checked(s)))
    return st


def test_capacity_state_and_no_side_effects(pkg, gpu_ok):
    g = gu.load("plane_160x120_n7")
    eng = pipeline(pkg, g, extra_slots=2)
    n_kf = g["n_kf"]
    refs = list(range(n_kf))
    eng.enable_stats(True)
    eng.enable_timing(True)
    eng.recon(refs, g["nbrs"], float(g["min_depth"]), float(g["max_depth"]))
    eng.inter_check(refs, g["nbrs"])
    eng.pointset(refs, source=1)
    before = _state(eng, refs)
    stats0, timing0 = eng.get_stats(reset=False), eng.get_timing(reset=False)
    ms = 0.3  # (the fixture's sigmas lie mostly above 0.01)
    exp = expected(eng, refs, max_sigma=ms)
    total = int(exp["offsets"][-1])
    assert total > 1
    # capacity one short: EINVAL, offsets filled, no point written
    out = {"xyz": np.full((total - 1, 3), 7.0, np.float32), "pixel": np.full(total - 1, 0xABCD, np.uint32)}
    with pytest.raises(pkg.SdmError) as e:
        eng.extract_points(refs, max_sigma=ms, out=out)
    assert e.value.code == EINVAL
    np.testing.assert_array_equal(e.value.offsets, exp["offsets"])
    assert (out["xyz"] == 7.0).all() and (out["pixel"] == 0xABCD).all()
    # exactly enough
    out = {"xyz": np.empty((total, 3), np.float32), "pixel": np.empty(total, np.uint32)}
    assert_same(eng.extract_points(refs, max_sigma=ms, out=out), {k: exp[k] for k in ("xyz", "pixel", "offsets")}, "exact capacity")
    # nothing changed: planes, lists, counters, stage timing
    assert eng.get_stats(reset=False) == stats0
    assert eng.get_timing(reset=False) == timing0
    after = _state(eng, refs)
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)
    # argument and state errors
    spare, spare2 = n_kf, n_kf + 1
    eng.upload_image(spare, g["im"][0], g["K"], g["Tcw"][0])
    for slots, src, code in (([0, 0], 1, EINVAL), ([-1], 1, EINVAL), ([n_kf + 2], 1, EINVAL),
                             ([0, spare2], 1, ESTATE), ([spare], 0, ESTATE)):
        with pytest.raises(pkg.SdmError) as e:
            eng.extract_points(slots, source=src)
        assert e.value.code == code, (slots, src)
    eng.upload_depth(spare, *_random_map(np.random.default_rng(1), g["H"], g["W"]))
    with pytest.raises(pkg.SdmError) as e:
        eng.extract_points([spare], source=1)  # never inter-keyframe checked
    assert e.value.code == ESTATE
    eng.extract_points([spare], source=0)
    b = __import__("sys").modules[pkg.__name__ + ".binding"]
    pb = b.PointBuffers()
    pb.capacity = 10
    offs = (ctypes.c_longlong * 2)()
    sl = (ctypes.c_int * 1)(0)
    assert eng.lib.sdm_extract_points(eng.ctx, 1, sl, 1, 0.01, 1e-6, ctypes.byref(pb), offs) == EINVAL  # no field
    assert eng.lib.sdm_extract_points(eng.ctx, 1, sl, 1, 0.01, 1e-6, None, offs) == EINVAL
    assert eng.lib.sdm_extract_points(eng.ctx, 1, sl, 1, 0.01, 1e-6, ctypes.byref(pb), None) == EINVAL
    eng.close()
    # xyz from a context without the point-set pool
    eng = pipeline(pkg, g, with_pointset=False)
    with pytest.raises(pkg.SdmError) as e:
        eng.extract_points([0], fields=("xyz",))
    assert e.value.code == ESTATE
    got = eng.extract_points([1, 0], max_sigma=ms, fields=("pixel", "rho_sigma"))
    assert int(got["offsets"][-1]) > 0
    eng.close()


def test_device_and_pinned_destinations(pkg, gpu_ok):
    torch = pytest.importorskip("torch")
    g = gu.load("plane_96x80_n20")
    eng = pipeline(pkg, g)
    refs = [7, 1, 12, 0, 19, 3]
    ref = eng.extract_points(refs, max_sigma=0.1, fields=ALL)
    total = int(ref["offsets"][-1])
    assert total > 0
    cap = total + 5
    dev = {"xyz": torch.empty((cap, 3), dtype=torch.float32, device="cuda"),
           "pixel": torch.empty(cap, dtype=torch.int32, device="cuda"),
           "rho_sigma": torch.empty((cap, 2), dtype=torch.float32, device="cuda"),
           "intensity": torch.empty(cap, dtype=torch.uint8, device="cuda")}
    got = eng.extract_points(refs, max_sigma=0.1, out=dev)
    host = {f: t.cpu().numpy() for f, t in got.items() if f != "offsets"}
    host["pixel"] = host["pixel"].view(np.uint32)
    host["offsets"] = got["offsets"]
    assert_same(host, ref, "device")
    pinned = {"xyz": eng.host_alloc((cap, 3), np.float32), "pixel": eng.host_alloc((cap,), np.uint32),
              "rho_sigma": eng.host_alloc((cap, 2), np.float32), "intensity": eng.host_alloc((cap,), np.uint8)}
    got = eng.extract_points(refs, max_sigma=0.1, out=pinned)
    assert_same({k: np.array(v) for k, v in got.items()}, ref, "pinned")
    for a in pinned.values():
        eng.host_free(a)
    eng.close()


def test_negative_min_rho_on_list_slots(pkg, gpu_ok):
    # off-list pixels of pipeline maps hold rho = 0: with min_rho < 0 they pass, so these slots must be walked whole
    g = gu.load("plane_96x80_n20")
    eng = pipeline(pkg, g)
    slots = [6, 2, 13, 0]
    P = g["W"] * g["H"]
    for src in (1, 0):
        listed = sum(eng.active_count(s) for s in slots)
        assert eng.extract_bound(slots, src) == listed < len(slots) * P
        assert eng.extract_bound(slots, src, min_rho=-1.0) == len(slots) * P
        for mr, ms in ((-1.0, 0.01), (-1.0, float("nan")), (-1e-30, 0.3), (-0.0, 0.3), (0.0, 0.3)):
            got = eng.extract_points(slots, source=src, max_sigma=ms, min_rho=mr, fields=ALL)
            exp = expected(eng, slots, source=src, max_sigma=ms, min_rho=mr)
            assert_same(got, exp, "src %d min_rho %r max_sigma %r" % (src, mr, ms))
            if mr < 0:
                assert int(exp["offsets"][-1]) > listed  # off-list zeros among the points
    eng.close()


def test_list_walk_and_zero_item_slots(pkg, gpu_ok):
    g = gu.load("plane_64x48_n7")
    W, H = g["W"], g["H"]
    eng = pkg.Engine(W, H, 6)
    flat = np.full((H, W), 128, np.uint8)  # no gradient: an empty active list
    rng = np.random.default_rng(5)
    for s in range(6):
        eng.upload_image(s, flat if s % 2 == 0 else g["im"][s], g["K"], g["Tcw"][s])
    for s in (1, 3, 5):  # maps with values off the lists, then declared pipeline maps: the list walk must skip those
        eng.upload_depth(s, *_random_map(rng, H, W, frac=0.6))
    eng.assume_pipeline_maps(range(6))
    empties = [0, 2, 4]
    assert all(eng.active_count(s) == 0 for s in empties)
    assert all(eng.active_count(s) > 0 for s in (1, 3, 5))
    order = [0, 3, 2, 1, 5, 4]  # zero-item slots first, in the middle and last
    assert eng.extract_bound(order, 0) == sum(eng.active_count(s) for s in order)
    got = eng.extract_points(order, source=0, max_sigma=0.3, fields=ALL)
    full = expected(eng, order, source=0, max_sigma=0.3)
    # expected from the walk over the lists: the full filter's points that lie on the slot's list
    exp = {f: [] for f in ALL}
    offs = [0]
    for i, s in enumerate(order):
        a, b = full["offsets"][i], full["offsets"][i + 1]
        on = np.isin(full["pixel"][a:b], eng.active_list(s)[0])
        for f in ALL:
            exp[f].append(full[f][a:b][on])
        offs.append(offs[-1] + int(on.sum()))
    exp = {f: np.concatenate(v) for f, v in exp.items()}
    exp["offsets"] = np.asarray(offs, np.int64)
    assert int(full["offsets"][-1]) > offs[-1] > 0  # the maps pass off the lists too: the walk did skip them
    assert_same(got, exp, "list walk")
    # min_rho < 0: the same slots walked whole
    assert_same(eng.extract_points(order, source=0, max_sigma=0.3, min_rho=-1.0, fields=ALL),
                expected(eng, order, source=0, max_sigma=0.3, min_rho=-1.0), "whole walk")
    # only zero-item slots: no tile at all
    got = eng.extract_points([4, 0, 2], source=0, fields=("pixel", "xyz"))
    assert list(got["offsets"]) == [0, 0, 0, 0] and got["pixel"].size == 0 and got["xyz"].shape == (0, 3)
    assert eng.extract_bound([4, 0, 2], 0) == 0
    eng.close()


def test_device_destination_checks(pkg, gpu_ok):
    torch = pytest.importorskip("torch")
    g = gu.load("plane_64x48_n7")
    eng = pipeline(pkg, g)
    buf = torch.empty(4096 + 1, dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):  # a view 4 bytes into the buffer: float2 stores need 8-byte alignment
        eng.extract_points([0, 1], max_sigma=0.3, out={"rho_sigma": buf[1:]})
    b = __import__("sys").modules[pkg.__name__ + ".binding"]
    pb = b.PointBuffers()
    pb.rho_sigma = buf[1:].data_ptr()
    pb.capacity = 2048
    pb.on_device = 1
    offs = (ctypes.c_longlong * 3)()
    sl = (ctypes.c_int * 2)(0, 1)
    assert eng.lib.sdm_extract_points(eng.ctx, 2, sl, 1, 0.3, 1e-6, ctypes.byref(pb), offs) == EINVAL
    eng.close()
