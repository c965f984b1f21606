"""GPU: sdm_extract_points_voxel_freespace / Engine.extract_points_voxel_freespace.  Every output the call shares with
extract_points_voxel_cameras is compared byte for byte with that call for the same arguments; crossings and the three
totals are compared with tests/carve_np.py fed the engine's own lists, kept points and the uploaded poses.  Everything is
integer or compared as bits: there are no tolerances."""
import ctypes
import sys

import numpy as np
import pytest

import carve_np
import golden_util as gu
from test_gpu_extract import ALL, EINVAL, _state, pipeline

pytestmark = pytest.mark.gpu

NEW = ("crossings", "rays_total", "rays_skipped", "cells_visited")


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


def centres_of(poses):
    return {int(s): carve_np.camera_centre(T) for s, T in poses.items()}


def same_bytes(got, exp, what=""):
    """the outputs of extract_points_voxel_cameras, byte for byte"""
    for f, e in exp.items():
        g = got[f]
        if hasattr(g, "cpu"):
            g, e = g.cpu().numpy(), e.cpu().numpy() if hasattr(e, "cpu") else e
        assert np.asarray(g).shape == np.asarray(e).shape, (what, f)
        assert np.asarray(g).tobytes() == np.asarray(e).tobytes(), (what, f)


def check_new(got, exp, centres, voxel, end_margin, max_steps, what=""):
    """crossings and the totals against carve_np over the lists and points `exp` holds"""
    ref = carve_np.freespace(exp["xyz"], exp["cam_offsets"], exp["cam_slots"], centres, voxel, end_margin, max_steps)
    cr = got["crossings"]
    cr = cr.cpu().numpy().view(np.uint32) if hasattr(cr, "cpu") else np.asarray(cr)
    assert cr.dtype == np.uint32 and cr.shape == ref["crossings"].shape, what
    np.testing.assert_array_equal(cr, ref["crossings"], err_msg=what)
    assert (got["rays_total"], got["rays_skipped"], got["cells_visited"]) == \
        (ref["rays_total"], ref["rays_skipped"], ref["cells_visited"]), what
    assert got["rays_total"] == exp["cam_total"]
    return ref


def run(eng, slots, rows, voxel, centres, end_margin=1, max_steps=4096, what="", exp=None, **kw):
    if exp is None:
        exp = eng.extract_points_voxel_cameras(slots, rows, voxel, fields=ALL, representative=True, **kw)
    got = eng.extract_points_voxel_freespace(slots, rows, voxel, end_margin, max_steps, fields=ALL, representative=True, **kw)
    assert set(got) == set(exp) | set(NEW)
    what = "%s voxel %r margin %d max_steps %d" % (what, voxel, end_margin, max_steps)
    same_bytes(got, exp, what)
    return got, exp, check_new(got, exp, centres, voxel, end_margin, max_steps, what)


# 1. the golden fixtures: short and full rows, both sources, three voxel sizes, three margins, a max_steps that skips
@pytest.mark.parametrize("name", gu.fixture_names())
def test_golden_fixtures(engines, name):
    g, eng = engines(name)
    refs = list(range(g["n_kf"]))
    centres = centres_of({k: g["Tcw"][k] for k in refs})
    for rows, short in ((np.ascontiguousarray(g["nbrs"][:, :3]), True), (g["nbrs"], False)):
        for src in (1, 0):
            what = "%s src %d short %d" % (name, src, short)
            kw = dict(source=src, max_sigma=0.3)
            crossed, exp = {}, None
            # (the reference walk is the slow part: the full rows, with several times the rays, take one margin per source)
            for margin in (0, 1, 2) if short else (1,):
                got, exp, ref = run(eng, refs, rows, 0.02, centres, margin, 4096, what, exp=exp, **kw)
                assert got["rays_skipped"] == 0
                crossed[margin] = int((got["crossings"] > 0).sum())
            if short or src == 1:
                _, _, ref = run(eng, refs, rows, 0.02, centres, 1, 80, what, exp=exp, **kw)
                assert 0 < ref["rays_skipped"] < ref["rays_total"]  # a share of the rays is longer than 80 steps
            if short and src == 1:
                print("%s: E %d, crossed at margin 0 / 1 / 2: %s, %d rays longer than 80 steps" %
                      (name, got["rays_total"], crossed, ref["rays_skipped"]))
                assert crossed[0] >= 100 and crossed[0] > crossed[1] > crossed[2]
            run(eng, refs, rows, 0.05, centres, 1, 4096, what, **kw)
            if short:  # walks of 300 to 400 steps: two keyframes keep the reference walk short
                run(eng, refs[:2], rows[:2], 0.005, centres, 1, 4096, what, **kw)


CRAFTED_O = {0: (10.5, 10.5, 10.25), 1: (6.5, 10.5, 8.5), 2: (10.5, 10.5, 10.5), 3: (10.5, 10.5, 9.25)}


def _crafted_engine(pkg, W=64, H=48):
    """K = (1, 1, 2, 2), identity rotations and rho with an exact reciprocal Z: pixel (x, y) of slot s becomes the point
    O_s + (Z (x - 2), Z (y - 2), Z) with O_s = -t_s.  Voxel 1.  The point-set pass leaves the 2-pixel border at (0, 0, 0):
    the border pixels of all four slots merge into the one voxel at the origin, which all four cameras then look at.
      slot 0: Z = 0.5 from (10.5, 10.5, 10.25): a sheet inside the camera's own layer of cells -- pixel (2, 2) lies in the
              camera's cell (N = 0, and every other ray of the camera counts it at s = 0: all lanes on one counter);
              N = floor((x - 1) / 2) + floor((y - 1) / 2) grows along the row, 0 to 52: very unequal walks in one wave
      slot 1: Z = 2 from (6.5, 10.5, 8.5): d = (2 (x - 2), 2 (y - 2), 2): pixel (3, 3) is an exact three-axis tie, (3, 2) a
              two-axis tie, (2, 2) axis-parallel; its sheet lies in slot 0's layer of cells, so the two merge and camera 1
              looks at slot 0's points from below
      slot 2: Z = 2^19 from (10.5, 10.5, 10.5): x <= 3 and y <= 3 stay mergeable but 2^19 steps away; the rest is unmergeable
      slot 3: Z = 0.5 from (10.5, 10.5, 9.25), below slot 0's sheet; half the map empty
    sigma grows with the slot, so the earlier slot wins every merge"""
    eng = pkg.Engine(W, H, 5, max_neighbours=3)
    rng = np.random.default_rng(W)
    im = rng.integers(0, 256, (H, W)).astype(np.uint8)
    K = np.array([1, 1, 2, 2], np.float32)
    O = CRAFTED_O
    Z = {0: 0.5, 1: 2.0, 2: 2.0 ** 19, 3: 0.5}
    poses = {}
    for s in range(4):
        T = np.eye(4, dtype=np.float32)[:3].copy()
        T[:, 3] = -np.array(O[s], np.float32)
        poses[s] = T
        eng.upload_image(s, im, K, T)
        rho = np.full((H, W), 1.0 / Z[s], np.float32)
        if s == 3:
            rho[:, W // 2:] = 0
        eng.upload_depth(s, rho, rng.uniform(0.001 + 0.002 * s, 0.002 + 0.002 * s, (H, W)).astype(np.float32))
    eng.pointset([0, 1, 2, 3], source=0)
    return eng, poses


# 2. crafted maps: ties, axis-parallel rays, N = 0, N = max_steps and max_steps + 1, unmergeable points, one hot counter,
# unequal walks in one wave, a pose change, an out-of-range camera
def test_crafted_maps(pkg, gpu_ok):
    eng, poses = _crafted_engine(pkg)
    slots, rows = [0, 1, 2, 3], np.array([[1, 3, 2], [0, 3, 2], [0, 1, 3], [0, 1, 2]], np.int32)
    kw = dict(source=0)
    centres = centres_of(poses)
    for c, o in CRAFTED_O.items():
        assert centres[c].tolist() == list(o)  # the centres sit where the docstring says
    got, exp, ref = run(eng, slots, rows, 1.0, centres, 0, 4096, "crafted", **kw)
    M = len(got["crossings"])
    xyz, co, cs = exp["xyz"], exp["cam_offsets"], exp["cam_slots"]
    k_of = np.repeat(np.arange(M), np.diff(co))
    steps = ref["steps"]
    assert (xyz[0] == 0).all() and cs[co[0]:co[1]].tolist() == [0, 1, 2, 3]  # the border pixels, seen by every camera
    home = np.flatnonzero((xyz == np.array([10.5, 10.5, 10.75], np.float32)).all(axis=1))  # pixel (2, 2) of slot 0
    assert len(home) == 1 and steps[co[home[0]]] == 0 and cs[co[home[0]]] == 0  # N = 0: it lies in its camera's cell
    own0 = (cs == 0) & (steps > 0)
    assert got["crossings"][home[0]] >= own0.sum() > 500  # every other ray of camera 0 starts in that voxel
    wave0, slot0 = steps[:64], steps[:co[exp["offsets"][1]]]  # the first wave's rays; the rays of slot 0's kept points
    assert wave0.max() - wave0.min() >= 10 and slot0.max() - slot0.min() >= 45 and len(slot0) > 512
    far = np.abs(xyz).max(axis=1) >= 2.0 ** 20  # unmergeable: every ray to them is skipped, nothing counts them
    assert far.sum() > 1000 and (got["crossings"][far] == 0).all() and (steps[far[k_of]] < 0).all()
    near2 = (np.abs(xyz[:, 2] - (10.5 + 2.0 ** 19)) < 1) & ~far
    assert near2.any() and (steps[near2[k_of] & (cs == 2)] < 0).all()  # mergeable, 2^19 steps away: skipped by max_steps
    for pixel, n_steps in (((3, 3), 6), ((3, 2), 4), ((2, 2), 2)):  # d = (2, 2, 2), (2, 0, 2), (0, 0, 2) from camera 1
        at = np.array([6.5 + 2 * (pixel[0] - 2), 10.5 + 2 * (pixel[1] - 2), 10.5], np.float32)
        tie = np.flatnonzero((xyz == at).all(axis=1))
        assert len(tie) == 1 and steps[(k_of == tie[0]) & (cs == 1)].tolist() == [n_steps], pixel
    assert got["rays_skipped"] > 0 and got["crossings"].max() > 500
    # N = max_steps walks, N = max_steps + 1 does not
    for limit in (16, 17):
        _, _, r = run(eng, slots, rows, 1.0, centres, 1, limit, "crafted", exp=exp, **kw)
        assert (steps == limit).any() and (steps == limit + 1).any()
        assert (r["steps"][steps == limit] == limit).all() and (r["steps"][steps == limit + 1] == -1).all()
    run(eng, slots, rows, 1.0, centres, 2, 65536, "crafted", exp=exp, **kw)
    run(eng, slots, rows, 1.0, centres, 60, 4096, "crafted", exp=exp, **kw)  # end_margin >= N for every ray of slot 0
    run(eng, slots, rows, 0.25, centres, 1, 4096, "crafted", **kw)
    run(eng, [3, 0], rows[[3, 0]], 1.0, centres, 1, 4096, "crafted two slots", **kw)

    # 3. a pose change moves the centres: the planes stay, the result follows the new pose
    before = eng.extract_points_voxel_freespace([0, 3], rows[[0, 3]], 1.0, 0, 4096, fields=ALL, **kw)
    moved = dict(poses)
    moved[0] = poses[0].copy()
    moved[0][:, 3] = [-10.5, -30.5, -10.25]  # O_0 = (10.5, 30.5, 10.25)
    eng.set_pose(0, moved[0])
    got, exp, _ = run(eng, [0, 3], rows[[0, 3]], 1.0, centres_of(moved), 0, 4096, "moved", **kw)
    assert got["xyz"].tobytes() == before["xyz"].tobytes()
    assert got["crossings"].tobytes() != before["crossings"].tobytes()
    # an out-of-range centre: that camera's rays are skipped, the others are walked
    for t in ((-3e6, 0, 0), (0, 0, 2e6)):
        moved[0][:, 3] = t
        eng.set_pose(0, moved[0])
        got, exp, ref = run(eng, [0, 3], rows[[0, 3]], 1.0, centres_of(moved), 0, 4096, "pose %r" % (t,), **kw)
        assert got["rays_skipped"] >= int((exp["cam_slots"] == 0).sum()) > 0
        assert got["rays_skipped"] < got["rays_total"]
    eng.close()


def _raw(eng, b, slots, rows, voxel, pb, vb, vc, fs, max_sigma=0.3, source=1):
    """the C call itself -> (rc, offsets)"""
    sl = (ctypes.c_int * len(slots))(*slots)
    flat = [int(v) for v in np.asarray(rows).reshape(-1)]
    nb = (ctypes.c_int * max(len(flat), 1))(*flat)
    offs = (ctypes.c_longlong * (len(slots) + 1))()
    rc = eng.lib.sdm_extract_points_voxel_freespace(eng.ctx, len(slots), sl, np.asarray(rows).shape[1], nb, source, max_sigma,
                                                    1e-6, voxel, ctypes.byref(pb), ctypes.byref(vb) if vb is not None else None,
                                                    ctypes.byref(vc), ctypes.byref(fs) if fs is not None else None, offs)
    return rc, np.array(offs[:], np.int64)


# 4. destinations, capacities, refusals
def test_destinations_capacity_and_refusals(pkg, engines):
    torch = pytest.importorskip("torch")
    b = sys.modules[pkg.__name__ + ".binding"]
    g, eng = engines("plane_96x80_n20")
    refs = [7, 1, 12, 0, 19, 3]
    rows = np.ascontiguousarray(g["nbrs"][refs][:, :3])
    centres = centres_of({k: g["Tcw"][k] for k in range(g["n_kf"])})
    kw = dict(max_sigma=0.3)
    got, exp, ref = run(eng, refs, rows, 0.02, centres, 1, 4096, "pageable", **kw)
    T, M, E = int(exp["plain_total"]), len(exp["source_index"]), int(exp["cam_total"])
    assert 1 < M < T and E > M and ref["crossings"].any()
    cap = M + 5
    dev = {"xyz": torch.empty((cap, 3), dtype=torch.float32, device="cuda"),
           "pixel": torch.empty(cap, dtype=torch.int32, device="cuda"),
           "rho_sigma": torch.empty((cap, 2), dtype=torch.float32, device="cuda"),
           "intensity": torch.empty(cap, dtype=torch.uint8, device="cuda"),
           "multiplicity": torch.empty(cap, dtype=torch.int32, device="cuda"),
           "source_index": torch.empty(cap, dtype=torch.int32, device="cuda"),
           "representative": torch.empty(T + 3, dtype=torch.int32, device="cuda"),
           "cam_offsets": torch.empty(cap + 1, dtype=torch.int64, device="cuda"),
           "cam_slots": torch.empty(E + 7, dtype=torch.int32, device="cuda"),
           "crossings": torch.full((cap,), -1, dtype=torch.int32, device="cuda")}
    d = eng.extract_points_voxel_freespace(refs, rows, 0.02, 1, 4096, out=dev, representative=True, **kw)
    same_bytes(d, exp, "device")
    check_new(d, exp, centres, 0.02, 1, 4096, "device")
    assert bool((dev["crossings"][M:] == -1).all())
    # on the device with nothing but crossings: the kept points and the lists stay in engine scratch
    only = {"crossings": torch.full((cap,), -1, dtype=torch.int32, device="cuda")}
    d = eng.extract_points_voxel_freespace(refs, rows, 0.02, 1, 4096, out=only, **kw)
    assert set(d) == {"crossings", "offsets", "plain_total", "cam_total"} | set(NEW[1:])
    check_new(d, exp, centres, 0.02, 1, 4096, "device, crossings only")
    assert bool((only["crossings"][M:] == -1).all())
    # one of the two lists on the device, the other in scratch
    for f, size in (("cam_offsets", cap + 1), ("cam_slots", E)):
        part = {"crossings": torch.empty(cap, dtype=torch.int32, device="cuda"),
                f: torch.empty(size, dtype=torch.int64 if f == "cam_offsets" else torch.int32, device="cuda")}
        d = eng.extract_points_voxel_freespace(refs, rows, 0.02, 1, 4096, out=part, **kw)
        check_new(d, exp, centres, 0.02, 1, 4096, "device, " + f)
        assert d[f].cpu().numpy().tobytes() == exp[f].tobytes()
    pinned = {"xyz": eng.host_alloc((cap, 3), np.float32), "crossings": eng.host_alloc((cap,), np.uint32),
              "cam_offsets": eng.host_alloc((cap + 1,), np.int64), "cam_slots": eng.host_alloc((E + 7,), np.int32)}
    d = eng.extract_points_voxel_freespace(refs, rows, 0.02, 1, 4096, out=pinned, **kw)
    same_bytes(d, {f: exp[f] for f in ("xyz", "cam_offsets", "cam_slots", "offsets", "multiplicity", "source_index")}, "pinned")
    check_new({k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in d.items()}, exp, centres, 0.02, 1, 4096, "pinned")
    for a in pinned.values():
        eng.host_free(a)

    # the C call: `out` and `vox` naming nothing, both pointers of `cams` NULL (cam_capacity ignored)
    def structs(capacity=M, margin=1, steps=4096, fill=0xABCD):
        pb, vc, fs = b.PointBuffers(), b.VoxelCameras(), b.VoxelFreespace()
        pb.capacity, vc.cam_capacity = capacity, -3
        cr = np.full(max(capacity, 1), fill, np.uint32)
        fs.crossings, fs.end_margin, fs.max_steps = cr.ctypes.data, margin, steps
        fs.rays_total, fs.rays_skipped, fs.cells_visited = 5, 6, 7
        return pb, vc, fs, cr

    pb, vc, fs, cr = structs()
    rc, offs = _raw(eng, b, refs, rows, 0.02, pb, None, vc, fs)
    assert rc == 0 and vc.cam_total == E
    np.testing.assert_array_equal(offs, exp["offsets"])
    np.testing.assert_array_equal(cr, ref["crossings"])
    assert (fs.rays_total, fs.rays_skipped, fs.cells_visited) == (E, ref["rays_skipped"], ref["cells_visited"])
    # M - 1 points of capacity: sdm_extract_points_voxel's refusal, its contract kept, crossings untouched, totals 0
    pb, vc, fs, cr = structs(capacity=M - 1)
    vb = b.VoxelBuffers()
    rc, offs = _raw(eng, b, refs, rows, 0.02, pb, vb, vc, fs)
    assert rc == EINVAL and vc.cam_total == 0 and vb.plain_total == T and (cr == 0xABCD).all()
    np.testing.assert_array_equal(offs, exp["offsets"])
    assert (fs.rays_total, fs.rays_skipped, fs.cells_visited) == (0, 0, 0)
    # E - 1 entries of cam_capacity: sdm_extract_points_voxel_cameras' refusal; E exactly passes
    for entries in (E - 1, E):
        pb, vc, fs, cr = structs()
        slots_out = np.full(E, -7, np.int32)
        vc.cam_slots, vc.cam_capacity = slots_out.ctypes.data, entries
        rc, offs = _raw(eng, b, refs, rows, 0.02, pb, None, vc, fs)
        assert vc.cam_total == E
        np.testing.assert_array_equal(offs, exp["offsets"])
        if entries < E:
            assert rc == EINVAL and (cr == 0xABCD).all() and (slots_out == -7).all()
            assert (fs.rays_total, fs.rays_skipped, fs.cells_visited) == (0, 0, 0)
        else:
            assert rc == 0 and fs.rays_total == E
            np.testing.assert_array_equal(cr, ref["crossings"])
            np.testing.assert_array_equal(slots_out, exp["cam_slots"])
    with pytest.raises(pkg.SdmError) as e:  # through the binding: the caller's arrays keep their content
        out = {"xyz": np.full((M - 1, 3), 7.0, np.float32), "crossings": np.full(M - 1, 9, np.uint32)}
        eng.extract_points_voxel_freespace(refs, rows, 0.02, out=out, **kw)
    assert e.value.code == EINVAL and e.value.plain_total == T and e.value.cam_total == 0
    assert (out["xyz"] == 7.0).all() and (out["crossings"] == 9).all()
    # every new SDM_EINVAL, on a live context; nothing is written
    for change in ("fs", "crossings", "margin", "steps0", "steps+", "align"):
        pb, vc, fs, cr = structs(margin=-1 if change == "margin" else 1,
                                 steps={"steps0": 0, "steps+": 65537}.get(change, 4096))
        buf = None
        if change == "crossings":
            fs.crossings = None
        if change == "align":
            buf = torch.full((cap + 1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            pb.on_device, fs.crossings = 1, buf.data_ptr() + 2
        rc, _ = _raw(eng, b, refs, rows, 0.02, pb, None, vc, None if change == "fs" else fs)
        assert rc == EINVAL and vc.cam_total == 0, change
        assert (fs.rays_total, fs.rays_skipped, fs.cells_visited) == ((5, 6, 7) if change == "fs" else (0, 0, 0)), change
        assert (cr == 0xABCD).all() and (buf is None or bool((buf == 0x5A5A5A5A).all()))
    pb, vc, fs, cr = structs(steps=65536, margin=0)  # the limits themselves are accepted
    assert _raw(eng, b, refs, rows, 0.02, pb, None, vc, fs)[0] == 0
    for bad in (dict(end_margin=-1), dict(max_steps=0), dict(max_steps=65537)):
        with pytest.raises(pkg.SdmError) as e:
            eng.extract_points_voxel_freespace(refs, rows, 0.02, **bad, **kw)
        assert e.value.code == EINVAL
    with pytest.raises(ValueError):  # a device destination needs its crossings tensor
        eng.extract_points_voxel_freespace(refs, rows, 0.02, out={"xyz": dev["xyz"]}, **kw)


# 5. determinism, no side effects, a smaller call after a larger one
def test_determinism_and_side_effects(pkg, gpu_ok):
    g = gu.load("strip_roll_160x120_n7")
    eng = pipeline(pkg, g)
    refs = list(range(g["n_kf"]))
    short = np.ascontiguousarray(g["nbrs"][:, :3])
    centres = centres_of({k: g["Tcw"][k] for k in refs})
    eng.enable_stats(True)
    cams = eng.extract_points_voxel_cameras(refs, short, 0.02, max_sigma=0.3, fields=ALL, representative=True)
    before = _state(eng, refs)
    stats0 = eng.get_stats(reset=False)

    def call():
        return eng.extract_points_voxel_freespace(refs, short, 0.02, 1, 4096, max_sigma=0.3, fields=ALL, representative=True)

    a = call()
    b2 = call()
    for f in a:
        assert np.asarray(a[f]).tobytes() == np.asarray(b2[f]).tobytes(), f
    assert eng.get_stats(reset=False) == stats0  # (the table set extract_points_voxel_cameras staged serves the call)
    for x, y in zip(before, _state(eng, refs)):
        np.testing.assert_array_equal(x, y)
    same_bytes(a, cams, "after")
    assert int((a["crossings"] > 0).sum()) >= 100  # the strip's occluding edges
    run(eng, [3], short[[3]], 0.02, centres, 1, 4096, "after a larger call", max_sigma=0.3)
    again = eng.extract_points_voxel_cameras(refs, short, 0.02, max_sigma=0.3, fields=ALL, representative=True)
    same_bytes(again, cams, "extract_points_voxel_cameras after the new call")
    eng.close()
