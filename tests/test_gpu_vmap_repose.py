"""GPU: re-placing the persistent voxel map under new keyframe poses (sdm_vmap_repose / Engine.vmap_repose) against
tests/vmap_repose_np.py -- after every call the delta, remap, all four infos, a full fetch of the map, the log, all camera
lists, the evidence and the flags.  Everything is copied bits, an integer, or pointset_pixel's one float32 formula: every
comparison is for equality.  The synthetic inputs and what they cover are tests/test_vmap_repose_cpu.py's."""
import ctypes
import sys

import numpy as np
import pytest
import torch

import golden_util as gu
import vmap_import_np as vi
import vmap_repose_np as vr
from test_gpu_extract import EINVAL, ESTATE, pipeline
from test_gpu_vmap import same_fetch, same_info, snapshot, unchanged
from test_gpu_vmap_class import RULE, Mirror, centres_of, feed, full_state, same_flags, state_unchanged
from test_gpu_vmap_import import to_host
from test_gpu_vmap_obs import obs_snapshot, obs_unchanged, same_obs
from test_vmap_repose_cpu import K_CAM, POSE_A, SYN_M, SYN_POSES, TAG_B, VOXEL, pose, synthetic_records, synthetic_table

pytestmark = pytest.mark.gpu
F = np.float32
NOID = 0xFFFFFFFF
KW = dict(max_sigma=0.3)
LAX = dict(min_multiplicity=2)   # a rule an import-made map can pass: it looks at the multiplicity alone


@pytest.fixture(scope="module")
def engines(pkg, gpu_ok):
    """the golden fixtures run through the pipeline once each"""
    made = {}

    def get(name):
        if name not in made:
            g = gu.load(name)
            made[name] = (g, pipeline(pkg, g))
        return made[name]

    yield get
    for _, eng in made.values():
        eng.close()


def pad_evidence(ref):
    for f in ref.ev:  # entries created later start at 0
        ref.ev[f] = np.concatenate([ref.ev[f], np.zeros(ref.vm.M - len(ref.ev[f]), np.uint64)])


def import_both(eng, ref, rec, pairs=None):
    """records (and pairs) into the engine's map and the mirror"""
    exp = vi.import_records(ref.vm, rec)
    got = eng.vmap_import(rec, updated=False)
    np.testing.assert_array_equal(got["dst_ids"], exp["dst_ids"])
    pad_evidence(ref)
    if pairs is not None and len(pairs["entry"]):
        assert eng.vmap_import_observations(pairs["entry"], pairs["tag"]) == \
            vi.import_observations(ref.ol, ref.vm.M, pairs["entry"], pairs["tag"])
    return got


def classify_both(eng, ref, rule):
    exp = ref.classify(rule, True)
    got = eng.vmap_classify(rule, True, ids=False)
    assert got["published_total"] == exp["published_total"]
    return got


def same_state(eng, ref, what=""):
    """all four infos, a full fetch, the log, all camera lists, the evidence and the flags"""
    same_info(eng, ref.vm, what)
    same_fetch(eng.vmap_fetch(), ref.vm.fetch(), what)
    same_obs(eng, ref, what)
    pad_evidence(ref)
    ev = eng.vmap_fetch_evidence()
    for f in ref.ev:
        assert ev[f].dtype == np.uint64
        np.testing.assert_array_equal(ev[f][:ref.vm.M], ref.ev[f], err_msg="%s %s" % (what, f))
    same_flags(eng, ref, what)


def check_repose(eng, ref, tags, K, T, carry, mode, what=""):
    """one sdm_vmap_repose against the restatement.  mode: "host", "device" or "none" (the form of remap)"""
    M = ref.vm.M
    pad_evidence(ref)
    exp, ev2, fl2 = vr.repose(ref.vm, ref.ol, tags, K, T, carry, ref.ev, ref.cl.flags(M))
    ref.ev, ref.cl.published = ev2, fl2
    dest = {"host": True, "none": False}.get(mode)
    if mode == "device":
        dest = torch.full((M + 3,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    got = eng.vmap_repose(tags, K, T, carry=carry, remap=dest)
    assert {f: got[f] for f in vr.DELTA} == {f: exp[f] for f in vr.DELTA}, (what, got, {f: exp[f] for f in vr.DELTA})
    if mode == "none":
        assert "remap" not in got
    else:
        mine = to_host(got["remap"], np.uint32) if mode == "device" else got["remap"]
        assert mine.dtype == np.uint32 and len(mine) == M
        np.testing.assert_array_equal(mine, exp["remap"], err_msg=what + " remap")
        if mode == "device":
            assert (to_host(dest, np.uint32)[M:] == 0x5A5A5A5A).all(), what
    same_state(eng, ref, what)
    return got, exp


# 1. synthetic maps made with vmap_import: the wave and tile edges, the table sizes, the hostile entries, the three forms of
# remap and both carries.  No carve runs on an import-made map: its counters read 0 (the zero and identity cases); its
# flags come from a classify that looks at the multiplicity alone
@pytest.mark.parametrize("M", SYN_M)
def test_synthetic_maps(pkg, gpu_ok, M):
    eng = pkg.Engine(32, 24, 1)
    rec, pairs, hostile = synthetic_records(M)
    try:
        eng.vmap_open(VOXEL)
        seen = dict(merged=0, dropped=0, published=0, lost=0)
        first = True
        for n_poses in SYN_POSES:
            tags, K, T = synthetic_table(n_poses)
            for carry in (0, 1):
                for mode in ("host", "device", "none"):
                    if not first:
                        eng.vmap_clear()
                    first = False
                    ref = Mirror(VOXEL)
                    import_both(eng, ref, rec, pairs)
                    assert ref.vm.M == M
                    flagged = classify_both(eng, ref, LAX)["published_total"] if M else 0
                    what = "M %d poses %d carry %d remap %s" % (M, n_poses, carry, mode)
                    got, exp = check_repose(eng, ref, tags, K, T, carry, mode, what)
                    assert got["examined"] == M
                    if n_poses == 0:
                        assert got["voxels"] == M and got["moved"] == 0
                        if mode != "none":
                            assert (exp["remap"] == np.arange(M)).all()
                    pub = eng.vmap_class_info()["published"]
                    assert pub == 0 if not carry else pub <= flagged
                    seen["merged"] += got["merged"]
                    seen["dropped"] += got["dropped"]
                    seen["published"] += pub
                    seen["lost"] += got["observations_before"] - got["observations"]
        # the map still works: an import and a second repose on top
        import_both(eng, ref, {f: (v + F(500 * VOXEL) if f == "xyz" else v) for f, v in rec.items()})
        check_repose(eng, ref, [TAG_B], [K_CAM], [POSE_A], 1, "host", "M %d a second repose" % M)
        if M >= 63:
            assert min(seen.values()) > 0, seen
    finally:
        eng.close()


def perturbed(Tcw, k):
    """a pose a little off Tcw: a small rotation in front and a shifted translation"""
    T = np.asarray(Tcw, np.float64).reshape(3, 4)
    d = pose(0.004 * (k + 1), -0.003 * (k + 1)).reshape(3, 4).astype(np.float64)
    out = np.concatenate([d[:, :3] @ T[:, :3], (d[:, :3] @ T[:, 3] + np.array([0.01, -0.02, 0.015]) * (k + 1)).reshape(3, 1)], axis=1)
    return out.astype(F)


# 2. the anchor to the engine's own K5, on every golden fixture
@pytest.mark.parametrize("name", gu.fixture_names())
def test_golden_anchor(engines, name):
    g, eng = engines(name)
    n_kf, W = g["n_kf"], g["W"]
    refs = list(range(n_kf))
    rows = np.ascontiguousarray(g["nbrs"][:, :3])
    poses = {k: np.array(g["Tcw"][k], F) for k in refs}
    eng.vmap_open(0.02)
    try:
        ref = Mirror(0.02)
        for k in refs:  # integrate, observe and carve; the tag of keyframe k is k
            feed(eng, ref, [k], rows[[k]], centres_of(poses), **KW)
        classify_both(eng, ref, RULE)
        M = ref.vm.M
        before = eng.vmap_fetch()
        ev0 = {f: np.array(a) for f, a in eng.vmap_fetch_evidence().items()}
        fl0 = np.array(eng.vmap_fetch_published())
        assert M > 0 and ev0["crossings"].any() and fl0.any()
        # the identity: the uploaded poses re-place nothing
        Kt, Tt = np.tile(g["K"], (n_kf, 1)), np.array([poses[k] for k in refs], F).reshape(n_kf, 12)
        got, _ = check_repose(eng, ref, refs[::-1], Kt[::-1], Tt[::-1], 1, "host", name + " identity")
        assert (got["reposed"], got["moved"], got["dropped"], got["merged"], got["voxels"]) == (M, 0, 0, 0, M)
        assert (got["remap"] == np.arange(M)).all()
        same_fetch(eng.vmap_fetch(), before, name + " identity: a byte-identical fetch")
        same_fetch(eng.vmap_fetch_evidence(), ev0, name + " identity: the evidence")
        assert eng.vmap_fetch_published().tobytes() == fl0.tobytes()
        # three keyframes at perturbed poses: the engine's own pointset under sdm_set_pose is the anchor
        moved = [1, n_kf // 2, n_kf - 1]
        for k in moved:
            poses[k] = perturbed(poses[k], k)
            eng.set_pose(k, poses[k])
        eng.pointset(moved, source=1)
        planes = {k: np.asarray(eng.download_pointset(k), F).reshape(-1, 3) for k in moved}
        got, exp = check_repose(eng, ref, moved, np.tile(g["K"], (3, 1)), [poses[k] for k in moved], 1, "device", name + " perturbed")
        now = eng.vmap_fetch()
        sel = np.flatnonzero(np.isin(now["tag"], moved))
        assert 0 < got["moved"] <= got["reposed"] < M and len(sel) > 0
        px = now["pixel"][sel]
        at = (px >> 16).astype(np.int64) * W + (px & 0xffff)
        want = np.stack([planes[int(t)][a] for t, a in zip(now["tag"][sel], at)])
        assert now["xyz"][sel].tobytes() == want.tobytes(), name + ": xyz against the plane at (tag, pixel)"
        # carried: the counter sums over remap, and published is the OR
        remap = exp["remap"]
        surv = remap != NOID
        ev1 = eng.vmap_fetch_evidence()
        for f in ev0:
            assert int(ev1[f].sum()) == int(ev0[f][surv].sum()), f
        orr = np.zeros(got["voxels"], np.uint8)
        np.maximum.at(orr, remap[surv].astype(np.int64), fl0[surv])
        assert eng.vmap_fetch_published().tobytes() == orr.tobytes()
        assert eng.vmap_class_info()["published"] == int(orr.sum())
        print(name, {f: got[f] for f in vr.DELTA})
        # and once more without the carry: counters and flags restart
        poses[moved[0]] = perturbed(poses[moved[0]], 5)
        check_repose(eng, ref, [moved[0]], [g["K"]], [poses[moved[0]]], 0, "none", name + " carry 0")
        assert not eng.vmap_fetch_published().any() and eng.vmap_class_info()["published"] == 0
        assert not any(a.any() for a in eng.vmap_fetch_evidence().values())
    finally:
        eng.vmap_close()
        for k in refs:  # the shared engine gets its poses and planes back
            eng.set_pose(k, np.array(g["Tcw"][k], F))
        eng.pointset(refs, source=1)


# 3. composition, device against device: the same by hand with existing calls on a second engine
def test_composition_with_existing_calls(pkg, gpu_ok):
    A, B = pkg.Engine(32, 24, 1), pkg.Engine(32, 24, 1)
    rec, pairs, _ = synthetic_records(2049)
    tags, K, T = synthetic_table(37)
    try:
        for e in (A, B):
            e.vmap_open(VOXEL)
            e.vmap_import(rec)
            e.vmap_import_observations(pairs["entry"], pairs["tag"])
        got = A.vmap_repose(tags, K, T)
        full, log = B.vmap_fetch(), B.vmap_fetch_observations()
        full["xyz"], _ = vr.new_xyz(full, tags, K, T)   # xyz replaced on the host
        B.vmap_clear()
        d = B.vmap_import({f: full[f] for f in ("xyz", "pixel", "rho_sigma", "intensity", "tag", "multiplicity")})
        B.vmap_import_observations(log["entry"], log["tag"], d["dst_ids"])
        np.testing.assert_array_equal(got["remap"], d["dst_ids"])
        assert got["merged"] > 0 and got["dropped"] == d["dropped"] > 0 and got["voxels"] == d["created"]
        ia, ib = A.vmap_info(), B.vmap_info()
        assert {f: ia[f] for f in ia if f not in ("calls", "points", "dropped", "rehashes")} == \
            {f: ib[f] for f in ib if f not in ("calls", "points", "dropped", "rehashes")}
        same_fetch(A.vmap_fetch(), B.vmap_fetch(), "records", skip=("epoch",))
        same_fetch(A.vmap_fetch_observations(), B.vmap_fetch_observations(), "log")
        same_fetch(A.vmap_fetch_cameras(), B.vmap_fetch_cameras(), "camera lists")
        assert A.vmap_obs_info()["observations"] == B.vmap_obs_info()["observations"] == got["observations"]
    finally:
        A.close()
        B.close()


# 4. interleaving and growth: a seeded sequence of imports, integrates, observes, reposes, classifies and fetches; the table
# rehashes and the records grow both before and after a repose
def test_interleaving_and_growth(engines):
    name = "plane_64x48_n7"
    g, eng = engines(name)
    rng = np.random.default_rng(0x5E9)
    n_kf = g["n_kf"]
    refs = list(range(n_kf))
    rows = np.ascontiguousarray(g["nbrs"][:, :3])
    poses = {k: np.array(g["Tcw"][k], F) for k in refs}
    syn, syn_pairs, _ = synthetic_records(5000)
    vox_kw = dict(fields=("xyz", "pixel", "rho_sigma", "intensity"), **KW)
    eng.vmap_open(0.02)
    try:
        ref = Mirror(0.02)
        cut = [0]
        calls = dict(n=0, reposes=0)
        grown = []   # (rehashes, a repose has run) after every growing call

        def imp(count):
            a, b = cut[0], cut[0] + count
            cut[0] = b
            import_both(eng, ref, {f: v[a:b] for f, v in syn.items()})
            ent = rng.integers(0, ref.vm.M, count).astype(np.uint32)
            tg = rng.integers(0, 12, count).astype(np.int32)
            assert eng.vmap_import_observations(ent, tg) == vi.import_observations(ref.ol, ref.vm.M, ent, tg)
            grown.append((eng.vmap_info()["rehashes"], calls["reposes"]))
            calls["n"] += 2

        def kf(k):
            feed(eng, ref, [k], rows[[k]], centres_of(poses), **KW)
            grown.append((eng.vmap_info()["rehashes"], calls["reposes"]))
            calls["n"] += 3

        def rep(carry, mode, kfs=(), table=0):
            cloud0 = eng.extract_points_voxel(refs, 0.02, **vox_kw)
            tags, K, T = synthetic_table(table, seed=calls["n"])
            keep = ~np.isin(tags, list(kfs))
            tags, K, T = list(tags[keep]), list(K[keep]), list(T[keep])
            for k in kfs:
                tags.append(k)
                K.append(g["K"])
                T.append(perturbed(g["Tcw"][k], int(rng.integers(0, 4))).reshape(12))
            got, _ = check_repose(eng, ref, tags, K, T, carry, mode, "call %d" % calls["n"])
            same_fetch(eng.extract_points_voxel(refs, 0.02, **vox_kw), cloud0, "extract_points_voxel around call %d" % calls["n"])
            calls["n"] += 1
            calls["reposes"] += 1
            return got

        def cls():
            classify_both(eng, ref, RULE if calls["n"] % 2 else LAX)
            same_flags(eng, ref, "call %d" % calls["n"])
            calls["n"] += 1

        kf(0)
        imp(1200)            # the table rehashes and the records grow before the first repose
        kf(1)
        cls()
        r1 = rep(1, "host", kfs=(0, 1), table=2)
        same_state(eng, ref, "after the first repose")
        imp(1500)            # the table rehashes and the records grow after a repose
        kf(2)
        cls()
        r2 = rep(0, "device", kfs=(2,), table=37)
        kf(3)
        kf(4)
        imp(2300)
        cls()
        r3 = rep(1, "none", kfs=(0, 3, 4), table=37)
        r4 = rep(1, "host")   # an empty table right after
        kf(5)
        cls()
        same_state(eng, ref, "the end")
        assert calls["n"] >= 30 and r1["moved"] > 0 and r2["merged"] > 0 and r3["dropped"] > 0 and r4["moved"] == 0
        before = [h for h, r in grown if r == 0]
        after = [h for h, r in grown if r > 0]
        assert before[-1] > 0 and after[-1] > before[-1], grown   # a rehash before and a rehash after a repose
        info = eng.vmap_info()
        assert info["voxels"] > 2048 and info["calls"] == ref.vm.calls
    finally:
        eng.vmap_close()


# 5. refusals: every SDM_EINVAL and SDM_ESTATE case leaves a snapshot of the whole state unchanged
def test_refusals(pkg, engines):
    b = sys.modules[pkg.__name__ + ".binding"]
    g, eng = engines("plane_64x48_n7")
    lib, ctx = eng.lib, eng.ctx
    refs = list(range(g["n_kf"]))
    rows = np.ascontiguousarray(g["nbrs"][:, :3])
    tags = np.array([2, 0, 1], np.int32)
    K = np.ascontiguousarray(np.tile(g["K"], (3, 1)), F)
    T = np.ascontiguousarray(np.array([perturbed(g["Tcw"][k], 1) for k in (2, 0, 1)], F).reshape(3, 12))
    ip, fp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_float)

    def call(n=3, tg=tags, k=K, t=T, d=None, **kw):
        d = b.VmapReposeDelta() if d is None else d
        for f in b.VMAP_REPOSE_OUTS:
            setattr(d, f, 9)
        for f, v in kw.items():
            setattr(d, f, v)
        rc = lib.sdm_vmap_repose(ctx, n, None if tg is None else tg.ctypes.data_as(ip), None if k is None else k.ctypes.data_as(fp),
                                 None if t is None else t.ctypes.data_as(fp), ctypes.byref(d))
        return rc, d

    rc, d = call()
    assert rc == ESTATE and b"no open voxel map" in lib.sdm_last_error()
    assert [getattr(d, f) for f in b.VMAP_REPOSE_OUTS] == [0] * 8
    eng.vmap_open(0.02)
    try:
        ref = Mirror(0.02)
        for k in refs[:3]:
            feed(eng, ref, [k], rows[[k]], centres_of({j: g["Tcw"][j] for j in refs}), **KW)
        classify_both(eng, ref, RULE)
        snap, osnap, st = snapshot(eng), obs_snapshot(eng), full_state(eng)
        M = snap[0]["voxels"]
        guard = np.full(M + 8, 0x5A5A5A5A, np.uint32)

        def refused(res, word, what, examined=0):
            rc, d = res
            assert rc == EINVAL and word in lib.sdm_last_error(), (what, rc, lib.sdm_last_error())
            assert [getattr(d, f) for f in b.VMAP_REPOSE_OUTS] == [examined] + [0] * 7, what
            unchanged(eng, snap, what)
            obs_unchanged(eng, osnap, what)
            state_unchanged(eng, st, what)
            assert (guard == 0x5A5A5A5A).all(), what

        assert lib.sdm_vmap_repose(ctx, 3, tags.ctypes.data_as(ip), K.ctypes.data_as(fp), T.ctypes.data_as(fp), None) == EINVAL
        unchanged(eng, snap, "null delta")
        refused(call(-1, remap=guard.ctypes.data, remap_capacity=len(guard)), b"negative n_poses", "n_poses < 0")
        refused(call(tg=None), b"null pose table", "null tags")
        refused(call(k=None), b"null pose table", "null K")
        refused(call(t=None), b"null pose table", "null Tcw")
        refused(call(tg=np.array([2, -1, 1], np.int32)), b"tag outside", "a negative tag")
        refused(call(tg=np.array([2, 0, 2], np.int32)), b"listed twice", "a tag listed twice")
        refused(call(carry=2), b"carry", "carry 2")
        refused(call(carry=-1), b"carry", "carry -1")
        refused(call(remap=guard.ctypes.data, remap_capacity=M - 1), b"remap_capacity", "a small remap", examined=M)
        dev = torch.full((M + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        refused(call(remap=dev.data_ptr() + 2, remap_capacity=M, on_device=1), b"not aligned", "a misaligned device remap")
        assert (to_host(dev, np.uint32) == 0x5A5A5A5A).all()
        with pytest.raises(ValueError):
            eng.vmap_repose([1, 2], K, T)
        with pytest.raises(pkg.SdmError) as err:
            eng.vmap_repose(tags, K, T, remap=np.zeros(M - 1, np.uint32))
        assert err.value.examined == M
        state_unchanged(eng, st, "binding refusals")
        # the map still works
        check_repose(eng, ref, tags, K, T, 1, "host", "after the refusals")
    finally:
        eng.vmap_close()
