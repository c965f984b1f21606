"""GPU: retiring keyframes from the persistent voxel map (sdm_vmap_retire / Engine.vmap_retire) against
tests/vmap_retire_np.py -- after every call the delta, remap and the three lists, all four infos, a full fetch of the map,
the log, all camera lists, the evidence and the flags.  Everything is copied bits or an integer: every comparison is for
equality.  The synthetic inputs and what they cover are tests/test_vmap_retire_cpu.py's."""
import ctypes
import sys

import numpy as np
import pytest
import torch

import golden_util as gu
import vmap_import_np as vi
import vmap_retire_np as vt
from test_gpu_extract import EINVAL, ESTATE, pipeline
from test_gpu_vmap import same_fetch, snapshot, unchanged
from test_gpu_vmap_class import RULE, Mirror, centres_of, feed, full_state, same_flags, state_unchanged
from test_gpu_vmap_import import to_host
from test_gpu_vmap_obs import obs_snapshot, obs_unchanged
from test_gpu_vmap_repose import KW, LAX, classify_both, check_repose, import_both, pad_evidence, same_state
from test_vmap_repose_cpu import K_CAM, POSE_A, SYN_M, TAG_B, VOXEL, synthetic_records
from test_vmap_retire_cpu import SYN_R, synthetic_tags

pytestmark = pytest.mark.gpu
F = np.float32
NOID = 0xFFFFFFFF
GUARD = 0x5A
LIST_DT = {"remap": np.uint32, "dropped_ids": np.uint32, "dropped_published": np.uint8, "removed_entry": np.uint32,
           "removed_tag": np.int32}
COUNT_OF = {"remap": "examined", "dropped_ids": "dropped", "dropped_published": "dropped", "removed_entry": "removed",
            "removed_tag": "removed"}


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


def device_lists(exp):
    """one guarded device tensor per list, three elements longer than the count it has to hold"""
    out = {}
    for f, dt in LIST_DT.items():
        n = exp[COUNT_OF[f]] + 3
        if dt == np.uint8:
            out[f] = torch.full((n,), GUARD, dtype=torch.uint8, device="cuda")
        else:
            out[f] = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    return out


def check_retire(eng, ref, tags, mode, carry, form="host", commit=True, what=""):
    """one sdm_vmap_retire against the restatement.  form: "host", "device" or "none" (the form of the four lists and remap)"""
    M = ref.vm.M
    pad_evidence(ref)
    flags = ref.cl.flags(M)
    before = full_state(eng) if not commit else None
    exp, ev2, fl2 = vt.retire(ref.vm, ref.ol, tags, mode, bool(carry), ref.ev, flags, commit)
    if commit:
        ref.ev, ref.cl.published = ev2, fl2
    kw = dict(remap=True, dropped=True, removed=True)
    dev = None
    if form == "none":
        kw = dict(remap=False, dropped=False, removed=False)
    elif form == "device":
        dev = device_lists(exp)
        kw = dict(remap=dev["remap"], dropped={f: dev[f] for f in ("dropped_ids", "dropped_published")},
                  removed={f: dev[f] for f in ("removed_entry", "removed_tag")})
    got = eng.vmap_retire(tags, mode=mode, carry=bool(carry), commit=commit, **kw)
    assert {f: got[f] for f in vt.DELTA} == {f: exp[f] for f in vt.DELTA}, (what, got, {f: exp[f] for f in vt.DELTA})
    for f, dt in LIST_DT.items():
        if form == "none":
            assert f not in got, (what, f)
            continue
        mine = to_host(got[f], dt) if form == "device" else got[f]
        assert mine.dtype == dt and len(mine) == exp[COUNT_OF[f]], (what, f, mine.dtype, len(mine))
        np.testing.assert_array_equal(mine, exp[f], err_msg="%s %s" % (what, f))
        if form == "device":   # nothing beyond the count is written
            tail = to_host(dev[f], dt)[exp[COUNT_OF[f]]:]
            assert len(tail) == 3 and tail.tobytes() == bytes([GUARD]) * tail.nbytes, (what, f)
    if not commit:
        state_unchanged(eng, before, what + " commit 0")
    same_state(eng, ref, what)
    return got, exp


def rebuilt(eng, rec, pairs, M, first):
    """the synthetic map again, in the engine and in a new mirror, with the flags of the multiplicity-only rule"""
    if not first:
        eng.vmap_clear()
    ref = Mirror(VOXEL)
    import_both(eng, ref, rec, pairs)
    assert ref.vm.M == M
    if M:
        classify_both(eng, ref, LAX)
    return ref


# 1. synthetic maps made with vmap_import: the wave and scan-tile edges, the four R, both modes, the three forms of the
# lists, both carries and commit = 0.  No carve runs on an import-made map: its counters read 0; its flags come from a
# classify that looks at the multiplicity alone
@pytest.mark.parametrize("M", SYN_M)
def test_synthetic_maps(pkg, gpu_ok, M):
    eng = pkg.Engine(32, 24, 1)
    rec, pairs, _ = synthetic_records(M)
    try:
        eng.vmap_open(VOXEL)
        seen = dict(dropped=0, dropped_published=0, orphaned=0, removed=0, vanished=0, published=0)
        first, turn = True, 0
        for n_tags in SYN_R:
            tags = synthetic_tags(n_tags)
            for mode in ("winner", "unobserved"):
                runs = [("host", True)] + ([("device", True), ("none", True), ("host", False)] if n_tags == 37 else [])
                for form, commit in runs:
                    ref = rebuilt(eng, rec, pairs, M, first)
                    first = False
                    carry = turn % 2
                    turn += 1
                    what = "M %d tags %d %s carry %d lists %s commit %d" % (M, n_tags, mode, carry, form, commit)
                    got, exp = check_retire(eng, ref, tags, mode, carry, form, commit, what)
                    if not commit:   # nothing has changed (checked in check_retire); the committing call gives the same outs
                        again, _ = check_retire(eng, ref, tags, mode, carry, form, True, what + ", then commit")
                        assert {f: again[f] for f in vt.DELTA} == {f: got[f] for f in vt.DELTA}, what
                        for f in LIST_DT:
                            np.testing.assert_array_equal(again[f], got[f], err_msg=what + " " + f)
                    assert got["examined"] == M
                    if n_tags == 37 and mode == "winner" and form == "host" and M >= 63:
                        # (more than the binding's first guess for the arrays it makes: it sized them and called again)
                        assert got["removed"] > got["observations_before"] // 4
                    if n_tags == 0 and mode == "winner" and form == "host":
                        assert got["voxels"] == M and (got["remap"] == np.arange(M)).all()
                    pub = eng.vmap_class_info()["published"]
                    assert pub == (got["published_total"] if carry else 0)
                    seen["dropped"] += got["dropped"]
                    seen["dropped_published"] += got["dropped_were_published"]
                    seen["orphaned"] += got["orphaned"]
                    seen["removed"] += got["removed"]
                    seen["vanished"] += got["observations_before"] - got["observations"] - got["removed"]
                    seen["published"] += pub
        # the map still works: an import, a second retire and a repose on top
        ref = rebuilt(eng, rec, pairs, M, False)
        check_retire(eng, ref, synthetic_tags(1), "winner", 1, "host", True, "M %d before the import" % M)
        import_both(eng, ref, {f: (v + F(500 * VOXEL) if f == "xyz" else v) for f, v in rec.items()}, pairs)
        check_retire(eng, ref, synthetic_tags(37), "unobserved", 1, "host", True, "M %d a second retire" % M)
        check_repose(eng, ref, [TAG_B], [K_CAM], [POSE_A], 1, "host", "M %d a repose after the retires" % M)
        if M >= 63:
            assert min(seen.values()) > 0, seen
    finally:
        eng.close()


# 2. the golden anchor: blocks of keyframes through pipeline, integrate, observe, carve and classify; one keyframe
# retired; a further block on top: the table and the set are usable after the rebuild, and new pairs append after the
# compacted log
@pytest.mark.parametrize("mode", ("winner", "unobserved"))
@pytest.mark.parametrize("name", gu.fixture_names())
def test_golden_anchor(engines, name, mode):
    g, eng = engines(name)
    n_kf = g["n_kf"]
    refs = list(range(n_kf))
    rows = np.ascontiguousarray(g["nbrs"][:, :3])
    centres = centres_of({k: np.array(g["Tcw"][k], F) for k in refs})
    last = refs[-max(1, n_kf // 4):]
    head = refs[:len(refs) - len(last)]
    blocks = [head[i::3] for i in range(3)]
    eng.vmap_open(0.02)
    try:
        ref = Mirror(0.02)
        for blk in blocks:   # the tag of keyframe k is k
            feed(eng, ref, blk, rows[blk], centres, **KW)
            classify_both(eng, ref, RULE)
        M, E = ref.vm.M, ref.ol.E
        assert M > 0 and E >= M and ref.cl.flags(M).any() and ref.ev["crossings"].any()
        carry = 1 if mode == "winner" else 0
        got, exp = check_retire(eng, ref, [1], mode, carry, "host", True, "%s %s" % (name, mode))
        assert got["dropped"] < M and got["removed"] > 0 and got["observations"] < E
        assert got["dropped"] > 0 or mode == "unobserved"   # (a neighbour may have seen every voxel of keyframe 1)
        assert (got["orphaned"] > 0) == (mode == "unobserved")
        print(name, mode, {f: got[f] for f in vt.DELTA})
        E2 = got["observations"]
        feed(eng, ref, last, rows[last], centres, **KW)
        classify_both(eng, ref, RULE)
        same_state(eng, ref, "%s %s: a further block" % (name, mode))
        assert ref.ol.E > E2 and ref.vm.M > got["voxels"]
        log = eng.vmap_fetch_observations()
        assert len(log["entry"]) == ref.ol.E and np.isin(log["tag"][E2:], last + rows[last].reshape(-1).tolist()).all()
    finally:
        eng.vmap_close()


# 3. composition, device against device: the same by hand with existing calls on a second engine
@pytest.mark.parametrize("mode", ("winner", "unobserved"))
def test_composition_with_existing_calls(pkg, gpu_ok, mode):
    A, B = pkg.Engine(32, 24, 1), pkg.Engine(32, 24, 1)
    rec, pairs, _ = synthetic_records(2049)
    tags = synthetic_tags(37)
    try:
        for e in (A, B):
            e.vmap_open(VOXEL)
            e.vmap_import(rec)
            e.vmap_import_observations(pairs["entry"], pairs["tag"])
        got = A.vmap_retire(tags, mode=mode)
        full, log = B.vmap_fetch(), B.vmap_fetch_observations()
        p = vt.plan(full["tag"], log["entry"], log["tag"], tags, mode)   # the filter in NumPy
        surv = p["remap"] != NOID
        B.vmap_clear()
        d = B.vmap_import({f: full[f][surv] for f in ("xyz", "pixel", "rho_sigma", "intensity", "tag", "multiplicity")})
        emap = np.full(len(surv), NOID, np.uint32)
        emap[surv] = d["dst_ids"]
        B.vmap_import_observations(log["entry"][p["keep"]], log["tag"][p["keep"]], emap)
        np.testing.assert_array_equal(got["remap"], emap)
        assert got["dropped"] > 0 and got["removed"] > 0 and got["voxels"] == d["created"]
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


# 4. interleaving and growth: a seeded sequence of imports, integrates, observes, carves, retires, classifies and fetches;
# the table rehashes and the records grow both before and after a retire
def test_interleaving_and_growth(engines):
    name = "plane_64x48_n7"
    g, eng = engines(name)
    rng = np.random.default_rng(0x7E71)
    n_kf = g["n_kf"]
    refs = list(range(n_kf))
    rows = np.ascontiguousarray(g["nbrs"][:, :3])
    centres = centres_of({k: np.array(g["Tcw"][k], F) for k in refs})
    syn, _, _ = synthetic_records(9000)
    vox_kw = dict(fields=("xyz", "pixel", "rho_sigma", "intensity"), **KW)
    eng.vmap_open(0.02)
    try:
        ref = Mirror(0.02)
        cut = [0]
        calls = dict(n=0, retires=0)
        grown = []   # (rehashes, a retire has run) after every growing call

        def imp(count):
            a, b = cut[0], cut[0] + count
            cut[0] = b
            import_both(eng, ref, {f: v[a:b] for f, v in syn.items()})
            ent = rng.integers(0, ref.vm.M, count).astype(np.uint32)
            tg = rng.integers(0, 12, count).astype(np.int32)
            assert eng.vmap_import_observations(ent, tg) == vi.import_observations(ref.ol, ref.vm.M, ent, tg)
            grown.append((eng.vmap_info()["rehashes"], calls["retires"]))
            calls["n"] += 2

        def kf(k):
            feed(eng, ref, [k], rows[[k]], centres, **KW)
            grown.append((eng.vmap_info()["rehashes"], calls["retires"]))
            calls["n"] += 3

        def ret(tags, mode, carry, form, commit=True):
            cloud0 = eng.extract_points_voxel(refs, 0.02, **vox_kw)
            got, _ = check_retire(eng, ref, tags, mode, carry, form, commit, "call %d" % calls["n"])
            same_fetch(eng.extract_points_voxel(refs, 0.02, **vox_kw), cloud0, "extract_points_voxel around call %d" % calls["n"])
            calls["n"] += 1
            calls["retires"] += 1 if commit else 0
            return got

        def cls():
            classify_both(eng, ref, RULE if calls["n"] % 2 else LAX)
            same_flags(eng, ref, "call %d" % calls["n"])
            calls["n"] += 1

        kf(0)
        imp(1200)            # the table rehashes and the records grow before the first retire
        kf(1)
        cls()
        r1 = ret([0, 25, 3], "winner", 1, "host")
        imp(2500)
        kf(2)
        cls()
        r2 = ret([1, 2, 5, 30, 31], "unobserved", 0, "device")
        kf(3)
        kf(0)                # a retired tag comes back: no memory of R
        imp(5300)            # past the largest M before the first retire: the table rehashes and the records grow again
        cls()
        r0 = ret([3, 7, 40], "winner", 1, "host", commit=False)
        r3 = ret([3, 7, 40], "winner", 1, "none")
        r4 = ret([], "winner", 1, "host")   # the empty R right after
        kf(4)
        cls()
        same_state(eng, ref, "the end")
        assert calls["n"] >= 30 and r1["dropped"] > 0 and r1["removed"] > 0 and r2["orphaned"] > 0 and r3["dropped"] == r0["dropped"] > 0
        assert r4["dropped"] == 0 and r4["voxels"] == r4["examined"]
        before = [h for h, r in grown if r == 0]
        after = [h for h, r in grown if r > 0]
        assert before[-1] > 0 and after[-1] > before[-1], grown   # a rehash before and a rehash after a retire
        info = eng.vmap_info()
        assert info["voxels"] > 0 and info["calls"] == ref.vm.calls
    finally:
        eng.vmap_close()


# 5. refusals: every SDM_EINVAL and SDM_ESTATE case leaves a snapshot of the whole state unchanged
def test_refusals(pkg, engines):
    b = sys.modules[pkg.__name__ + ".binding"]
    g, eng = engines("plane_64x48_n7")
    lib, ctx = eng.lib, eng.ctx
    refs = list(range(g["n_kf"]))
    rows = np.ascontiguousarray(g["nbrs"][:, :3])
    tags = np.array([2, 0], np.int32)
    ip = ctypes.POINTER(ctypes.c_int)

    def call(n=2, tg=tags, commit=1, **kw):
        d = b.VmapRetireDelta()
        for f in b.VMAP_RETIRE_OUTS:
            setattr(d, f, 9)
        for f, v in kw.items():
            setattr(d, f, v)
        return lib.sdm_vmap_retire(ctx, n, None if tg is None else tg.ctypes.data_as(ip), commit, ctypes.byref(d)), d

    rc, d = call()
    assert rc == ESTATE and b"no open voxel map" in lib.sdm_last_error()
    assert [getattr(d, f) for f in b.VMAP_RETIRE_OUTS] == [0] * 9
    eng.vmap_open(0.02)
    try:
        ref = Mirror(0.02)
        for k in refs[:3]:
            feed(eng, ref, [k], rows[[k]], centres_of({j: g["Tcw"][j] for j in refs}), **KW)
        classify_both(eng, ref, RULE)
        snap, osnap, st = snapshot(eng), obs_snapshot(eng), full_state(eng)
        M, E = snap[0]["voxels"], osnap[0]["observations"]
        want = vt.plan(ref.vm.rec["tag"], ref.ol.entry, ref.ol.tag, tags, "winner", ref.cl.flags(M), False)
        assert want["dropped"] > 1 and want["removed"] > 1
        guards = {f: np.full(max(M, E) + 8, GUARD * 0x01010101 if dt != np.uint8 else GUARD, dt) for f, dt in LIST_DT.items()}

        def refused(res, word, what, outs=None):
            rc, d = res
            assert rc == EINVAL and word in lib.sdm_last_error(), (what, rc, lib.sdm_last_error())
            exp = dict.fromkeys(b.VMAP_RETIRE_OUTS, 0)
            exp.update(outs or {})
            assert {f: getattr(d, f) for f in b.VMAP_RETIRE_OUTS} == exp, what
            unchanged(eng, snap, what)
            obs_unchanged(eng, osnap, what)
            state_unchanged(eng, st, what)
            for f, a in guards.items():
                assert a.tobytes() == bytes([GUARD]) * a.nbytes, (what, f)

        def ptrs(**caps):
            kw = {f: a.ctypes.data for f, a in guards.items()}
            kw.update(remap_capacity=M, dropped_capacity=M, removed_capacity=E)
            kw.update(caps)
            return kw

        assert lib.sdm_vmap_retire(ctx, 2, tags.ctypes.data_as(ip), 1, None) == EINVAL
        unchanged(eng, snap, "null delta")
        refused(call(-1, **ptrs()), b"negative n_tags", "n_tags < 0")
        refused(call(tg=None), b"null tags", "null tags")
        refused(call(tg=np.array([2, -1], np.int32)), b"tag outside", "a negative tag")
        refused(call(tg=np.array([2, 2], np.int32)), b"listed twice", "a tag listed twice")
        for v in (2, -1):
            refused(call(mode=v), b"mode", "mode %d" % v)
            refused(call(carry=v), b"carry", "carry %d" % v)
            refused(call(commit=v), b"commit", "commit %d" % v)
        refused(call(**ptrs(remap_capacity=-1)), b"negative capacity", "remap_capacity < 0")
        refused(call(**ptrs(dropped_capacity=-1)), b"negative capacity", "dropped_capacity < 0")
        refused(call(**ptrs(removed_capacity=-1)), b"negative capacity", "removed_capacity < 0")
        refused(call(dropped_published=guards["dropped_published"].ctypes.data, dropped_capacity=M), b"dropped_published without",
                "dropped_published alone")
        refused(call(removed_tag=guards["removed_tag"].ctypes.data, removed_capacity=E), b"removed_tag without", "removed_tag alone")
        dev = torch.full((M + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        for f, capf in (("remap", "remap_capacity"), ("dropped_ids", "dropped_capacity"), ("removed_entry", "removed_capacity")):
            refused(call(on_device=1, **{f: dev.data_ptr() + 2, capf: M}), b"not aligned", "a misaligned device " + f)
        refused(call(on_device=1, removed_entry=dev.data_ptr(), removed_tag=dev.data_ptr() + 1, removed_capacity=M), b"not aligned",
                "a misaligned device removed_tag")
        assert (to_host(dev, np.uint32) == 0x5A5A5A5A).all()
        # the capacity contract: all counts filled, no array written, nothing changed
        counts = {f: want[f] for f in b.VMAP_RETIRE_OUTS}
        for commit in (1, 0):
            refused(call(commit=commit, **ptrs(remap_capacity=M - 1)), b"remap_capacity", "a small remap", counts)
            refused(call(commit=commit, **ptrs(dropped_capacity=want["dropped"] - 1)), b"dropped_capacity", "a small dropped list", counts)
            refused(call(commit=commit, **ptrs(removed_capacity=want["removed"] - 1)), b"removed_capacity", "a small removed list", counts)
        with pytest.raises(ValueError):
            eng.vmap_retire(tags, mode="loser")
        with pytest.raises(ValueError):
            eng.vmap_retire(tags, remap=dev)   # a device remap beside lists made here
        with pytest.raises(pkg.SdmError) as err:
            eng.vmap_retire(tags, dropped={"dropped_ids": np.zeros(want["dropped"] - 1, np.uint32)})
        assert err.value.dropped == want["dropped"] and err.value.examined == M
        state_unchanged(eng, st, "binding refusals")
        # the map still works
        check_retire(eng, ref, tags, "winner", 1, "host", True, "after the refusals")
    finally:
        eng.vmap_close()
