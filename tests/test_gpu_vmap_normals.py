"""GPU: per-entry surface normals of the persistent voxel map (sdm_vmap_normals / Engine.vmap_normals) against
tests/vmap_normals_np.py fed the records and flags the engine holds -- after every call the three arrays, byte for byte, and
the four totals.  The arithmetic is specified operation by operation, so every comparison is for equality.  The maps and what
they cover are tests/test_vmap_normals_cpu.py's."""
import ctypes
import sys

import numpy as np
import pytest
import torch

import vmap_normals_np as vn
from test_gpu_extract import EINVAL, ESTATE
from test_gpu_slices import LOG2, default_env, environment
from test_gpu_vmap_class import full_state, state_unchanged
from test_vmap_comp_cpu import FILTERS, RANDOM_VOXEL, random_case
from test_vmap_normals_cpu import FAR, MAPS, MIXED, RADII, table, tagged
from test_vmap_repose_cpu import K_CAM, POSE_A, TAG_A, TAG_B, VOXEL, synthetic_records, synthetic_table

pytestmark = pytest.mark.gpu
F = np.float32
PUBLISH = dict(min_multiplicity=2)   # a committing classify under this rule publishes the entries of two points or more
SENTINEL = 0x07070707
DTYPES = dict(zip(vn.ARRAYS, (F, F, np.uint32)))
ARGS = dict(zip(vn.ARRAYS, ("normals", "variations", "counts")))
# the tables of the synthetic maps: the A entries' tag, two tags of the rest and one no entry carries; B is absent
SYN = table({TAG_A: (0.0, 0.0, -1.0), 25: (5.0, 5.0, 5.0), 41: (np.nan, 0.0, 0.0), 1000: (0.0, 0.0, 0.0)})


def host(t, f):
    return t.cpu().numpy().view(DTYPES[f]) if torch.is_tensor(t) else t


def same(got, exp, what, fields=vn.ARRAYS):
    for f in fields:
        g = host(got[f], f)
        assert g.dtype == DTYPES[f] and g.shape == exp[f].shape, (what, f, g.dtype, g.shape, exp[f].shape)
        assert g.tobytes() == exp[f].tobytes(), (what, f, np.flatnonzero((g.view(np.uint32) != exp[f].view(np.uint32)).reshape(len(g), -1).any(1))[:8])
    assert {f: got[f] for f in vn.OUTS} == {f: exp[f] for f in vn.OUTS}, (what, {f: (got[f], exp[f]) for f in vn.OUTS})


def records(eng):
    rec = eng.vmap_fetch(fields=("xyz", "multiplicity", "tag"))
    return {"xyz": np.array(rec["xyz"]).reshape(-1, 3), "multiplicity": np.array(rec["multiplicity"]), "tag": np.array(rec["tag"])}


def flags_of(eng):
    """the flags as the engine holds them, or None before the first classify"""
    return np.array(eng.vmap_fetch_published()) if eng.vmap_class_info()["calls"] else None


def expected(eng, **kw):
    return vn.normals(records(eng), flags_of(eng), eng.vmap_info()["voxel_size"], **kw)


def run(eng, what, device=False, exact=False, want=vn.ARRAYS, exp=None, **kw):
    """one sdm_vmap_normals against the restatement on the engine's own records and flags.  exact: destinations of exactly
    the range (else 3 elements more; the words past the range keep their sentinel); want: the arrays asked for, the others are
    NULL"""
    exp = exp or expected(eng, **kw)
    n = exp["entries"]
    dest = {}
    for f in vn.ARRAYS:
        per = 3 if f == "normal" else 1
        if f not in want:
            dest[f] = False
        elif device or exact:
            m = max(n if exact else n + 3, 1)
            if device:
                dest[f] = torch.full((m, per) if per > 1 else (m,), SENTINEL, dtype=torch.int32, device="cuda")
            else:
                dest[f] = np.full((m, per) if per > 1 else m, SENTINEL, np.uint32).view(DTYPES[f])
        else:
            dest[f] = True
    got = eng.vmap_normals(**{ARGS[f]: d for f, d in dest.items()}, **kw)
    assert set(got) == set(want) | set(vn.OUTS), (what, sorted(got))
    same(got, exp, what, want)
    for f in want:   # nothing is written past the range
        if dest[f] is not True:
            assert (host(dest[f], f).view(np.uint32).reshape(-1)[exp[f].size:] == SENTINEL).all(), (what, f)
    return got


def imported(eng, rec, voxel):
    eng.vmap_open(voxel)
    if len(rec["pixel"]):
        assert (eng.vmap_import(rec, updated=False)["dst_ids"] == np.arange(len(rec["pixel"]))).all()


def combos(M):
    """(radius, arguments) of a map's calls: both radii x the four filters; in turn with the mixed table (some tags present,
    some absent, one pose not finite), without a table, and with the full one; min_points from 3 up to 9"""
    tables = (dict(tags=MIXED[0], Tcw=MIXED[1]), dict(), dict(tags=FAR[0], Tcw=FAR[1]))
    out = []
    for r in RADII:
        for fi, flt in enumerate(FILTERS):
            out.append((r, dict(flt, min_points=3 + fi * r, **tables[(fi + r - 1) % 3])))
    return out


# 1. parity on every map of the CPU test, made with vmap_import: both radii, the filters before any classify (no flag:
# require_published makes no member) and after a committing one, with and without a pose table, host and device destinations,
# each destination NULL in turn and all NULL, destinations of exactly the range
@pytest.mark.parametrize("name", sorted(MAPS))
def test_parity_on_imported_maps(pkg, gpu_ok, name):
    case, voxel = MAPS[name]
    rec, _ = case()
    M = len(rec["pixel"])
    eng = pkg.Engine(32, 24, 1)
    try:
        imported(eng, rec, voxel)
        assert (records(eng)["tag"] == rec["tag"]).all()
        for classified in (False, True):
            if classified:
                assert eng.vmap_classify(PUBLISH, True, ids=False)["published_total"] == int((rec["multiplicity"] >= 2).sum())
            for i, (r, kw) in enumerate(combos(M)):
                what = "%s radius %d %r classified %d" % (name, r, {k: v for k, v in kw.items() if k not in ("tags", "Tcw")}, classified)
                exp = expected(eng, radius=r, **kw)
                got = run(eng, what, device=(i % 2 == 1), exact=(i % 4 >= 2 and M > 0), exp=exp, radius=r, **kw)
                assert got["entries"] == M
                if kw.get("require_published") and not classified:
                    assert got["members"] == 0 and not host(got["points"], "points").any()
                if i == 0:
                    for want in (("variation", "points"), ("normal", "points"), ("normal", "variation"), ("points",), ()):
                        run(eng, "%s only %r" % (what, want), device=classified, exact=(M > 0), want=want, exp=exp, radius=r, **kw)
    finally:
        eng.close()


# 2. ranges that start and end inside a wave, on the map of 2049 entries and on the plane
@pytest.mark.parametrize("name", ("random 2049", "plane"))
def test_ranges(pkg, gpu_ok, name):
    case, voxel = MAPS[name]
    rec, _ = case()
    M = len(rec["pixel"])
    eng = pkg.Engine(32, 24, 1)
    try:
        imported(eng, rec, voxel)
        eng.vmap_classify(PUBLISH, True, ids=False)
        whole = {r: expected(eng, tags=MIXED[0], Tcw=MIXED[1], radius=r) for r in RADII}
        i = 0
        for first in (1, 63, 65):
            for count in (0, 1, 64):
                for r in RADII:
                    got = run(eng, "%s first %d count %d radius %d" % (name, first, count, r), device=(i % 2 == 0), exact=(i % 3 == 0),
                              tags=MIXED[0], Tcw=MIXED[1], radius=r, first=first, count=count)
                    i += 1
                    for f in vn.ARRAYS:   # a sub-range is the slice of the whole
                        assert host(got[f], f).tobytes() == whole[r][f][first:first + count].tobytes(), (f, first, count, r)
                    assert got["entries"] == count
        run(eng, "to the end", first=M - 65, radius=2, **FILTERS[3])
        got = run(eng, "the empty tail", first=M)
        assert [got[f] for f in vn.OUTS] == [0] * 4
    finally:
        eng.close()


def outs_of(a, b):
    return [getattr(a, f) for f in b.VMAP_NORMAL_OUTS]


# 3. state, every refusal, and determinism: a snapshot of the infos, a full fetch, the evidence, the flags and the log before
# and after every call; two runs give the same bits
def test_state_refusals_and_determinism(pkg, gpu_ok):
    b = sys.modules[pkg.__name__ + ".binding"]
    eng = pkg.Engine(32, 24, 1)
    lib, ctx = eng.lib, eng.ctx
    rec, pairs, _ = synthetic_records(2049)
    M = 2049
    normal = np.full((M + 8, 3), SENTINEL, np.uint32).view(F)
    variation = np.full(M + 8, SENTINEL, np.uint32).view(F)
    points = np.full(M + 8, SENTINEL, np.uint32)
    bufs = (normal, variation, points)
    tags = np.ascontiguousarray(SYN[0])
    Tcw = np.ascontiguousarray(SYN[1])
    ip, fp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_float)

    def untouched():
        return all((x.view(np.uint32) == SENTINEL).all() for x in bufs)

    def call(n=len(tags), tg=tags, T=Tcw, **kw):
        a = b.VmapNormalArgs()
        a.radius, a.min_points, a.first, a.count, a.capacity = 1, 3, 0, -1, M + 8
        a.normal, a.variation, a.points = normal.ctypes.data, variation.ctypes.data, points.ctypes.data
        for f in b.VMAP_NORMAL_OUTS:
            setattr(a, f, 9)
        for f, v in kw.items():
            setattr(a, f, v)
        return lib.sdm_vmap_normals(ctx, n, None if tg is None else tg.ctypes.data_as(ip), None if T is None else T.ctypes.data_as(fp),
                                    ctypes.byref(a)), a

    try:
        code, a = call()
        assert code == ESTATE and b"no open voxel map" in lib.sdm_last_error() and outs_of(a, b) == [0] * 4
        imported(eng, rec, VOXEL)
        eng.vmap_import_observations(pairs["entry"], pairs["tag"])
        eng.vmap_classify(PUBLISH, True, ids=False)
        st = full_state(eng)
        eng.dispatch_counts(reset=True)

        runs = []
        for _ in range(2):
            res = [run(eng, "host", tags=SYN[0], Tcw=SYN[1], radius=2),
                   run(eng, "device", device=True, tags=SYN[0], Tcw=SYN[1], radius=1, min_points=4, min_multiplicity=2, require_published=True),
                   run(eng, "exact", exact=True, radius=2, min_points=6, first=3, count=2000)]
            runs.append([host(x[f], f).tobytes() for x in res for f in vn.ARRAYS] + [[x[f] for f in vn.OUTS] for x in res])
            state_unchanged(eng, st, "after the calls")
        assert runs[0] == runs[1]
        assert res[0]["oriented"] > 0 and res[0]["estimated"] > res[0]["oriented"]
        assert eng.dispatch_counts()[2] == 0   # no launch of the default engine took a second dispatch

        def refused(res, word, what, code=EINVAL):
            got, a = res
            assert got == code and word in lib.sdm_last_error(), (what, got, lib.sdm_last_error())
            assert outs_of(a, b) == [0] * 4, what
            state_unchanged(eng, st, what)

        assert lib.sdm_vmap_normals(ctx, 0, None, None, None) == EINVAL and b"null argument" in lib.sdm_last_error()
        for r in (0, 3, -1):
            refused(call(radius=r), b"radius", "radius %d" % r)
        for r, p in ((1, 2), (1, 28), (2, 126), (2, 0)):
            refused(call(radius=r, min_points=p), b"min_points", "radius %d min_points %d" % (r, p))
        for r in (2, -1):
            refused(call(require_published=r), b"require_published", "require_published %d" % r)
        refused(call(first=-1), b"range", "first < 0")
        refused(call(count=-2), b"range", "count < -1")
        refused(call(first=M + 1), b"range", "first > M")
        refused(call(first=1, count=M), b"range", "first + count > M")
        refused(call(first=1 << 62, count=1 << 62), b"range", "a sum that overflows")
        refused(call(capacity=-1), b"negative capacity", "capacity < 0")
        refused(call(capacity=-1, normal=None, variation=None, points=None), b"negative capacity", "capacity < 0 without destinations")
        refused(call(capacity=M - 1), b"capacity below", "capacity < the range")
        refused(call(capacity=M - 1, normal=None, variation=None), b"capacity below", "capacity < the range with points alone")
        refused(call(capacity=M - 1, variation=None, points=None), b"capacity below", "capacity < the range with normal alone")
        refused(call(first=10, count=100, capacity=99), b"capacity below", "capacity < count")
        refused(call(on_device=1, normal=normal.ctypes.data + 2), b"not aligned", "a misaligned normal")
        refused(call(on_device=1, variation=variation.ctypes.data + 1), b"not aligned", "a misaligned variation")
        refused(call(on_device=1, points=points.ctypes.data + 3), b"not aligned", "a misaligned points")
        refused(call(n=-1), b"negative n_poses", "n_poses < 0")
        refused(call(tg=None), b"null pose table", "NULL tags")
        refused(call(T=None), b"null pose table", "NULL Tcw")
        bad = tags.copy()
        bad[1] = -1
        refused(call(tg=bad), b"tag outside", "a negative tag")
        bad[1] = bad[3]
        refused(call(tg=bad), b"listed twice", "a tag listed twice")
        assert untouched()   # no refusal wrote
        with pytest.raises(ValueError):
            eng.vmap_normals(normals=torch.zeros((M, 3), dtype=torch.float32, device="cuda"), variations=np.zeros(M, F))
        with pytest.raises(ValueError):
            eng.vmap_normals(normals=np.zeros((M, 3), np.float64))
        with pytest.raises(ValueError):
            eng.vmap_normals(tags=[1, 2], Tcw=np.zeros((1, 12), F))
        with pytest.raises(pkg.SdmError):
            eng.vmap_normals(radius=3)
        with pytest.raises(pkg.SdmError):
            eng.vmap_normals(counts=np.zeros(M - 1, np.uint32))
        state_unchanged(eng, st, "binding refusals")
        # the edges that are no refusals: capacity exactly the range, no destination with a capacity below it, no table,
        # the largest min_points, first == M
        exp = expected(eng, tags=SYN[0], Tcw=SYN[1])
        code, a = call(capacity=M)
        assert code == 0 and outs_of(a, b) == [exp[f] for f in vn.OUTS]
        for f, x in zip(vn.ARRAYS, bufs):
            assert x[:M].tobytes() == exp[f].tobytes() and (x[M:].view(np.uint32) == SENTINEL).all(), f
        for x in bufs:
            x.view(np.uint32)[:] = SENTINEL
        code, a = call(capacity=0, normal=None, variation=None, points=None)
        assert code == 0 and outs_of(a, b) == [exp[f] for f in vn.OUTS] and untouched()
        code, a = call(n=0, tg=None, T=None, capacity=0, normal=None, variation=None, points=None)
        assert code == 0 and a.oriented == 0 and a.estimated == exp["estimated"]
        code, a = call(radius=2, min_points=125, capacity=0, normal=None, variation=None, points=None)
        assert code == 0 and a.estimated == 0 and a.members == M
        code, a = call(first=M, count=0)
        assert code == 0 and outs_of(a, b) == [0] * 4 and untouched()
        code, a = call(first=M, count=-1, capacity=0)
        assert code == 0 and outs_of(a, b) == [0] * 4 and untouched()
        state_unchanged(eng, st, "after the edges")
        eng.vmap_clear()   # an open map without an entry: valid, nothing is queued, nothing is written
        code, a = call()
        assert code == 0 and outs_of(a, b) == [0] * 4 and untouched()
    finally:
        eng.close()


# 4. across a rehash and a record growth between two calls
def test_normals_across_growth(pkg, gpu_ok):
    eng = pkg.Engine(32, 24, 1)
    rec1, _ = tagged(random_case(65, 8))
    rec2, _ = tagged(random_case(2049, 24))
    rec2 = dict(rec2, xyz=rec2["xyz"] + np.array([0, 0, 20 * RANDOM_VOXEL], F))   # cells of their own, far from the first map's
    try:
        imported(eng, rec1, RANDOM_VOXEL)
        first = run(eng, "the small map", tags=MIXED[0], Tcw=MIXED[1], radius=2)
        info0 = eng.vmap_info()
        eng.vmap_import(rec2, updated=False)
        assert eng.vmap_info()["rehashes"] > info0["rehashes"] and eng.vmap_info()["voxels"] == 65 + 2049
        second = run(eng, "after the growth", device=True, tags=MIXED[0], Tcw=MIXED[1], radius=2)
        assert second["members"] == first["members"] + 2049
        for f in vn.ARRAYS:   # the first map's entries are as they were
            assert host(second[f], f)[:65].tobytes() == first[f].tobytes(), f
        run(eng, "after the growth, filtered", radius=1, min_points=5, min_multiplicity=2)
    finally:
        eng.close()


# 5. after a repose and after a committing retire: ids and cells have moved, the table has been rebuilt
def test_normals_after_repose_and_retire(pkg, gpu_ok):
    eng = pkg.Engine(32, 24, 1)
    rec, pairs, _ = synthetic_records(2049)
    try:
        imported(eng, rec, VOXEL)
        eng.vmap_import_observations(pairs["entry"], pairs["tag"])
        eng.vmap_classify(PUBLISH, True, ids=False)
        before = run(eng, "as imported", tags=SYN[0], Tcw=SYN[1], radius=2)
        tags, K, T = synthetic_table(2)
        moved = eng.vmap_repose(tags, K, T, carry=True)
        assert moved["merged"] > 0 and moved["dropped"] > 0 and moved["voxels"] < 2049
        for i, (r, kw) in enumerate(combos(0)[2:6]):
            kw = dict(kw, **(dict(tags=SYN[0], Tcw=SYN[1]) if "tags" in kw else {}))
            run(eng, "after the repose, %d" % i, device=(i % 2 == 0), radius=r, **kw)
        gone = eng.vmap_retire([TAG_A], carry=True)
        assert gone["dropped"] > 0 and gone["voxels"] < moved["voxels"]
        for i, (r, kw) in enumerate(combos(0)[2:6]):
            kw = dict(kw, **(dict(tags=SYN[0], Tcw=SYN[1]) if "tags" in kw else {}))
            after = run(eng, "after the retire, %d" % i, device=(i % 2 == 1), radius=r, **kw)
        assert after["entries"] == gone["voxels"] < before["entries"]
        eng.vmap_repose([TAG_B], [K_CAM], [POSE_A])
        run(eng, "after a second repose", tags=SYN[0], Tcw=SYN[1], radius=1)
    finally:
        eng.close()


# 6. slicing: an engine whose launches go out one workgroup at a time beside a default one, on the map of 2049 entries and the
# plane; the dispatch counters prove the slicing
@pytest.mark.parametrize("name", ("random 2049", "plane"))
def test_normals_in_slices(pkg, gpu_ok, name):
    case, voxel = MAPS[name]
    rec, _ = case()
    M = len(rec["pixel"])
    with default_env(), environment(**{LOG2: 8}):
        sliced = pkg.Engine(32, 24, 1)
    with default_env():
        plain = pkg.Engine(32, 24, 1)
    try:
        res = []
        for eng in (sliced, plain):
            imported(eng, rec, voxel)
            eng.vmap_classify(PUBLISH, True, ids=False)
            exp = [expected(eng, tags=MIXED[0], Tcw=MIXED[1], radius=2),
                   expected(eng, tags=FAR[0], Tcw=FAR[1], radius=1, first=1, count=M - 2, require_published=True)]
            eng.dispatch_counts(reset=True)
            a = run(eng, "whole", exp=exp[0], tags=MIXED[0], Tcw=MIXED[1], radius=2)
            ca = eng.dispatch_counts(reset=True)
            f = run(eng, "filtered", device=True, exp=exp[1], tags=FAR[0], Tcw=FAR[1], radius=1, first=1, count=M - 2, require_published=True)
            cf = eng.dispatch_counts(reset=True)
            res.append(([host(x[k], k).tobytes() for x in (a, f) for k in vn.ARRAYS], ca, cf))
        assert res[0][0] == res[1][0]
        # (the call's one sliced launch goes out one workgroup of 256 entries at a time)
        blocks = (M + 255) // 256
        assert res[0][1][2] == 1 and res[0][1][1] == blocks and res[0][2][2] == 1 and res[0][2][1] == (M - 2 + 255) // 256, res[0]
        assert res[1][1][2] == 0 and res[1][2][2] == 0, res[1]
    finally:
        sliced.close()
        plain.close()
