"""GPU: the triangle mesh of the persistent voxel map (sdm_vmap_mesh / Engine.vmap_mesh) against tests/vmap_mesh_np.py fed the
records and flags the engine holds and the same normals -- after every call the three arrays, byte for byte, and the seven
totals.  Every output is an integer, so every comparison is for equality.  The maps, the normals and what they cover are
tests/test_vmap_mesh_cpu.py's; the estimated normals come from the engine's own sdm_vmap_normals."""
import ctypes
import sys

import numpy as np
import pytest
import torch

import hostile_keys as hk
import test_hostile_keys_cpu as hm
import vmap_mesh_np as vm
from test_gpu_extract import EINVAL, ESTATE
from test_gpu_hostile_table import map_model, witness
from test_gpu_slices import LOG2, default_env, environment
from test_gpu_vmap_class import Mirror, full_state, state_unchanged
from test_gpu_vmap_import import check_import
from test_gpu_vmap_normals import PUBLISH, SYN, flags_of, imported, records
from test_vmap_comp_cpu import FILTERS, RANDOM_VOXEL, random_case
from test_vmap_mesh_cpu import MAPS, crafted_normals
from test_vmap_normals_cpu import FAR, tagged
from test_vmap_repose_cpu import K_CAM, POSE_A, TAG_A, TAG_B, VOXEL, synthetic_records, synthetic_table

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = 0x07
PAD = 3
ARGS = ("tri", "owner_tris", "vertex_used")


def host(t):
    if not torch.is_tensor(t):
        return t
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def same(got, exp, what, fields=vm.ARRAYS):
    for f in fields:
        g = host(got[f])
        assert g.dtype == vm.DTYPES[f] and g.shape == exp[f].shape, (what, f, g.dtype, g.shape, exp[f].shape)
        assert g.tobytes() == exp[f].tobytes(), (what, f, np.flatnonzero((g != exp[f]).reshape(len(g), -1).any(1))[:8])
    assert {f: got[f] for f in vm.OUTS} == {f: exp[f] for f in vm.OUTS}, (what, {f: (got[f], exp[f]) for f in vm.OUTS})


def expected(eng, normal, **kw):
    return vm.mesh(records(eng), flags_of(eng), eng.vmap_info()["voxel_size"], normal, **kw)


def engine_normals(eng, **flt):
    """the engine's own normals of the whole map under a filter, as a host array"""
    return eng.vmap_normals(tags=FAR[0], Tcw=FAR[1], radius=2, min_points=3, variations=False, counts=False, **flt)["normal"]


def run(eng, what, normal, device=False, exact=False, want=vm.ARRAYS, exp=None, **kw):
    """one sdm_vmap_mesh against the restatement on the engine's own records and flags.  normal: float32[range, 3] on the host
    (uploaded here for a device call).  exact: destinations of exactly their sizes (else PAD elements more; what lies past the
    end keeps its sentinel); want: the arrays asked for, the others are NULL"""
    normal = np.ascontiguousarray(normal, F).reshape(-1, 3)
    exp = exp or expected(eng, normal, **kw)
    M = eng.vmap_info()["voxels"]
    sizes = {"tri": exp["triangles"], "owner_tris": exp["entries"], "vertex_used": M}
    dest = {}
    for f in vm.ARRAYS:
        per = 3 if f == "tri" else 1
        m = max(sizes[f] + (0 if exact else PAD), 1)
        if f not in want:
            dest[f] = False
        elif device:
            dest[f] = torch.full((m, per) if per > 1 else (m,), SENTINEL, dtype=torch.int32 if f == "tri" else torch.uint8, device="cuda")
        elif exact or f == "tri":
            dest[f] = np.full((m, per) if per > 1 else m, SENTINEL, vm.DTYPES[f])
        else:
            dest[f] = True
    given = torch.from_numpy(normal).cuda() if device else normal
    got = eng.vmap_mesh(given, **dest, **kw)
    assert set(got) == set(want) | set(vm.OUTS), (what, sorted(got))
    if exp["entries"] == 0:   # an empty range queues nothing: the plane of a caller's own destination is not written either
        for f in want:
            if dest[f] is not True:
                assert (host(dest[f]) == SENTINEL).all(), (what, f)
        same(got, exp, what, [f for f in want if f != "vertex_used" or dest[f] is True])
        return got
    same(got, exp, what, want)
    for f in want:   # nothing is written past the end
        if dest[f] is not True:
            assert (host(dest[f]).reshape(-1)[exp[f].size:] == SENTINEL).all(), (what, f)
    return got


# 1. parity on every map of the CPU test, made with vmap_import: the filters before any classify (no flag: require_published
# makes no member) and after a committing one, the engine's own normals and the crafted ones, host and device pointers, each
# destination NULL in turn and all NULL, destinations of exactly their sizes, the binding's own two calls (tri=True)
@pytest.mark.parametrize("name", sorted(MAPS))
def test_parity_on_imported_maps(pkg, gpu_ok, name):
    case, voxel = MAPS[name]
    rec, _ = case()
    M = len(rec["pixel"])
    eng = pkg.Engine(32, 24, 1)
    try:
        imported(eng, rec, voxel)
        for classified in (False, True):
            if classified:
                assert eng.vmap_classify(PUBLISH, True, ids=False)["published_total"] == int((rec["multiplicity"] >= 2).sum())
            i = 0
            for fi, flt in enumerate(FILTERS):
                for nrm in (engine_normals(eng, **flt) if M else np.zeros((0, 3), F), crafted_normals(M, fi)):
                    what = "%s %r classified %d call %d" % (name, flt, classified, i)
                    exp = expected(eng, nrm, **flt)
                    got = run(eng, what, nrm, device=(i % 2 == 1), exact=(i % 4 >= 2), exp=exp, **flt)
                    assert got["entries"] == M
                    if flt.get("require_published") and not classified:
                        assert got["members"] == 0 and got["triangles"] == 0
                    if i == 0:
                        for want in (("owner_tris", "vertex_used"), ("tri", "vertex_used"), ("tri", "owner_tris"), ("tri",), ()):
                            run(eng, "%s only %r" % (what, want), nrm, device=classified, exact=True, want=want, exp=exp, **flt)
                        twice = eng.vmap_mesh(nrm, **flt)   # one call for the totals, one to fill
                        same(twice, exp, what + " tri=True")
                        assert eng.vmap_mesh(nrm, tri=False, owner_tris=False, vertex_used=False, **flt) == {f: exp[f] for f in vm.OUTS}
                    i += 1
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
        nrm = engine_normals(eng)
        whole = expected(eng, nrm)
        assert whole["triangles"] > 100
        i = 0
        for first in (1, 63, 65):
            for count in (0, 1, 64):
                got = run(eng, "%s first %d count %d" % (name, first, count), nrm[first:first + count], device=(i % 2 == 0),
                          exact=(i % 3 == 0), first=first, count=count)
                i += 1
                inside = (whole["tri"][:, 0] >= first) & (whole["tri"][:, 0] < first + count)   # a sub-range is the slice
                assert host(got["tri"]).tobytes() == whole["tri"][inside].tobytes(), (first, count)
                assert host(got["owner_tris"]).tobytes() == whole["owner_tris"][first:first + count].tobytes()
                assert got["entries"] == count
        run(eng, "to the end", nrm[M - 65:], first=M - 65, **FILTERS[3])
        run(eng, "more normals than the range", nrm, first=2, count=70)   # (the binding's capacity is the rows given)
        got = run(eng, "the empty tail", nrm[M:], first=M)
        assert [got[f] for f in vm.OUTS] == [0] * 7
    finally:
        eng.close()


def outs_of(a, b):
    return [getattr(a, f) for f in b.VMAP_MESH_OUTS]


# 3. the capacity contract, state, every refusal, and determinism: a snapshot of the infos, a full fetch, the evidence, the
# flags and the log before and after every call; two runs give the same bits
def test_capacity_state_refusals_and_determinism(pkg, gpu_ok):
    b = sys.modules[pkg.__name__ + ".binding"]
    eng = pkg.Engine(32, 24, 1)
    lib, ctx = eng.lib, eng.ctx
    rec, pairs, _ = synthetic_records(2049)
    M = 2049
    normal = np.zeros((M + 8, 3), F)
    tri = np.full((2 * M + 8, 3), 0x07070707, np.uint32)
    owner = np.full(M + 8, SENTINEL, np.uint8)
    used = np.full(M + 8, SENTINEL, np.uint8)
    bufs = (tri, owner, used)

    def untouched():
        return (tri == 0x07070707).all() and (owner == SENTINEL).all() and (used == SENTINEL).all()

    def reset():
        tri[:], owner[:], used[:] = 0x07070707, SENTINEL, SENTINEL

    def call(**kw):
        a = b.VmapMeshArgs()
        a.first, a.count, a.capacity, a.tri_capacity, a.used_capacity = 0, -1, M + 8, 2 * M + 8, M + 8
        a.normal, a.tri, a.owner_tris, a.vertex_used = normal.ctypes.data, tri.ctypes.data, owner.ctypes.data, used.ctypes.data
        for f in b.VMAP_MESH_OUTS:
            setattr(a, f, 9)
        for f, v in kw.items():
            setattr(a, f, v)
        return lib.sdm_vmap_mesh(ctx, ctypes.byref(a)), a

    try:
        code, a = call()
        assert code == ESTATE and b"no open voxel map" in lib.sdm_last_error() and outs_of(a, b) == [0] * 7
        imported(eng, rec, VOXEL)
        eng.vmap_import_observations(pairs["entry"], pairs["tag"])
        eng.vmap_classify(PUBLISH, True, ids=False)
        nrm = eng.vmap_normals(tags=SYN[0], Tcw=SYN[1], radius=2, variations=False, counts=False)["normal"]
        normal[:M] = nrm
        st = full_state(eng)
        eng.dispatch_counts(reset=True)

        runs = []
        for _ in range(2):
            res = [run(eng, "host", nrm), run(eng, "device", nrm, device=True, min_multiplicity=2, require_published=True),
                   run(eng, "exact", nrm[3:2003], exact=True, first=3, count=2000),
                   run(eng, "crafted", crafted_normals(M), device=True, exact=True)]
            runs.append([host(x[f]).tobytes() for x in res for f in vm.ARRAYS] + [[x[f] for f in vm.OUTS] for x in res])
            state_unchanged(eng, st, "after the calls")
        assert runs[0] == runs[1]
        assert res[0]["quads"] > 0 and res[0]["owners"] > res[0]["quads"]
        assert eng.dispatch_counts()[2] == 0   # no launch of the default engine took a second dispatch

        # the capacity: T - 1 is refused with the totals filled and nothing written, T is accepted
        exp = expected(eng, nrm)
        T = exp["triangles"]
        assert T > 1
        code, a = call(tri_capacity=T - 1)
        assert code == EINVAL and b"tri_capacity" in lib.sdm_last_error() and b"totals are filled" in lib.sdm_last_error()
        assert outs_of(a, b) == [exp[f] for f in vm.OUTS] and untouched()
        state_unchanged(eng, st, "the capacity refusal")
        with pytest.raises(pkg.SdmError) as err:
            eng.vmap_mesh(nrm, tri_capacity=T - 1)
        assert err.value.code == EINVAL and [getattr(err.value, f) for f in vm.OUTS] == [exp[f] for f in vm.OUTS]
        code, a = call(tri_capacity=T - 1, tri=None)   # no list: nothing to refuse
        assert code == 0 and outs_of(a, b) == [exp[f] for f in vm.OUTS] and (tri == 0x07070707).all()
        assert owner[:M].tobytes() == exp["owner_tris"].tobytes() and used[:M].tobytes() == exp["vertex_used"].tobytes()
        reset()
        code, a = call(tri_capacity=T, capacity=M, used_capacity=M)   # exact capacities of every kind
        assert code == 0 and outs_of(a, b) == [exp[f] for f in vm.OUTS]
        assert tri[:T].tobytes() == exp["tri"].tobytes() and (tri[T:] == 0x07070707).all()
        assert owner[:M].tobytes() == exp["owner_tris"].tobytes() and (owner[M:] == SENTINEL).all()
        assert used[:M].tobytes() == exp["vertex_used"].tobytes() and (used[M:] == SENTINEL).all()
        reset()

        def refused(res, word, what, code=EINVAL):
            got, a = res
            assert got == code and word in lib.sdm_last_error(), (what, got, lib.sdm_last_error())
            assert outs_of(a, b) == [0] * 7, what
            state_unchanged(eng, st, what)

        assert lib.sdm_vmap_mesh(ctx, None) == EINVAL and b"null argument" in lib.sdm_last_error()
        for r in (2, -1):
            refused(call(require_published=r), b"require_published", "require_published %d" % r)
        refused(call(first=-1), b"range", "first < 0")
        refused(call(count=-2), b"range", "count < -1")
        refused(call(first=M + 1), b"range", "first > M")
        refused(call(first=1, count=M), b"range", "first + count > M")
        refused(call(first=1 << 62, count=1 << 62), b"range", "a sum that overflows")
        refused(call(normal=None), b"null normal", "NULL normal")
        refused(call(normal=None, tri=None, owner_tris=None, vertex_used=None), b"null normal", "NULL normal, totals only")
        for f in ("capacity", "tri_capacity", "used_capacity"):
            refused(call(**{f: -1}), b"negative capacity", f + " < 0")
            refused(call(tri=None, owner_tris=None, vertex_used=None, **{f: -1}), b"negative capacity", f + " < 0 without destinations")
        refused(call(capacity=M - 1), b"capacity below the range", "capacity < the range")
        refused(call(capacity=M - 1, tri=None, owner_tris=None, vertex_used=None), b"capacity below the range", "capacity < the range, normal alone")
        refused(call(first=10, count=100, capacity=99), b"capacity below the range", "capacity < count")
        refused(call(used_capacity=M - 1), b"used_capacity below", "used_capacity < M")
        refused(call(first=10, count=100, used_capacity=100), b"used_capacity below", "used_capacity = count < M")
        refused(call(on_device=1, normal=normal.ctypes.data + 2), b"not aligned", "a misaligned normal")
        refused(call(on_device=1, tri=tri.ctypes.data + 1), b"not aligned", "a misaligned tri")
        assert untouched()   # no refusal wrote
        with pytest.raises(ValueError):
            eng.vmap_mesh(torch.zeros((M, 3), dtype=torch.float32, device="cuda"), owner_tris=np.zeros(M, np.uint8))
        with pytest.raises(ValueError):
            eng.vmap_mesh(nrm, owner_tris=np.zeros(M, np.uint32))
        with pytest.raises(ValueError):
            eng.vmap_mesh(np.zeros(3 * M + 1, F))
        with pytest.raises(pkg.SdmError):
            eng.vmap_mesh(nrm[:M - 1])
        with pytest.raises(pkg.SdmError):
            eng.vmap_mesh(nrm, vertex_used=np.zeros(M - 1, np.uint8))
        with pytest.raises(pkg.SdmError):
            eng.vmap_mesh(nrm, require_published=2)
        state_unchanged(eng, st, "binding refusals")
        # the edges that are no refusals: no destination with capacities of 0, a used_capacity below M without the plane,
        # first == M with and without normals
        code, a = call(tri_capacity=0, used_capacity=0, tri=None, owner_tris=None, vertex_used=None)
        assert code == 0 and outs_of(a, b) == [exp[f] for f in vm.OUTS] and untouched()
        code, a = call(used_capacity=5, vertex_used=None, tri=None)
        assert code == 0 and a.vertices == exp["vertices"] and owner[:M].tobytes() == exp["owner_tris"].tobytes()
        reset()
        code, a = call(first=M, count=0)
        assert code == 0 and outs_of(a, b) == [0] * 7 and untouched()
        code, a = call(first=M, count=-1, capacity=0, normal=None)
        assert code == 0 and outs_of(a, b) == [0] * 7 and untouched()
        state_unchanged(eng, st, "after the edges")
        eng.vmap_clear()   # an open map without an entry: valid, nothing is queued, nothing is written
        code, a = call()
        assert code == 0 and outs_of(a, b) == [0] * 7 and untouched()
    finally:
        eng.close()


# 4. across a rehash and a record growth between two calls
def test_mesh_across_growth(pkg, gpu_ok):
    eng = pkg.Engine(32, 24, 1)
    rec1, _ = tagged(random_case(65, 8))
    rec2, _ = tagged(random_case(2049, 24))
    rec2 = dict(rec2, xyz=rec2["xyz"] + np.array([0, 0, 20 * RANDOM_VOXEL], F))   # cells of their own, far from the first map's
    try:
        imported(eng, rec1, RANDOM_VOXEL)
        n1 = engine_normals(eng)
        first = run(eng, "the small map", n1)
        info0 = eng.vmap_info()
        eng.vmap_import(rec2, updated=False)
        assert eng.vmap_info()["rehashes"] > info0["rehashes"] and eng.vmap_info()["voxels"] == 65 + 2049
        n2 = engine_normals(eng)
        assert n2[:65].tobytes() == n1.tobytes()
        second = run(eng, "after the growth", n2, device=True)
        assert second["members"] == first["members"] + 2049
        mine = host(second["tri"])
        assert mine[mine[:, 0] < 65].tobytes() == first["tri"].tobytes()   # the first map's triangles are as they were
        run(eng, "after the growth, filtered", engine_normals(eng, min_multiplicity=2), min_multiplicity=2)
    finally:
        eng.close()


# 5. after a repose and after a committing retire: ids and cells have moved, the table has been rebuilt
def test_mesh_after_repose_and_retire(pkg, gpu_ok):
    eng = pkg.Engine(32, 24, 1)
    rec, pairs, _ = synthetic_records(2049)
    try:
        imported(eng, rec, VOXEL)
        eng.vmap_import_observations(pairs["entry"], pairs["tag"])
        eng.vmap_classify(PUBLISH, True, ids=False)
        before = run(eng, "as imported", engine_normals(eng))
        tags, K, T = synthetic_table(2)
        moved = eng.vmap_repose(tags, K, T, carry=True)
        assert moved["merged"] > 0 and moved["dropped"] > 0 and moved["voxels"] < 2049
        for i, flt in enumerate(FILTERS):
            run(eng, "after the repose, %d" % i, engine_normals(eng, **flt), device=(i % 2 == 0), **flt)
        gone = eng.vmap_retire([TAG_A], carry=True)
        assert gone["dropped"] > 0 and gone["voxels"] < moved["voxels"]
        for i, flt in enumerate(FILTERS):
            after = run(eng, "after the retire, %d" % i, engine_normals(eng, **flt), device=(i % 2 == 1), **flt)
        assert after["entries"] == gone["voxels"] < before["entries"]
        eng.vmap_repose([TAG_B], [K_CAM], [POSE_A])
        run(eng, "after a second repose", crafted_normals(eng.vmap_info()["voxels"], 1))
    finally:
        eng.close()


# 6. colliding keys and probes that wrap the table's end (tests/hostile_keys.py): the chain of keys with one home at the
# table's last slot, then the pieces around it; the device's witness says the layout happened
def test_mesh_on_the_hostile_table(pkg, gpu_ok):
    eng = pkg.Engine(32, 24, 1)
    try:
        eng.vmap_open(hm.VOXEL)
        ref = Mirror(hm.VOXEL)
        chain_cells, ra = hm.chain_records()
        pieces, rb = hm.piece_records()
        ga, _ = check_import(eng, ref, ra, "the chain")
        assert ga["created"] == hm.L and eng.vmap_info()["table_slots"] == 1024
        assert witness(eng, 16, map_model(eng, ref), "the chain alone") == (hm.L - 1, hm.L - 1)
        M = eng.vmap_info()["voxels"]
        a = run(eng, "the chain", engine_normals(eng))
        run(eng, "the chain, crafted", crafted_normals(M), device=True)
        gb, _ = check_import(eng, ref, rb, "the pieces")
        assert gb["created"] == len(pieces) and eng.vmap_info()["table_slots"] == hm.CAP_PIECES
        m = map_model(eng, ref)
        inside = hk.homes_in_run(hk.cell_key(pieces), hm.CAP_PIECES, m["run"])
        assert int(inside.sum()) >= hm.MIN_PIECES_IN_RUN and m["min_wraps"] >= hm.L - 1
        witness(eng, 16, m, "chain and pieces")
        M = eng.vmap_info()["voxels"]
        eng.vmap_classify(dict(min_neighbours=3), True, ids=False)
        got = []
        for i, flt in enumerate(FILTERS):
            nrm = engine_normals(eng, **flt)
            got.append(run(eng, "chain and pieces %d" % i, nrm, device=(i % 2 == 1), exact=(i >= 2), **flt))
            run(eng, "chain and pieces, crafted %d" % i, crafted_normals(M, i), device=(i % 2 == 0), **flt)
        assert got[0]["triangles"] > 0 and got[0]["members"] == M
        print("hostile table: chain", {f: a[f] for f in vm.OUTS}, "with the pieces", {f: got[0][f] for f in vm.OUTS})
    finally:
        eng.close()


# 7. slicing: an engine whose launches go out one workgroup at a time beside a default one, on the map of 2049 entries and the
# plane; the dispatch counters prove the slicing
@pytest.mark.parametrize("name", ("random 2049", "plane"))
def test_mesh_in_slices(pkg, gpu_ok, name):
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
            n0, n1 = engine_normals(eng), engine_normals(eng, require_published=True)
            exp = [expected(eng, n0), expected(eng, n1[1:M - 1], first=1, count=M - 2, require_published=True)]
            eng.dispatch_counts(reset=True)
            a = run(eng, "whole", n0, exp=exp[0])
            ca = eng.dispatch_counts(reset=True)
            f = run(eng, "filtered", n1[1:M - 1], device=True, exp=exp[1], first=1, count=M - 2, require_published=True)
            cf = eng.dispatch_counts(reset=True)
            res.append(([host(x[k]).tobytes() for x in (a, f) for k in vm.ARRAYS], ca, cf))
        assert res[0][0] == res[1][0]
        # the call's four sliced launches: find over the range and the vertex count over the map go out one workgroup of
        # 256 at a time, the tile count and the write one tile of 2048 entries at a time
        for n, c in ((M, res[0][1]), (M - 2, res[0][2])):
            parts = [(n + 255) // 256, (n + 2047) // 2048, (M + 255) // 256, (n + 2047) // 2048]
            assert c[0] == 4 and c[1] == sum(parts) and c[2] == sum(p > 1 for p in parts), (n, c, parts)
        assert res[1][1][0] == 4 and res[1][1][2] == 0 and res[1][2][2] == 0, res[1]
    finally:
        sliced.close()
        plain.close()
