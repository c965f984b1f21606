"""GPU: connected components of the persistent voxel map's entries (sdm_vmap_components / Engine.vmap_components) against
tests/vmap_comp_np.py fed the records and flags the engine holds -- after every call the three arrays and the six totals.
Every output is an integer: every comparison is for equality.  The maps and what they cover are
tests/test_vmap_comp_cpu.py's."""
import ctypes
import sys

import numpy as np
import pytest
import torch

import vmap_comp_np as vq
from test_gpu_extract import EINVAL, ESTATE
from test_gpu_slices import LOG2, default_env, environment
from test_gpu_vmap_class import full_state, state_unchanged
from test_vmap_comp_cpu import CONNECTIVITIES, FILTERS, MAPS, RANDOM_VOXEL, SMALL, block_case, lines_case, random_case, small_case
from test_vmap_repose_cpu import K_CAM, POSE_A, TAG_A, TAG_B, VOXEL, synthetic_records, synthetic_table

pytestmark = pytest.mark.gpu
PUBLISH = dict(min_multiplicity=2)   # a committing classify under this rule publishes the entries of two points or more
SENTINEL = 0x07070707
# every connectivity without a filter and with both, and the two single filters at 26
COMBOS = tuple((c, kw) for c in CONNECTIVITIES for kw in (FILTERS[0], FILTERS[3])) + ((26, FILTERS[1]), (26, FILTERS[2]))


def host(t):
    return t.cpu().numpy().view(np.uint32) if torch.is_tensor(t) else t


def same(got, exp, what, fields=vq.ARRAYS):
    for f in fields:
        g = host(got[f])
        assert g.dtype == np.uint32 and g.shape == exp[f].shape, (what, f, g.dtype, g.shape, exp[f].shape)
        assert g.tobytes() == exp[f].tobytes(), (what, f, np.flatnonzero(g != exp[f])[:8])
    assert {f: got[f] for f in vq.OUTS} == {f: exp[f] for f in vq.OUTS}, (what, {f: (got[f], exp[f]) for f in vq.OUTS})


def records(eng):
    rec = eng.vmap_fetch(fields=("xyz", "multiplicity"))
    return {"xyz": np.array(rec["xyz"]).reshape(-1, 3), "multiplicity": np.array(rec["multiplicity"])}


def flags_of(eng):
    """the flags as the engine holds them, or None before the first classify"""
    return np.array(eng.vmap_fetch_published()) if eng.vmap_class_info()["calls"] else None


def expected(eng, **kw):
    return vq.components(records(eng), flags_of(eng), eng.vmap_info()["voxel_size"], **kw)


def comp(eng, what, device=False, exact=False, want=vq.ARRAYS, exp=None, **kw):
    """one sdm_vmap_components against the restatement on the engine's own records and flags.  exact: destinations of
    exactly M (small_ids: exactly `small`) elements; want: the arrays asked for, the others are NULL"""
    exp = exp or expected(eng, **kw)
    M = exp["entries"]
    dest = {}
    for f, arg in zip(vq.ARRAYS, ("labels", "sizes", "small_ids")):
        if f not in want:
            dest[arg] = False
        elif device or exact:
            n = max((exp["small"] if f == "small_ids" else M) if exact else M + 3, 1)
            dest[arg] = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda") if device else np.full(n, SENTINEL, np.uint32)
        else:
            dest[arg] = True
    got = eng.vmap_components(**dest, **kw)
    assert set(got) == set(want) | set(vq.OUTS), (what, sorted(got))
    same(got, exp, what, want)
    for f, arg in zip(vq.ARRAYS, ("labels", "sizes", "small_ids")):   # nothing is written past the M (small) elements
        if f in want and dest[arg] is not True:
            assert (host(dest[arg])[len(exp[f]):] == SENTINEL).all(), (what, f)
    return got


def imported(eng, rec, voxel):
    eng.vmap_open(voxel)
    if len(rec["pixel"]):
        assert (eng.vmap_import(rec, updated=False)["dst_ids"] == np.arange(len(rec["pixel"]))).all()


# 1. parity on every crafted and random map, made with vmap_import: the three connectivities, both filters before any
# classify (no flag: require_published makes no member) and after a committing one, host and device destinations, each
# destination NULL in turn and all NULL, destinations of exactly M and exactly `small` elements
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
            for i, (c, kw) in enumerate(COMBOS):
                what = "%s connectivity %d %r classified %d" % (name, c, kw, classified)
                exp = expected(eng, connectivity=c, min_size=4, **kw)
                got = comp(eng, what, device=(i % 2 == 1), exact=(i % 4 >= 2 and M > 0), exp=exp, connectivity=c, min_size=4, **kw)
                assert got["entries"] == M
                if kw.get("require_published") and not classified:
                    assert got["members"] == 0 and (host(got["label"]) == vq.NO_COMPONENT).all()
                if i == 0:
                    for want in (("size", "small_ids"), ("label", "small_ids"), ("label", "size"), ("small_ids",), ()):
                        comp(eng, "%s only %r" % (what, want), device=classified, exact=(M > 0), want=want, exp=exp, connectivity=c,
                             min_size=4, **kw)
        if name == "small":   # what the crafted pieces are for, read from the engine's own answer
            res = {c: eng.vmap_components(connectivity=c) for c in CONNECTIVITIES}
            for piece, joined in (("face", [1, 1, 1]), ("edge", [0, 1, 1]), ("corner", [0, 0, 1]), ("z into y", [0, 0, 0]),
                                  ("y into x", [0, 0, 0]), ("last cells", [1, 1, 1]), ("first cells", [1, 1, 1])):
                a, n = SMALL[piece]
                assert [int(len(set(res[c]["label"][a:a + n].tolist())) == 1) for c in CONNECTIVITIES] == joined, piece
    finally:
        eng.close()


def outs_of(a, b):
    return [getattr(a, f) for f in b.VMAP_COMP_OUTS]


# 2. the capacity refusal: the totals are filled, no destination is written, and the second call with small_capacity = small
# succeeds; the binding raises with the totals
def test_capacity_refusal(pkg, gpu_ok):
    b = sys.modules[pkg.__name__ + ".binding"]
    rec, _ = random_case(2049, 24)
    M = 2049
    eng = pkg.Engine(32, 24, 1)
    try:
        imported(eng, rec, RANDOM_VOXEL)
        exp = expected(eng, connectivity=6, min_size=5)
        small = exp["small"]
        assert 1 < small < M
        st = full_state(eng)
        for device in (False, True):
            if device:
                bufs = [torch.full((M,), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(3)]
                ptrs = [t.data_ptr() for t in bufs]
            else:
                bufs = [np.full(M, SENTINEL, np.uint32) for _ in range(3)]
                ptrs = [t.ctypes.data for t in bufs]
            a = b.VmapCompArgs()
            a.connectivity, a.min_size, a.on_device, a.capacity, a.small_capacity = 6, 5, int(device), M, small - 1
            a.label, a.size, a.small_ids = ptrs
            assert eng.lib.sdm_vmap_components(eng.ctx, ctypes.byref(a)) == EINVAL
            assert b"small_capacity" in eng.lib.sdm_last_error()
            assert outs_of(a, b) == [exp[f] for f in vq.OUTS]                   # the totals are filled
            assert all((host(t) == SENTINEL).all() for t in bufs)               # the destinations hold their sentinel bytes
            state_unchanged(eng, st, "the capacity refusal")
            a.small_capacity = a.small
            assert eng.lib.sdm_vmap_components(eng.ctx, ctypes.byref(a)) == 0
            got = dict({f: host(t) for f, t in zip(vq.ARRAYS, bufs)}, **{f: getattr(a, f) for f in vq.OUTS})
            got["small_ids"], rest = got["small_ids"][:small], got["small_ids"][small:]
            same(got, exp, "the second call, device %d" % device)
            assert (rest == SENTINEL).all()
        with pytest.raises(pkg.SdmError) as e:
            eng.vmap_components(connectivity=6, min_size=5, small_ids=np.zeros(small - 1, np.uint32))
        assert [getattr(e.value, f) for f in vq.OUTS] == [exp[f] for f in vq.OUTS]
        # a list nobody asked for is no refusal, whatever small_capacity says
        got = eng.vmap_components(connectivity=6, min_size=5, small_ids=False)
        assert got["small"] == small and "small_ids" not in got
        state_unchanged(eng, st, "after the refusals")
    finally:
        eng.close()


# 3. state, every other refusal, and determinism: a snapshot of the infos, a full fetch, the evidence, the flags and the log
# before and after every call; two runs give the same bits
def test_state_refusals_and_determinism(pkg, gpu_ok):
    b = sys.modules[pkg.__name__ + ".binding"]
    eng = pkg.Engine(32, 24, 1)
    lib, ctx = eng.lib, eng.ctx
    rec, pairs, _ = synthetic_records(2049)
    M = 2049
    label, size, small = (np.full(M + 8, SENTINEL, np.uint32) for _ in range(3))

    def call(**kw):
        a = b.VmapCompArgs()
        a.connectivity, a.min_size, a.capacity, a.small_capacity = 26, 4, M + 8, M + 8
        a.label, a.size, a.small_ids = label.ctypes.data, size.ctypes.data, small.ctypes.data
        for f in b.VMAP_COMP_OUTS:
            setattr(a, f, 9)
        for f, v in kw.items():
            setattr(a, f, v)
        return lib.sdm_vmap_components(ctx, ctypes.byref(a)), a

    try:
        code, a = call()
        assert code == ESTATE and b"no open voxel map" in lib.sdm_last_error() and outs_of(a, b) == [0] * 6
        imported(eng, rec, VOXEL)
        eng.vmap_import_observations(pairs["entry"], pairs["tag"])
        eng.vmap_classify(PUBLISH, True, ids=False)
        st = full_state(eng)
        eng.dispatch_counts(reset=True)

        runs = []
        for _ in range(2):
            res = [comp(eng, "host", connectivity=26, min_size=4),
                   comp(eng, "device", device=True, connectivity=6, min_size=3, min_multiplicity=2, require_published=True),
                   comp(eng, "exact", exact=True, connectivity=18, min_size=100)]
            runs.append([host(x[f]).tobytes() for x in res for f in vq.ARRAYS] + [[x[f] for f in vq.OUTS] for x in res])
            state_unchanged(eng, st, "after the calls")
        assert runs[0] == runs[1]
        assert eng.dispatch_counts()[2] == 0   # no launch of the default engine took a second dispatch

        def refused(res, word, what, code=EINVAL):
            got, a = res
            assert got == code and word in lib.sdm_last_error(), (what, got, lib.sdm_last_error())
            assert outs_of(a, b) == [0] * 6, what
            state_unchanged(eng, st, what)

        assert lib.sdm_vmap_components(ctx, None) == EINVAL and b"null argument" in lib.sdm_last_error()
        for c in (0, 4, 8, 27, -26):
            refused(call(connectivity=c), b"connectivity", "connectivity %d" % c)
        for r in (2, -1):
            refused(call(require_published=r), b"require_published", "require_published %d" % r)
        refused(call(capacity=-1), b"negative capacity", "capacity < 0")
        refused(call(small_capacity=-1), b"negative capacity", "small_capacity < 0")
        refused(call(small_capacity=-1, small_ids=None), b"negative capacity", "small_capacity < 0 without the list")
        refused(call(capacity=M - 1), b"capacity below", "capacity < M")
        refused(call(capacity=M - 1, label=None), b"capacity below", "capacity < M with size alone")
        refused(call(capacity=M - 1, size=None), b"capacity below", "capacity < M with label alone")
        refused(call(on_device=1, label=label.ctypes.data + 2), b"not aligned", "a misaligned label")
        refused(call(on_device=1, size=size.ctypes.data + 1), b"not aligned", "a misaligned size")
        refused(call(on_device=1, small_ids=small.ctypes.data + 3), b"not aligned", "a misaligned small_ids")
        assert (label == SENTINEL).all() and (size == SENTINEL).all() and (small == SENTINEL).all()   # no refusal wrote
        with pytest.raises(ValueError):
            eng.vmap_components(labels=torch.zeros(M, dtype=torch.int32, device="cuda"), sizes=np.zeros(M, np.uint32))
        with pytest.raises(ValueError):
            eng.vmap_components(labels=np.zeros(M, np.int64))
        with pytest.raises(pkg.SdmError):
            eng.vmap_components(connectivity=7)
        with pytest.raises(pkg.SdmError):
            eng.vmap_components(labels=np.zeros(M - 1, np.uint32))
        state_unchanged(eng, st, "binding refusals")
        # the edges that are no refusals: capacity exactly M, no label or size with a capacity below M, the totals alone
        exp = expected(eng, connectivity=26, min_size=4)
        code, a = call(capacity=M, small_capacity=exp["small"])
        assert code == 0 and outs_of(a, b) == [exp[f] for f in vq.OUTS]
        np.testing.assert_array_equal(label[:M], exp["label"])
        np.testing.assert_array_equal(size[:M], exp["size"])
        np.testing.assert_array_equal(small[:exp["small"]], exp["small_ids"])
        assert (label[M:] == SENTINEL).all() and (size[M:] == SENTINEL).all() and (small[exp["small"]:] == SENTINEL).all()
        label[:], size[:], small[:] = SENTINEL, SENTINEL, SENTINEL
        code, a = call(capacity=0, label=None, size=None)
        assert code == 0 and outs_of(a, b) == [exp[f] for f in vq.OUTS] and (label == SENTINEL).all()
        np.testing.assert_array_equal(small[:exp["small"]], exp["small_ids"])
        small[:] = SENTINEL
        code, a = call(capacity=0, small_capacity=0, label=None, size=None, small_ids=None)
        assert code == 0 and outs_of(a, b) == [exp[f] for f in vq.OUTS] and (small == SENTINEL).all()
        code, a = call(min_size=0, small_capacity=0)
        assert code == 0 and a.small == 0 and a.small_components == 0 and a.members == exp["members"]
        state_unchanged(eng, st, "after the edges")
        eng.vmap_clear()   # an open map without an entry: valid, nothing is queued, nothing is written
        label[:], size[:] = SENTINEL, SENTINEL
        code, a = call()
        assert code == 0 and outs_of(a, b) == [0] * 6 and (label == SENTINEL).all() and (size == SENTINEL).all()
    finally:
        eng.close()


# 4. across a rehash and a record growth between two calls
def test_components_across_growth(pkg, gpu_ok):
    eng = pkg.Engine(32, 24, 1)
    rec1, _ = random_case(65, 8)
    rec2, _ = random_case(2049, 24)
    rec2 = dict(rec2, xyz=rec2["xyz"] + np.array([0, 0, 20 * RANDOM_VOXEL], np.float32))   # cells of their own, not adjacent to the first map's
    try:
        imported(eng, rec1, RANDOM_VOXEL)
        first = comp(eng, "the small map", min_size=4)
        info0 = eng.vmap_info()
        eng.vmap_import(rec2, updated=False)
        assert eng.vmap_info()["rehashes"] > info0["rehashes"] and eng.vmap_info()["voxels"] == 65 + 2049
        second = comp(eng, "after the growth", device=True, min_size=4)
        assert second["members"] == first["members"] + 2049 and second["largest"] > first["largest"]
        np.testing.assert_array_equal(host(second["label"])[:65], first["label"])   # the first map's pieces are as they were
        for c in (6, 18):
            comp(eng, "after the growth, %d" % c, connectivity=c, min_size=9, min_multiplicity=2)
    finally:
        eng.close()


# 5. after a repose and after a committing retire: ids and cells have moved, the table has been rebuilt
def test_components_after_repose_and_retire(pkg, gpu_ok):
    eng = pkg.Engine(32, 24, 1)
    rec, pairs, _ = synthetic_records(2049)
    try:
        imported(eng, rec, VOXEL)
        eng.vmap_import_observations(pairs["entry"], pairs["tag"])
        eng.vmap_classify(PUBLISH, True, ids=False)
        before = comp(eng, "as imported", min_size=4)
        tags, K, T = synthetic_table(2)
        moved = eng.vmap_repose(tags, K, T, carry=True)
        assert moved["merged"] > 0 and moved["dropped"] > 0 and moved["voxels"] < 2049
        for i, (c, kw) in enumerate(COMBOS):
            comp(eng, "after the repose, %d %r" % (c, kw), device=(i % 2 == 0), connectivity=c, min_size=4, **kw)
        gone = eng.vmap_retire([TAG_A], carry=True)
        assert gone["dropped"] > 0 and gone["voxels"] < moved["voxels"]
        for i, (c, kw) in enumerate(COMBOS):
            after = comp(eng, "after the retire, %d %r" % (c, kw), device=(i % 2 == 1), connectivity=c, min_size=4, **kw)
        assert after["entries"] == gone["voxels"] < before["entries"]
        eng.vmap_repose([TAG_B], [K_CAM], [POSE_A])
        comp(eng, "after a second repose", min_size=2)
    finally:
        eng.close()


# 6. slicing: an engine whose launches go out one workgroup at a time beside a default one, on the maps where a link of one
# slice meets the links of every other: the lines of 2049 cells and the 17 x 17 x 17 block
@pytest.mark.parametrize("case", (lines_case, block_case))
def test_components_in_slices(pkg, gpu_ok, case):
    rec, _ = case()
    with default_env(), environment(**{LOG2: 8}):
        sliced = pkg.Engine(32, 24, 1)
    with default_env():
        plain = pkg.Engine(32, 24, 1)
    try:
        res = []
        for eng in (sliced, plain):
            imported(eng, rec, 1.0)
            eng.vmap_classify(PUBLISH, True, ids=False)
            exp = [expected(eng, connectivity=c, min_size=5, **kw) for c, kw in ((26, {}), (6, dict(require_published=True)))]
            eng.dispatch_counts(reset=True)
            a = comp(eng, "whole", exp=exp[0], connectivity=26, min_size=5)
            ca = eng.dispatch_counts(reset=True)
            f = comp(eng, "filtered", device=True, exp=exp[1], connectivity=6, min_size=5, require_published=True)
            cf = eng.dispatch_counts(reset=True)
            res.append(([host(x[k]).tobytes() for x in (a, f) for k in vq.ARRAYS], ca, cf))
        assert res[0][0] == res[1][0]
        # (the call's five sliced launches -- init, link, flatten, count, write -- each take more than one dispatch)
        assert res[0][1][2] >= 5 and res[0][2][2] >= 5 and res[0][1][1] > 5 * res[0][1][2] // 2, res[0]
        assert res[1][1][2] == 0 and res[1][2][2] == 0, res[1]
    finally:
        sliced.close()
        plain.close()
