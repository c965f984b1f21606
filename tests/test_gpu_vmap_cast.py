"""GPU: ray queries on the persistent voxel map (sdm_vmap_cast_segments, sdm_vmap_render / Engine.vmap_cast_segments,
.vmap_render) against tests/vmap_cast_np.py fed the records and flags the engine holds -- after every call every output
array and the four totals.  Every output is an integer, a copied id, or one float formula restated operation by operation:
every comparison is for equality, hit_rho's on the bits.  The synthetic inputs and what they cover are
tests/test_vmap_cast_cpu.py's."""
import ctypes
import sys

import numpy as np
import pytest
import torch

import golden_util as gu
import vmap_cast_np as vk
from test_gpu_extract import EINVAL, ESTATE, pipeline
from test_gpu_slices import LOG2, default_env, environment
from test_gpu_vmap_class import full_state, state_unchanged
from test_vmap_cast_cpu import (CRAFTED_COMBOS, EQ_MARGIN, EQ_STEPS, EQ_VOXEL, FILTERS, PINNED, POSE_AT, POSE_AWAY, POSE_NAN,
                                RENDER_K, RENDER_SIZES, RHO_FAR, SYN_M, SYN_RAYS, VOXEL, crafted_case, log_rays,
                                synthetic_case, synthetic_rays)
from test_vmap_recarve_cpu import build

pytestmark = pytest.mark.gpu
F = np.float32
KW = dict(max_sigma=0.3)
ARRAYS = {"hit_id": np.uint32, "hit_step": np.int32, "hit_rho": np.float32}
PUBLISH = dict(min_multiplicity=2)   # a committing classify under this rule publishes the entries of two points or more


def cuda(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a.copy()).cuda()


def host(t, dt):
    return t.cpu().numpy().view(dt) if torch.is_tensor(t) else t


def same(got, exp, what, fields):
    for f in fields:
        g = host(got[f], ARRAYS[f])
        assert g.dtype == ARRAYS[f] and g.shape == exp[f].shape, (what, f, g.dtype, g.shape, exp[f].shape)
        assert g.tobytes() == exp[f].tobytes(), (what, f, np.flatnonzero(g.reshape(-1) != exp[f].reshape(-1))[:8])
    assert {f: got[f] for f in vk.OUTS} == {f: exp[f] for f in vk.OUTS}, (what, {f: (got[f], exp[f]) for f in vk.OUTS})


def records(eng):
    rec = eng.vmap_fetch(fields=("xyz", "multiplicity"))
    return {"xyz": np.array(rec["xyz"]).reshape(-1, 3), "multiplicity": np.array(rec["multiplicity"])}


def flags_of(eng):
    """the flags as the engine holds them, or None before the first classify"""
    return np.array(eng.vmap_fetch_published()) if eng.vmap_class_info()["calls"] else None


def cast(eng, O, P, what, device=False, steps=True, exact=False, **kw):
    """one sdm_vmap_cast_segments against the restatement on the engine's own records and flags"""
    exp = vk.cast_segments(records(eng), flags_of(eng), O, P, eng.vmap_info()["voxel_size"], **kw)
    n = len(O)
    ids = True
    if exact and n:  # destinations of exactly n elements
        ids = torch.empty(n, dtype=torch.int32, device="cuda") if device else np.empty(n, np.uint32)
        steps = (torch.empty(n, dtype=torch.int32, device="cuda") if device else np.empty(n, np.int32)) if steps else False
    got = eng.vmap_cast_segments(cuda(O) if device else O, cuda(P) if device else P, steps=steps, ids=ids, **kw)
    assert ("hit_step" in got) == (steps is not False)
    if device:
        assert got["hit_id"].is_cuda
    same(got, exp, what, ("hit_id", "hit_step") if steps is not False else ("hit_id",))
    return got


def render(eng, T, W, H, what, device=False, **kw):
    exp = vk.render(records(eng), flags_of(eng), RENDER_K, T, W, H, RHO_FAR, eng.vmap_info()["voxel_size"], **kw)
    dest = {}
    if device:  # destinations of exactly W * H elements
        dest = dict(ids=torch.empty(W * H, dtype=torch.int32, device="cuda"), steps=torch.empty(W * H, dtype=torch.int32, device="cuda"),
                    rho=torch.empty(W * H, dtype=torch.float32, device="cuda"))
    got = eng.vmap_render(RENDER_K, T, W, H, RHO_FAR, **dest, **kw)
    same(got, exp, what, tuple(ARRAYS))
    return got


def imported(eng, rec, voxel=VOXEL):
    eng.vmap_open(voxel)
    if len(rec["pixel"]):
        assert (eng.vmap_import(rec, updated=False)["dst_ids"] == np.arange(len(rec["pixel"]))).all()


# 1. parity on maps made with vmap_import: the wave edges in rays and entries, host and device, hit_step NULL, destinations
# of exactly n elements, the margins, both filters before any classify (no flag: nothing is published) and after a
# committing one
@pytest.mark.parametrize("M", SYN_M)
def test_parity_on_imported_maps(pkg, gpu_ok, M):
    eng = pkg.Engine(32, 24, 1)
    rec, _ = synthetic_case(M, 0)
    try:
        imported(eng, rec)
        seen = dict(hit=0, skipped=0, miss=0)
        for classified in (False, True):
            if classified:
                pub = eng.vmap_classify(PUBLISH, True, ids=False)["published_total"]
                assert pub == int((rec["multiplicity"] >= 2).sum()) and (M < 65 or 0 < pub < M)
            for n in SYN_RAYS:
                O, P = synthetic_rays(rec, n)
                what = "M %d rays %d classified %d" % (M, n, classified)
                got = cast(eng, O, P, what, device=(n % 2 == 0), exact=(n in (1, 64, 1025)))
                assert got["rays_total"] == n
                seen["hit"] += got["rays_hit"]
                seen["skipped"] += got["rays_skipped"]
                seen["miss"] += n - got["rays_hit"] - got["rays_skipped"]
                cast(eng, O, P, what + " published only", device=(n % 2 == 1), exact=(n == 65), steps=False, require_published=True)
                if n == 1025:
                    for kw in FILTERS[1:] + (dict(start_margin=1, end_margin=1), dict(max_steps=200, start_margin=3),
                                             dict(min_multiplicity=4), dict(end_margin=1000)):
                        got = cast(eng, O, P, "%s %r" % (what, kw), **kw)
                        if not classified and kw.get("require_published"):
                            assert got["rays_hit"] == 0 and got["cells_visited"] > 0
        assert seen["skipped"] > 0 and seen["miss"] > 0 and (seen["hit"] > 0) == (M > 0), seen
    finally:
        eng.close()


# 2. the crafted rays: N == max_steps and max_steps + 1, N = 0, margins beyond N, axis ties, the last cells of the range,
# NaN and Inf coordinates, entries that are transparent and entries behind them
def test_crafted_rays(pkg, gpu_ok):
    eng = pkg.Engine(32, 24, 1)
    rec, _, O, P = crafted_case()
    try:
        imported(eng, rec, 1.0)
        for classified in (False, True):
            if classified:
                assert eng.vmap_classify(PUBLISH, True, ids=False)["published_total"] == 12
            for i, kw in enumerate(CRAFTED_COMBOS):
                cast(eng, O, P, "crafted %r classified %d" % (kw, classified), device=(i % 2 == 1), **kw)
        got = eng.vmap_cast_segments(O, P, max_steps=64, start_margin=1)
        assert got["hit_id"][[0, 9, 8, 11]].tolist() == [1, 9, vk.NO_HIT, 1] and got["hit_step"][[0, 9, 8, 11]].tolist() == [1, 4, 0, 1]
        assert got["hit_id"][[13, 14, 15, 16, 17]].tolist() == [12, vk.SKIPPED, 13, vk.SKIPPED, vk.NO_HIT]
    finally:
        eng.close()


# 3. the render: a pose looking at the map, one looking away (all misses), a NaN pose (all skipped); hit_rho bitwise
@pytest.mark.parametrize("W,H", RENDER_SIZES)
def test_render(pkg, gpu_ok, W, H):
    eng = pkg.Engine(32, 24, 1)
    rec, _ = synthetic_case(2049, 0)
    try:
        imported(eng, rec)
        for classified in (False, True):
            if classified:
                eng.vmap_classify(PUBLISH, True, ids=False)
            for device in (False, True):
                what = "%d x %d classified %d device %d" % (W, H, classified, device)
                at = render(eng, POSE_AT, W, H, what + " at", device)
                away = render(eng, POSE_AWAY, W, H, what + " away", device)
                none = render(eng, POSE_NAN, W, H, what + " no pose", device)
                assert away["rays_hit"] == 0 and away["rays_skipped"] == 0 and none["rays_skipped"] == W * H
                if (W, H) == (33, 17):
                    assert at["rays_hit"] > W * H // 8 and (host(at["hit_rho"], F) > 0).sum() == at["rays_hit"]
                render(eng, POSE_AT, W, H, what + " filtered", device, min_multiplicity=2, require_published=True, start_margin=2)
        got = eng.vmap_render(RENDER_K, POSE_AT, W, H, RHO_FAR, ids=False, steps=False)   # hit_rho alone
        assert set(got) == {"hit_rho"} | set(vk.OUTS) and got["hit_rho"].shape == (H, W)
    finally:
        eng.close()


# 4. across a rehash and a record growth between two casts
def test_casts_across_growth(pkg, gpu_ok):
    eng = pkg.Engine(32, 24, 1)
    rec1, _ = synthetic_case(65, 0)
    rec2, _ = synthetic_case(2049, 0)
    rec2 = dict(rec2, xyz=rec2["xyz"] + np.array([0, 0, 6 * VOXEL], F))   # voxels of their own, behind the first map's
    try:
        imported(eng, rec1)
        O, P = synthetic_rays(rec2, 1025)
        first = cast(eng, O, P, "the small map")
        info0 = eng.vmap_info()
        eng.vmap_import(rec2, updated=False)
        assert eng.vmap_info()["rehashes"] > info0["rehashes"] and eng.vmap_info()["voxels"] == 65 + 2049
        second = cast(eng, O, P, "after the growth")
        assert second["rays_hit"] > first["rays_hit"]
        render(eng, POSE_AT, 33, 17, "after the growth")
    finally:
        eng.close()


# 5. the occlusion recipe on a golden fixture: is the (entry, camera) pair of the log occluded by another entry?  Keyframe 0
# of the strip, integrated and observed alone at voxel 0.005: 25 of its 8937 pairs are (tests/test_vmap_cast_cpu.py)
def test_occlusion_recipe(pkg, gpu_ok):
    name = "strip_roll_160x120_n7"
    g = gu.load(name)
    eng = pipeline(pkg, g)
    rows = np.ascontiguousarray(g["nbrs"][:, :3])
    try:
        eng.vmap_open(EQ_VOXEL)
        eng.vmap_integrate([0], updated=False, **KW)
        eng.vmap_observe([0], rows[[0]], **KW)
        rec, log = eng.vmap_fetch(), eng.vmap_fetch_observations()
        vm, ol = build({f: rec[f] for f in ("xyz", "pixel", "rho_sigma", "intensity", "tag", "multiplicity")}, log, EQ_VOXEL)
        tags = np.unique(np.append(rows[0], 0)).astype(np.int32)
        O, P, entry = log_rays(vm, ol, tags, [g["Tcw"][k] for k in tags])
        inner = cast(eng, O, P, "occluded pairs", end_margin=EQ_MARGIN + 1, max_steps=EQ_STEPS)
        whole = cast(eng, O, P, "every pair to its end", device=True, max_steps=EQ_STEPS)
        print(name, {f: inner[f] for f in vk.OUTS}, {f: whole[f] for f in vk.OUTS})
        assert (inner["rays_hit"], inner["cells_visited"], whole["rays_hit"], whole["cells_visited"]) == PINNED[name]
        occluded = inner["hit_id"] != vk.NO_HIT
        assert occluded.sum() == 25 and (inner["hit_id"][occluded] != entry[occluded]).all()
    finally:
        eng.close()


def outs_of(a, b):
    return [getattr(a, f) for f in b.VMAP_CAST_OUTS]


# 6. state and refusals: a snapshot of the infos, a full fetch, the evidence, the flags and the log before and after every
# call; every SDM_EINVAL and SDM_ESTATE case with that same snapshot; two runs give the same bits
def test_state_refusals_and_determinism(pkg, gpu_ok):
    b = sys.modules[pkg.__name__ + ".binding"]
    eng = pkg.Engine(32, 24, 1)
    lib, ctx = eng.lib, eng.ctx
    rec, pairs = synthetic_case(2049, 5000)
    O, P = synthetic_rays(rec, 257)
    O, P = np.ascontiguousarray(O), np.ascontiguousarray(P)
    ids, steps, rho = np.zeros(600, np.uint32), np.zeros(600, np.int32), np.zeros(600, F)
    K, T = np.ascontiguousarray(RENDER_K), np.ascontiguousarray(POSE_AT)
    fp = ctypes.POINTER(ctypes.c_float)

    def args(**kw):
        a = b.VmapCastArgs()
        a.max_steps, a.capacity = 4096, 600
        a.hit_id, a.hit_step, a.hit_rho = ids.ctypes.data, steps.ctypes.data, rho.ctypes.data
        for f in b.VMAP_CAST_OUTS:
            setattr(a, f, 9)
        for f, v in kw.items():
            setattr(a, f, v)
        return a

    def seg(n=257, o=O.ctypes.data, p=P.ctypes.data, **kw):
        a = args(**kw)
        return lib.sdm_vmap_cast_segments(ctx, n, o, p, ctypes.byref(a)), a

    def ren(W=33, H=17, rho_far=RHO_FAR, k=K, t=T, **kw):
        a = args(**kw)
        return lib.sdm_vmap_render(ctx, None if k is None else k.ctypes.data_as(fp), None if t is None else t.ctypes.data_as(fp), W, H,
                                   rho_far, ctypes.byref(a)), a

    try:
        for code, a in (seg(), ren()):
            assert code == ESTATE and b"no open voxel map" in lib.sdm_last_error() and outs_of(a, b) == [0] * 4
        imported(eng, rec)
        eng.vmap_import_observations(pairs["entry"], pairs["tag"])
        eng.vmap_classify(PUBLISH, True, ids=False)
        st = full_state(eng)
        eng.dispatch_counts(reset=True)

        # the calls themselves move nothing, and two runs give the same bits
        runs = []
        for _ in range(2):
            a = cast(eng, O, P, "host")
            c = cast(eng, O, P, "device", device=True, min_multiplicity=2, require_published=True)
            r = render(eng, POSE_AT, 33, 17, "render")
            d = render(eng, POSE_AT, 33, 17, "render to the device", device=True, start_margin=1)
            runs.append([host(x[f], ARRAYS[f]).tobytes() for x in (a, c, r, d) for f in ARRAYS if f in x] +
                        [[x[f] for f in vk.OUTS] for x in (a, c, r, d)])
            state_unchanged(eng, st, "after the casts and the renders")
        assert runs[0] == runs[1]
        assert eng.dispatch_counts()[2] == 0   # no launch of the default engine took a second dispatch

        def refused(res, word, what, code=EINVAL):
            got, a = res
            assert got == code and word in lib.sdm_last_error(), (what, got, lib.sdm_last_error())
            assert outs_of(a, b) == [0] * 4, what
            state_unchanged(eng, st, what)

        ids[:], steps[:], rho[:] = 7, 7, 7
        assert lib.sdm_vmap_cast_segments(ctx, 257, O.ctypes.data, P.ctypes.data, None) == EINVAL
        assert lib.sdm_vmap_render(ctx, K.ctypes.data_as(fp), T.ctypes.data_as(fp), 33, 17, RHO_FAR, None) == EINVAL
        refused(seg(-1), b"n outside", "n < 0")
        refused(seg((1 << 30) + 1, capacity=1 << 40), b"n outside", "n > 2^30")
        refused(seg(o=None), b"null origins or ends", "null origins")
        refused(seg(p=None), b"null origins or ends", "null ends")
        refused(seg(hit_id=None, hit_step=None), b"no output requested", "no destination (hit_rho does not count)")
        refused(seg(capacity=256), b"capacity", "capacity < n")
        refused(seg(on_device=1, hit_id=ids.ctypes.data + 2), b"not aligned", "a misaligned hit_id")
        refused(seg(on_device=1, hit_step=steps.ctypes.data + 1), b"not aligned", "a misaligned hit_step")
        refused(seg(o=O.ctypes.data + 2, on_device=1), b"not aligned", "misaligned origins")
        refused(seg(p=P.ctypes.data + 1, on_device=1), b"not aligned", "misaligned ends")
        refused(seg(start_margin=-1), b"negative start_margin or end_margin", "start_margin < 0")
        refused(seg(end_margin=-1), b"negative start_margin or end_margin", "end_margin < 0")
        refused(seg(max_steps=0), b"max_steps", "max_steps 0")
        refused(seg(max_steps=65537), b"max_steps", "max_steps beyond SDM_FREESPACE_MAX_STEPS")
        refused(seg(require_published=2), b"require_published", "require_published 2")
        refused(seg(require_published=-1), b"require_published", "require_published -1")
        for W, H in ((0, 17), (33, 0), (65536, 1), (1, 65536), (-1, 17)):
            refused(ren(W, H), b"W or H outside", "W %d H %d" % (W, H))
        refused(ren(40000, 40000, capacity=1 << 40), b"W * H above 2^30", "W * H > 2^30")
        refused(ren(k=None), b"null K or Tcw", "null K")
        refused(ren(t=None), b"null K or Tcw", "null Tcw")
        refused(ren(hit_id=None, hit_step=None, hit_rho=None), b"no output requested", "no destination at all")
        refused(ren(capacity=33 * 17 - 1), b"capacity", "capacity < W * H")
        refused(ren(on_device=1, hit_rho=rho.ctypes.data + 2), b"not aligned", "a misaligned hit_rho")
        refused(ren(end_margin=-1), b"negative start_margin or end_margin", "render: end_margin < 0")
        refused(ren(max_steps=0), b"max_steps", "render: max_steps 0")
        refused(ren(require_published=3), b"require_published", "render: require_published 3")
        for bad in (float("nan"), 0.0, -1.0, 9.9e-7, float("-inf")):
            refused(ren(rho_far=bad), b"rho_far", "rho_far %r" % bad)
        assert (ids == 7).all() and (steps == 7).all() and (rho == 7).all()   # no refusal wrote a destination
        with pytest.raises(ValueError):
            eng.vmap_cast_segments(O, P[:5])
        with pytest.raises(ValueError):
            eng.vmap_cast_segments(cuda(O), P)
        with pytest.raises(pkg.SdmError):
            eng.vmap_cast_segments(O, P, max_steps=0)
        with pytest.raises(pkg.SdmError):
            eng.vmap_render(RENDER_K, POSE_AT, 33, 17, 0.0)
        state_unchanged(eng, st, "binding refusals")
        # the edges that are no refusals
        code, a = seg(0, None, None)
        assert code == 0 and outs_of(a, b) == [0] * 4 and (ids == 7).all()
        code, a = seg(257, capacity=257, max_steps=65536, hit_step=None)
        exp = vk.cast_segments(records(eng), flags_of(eng), O, P, VOXEL, max_steps=65536)
        assert code == 0 and outs_of(a, b) == [exp[f] for f in vk.OUTS] and (steps == 7).all() and (ids[257:] == 7).all()
        np.testing.assert_array_equal(ids[:257], exp["hit_id"])
        code, a = ren(1, 1, 1.1e-6, capacity=1)
        assert code == 0 and a.rays_total == 1
        state_unchanged(eng, st, "after the edges")
        cast(eng, O, P, "after the refusals")
    finally:
        eng.close()


# 7. slicing: an engine whose launches go out one workgroup at a time beside a default one
def test_casts_in_slices(pkg, gpu_ok):
    rec, _ = synthetic_case(2049, 0)
    O, P = synthetic_rays(rec, 1025)
    with default_env(), environment(**{LOG2: 8}):
        sliced = pkg.Engine(32, 24, 1)
    with default_env():
        plain = pkg.Engine(32, 24, 1)
    try:
        res = []
        for eng in (sliced, plain):
            imported(eng, rec)
            eng.vmap_classify(PUBLISH, True, ids=False)
            eng.dispatch_counts(reset=True)
            a = cast(eng, O, P, "1025 rays", min_multiplicity=2)
            ca = eng.dispatch_counts(reset=True)
            r = render(eng, POSE_AT, 33, 17, "33 x 17", require_published=True)
            cr = eng.dispatch_counts(reset=True)
            res.append(([x[f].tobytes() for x in (a, r) for f in ARRAYS if f in x], ca, cr))
        assert res[0][0] == res[1][0]
        # (the fetches the comparison makes are counted too: the cast's own group is the one of 5 and of 3 dispatches)
        assert res[0][1][2] > 0 and res[0][1][1] >= 5 and res[0][2][2] > 0 and res[0][2][1] >= 3, res[0]
        assert res[1][1][2] == 0 and res[1][2][2] == 0, res[1]
    finally:
        sliced.close()
        plain.close()
