"""GPU: rebuilding the persistent voxel map's free-space evidence from its observation log (sdm_vmap_recarve /
Engine.vmap_recarve) against tests/vmap_recarve_np.py -- after every call the seven outs and a full fetch of the evidence.
Every counter and total is a sum of ones: every comparison is for equality.  The synthetic inputs and what they cover
are tests/test_vmap_recarve_cpu.py's."""
import ctypes
import sys

import numpy as np
import pytest

import golden_util as gu
import vmap_class_np as vcl
import vmap_recarve_np as vr
from test_gpu_extract import EINVAL, ESTATE, pipeline
from test_gpu_vmap import same_fetch
from test_gpu_vmap_class import full_state, state_unchanged
from test_gpu_vmap_repose import perturbed
from test_vmap_recarve_cpu import (COUNTERS, EQ_MARGIN, EQ_STEPS, EQ_VOXEL, PINNED, SYN_CASES, SYN_POSES, VOXEL, build,
                                   crafted_case, synthetic_case, table)

pytestmark = pytest.mark.gpu
F = np.float32
KW = dict(max_sigma=0.3)
RECORD = ("xyz", "pixel", "rho_sigma", "intensity", "tag", "multiplicity")


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


class Model:
    """the restatement's map and log beside the engine's, and the two counters"""

    def __init__(self, eng, rec, pairs, voxel):
        self.eng, self.voxel = eng, voxel
        self.vm, self.ol = build(rec, pairs, voxel)
        got = eng.vmap_import(rec, updated=False)
        assert (got["dst_ids"] == np.arange(self.vm.M)).all()
        if len(pairs["entry"]):
            assert eng.vmap_import_observations(pairs["entry"], pairs["tag"])["created"] == self.ol.E
        self.ev = {f: np.zeros(0, np.uint64) for f in COUNTERS}

    def same_evidence(self, what=""):
        got = self.eng.vmap_fetch_evidence()
        for f in COUNTERS:
            exp = np.zeros(self.vm.M, np.uint64)
            exp[:len(self.ev[f])] = self.ev[f]
            assert got[f].dtype == np.uint64 and got[f].shape == exp.shape, (what, f)
            np.testing.assert_array_equal(got[f], exp, err_msg="%s %s" % (what, f))

    def recarve(self, tags, Tcw, what="", reset=True, first=0, count=None, end_margin=1, max_steps=4096):
        """one sdm_vmap_recarve against the restatement: the seven outs and a full fetch of the evidence"""
        exp = vr.recarve((self.vm.keys, self.vm.ids), self.vm.rec["xyz"], self.ol.entry, self.ol.tag, tags, Tcw, self.voxel,
                         end_margin, max_steps, first, count)
        self.ev = vr.accumulate(self.ev, self.vm.M, exp, reset)
        got = self.eng.vmap_recarve(tags, Tcw, end_margin, max_steps, reset, first, count)
        assert got == {f: exp[f] for f in vr.OUTS}, (what, got, {f: exp[f] for f in vr.OUTS})
        self.same_evidence(what)
        return got


# 1. parity on maps made with vmap_import: the wave edges, the tables of 0, 1, 2 and 37 poses with their hostile poses, both
# resets, the range whole, split at the 64-boundaries +-1, and empty.  No carve has run on such a map: the first recarve
# allocates the counters
@pytest.mark.parametrize("M,E", SYN_CASES)
def test_parity_on_imported_maps(pkg, gpu_ok, M, E):
    eng = pkg.Engine(32, 24, 1)
    rec, pairs = synthetic_case(M, E)
    try:
        eng.vmap_open(VOXEL)
        m = Model(eng, rec, pairs, VOXEL)
        m.same_evidence("before any carve")
        seen = dict(hit=0, skipped=0, unposed=0, rays=0)
        for n_poses in SYN_POSES:
            tags, Tcw = table(n_poses)
            what = "M %d E %d poses %d" % (M, E, n_poses)
            whole = m.recarve(tags, Tcw, what + " whole")
            assert whole["pairs_total"] == E
            if n_poses == 0:
                assert whole["pairs_unposed"] == E and not m.ev["crossings"].any() and not m.ev["ends"].any()
            once = {f: m.ev[f].copy() for f in COUNTERS}
            m.recarve(tags, Tcw, what + " again without reset", reset=False)
            for f in COUNTERS:
                np.testing.assert_array_equal(m.ev[f], 2 * once[f])
            cuts = sorted({min(c, E) for c in (0, 1, 63, 64, 65, 127, 128, 129, E)})
            for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
                m.recarve(tags, Tcw, "%s pairs %d .. %d" % (what, a, b), reset=(i == 0), first=a, count=b - a)
            if len(cuts) > 1:
                for f in COUNTERS:  # additive over the split
                    np.testing.assert_array_equal(m.ev[f], once[f], err_msg=what + " split")
            got = m.recarve(tags, Tcw, what + " an empty range", reset=False, first=E, count=0)
            assert list(got.values()) == [0] * 7
            m.recarve(tags, Tcw, what + " an empty range with reset", reset=True, first=E // 2, count=0)
            assert not m.ev["crossings"].any() and not m.ev["ends"].any()
            seen["hit"] += whole["cells_hit"]
            seen["skipped"] += whole["rays_skipped"]
            seen["unposed"] += whole["pairs_unposed"]
            seen["rays"] += whole["rays_total"]
        tags, Tcw = table(37)
        m.recarve(tags, Tcw, "short rays only", max_steps=900, end_margin=0)
        m.recarve(tags, Tcw, "a margin beyond most rays", reset=False, end_margin=1000)
        if E >= 63:
            assert min(seen.values()) > 0, seen
    finally:
        eng.close()


# 2. the crafted rays: N == max_steps and max_steps + 1, end_margin 0, 1 and beyond N, a centre in the point's own cell, an
# entry with no pairs, a tag absent from the table
def test_crafted_rays(pkg, gpu_ok):
    eng = pkg.Engine(32, 24, 1)
    rec, pairs, tags, Tcw = crafted_case()
    try:
        eng.vmap_open(1.0)
        m = Model(eng, rec, pairs, 1.0)
        got = m.recarve(tags, Tcw, "margin 0", end_margin=0, max_steps=64)
        assert m.ev["crossings"].tolist() == [0, 6, 5, 3, 2, 1, 0, 0, 10, 0, 0, 0] and m.ev["ends"].tolist() == [1] * 11 + [0]
        assert got["ends_hit"] == 11 and got["rays_skipped"] == 0
        m.recarve(tags, Tcw, "margin 1", end_margin=1, max_steps=64)
        assert m.ev["crossings"].tolist() == [0, 5, 4, 2, 1, 0, 0, 0, 8, 0, 0, 0]
        assert m.recarve(tags, Tcw, "N == max_steps", end_margin=0, max_steps=6)["rays_skipped"] == 0
        assert m.recarve(tags, Tcw, "N == max_steps + 1", end_margin=0, max_steps=5)["rays_skipped"] == 1
        assert m.ev["ends"][0] == 0
        for margin in (6, 7, 1000):
            got = m.recarve(tags, Tcw, "margin %d" % margin, end_margin=margin, max_steps=64)
            assert got["cells_visited"] == 0 and got["ends_hit"] == 11
        got = m.recarve([3], Tcw, "a tag absent from the table", end_margin=0, max_steps=64)
        assert (got["pairs_unposed"], got["rays_total"]) == (11, 0) and not m.ev["ends"].any()
        got = m.recarve([], np.zeros((0, 12), F), "no table", reset=False)
        assert got["pairs_unposed"] == 11
    finally:
        eng.close()


# 3. where every multiplicity is 1 a recarve of the whole log is the carve: keyframe 0 of every golden fixture, integrated,
# observed and carved alone with its neighbour row, engine against engine and both against the pinned totals
@pytest.mark.parametrize("name", gu.fixture_names())
def test_recarve_of_the_whole_log_is_the_carve(engines, name):
    g, eng = engines(name)
    rows = np.ascontiguousarray(g["nbrs"][:, :3])
    eng.vmap_open(EQ_VOXEL)
    try:
        eng.vmap_integrate([0], updated=False, **KW)
        eng.vmap_observe([0], rows[[0]], **KW)
        carved = eng.vmap_carve([0], rows[[0]], EQ_MARGIN, EQ_STEPS, **KW)
        ev0 = {f: np.array(a) for f, a in eng.vmap_fetch_evidence().items()}
        M = eng.vmap_info()["voxels"]
        assert M == carved["plain_total"] == PINNED[name][0] and (eng.vmap_fetch(fields=("multiplicity",))["multiplicity"] == 1).all()
        tags = np.unique(np.append(rows[0], 0)).astype(np.int32)
        got = eng.vmap_recarve(tags, [g["Tcw"][k] for k in tags], EQ_MARGIN, EQ_STEPS, reset=True)
        print(name, got)
        same_fetch(eng.vmap_fetch_evidence(), ev0, name + ": the recarve's counters against the carve's")
        for f in ("rays_total", "rays_skipped", "cells_visited", "cells_hit", "ends_hit"):
            assert got[f] == carved[f], (f, got, carved)
        assert got["pairs_unposed"] == 0 and got["pairs_total"] == eng.vmap_obs_info()["observations"]
        assert (M, got["rays_total"], got["cells_visited"], got["cells_hit"], got["ends_hit"]) == PINNED[name]
    finally:
        eng.vmap_close()


CLOUD = dict(fields=("xyz", "pixel", "rho_sigma", "intensity"), **KW)


def others(eng, refs, voxel):
    """what a recarve must leave alone: the map, the log, the lists, the flags, the infos -- and the merged cloud"""
    return full_state(eng), eng.extract_points_voxel(refs, voxel, **CLOUD)


def same_others(eng, before, refs, voxel, what):
    st, cloud = before
    state_unchanged(eng, st[:4] + (eng.vmap_fetch_evidence(),) + st[5:], what)   # (everything but the counters)
    same_fetch(eng.extract_points_voxel(refs, voxel, **CLOUD), cloud, what)


# 4. the loop-closure recipe: repose, recarve with the same table, classify
def test_loop_closure_recipe(pkg, engines):
    name = "plane_64x48_n7"
    g, eng = engines(name)
    refs = list(range(g["n_kf"]))
    rows = np.ascontiguousarray(g["nbrs"][:, :3])
    kfs = [0, 1, 2]
    B = pkg.Engine(32, 24, 1)
    eng.vmap_open(0.02)
    try:
        for k in kfs:
            eng.vmap_integrate([k], updated=False, **KW)
            eng.vmap_observe([k], rows[[k]], **KW)
            eng.vmap_carve([k], rows[[k]], 1, 4096, **KW)
        poses = np.array([perturbed(g["Tcw"][k], k) for k in kfs], F).reshape(3, 12)
        for k, T in zip(kfs, poses):
            eng.set_pose(k, T)
        d = eng.vmap_repose(kfs, np.tile(g["K"], (3, 1)), poses, carry=False, remap=False)
        assert d["moved"] > 0 and not any(a.any() for a in eng.vmap_fetch_evidence().values())
        before = others(eng, refs, 0.02)
        got = eng.vmap_recarve(kfs, poses)
        same_others(eng, before, refs, 0.02, "the map, the log, the lists, the flags, the infos and the merged cloud")
        # the counters: the restatement on the fetched records and log
        rec, log = eng.vmap_fetch(), eng.vmap_fetch_observations()
        exp = vr.recarve(vr.map_index(rec["xyz"], 0.02), rec["xyz"], log["entry"], log["tag"], kfs, poses, 0.02)
        assert got == {f: exp[f] for f in vr.OUTS}, (got, {f: exp[f] for f in vr.OUTS})
        ev = eng.vmap_fetch_evidence()
        same_fetch(ev, {f: exp[f] for f in COUNTERS}, "against the restatement")
        print(name, got)
        assert got["cells_hit"] > 0 and got["rays_total"] > 0 and got["ends_hit"] == got["rays_total"] - got["rays_skipped"]
        # a second engine that imports the reposed records and log and recarves
        B.vmap_open(0.02)
        assert (B.vmap_import({f: rec[f] for f in RECORD}, updated=False)["dst_ids"] == np.arange(len(rec["pixel"]))).all()
        B.vmap_import_observations(log["entry"], log["tag"])
        assert B.vmap_recarve(kfs[::-1], poses[::-1]) == got
        same_fetch(B.vmap_fetch_evidence(), ev, "against the second engine")
        # classify sees the new counters
        rule = dict(min_ends=2)
        vm, ol = build({f: rec[f] for f in RECORD}, log, 0.02)
        want = vcl.Classifier().classify(vm, ev["crossings"], ev["ends"], np.diff(ol.cameras(vm.M)[0]), vcl.rule_of(**rule), True)
        mine = eng.vmap_classify(rule, True, ids=False)
        assert mine["published_total"] == want["published_total"] > 0
    finally:
        B.close()
        eng.vmap_close()
        for k in refs:  # the shared engine gets its poses and planes back
            eng.set_pose(k, np.array(g["Tcw"][k], F))
        eng.pointset(refs, source=1)


# 5. state: the counters survive a rehash and a record growth forced between two recarves; clear zeroes them
def test_counters_survive_growth_and_clear(pkg, gpu_ok):
    eng = pkg.Engine(32, 24, 1)
    rec1, pairs1 = synthetic_case(65, 700)
    rec2, pairs2 = synthetic_case(2049, 5000)
    rec2 = dict(rec2, xyz=rec2["xyz"] + np.array([300 * VOXEL, 0, 0], F))   # voxels of their own, beside the first map's
    tags, Tcw = table(37)
    try:
        eng.vmap_open(VOXEL)
        m = Model(eng, rec1, pairs1, VOXEL)
        m.recarve(tags, Tcw, "the small map")
        assert m.ev["crossings"].any()
        info0 = eng.vmap_info()
        # the second import rehashes the table and grows the records; the counters come along, new entries read 0
        both = {f: np.concatenate([rec1[f], rec2[f]]) for f in rec1}
        allp = {"entry": np.concatenate([pairs1["entry"], pairs2["entry"] + np.uint32(65)]),
                "tag": np.concatenate([pairs1["tag"], pairs2["tag"]])}
        eng.vmap_import(rec2, updated=False)
        eng.vmap_import_observations(pairs2["entry"] + np.uint32(65), pairs2["tag"])
        assert eng.vmap_info()["rehashes"] > info0["rehashes"] and eng.vmap_info()["voxels"] == 65 + 2049
        m.vm, m.ol = build(both, allp, VOXEL)
        m.same_evidence("after the growth")
        m.recarve(tags, Tcw, "the new pairs on top", reset=False, first=700)
        m.recarve(tags, Tcw, "the old pairs once more", reset=False, first=0, count=700)
        eng.vmap_clear()
        m = Model(eng, rec1, pairs1, VOXEL)
        m.same_evidence("after clear")
        m.recarve(tags, Tcw, "after clear", reset=False)
    finally:
        eng.close()


# 6. refusals: every SDM_EINVAL and SDM_ESTATE case leaves a snapshot of the whole state unchanged
def test_refusals(pkg, gpu_ok):
    b = sys.modules[pkg.__name__ + ".binding"]
    eng = pkg.Engine(32, 24, 1)
    lib, ctx = eng.lib, eng.ctx
    rec, pairs = synthetic_case(65, 700)
    tags, Tcw = table(37)
    Tcw = np.ascontiguousarray(Tcw, F)
    ip, fp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_float)

    def call(n=37, tg=tags, t=Tcw, **kw):
        rc = b.VmapRecarveArgs()
        rc.end_margin, rc.max_steps, rc.reset, rc.first, rc.count = 1, 4096, 1, 0, -1
        for f in b.VMAP_RECARVE_OUTS:
            setattr(rc, f, 9)
        for f, v in kw.items():
            setattr(rc, f, v)
        code = lib.sdm_vmap_recarve(ctx, n, None if tg is None else tg.ctypes.data_as(ip), None if t is None else t.ctypes.data_as(fp),
                                    ctypes.byref(rc))
        return code, rc

    try:
        code, rc = call()
        assert code == ESTATE and b"no open voxel map" in lib.sdm_last_error()
        assert [getattr(rc, f) for f in b.VMAP_RECARVE_OUTS] == [0] * 7
        eng.vmap_open(VOXEL)
        m = Model(eng, rec, pairs, VOXEL)
        m.recarve(tags, Tcw, "before the refusals")
        eng.vmap_classify(dict(min_ends=1), True, ids=False)
        assert m.ev["crossings"].any() and eng.vmap_class_info()["published"] > 0
        st = full_state(eng)

        def refused(res, word, what):
            code, rc = res
            assert code == EINVAL and word in lib.sdm_last_error(), (what, code, lib.sdm_last_error())
            assert [getattr(rc, f) for f in b.VMAP_RECARVE_OUTS] == [0] * 7, what
            state_unchanged(eng, st, what)

        assert lib.sdm_vmap_recarve(ctx, 37, tags.ctypes.data_as(ip), Tcw.ctypes.data_as(fp), None) == EINVAL
        state_unchanged(eng, st, "null rc")
        refused(call(-1), b"negative n_poses", "n_poses < 0")
        refused(call(tg=None), b"null pose table", "null tags")
        refused(call(t=None), b"null pose table", "null Tcw")
        neg, twice = tags.copy(), tags.copy()
        neg[20], twice[30] = -1, twice[3]
        refused(call(tg=neg), b"tag outside", "a negative tag")
        refused(call(tg=twice), b"listed twice", "a tag listed twice")
        refused(call(end_margin=-1), b"end_margin", "end_margin < 0")
        refused(call(max_steps=0), b"max_steps", "max_steps 0")
        refused(call(max_steps=65537), b"max_steps", "max_steps beyond SDM_FREESPACE_MAX_STEPS")
        refused(call(reset=2), b"reset", "reset 2")
        refused(call(reset=-1), b"reset", "reset -1")
        refused(call(first=-1), b"range beyond", "first < 0")
        refused(call(count=-2), b"range beyond", "count < -1")
        refused(call(first=1, count=700), b"range beyond", "first + count > E")
        refused(call(first=701), b"range beyond", "first > E")
        refused(call(first=1 << 62, count=1 << 62), b"range beyond", "a sum that overflows")
        with pytest.raises(ValueError):
            eng.vmap_recarve([1, 2], Tcw[:1])
        with pytest.raises(pkg.SdmError):
            eng.vmap_recarve(tags, Tcw, max_steps=0)
        state_unchanged(eng, st, "binding refusals")
        # the edges that are no refusals, and the map still works
        assert eng.vmap_recarve(tags, Tcw, max_steps=65536, reset=False, first=700, count=0)["pairs_total"] == 0
        state_unchanged(eng, st, "an empty range without reset")
        m.recarve(tags, Tcw, "after the refusals", reset=False, first=699, count=None)
    finally:
        eng.close()
