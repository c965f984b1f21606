"""GPU: importing records and observations into the persistent voxel map (sdm_vmap_import, sdm_vmap_import_observations /
Engine.vmap_import, .vmap_import_observations, shard.vmap_allgather_merge) against tests/vmap_import_np.py -- after every
call the delta, dst_ids, updated_ids, both infos, a full fetch of the map, the log and all camera lists.  Everything is an
integer or copied bits: every comparison is for equality.

Not run here: the refusals M + R > 2^30 and E + P > 2^30, which no source a test can afford reaches."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import golden_util as gu
import vmap_import_np as vi
import vmap_np
import vmap_obs_np as vo
from test_gpu_extract import EINVAL, ESTATE, _state, pipeline
from test_gpu_shard import _free_port
from test_gpu_vmap import INFO, same_fetch, same_info, snapshot, unchanged
from test_gpu_vmap_obs import Mirror, both, obs_snapshot, obs_unchanged, same_obs, step
from test_vmap_cpu import make_cloud, part
from test_vmap_import_cpu import PINNED_MERGE, make_records
from test_vmap_obs_cpu import FINAL_M, PINNED
from test_voxcam_cpu import N_SHORT

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SAT = (1 << 32) - 1
NOID = 0xFFFFFFFF
KW = dict(max_sigma=0.3)
RECORD_FIELDS = ("xyz", "pixel", "rho_sigma", "intensity", "tag", "multiplicity")
_TORCH = {"xyz": torch.float32, "rho_sigma": torch.float32, "intensity": torch.uint8}


def to_device(arrays):
    """{field: host array} as torch tensors on the GPU (32-bit integers as int32: the same bits)"""
    out = {}
    for f, a in arrays.items():
        a = np.ascontiguousarray(a)
        if a.dtype in (np.uint32, np.int32):
            a = a.view(np.int32)
        out[f] = torch.from_numpy(a.copy()).cuda()
    return out


def to_host(t, dt):
    return t.cpu().numpy().view(dt)


def check_import(eng, ref, rec, what="", device=False, dst_ids=True, updated=True):
    """one sdm_vmap_import against the restatement: delta, dst_ids, updated_ids, info and a full fetch"""
    exp = vi.import_records(ref.vm, rec)
    got = eng.vmap_import(to_device(rec) if device else rec, dst_ids=dst_ids, updated=updated)
    assert {f: got[f] for f in vi.DELTA} == {f: exp[f] for f in vi.DELTA}, (what, got, exp)
    for f, want in (("dst_ids", dst_ids), ("updated_ids", updated)):
        if want is False:
            assert f not in got
            continue
        mine = to_host(got[f], np.uint32) if device else got[f]
        assert mine.dtype == np.uint32
        np.testing.assert_array_equal(mine, exp[f], err_msg="%s %s" % (what, f))
    same_info(eng, ref.vm, what)
    same_fetch(eng.vmap_fetch(), ref.vm.fetch(), what)
    return got, exp


def check_pairs(eng, ref, entry, tag, entry_map=None, what="", device=False):
    """one sdm_vmap_import_observations against the restatement: the outs, the info, the log and every camera list"""
    exp = vi.import_observations(ref.ol, ref.vm.M, entry, tag, entry_map)
    if device:
        d = to_device({"entry": np.asarray(entry, np.uint32), "tag": np.asarray(tag, np.int32)})
        m = None if entry_map is None else (entry_map if torch.is_tensor(entry_map) else to_device({"m": np.asarray(entry_map, np.uint32)})["m"])
        got = eng.vmap_import_observations(d["entry"], d["tag"], m)
    else:
        got = eng.vmap_import_observations(entry, tag, entry_map)
    assert got == exp, (what, got, exp)
    same_obs(eng, ref, what)
    return got


@pytest.fixture(scope="module")
def trios(pkg, gpu_ok):
    """per golden fixture three engines that ran the pipeline: rank 0, rank 1 and the one that sees everything"""
    made = {}

    def get(name):
        if name not in made:
            g = gu.load(name)
            made[name] = (g, [pipeline(pkg, g) for _ in range(3)])
        return made[name]

    yield get
    for _, engs in made.values():
        for e in engs:
            e.close()


def run_keyframes(eng, ref, g, kfs):
    """one integrate-then-observe per keyframe with the short neighbour rows, engine and restatement side by side"""
    for k in kfs:
        row = np.ascontiguousarray(g["nbrs"][[k]][:, :N_SHORT])
        both(eng, ref, [k], **KW)
        assert eng.vmap_observe([k], row, **KW) == ref.observe(eng, [k], row, **KW)
    same_fetch(eng.vmap_fetch(), ref.vm.fetch(), "keyframes")
    same_obs(eng, ref, "keyframes")


# 1. the golden fixtures' two-rank recipe: two engines in one process, host arrays and device to device
@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
@pytest.mark.parametrize("name", gu.fixture_names())
def test_golden_two_rank_merge(trios, name, device):
    g, (A, B, C) = trios(name)
    n, voxel = g["n_kf"], 0.02
    for e in (A, B, C):
        e.vmap_open(voxel)
    try:
        ra, rb, rc = Mirror(voxel), Mirror(voxel), Mirror(voxel)
        run_keyframes(A, ra, g, range(0, n // 2))
        run_keyframes(B, rb, g, range(n // 2, n))
        run_keyframes(C, rc, g, range(n))
        m1, e1 = B.vmap_info()["voxels"], B.vmap_obs_info()["observations"]
        if device:  # engine B's fetch goes into torch tensors that engine A imports
            rec = {f: torch.empty((m1, 3) if f == "xyz" else (m1, 2) if f == "rho_sigma" else (m1,), dtype=_TORCH.get(f, torch.int32),
                                  device="cuda") for f in RECORD_FIELDS}
            B.vmap_fetch(out=rec)
            log = {f: torch.empty(e1, dtype=torch.int32, device="cuda") for f in ("entry", "tag")}
            B.vmap_fetch_observations(out=log)
            exp = vi.import_records(ra.vm, rb.vm.fetch())
            got = A.vmap_import(rec)
            dst = got["dst_ids"]
            assert dst.is_cuda
            np.testing.assert_array_equal(to_host(dst, np.uint32), exp["dst_ids"])
            np.testing.assert_array_equal(to_host(got["updated_ids"], np.uint32), exp["updated_ids"])
            assert {f: got[f] for f in vi.DELTA} == {f: exp[f] for f in vi.DELTA}
            same_info(A, ra.vm, name)
            same_fetch(A.vmap_fetch(), ra.vm.fetch(), name)
            oexp = vi.import_observations(ra.ol, ra.vm.M, rb.ol.entry, rb.ol.tag, exp["dst_ids"])
            ogot = A.vmap_import_observations(log["entry"], log["tag"], dst)
            assert ogot == oexp
            same_obs(A, ra, name)
        else:
            rec = B.vmap_fetch()
            log = B.vmap_fetch_observations()
            got, exp = check_import(A, ra, {f: rec[f] for f in RECORD_FIELDS}, name)
            ogot = check_pairs(A, ra, log["entry"], log["tag"], got["dst_ids"], name)
        figures = (m1, got["created"], got["updated"], e1, ogot["created"])
        print(name, "device" if device else "host", figures)
        assert figures == PINNED_MERGE[name]
        assert got["dropped"] == 0 and ogot["rejected"] == 0
        # the third engine integrated and observed everything: every field but epoch, and every camera list
        assert A.vmap_info()["voxels"] == C.vmap_info()["voxels"] == FINAL_M[name]
        assert A.vmap_info()["points"] == C.vmap_info()["points"]
        assert A.vmap_obs_info()["observations"] == C.vmap_obs_info()["observations"] == PINNED[name][0]
        same_fetch(A.vmap_fetch(), C.vmap_fetch(), name + " against the one-map run", skip=("epoch",))
        same_fetch(A.vmap_fetch_cameras(), C.vmap_fetch_cameras(), name + " camera lists against the one-map run")
    finally:
        for e in (A, B, C):
            e.vmap_close()


# 2. crafted sources: the sizes around one tile, the saturation case, optional sources, the destinations' three forms
def test_crafted_sizes_and_call_variants(pkg, gpu_ok):
    rng = np.random.default_rng(11)
    eng = pkg.Engine(32, 24, 1)
    try:
        eng.vmap_open(0.25)
        ref = Mirror(0.25)
        seen = dict(dropped=0, updated=0)
        for i, R in enumerate((0, 1, 2047, 2048, 2049, 2050)):
            rec = make_records(rng, R) if R >= 40 else {f: v[:R] for f, v in make_records(rng, 40).items()}
            got, _ = check_import(eng, ref, rec, "R = %d" % R, device=bool(i & 1))
            assert got["total"] == R
            seen["dropped"] += got["dropped"]
            seen["updated"] += got["updated"]
        assert seen["dropped"] > 0 and seen["updated"] > 0 and eng.vmap_info()["calls"] == 6
        M = ref.vm.M
        for i, P in enumerate((0, 1, 2047, 2048, 2049, 2050)):
            entry = rng.integers(0, M + 20, P).astype(np.uint32)
            tag = rng.integers(-2, 30, P).astype(np.int32)
            emap = None
            if i >= 3:  # through a map that carries dropped records and is shorter than some entries
                emap = rng.integers(0, M + 5, M + 10).astype(np.uint32)
                emap[rng.integers(0, len(emap), 9)] = NOID
            got = check_pairs(eng, ref, entry, tag, emap, "P = %d" % P, device=bool(i & 1))
            assert got["total"] == P and (P < 2000 or (got["rejected"] > 0 and got["created"] > 0))
        assert eng.vmap_obs_info()["calls"] == 6
        assert check_pairs(eng, ref, entry, tag, emap, "the same pairs again")["created"] == 0

        # saturation: two records of 2^31 + 1 in one voxel in one call
        eng.vmap_clear()
        ref.clear()
        big = (1 << 31) + 1
        sat = {"xyz": np.array([[0.1, 0.1, 0.1], [0.12, 0.1, 0.1], [0.9, 0.9, 0.9]], F), "rho_sigma": np.array([[1, 0.1]] * 3, F),
               "multiplicity": np.array([big, big, 5], np.uint32)}
        check_import(eng, ref, sat, "saturation")
        mult = eng.vmap_fetch(fields=("multiplicity",))["multiplicity"].tolist()
        assert mult == [SAT, 5] and (big + big) & SAT == 2 != SAT
        assert eng.vmap_info()["points"] == 2 * big + 5
        check_import(eng, ref, sat, "saturated stays saturated", device=True)
        check_import(eng, ref, {"xyz": sat["xyz"][2:], "rho_sigma": sat["rho_sigma"][2:], "multiplicity": np.array([SAT - 9], np.uint32)},
                     "clamps across calls")
        assert eng.vmap_fetch(fields=("multiplicity",))["multiplicity"].tolist() == [SAT, SAT]

        # NULL optional sources (zeros, multiplicity 1) and the three forms of the destinations
        eng.vmap_clear()
        ref.clear()
        rec = make_records(rng, 3000)
        check_import(eng, ref, part(rec, 0, 1000), "all sources")
        bare = {"xyz": rec["xyz"][1000:2000], "rho_sigma": rec["rho_sigma"][1000:2000]}
        got, _ = check_import(eng, ref, bare, "required sources only", dst_ids=False, updated=False)
        assert got["updated"] > 0
        check_import(eng, ref, {"xyz": rec["xyz"][2000:], "rho_sigma": rec["rho_sigma"][2000:], "tag": rec["tag"][2000:]},
                     "device destinations", device=True)
        mine = np.full(1000, 7, np.uint32)
        got, exp = check_import(eng, ref, part(rec, 0, 1000), "caller's dst_ids, no updated_ids", dst_ids=mine, updated=False)
        assert got["dst_ids"] is not None and np.array_equal(mine, exp["dst_ids"])
    finally:
        eng.close()


# 3. a device-generated source beyond 2048 x 2048 records and pairs: the second scan level
def test_second_scan_level(pkg, gpu_ok):
    R = 2048 * 2048 + 2049
    eng = pkg.Engine(32, 24, 1)
    try:
        eng.vmap_open(0.5, 4096)
        ref = Mirror(0.5)
        i = torch.arange(R, dtype=torch.int64, device="cuda")
        cell = (i * 2654435761) % 3001  # a few thousand distinct voxels, every one met about 1400 times
        xyz = torch.stack([(cell % 17).float() * 0.5 + 0.25, ((cell // 17) % 17).float() * 0.5 - 3.75, (cell // 289).float() * 0.5 + 0.25], 1)
        sigma = ((i * 40503) % 1009).float() * 1e-4 + 0.001
        rec = {"xyz": xyz.contiguous(), "rho_sigma": torch.stack([torch.ones_like(sigma), sigma], 1).contiguous(),
               "pixel": (i % (1 << 26)).int(), "intensity": (i % 251).to(torch.uint8), "tag": (i % 37).int(),
               "multiplicity": (1 + i % 3).int()}
        host = {f: to_host(t, {"pixel": np.uint32, "multiplicity": np.uint32, "tag": np.int32}.get(f, t.cpu().numpy().dtype))
                for f, t in rec.items()}
        eng.vmap_import(part(host, 0, 1000))  # some entries exist: the big call creates AND updates
        vi.import_records(ref.vm, part(host, 0, 1000))
        exp = vi.import_records(ref.vm, host)
        got = eng.vmap_import(rec)
        assert {f: got[f] for f in vi.DELTA} == {f: exp[f] for f in vi.DELTA}
        assert got["total"] == R and got["created"] > 0 and got["updated"] > 0 and ref.vm.M == 3001
        assert int(exp["dst_ids"][-1]) != NOID  # the last tile's records were placed
        np.testing.assert_array_equal(to_host(got["dst_ids"], np.uint32), exp["dst_ids"])
        np.testing.assert_array_equal(to_host(got["updated_ids"], np.uint32), exp["updated_ids"])
        same_info(eng, ref.vm, "big import")
        same_fetch(eng.vmap_fetch(), ref.vm.fetch(), "big import")
        # the same number of pairs, most of them repeats, through the import's own dst_ids
        entry, tag = (i % R).int(), ((i * 7919) % 53).int() - 1
        oexp = vi.import_observations(ref.ol, ref.vm.M, to_host(entry, np.uint32), to_host(tag, np.int32), exp["dst_ids"])
        ogot = eng.vmap_import_observations(entry, tag, got["dst_ids"])
        assert ogot == oexp and ogot["rejected"] > 0 and ogot["created"] > 3001
        same_obs(eng, ref, "big pair import")
    finally:
        eng.close()


# 4. an import that forces a rehash and record growth on a map that holds evidence, observations and published flags
def test_growth_keeps_evidence_observations_and_flags(pkg, gpu_ok):
    g = gu.load("plane_64x48_n7")
    eng = pipeline(pkg, g)
    try:
        refs = list(range(g["n_kf"]))
        eng.vmap_open(0.02)
        ref = Mirror(0.02)
        for k in refs:
            both(eng, ref, [k], **KW)
            step(eng, ref, [k], g["nbrs"][[k]], **KW)
        eng.vmap_carve(refs, g["nbrs"], **KW)
        d = eng.vmap_classify({"min_multiplicity": 2}, commit=True)
        ev0 = {f: np.array(a) for f, a in eng.vmap_fetch_evidence().items()}
        pub0, cams0 = np.array(eng.vmap_fetch_published()), {f: np.array(a) for f, a in eng.vmap_fetch_cameras().items()}
        info0, M0 = eng.vmap_info(), ref.vm.M
        assert ev0["crossings"].any() and ev0["ends"].any() and 0 < d["accepted"] == int(pub0.sum()) < M0
        rng = np.random.default_rng(5)
        R = 4 * info0["table_slots"]
        rec = make_records(rng, R, nasty=False, spread=40.0)  # far more new voxels than the table and the records hold
        rec["xyz"][:500] = eng.vmap_fetch(fields=("xyz",))["xyz"][:500]  # and some records of existing entries
        got, _ = check_import(eng, ref, rec, "growing import")
        info = eng.vmap_info()
        assert info["rehashes"] > info0["rehashes"] and got["created"] > info0["table_slots"] and info["voxels"] == M0 + got["created"]
        ev, pub, cams = eng.vmap_fetch_evidence(), eng.vmap_fetch_published(), eng.vmap_fetch_cameras()
        for f in ev0:
            assert np.array_equal(ev[f][:M0], ev0[f]) and not ev[f][M0:].any(), f
        assert np.array_equal(pub[:M0], pub0) and not pub[M0:].any()
        assert np.array_equal(cams["cam_offsets"][:M0 + 1], cams0["cam_offsets"]) and np.array_equal(cams["cam_tags"], cams0["cam_tags"])
        assert (cams["cam_offsets"][M0:] == cams0["cam_offsets"][-1]).all()  # the new entries' lists are empty
        same_obs(eng, ref, "after the growth")
        assert eng.vmap_class_info()["published"] == int(pub0.sum())
        # observations on the new entries; then the map still integrates, observes, carves and classifies
        check_pairs(eng, ref, np.arange(M0 - 5, M0 + 300, dtype=np.uint32), np.full(305, 77, np.int32), None, "pairs on new entries")
        both(eng, ref, [0], **KW)
        step(eng, ref, [0], g["nbrs"][[0]], **KW)
        eng.vmap_carve([0], g["nbrs"][[0]], **KW)
        assert eng.vmap_classify({"min_multiplicity": 2}, commit=True)["examined"] == ref.vm.M
    finally:
        eng.close()


# 5. I1 split invariance and I3 round trip on the device, determinism over repeated runs, and no side effect on the engine
def test_invariants_determinism_and_side_effects(pkg, gpu_ok):
    g = gu.load("plane_64x48_n7")
    eng = pipeline(pkg, g)
    other = pkg.Engine(32, 24, 1)
    try:
        refs = list(range(g["n_kf"]))
        before = _state(eng, refs)
        stats0 = eng.get_stats(reset=False)
        rng = np.random.default_rng(21)
        rec = make_records(rng, 6000)
        entry, tag = rng.integers(0, 900, 9000).astype(np.uint32), rng.integers(-1, 12, 9000).astype(np.int32)
        runs = []
        for cuts in ([], [], [], [1, 2048, 2049, 5999], [3000]):  # three identical runs, then two splits
            eng.vmap_open(0.25)
            ref = Mirror(0.25)
            both(eng, ref, refs[:3], **KW)
            dst, upd = [], []
            for a, b in zip([0] + cuts, cuts + [6000]):
                got, _ = check_import(eng, ref, part(rec, a, b), "cut %d" % a, device=bool(len(cuts) & 1))
                dst.append(np.asarray(to_host(got["dst_ids"], np.uint32) if torch.is_tensor(got["dst_ids"]) else got["dst_ids"]))
                upd.append(got["updated_ids"])
            pc = [0] + [c * 3 // 2 for c in cuts] + [9000]
            for a, b in zip(pc[:-1], pc[1:]):
                check_pairs(eng, ref, entry[a:b], tag[a:b], None, "pairs %d" % a)
            full = eng.vmap_fetch()
            runs.append((np.concatenate(dst), {f: np.array(v) for f, v in full.items() if f != "epoch"}, eng.vmap_info()["voxels"],
                         eng.vmap_info()["points"], obs_snapshot(eng)[1:], upd if not cuts else None, np.array(full["epoch"])))
            if not cuts and len(runs) == 1:  # I3: the map's own full fetch into an empty map reproduces it, ids included
                other.vmap_open(0.25)
                back = other.vmap_import({f: full[f] for f in RECORD_FIELDS})
                assert back["created"] == len(full["pixel"]) and np.array_equal(back["dst_ids"], np.arange(len(full["pixel"])))
                same_fetch(other.vmap_fetch(), full, "round trip", skip=("epoch",))
                # (`points` is the sum of what the records carry: the source's own count is larger where one saturated)
                assert other.vmap_info()["points"] == int(full["multiplicity"].astype(np.int64).sum()) < eng.vmap_info()["points"]
                assert (other.vmap_fetch()["epoch"] == 1).all()
                other.vmap_close()
            eng.vmap_close()
        first = runs[0]
        for k, run in enumerate(runs[1:], 1):
            assert np.array_equal(run[0], first[0]), k
            same_fetch(run[1], first[1], "run %d" % k)
            assert run[2:4] == first[2:4]
            same_fetch(run[4][0], first[4][0], "log of run %d" % k)
            same_fetch(run[4][1], first[4][1], "lists of run %d" % k)
            if k < 3:  # identical calls: updated_ids and epoch too
                assert np.array_equal(np.asarray(to_host(run[5][0], np.uint32) if torch.is_tensor(run[5][0]) else run[5][0]),
                                      np.asarray(first[5][0]))
                assert np.array_equal(run[6], first[6])
        for x, y in zip(before, _state(eng, refs)):  # no plane, list or counter of the engine moved
            np.testing.assert_array_equal(x, y)
        assert eng.get_stats(reset=False) == stats0
    finally:
        eng.close()
        other.close()


# 6. every refusal, each with the proof that nothing changed
def test_refusals_change_nothing(pkg, gpu_ok):
    b = sys.modules[pkg.__name__ + ".binding"]
    eng = pkg.Engine(32, 24, 1)
    lib, ctx = eng.lib, eng.ctx
    rng = np.random.default_rng(3)
    rec = make_records(rng, 500)
    keep = {f: np.ascontiguousarray(rec[f]) for f in RECORD_FIELDS}
    dev = to_device(keep)

    def structs(src=keep, on_device=0, cap=500):
        pb, vf, d = b.PointBuffers(), b.VmapFields(), b.VmapImportDelta()
        for f in ("xyz", "pixel", "rho_sigma", "intensity"):
            setattr(pb, f, src[f].data_ptr() if on_device else src[f].ctypes.data)
        vf.tag = src["tag"].data_ptr() if on_device else src["tag"].ctypes.data
        vf.multiplicity = src["multiplicity"].data_ptr() if on_device else src["multiplicity"].ctypes.data
        pb.capacity, pb.on_device = cap, on_device
        return pb, vf, d

    def call(pb, vf, d, count=500):
        return lib.sdm_vmap_import(ctx, ctypes.byref(pb) if pb is not None else None, ctypes.byref(vf) if vf is not None else None,
                                   count, ctypes.byref(d) if d is not None else None)

    try:
        pb, vf, d = structs()
        d.total = d.created = 9
        assert call(pb, vf, d) == ESTATE and b"no open voxel map" in lib.sdm_last_error() and (d.total, d.created) == (0, 0)
        io = b.VmapObsImport()
        ent, tg = np.arange(10, dtype=np.uint32), np.zeros(10, np.int32)
        io.entry, io.tag = ent.ctypes.data, tg.ctypes.data
        assert lib.sdm_vmap_import_observations(ctx, 10, ctypes.byref(io)) == ESTATE
        eng.vmap_open(0.25)
        eng.vmap_import(part(keep, 0, 300))
        eng.vmap_import_observations(np.arange(50, dtype=np.uint32), np.arange(50, dtype=np.int32))
        snap, osnap = snapshot(eng), obs_snapshot(eng)
        M = snap[0]["voxels"]
        guard = np.full(600, 0x5A5A5A5A, np.uint32)

        def refused(rc, word, d=None, what=""):
            assert rc == EINVAL and word in lib.sdm_last_error(), (what, rc, lib.sdm_last_error())
            if d is not None:
                assert (d.dropped, d.created, d.updated) == (0, 0, 0), what
            unchanged(eng, snap, what)
            obs_unchanged(eng, osnap, what)
            assert (guard == 0x5A5A5A5A).all(), what

        assert call(None, None, None) == EINVAL  # a NULL src
        unchanged(eng, snap, "null src")
        for f in ("xyz", "rho_sigma"):  # a NULL required source
            pb, vf, d = structs()
            setattr(pb, f, None)
            d.dst_ids = guard.ctypes.data
            refused(call(pb, vf, d), b"null source", d, f)
        pb, vf, d = structs()
        refused(call(pb, vf, d, -1), b"negative", d, "count < 0")
        pb, vf, d = structs(cap=499)
        refused(call(pb, vf, d), b"count exceeds capacity", d, "count > capacity")
        pb, vf, d = structs(cap=-1)
        refused(call(pb, vf, d, 0), b"negative", d, "capacity < 0")
        for f in ("xyz", "pixel", "rho_sigma", "tag", "multiplicity"):  # a misaligned device source
            pb, vf, d = structs(dev, 1)
            tgt = vf if f in ("tag", "multiplicity") else pb
            setattr(tgt, f, getattr(tgt, f) + (4 if f == "rho_sigma" else 2))
            refused(call(pb, vf, d, 400), b"not aligned", d, "misaligned " + f)
        ids_dev = torch.zeros(600, dtype=torch.int32, device="cuda")
        for f in ("dst_ids", "updated_ids"):  # a misaligned device destination
            pb, vf, d = structs()
            d.on_device, d.updated_capacity = 1, 500
            setattr(d, f, ids_dev.data_ptr() + 2)
            refused(call(pb, vf, d), b"not aligned", d, "misaligned " + f)
        assert not ids_dev.any()
        pb, vf, d = structs()
        d.updated_ids, d.updated_capacity = guard.ctypes.data, min(M, 500) - 1
        refused(call(pb, vf, d), b"updated_capacity", d, "small updated_capacity")
        assert (d.total, d.first_created) == (500, M)  # filled, as in integrate
        d.updated_capacity = -1
        refused(call(pb, vf, d), b"negative capacity", d, "negative updated_capacity")

        def ocall(count=10, **kw):
            io = b.VmapObsImport()
            io.entry, io.tag = ent.ctypes.data, tg.ctypes.data
            for f, v in kw.items():
                setattr(io, f, v)
            io.total = io.created = 9
            return lib.sdm_vmap_import_observations(ctx, count, ctypes.byref(io)), io

        rc, io = ocall(-1)
        refused(rc, b"negative count", what="P < 0")
        assert (io.total, io.created) == (0, 0)
        refused(ocall(map_count=-1)[0], b"negative map_count", what="map_count < 0")
        refused(ocall(entry=None)[0], b"null source", what="null entry")
        refused(ocall(tag=None)[0], b"null source", what="null tag")
        refused(lib.sdm_vmap_import_observations(ctx, 10, None), b"null argument", what="null io")
        t = torch.zeros(16, dtype=torch.int32, device="cuda")
        for f in ("entry", "tag", "entry_map"):
            args = dict(entry=t.data_ptr(), tag=t.data_ptr(), entry_map=t.data_ptr(), map_count=16, on_device=1)
            args[f] += 2
            refused(ocall(**args)[0], b"not aligned", what="misaligned " + f)
        with pytest.raises(ValueError):
            eng.vmap_import({"xyz": keep["xyz"]})
        with pytest.raises(ValueError):
            eng.vmap_import({"xyz": keep["xyz"], "rho_sigma": dev["rho_sigma"]})
        with pytest.raises(ValueError):  # fields of different lengths are refused, not truncated
            eng.vmap_import({"xyz": keep["xyz"], "rho_sigma": keep["rho_sigma"], "tag": keep["tag"][:499]})
        unchanged(eng, snap, "binding refusals")
        # the map still works
        ref = Mirror(0.25)
        vi.import_records(ref.vm, part(keep, 0, 300))
        vi.import_observations(ref.ol, ref.vm.M, np.arange(50, dtype=np.uint32), np.arange(50, dtype=np.int32))
        check_import(eng, ref, keep, "after the refusals")
        check_pairs(eng, ref, ent, tg, None, "after the refusals")
    finally:
        eng.close()


# 6b. the forms of the C call the binding never makes: extra == NULL, delta == NULL, and sources and destinations on
# different sides
def test_raw_call_forms(pkg, gpu_ok):
    b = sys.modules[pkg.__name__ + ".binding"]
    eng = pkg.Engine(32, 24, 1)
    lib, ctx = eng.lib, eng.ctx
    rng = np.random.default_rng(8)
    rec = {f: np.ascontiguousarray(v) for f, v in make_records(rng, 2500).items()}
    try:
        eng.vmap_open(0.25)
        ref = Mirror(0.25)

        def buffers(src, on_device, fields=("xyz", "pixel", "rho_sigma", "intensity")):
            pb = b.PointBuffers()
            for f in fields:
                setattr(pb, f, src[f].data_ptr() if on_device else src[f].ctypes.data)
            pb.capacity, pb.on_device = len(src["pixel"]), on_device
            return pb

        def extras(src, on_device):
            vf = b.VmapFields()
            vf.tag = src["tag"].data_ptr() if on_device else src["tag"].ctypes.data
            vf.multiplicity = src["multiplicity"].data_ptr() if on_device else src["multiplicity"].ctypes.data
            return vf

        def after(exp, what, d=None, dst=None, upd=None):
            if d is not None:
                assert {f: getattr(d, f) for f in vi.DELTA} == {f: exp[f] for f in vi.DELTA}, what
                np.testing.assert_array_equal(dst[:len(exp["dst_ids"])], exp["dst_ids"], err_msg=what)
                np.testing.assert_array_equal(upd[:exp["updated"]], exp["updated_ids"], err_msg=what)
            same_info(eng, ref.vm, what)
            same_fetch(eng.vmap_fetch(), ref.vm.fetch(), what)

        # extra == NULL with a delta: tags read 0 and multiplicities 1
        one = part(rec, 0, 800)
        dst, upd, d = np.zeros(800, np.uint32), np.zeros(800, np.uint32), b.VmapImportDelta()
        d.dst_ids, d.updated_ids, d.updated_capacity = dst.ctypes.data, upd.ctypes.data, 800
        exp = vi.import_records(ref.vm, {f: one[f] for f in ("xyz", "pixel", "rho_sigma", "intensity")})
        assert lib.sdm_vmap_import(ctx, ctypes.byref(buffers(one, 0)), None, 800, ctypes.byref(d)) == 0
        after(exp, "extra == NULL", d, dst, upd)
        assert not ref.vm.fetch()["tag"].any() and exp["dropped"] > 0
        # delta == NULL: the map changes all the same
        two = {f: np.ascontiguousarray(v) for f, v in part(rec, 800, 1500).items()}
        exp = vi.import_records(ref.vm, two)
        assert lib.sdm_vmap_import(ctx, ctypes.byref(buffers(two, 0)), ctypes.byref(extras(two, 0)), 700, None) == 0
        after(exp, "delta == NULL")
        assert exp["created"] > 0 and exp["updated"] > 0
        # host sources, device destinations
        three = {f: np.ascontiguousarray(v) for f, v in part(rec, 1500, 2000).items()}
        tdst, tupd = torch.zeros(500, dtype=torch.int32, device="cuda"), torch.zeros(500, dtype=torch.int32, device="cuda")
        d = b.VmapImportDelta()
        d.dst_ids, d.updated_ids, d.updated_capacity, d.on_device = tdst.data_ptr(), tupd.data_ptr(), 500, 1
        exp = vi.import_records(ref.vm, three)
        assert lib.sdm_vmap_import(ctx, ctypes.byref(buffers(three, 0)), ctypes.byref(extras(three, 0)), 500, ctypes.byref(d)) == 0
        after(exp, "host sources, device destinations", d, to_host(tdst, np.uint32), to_host(tupd, np.uint32))
        assert exp["updated"] > 0
        # device sources, host destinations
        four = {f: np.ascontiguousarray(v) for f, v in part(rec, 2000, 2500).items()}
        fdev = to_device(four)
        dst, upd, d = np.zeros(500, np.uint32), np.zeros(500, np.uint32), b.VmapImportDelta()
        d.dst_ids, d.updated_ids, d.updated_capacity = dst.ctypes.data, upd.ctypes.data, 500
        exp = vi.import_records(ref.vm, four)
        assert lib.sdm_vmap_import(ctx, ctypes.byref(buffers(fdev, 1)), ctypes.byref(extras(fdev, 1)), 500, ctypes.byref(d)) == 0
        after(exp, "device sources, host destinations", d, dst, upd)
        assert exp["updated"] > 0 and eng.vmap_info()["calls"] == 4
    finally:
        eng.close()


# 7. two ranks on one GPU over gloo: rank 0's merged map and lists equal the single-engine run
def test_sharded_merge_equals_single_engine(pkg, gpu_ok, tmp_path):
    name = "plane_64x48_n7"
    g = gu.load(name)
    eng = pipeline(pkg, g)
    try:
        eng.vmap_open(0.02)
        for k in range(g["n_kf"]):
            eng.vmap_integrate([k], **KW)
            eng.vmap_observe([k], g["nbrs"][[k]], **KW)
        want, cams, info = eng.vmap_fetch(), eng.vmap_fetch_cameras(), eng.vmap_info()
        E = eng.vmap_obs_info()["observations"]
    finally:
        eng.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "vmap_merge_worker.py"), str(tmp_path), name, "0.02"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2")
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=180)  # two engine set-ups and imports
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    z = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % rank)) for rank in range(2)]
    assert int(z[0]["before"][0]) < info["voxels"] and int(z[1]["before"][0]) < info["voxels"]  # neither rank had it all
    same_fetch({f: z[0][f] for f in want if f != "epoch"}, {f: want[f] for f in want if f != "epoch"}, "rank 0's merged map")
    same_fetch({f: z[0][f] for f in cams}, cams, "rank 0's camera lists")
    assert int(z[0]["points"][0]) == info["points"] and int(z[0]["observations"][0]) == E
    # rank 1 holds the same entries under other ids: the same records and lists, matched by (tag, pixel)
    assert len(z[1]["pixel"]) == info["voxels"] and int(z[1]["observations"][0]) == E
    key = lambda m: np.lexsort((m["pixel"], m["tag"]))
    o0, o1 = key(z[0]), key(z[1])
    for f in ("xyz", "pixel", "rho_sigma", "intensity", "tag", "multiplicity"):
        assert z[0][f][o0].tobytes() == z[1][f][o1].tobytes(), f
    l0, l1 = vo.lists(z[0]["cam_offsets"], z[0]["cam_tags"]), vo.lists(z[1]["cam_offsets"], z[1]["cam_tags"])
    assert [l0[i] for i in o0] == [l1[i] for i in o1]
