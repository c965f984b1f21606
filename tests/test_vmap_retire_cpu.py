"""CPU: tests/vmap_retire_np.py (the NumPy statement of sdm_vmap_retire) -- against a plain per-entry / per-pair loop, its
invariants R1 .. R5 (the identity, composition, the empty map, the tie to integrating without the keyframe, UNOBSERVED
keeps at least what WINNER keeps), one pinned six-entry case with literal ids, and the synthetic inputs of
tests/test_gpu_vmap_retire.py, defined here, with the assertion that they cover what that test is there for.

The synthetic maps are tests/test_vmap_repose_cpu.py's: records with the tags A = 3, B = 7, 20 .. 59 and a few hostile
ones, and a log whose tags are 5 on the A and B entries and 0 .. 8 on random entries.  The four sets R:
  0 tags    nothing
  1 tag     TAG_B: the B entries go in mode WINNER; in mode UNOBSERVED those with a live pair stay as orphans
  2 tags    and a tag no entry and no pair carries
  37 tags   TAG_B, every log tag but 3, 0 and 2^31 - 1, the record tags 20 .. 44, and tags nothing carries"""
import numpy as np
import pytest

import golden_util as gu
import vmap_import_np as vi
import vmap_np
import vmap_obs_np as vo
import vmap_retire_np as vt
from test_vmap_repose_cpu import LOG_TAG, SYN_M, TAG_A, TAG_B, build, clone, same_map
from test_voxel_cpu import _fixture_cloud

F = np.float32
NOID = vt.NOID
SYN_R = (0, 1, 2, 37)
TAG_UNUSED = 1000
LIVE_LOG_TAG = 3


def synthetic_tags(n):
    """R of n tags, unsorted"""
    if n == 0:
        return np.zeros(0, np.int32)
    if n == 1:
        return np.array([TAG_B], np.int32)
    if n == 2:
        return np.array([TAG_UNUSED, TAG_B], np.int32)
    assert n == 37
    tags = [TAG_B, (1 << 31) - 1, 0, 1, 2, 4, LOG_TAG, 6, 8] + list(range(44, 19, -1)) + [TAG_UNUSED, 201, 202]
    assert len(tags) == 37 and len(set(tags)) == 37 and LIVE_LOG_TAG not in tags and TAG_A not in tags
    return np.array(tags, np.int32)


def synthetic_flags(rec):
    """what a classify under the multiplicity-only rule (min_multiplicity = 2) publishes on an import-made map"""
    return (np.asarray(rec["multiplicity"]) >= 2).astype(np.uint8)


def same_log(a, b):
    assert a.E == b.E and (a.entry == b.entry).all() and (a.tag == b.tag).all() and (a.pairs == b.pairs).all()


def same_plan(a, b, what=""):
    for f in vt.DELTA:
        assert a[f] == b[f], (what, f, a[f], b[f])
    for f in vt.LISTS:
        assert a[f].dtype == b[f].dtype and a[f].tolist() == b[f].tolist(), (what, f)


@pytest.mark.parametrize("mode", sorted(vt.MODES))
@pytest.mark.parametrize("n_tags", SYN_R)
@pytest.mark.parametrize("M", SYN_M)
def test_against_the_loop(M, n_tags, mode):
    vm, ol, rec, _, _ = build(M)
    flags = synthetic_flags(vm.rec)
    tags = synthetic_tags(n_tags)
    ev = {"crossings": np.arange(M, dtype=np.uint64) * 3 + 1, "ends": np.arange(M, dtype=np.uint64)[::-1].copy()}
    for carry in (False, True):
        want = vt.retire_loop(vm.rec["tag"], ol.entry, ol.tag, tags, mode, flags, carry)
        v2, o2 = clone(vm, ol)
        dry, ev1, fl1 = vt.retire(v2, o2, tags, mode, carry, ev, flags, commit=False)
        same_plan(dry, want, "commit 0")
        same_map(v2, vm)
        same_log(o2, ol)
        assert v2.calls == vm.calls and ev1 is ev and fl1 is flags   # nothing changed
        got, ev2, fl2 = vt.retire(v2, o2, tags, mode, carry, ev, flags)
        same_plan(got, want, "commit 1")
        assert list(zip(o2.entry.tolist(), o2.tag.tolist())) == want["new_log"]
        surv = np.flatnonzero(got["remap"] != NOID)
        assert v2.M == got["voxels"] == len(surv) and (got["remap"][surv] == np.arange(len(surv))).all()
        for f in vmap_np.FIELDS:
            assert v2.rec[f].tobytes() == vm.rec[f][surv].tobytes(), f
        assert (v2.calls, v2.points, v2.dropped) == (vm.calls + 1, vm.points, vm.dropped) and o2.calls == ol.calls
        # the key index finds exactly the survivors' voxels under their new ids
        k2 = dict(zip(v2.keys.tolist(), v2.ids.tolist()))
        k1 = dict(zip(vm.keys.tolist(), vm.ids.tolist()))
        assert k2 == {k: int(got["remap"][i]) for k, i in k1.items() if got["remap"][i] != NOID}
        assert (np.diff(v2.keys) > 0).all()
        # the camera lists are the old ones without R
        offs, cams = o2.cameras(v2.M)
        o_offs, o_cams = ol.cameras(vm.M)
        for i in surv[:200]:
            old = [t for t in o_cams[o_offs[i]:o_offs[i + 1]].tolist() if t not in set(tags.tolist())]
            j = got["remap"][i]
            assert cams[offs[j]:offs[j + 1]].tolist() == old
        if carry:
            assert all((ev2[f] == ev[f][surv]).all() for f in ev) and (fl2 == flags[surv]).all()
            assert got["published_total"] == int(fl2.sum())
        else:
            assert not ev2["crossings"].any() and not ev2["ends"].any() and not fl2.any() and got["published_total"] == 0
        assert len(fl2) == len(ev2["ends"]) == v2.M


# R1: the empty R is the identity (with carry on evidence and flags too)
@pytest.mark.parametrize("M", SYN_M)
def test_r1_empty_set_is_the_identity(M):
    vm, ol, *_ = build(M)
    ev = {f: np.arange(M, dtype=np.uint64) * 3 + 1 for f in ("crossings", "ends")}
    flags = (np.arange(M) % 3 == 0).astype(np.uint8)
    v2, o2 = clone(vm, ol)
    d, ev2, fl2 = vt.retire(v2, o2, None, "winner", True, ev, flags)
    assert (d["examined"], d["dropped"], d["orphaned"], d["removed"], d["voxels"]) == (M, 0, 0, 0, M)
    assert (d["remap"] == np.arange(M)).all() and d["observations"] == d["observations_before"] == ol.E
    same_map(v2, vm)
    same_log(o2, ol)
    assert v2.calls == vm.calls + 1 and o2.calls == ol.calls
    assert all((ev2[f] == ev[f]).all() for f in ev) and (fl2 == flags).all() and d["published_total"] == int(flags.sum())
    d, ev2, fl2 = vt.retire(v2, o2, [], "winner", False, ev, flags)
    assert not ev2["crossings"].any() and not ev2["ends"].any() and not fl2.any() and d["published_total"] == 0


# R2: retire A then retire B is retire A u B, apart from `calls`; the remaps compose
@pytest.mark.parametrize("mode", sorted(vt.MODES))
@pytest.mark.parametrize("M", (65, 2049))
def test_r2_composition(M, mode):
    vm, ol, *_ = build(M)
    ev = {"crossings": np.arange(M, dtype=np.uint64) + 1, "ends": np.arange(M, dtype=np.uint64) * 7}
    flags = synthetic_flags(vm.rec)
    tags = synthetic_tags(37)
    A, B = tags[::2], tags[1::2]   # (both halves hold log tags and record tags)
    v1, o1 = clone(vm, ol)
    d1, e1, f1 = vt.retire(v1, o1, A, mode, True, ev, flags)
    d2, e2, f2 = vt.retire(v1, o1, B, mode, True, e1, f1)
    v3, o3 = clone(vm, ol)
    d3, e3, f3 = vt.retire(v3, o3, tags, mode, True, ev, flags)
    assert d1["dropped"] > 0 and d2["dropped"] > 0
    same_map(v1, v3)
    same_log(o1, o3)
    assert v1.calls == v3.calls + 1
    assert o1.cameras(v1.M)[0].tolist() == o3.cameras(v3.M)[0].tolist() and o1.cameras(v1.M)[1].tolist() == o3.cameras(v3.M)[1].tolist()
    assert all((e2[f] == e3[f]).all() for f in ev) and (f2 == f3).all()
    comp = np.full(M, NOID, np.uint32)
    s = d1["remap"] != NOID
    comp[s] = d2["remap"][d1["remap"][s]]
    assert (comp == d3["remap"]).all()
    assert d1["dropped"] + d2["dropped"] == d3["dropped"] and d2["voxels"] == d3["voxels"] and d2["observations"] == d3["observations"]


# R3: retiring every tag empties the map; an import then creates ids from 0 and the fetch is a fresh map's
@pytest.mark.parametrize("mode", sorted(vt.MODES))
def test_r3_retiring_everything_empties_the_map(mode):
    vm, ol, rec, pairs, _ = build(2049)
    every = np.unique(np.concatenate([vm.rec["tag"], ol.tag]))
    d, _, _ = vt.retire(vm, ol, every, mode)
    assert (d["voxels"], d["observations"], d["removed"], d["orphaned"]) == (0, 0, 0, 0) and d["dropped"] == 2049
    assert vm.M == 0 and ol.E == 0 and len(vm.keys) == 0 and len(ol.pairs) == 0
    fresh = vmap_np.VoxelMap(vm.voxel_size)
    a, b = vi.import_records(vm, rec), vi.import_records(fresh, rec)
    assert (a["dst_ids"] == b["dst_ids"]).all() and a["first_created"] == 0
    for f in vmap_np.FIELDS:
        if f != "epoch":
            assert vm.rec[f].tobytes() == fresh.rec[f].tobytes(), f
    assert (vm.keys == fresh.keys).all() and (vm.ids == fresh.ids).all()
    vi.import_observations(ol, vm.M, pairs["entry"], pairs["tag"])
    fl = vo.ObservationLog()
    vi.import_observations(fl, fresh.M, pairs["entry"], pairs["tag"])
    same_log(ol, fl)


def _fixture_blocks(name):
    g = gu.load(name)
    xyz, sigma, slot = _fixture_cloud(g)   # (sigma gate 0.3)
    T = len(xyz)
    cloud = {"xyz": xyz, "pixel": np.arange(T, dtype=np.uint32), "rho_sigma": np.stack([np.ones(T, F), sigma], 1),
             "intensity": (np.arange(T) % 251).astype(np.uint8)}
    offs = np.searchsorted(slot, np.arange(g["n_kf"] + 1))
    return g, cloud, slot, offs


def _integrated(cloud, slot, offs, kfs, voxel=0.02, observe=False):
    vm, ol = vmap_np.VoxelMap(voxel), vo.ObservationLog()
    for k in kfs:
        a, b = offs[k], offs[k + 1]
        part = {f: v[a:b] for f, v in cloud.items()}
        vm.integrate(part, slot[a:b])
        if observe:   # the recipe: integrate, then observe, per block (no neighbour table: the own tag alone)
            ol.observe((vm.keys, vm.ids), voxel, part["xyz"], np.zeros(b - a, np.int64), None, [k], None)
    return vm, ol


# R4: the tie to existing semantics.  (survivors, dropped, voxels of the map without the keyframe, of those without a
# survivor) per fixture, retiring keyframe 1
R4_COUNTS = ((669, 17, 681, 12), (964, 44, 999, 35), (664, 27, 687, 23), (922, 74, 974, 52))
R4_RETIRED = 1


@pytest.mark.parametrize("idx,name", list(enumerate(gu.fixture_names())))
def test_r4_winner_against_integrating_without_the_keyframe(idx, name):
    g, cloud, slot, offs = _fixture_blocks(name)
    kfs = list(range(g["n_kf"]))
    vm, ol = _integrated(cloud, slot, offs, kfs)
    whole = clone(vm, ol)[0]
    d, _, _ = vt.retire(vm, ol, [R4_RETIRED], "winner")
    fresh, _ = _integrated(cloud, slot, offs, [k for k in kfs if k != R4_RETIRED])
    at = np.searchsorted(fresh.keys, vm.keys)
    assert (at < len(fresh.keys)).all() and (fresh.keys[at] == vm.keys).all()   # every survivor's voxel is in the fresh map
    fid = np.empty(vm.M, np.int64)
    fid[vm.ids] = fresh.ids[at]
    for f in ("xyz", "pixel", "rho_sigma", "intensity", "tag"):
        assert vm.rec[f].tobytes() == fresh.rec[f][fid].tobytes(), f
    # the fresh map's voxels without a survivor are exactly those whose overall winner was the retired keyframe
    lone = fresh.keys[~np.isin(fresh.keys, vm.keys)]
    won = whole.keys[whole.rec["tag"][whole.ids] == R4_RETIRED]
    assert (np.sort(lone) == np.sort(won[np.isin(won, fresh.keys)])).all()
    counts = (d["voxels"], d["dropped"], fresh.M, len(lone))
    print(name, counts)
    assert min(counts) > 0
    assert counts == R4_COUNTS[idx]


# R5: with the recipe integrate + observe, UNOBSERVED keeps at least what WINNER keeps; orphaned per fixture, retiring keyframe 1
R5_ORPHANED = (12, 35, 23, 52)


@pytest.mark.parametrize("idx,name", list(enumerate(gu.fixture_names())))
def test_r5_unobserved_keeps_at_least_the_winners_survivors(idx, name):
    g, cloud, slot, offs = _fixture_blocks(name)
    vm, ol = _integrated(cloud, slot, offs, range(g["n_kf"]), observe=True)
    assert ol.E >= vm.M
    w = vt.plan(vm.rec["tag"], ol.entry, ol.tag, [R4_RETIRED], "winner")
    u = vt.plan(vm.rec["tag"], ol.entry, ol.tag, [R4_RETIRED], "unobserved")
    sw, su = w["remap"] != NOID, u["remap"] != NOID
    assert (su | ~sw).all() and su.sum() > sw.sum() and w["orphaned"] == 0
    assert u["orphaned"] == int(su.sum() - sw.sum())
    print(name, "orphaned", u["orphaned"], "dropped", u["dropped"], w["dropped"])
    assert u["orphaned"] > 0 and u["orphaned"] == R5_ORPHANED[idx]


def test_pinned_small_case():
    """six entries; R = {2, 9}: entries 1 and 4 carry tag 2; entry 4 keeps a live pair"""
    vm, ol = vmap_np.VoxelMap(1.0), vo.ObservationLog()
    rec = {"xyz": np.array([[0.5, 0.5, 1.5], [5.5, 0.5, 1.5], [9.5, 0.5, 1.5], [20.5, 0.5, 0.5], [7.5, 7.5, 7.5], [30.5, 0.5, 0.5]], F),
           "pixel": np.arange(6, dtype=np.uint32), "rho_sigma": np.array([[1, 0.2], [1, 0.1], [1, 0.3], [1, 0.4], [1, 0.2], [0.5, 0.5]], F),
           "intensity": np.arange(6, dtype=np.uint8), "tag": np.array([1, 2, 3, 4, 2, 6], np.int32),
           "multiplicity": np.array([1, 2, 3, 4, 5, 6], np.uint32)}
    vi.import_records(vm, rec)
    vi.import_observations(ol, 6, [0, 1, 1, 2, 4, 4, 3, 0, 5], [9, 2, 9, 3, 2, 8, 9, 1, 6])
    ev = {"crossings": np.array([1, 2, 4, 8, 16, 32], np.uint64), "ends": np.array([6, 5, 4, 3, 2, 1], np.uint64)}
    flags = np.array([0, 1, 1, 0, 1, 0], np.uint8)
    v1, o1 = clone(vm, ol)
    d, e1, f1 = vt.retire(v1, o1, [9, 2], "winner", True, ev, flags)
    assert d["remap"].tolist() == [0, NOID, 1, 2, NOID, 3]
    assert {f: d[f] for f in vt.DELTA} == {"examined": 6, "dropped": 2, "dropped_were_published": 2, "orphaned": 0, "voxels": 4,
                                           "observations_before": 9, "observations": 3, "removed": 2, "published_total": 1}
    assert d["dropped_ids"].tolist() == [1, 4] and d["dropped_published"].tolist() == [1, 1]
    assert d["removed_entry"].tolist() == [0, 3] and d["removed_tag"].tolist() == [9, 9]
    assert list(zip(o1.entry.tolist(), o1.tag.tolist())) == [(1, 3), (0, 1), (3, 6)]
    assert v1.rec["tag"].tolist() == [1, 3, 4, 6] and v1.rec["multiplicity"].tolist() == [1, 3, 4, 6] and v1.calls == 2
    assert e1["crossings"].tolist() == [1, 4, 8, 32] and e1["ends"].tolist() == [6, 4, 3, 1] and f1.tolist() == [0, 1, 0, 0]
    assert vo.lists(*o1.cameras(4)) == [[1], [3], [], [6]]
    v2, o2 = clone(vm, ol)
    d, e2, f2 = vt.retire(v2, o2, [9, 2], "unobserved", False, ev, flags)
    assert d["remap"].tolist() == [0, NOID, 1, NOID, 2, 3]
    assert {f: d[f] for f in vt.DELTA} == {"examined": 6, "dropped": 2, "dropped_were_published": 1, "orphaned": 1, "voxels": 4,
                                           "observations_before": 9, "observations": 4, "removed": 2, "published_total": 0}
    assert d["dropped_ids"].tolist() == [1, 3] and d["dropped_published"].tolist() == [1, 0]
    assert d["removed_entry"].tolist() == [0, 4] and d["removed_tag"].tolist() == [9, 2]
    assert list(zip(o2.entry.tolist(), o2.tag.tolist())) == [(1, 3), (2, 8), (0, 1), (3, 6)]
    assert v2.rec["tag"].tolist() == [1, 3, 2, 6] and not e2["crossings"].any() and not f2.any()


def test_synthetic_inputs_cover_the_cases():
    """over the four R and both modes the synthetic maps give every case the GPU test is there for"""
    for M in SYN_M:
        vm, ol, *_ = build(M)
        flags = synthetic_flags(vm.rec)
        seen = dict(dropped=0, dropped_published=0, orphaned=0, removed=0, vanished=0, emptied=0, kept=0)
        for n in SYN_R:
            tags = synthetic_tags(n)
            if n > 1:
                assert (np.diff(tags) < 0).any()   # unsorted
            if n >= 2:
                assert not np.isin(tags, np.concatenate([vm.rec["tag"], ol.tag])).all()   # a tag nothing carries
            for mode in sorted(vt.MODES):
                d = vt.plan(vm.rec["tag"], ol.entry, ol.tag, tags, mode, flags, True)
                if n == 0 and mode == "winner":
                    assert d["dropped"] == d["removed"] == 0 and d["voxels"] == M
                seen["dropped"] += d["dropped"]
                seen["dropped_published"] += d["dropped_were_published"]
                seen["orphaned"] += d["orphaned"]
                seen["removed"] += d["removed"]
                seen["vanished"] += d["observations_before"] - d["observations"] - d["removed"]
                seen["kept"] += d["observations"]
                if mode == "winner" and M:
                    surv = d["remap"] != NOID
                    had = np.bincount(ol.entry, minlength=M) > 0
                    has = np.bincount(ol.entry[d["keep"]], minlength=M) > 0
                    seen["emptied"] += int((surv & had & ~has).sum())
        if M >= 63:
            assert min(seen.values()) > 0, (M, seen)
