"""NumPy restatement of sdm_vmap_retire (include/sdm_c.h): removing a set R of keyframe tags from a persistent voxel map.
Works in place on the mirrors of the calls that build the map: vmap_np.VoxelMap and vmap_obs_np.ObservationLog.

  pairs      pair k of the old log is RETIRED iff its tag is in R
  survivors  mode "winner": entry i survives iff its record's tag is not in R
             mode "unobserved": entry i survives iff one of its pairs is not retired (never observed: does not survive)
  map        new id = rank of i among the survivors; every record field is copied; remap[i] = new id or NOID; calls += 1;
             points and dropped stay
  log        the old log in log order without the retired pairs and the pairs of dropped entries, entries through remap;
             `removed` lists the retired pairs of SURVIVING entries (old entry ids, old log order); the log's calls stay
  carry      0: counters and flags restart at 0; 1: a survivor keeps its own
  orphaned   survivors whose record's tag is in R

retire_loop is the same statement as a plain per-entry / per-pair Python loop; tests/test_vmap_retire_cpu.py holds the two
against each other."""
import numpy as np

import vmap_np

NOID = 0xFFFFFFFF
MODES = {"winner": 0, "unobserved": 1}
DELTA = ("examined", "dropped", "dropped_were_published", "orphaned", "voxels", "observations_before", "observations",
         "removed", "published_total")
LISTS = ("remap", "dropped_ids", "dropped_published", "removed_entry", "removed_tag")


def _tags(tags):
    R = np.asarray([] if tags is None else tags, np.int64).reshape(-1)
    assert len(set(R.tolist())) == len(R) and (R >= 0).all() and (R < (1 << 31)).all()
    return R


def plan(rec_tag, log_entry, log_tag, tags, mode, flags=None, carry=False):
    """The delta and the lists of a retire of R = tags from a map whose records carry rec_tag[M] and whose log is
    (log_entry[E], log_tag[E]); flags uint8[M] or None (every flag 0).  Nothing is changed.  Also returns "keep":
    bool[E], the pairs that stay."""
    assert mode in MODES
    R = _tags(tags)
    rec_tag = np.asarray(rec_tag, np.int64).reshape(-1)
    le = np.asarray(log_entry, np.int64).reshape(-1)
    lt = np.asarray(log_tag, np.int64).reshape(-1)
    M, E = len(rec_tag), len(le)
    pub = np.zeros(M, bool) if flags is None else np.asarray(flags).reshape(-1) != 0
    retired = np.isin(lt, R)
    rec_ret = np.isin(rec_tag, R)
    if mode == "winner":
        surv = ~rec_ret
    else:
        surv = np.zeros(M, bool)
        surv[le[~retired]] = True
    remap = np.full(M, NOID, np.uint32)
    remap[surv] = np.arange(int(surv.sum()), dtype=np.uint32)
    dropped_ids = np.flatnonzero(~surv).astype(np.uint32)
    on_surv = surv[le] if E else np.zeros(0, bool)
    rem = retired & on_surv
    keep = ~retired & on_surv
    return {"examined": M, "dropped": len(dropped_ids), "dropped_were_published": int(pub[~surv].sum()),
            "orphaned": int((surv & rec_ret).sum()), "voxels": int(surv.sum()), "observations_before": E,
            "observations": int(keep.sum()), "removed": int(rem.sum()),
            "published_total": int(pub[surv].sum()) if carry else 0, "remap": remap, "dropped_ids": dropped_ids,
            "dropped_published": pub[~surv].astype(np.uint8), "removed_entry": le[rem].astype(np.uint32),
            "removed_tag": lt[rem].astype(np.int32), "keep": keep}


def retire(vm, ol, tags, mode="winner", carry=False, ev=None, flags=None, commit=True):
    """Retires R = tags from the vmap_np.VoxelMap `vm` and the vmap_obs_np.ObservationLog `ol` (or None) in place (commit
    False: nothing changes).  ev: {"crossings", "ends"} uint64[M] or None; flags: uint8[M] or None.  Returns (delta, ev,
    flags): the delta with the outs and the five lists, and the counters and flags after the call (None where None came
    in)."""
    le = np.zeros(0, np.uint32) if ol is None else ol.entry
    lt = np.zeros(0, np.int32) if ol is None else ol.tag
    d = plan(vm.rec["tag"], le, lt, tags, mode, flags, carry)
    keep = d.pop("keep")
    if not commit:
        return d, ev, flags
    surv = d["remap"] != NOID
    M2 = d["voxels"]
    vm.rec = {f: vm.rec[f][surv].copy() for f in vmap_np.FIELDS}
    live = surv[vm.ids]  # (keys stay sorted: a subsequence)
    vm.keys, vm.ids = vm.keys[live], d["remap"][vm.ids[live]].astype(np.int64)
    vm.calls += 1
    if ol is not None and ol.E:
        ol.entry = d["remap"][ol.entry[keep]].astype(np.uint32)
        ol.tag = ol.tag[keep].copy()
        ol.pairs = np.sort((ol.entry.astype(np.int64) << 32) | ol.tag.astype(np.int64))
    ev2 = flags2 = None
    if ev is not None:
        ev2 = {f: (np.asarray(ev[f], np.uint64)[surv].copy() if carry else np.zeros(M2, np.uint64)) for f in ev}
    if flags is not None:
        flags2 = (np.asarray(flags)[surv] != 0).astype(np.uint8) if carry else np.zeros(M2, np.uint8)
    return d, ev2, flags2


def retire_loop(rec_tag, log_entry, log_tag, tags, mode, flags=None, carry=False):
    """plan() as a plain loop over the pairs and the entries: the same keys except "keep", plus "new_log": the list of
    (new entry, tag) of the log after the call"""
    R = set(int(t) for t in _tags(tags))
    M = len(rec_tag)
    seen = [False] * M
    for e, t in zip(log_entry, log_tag):
        if int(t) not in R:
            seen[int(e)] = True
    remap, dropped_ids, dropped_published = [], [], []
    orphaned = dropped_pub = pub_total = nxt = 0
    for i in range(M):
        in_r = int(rec_tag[i]) in R
        s = seen[i] if mode == "unobserved" else not in_r
        p = 0 if flags is None else int(flags[i] != 0)
        if s:
            remap.append(nxt)
            nxt += 1
            orphaned += in_r
            pub_total += p
        else:
            remap.append(NOID)
            dropped_ids.append(i)
            dropped_published.append(p)
            dropped_pub += p
    removed_entry, removed_tag, new_log = [], [], []
    for e, t in zip(log_entry, log_tag):
        e, t = int(e), int(t)
        if remap[e] == NOID:
            continue
        if t in R:
            removed_entry.append(e)
            removed_tag.append(t)
        else:
            new_log.append((remap[e], t))
    return {"examined": M, "dropped": len(dropped_ids), "dropped_were_published": dropped_pub, "orphaned": orphaned,
            "voxels": nxt, "observations_before": len(log_entry), "observations": len(new_log),
            "removed": len(removed_entry), "published_total": pub_total if carry else 0,
            "remap": np.array(remap, np.uint32), "dropped_ids": np.array(dropped_ids, np.uint32),
            "dropped_published": np.array(dropped_published, np.uint8), "removed_entry": np.array(removed_entry, np.uint32),
            "removed_tag": np.array(removed_tag, np.int32), "new_log": new_log}
