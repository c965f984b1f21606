"""The whole life cycle of the persistent voxel map on a host-side model: cloud_model.World (the oracle-driven planes and
the plain cloud, the support words and the five map calls built on them) extended by the calls merged since -- observe,
classify, import, import_observations, repose, retire, recarve and the four fetches -- plus the generator of the random
call sequences that tests/test_gpu_mapfuzz.py runs against an engine and tests/test_mapfuzz_cpu.py runs against this model
alone.  Nothing here touches an engine, and nothing here imports torch.

  map state      test_gpu_vmap_class.Mirror: vmap_np.VoxelMap, vmap_obs_np.ObservationLog, the two evidence counters and
                 vmap_class_np.Classifier, fed cloud_model.cloud / support_words over the model's planes and current poses
  semantics      vmap_np, vmap_obs_np, vmap_carve_np, vmap_class_np, vmap_import_np, vmap_repose_np, vmap_retire_np,
                 vmap_recarve_np, each called as the per-call tests call it
  tags           persistent identities: tag = slot + N_KF x (times the slot has been uploaded again).  A recycled slot
                 integrates under a new tag while the old tag's records stay; MapWorld.table holds, per tag, (K, the
                 current Tcw, the Tcw the map last saw) -- what the caller of repose and recarve holds.  The pose of a tag
                 whose slot is gone moves only in that table (a loop closure): a repose's drawn pose becomes its current one
  refusals       SDM_ESTATE without an open map for every new call, SDM_EINVAL for a tag listed twice (repose, retire,
                 recarve), ratio_den == 0, a recarve range beyond E, and the slot and neighbour states observe inherits;
                 each steered into every sequence; a refused call leaves the model untouched
  queries        the five read-only calls (QUERY_OPS: cast_segments, render, components, normals, mesh) come from a stream
                 of their own beside the main one (QueryStream: a second RNG, the counters MapWorld.qcov): with them
                 filtered out a sequence is the one generated without them.  MapWorld.apply answers them through
                 vmap_cast_np, vmap_comp_np, vmap_normals_np and vmap_mesh_np on the model's own records, flags ("none yet"
                 before the first committing classify of the map) and voxel size, and changes nothing.  Their refusals:
                 SDM_ESTATE without a map for each, SDM_EINVAL for require_published 2, a connectivity that is none of the
                 three, radius 3, a range beyond M, a tag listed twice, and a small_ids / tri destination one element short
                 (refused with the totals).  check_query_coverage holds the conditions on the stream; its sensitivity
                 counters count the queries whose answer differs on the state before the last change (sens_query_stale)
                 and with every flag cleared (sens_query_flags)

MapWorld.apply(op, args) applies one call and returns what the engine must answer; it keeps the coverage counters that
check_coverage asserts (conditions on the sequences, not on an engine) and the sensitivity counters, each the number of
calls in which a deliberately wrong variant of the model answers differently (counts, never expectations)."""
import copy

import numpy as np

import carve_np
import cloud_model as cm
import vmap_cast_np as vk
import vmap_comp_np as vq
import vmap_import_np as vi
import vmap_mesh_np as vms
import vmap_normals_np as vn
import vmap_recarve_np as vrc
import vmap_repose_np as vrp
import vmap_retire_np as vrt
from test_gpu_extract import EINVAL, ESTATE
from test_gpu_vmap_class import NOTHING, RULE, Mirror

N_KF = cm.N_KF
STEPS = 160
NOID = 0xFFFFFFFF
F = np.float32
LAX = dict(min_multiplicity=2)  # test_gpu_vmap_repose.LAX (that module imports torch; the GPU test holds the two equal)
SEEN = dict(min_multiplicity=1, min_cameras=1, min_ends=1, ratio_num=4, max_sigma=0.25, min_neighbours=0)
RULES = {"rule": RULE, "nothing": NOTHING, "lax": LAX, "seen": SEEN, "near": dict(min_neighbours=1), "all": {}}
COUNTS = ("examined", "accepted", "retracted", "published_total")
FETCHES = ("vmap_fetch", "vmap_fetch_evidence", "vmap_fetch_cameras", "vmap_fetch_published")
NEW_OPS = ("vmap_observe", "vmap_classify", "vmap_import", "vmap_import_observations", "vmap_repose", "vmap_retire",
           "vmap_recarve") + FETCHES
OLD_OPS = ("vmap_open", "vmap_integrate", "vmap_carve", "vmap_clear", "vmap_close")
MAP_OPS = OLD_OPS + NEW_OPS
OPS = cm.PIPE_OPS + MAP_OPS
READS = ("vmap_integrate", "vmap_observe", "vmap_carve")  # the calls that read a cloud
RECON_OPS = ("recon", "search_fuse", "recon+batch", "inter", "inter_commit", "fused")
NO_MAP = ("observe", "classify", "import", "import_observations", "repose", "retire", "recarve", "fetch")
TWICE = ("repose", "retire", "recarve")
OBS_STATES = ("no_depth", "no_chk", "nbr_no_depth")
REFUSALS = tuple("refuse_no_map_" + o for o in NO_MAP) + tuple("refuse_twice_" + o for o in TWICE) + \
    ("refuse_ratio_den", "refuse_range") + tuple("refuse_obs_" + s for s in OBS_STATES)
GROWTH = ("integrate", "observe", "carve", "classify")
CONTENT = ("refuse_range", "repose_moved", "repose_merged", "repose_dropped", "retire_winner_both", "retire_unobserved_both",
           "retire_orphaned", "grown_after_repose", "grown_after_retire", "recarve_chain", "carry_repose_published",
           "carry_retire_published", "recarve_unposed", "recarve_short", "sens_repose_stale", "sens_retire_mode",
           "sens_recarve_prev")
SENS = ("sens_observe_pose", "sens_repose_stale", "sens_retire_mode", "sens_recarve_prev", "sens_listed")
_WEIGHT = dict({o: (1.2 if o.startswith("pointset") else 0.55) * cm._WEIGHT[o] for o in cm.PIPE_OPS},
               vmap_open=1, vmap_integrate=5, vmap_carve=3, vmap_clear=0.4, vmap_close=0.4, vmap_observe=5, vmap_classify=3,
               vmap_import=1.5, vmap_import_observations=1.5, vmap_repose=2, vmap_retire=1.5, vmap_recarve=2,
               vmap_fetch=1, vmap_fetch_evidence=1, vmap_fetch_cameras=1, vmap_fetch_published=1)


# ---- the read-only queries: a stream of their own beside the main one (generate) ---------------------------------------
QUERY_OPS = ("vmap_cast_segments", "vmap_render", "vmap_components", "vmap_normals", "vmap_mesh")
QKINDS = tuple(o[5:] for o in QUERY_OPS)
QARRAYS = {"vmap_cast_segments": ("hit_id", "hit_step"), "vmap_render": ("hit_id", "hit_step", "hit_rho"),
           "vmap_components": vq.ARRAYS, "vmap_normals": vn.ARRAYS, "vmap_mesh": vms.ARRAYS}
QTOTALS = {"vmap_cast_segments": vk.OUTS, "vmap_render": vk.OUTS, "vmap_components": vq.OUTS, "vmap_normals": vn.OUTS,
           "vmap_mesh": vms.OUTS}
QEVENTS = ("repose", "retire", "classify")  # a query straight behind one of them (retire and classify: committing)
QFIRST = ("clear", "import", "set_pose", "big")  # further events whose first occurrence is followed by every query kind
QINVALID = ("published2", "connectivity", "radius", "range", "twice", "small_short", "tri_short")
QREFUSALS = tuple("refuse_no_map_" + k for k in QKINDS) + tuple("refuse_" + r for r in QINVALID)
QCONTENT = ("rays_hit", "rays_miss", "rays_skipped", "render_hit_and_zero", "comp_rich", "normals_rich", "mesh_quads_singles",
            "mesh_empty", "mesh_from_normals", "mesh_crafted")
QPER_KIND = ("n", "sens_query_stale", "sens_query_flags", "pub_before", "pub_after") + tuple("after_" + e for e in QEVENTS)
BIG = 50  # the main generator keeps a map of this many entries alive while its content conditions are open


class FullMirror(Mirror):
    """test_gpu_vmap_class.Mirror fed the model's clouds (cloud_model.MapMirror's two feeds)"""
    integrate_cloud = cm.MapMirror.integrate_cloud
    carve_cloud = cm.MapMirror.carve_cloud

    def pad(self):
        for f in self.ev:  # entries created later start at 0
            self.ev[f] = np.concatenate([self.ev[f], np.zeros(self.vm.M - len(self.ev[f]), np.uint64)])


def jolt(rng, T, shift=0.02):
    """a pose a little off T: a small rotation in front and a shifted translation"""
    T = np.asarray(T, np.float64).reshape(3, 4)
    a = rng.normal(0, 0.004)
    c, s = np.cos(a), np.sin(a)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    return np.concatenate([R @ T[:, :3], (R @ T[:, 3] + rng.normal(0, shift, 3)).reshape(3, 1)], axis=1).astype(F)


def _same_state(x, y):
    """two states of MapWorld._query_state's kind hold the same bits"""
    if x is None or y is None:
        return x is y
    return x[2] == y[2] and (x[1] is None) == (y[1] is None) and (x[1] is None or x[1].tobytes() == y[1].tobytes()) and \
        all(x[0][f].tobytes() == y[0][f].tobytes() for f in x[0])


def _differs(op, x, y):
    """two answers of a query differ in a total or in a byte of an array"""
    return any(x[f] != y[f] for f in QTOTALS[op]) or \
        any(x[f].shape != y[f].shape or x[f].tobytes() != y[f].tobytes() for f in QARRAYS[op])


class MapWorld(cm.World):
    def __init__(self, oracle, seq, lam=8.0):
        super().__init__(oracle, seq, lam)
        self.count.update(dict.fromkeys(NEW_OPS, 0))
        self.gen = {k: 0 for k in range(seq.n_kf)}  # how often the slot has been uploaded again
        self.table = {}                               # tag -> {"K", "T": the current pose, "known": the pose the map last saw}
        for k in range(seq.n_kf):
            self._new_tag(k)
        self.before_pose = None                       # (slot, its pose before the last set_pose)
        self.posed = set()                            # slots re-posed since the last reconstruction
        self.mcov = dict.fromkeys(
            ("map_calls", "refusals") + REFUSALS +
            ("observe_after_set_pose", "repose_moved", "repose_merged", "repose_dropped", "retire_winner_both",
             "retire_unobserved_both", "retire_orphaned", "grown_after_repose", "grown_after_retire", "recarve_chain",
             "carry_repose_published", "carry_retire_published", "recarve_unposed", "recarve_short", "pairs_created",
             "max_pairs") + SENS, 0)
        # the queries' own counters: nothing of the main stream's (count, cov, mcov, last) is touched by a query
        self.qcov = dict.fromkeys(("calls", "refusals") + QREFUSALS + QCONTENT + tuple("first_" + e for e in QFIRST) +
                                  tuple("%s_%s" % (p, k) for p in QPER_KIND for k in QKINDS), 0)
        self.qnow = self.qprev = None  # what the queries read, now and before the last call that changed it
        self.qlast = None              # the last call of the main stream that was not refused: (op, it committed)
        self.qapplied = False          # the main stream's last call was not refused
        self.qchanged = False          # that call changed what the queries read
        self.qnormal = None            # the last vmap_normals of the state as it stands: (its range and filters, the normals)
        self._map_reset()

    # -- tags and the caller's pose table
    def tag(self, k):
        return int(k) + N_KF * self.gen[int(k)]

    def _new_tag(self, k):
        T = np.array(self.m.Tcw[k], F).reshape(3, 4)
        self.table[self.tag(k)] = {"K": np.array(self.seq.K, F).reshape(4), "T": T, "known": T.copy()}

    def live(self, t):
        """the tag still names its slot's keyframe"""
        return t in self.table and self.tag(t % N_KF) == t

    def _uploaded(self, k, im, Tcw):
        super()._uploaded(k, im, Tcw)
        self.gen[k] += 1
        self._new_tag(k)
        if self.before_pose is not None and self.before_pose[0] == k:
            self.before_pose = None
        self.posed.discard(k)

    def _map_reset(self):
        self.after = {"repose": None, "retire": None}  # what has run on the rebuilt table and set since
        self.fed = set()        # the tags integrated into this map and not retired since
        self.chain = 0          # 1: after a carry-0 repose / retire, 2: then a whole-log recarve with reset
        self.prev_xyz = np.zeros((0, 3), F)  # per entry: its record's xyz before the last repose (sensitivity only)

    def _event(self, what):
        for kind, seen in self.after.items():
            if seen is not None and what not in seen:
                seen.add(what)
                if len(seen) == len(GROWTH):
                    self.mcov["grown_after_" + kind] += 1

    def _sync_prev(self):
        M = self.map.vm.M
        if len(self.prev_xyz) < M:
            self.prev_xyz = np.concatenate([self.prev_xyz, self.map.vm.rec["xyz"][len(self.prev_xyz):M]])

    def published(self):
        return 0 if self.map is None else self.map.cl.info()["published"]

    def record_tags(self):
        return [] if self.map is None else sorted(set(self.map.vm.rec["tag"].tolist()))

    def log_tags(self):
        return [] if self.map is None else sorted(set(self.map.ol.tag.tolist()))

    # -- refusals
    def refusal(self, op, a):
        if op in QUERY_OPS:
            return self._query_refusal(op, a)
        if op not in NEW_OPS:
            return super().refusal(op, a)
        if self.map is None:
            return ESTATE, "no_map"
        if op == "vmap_observe":
            return super().refusal(op, a)
        if op in ("vmap_repose", "vmap_retire", "vmap_recarve") and len(set(a["tags"])) != len(a["tags"]):
            return EINVAL, "twice"
        if op == "vmap_classify" and a["rule"].get("ratio_den", 1) == 0:
            return EINVAL, "ratio_den"
        if op == "vmap_recarve" and a["first"] + (0 if a["count"] is None else a["count"]) > self.map.ol.E:
            return EINVAL, "range"
        return None

    # -- one call
    def apply(self, op, a):
        if op in QUERY_OPS:
            return self._query(op, a)
        res = self._apply(op, a)
        if not res.get("refused"):
            self.qlast = (op, bool(a.get("commit", True)) if op in ("vmap_classify", "vmap_retire") else True)
        cur = self._query_state()
        self.qapplied = not res.get("refused")
        self.qchanged = not _same_state(cur, self.qnow)
        if self.qchanged:
            self.qprev, self.qnow, self.qnormal = self.qnow if cur is not None else None, cur, None
        return res

    def _apply(self, op, a):
        if op in NEW_OPS:
            self.count[op] += 1
            res = self._map(op, a)
            self.last = (op, [])
        else:
            if op == "set_pose":
                self.before_pose = (a["k"], np.array(self.m.Tcw[a["k"]], F))
            res = super().apply(op, a)
            if op == "set_pose":
                self.table[self.tag(a["k"])]["T"] = np.array(a["T"], F).reshape(3, 4)
                self.posed.add(a["k"])
            elif op in RECON_OPS and not res.get("refused"):
                self.posed.clear()
            elif op in OLD_OPS and not res["refused"]:
                self._old(op, a, res)
        if op in MAP_OPS:
            self.mcov["map_calls"] += 1
            self.mcov["refusals"] += bool(res["refused"])
        if self.map is not None:
            self.cov["max_voxels"] = max(self.cov["max_voxels"], self.map.vm.M)
            self.mcov["max_pairs"] = max(self.mcov["max_pairs"], self.map.ol.E)
        return res

    def _old(self, op, a, res):
        """the bookkeeping of this model around the five calls cloud_model.World applies"""
        if op == "vmap_open":
            self.map = FullMirror(a["voxel"])
        if op in ("vmap_open", "vmap_clear", "vmap_close"):
            self._map_reset()
        elif op == "vmap_integrate":
            for k, t in zip(a["slots"], a["tags"] if a["tags"] is not None else a["slots"]):
                self.fed.add(int(t))
                if t in self.table:
                    self.table[t]["known"] = self.table[t]["T"].copy()
            if res["delta"]["created"] > 0:
                self._event("integrate")
            self._sync_prev()
        elif op == "vmap_carve":
            self._event("carve")

    def _refused(self, op, a, ref):
        c = self.mcov
        kind = ref[1]
        name = "fetch" if op in FETCHES else op[5:]
        if kind == "no_map":
            c["refuse_no_map_" + name] += 1
        elif kind == "twice":
            c["refuse_twice_" + name] += 1
        elif kind in ("ratio_den", "range"):
            c["refuse_" + kind] += 1
        else:
            c["refuse_obs_" + kind] += 1
            if kind == "no_depth":
                self.cov["hist_reupload"] += sum("reupload" in self.history(k) for k in a["slots"])
        return {"refused": ref[0]}

    # -- the read-only queries
    def _query_state(self):
        """what the five queries read, as copies: (records, flags or None before the first committing classify, voxel size)"""
        mp = self.map
        if mp is None:
            return None
        M = mp.vm.M
        rec = {f: mp.vm.rec[f][:M].copy() for f in ("xyz", "multiplicity", "tag")}
        return rec, (mp.cl.flags(M).copy() if mp.cl.calls else None), mp.voxel

    def _query_refusal(self, op, a):
        if self.map is None:
            return ESTATE, "no_map"
        M = self.map.vm.M
        if a["require_published"] not in (0, 1):
            return EINVAL, "published2"
        if op == "vmap_components" and a["connectivity"] not in vq.MAX_L1:
            return EINVAL, "connectivity"
        if op == "vmap_normals" and a["radius"] not in (1, 2):
            return EINVAL, "radius"
        if op in ("vmap_normals", "vmap_mesh") and a["first"] + (0 if a["count"] is None else a["count"]) > M:
            return EINVAL, "range"
        if op == "vmap_normals" and a["tags"] is not None and len(set(a["tags"])) != len(a["tags"]):
            return EINVAL, "twice"
        if a.get("short"):  # a small_ids / tri destination one element short of what the call would fill
            return EINVAL, "small_short" if op == "vmap_components" else "tri_short"
        return None

    @staticmethod
    def answer(op, a, state):
        """the restatement of the call on a state of _query_state's kind"""
        rec, flags, voxel = state
        flt = dict(min_multiplicity=a["min_multiplicity"], require_published=bool(a["require_published"]))
        if op in ("vmap_cast_segments", "vmap_render"):
            flt.update(start_margin=a["start_margin"], end_margin=a["end_margin"], max_steps=a["max_steps"])
            if op == "vmap_render":
                return vk.render(rec, flags, a["K"], a["T"], a["W"], a["H"], a["rho_far"], voxel, **flt)
            return vk.cast_segments(rec, flags, a["origins"], a["ends"], voxel, **flt)
        if op == "vmap_components":
            return vq.components(rec, flags, voxel, connectivity=a["connectivity"], min_size=a["min_size"], **flt)
        if op == "vmap_normals":
            return vn.normals(rec, flags, voxel, tags=a["tags"], Tcw=a["T"], radius=a["radius"], min_points=a["min_points"],
                              first=a["first"], count=a["count"], **flt)
        return vms.mesh(rec, flags, voxel, a["normal"], first=a["first"], count=a["count"], **flt)

    def _query(self, op, a):
        """one read-only query: its answer from the model's own state, which it leaves as it is"""
        c, k = self.qcov, op[5:]
        c["calls"] += 1
        ref = self._query_refusal(op, a)
        if ref is not None and ref[1] not in ("small_short", "tri_short"):
            c["refusals"] += 1
            c["refuse_no_map_" + k if ref[1] == "no_map" else "refuse_" + ref[1]] += 1
            return {"refused": ref[0]}
        now = self.qnow
        assert _same_state(now, self._query_state()), "the queries' copy of the state is behind the model"
        exp = self.answer(op, a, now)
        totals = {f: exp[f] for f in QTOTALS[op]}
        if ref is not None:  # too short: refused with the totals filled
            assert totals["small" if op == "vmap_components" else "triangles"] >= 2, (op, totals)
            c["refusals"] += 1
            c["refuse_" + ref[1]] += 1
            return {"refused": ref[0], "totals": totals}
        rec, flags, _ = now
        M = len(rec["multiplicity"])
        c["n_" + k] += 1
        # sensitivity (counts, never expectations): the answer from the state before the last change, and without the flags
        if self.qprev is not None:
            try:
                c["sens_query_stale_" + k] += _differs(op, self.answer(op, a, self.qprev), exp)
            except AssertionError:  # (a range that the earlier map does not hold)
                c["sens_query_stale_" + k] += 1
        if a["require_published"] and flags is not None and flags.any():
            c["sens_query_flags_" + k] += _differs(op, self.answer(op, a, (rec, None, now[2])), exp)
        # conditions on the sequence
        for e in QEVENTS:
            c["after_%s_%s" % (e, k)] += self.qlast == ("vmap_" + e, True)
        for e in QFIRST:  # (big: a map of more than BIG entries, whatever came before)
            c["first_" + e] += M > BIG if e == "big" else self.qlast[0] == ("set_pose" if e == "set_pose" else "vmap_" + e)
        if a["require_published"] and M:
            c[("pub_after_" if self.map.cl.calls else "pub_before_") + k] += 1
        if op == "vmap_cast_segments":
            c["rays_hit"] += exp["rays_hit"]
            c["rays_skipped"] += exp["rays_skipped"]
            c["rays_miss"] += exp["rays_total"] - exp["rays_hit"] - exp["rays_skipped"]
        elif op == "vmap_render":
            c["render_hit_and_zero"] += 0 < exp["rays_hit"] < exp["rays_total"]
        elif op == "vmap_components":
            c["comp_rich"] += exp["components"] >= 2 and exp["small"] > 0 and exp["members"] < exp["entries"]
        elif op == "vmap_normals":
            c["normals_rich"] += 0 < exp["estimated"] < exp["entries"] and exp["oriented"] > 0
            self.qnormal = ({f: a[f] for f in ("min_multiplicity", "require_published", "first", "count")}, exp["normal"].copy())
        else:
            c["mesh_quads_singles"] += exp["quads"] > 0 and exp["singles"] > 0
            c["mesh_empty"] += exp["entries"] > 0 and exp["triangles"] == 0
            c["mesh_" + a["source"]] += 1
        return {"refused": None, "answer": exp, "totals": totals}

    def _map(self, op, a):
        ref = self.refusal(op, a)
        if ref is not None:
            return self._refused(op, a, ref)
        mp, c = self.map, self.mcov
        vm, ol, cl = mp.vm, mp.ol, mp.cl
        M = vm.M
        mp.pad()
        self._sync_prev()
        res = {"refused": None}
        if op == "vmap_observe":
            slots, src, ms, mr, nbrs = a["slots"], a["source"], a["max_sigma"], a["min_rho"], a.get("nbrs")
            pl = cm.cloud(self.m, slots, src, ms, mr)
            sup = cm.support_words(self.m, slots, nbrs, pl) if nbrs is not None else None
            own = a["tags"] if a["tags"] is not None else slots
            ntags = None if nbrs is None else a["nbr_tags"] if a.get("nbr_tags") is not None else nbrs
            row = np.repeat(np.arange(len(slots)), np.diff(pl["offsets"]))
            index = (vm.keys, vm.ids)
            reads = set(slots) | set(int(j) for r in (nbrs or ()) for j in r)
            stale = None
            if nbrs is not None and self.before_pose is not None and self.before_pose[0] in reads:
                k, T = self.before_pose  # WRONG on purpose: the support words under the pose before the last set_pose
                now, self.m.Tcw[k] = self.m.Tcw[k], T
                stale = copy.copy(ol)
                stale_d = stale.observe(index, mp.voxel, pl["xyz"], row, cm.support_words(self.m, slots, nbrs, pl), own, ntags)
                self.m.Tcw[k] = now
            d = ol.observe(index, mp.voxel, pl["xyz"], row, sup, own, ntags)
            if stale is not None:
                c["sens_observe_pose"] += not (stale_d == d and np.array_equal(stale.entry, ol.entry) and
                                               np.array_equal(stale.tag, ol.tag))
            wrong = cm.plain(self.m, slots, src, ms, mr, listed_only=self.lam)
            c["sens_listed"] += not (np.array_equal(wrong[0], pl["offsets"]) and np.array_equal(wrong[1], pl["pixel"]))
            self.cov["points"] += len(pl["pixel"])
            for k in slots:
                for h in self.history(k):
                    self.cov["hist_" + h] += 1
            if nbrs is not None and self.posed & set(int(j) for r in nbrs for j in r):
                c["observe_after_set_pose"] += 1
            c["pairs_created"] += d["created"]
            if d["created"] > 0:
                self._event("observe")
            res.update(plain=pl, delta=d)
        elif op == "vmap_classify":
            exp = mp.classify(a["rule"], bool(a["commit"]))
            if a["commit"]:
                self._event("classify")
            if self.chain == 2 and exp["accepted"] + exp["retracted"] > 0:
                c["recarve_chain"] += 1
                self.chain = 0
            res.update(delta={f: exp[f] for f in COUNTS}, accepted_ids=exp["accepted_ids"], retracted_ids=exp["retracted_ids"])
        elif op == "vmap_import":
            exp = vi.import_records(vm, a["records"])
            mp.pad()
            self._sync_prev()
            res.update(delta={f: exp[f] for f in vi.DELTA}, dst_ids=exp["dst_ids"], updated_ids=exp["updated_ids"])
        elif op == "vmap_import_observations":
            res.update(delta=vi.import_observations(ol, M, a["entry"], a["tag"], a.get("entry_map")))
        elif op == "vmap_repose":
            tags, K, T = a["tags"], a["K"], a["T"]
            old = {f: vm.rec[f].copy() for f in ("xyz", "pixel", "tag")}
            if tags:  # WRONG on purpose: the table of the poses the map last saw
                known = [self.table[t]["known"] if t in self.table else P for t, P in zip(tags, T)]
                right, wrong = vrp.new_xyz(vm.rec, tags, K, T)[0], vrp.new_xyz(vm.rec, tags, K, known)[0]
                c["sens_repose_stale"] += right.tobytes() != wrong.tobytes()
            exp, mp.ev, cl.published = vrp.repose(vm, ol, tags, K, T, a["carry"], mp.ev, cl.flags(M))
            for t, P in zip(tags, T):
                if t in self.table:
                    self.table[t]["T"] = np.array(P, F).reshape(3, 4)
                    self.table[t]["known"] = self.table[t]["T"].copy()
            remap = exp["remap"].astype(np.int64)
            self.prev_xyz = vm.rec["xyz"].copy()
            at = np.flatnonzero(exp["remap"] != NOID)
            at = at[(old["pixel"][at] == vm.rec["pixel"][remap[at]]) & (old["tag"][at] == vm.rec["tag"][remap[at]])]
            self.prev_xyz[remap[at]] = old["xyz"][at]
            for f in ("moved", "merged", "dropped"):
                c["repose_" + f] += exp[f] > 0
            self.after["repose"] = set()
            self.chain = 0 if a["carry"] else 1
            c["carry_repose_published"] += bool(a["carry"] and self.published() > 0)
            res.update(delta={f: exp[f] for f in vrp.DELTA}, remap=exp["remap"])
        elif op == "vmap_retire":
            flags = cl.flags(M)
            other = vrt.plan(vm.rec["tag"], ol.entry, ol.tag, a["tags"], "unobserved" if a["mode"] == "winner" else "winner",
                             flags, a["carry"])  # WRONG on purpose: the other mode
            exp, ev2, fl2 = vrt.retire(vm, ol, a["tags"], a["mode"], bool(a["carry"]), mp.ev, flags, bool(a["commit"]))
            c["sens_retire_mode"] += not np.array_equal(other["remap"], exp["remap"])
            c["retire_%s_both" % a["mode"]] += exp["dropped"] > 0 and exp["removed"] > 0
            c["retire_orphaned"] += exp["orphaned"] > 0
            if a["commit"]:
                mp.ev, cl.published = ev2, fl2
                self.prev_xyz = self.prev_xyz[exp["remap"] != NOID]
                self.after["retire"] = set()
                self.fed -= set(a["tags"])
                self.chain = 0 if a["carry"] else 1
                c["carry_retire_published"] += bool(a["carry"] and self.published() > 0)
            res.update(delta={f: exp[f] for f in vrt.DELTA}, **{f: exp[f] for f in vrt.LISTS})
        elif op == "vmap_recarve":
            args = (ol.entry, ol.tag, a["tags"], a["T"], mp.voxel, a["end_margin"], a["max_steps"], a["first"], a["count"])
            exp = vrc.recarve((vm.keys, vm.ids), vm.rec["xyz"], *args)
            if self.prev_xyz.tobytes() != vm.rec["xyz"].tobytes():  # WRONG on purpose: the rays end where the records were
                wrong = vrc.recarve((vm.keys, vm.ids), self.prev_xyz, *args)
                c["sens_recarve_prev"] += any(not np.array_equal(wrong[f], exp[f]) for f in ("crossings", "ends"))
            mp.ev = vrc.accumulate(mp.ev, M, exp, a["reset"])
            c["recarve_unposed"] += exp["pairs_unposed"] > 0
            c["recarve_short"] += bool(a.get("short") and exp["rays_skipped"] > 0)
            whole = a["first"] == 0 and a["count"] in (None, ol.E)
            if self.chain == 1 and a["reset"] and whole and exp["rays_total"] > 0:
                self.chain = 2
            res.update(totals={f: exp[f] for f in vrc.OUTS})
        else:
            ids, first, count = a.get("ids"), a["first"], a["count"]
            sel = np.asarray(ids, np.int64) if ids is not None else np.arange(first, M if count is None else first + count)
            assert ((sel >= 0) & (sel < M)).all()
            if op == "vmap_fetch":
                got = vm.fetch(ids, first, count)
            elif op == "vmap_fetch_evidence":
                got = {f: mp.ev[f][sel] for f in ("crossings", "ends")}
            elif op == "vmap_fetch_cameras":
                offs, tags = ol.cameras(M, ids, first, count)
                got = {"cam_offsets": offs, "cam_tags": tags}
            else:
                got = {"published": cl.flags(M)[sel]}
            res.update(fetch=got, n=len(sel))
        return res


# ---- the sequences ------------------------------------------------------------------------------------------------------
def describe(op, a):
    """cloud_model.describe, with the records and pose tables of the new ops by size"""
    def short(v):
        if isinstance(v, dict):
            return {f: short(x) for f, x in v.items()}
        if isinstance(v, (list, tuple)) and v and isinstance(v[0], np.ndarray):
            return "<%d x %s>" % (len(v), "x".join(map(str, v[0].shape)))
        if isinstance(v, np.ndarray):
            return "<%s %s>" % (v.dtype, "x".join(map(str, v.shape))) if v.size > 40 else v.tolist()
        return v
    return "%s %r" % (op, {k: short(v) for k, v in a.items()})


def _table(w, tags):
    """(K, T) rows of the caller's table for tags; a tag it does not hold gets keyframe 0's"""
    K = [w.table[t]["K"] if t in w.table else np.array(w.seq.K, F).reshape(4) for t in tags]
    T = [w.table[t]["T"].copy() if t in w.table else np.array(w.seq.Tcw[0], F).reshape(3, 4) for t in tags]
    return K, T


def _absent(rng, n):
    return sorted(set(int(t) for t in rng.integers(2000, 3000, n)))


def _dest(rng, p=0.35):
    return "device" if rng.random() < p else "host"


def _read_args(rng, w, op, kw):
    """the cloud arguments of integrate, observe and carve from cloud_model's draw, the tags from this model"""
    keys = ("want", "refuse", "wide", "short", "rich", "neg")
    ckw = {k: kw[k] for k in keys if k in kw}
    ckw.setdefault("refuse", False)
    if kw.get("short") or kw.get("rich"):
        ckw["wide"] = True
    _, a = cm._cloud_args(rng, w, "vmap_carve" if op == "vmap_observe" else op, **ckw)
    if op == "vmap_carve":
        return op, a
    slots = a["slots"]
    if op == "vmap_observe":
        del a["end_margin"], a["max_steps"]
        k = kw.get("want_nbr")
        if k is not None and w.m.has_depth[k]:
            if a["nbrs"] is None:
                a["nbrs"] = cm._rows(rng, w, slots, cm.N_NBR, allow_self=True)
            a["nbrs"][0][0] = int(k)
        if kw.get("rows") and a["nbrs"] is None:
            a["nbrs"] = cm._rows(rng, w, slots, cm.N_NBR, allow_self=True)
        bare = [k for k in range(N_KF) if not w.m.has_depth[k]]
        bare = [k for k in bare if "reupload" in w.hist[k]] or bare  # (the ones uploaded again count as a history)
        unchecked = [k for k in range(N_KF) if w.m.has_depth[k] and not w.m.has_chk[k]]
        state = kw.get("state")
        if state == "no_depth" and bare:
            slots.append(int(rng.choice([k for k in bare if k not in slots])))
            if a["nbrs"] is not None:
                a["nbrs"].append(list(a["nbrs"][0]))
        elif state == "nbr_no_depth" and bare:
            if a["nbrs"] is None:
                a["nbrs"] = cm._rows(rng, w, slots, cm.N_NBR, allow_self=True)
            a["nbrs"][int(rng.integers(0, len(slots)))][int(rng.integers(0, len(a["nbrs"][0])))] = int(rng.choice(bare))
        elif state == "no_chk" and unchecked:
            a["source"] = 1
            pick = int(rng.choice(unchecked))
            if pick not in slots:
                slots.append(pick)
                if a["nbrs"] is not None:
                    a["nbrs"].append(list(a["nbrs"][0]))
    else:
        del a["tags"]
        if rng.random() < 0.2:
            a["dest"] = "none"  # updated == NULL: the delta alone
    mine = [w.tag(k) for k in slots]
    a["tags"] = None if mine == list(slots) and rng.random() < 0.5 else mine
    if op == "vmap_observe":
        a["nbr_tags"] = None
        if a["nbrs"] is not None and rng.random() < 0.6:
            a["nbr_tags"] = [[w.tag(j) for j in row] for row in a["nbrs"]]
    return op, a


def _best_rule(w, want_change=False):
    """the name of a rule under which entries pass (want_change: under which the flags change), from a dry run"""
    for name in ("seen", "lax", "near", "all"):
        exp = w.map.classify(RULES[name], False)
        if (exp["accepted"] + exp["retracted"] > 0) if want_change else \
                (exp["published_total"] + exp["accepted"] - exp["retracted"] > 0):
            return name
    return "all"


def _map_args(rng, w, op, kw):
    """the draw of one of the new calls; kw steers it (wrong: as it is, though no map is open)"""
    mp = w.map
    M = mp.vm.M if mp else 0
    E = mp.ol.E if mp else 0
    if op == "vmap_classify":
        name = kw.get("rule") or str(rng.choice(sorted(RULES)))
        if name.startswith("best"):  # (the dry runs only once the plan is taken)
            name = _best_rule(w, name == "best_change")
        rule = dict(RULE, ratio_den=0) if kw.get("den0") else dict(RULES[name])
        return op, {"rule": rule, "commit": int(kw.get("commit", rng.random() < 0.7)), "dest": str(rng.choice(["host", "device", "none"]))}
    if op == "vmap_import":
        voxel = mp.voxel if mp else 0.05
        if M:
            sel = rng.integers(0, M, int(rng.integers(1, min(M, 200) + 1)))
            rec = {f: mp.vm.rec[f][sel].copy() for f in ("xyz", "pixel", "rho_sigma", "intensity", "tag", "multiplicity")}
        else:
            n = 5
            rec = {"xyz": rng.normal(0, 1, (n, 3)).astype(F), "pixel": rng.integers(0, 99, n).astype(np.uint32),
                   "rho_sigma": rng.uniform(0.01, 1, (n, 2)).astype(F), "intensity": rng.integers(0, 255, n).astype(np.uint8),
                   "tag": np.zeros(n, np.int32), "multiplicity": np.ones(n, np.uint32)}
        shift = rng.choice([0, 0, 1, -1, 2, 6], 3)  # whole voxels: some records meet entries, some do not
        rec["xyz"] = (rec["xyz"] + (shift * voxel).astype(F)).astype(F)
        rec["rho_sigma"][:, 1] *= F(rng.choice([0.5, 1.0, 2.0]))  # (below, at and above the stored sigma: updates and ties)
        n = len(rec["pixel"])
        if n > 3:
            rec["multiplicity"][int(rng.integers(0, n))] = 0        # dropped
            rec["xyz"][int(rng.integers(0, n)), 1] = np.nan          # dropped
        extra = rng.random() < 0.6
        if not extra:
            del rec["tag"], rec["multiplicity"]
        return op, {"records": rec, "extra": extra, "dest": _dest(rng)}
    if op == "vmap_import_observations":
        P = int(rng.integers(1, 150))
        known = w.record_tags() + w.log_tags()
        pool = sorted(set(known)) + [1000 + int(t) for t in rng.integers(0, 6, 2)]
        tag = rng.choice(pool, P).astype(np.int32)
        tag[rng.random(P) < 0.05] = -1  # rejected
        emap = None
        if M and rng.random() < 0.4:
            L = int(rng.integers(1, M + 1))
            emap = rng.integers(0, M, L).astype(np.uint32)
            emap[rng.random(L) < 0.1] = NOID
            entry = rng.integers(0, L + 2, P).astype(np.uint32)  # (some beyond the map: rejected)
        else:
            entry = (rng.integers(0, M, P) if M else np.zeros(P)).astype(np.uint32)
            entry[rng.random(P) < 0.1] += np.uint32(M)          # beyond the entries: rejected
            if E:  # pairs the log holds already
                at = rng.integers(0, E, P // 3)
                entry[:len(at)], tag[:len(at)] = mp.ol.entry[at], mp.ol.tag[at]
        return op, {"entry": entry, "tag": tag, "entry_map": emap, "dest": _dest(rng)}
    if op == "vmap_repose":
        pres = [int(t) for t in w.record_tags() if 0 <= t < (1 << 31)]
        tags = [t for t in pres if rng.random() < 0.7 or t in kw.get("include", ())] + _absent(rng, int(rng.integers(0, 3)))
        if kw.get("empty") or (not kw and rng.random() < 0.1):
            tags = []  # n_poses == 0
        tags = [int(t) for t in rng.permutation(tags)]
        K, T = _table(w, tags)
        gone = [i for i, t in enumerate(tags) if t in w.table and not w.live(t)]
        for i in gone:  # the caller's poses of keyframes whose slots are gone move with the loop closure
            if kw.get("jolt") or rng.random() < 0.4:
                T[i] = jolt(rng, T[i])
        if kw.get("nan") and gone:
            T[gone[0]] = T[gone[0]].copy()
            T[gone[0]][:, 3] = np.nan  # a non-finite pose is no error: its entries' xyz are unmergeable
        if kw.get("dup"):
            tags, K, T = (tags + tags[:1], K + K[:1], T + T[:1]) if tags else ([7, 7],) + tuple(x * 2 for x in _table(w, [7]))
        return op, {"tags": tags, "K": K, "T": T, "carry": int(kw.get("carry", rng.integers(0, 2))),
                    "dest": str(rng.choice(["host", "device", "none"]))}
    if op == "vmap_retire":
        pres = sorted(set(t for t in w.record_tags() + w.log_tags() if 0 <= t < (1 << 31)))
        if "R" in kw:
            tags = list(kw["R"])
        elif rng.random() < 0.1:
            tags = []
        else:
            tags = [int(t) for t in pres if rng.random() < 0.3] + _absent(rng, int(rng.integers(0, 3)))
        tags = [int(t) for t in rng.permutation(tags)]
        if kw.get("dup"):
            tags = tags + tags[:1] if tags else [7, 7]
        return op, {"tags": tags, "mode": kw.get("mode") or str(rng.choice(["winner", "unobserved"])),
                    "carry": int(kw.get("carry", rng.integers(0, 2))), "commit": int(kw.get("commit", rng.random() < 0.7)),
                    "dest": str(rng.choice(["host", "device", "none"]))}
    if op == "vmap_recarve":
        pres = [int(t) for t in w.log_tags()]
        every = kw.get("whole") and not kw.get("subset")
        tags = [t for t in pres if every or rng.random() < 0.75] + _absent(rng, int(rng.integers(0, 2)))
        tags = [int(t) for t in rng.permutation(tags)]
        _, T = _table(w, tags)
        first, count = 0, None
        if not kw.get("whole") and E and rng.random() < 0.45:
            first = int(rng.integers(0, E + 1))
            count = int(rng.integers(0, E - first + 1))
        a = {"tags": tags, "T": T, "reset": int(kw.get("reset", rng.integers(0, 2))), "first": first, "count": count,
             "end_margin": int(rng.integers(0, 3)), "max_steps": int(rng.choice([4096, 65536]))}
        if kw.get("dup"):
            a["tags"], a["T"] = (tags + tags[:1], T + T[:1]) if tags else ([7, 7], _table(w, [7, 7])[1])
        elif kw.get("beyond"):
            a["first"], a["count"] = E, 1
        elif mp and E and (kw.get("short") or rng.random() < 0.25):  # below the longest walk of this very call, from the model
            dry = vrc.recarve((mp.vm.keys, mp.vm.ids), mp.vm.rec["xyz"], mp.ol.entry, mp.ol.tag, tags, T, mp.voxel,
                              a["end_margin"], 65536, first, count)
            longest = int(dry["steps"].max(initial=0))
            if longest > 1:
                a["max_steps"], a["short"] = max(longest - 1 - int(rng.integers(0, 3)), 1), True
        return op, a
    assert op in FETCHES
    a = {"ids": None, "first": 0, "count": None, "dest": _dest(rng)}
    if M and rng.random() < 0.5:
        ids = rng.integers(0, M, int(rng.integers(2, 40))).astype(np.uint32)
        ids[-1] = ids[0]  # ids may repeat
        a["ids"] = ids
    elif rng.random() < 0.7:
        a["first"] = int(rng.integers(0, M + 1))
        a["count"] = int(rng.integers(0, M - a["first"] + 1))
    return op, a


def _placed(w, k):
    """most points of the slot's depth map have an xyz: its point set was written after the map last changed (a point set
    is all zeros until a point-set call writes it, and every point without one falls into the voxel of the origin)"""
    xyz = cm.cloud(w.m, [k], 0, 0.3, 1e-6)["xyz"]
    return None if not len(xyz) else bool(xyz.any(axis=1).mean() > 0.5)  # (None: the depth map holds no point)


def _retire_pick(w, mode, orphan=False):
    """R of one tag whose retiring in `mode` drops entries and removes pairs of survivors (orphan: leaves orphans)"""
    vm, ol = w.map.vm, w.map.ol
    pool = set(w.log_tags()) & set(w.record_tags()) if orphan or mode == "winner" else set(w.log_tags())
    for t in sorted(pool, key=lambda t: w.live(t)):
        if t < 0:
            continue
        d = vrt.plan(vm.rec["tag"], ol.entry, ol.tag, [t], mode)
        if (d["orphaned"] > 0) if orphan else (d["dropped"] > 0 and d["removed"] > 0 and d["voxels"] > 0):
            return [int(t)]
    return None


def _plans(rng, w, room):
    """the calls that would close a gap of the coverage now, as (op, keywords of the draw)"""
    m, c, cc, mp = w.m, w.mcov, w.cov, w.map
    last, touched = w.last
    ks = range(N_KF)
    deep = [k for k in ks if m.has_depth[k]]
    bare = [k for k in ks if not m.has_depth[k]]
    unchecked = [k for k in deep if not m.has_chk[k]]
    out = []
    if mp is None:
        if room:
            for name in NO_MAP:
                if c["refuse_no_map_" + name] < 1:
                    out.append((str(rng.choice(FETCHES)) if name == "fetch" else "vmap_" + name, dict(wrong=True)))
        return out or [("vmap_open", {})]
    M, E = mp.vm.M, mp.ol.E
    read = lambda: str(rng.choice(READS))
    placed = lambda: {k: _placed(w, k) for k in deep}  # (a cloud per keyframe: only where a plan needs it)
    content = any(c[k] < 1 for k in CONTENT)  # a gap that only a map with entries and pairs can close
    if content and M < 50:
        at = placed()
        unseen = [k for k in deep if at[k] and w.tag(k) not in w.fed]
        if unseen:
            return [("vmap_integrate", dict(rich=True, want=tuple(unseen[:2])))]
        if [k for k in deep if at[k] is False]:
            return [("pointset0", dict(want=tuple(k for k in deep if at[k] is False)[:3]))]
        if mp.vm.calls >= 4:  # every keyframe is in and the map is still small: a finer one
            return [("vmap_close", dict(forced=True, must=True))]
    if content and E == 0:
        return [("vmap_observe", dict(rich=True, rows=True))]
    if room:
        for name in TWICE:
            if c["refuse_twice_" + name] < 1:
                out.append(("vmap_" + name, dict(dup=True)))
        if c["refuse_ratio_den"] < 1:
            out.append(("vmap_classify", dict(den0=True)))
        if c["refuse_range"] < 1:
            out.append(("vmap_recarve", dict(beyond=True)))
        rebare = [k for k in bare if "reupload" in w.hist[k]]
        for s in OBS_STATES:
            if c["refuse_obs_" + s] < 1 or (s == "no_depth" and cc["hist_reupload"] < 1):
                if unchecked if s == "no_chk" else (rebare if s == "no_depth" and cc["hist_reupload"] < 1 else bare):
                    out.append(("vmap_observe", dict(state=s, want=tuple(bare) if s == "no_depth" else ())))
                elif s != "no_chk" and last != "reupload":
                    out.append(("reupload", {}))
                elif s == "no_chk":
                    out.append(("recon+batch", {}))
    # the histories of the slots a map call reads (cloud_model._plans, for the three reading calls)
    rebuilt = [k for k in deep if "lam_rebuilt" in w.history(k)]
    stale = [k for k in deep if w.recon_lam[k] not in (None, w.lam) and w.list_lam[k] != w.lam]
    other = [k for k in deep if not w.pipeline_state(k)]
    if last == "lambda" and cc["hist_lam_stale"] < 1 and deep:
        out.append((read(), dict(want=tuple(deep[:2]))))
    if cc["hist_lam_rebuilt"] < 1:
        if rebuilt:
            out.append((read(), dict(want=tuple(rebuilt[:3]))))
        elif stale and last != "lambda":
            out.append((str(rng.choice(["intra_check", "pointset0"])), dict(want=tuple(stale[:3]))))
    if cc["hist_lam_stale"] < 1 and stale:
        out.append((read(), dict(want=tuple(stale[:3]))))
    if last in ("upload_depth", "assume", "inter_commit") and cc["hist_" + last] < 1 and touched and all(m.has_depth[k] for k in touched):
        out.append((read(), dict(want=tuple(touched[:3]))))
    for h in ("upload_depth", "inter_commit", "assume"):
        if cc["hist_" + h] < 1 and last != h:
            out.append((h, {}))
    if (cc["hist_lam_stale"] < 1 or cc["hist_lam_rebuilt"] < 1) and not stale and not rebuilt and last != "lambda":
        out.append(("lambda", {}))
    if cc["sensitive_calls"] + c["sens_listed"] < 1 and other:
        out.append((read(), dict(want=tuple(other[:3]), neg=True)))
    # an observe behind a set_pose of one of its neighbours
    if c["observe_after_set_pose"] < 1 or c["sens_observe_pose"] < 1:
        if last == "set_pose" and m.has_depth[touched[0]]:
            seen = [k for k in deep if w.tag(k) in w.record_tags() and k != touched[0]]
            return [("vmap_observe", dict(want_nbr=touched[0], rich=True, want=tuple(seen[:2])))]
        out.append(("set_pose", dict(big=True)))
    # repose: moved, merged, dropped, carried flags
    rec_tags = [t for t in w.record_tags() if t in w.table]
    moved = [t for t in rec_tags if w.table[t]["T"].tobytes() != w.table[t]["known"].tobytes()]
    gone = [t for t in rec_tags if not w.live(t)]
    far = len(w.prev_xyz) == M and bool((np.abs(w.prev_xyz - mp.vm.rec["xyz"]).max(axis=1) > mp.voxel / 2).any())
    if c["repose_moved"] < 1 or c["sens_repose_stale"] < 1 or (c["sens_recarve_prev"] < 1 and not far):
        out.append(("vmap_repose", dict(include=tuple(moved))) if moved else ("set_pose", dict(big=True)))
    if c["repose_merged"] < 1 or c["repose_dropped"] < 1:
        if gone:
            out.append(("vmap_repose", dict(include=tuple(gone), jolt=True, nan=c["repose_dropped"] < 1)))
        elif rec_tags and last != "reupload":
            out.append(("reupload", dict(k=int(rng.choice(rec_tags)) % N_KF)))
    for kind in ("repose", "retire"):
        if c["carry_%s_published" % kind] < 1:
            if w.published() == 0:
                out.append(("vmap_classify", dict(rule="best", commit=1)))
            elif kind == "repose":
                out.append(("vmap_repose", dict(carry=1)))
            else:
                out.append(("vmap_retire", dict(carry=1, commit=1, mode="winner", R=_absent(rng, 1))))
    # growth on the rebuilt table and set
    for kind in ("repose", "retire"):
        seen = w.after[kind]
        if c["grown_after_" + kind] < 1 and seen is not None:
            nxt = [g for g in GROWTH if g not in seen][0]
            at = placed() if nxt in ("integrate", "observe") else {}
            fresh = [k for k in deep if at.get(k) and w.tag(k) not in w.fed]
            if nxt == "integrate" and not fresh:  # a keyframe the map has not seen, with its point set written
                unseen = [k for k in deep if w.tag(k) not in w.fed and at[k] is False]
                return [("pointset0", dict(want=tuple(unseen[:2])))] if unseen else [("reupload", {})] if last != "reupload" else []
            plan = {"integrate": ("vmap_integrate", dict(rich=True, want=tuple(fresh[:2]))),
                    "observe": ("vmap_observe", dict(rich=True, rows=True, want=tuple(fresh[:2]))),
                    "carve": ("vmap_carve", dict(wide=True)), "classify": ("vmap_classify", dict(commit=1))}[nxt]
            return [plan]
    if c["grown_after_repose"] < 1 and w.after["repose"] is None:
        out.append(("vmap_repose", {}))
    # retire: per mode entries dropped and pairs of survivors removed; orphans
    for key, mode, orphan in (("retire_winner_both", "winner", False), ("retire_unobserved_both", "unobserved", False),
                              ("retire_orphaned", "unobserved", True)):
        if c[key] < 1:
            R = _retire_pick(w, mode, orphan)
            if R:
                out.append(("vmap_retire", dict(mode=mode, R=R, commit=int(c["grown_after_retire"] < 1 or rng.random() < 0.5))))
            else:
                out.append(("vmap_observe", dict(rich=True, rows=True)))
    if c["grown_after_retire"] < 1 and w.after["retire"] is None:
        out.append(("vmap_retire", dict(commit=1)))
    # the loop-closure recipe's tail: carry 0, a recarve of the whole log with reset, a classify that changes flags
    if c["recarve_chain"] < 1:
        if w.chain == 0:
            out.append(("vmap_repose", dict(carry=0)))
        elif w.chain == 1:
            return [("vmap_recarve", dict(whole=True, reset=1))]
        else:
            return [("vmap_classify", dict(rule="best_change"))]
    if c["recarve_unposed"] < 1:
        out.append(("vmap_recarve", dict(subset=True)))
    if c["recarve_short"] < 1:
        out.append(("vmap_recarve", dict(short=True)))
    if c["sens_recarve_prev"] < 1 and far:  # records that the last repose moved by more than half a voxel
        out.append(("vmap_recarve", dict(whole=True)))
    return out


def generate(seed, w, steps=STEPS, queries=True):
    """yields (op, args); the caller applies each to the MapWorld (and to an engine) before asking for the next, so every
    draw is a function of the seed and the model's state alone.  Weighted random draws; the gaps the coverage conditions
    still have are closed with rising urgency as the steps run out (cloud_model.generate's scheme).

    queries: the five read-only queries are interleaved from a stream of their own (QueryStream: a second RNG, counters of
    its own).  The main stream neither sees nor counts them: with the QUERY_OPS filtered out the sequence is the one that
    queries=False yields, which tests/test_mapfuzz_cpu.py asserts."""
    q = QueryStream(seed, w, steps) if queries else None
    for step, (op, a) in enumerate(_main_stream(seed, w, steps)):
        yield op, a
        if q is not None:
            yield from q.behind(step, op, a)


def _main_stream(seed, w, steps):
    rng = np.random.default_rng(9100 + seed)
    p = np.array([_WEIGHT[o] for o in OPS], float)
    p /= p.sum()
    for step in range(steps):
        m, c = w.m, w.mcov
        kw, op = {}, None
        need = {o: 3 - w.count[o] for o in OPS if w.count[o] < 3}
        # refusals stay below a fifth of the map calls (the first few, before a map is open, on credit)
        room = 5 * (c["refusals"] + 1) <= c["map_calls"] + (40 if 2 * step < steps else 0)
        plans = _plans(rng, w, room)
        left = steps - step
        urgent = left <= 2.0 * len(plans) + sum(need.values()) + 10
        bare = [k for k in range(N_KF) if not m.has_depth[k]]
        if sum(m.has_depth.values()) < 5:
            op = "recon"
        elif need and left <= sum(need.values()) + 3:  # the last steps belong to the op kinds still short of three
            names = sorted(need)
            op, kw = str(rng.choice(names, p=np.array([need[o] for o in names], float) / sum(need.values()))), \
                dict(forced=True, must=True)
        elif plans and (urgent or plans[0][1].get("wrong") or rng.random() < 0.55):
            op, kw = plans[0] if len(plans) == 1 or rng.random() < 0.4 else plans[int(rng.integers(0, len(plans)))]
        elif bare and rng.random() < 0.4:
            op = "recon"
        elif need and left <= 2 * sum(need.values()) + 8 and rng.random() < 0.9:
            names = sorted(need)
            op, kw = str(rng.choice(names, p=np.array([need[o] for o in names], float) / sum(need.values()))), dict(forced=True)
        if op is None:
            op = str(rng.choice(OPS, p=p))
        # the map's life: open before use, close before opening again; a call in the wrong state only as a steered refusal
        if op in MAP_OPS and not kw.get("wrong"):
            # a map with entries lives until the gaps that need one are closed
            busy = w.map is not None and w.map.vm.M >= 50 and any(c[k] < 1 for k in CONTENT)
            if op == "vmap_open" and w.map is not None and kw.get("forced"):
                op = "vmap_close"
            elif op == "vmap_open" and w.map is not None:
                op = "vmap_close" if (w.count["vmap_close"] < 3 and w.map.vm.calls >= 4 and not busy) else "vmap_integrate"
            elif op != "vmap_open" and w.map is None:
                op, kw = "vmap_open", {}
            elif op in ("vmap_clear", "vmap_close") and (w.map.vm.calls < 4 or busy) and not kw.get("must"):
                op, kw = "vmap_observe" if w.map.vm.M else "vmap_integrate", {}
        if op in cm.PIPE_OPS:
            if op == "reupload" and "k" in kw:
                yield op, {"k": kw["k"]}
            else:
                o, a = cm._pipeline_args(rng, w, op, kw.get("want", ()))
                if o == "set_pose" and (kw.get("big") or rng.random() < 0.5):  # (cloud_model's 1e-4 rarely flips a support bit)
                    a["T"][:, 3] += rng.normal(0, 1e-2 if kw.get("big") else 3e-3, 3).astype(F)
                yield o, a
        elif op in ("vmap_open", "vmap_clear", "vmap_close"):
            o, a = cm._cloud_args(rng, w, op)
            if op == "vmap_open" and any(c[k] < 1 for k in CONTENT) and a["voxel"] == cm.VOXELS[2]:
                a["voxel"] = float(cm.VOXELS[int(rng.integers(0, 2))])  # (at 0.1 the whole scene is a few dozen entries)
            yield o, a
        elif op in READS:
            yield _read_args(rng, w, op, kw)
        else:
            yield _map_args(rng, w, op, kw)


def crafted_normals(rng, n, mode="mixed"):
    """float32[n, 3] for vmap_mesh, the cases vmap_mesh_np.STATS names: "zero" -- no owner at all; "axis" -- every normal
    along one axis; "mixed" -- per entry a random normal, an axis-aligned one, a tie of two or of three magnitudes, a zero
    row, a NaN row or a NaN component"""
    out = np.zeros((n, 3), F)
    if mode == "zero":
        return out
    if mode == "axis":
        out[:, int(rng.integers(0, 3))] = rng.choice(np.array([1, -1], F), n)
        return out
    out[:] = rng.normal(size=(n, 3))
    kind = rng.integers(0, 8, n)
    for i in np.flatnonzero(kind > 1):
        s = abs(out[i, 0]) + F(0.5)
        out[i] = {2: (0, 0, s), 3: (0, -s, 0), 4: (s, -s, s / 4), 5: (s, s, -s), 6: (0, 0, 0)}.get(int(kind[i]), (np.nan,) * 3)
    if n:
        out[int(rng.integers(0, n)), int(rng.integers(0, 3))] = np.nan
    return out


class QueryStream:
    """The five read-only queries beside the main stream: what to issue behind the main stream's step that has just been
    applied.  Draws come from an RNG of its own and the counters are MapWorld.qcov, so the main stream is as it would be
    without them.  Queries are issued with probability RATE behind any call while a map is open, and steered: behind a
    repose, a committing retire and a committing classify every kind that has not followed one yet; behind the first clear,
    import and set_pose and once the map exceeds BIG entries all five; with require_published before the first committing
    classify of a map and when entries are published; where the content conditions of check_query_coverage are open on a
    map of more than BIG entries; and the refusals, while they stay below a fifth of the stream's calls."""
    RATE = 0.02  # (nearly all of a sequence's 60 to 70 queries are steered; EXPERIMENTS.md has what a query costs)
    TRIES = 5  # of a steered query whose condition may stay open on this map

    def __init__(self, seed, w, steps):
        self.rng, self.w, self.steps = np.random.default_rng(9300 + seed), w, steps
        self.tries = {}

    def _try(self, key):
        self.tries[key] = self.tries.get(key, 0) + 1
        return self.tries[key] <= self.TRIES

    def behind(self, step, op, a):
        w, c, rng = self.w, self.w.qcov, self.rng
        if op == "recon+batch":  # (the call drawn next runs straight behind the overlapped batch: test_gpu_mapfuzz.MapRun.run)
            return
        late = 4 * step > 3 * self.steps
        room = lambda: 5 * (c["refusals"] + 1) <= c["calls"] + (25 if 2 * step < self.steps else 0)
        if w.map is None:
            short = [k for k in QKINDS if c["refuse_no_map_" + k] < 1]
            if short and room():
                yield self.draw("vmap_" + short[0])
            return
        mp, ok = w.map, w.qapplied
        M = mp.vm.M
        event = "repose" if ok and op == "vmap_repose" else \
            op[5:] if ok and op in ("vmap_retire", "vmap_classify") and a["commit"] else None
        first = [e for e, hit in (("clear", ok and op == "vmap_clear"), ("import", ok and op == "vmap_import"),
                                  ("set_pose", op == "set_pose"), ("big", M > BIG)) if hit and c["first_" + e] < 1]
        todo = {}
        for k in QKINDS:
            kw = None
            if first or (event and c["after_%s_%s" % (event, k)] < 1):
                kw = {}
            if w.qchanged and M and w.qprev is not None and c["sens_query_stale_" + k] < 1 and self._try(("stale", k)):
                kw = {}
            if M and mp.cl.calls == 0 and c["pub_before_" + k] < 1:
                kw = {"pub": 1}
            if w.published() > 0 and (c["pub_after_" + k] < 1 or (c["sens_query_flags_" + k] < 1 and self._try(("flags", k)))):
                kw = {"pub": 1}
            if late and c["n_" + k] < 3:
                kw = kw or {}
            if kw is not None:
                todo[k] = dict(kw, content=True)
        if M > BIG:  # the conditions on what the answers hold
            for key, k, kw in (("rays_hit", "cast_segments", {}), ("rays_miss", "cast_segments", {}),
                               ("rays_skipped", "cast_segments", {}), ("render_hit_and_zero", "render", {}),
                               ("comp_rich", "components", {}), ("normals_rich", "normals", {}),
                               ("mesh_quads_singles", "mesh", {}), ("mesh_from_normals", "mesh", {})):
                if c[key] < 1 and k not in todo and self._try(key):
                    todo[k] = dict(kw, content=True)
                    if k == "mesh" and w.qnormal is None:
                        todo.setdefault("normals", dict(content=True))
        for k in QKINDS:  # (normals before the mesh that takes them)
            if k in todo:
                yield self.draw("vmap_" + k, **todo[k])
        for key, mode in (("mesh_empty", "zero"), ("mesh_crafted", "mixed")):
            if M and c[key] < 1 and (M > BIG or late):
                yield self.draw("vmap_mesh", crafted=mode)
        open_ = [r for r in QINVALID if c["refuse_" + r] < 1]
        if open_ and room():
            item = self.refused(open_[0] if late or len(open_) == 1 else str(rng.choice(open_)))
            if item is not None:
                yield item
        behind_ = 5 * c["refusals"] > c["calls"]  # (the first refusals came on credit: the stream owes the calls)
        owing = behind_ or (open_ and not room())
        if rng.random() < (1 if late and owing else 3 * self.RATE if owing else self.RATE):
            yield self.draw(str(rng.choice(QUERY_OPS)))

    def refused(self, kind):
        """a call that must be refused with SDM_EINVAL, or None where this map has none of the kind"""
        rng, w = self.rng, self.w
        M = w.map.vm.M
        if kind == "published2":
            return self.draw(str(rng.choice(QUERY_OPS)), refuse=kind)
        if kind == "connectivity":
            return self.draw("vmap_components", refuse=kind)
        if kind in ("radius", "twice"):
            return self.draw("vmap_normals", refuse=kind)
        if kind == "range":
            return self.draw(str(rng.choice(["vmap_normals", "vmap_mesh"])), refuse=kind)
        op, a = self.draw("vmap_components" if kind == "small_short" else "vmap_mesh", refuse=kind)
        dry = w.answer(op, a, w.qnow)  # the destination is one short of these totals: there must be two at least
        return (op, a) if M and dry["small" if kind == "small_short" else "triangles"] >= 2 else None

    def segments(self, n):
        """n segments: the occlusion test of pairs of the log (from the centre of the tag's current pose to the entry),
        random ones through the map's bounding box, degenerate ones and ones with a coordinate that is not finite"""
        rng, w = self.rng, self.w
        mp = w.map
        xyz = mp.vm.rec["xyz"] if mp is not None else np.zeros((0, 3), F)
        fin = xyz[np.isfinite(xyz).all(axis=1)]
        lo, hi = (fin.min(axis=0) - mp.voxel, fin.max(axis=0) + mp.voxel) if len(fin) else (-np.ones(3), np.ones(3))
        pairs = [i for i in range(mp.ol.E) if int(mp.ol.tag[i]) in w.table] if mp is not None else []
        centre = {}
        kinds = rng.choice(4, n, p=[0.45, 0.45, 0.05, 0.05])
        if n >= 4:
            kinds[:4] = np.arange(4)
        O, P = rng.uniform(lo, hi, (n, 3)).astype(F), rng.uniform(lo, hi, (n, 3)).astype(F)
        for i in range(n):
            if kinds[i] == 0 and pairs:
                j = int(rng.choice(pairs))
                t = int(mp.ol.tag[j])
                if t not in centre:
                    centre[t] = carve_np.camera_centre(w.table[t]["T"])
                O[i], P[i] = centre[t], xyz[int(mp.ol.entry[j])]
            elif kinds[i] == 2:
                P[i] = O[i]
            elif kinds[i] == 3:
                P[i, int(rng.integers(0, 3))] = rng.choice(np.array([np.nan, np.inf, -np.inf], F))
        return O, P

    def draw(self, op, content=False, pub=None, crafted=None, refuse=None):
        """the draw of one query; content: the arguments under which the answer holds the most; pub: require_published;
        crafted: the mesh's normals; refuse: the argument that is wrong (with no map open every call is refused as it is)"""
        rng, w = self.rng, self.w
        mp = w.map
        M = mp.vm.M if mp is not None else 0
        plain = content or refuse is not None
        a = {"min_multiplicity": 0 if plain else int(rng.integers(0, 3)),
             "require_published": 2 if refuse == "published2" else int(rng.random() < 0.25 and not plain) if pub is None else int(pub),
             "dest": _dest(rng)}

        def window():
            a["first"], a["count"] = 0, None
            if refuse == "range":
                a["first"], a["count"] = M, 1
            elif not plain and rng.random() < 0.4:
                a["first"] = int(rng.integers(0, M + 1))
                a["count"] = int(rng.integers(0, M - a["first"] + 1))

        if op in ("vmap_cast_segments", "vmap_render"):
            a.update(start_margin=0 if plain else int(rng.integers(0, 3)), end_margin=0 if plain else int(rng.integers(0, 3)),
                     max_steps=4096 if plain else int(rng.choice([4096, 65536, 48])))
        if op == "vmap_cast_segments":
            n = 130 if content else int(rng.choice([1, 65, int(rng.integers(150, 300))]))
            a["origins"], a["ends"] = self.segments(n)
        elif op == "vmap_render":
            t = int(rng.choice(sorted(t for t in w.table if w.live(t))))
            T = w.table[t]["T"].copy()
            if not plain and rng.random() < 0.5:
                T = jolt(rng, T)
            c = w.qcov  # (the large view where its hits are still needed: a 9 x 7 view of a sparse map often has none)
            large = content and (c["render_hit_and_zero"] < 1 or (pub and c["sens_query_flags_render"] < 1))
            W, H = (33, 17) if large or rng.random() < 0.1 else (9, 7)
            K = np.array(w.seq.K, F).reshape(4) * np.array([W / cm.W, H / cm.H, W / cm.W, H / cm.H], F)
            # (the slab lies at depths 1 .. 1.1: rays to depth 1.25 cross it; the restatement's cost grows with their length)
            a.update(K=K.astype(F), T=T, W=W, H=H, rho_far=0.8 if plain else float(rng.choice([0.8, 0.5, 1.5])))
        elif op == "vmap_components":
            a.update(connectivity=12 if refuse == "connectivity" else int(rng.choice([6, 18, 26])),
                     min_size=4 if content else int(rng.choice([0, 3, 6])))
            if content and pub is None:
                a["min_multiplicity"] = 2
            if refuse == "small_short":
                a.update(min_size=M + 1, short=True)
        elif op == "vmap_normals":
            held = [int(t) for t in w.record_tags() if t in w.table]
            tags = [t for t in held if plain or rng.random() < 0.7]
            tags += [t for t in sorted(w.table) if t not in held][:1] or _absent(rng, 1)  # a tag the map does not hold
            tags = [int(t) for t in rng.permutation(tags)]
            if refuse == "twice":
                tags = tags + tags[:1]
            if not plain and rng.random() < 0.3:
                tags = None
            a.update(tags=tags, T=None if tags is None else _table(w, tags)[1], radius=3 if refuse == "radius" else
                     1 if plain else int(rng.choice([1, 2])), min_points=3 if plain else int(rng.choice([3, 4, 6])))
            window()
        else:
            src = w.qnormal
            if refuse == "tri_short":
                a["short"] = True
            if crafted is None and refuse != "range" and src is not None and (plain or rng.random() < 0.6) and \
                    (pub is None or src[0]["require_published"] == pub):
                a.update(src[0], normal=src[1].copy(), source="from_normals")
            else:
                window()
                n = (M - a["first"] if a["count"] is None else a["count"]) if mp is not None else 0
                mode = crafted or ("axis" if plain else str(rng.choice(["mixed", "axis", "zero"], p=[0.6, 0.3, 0.1])))
                a.update(normal=crafted_normals(rng, n, mode), source="crafted")
            if refuse == "published2":
                a["require_published"] = 2
        return op, a


def online_recipe(w):
    """the online recipe the headers describe, as one fixed sequence: per block integrate, observe, carve, classify; on
    loop closure set_pose, repose, retire, recarve, classify; then records and pairs as from another rank, and the fetches.
    A generator like generate(): the later arguments are read from the model as it stands then."""
    seq = w.seq
    ks = list(range(N_KF))
    rows = lambda slots: [[int(j) for j in seq.neighbours(k, cm.N_NBR)] for k in slots]
    cloud = dict(source=0, max_sigma=0.3, min_rho=1e-6)
    yield "recon", {"refs": ks, "nbrs": rows(ks)}
    yield "pointset0", {"refs": ks}
    yield "vmap_open", {"voxel": 0.01}
    for blk in ([0, 1, 2], [3, 4]):
        yield "vmap_integrate", dict(cloud, slots=blk, tags=None, dest="host")
        yield "vmap_observe", dict(cloud, slots=blk, nbrs=rows(blk), tags=None, nbr_tags=None)
        yield "vmap_carve", dict(cloud, slots=blk, nbrs=rows(blk), end_margin=1, max_steps=4096)
        yield "vmap_classify", {"rule": dict(SEEN), "commit": 1, "dest": "host"}
    rng = np.random.default_rng(5)
    for k in (1, 3):  # the loop closure moves two keyframes
        yield "set_pose", {"k": k, "T": jolt(rng, seq.Tcw[k], 0.01)}
    tags = [3, 1, 0]
    K, T = _table(w, tags)
    yield "vmap_repose", {"tags": tags, "K": K, "T": T, "carry": 0, "dest": "host"}
    yield "vmap_retire", {"tags": [2], "mode": "unobserved", "carry": 0, "commit": 1, "dest": "host"}
    tags = [0, 1, 3, 4]
    yield "vmap_recarve", {"tags": tags, "T": _table(w, tags)[1], "reset": 1, "first": 0, "count": None, "end_margin": 1,
                           "max_steps": 4096}
    yield "vmap_classify", {"rule": dict(SEEN), "commit": 1, "dest": "device"}
    mp = w.map
    sel = np.arange(0, mp.vm.M, 3)
    rec = {f: mp.vm.rec[f][sel].copy() for f in ("xyz", "pixel", "rho_sigma", "intensity", "tag", "multiplicity")}
    rec["xyz"] = (rec["xyz"] + F(2 * mp.voxel)).astype(F)
    yield "vmap_import", {"records": rec, "extra": True, "dest": "device"}
    half = mp.ol.E // 2
    yield "vmap_import_observations", {"entry": mp.ol.entry[:half].copy(), "tag": (mp.ol.tag[:half] + 100).astype(np.int32),
                                       "entry_map": None, "dest": "host"}
    yield "vmap_classify", {"rule": dict(RULE), "commit": 1, "dest": "host"}
    for op in FETCHES:
        yield op, {"ids": None, "first": 0, "count": None, "dest": "host"}
    # the consumer's step: small components, normals, the mesh from them, the occlusion test of the log's pairs, a view
    flt = dict(min_multiplicity=0, require_published=0)
    yield "vmap_components", dict(flt, connectivity=26, min_size=4, dest="host")
    tags = [int(t) for t in w.record_tags() if t in w.table]
    yield "vmap_normals", dict(flt, tags=tags, T=_table(w, tags)[1], radius=1, min_points=3, first=0, count=None, dest="device")
    yield "vmap_mesh", dict(w.qnormal[0], normal=w.qnormal[1].copy(), source="from_normals", dest="device")
    at = np.flatnonzero(np.isin(mp.ol.tag, sorted(w.table)))  # (the pairs imported as from another rank have no pose here)
    O = np.stack([carve_np.camera_centre(w.table[int(t)]["T"]) for t in mp.ol.tag[at]]).astype(F)
    yield "vmap_cast_segments", dict(flt, origins=O, ends=mp.vm.rec["xyz"][mp.ol.entry[at].astype(np.int64)].copy(),
                                     start_margin=0, end_margin=1, max_steps=4096, dest="host")
    Wr, Hr = 33, 17
    K = np.array(seq.K, F).reshape(4) * np.array([Wr / cm.W, Hr / cm.H, Wr / cm.W, Hr / cm.H], F)
    yield "vmap_render", dict(flt, K=K.astype(F), T=w.table[0]["T"].copy(), W=Wr, H=Hr, rho_far=0.3, start_margin=0, end_margin=0,
                              max_steps=4096, dest="host")


def check_query_coverage(w, seed):
    """the conditions every sequence's query stream must meet (counted by MapWorld._query, on the model alone)"""
    c = w.qcov
    what = "seed %d: %r" % (seed, c)
    for k in QKINDS:
        assert c["n_" + k] >= 3, ("query kind %s is answered %d times" % (k, c["n_" + k]), what)
        for e in QEVENTS:  # straight behind a repose, a committing retire, a committing classify
            assert c["after_%s_%s" % (e, k)] >= 1, (e, k, what)
        # with require_published before any classify of the open map and after a committing one
        assert c["pub_before_" + k] >= 1 and c["pub_after_" + k] >= 1, (k, what)
        # a query answered from the table or the flags as they were would be noticed
        assert c["sens_query_stale_" + k] >= 1 and c["sens_query_flags_" + k] >= 1, (k, what)
    for r in QREFUSALS:
        assert c[r] >= 1, (r, what)
    assert 5 * c["refusals"] <= c["calls"], what
    for key in QCONTENT:
        assert c[key] >= 1, (key, what)
    for e in QFIRST:  # all five behind the first clear, import and set_pose, and on a map of more than BIG entries
        assert c["first_" + e] >= len(QKINDS), (e, what)


def check_coverage(w, seed):
    """the conditions every sequence must meet; the first rehash of the table (max_voxels) and of the observation set
    (max_pairs) are judged over the default seeds by the caller"""
    c, cc = w.mcov, w.cov
    what = "seed %d: %r %r %r" % (seed, c, {k: v for k, v in cc.items() if k.startswith("hist_")}, w.count)
    for op in OPS:
        assert w.count[op] >= 3, ("op kind %s occurs %d times" % (op, w.count[op]), what)
    for kind in REFUSALS:
        assert c[kind] >= 1, (kind, what)
    assert 5 * c["refusals"] <= c["map_calls"], what
    for h in cm.HISTORIES:
        assert cc["hist_" + h] >= 1, (h, what)
    for key in ("observe_after_set_pose", "repose_moved", "repose_merged", "repose_dropped", "retire_winner_both",
                "retire_unobserved_both", "retire_orphaned", "grown_after_repose", "grown_after_retire", "recarve_chain",
                "carry_repose_published", "carry_retire_published", "recarve_unposed", "recarve_short", "pairs_created"):
        assert c[key] >= 1, (key, what)
    assert cc["created"] > 0, what
    assert cc["sensitive_calls"] + c["sens_listed"] >= 1, ("sens_listed", what)
    for key in SENS[:-1]:
        assert c[key] >= 1, (key, what)
