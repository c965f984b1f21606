"""The point-cloud calls on a host-side model: what sdm_extract_points and everything built on it must return when the
engine's planes are the ones the reference's writers would hold (test_gpu_statefuzz.Model, oracle arithmetic), plus the
generator of the random call sequences that tests/test_gpu_cloudfuzz.py runs against an engine and
tests/test_cloudfuzz_cpu.py runs against this model alone.  Nothing here touches an engine.

  plain cloud    test_gpu_extract.host_filter over the model's planes; xyz as the last point-set call left it
  support words  support_np.inter_support over the model's depth maps and current poses, at the kept pixels
  downstream     voxel_np, voxcam_np, carve_np, vmap_np, vmap_carve_np and test_gpu_vmap_carve.Mirror's two counters
  refusals       SDM_ESTATE for a slot or neighbour without a depth map, source 1 without a checked plane, a map call
                 without an open map, vmap_open with one (each steered into every sequence and asserted); a refused
                 call leaves everything as it was

World.apply(op, args) applies one call to the model and returns what the engine must answer; it also keeps the
coverage counters that check_coverage asserts (the conditions are on the sequences, not on an engine)."""
import numpy as np

import carve_np
import support_np
import vmap_carve_np as vc
import vmap_np
import voxcam_np
import voxel_np
from test_gpu_extract import ALL, ESTATE, host_filter
from test_gpu_statefuzz import Model
from test_gpu_vmap_carve import Mirror

W, H, N_KF, N_NBR = 96, 72, 8, 5
STEPS = 115
SEED0 = 0x5EED0F00
LAMBDAS = (8.0, 12.0, 5.0)
# the scene is a slab of about 1.1 x 0.85 x 0.1 one unit in front of the cameras, uploaded maps spread over depths 0.67 .. 2:
# 0.02 puts an uploaded map's ~2000 points into more than 512 voxels (the table leaves its first 1024 slots), 0.05 and
# 0.1 make keyframes share voxels (updated > 0); the walks are 20 .. 150 steps long
VOXELS = (0.02, 0.05, 0.1)
PIPE_OPS = ("recon", "search_fuse", "intra_check", "intra_grow", "inter", "inter_commit", "fused", "pointset0", "pointset1",
            "upload_depth", "assume", "set_pose", "lambda", "reupload", "recon+batch")
CLOUD_OPS = ("extract", "extract_support", "voxel", "voxel_cameras", "voxel_freespace", "vmap_open", "vmap_integrate",
             "vmap_carve", "vmap_clear", "vmap_close")
_WEIGHT = {"recon": 5, "fused": 3, "inter": 3, "inter_commit": 2.5, "search_fuse": 1.5, "intra_check": 1.5, "intra_grow": 1.5,
           "pointset0": 1.5, "pointset1": 2, "upload_depth": 2.5, "assume": 2.5, "set_pose": 2, "lambda": 3.5, "reupload": 3,
           "recon+batch": 2,
           "extract": 6, "extract_support": 4, "voxel": 2.5, "voxel_cameras": 2.5, "voxel_freespace": 2.5, "vmap_open": 2,
           "vmap_integrate": 8, "vmap_carve": 5, "vmap_clear": 0.7, "vmap_close": 0.7}
HISTORIES = ("lam_stale", "lam_rebuilt", "upload_depth", "assume", "inter_commit", "reupload")
VOXEL_OUT = ("multiplicity", "source_index", "representative")


def seeds():
    """the seeds of both tests; SDM_FUZZ_FIRST / SDM_FUZZ_SEEDS as in test_gpu_statefuzz.py, for deeper one-off runs"""
    import os
    first = int(os.environ.get("SDM_FUZZ_FIRST", "1"))
    return list(range(first, first + int(os.environ.get("SDM_FUZZ_SEEDS", "8"))))


# ---- the clouds -------------------------------------------------------------------------------------------------------
def plain(m, slots, source, max_sigma, min_rho, listed_only=None):
    """-> offsets int64[n + 1], pixel uint32[T], rho_sigma float32[T, 2], xyz float32[T, 3], intensity uint8[T].
    listed_only = lambdaG: the deliberately WRONG variant that keeps only pixels on the list of that lambdaG (what an engine
    that always walks its lists would return); never an expectation, only the sensitivity count."""
    offs, pix, rs, xyz, inten = [0], [], [], [], []
    for k in slots:
        rho = m.chk[k] if source else m.rho[k]
        sig = m.sig[k]
        if listed_only is not None:
            on = np.zeros(rho.shape, bool)
            on[2:-2, 2:-2] = m.der[k][0][2:-2, 2:-2] >= listed_only
            rho = np.where(on, rho, np.float32(np.nan))  # (a NaN rho fails for every min_rho)
        code, flat = host_filter(rho, sig, max_sigma, min_rho)
        pix.append(code.astype(np.uint32))
        rs.append(np.stack([rho.reshape(-1)[flat], sig.reshape(-1)[flat]], 1).astype(np.float32))
        xyz.append(np.ascontiguousarray(m.xyz[k], np.float32).reshape(-1, 3)[flat])
        inten.append(np.ascontiguousarray(m.im[k], np.uint8).reshape(-1)[flat])
        offs.append(offs[-1] + len(code))
    cat = lambda v, shape, dt: np.concatenate(v).astype(dt) if v else np.zeros(shape, dt)
    return (np.asarray(offs, np.int64), cat(pix, (0,), np.uint32), cat(rs, (0, 2), np.float32), cat(xyz, (0, 3), np.float32),
            cat(inten, (0,), np.uint8))


def cloud(m, slots, source, max_sigma, min_rho, **kw):
    o, p, rs, x, i = plain(m, slots, source, max_sigma, min_rho, **kw)
    return {"offsets": o, "pixel": p, "rho_sigma": rs, "xyz": x, "intensity": i}


def support_words(m, slots, nbrs, pl):
    """uint64[T]: bit j of a point of slots[i] is set iff neighbour nbrs[i][j] is counted at the slot's depth-map rho"""
    out = np.zeros(len(pl["pixel"]), np.uint64)
    for i, k in enumerate(slots):
        a, b = pl["offsets"][i], pl["offsets"][i + 1]
        if a == b:
            continue
        row = [int(j) for j in nbrs[i]]
        kfs = {j: support_np.keyframe(m.K, m.Tcw[j], m.H, m.W) for j in set(row) | {k}}
        words = support_np.inter_support(kfs[k], m.rho[k], [kfs[j] for j in row], [m.rho[j] for j in row],
                                         [m.sig[j] for j in row])[1]
        code = pl["pixel"][a:b].astype(np.int64)
        out[a:b] = words[code >> 16, code & 0xffff]
    return out


def centres(m):
    return {k: carve_np.camera_centre(m.Tcw[k]) for k in range(m.n_kf)}


def merged(pl, voxel):
    """extract_points_voxel(representative=True) of a plain cloud"""
    kept, mult, rep, offs = voxel_np.voxel_merge(pl["xyz"], pl["rho_sigma"][:, 1], voxel, pl["offsets"])
    exp = {f: pl[f][kept] for f in ALL}
    exp.update(offsets=offs, multiplicity=mult.astype(np.uint32), source_index=kept.astype(np.uint32),
               representative=rep.astype(np.uint32), plain_total=len(pl["pixel"]))
    return exp


class MapMirror(Mirror):
    """test_gpu_vmap_carve.Mirror fed the model's clouds instead of an engine's"""

    def integrate_cloud(self, pl, slots, tags):
        d = self.vm.integrate(pl, vmap_np.point_tags(pl["offsets"], slots, tags))
        for f in self.ev:  # entries created later start at 0
            self.ev[f] = np.concatenate([self.ev[f], np.zeros(self.vm.M - len(self.ev[f]), np.uint64)])
        return d

    def carve_cloud(self, pl, sup, slots, nbrs, cen, end_margin, max_steps, count=True):
        row = np.repeat(np.arange(len(slots)), np.diff(pl["offsets"]))
        exp = vc.carve((self.vm.keys, self.vm.ids), pl["xyz"], row, sup, slots, nbrs, cen, self.voxel, end_margin, max_steps)
        # rays with a cell outside the grid, which no max_steps would walk
        inv = np.float32(1.0) / np.float32(self.voxel)
        with np.errstate(invalid="ignore", over="ignore"):
            by_slot = np.stack([np.asarray(cen[k], np.float32) for k in range(len(cen))])
            ends = [np.floor(p * inv) for p in (pl["xyz"][exp["ray_g"]], by_slot[exp["ray_slot"]])]
            exp["rays_unwalkable"] = int((~np.all([((e >= -vc.LIM) & (e < vc.LIM)).all(axis=1) for e in ends], axis=0)).sum())
        if count:
            for f in self.ev:
                self.ev[f] = self.ev[f] + exp[f]
        return exp


# ---- the model of one engine --------------------------------------------------------------------------------------------
class World:
    def __init__(self, oracle, seq, lam=8.0):
        self.o, self.seq = oracle, seq
        self.m = Model(oracle, seq.W, seq.H, seq.n_kf, seq.K)
        self.lam = lam
        oracle.params.lambdaG = lam
        for k in range(seq.n_kf):
            self.m.upload_image(k, seq.im[k], seq.Tcw[k])
        ks = range(seq.n_kf)
        # what the engine's host-side flags should be, predicted from the calls alone (coverage only, never an expectation)
        self.list_lam = {k: lam for k in ks}     # lambdaG of the slot's pixel list
        self.recon_lam = {k: None for k in ks}   # lambdaG the depth map was reconstructed under (None: not a pipeline map)
        self.hist = {k: set() for k in ks}  # what happened to the slot since its last reconstruction
        self.map = None
        self.voxels_used = []
        self.integrated = {}                     # slot -> 0 integrated, 1 then re-posed, 2 then its point set rewritten
        self.last = (None, [])                   # the previous op and the slots it wrote
        self.count = dict.fromkeys(PIPE_OPS + CLOUD_OPS, 0)
        self.cov = dict.fromkeys(
            ("cloud_calls", "refusals", "refuse_no_depth", "refuse_no_chk", "refuse_nbr_no_depth", "refuse_open_while_open",
             "refuse_no_map",
             "points", "calls_src1_points", "calls_min_rho_neg", "slots_pipeline", "slots_other", "after_batch",
             "sensitive_calls", "created", "updated_later", "integrate_after_repose", "carve_skipped_by_max_steps", "clears",
             "reopens_other_voxel", "max_voxels", "kept_checked") + tuple("hist_" + h for h in HISTORIES), 0)

    # -- state the generator and the coverage read
    def pipeline_state(self, k):
        """the slot's depth map is a pipeline map under the current lambdaG with the list of that lambdaG"""
        return self.recon_lam[k] == self.lam and self.list_lam[k] == self.lam

    def history(self, k):
        h = set(self.hist[k]) & set(HISTORIES)
        if self.m.has_depth[k] and self.list_lam[k] != self.lam:
            h.add("lam_stale")
        if self.recon_lam[k] is not None and self.recon_lam[k] != self.lam and self.list_lam[k] == self.lam:
            h.add("lam_rebuilt")
        if self.m.has_depth[k]:
            h.discard("reupload")  # ("reupload with no depth yet")
        return h

    def zero_outside_list(self, k):
        inside = np.zeros((self.m.H, self.m.W), bool)
        inside[2:-2, 2:-2] = self.m.der[k][0][2:-2, 2:-2] >= self.lam
        return not self.m.rho[k][~inside].any() and not self.m.sig[k][~inside].any()

    def _rebuild(self, slots):
        for k in slots:
            self.list_lam[k] = self.lam

    def _reconstructed(self, k):
        self.m.has_depth[k] = True
        self.recon_lam[k] = self.lam
        self.hist[k] = set()

    def _uploaded(self, k, im, Tcw):
        self.m.upload_image(k, im, Tcw)
        self.list_lam[k] = self.lam
        self.recon_lam[k] = None
        self.hist[k] = {"reupload"}

    def batch_images(self, a):
        return [np.clip(self.seq.im[k].astype(np.int32) + a["d"], 0, 255).astype(np.uint8) for k in a["bs"]]

    def refusal(self, op, a):
        """(SDM_ESTATE, kind) when the call must be refused, else None"""
        if op == "vmap_open":
            return (ESTATE, "open_while_open") if self.map is not None else None
        if op.startswith("vmap_") and self.map is None:
            return ESTATE, "no_map"
        if op in ("vmap_clear", "vmap_close"):
            return None
        if not all(self.m.has_depth[k] for k in a["slots"]):
            return ESTATE, "no_depth"
        if a["source"] and not all(self.m.has_chk[k] for k in a["slots"]):
            return ESTATE, "no_chk"
        if a.get("nbrs") is not None and not all(self.m.has_depth[int(j)] for row in a["nbrs"] for j in row):
            return ESTATE, "nbr_no_depth"
        return None

    # -- one call
    def apply(self, op, a):
        self.count[op] += 1
        res = self._pipeline(op, a) if op in PIPE_OPS else self._cloud(op, a)
        self.last = (op, list(res.get("touched", [])) if op in PIPE_OPS else [])
        if self.map is not None:
            self.cov["max_voxels"] = max(self.cov["max_voxels"], self.map.vm.M)
        return res

    def _pipeline(self, op, a):
        m, o, seq = self.m, self.o, self.seq
        mind, maxd = seq.min_depth, seq.max_depth
        touched = list(a.get("refs", []))

        def recon(refs, nbrs, fn):
            self._rebuild([k for k in refs] + [int(j) for nb in nbrs for j in nb])
            for k, nb in zip(refs, nbrs):
                m.rho[k], m.sig[k], _ = fn(m.kf(k), [m.kf(j) for j in nb], None, mind, maxd)
                self._reconstructed(k)

        if op == "recon+batch":
            recon(a["refs"], a["nbrs"], o.semi_dense_recon)
            for k, im in zip(a["bs"], self.batch_images(a)):
                self._uploaded(k, im, seq.Tcw[k])
            recon(a["bs"], [seq.neighbours(k, N_NBR) for k in a["bs"]], o.semi_dense_recon)
            touched = sorted(set(a["refs"]) | set(a["bs"]))
        elif op == "recon":
            recon(a["refs"], a["nbrs"], o.semi_dense_recon)
        elif op == "search_fuse":
            recon(a["refs"], a["nbrs"], o.recon_search_fuse)
        elif op == "intra_check":
            self._rebuild(a["refs"])
            for k in a["refs"]:
                m.rho[k], m.sig[k] = o.intra_check(m.rho[k], m.sig[k])
        elif op == "intra_grow":
            self._rebuild(a["refs"])
            for k in a["refs"]:
                m.rho[k], m.sig[k] = o.intra_grow(m.rho[k], m.sig[k], m.der[k][0])
        elif op in ("inter", "inter_commit", "fused"):
            refs, nbrs = a["refs"], a["nbrs"]
            if not all(m.has_depth[k] for k in refs) or not all(m.has_depth[j] for nb in nbrs for j in nb):
                return {"refused": ESTATE, "touched": []}  # the reference's gate (PM.cc:292-298)
            self._rebuild(refs)
            new = {k: o.inter_check(m.kf(k), m.rho[k], [m.kf(j) for j in nb], [m.rho[j] for j in nb], [m.sig[j] for j in nb])
                   for k, nb in zip(refs, nbrs)}  # every reference against the maps as they were before the call
            for k in refs:
                m.chk[k] = new[k]
                m.has_chk[k] = True
                self.cov["kept_checked"] += int((new[k] > 1e-6).sum())
                if op == "inter_commit":
                    m.rho[k] = new[k].copy()
                    self.hist[k].add("inter_commit")
                if op == "fused":
                    m.xyz[k] = o.pointset(m.kf(k), m.chk[k])
                    self._point_set_written(k)
        elif op in ("pointset0", "pointset1"):
            self._rebuild(a["refs"])
            for k in a["refs"]:
                m.xyz[k] = o.pointset(m.kf(k), m.chk[k] if op == "pointset1" else m.rho[k])
                self._point_set_written(k)
        elif op == "upload_depth":
            k = a["k"]
            m.rho[k], m.sig[k] = a["rho"], a["sigma"]
            m.has_depth[k] = True
            self.recon_lam[k] = None
            self.hist[k].add("upload_depth")
            touched = [k]
        elif op == "assume":
            self._rebuild(a["refs"])
            for k in a["refs"]:
                assert self.zero_outside_list(k)  # legitimate only for maps that are zero outside the current list
                m.has_depth[k] = True
                self.recon_lam[k] = self.lam
                self.hist[k].add("assume")
        elif op == "set_pose":
            m.Tcw[a["k"]] = a["T"]
            if self.integrated.get(a["k"]) is not None:
                self.integrated[a["k"]] = 1
            touched = [a["k"]]
        elif op == "lambda":
            self.lam = a["lam"]
            o.params.lambdaG = a["lam"]
            touched = []
        elif op == "reupload":
            self._uploaded(a["k"], seq.im[a["k"]], seq.Tcw[a["k"]])
            touched = [a["k"]]
        return {"refused": None, "touched": touched}

    def _point_set_written(self, k):
        if self.integrated.get(k) == 1:
            self.integrated[k] = 2

    def _cloud(self, op, a):
        cov = self.cov
        cov["cloud_calls"] += 1
        ref = self.refusal(op, a)
        if ref is not None:
            cov["refusals"] += 1
            cov["refuse_" + ref[1]] += 1
            if ref[1] == "no_depth":
                cov["hist_reupload"] += sum("reupload" in self.history(k) for k in a["slots"])
            return {"refused": ref[0]}
        if op == "vmap_open":
            self.map = MapMirror(a["voxel"])
            if self.voxels_used and self.voxels_used[-1] != a["voxel"]:
                cov["reopens_other_voxel"] += 1
            self.voxels_used.append(a["voxel"])
            self.integrated = {}
            return {"refused": None}
        if op == "vmap_clear":
            self.map.clear()
            self.integrated = {}
            cov["clears"] += 1
            return {"refused": None}
        if op == "vmap_close":
            self.map = None
            self.integrated = {}
            return {"refused": None}
        slots, src, ms, mr = a["slots"], a["source"], a["max_sigma"], a["min_rho"]
        pl = cloud(self.m, slots, src, ms, mr)
        T = len(pl["pixel"])
        cov["points"] += T
        cov["calls_src1_points"] += bool(src and T)
        cov["calls_min_rho_neg"] += mr < 0
        wrong = plain(self.m, slots, src, ms, mr, listed_only=self.lam)
        cov["sensitive_calls"] += not (np.array_equal(wrong[0], pl["offsets"]) and np.array_equal(wrong[1], pl["pixel"]))
        for k in slots:
            cov["slots_pipeline" if self.pipeline_state(k) else "slots_other"] += 1
            for h in self.history(k):
                cov["hist_" + h] += 1
        if self.last[0] == "recon+batch" and set(slots) & set(self.last[1]):
            cov["after_batch"] += 1
        res = {"refused": None, "plain": pl}
        nbrs = a.get("nbrs")
        sup = support_words(self.m, slots, nbrs, pl) if nbrs is not None else None
        if op == "extract_support":
            res["support"] = sup
        elif op in ("voxel", "voxel_cameras", "voxel_freespace"):
            mg = merged(pl, a["voxel"])
            if op != "voxel":
                co, cs = voxcam_np.voxel_cameras(sup, pl["offsets"], slots, nbrs, mg["representative"], len(mg["source_index"]))
                mg.update(cam_offsets=co, cam_slots=cs, cam_total=len(cs))
            if op == "voxel_freespace":
                fs = carve_np.freespace(mg["xyz"], mg["cam_offsets"], mg["cam_slots"], centres(self.m), a["voxel"],
                                        a["end_margin"], a["max_steps"])
                mg.update({f: fs[f] for f in ("crossings", "rays_total", "rays_skipped", "cells_visited")})
                res["steps"] = fs["steps"]
            res["merged"] = mg
        elif op == "vmap_integrate":
            first = self.map.vm.calls == 0
            d = self.map.integrate_cloud(pl, slots, a["tags"])
            cov["created"] += d["created"]
            cov["updated_later"] += 0 if first else d["updated"]
            if any(self.integrated.get(k) == 2 for k in slots):
                cov["integrate_after_repose"] += 1
            for k in slots:
                self.integrated[k] = 0
            res["delta"] = d
        elif op == "vmap_carve":
            exp = self.map.carve_cloud(pl, sup, slots, nbrs, centres(self.m), a["end_margin"], a["max_steps"])
            if int((exp["steps"] < 0).sum()) > exp["rays_unwalkable"]:  # rays that only max_steps kept from being walked
                cov["carve_skipped_by_max_steps"] += 1
            res["totals"] = {f: exp[f] for f in vc.TOTALS}
            res["steps"] = exp["steps"]
        return res


# ---- the sequences ------------------------------------------------------------------------------------------------------
def describe(op, a):
    """one line per op for failure messages: arrays by shape, everything else as it is"""
    short = {k: ("<%s %s>" % (v.dtype, "x".join(map(str, v.shape))) if isinstance(v, np.ndarray) and v.size > 40 else
                 v.tolist() if isinstance(v, np.ndarray) else v) for k, v in a.items()}
    return "%s %r" % (op, short)


def _rows(rng, w, slots, width, allow_self):
    """neighbour rows: mostly the scene's own, sometimes random with repeated and self entries; an entry without a depth
    map is replaced (deliberate refusals put one back)"""
    m, seq = w.m, w.seq
    deep = [k for k in range(seq.n_kf) if m.has_depth[k]]
    rows = []
    for k in slots:
        if rng.random() < 0.8:
            row = [int(j) for j in seq.neighbours(k, N_NBR)][:width]
        elif allow_self:
            row = [int(j) for j in rng.integers(0, seq.n_kf, width)]
        else:
            row = [int(j) for j in rng.permutation([j for j in range(seq.n_kf) if j != k])[:width]]
        row = [j if m.has_depth[j] else int(rng.choice([d for d in deep if allow_self or d != k] or [j])) for j in row]
        rows.append(row)
    return rows


def _pipeline_args(rng, w, op, want=()):
    """the existing fuzz's draws; returns (op, args) -- an op that could do nothing now is replaced; want: slots an
    intra-keyframe or point-set call should include"""
    m, seq = w.m, w.seq
    n_kf = seq.n_kf
    refs = sorted(rng.choice(n_kf, int(rng.integers(1, 5)), replace=False).tolist())
    bare = [k for k in range(n_kf) if not m.has_depth[k]]
    if rng.random() < 0.8:
        nbrs = [[int(j) for j in seq.neighbours(k, N_NBR)] for k in refs]
    else:
        nbrs = [[int(j) for j in rng.permutation([j for j in range(n_kf) if j != k])[:N_NBR]] for k in refs]
    if op in ("recon", "search_fuse", "recon+batch") and bare and rng.random() < 0.7:
        refs = sorted(set(refs[:2]) | set(bare[:3]))  # keyframes without a map are reconstructed soon
        nbrs = [[int(j) for j in seq.neighbours(k, N_NBR)] for k in refs]
    if op in ("recon", "search_fuse", "inter", "inter_commit", "fused"):
        return op, {"refs": refs, "nbrs": nbrs}
    if op == "recon+batch":
        bs = sorted(rng.choice(n_kf, int(rng.integers(5, n_kf + 1)), replace=False).tolist())
        return op, {"refs": refs, "nbrs": nbrs, "bs": bs, "d": int(rng.integers(-3, 4))}
    if op in ("intra_check", "intra_grow", "pointset0"):
        refs = sorted(set(refs) | set(want))
        stage1 = [k for k, s in w.integrated.items() if s == 1]
        if op == "pointset0" and stage1:
            refs = sorted(set(refs) | {stage1[0]})
        return op, {"refs": refs}
    if op == "pointset1":
        stage1 = [k for k, s in w.integrated.items() if s == 1 and m.has_chk[k]]
        refs = sorted(set(k for k in refs if m.has_chk[k]) | set(stage1[:1])) or [k for k in range(n_kf) if m.has_chk[k]][:2]
        return ("pointset1", {"refs": refs}) if refs else _pipeline_args(rng, w, "fused")
    if op == "upload_depth":
        r = np.where(rng.random((H, W)) < 0.3, rng.uniform(0.5, 1.5, (H, W)), 0).astype(np.float32)
        s = np.where(r > 0, rng.uniform(0.01, 0.2, (H, W)), 0).astype(np.float32)
        r[:2] = r[-2:] = 0
        r[:, :2] = r[:, -2:] = 0
        return op, {"k": refs[0], "rho": r, "sigma": s}
    if op == "assume":
        ok = [k for k in range(n_kf) if w.zero_outside_list(k)]
        news = [k for k in ok if not w.pipeline_state(k) and m.has_depth[k]]  # slots whose flags the call changes, first
        pick = (news + [k for k in refs if k in ok])[:3]
        return ("assume", {"refs": sorted(set(pick))}) if pick else _pipeline_args(rng, w, "lambda")
    if op == "set_pose":
        k = refs[0]
        mine = [s for s, st in w.integrated.items() if st == 0]
        if mine and rng.random() < 0.85:
            k = int(rng.choice(mine))
        T = seq.Tcw[k].copy()
        T[:, 3] += rng.normal(0, 1e-4, 3).astype(np.float32)
        return op, {"k": k, "T": T}
    if op == "lambda":
        return op, {"lam": float(rng.choice([v for v in LAMBDAS if v != w.lam]))}
    assert op == "reupload"
    return op, {"k": refs[0]}


def _cloud_args(rng, w, op, want=(), refuse=None, wide=False, short=False, rich=False, neg=False):
    """want: slots the call should read if it can; refuse: make it a refusal if the state offers one (None: sometimes);
    wide: the sigma gate 0.3, so that the cloud holds points; short: a free-space call whose max_steps lies below its longest
    walk; rich: the depth maps' own points (source 0, min_rho 1e-6); neg: min_rho < 0"""
    m, seq = w.m, w.seq
    n_kf = seq.n_kf
    if op in ("vmap_clear", "vmap_close"):
        return op, {}
    if op == "vmap_open":
        others = [v for v in VOXELS if not w.voxels_used or v != w.voxels_used[-1]]
        return op, {"voxel": float(rng.choice(others))}
    # (the synthetic scene's sigmas lie mostly above 0.01: the wider gate is drawn more often, so that clouds hold points)
    a = {"source": int(rng.integers(0, 2)), "max_sigma": float(rng.choice([0.01, 0.3], p=[0.3, 0.7])),
         "min_rho": float(rng.choice([1e-6, -1.0, 0.5], p=[0.5, 0.25, 0.25]))}
    refuse = rng.random() < 0.05 if refuse is None else refuse
    if wide:
        a["max_sigma"], refuse = 0.3, False
    if rich:
        a["source"], a["min_rho"] = 0, 1e-6
    if neg:
        a["min_rho"] = -1.0
    bare = [k for k in range(n_kf) if not m.has_depth[k]]
    deep = [k for k in range(n_kf) if m.has_depth[k]]
    unchecked = [k for k in deep if not m.has_chk[k]]
    if a["source"] and not (all(m.has_chk[k] for k in want if k in deep) and [k for k in deep if m.has_chk[k]]):
        a["source"] = 0
    good = [k for k in deep if not a["source"] or m.has_chk[k]]
    # slots whose history is still short of its count come first
    rare = [k for k in good if any(w.cov["hist_" + h] < 4 for h in w.history(k))]
    first = [k for k in want if k in good] or ([int(rng.choice(rare))] if rare and rng.random() < 0.75 else [])
    cnt = max(int(rng.integers(1, 5)), len(first))
    rest = [int(k) for k in rng.permutation([k for k in good if k not in first])]
    slots = (first + rest)[:max(cnt, 1)]
    slots = [int(k) for k in rng.permutation(slots)]
    with_rows = op in ("extract_support", "voxel_cameras", "voxel_freespace") or (op == "vmap_carve" and rng.random() < 0.7)
    if with_rows:
        width = N_NBR if rng.random() < 0.7 else int(rng.integers(1, N_NBR + 1))
        a["nbrs"] = _rows(rng, w, slots, width, allow_self=True)
    elif op == "vmap_carve":
        a["nbrs"] = None
    if refuse:
        kinds = [k for k, ok in (("no_depth", bare), ("no_chk", unchecked), ("nbr_no_depth", bare and with_rows)) if ok]
        kinds.sort(key=lambda k: w.cov["refuse_" + k] - (2 if k == "no_depth" and w.cov["hist_reupload"] < 3 else 0)
                   - (3 if k == "nbr_no_depth" and w.cov["refuse_nbr_no_depth"] < 1 and w.cov["hist_reupload"] > 0 else 0))
        if kinds and not slots:
            kinds = [k for k in kinds if k != "nbr_no_depth"] or kinds
        if kinds:
            kind = kinds[0] if rng.random() < 0.8 else str(rng.choice(kinds))
            if kind == "no_depth":
                slots = slots[:2] + [int(rng.choice([k for k in want if k in bare] or bare))]
            elif kind == "no_chk":
                a["source"] = 1
                slots = [k for k in slots if k not in unchecked][:2] + [int(rng.choice(unchecked))]
            else:
                a["nbrs"][int(rng.integers(0, len(slots)))][int(rng.integers(0, len(a["nbrs"][0])))] = int(rng.choice(bare))
    assert slots and len(set(slots)) == len(slots)
    a["slots"] = slots
    if with_rows and len(a["nbrs"]) != len(slots):  # (a refusal changed the slots: the rows follow)
        a["nbrs"] = (a["nbrs"] + _rows(rng, w, slots[len(a["nbrs"]):], len(a["nbrs"][0]), True))[:len(slots)]
    if op in ("extract", "extract_support", "voxel", "voxel_cameras", "voxel_freespace"):
        pick = [f for f in ALL if rng.random() < 0.6]
        if op == "extract" and not pick:
            pick = [ALL[int(rng.integers(0, len(ALL)))]]
        a["fields"] = tuple(pick)
        a["dest"] = "device" if rng.random() < 0.4 else "host"
    if op in ("voxel", "voxel_cameras", "voxel_freespace"):
        a["voxel"] = float(rng.choice(VOXELS))
    if op == "vmap_integrate":
        a["tags"] = None if rng.random() < 0.5 else [int(t) for t in rng.integers(-5, 1000, len(slots))]
        a["dest"] = "device" if rng.random() < 0.3 else "host"
    if op in ("voxel_freespace", "vmap_carve"):
        a["end_margin"] = int(rng.integers(0, 3))
        a["max_steps"] = 0 if short else int(rng.choice([4096, 65536, 0]))
        if a["max_steps"] == 0:  # a value below the longest walk of this very call, from the model
            longest = 0
            if w.refusal(op, a) is None:
                longest = _longest_own_walk(w, a, w.map.voxel if op == "vmap_carve" else a["voxel"])
            a["max_steps"] = max(longest - 1 - int(rng.integers(0, 3)), 1) if longest > 1 else 4096
    return op, a


def _longest_own_walk(w, a, voxel):
    """the longest walk, in steps, from a slot's own camera to one of its plain points (cells as the free-space calls
    cut them); the calls' other rays can only add longer ones"""
    pl = cloud(w.m, a["slots"], a["source"], a["max_sigma"], a["min_rho"])
    if not len(pl["pixel"]):
        return 0
    inv = np.float32(1.0) / np.float32(voxel)
    cen = centres(w.m)
    O = np.repeat(np.stack([cen[k] for k in a["slots"]]), np.diff(pl["offsets"]), axis=0)
    with np.errstate(invalid="ignore", over="ignore"):
        fO, fP = np.floor(O * inv), np.floor(pl["xyz"] * inv)
        ok = ((fO >= -carve_np.LIM) & (fO < carve_np.LIM) & (fP >= -carve_np.LIM) & (fP < carve_np.LIM)).all(axis=1)
    return int(np.abs(fP[ok] - fO[ok]).sum(axis=1).max(initial=0))


def _deficits(c):
    """what check_coverage still misses, as numbers of calls"""
    d = {"hist_" + h: max(0, 3 - c["hist_" + h]) for h in HISTORIES}
    d.update(after_batch=max(0, 2 - c["after_batch"]), sensitive_calls=max(0, 5 - c["sensitive_calls"]),
             slots_other=max(0, 10 - c["slots_other"] + 2) // 3, slots_pipeline=max(0, 10 - c["slots_pipeline"] + 2) // 3)
    for k in ("refuse_no_depth", "refuse_no_chk", "refuse_nbr_no_depth", "refuse_open_while_open", "refuse_no_map",
              "integrate_after_repose", "carve_skipped_by_max_steps",
              "clears", "reopens_other_voxel", "created", "updated_later"):
        d[k] = int(c[k] < 1)
    return {k: v for k, v in d.items() if v}


def _plans(rng, w, room):
    """(follow-ups, feasible now, first steps): the calls that would close a gap of the coverage, as (op, keywords of the
    draw).  A follow-up only counts directly after the call it follows."""
    m, c, last, touched = w.m, w.cov, w.last[0], w.last[1]
    d = _deficits(c)
    ks = range(w.seq.n_kf)
    deep = [k for k in ks if m.has_depth[k]]
    bare = [k for k in ks if not m.has_depth[k]]
    unchecked = [k for k in deep if not m.has_chk[k]]
    rebuilt = [k for k in deep if "lam_rebuilt" in w.history(k)]
    stale = [k for k in deep if w.recon_lam[k] not in (None, w.lam) and w.list_lam[k] != w.lam]
    other = [k for k in deep if not w.pipeline_state(k)]
    stage = {s: [k for k, v in w.integrated.items() if v == s and m.has_depth[k]] for s in (0, 1, 2)}
    mp = w.map
    pick = lambda names: str(rng.choice(names))
    reads = ["extract", "extract_support", "voxel", "voxel_freespace"] + (["vmap_integrate", "vmap_carve"] if mp else [])
    rows = ["extract_support", "voxel_cameras"]
    follow, now, start = [], [], []
    refusals_open = room and ("hist_reupload" in d or "refuse_no_depth" in d or "refuse_nbr_no_depth" in d)
    if last == "recon+batch" and "after_batch" in d:  # a cloud call straight after the overlapped batch, reading its slots
        follow.append((pick(reads), dict(want=tuple(int(k) for k in rng.permutation(touched)[:2]), refuse=False)))
    if last == "reupload" and bare and refusals_open:  # a keyframe uploaded again and not yet reconstructed: a refusal
        follow.append((pick(rows if "refuse_nbr_no_depth" in d and c["hist_reupload"] else reads[:3] + rows),
                       dict(want=tuple(bare), refuse=True)))
    if last in ("upload_depth", "assume", "inter_commit") and "hist_" + last in d and all(m.has_depth[k] for k in touched):
        follow.append((pick(reads), dict(want=tuple(touched[:3]), refuse=False)))  # the flags as that call left them
    if last == "lambda" and "hist_lam_stale" in d and deep:
        follow.append((pick(reads[:3]), dict(want=tuple(deep[:2]), refuse=False)))  # the lists of the lambdaG before
    if "hist_lam_rebuilt" in d and rebuilt:
        now.append((pick(reads[:3]), dict(want=tuple(rebuilt[:3]), refuse=False)))
    elif "hist_lam_rebuilt" in d and stale and last != "lambda":
        now.append((pick(["intra_check", "pointset0"]), dict(want=tuple(stale[:3]))))  # rebuilds their lists, keeps their maps
    if "hist_lam_stale" in d and stale:
        now.append((pick(reads[:3]), dict(want=tuple(stale[:3]), refuse=False)))
    if bare and refusals_open:
        now.append((pick(rows if "refuse_nbr_no_depth" in d and c["hist_reupload"] else reads[:3] + rows),
                    dict(want=tuple(bare), refuse=True)))
    if unchecked and room and "refuse_no_chk" in d:
        now.append((pick(reads[:3]), dict(refuse=True)))
    if room and mp and "refuse_open_while_open" in d:
        now.append(("vmap_open", dict(wrong=True)))  # a second map over the open one: a refusal
    if room and mp is None and "refuse_no_map" in d:
        now.append((pick(["vmap_integrate", "vmap_carve", "vmap_clear", "vmap_close"]), dict(wrong=True, refuse=False)))
    if stage[2] and mp:
        now.append(("vmap_integrate", dict(want=(stage[2][0],), refuse=False, keen=True)))
    if stage[1]:
        now.append(("pointset0", dict(keen=True)))
    if mp and stage[0] and not stage[1] and not stage[2] and "integrate_after_repose" in d:
        now.append(("set_pose", dict(keen=True)))
    if mp and mp.vm.M > 1 and "carve_skipped_by_max_steps" in d:
        now.append(("vmap_carve", dict(short=True)))
    if mp and (mp.vm.M < 2 or ("updated_later" in d and mp.vm.calls > 0)):
        # the keyframes with the most points under the wide gate: entries are created, and replaced by a later call
        size = {k: int(plain(m, [k], 0, 0.3, 1e-6)[0][-1]) for k in deep}
        fresh = {k: n for k, n in size.items() if k not in w.integrated and n > 0} or size  # (a tie replaces nothing)
        now.append(("vmap_integrate", dict(want=tuple(sorted(fresh, key=lambda k: -fresh[k])[:2]), rich=True)))
    if ("slots_other" in d or "sensitive_calls" in d) and other:
        now.append((pick(reads[:3]), dict(want=tuple(other[:3]), refuse=False, neg="sensitive_calls" in d)))
    if "slots_pipeline" in d and len(other) < len(deep):
        now.append((pick(reads[:3]), dict(want=tuple(k for k in deep if k not in other)[:3], refuse=False)))
    for h in ("upload_depth", "inter_commit", "assume"):
        if "hist_" + h in d:
            start.append((h, {}))
    if ("hist_lam_stale" in d or "hist_lam_rebuilt" in d) and not stale and not rebuilt:
        start.append(("lambda", {}))
    if not bare and room and ("hist_reupload" in d or "refuse_no_depth" in d or "refuse_nbr_no_depth" in d):
        start.append(("reupload", {}))
    if not unchecked and room and "refuse_no_chk" in d:
        start.append(("recon+batch", {}))  # fresh keyframes with a depth map and no checked plane
    if "after_batch" in d:
        start.append(("recon+batch", {}))
    if mp is None and any(k in d for k in ("integrate_after_repose", "carve_skipped_by_max_steps", "clears", "reopens_other_voxel",
                                           "created", "updated_later")):
        start.append(("vmap_open", {}))
    if mp and not w.integrated and "integrate_after_repose" in d:
        start.append(("vmap_integrate", dict(refuse=False)))
    if mp and mp.vm.calls >= 3 and "clears" in d:
        start.append(("vmap_clear", dict(forced=True)))
    if mp and mp.vm.calls >= 3 and "reopens_other_voxel" in d and len(d) <= 2:
        start.append(("vmap_close", dict(forced=True)))
    return follow, now, start, d


def generate(seed, w, steps=STEPS):
    """yields (op, args); the caller applies each to the World (and to an engine) before asking for the next, so every
    draw is a function of the seed and the model's state alone.  Mostly weighted random draws; the gaps that the coverage
    conditions still have are closed with rising urgency as the steps run out."""
    rng = np.random.default_rng(9000 + seed)
    ops = PIPE_OPS + CLOUD_OPS
    for step in range(steps):
        m, c = w.m, w.cov
        kw, op = {}, None
        bare = [k for k in range(w.seq.n_kf) if not m.has_depth[k]]
        need = {o: 3 - w.count[o] for o in ops if w.count[o] < 3}
        room = 4 * (c["refusals"] + 2) <= c["cloud_calls"]  # refusals stay below a quarter of the cloud calls
        follow, now, start, d = _plans(rng, w, room)
        left = steps - step
        urgent = left <= 1.5 * sum(d.values()) + 0.5 * sum(need.values()) + 6
        if sum(m.has_depth.values()) < 5:
            op = "recon"
        elif follow and (urgent or rng.random() < 0.9):
            op, kw = follow[0]
        elif need and left <= sum(need.values()) + 3:  # the last steps belong to the op kinds still short of three
            names = sorted(need)
            op, kw = str(rng.choice(names, p=np.array([need[o] for o in names], float) / sum(need.values()))), dict(forced=True)
        elif now and (urgent or rng.random() < 0.45):
            op, kw = now[int(rng.integers(0, len(now)))]
        elif bare and rng.random() < 0.4:
            op = "recon"
        elif start and (urgent or rng.random() < 0.2):
            op, kw = start[int(rng.integers(0, len(start)))]
        elif need and left <= 2 * sum(need.values()) + 6 and rng.random() < 0.9:
            names = sorted(need)
            op, kw = str(rng.choice(names, p=np.array([need[o] for o in names], float) / sum(need.values()))), dict(forced=True)
        if op is None:
            p = np.array([_WEIGHT[o] for o in ops], float)
            op = str(rng.choice(ops, p=p / p.sum()))
        if kw.get("keen") and c["integrate_after_repose"] >= 1 and not urgent and rng.random() < 0.8:
            op, kw = str(rng.choice(ops, p=np.array([_WEIGHT[o] for o in ops], float) / sum(_WEIGHT.values()))), {}
        # the map's life: open before use, close before opening again; an occasional call in the wrong state is a refusal
        if op.startswith("vmap_") and not kw.get("wrong") and (rng.random() >= 0.05 or not room or kw):
            if op == "vmap_open" and w.map is not None:
                op = "vmap_close" if w.count["vmap_close"] < 3 or rng.random() < 0.3 else "vmap_integrate"
            elif op != "vmap_open" and w.map is None:
                op = "vmap_open"
            elif op in ("vmap_clear", "vmap_close") and not kw.get("forced") and \
                    (w.map.vm.calls < 5 or (c["integrate_after_repose"] < 1 and any(w.integrated.values()))):
                op = "vmap_integrate"  # (a map lives long enough to be merged into more than once)
        if op in PIPE_OPS:
            yield _pipeline_args(rng, w, op, kw.get("want", ()))
        else:
            refuse = kw.get("refuse")
            yield _cloud_args(rng, w, op, want=kw.get("want", ()), refuse=refuse if room or not refuse else False,
                              wide=kw.get("short", False) or kw.get("rich", False), short=kw.get("short", False),
                              rich=kw.get("rich", False), neg=kw.get("neg", False))


def check_coverage(w, seed):
    """the conditions every sequence must meet (ISSUE: the sequences earn their keep); max_voxels is judged over the
    default seeds by the caller"""
    c, what = w.cov, "seed %d: %r %r" % (seed, w.cov, w.count)
    for op, n in w.count.items():
        assert n >= 3, ("op kind %s occurs %d times" % (op, n), what)
    for kind in ("refuse_no_depth", "refuse_no_chk", "refuse_nbr_no_depth", "refuse_open_while_open", "refuse_no_map"):
        assert c[kind] >= 1, (kind, what)
    assert 4 * c["refusals"] <= c["cloud_calls"], what
    assert c["points"] > 2000 and c["calls_src1_points"] >= 1 and c["calls_min_rho_neg"] >= 1, what
    assert c["slots_pipeline"] >= 10 and c["slots_other"] >= 10, what
    for h in HISTORIES:
        assert c["hist_" + h] >= 3, (h, what)
    assert c["after_batch"] >= 2, what
    assert c["kept_checked"] > 2000, what  # the inter-keyframe checks keep pixels alive, as in the existing fuzz
    assert c["sensitive_calls"] >= 5, what
    assert c["created"] > 0 and c["updated_later"] > 0, what
    assert c["integrate_after_repose"] >= 1 and c["carve_skipped_by_max_steps"] >= 1, what
    assert c["clears"] >= 1 and c["reopens_other_voxel"] >= 1, what
