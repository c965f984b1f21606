"""GPU: random sequences that mix the pipeline's calls with the point-cloud calls, against tests/cloud_model.py.

The other cloud tests feed their NumPy mirrors the engine's own extract_points: a point missing from the plain cloud is
missing from both sides.  Here the expectation comes from the model's planes alone (oracle arithmetic), while the calls of
test_gpu_statefuzz.py drive the host-side flags the extraction decides by: the lambdaG of a list and of a map,
"zero outside the list", list lengths left in flight by an upload, the cached table sets, the shared staging block.

After every cloud call its whole result equals the model's (floats as bits) and the slots' planes are untouched; after
every pipeline call the touched planes equal the model's; while a voxel map is open, its info, all entries and both
counters equal the mirror after every call of either kind.  A cloud call that follows an overlapped batch upload is
issued straight behind it (the model's answer and the next draw are computed before the batch is queued, the batch's own
checks come after the cloud call), unless its destinations are device tensors, which are sized from the model's answer.
What this reaches is the host side: list lengths still in flight and the table sets.  A 96x72 batch is done on the device
within microseconds of the binding's own work, so no kernel of the cloud call can be claimed to overlap it.  Each sequence
must also meet the coverage conditions tests/test_cloudfuzz_cpu.py asserts for the generator (cloud_model.check_coverage)."""
import numpy as np
import pytest

import cloud_model as cm
from common import Sequence, assert_bit_equal
from test_gpu_vmap import DELTA, same_fetch, same_info
from test_gpu_vmap_carve import same_evidence

pytestmark = pytest.mark.gpu

try:
    import torch
except ImportError:  # host destinations only
    torch = None

# dtype of every array a cloud call returns
DT = {"xyz": np.float32, "pixel": np.uint32, "rho_sigma": np.float32, "intensity": np.uint8, "support": np.uint64,
      "multiplicity": np.uint32, "source_index": np.uint32, "representative": np.uint32, "cam_offsets": np.int64,
      "cam_slots": np.int32, "crossings": np.uint32, "offsets": np.int64, "updated_ids": np.uint32}
PER = {"xyz": 3, "rho_sigma": 2}


def same_array(got, exp, f, what):
    if hasattr(got, "cpu"):
        got = got.cpu().numpy()
    got = np.ascontiguousarray(got)
    if got.dtype != DT[f]:
        assert got.dtype.itemsize == np.dtype(DT[f]).itemsize, (what, f, got.dtype)
        got = got.view(DT[f])
    exp = np.ascontiguousarray(np.asarray(exp).astype(DT[f]))
    assert got.shape == exp.shape, "%s: %s has shape %r, the model %r" % (what, f, got.shape, exp.shape)
    if got.tobytes() != exp.tobytes():
        bad = np.flatnonzero((got.reshape(-1).view(np.uint8) != exp.reshape(-1).view(np.uint8)))
        at = int(bad[0]) // got.dtype.itemsize
        raise AssertionError("%s: %s differs in %d bytes; first at element %d: %r, the model %r" %
                             (what, f, len(bad), at, got.reshape(-1)[at], exp.reshape(-1)[at]))


def device_out(sizes):
    """{field: number of elements} -> torch device tensors of the field's element size, filled with a sentinel"""
    kind = {1: torch.uint8, 4: torch.int32, 8: torch.int64}
    out = {}
    for f, n in sizes.items():
        if f in ("xyz", "rho_sigma"):
            out[f] = torch.full((n, PER[f]), -7.0, dtype=torch.float32, device="cuda")
        else:
            out[f] = torch.full((n,), 77, dtype=kind[np.dtype(DT[f]).itemsize], device="cuda")
    return out


class Run:
    """one engine and its World"""

    def __init__(self, pkg, oracle, seed, overlap):
        self.pkg, self.seed = pkg, seed
        self.seq = Sequence(pkg, oracle, cm.W, cm.H, cm.N_KF, cm.SEED0 + seed)  # consistent geometry: the checks keep pixels
        self.eng = pkg.Engine(cm.W, cm.H, cm.N_KF, max_neighbours=cm.N_NBR, with_pointset=True)
        self.eng.set_ingest_overlap(overlap)  # batch uploads of >= 5 keyframes run next to whatever does not use their slots
        self.w = cm.World(oracle, self.seq)
        for k in range(cm.N_KF):
            self.eng.upload_image(k, self.seq.im[k], self.seq.K, self.seq.Tcw[k])
        self.log = []
        self.pending = None  # plane checks of an overlapped batch, held back while a cloud call follows it
        self.early = None    # ... and that cloud call's outcome, when it has run straight behind the batch

    def close(self):
        self.eng.close()

    # -- checks
    def check_planes(self, slots, what):
        eng, m = self.eng, self.w.m
        for k in slots:
            gr, gs = eng.download_depth(k)
            assert_bit_equal(gr, m.rho[k], "%s kf %d rho" % (what, k))
            assert_bit_equal(gs, m.sig[k], "%s kf %d sigma" % (what, k))
            if m.has_chk[k]:
                assert_bit_equal(eng.download_checked(k), m.chk[k], "%s kf %d checked" % (what, k))
            assert_bit_equal(eng.download_pointset(k), m.xyz[k], "%s kf %d xyz" % (what, k))

    def check_map(self, what):
        mp = self.w.map
        if mp is None:
            with pytest.raises(self.pkg.SdmError) as e:
                self.eng.vmap_info()
            assert e.value.code == cm.ESTATE, what
            return
        info = same_info(self.eng, mp.vm, what)
        assert np.float32(info["voxel_size"]) == np.float32(mp.voxel), what
        same_fetch(self.eng.vmap_fetch(), mp.vm.fetch(), what)
        same_evidence(self.eng, mp, what)

    def flush(self):
        if self.pending is not None:
            what, slots = self.pending
            self.pending = None
            self.check_planes(slots, what)
            self.check_map(what)

    # -- one op on engine and model
    def run(self, ops):
        """ops: an iterator of (op, args) that is advanced only after the model has taken the op before (cm.generate)"""
        ops = iter(ops)
        held, i = None, 0
        while True:
            item = held if held is not None else next(ops, None)
            held = None
            if item is None:
                break
            op, a = item
            self.log.append("%3d %s" % (i, cm.describe(op, a)))
            what = "seed %d step %d %s" % (self.seed, i, op)
            try:
                if op == "recon+batch":
                    # model first, and the next op drawn, so that nothing but the binding lies between the batch and a
                    # cloud call that follows it; the batch's own checks come after that call
                    self.flush()
                    exp = self.w.apply(op, a)
                    held = next(ops, None)
                    self.pipeline(op, a, exp)
                    self.pending = (what, exp["touched"])
                    if held is not None and held[0] in cm.CLOUD_OPS and self.runs_blind(*held):
                        self.early = self.engine_cloud(held[0], held[1], None, self.w.refusal(*held) is not None)
                elif op in cm.PIPE_OPS:
                    self.flush()
                    exp = self.w.apply(op, a)
                    self.pipeline(op, a, exp)
                    self.check_planes(exp["touched"], what)
                    self.check_map(what)
                else:
                    raw, self.early = self.early, None
                    if raw is None and self.runs_blind(op, a):  # the engine first: the model's arithmetic is not in between
                        raw = self.engine_cloud(op, a, None, self.w.refusal(op, a) is not None)
                    exp = self.w.apply(op, a)
                    if raw is None:
                        raw = self.engine_cloud(op, a, exp, bool(exp["refused"]))
                    self.compare_cloud(op, a, exp, raw, what)
                    self.flush()
                    read = set(a.get("slots", ())) | set(int(j) for row in (a.get("nbrs") or ()) for j in row)
                    self.check_planes(sorted(read), what + " (planes after the cloud call)")
                    self.check_map(what)
            except (Exception, pytest.fail.Exception) as e:  # (pytest.raises' "DID NOT RAISE" is no Exception)
                raise AssertionError("%s failed: %s\nthe last ops:\n%s" % (what, e, "\n".join(self.log[-10:]))) from e
            i += 1
        self.flush()
        if self.w.map is not None:
            self.eng.vmap_close()
            self.w.map = None

    def runs_blind(self, op, a):
        """the engine call needs nothing from the model: a refusal, or destinations that the binding sizes itself"""
        return self.w.refusal(op, a) is not None or a.get("dest") != "device" or torch is None

    def pipeline(self, op, a, exp):
        eng, seq = self.eng, self.seq
        mind, maxd = seq.min_depth, seq.max_depth
        if op == "recon+batch":
            # a reconstruction is queued and, without waiting for it, a batch of 5 .. 8 keyframes is uploaded into slots
            # that may be the ones it reads or writes; the new keyframes are reconstructed at once
            eng.recon(a["refs"], a["nbrs"], mind, maxd)
            eng.upload_images_batch(a["bs"], self.w.batch_images(a), seq.K, [seq.Tcw[k] for k in a["bs"]])
            eng.recon(a["bs"], [seq.neighbours(k, cm.N_NBR) for k in a["bs"]], mind, maxd)
        elif op == "recon":
            eng.recon(a["refs"], a["nbrs"], mind, maxd)
        elif op == "search_fuse":
            eng.search_fuse(a["refs"], a["nbrs"], mind, maxd)
        elif op == "intra_check":
            eng.intra_check(a["refs"])
        elif op == "intra_grow":
            eng.intra_grow(a["refs"])
        elif op in ("inter", "inter_commit", "fused"):
            call = (lambda: eng.inter_check_pointset(a["refs"], a["nbrs"])) if op == "fused" else \
                (lambda: eng.inter_check(a["refs"], a["nbrs"], commit=op == "inter_commit"))
            if exp["refused"]:
                with pytest.raises(self.pkg.SdmError) as e:
                    call()
                assert e.value.code == exp["refused"]
            else:
                call()
        elif op in ("pointset0", "pointset1"):
            eng.pointset(a["refs"], source=int(op == "pointset1"))
        elif op == "upload_depth":
            eng.upload_depth(a["k"], a["rho"], a["sigma"])
        elif op == "assume":
            eng.assume_pipeline_maps(a["refs"])
        elif op == "set_pose":
            eng.set_pose(a["k"], a["T"])
        elif op == "lambda":
            eng.set_params(lambdaG=a["lam"])
        elif op == "reupload":
            eng.upload_image(a["k"], seq.im[a["k"]], seq.K, seq.Tcw[a["k"]])
        else:
            raise ValueError(op)

    def engine_cloud(self, op, a, exp, refused):
        """the engine's call: ("err", code), or ("ok", result, device destinations).  exp: the model's answer when the
        destinations are device tensors, which are sized from it; else None"""
        eng = self.eng
        outs = {}
        if op == "vmap_open":
            call = lambda: eng.vmap_open(a["voxel"])
        elif op == "vmap_clear":
            call = eng.vmap_clear
        elif op == "vmap_close":
            call = eng.vmap_close
        else:
            slots = a["slots"]
            kw = dict(source=a["source"], max_sigma=a["max_sigma"], min_rho=a["min_rho"])
            nbrs = None if a.get("nbrs") is None else np.ascontiguousarray(a["nbrs"], np.int32)
            if exp is not None and not refused and a.get("dest") == "device" and torch is not None:
                outs = device_out({f: n + pad for f, (n, pad) in self.lengths(op, a, exp).items()})
            out = outs or None
            if op == "extract":
                call = lambda: eng.extract_points(slots, fields=a["fields"], out=out, **kw)
            elif op == "extract_support":
                call = lambda: eng.extract_points_support(slots, nbrs, fields=a["fields"], out=out, **kw)
            elif op == "voxel":
                call = lambda: eng.extract_points_voxel(slots, a["voxel"], fields=a["fields"], out=out, representative=True, **kw)
            elif op == "voxel_cameras":
                call = lambda: eng.extract_points_voxel_cameras(slots, nbrs, a["voxel"], fields=a["fields"], out=out,
                                                                representative=True, **kw)
            elif op == "voxel_freespace":
                call = lambda: eng.extract_points_voxel_freespace(slots, nbrs, a["voxel"], a["end_margin"], a["max_steps"],
                                                                  fields=a["fields"], out=out, representative=True, **kw)
            elif op == "vmap_integrate":
                call = lambda: eng.vmap_integrate(slots, a["tags"], updated=outs.get("updated_ids", True), **kw)
            else:
                assert op == "vmap_carve"
                call = lambda: eng.vmap_carve(slots, nbrs, a["end_margin"], a["max_steps"], **kw)
        if refused:
            with pytest.raises(self.pkg.SdmError) as e:
                call()
            return "err", e.value.code
        return "ok", call(), outs

    @staticmethod
    def lengths(op, a, exp):
        """{destination: (elements the call fills, spare elements behind them)}"""
        T = len(exp["plain"]["pixel"])
        if op in ("extract", "extract_support"):
            return {f: (T, 3) for f in a["fields"] + (("support",) if op == "extract_support" else ())}
        if op == "vmap_integrate":  # needs min(entries before the call, T): the mirror's entries after it bound them
            return {"updated_ids": (exp["delta"]["updated"], min(exp["delta"]["first_created"], T) + 2)}
        mg = exp["merged"]
        M = len(mg["source_index"])
        n = {f: (M, 5) for f in a["fields"] + ("multiplicity", "source_index")}
        n["representative"] = (T, 3)
        if op != "voxel":
            n.update(cam_offsets=(M + 1, 5), cam_slots=(int(mg["cam_total"]), 7))
        if op == "voxel_freespace":
            n["crossings"] = (M, 5)
        return n

    def compare_cloud(self, op, a, exp, raw, what):
        if exp["refused"]:
            assert raw == ("err", exp["refused"]), (what, raw)
            return
        assert raw[0] == "ok", (what, raw)
        got, outs = raw[1], raw[2]
        for f, t in outs.items():  # what lies behind the results in a device destination stays as it was
            n = self.lengths(op, a, exp)[f][0]
            rest = t[n:].cpu().numpy()
            assert (rest == (-7.0 if f in PER else 77)).all(), "%s: %s written behind its %d elements" % (what, f, n)
        if op in ("vmap_open", "vmap_clear", "vmap_close"):
            return
        pl = exp["plain"]
        if op in ("extract", "extract_support"):
            fields = a["fields"] + (("support",) if op == "extract_support" else ())
            assert set(got) == set(fields) | {"offsets"}, (what, sorted(got))
            same_array(got["offsets"], pl["offsets"], "offsets", what)
            for f in fields:
                same_array(got[f], exp["support"] if f == "support" else pl[f], f, what)
        elif op in ("voxel", "voxel_cameras", "voxel_freespace"):
            mg = exp["merged"]
            arrays = a["fields"] + cm.VOXEL_OUT + (() if op == "voxel" else ("cam_offsets", "cam_slots")) + \
                (("crossings",) if op == "voxel_freespace" else ())
            scalars = ("plain_total",) + (() if op == "voxel" else ("cam_total",)) + \
                (("rays_total", "rays_skipped", "cells_visited") if op == "voxel_freespace" else ())
            assert set(got) == set(arrays) | set(scalars) | {"offsets"}, (what, sorted(got))
            for f in scalars:
                assert int(got[f]) == int(mg[f]), "%s: %s is %d, the model %d" % (what, f, got[f], mg[f])
            same_array(got["offsets"], mg["offsets"], "offsets", what)
            for f in arrays:
                same_array(got[f], mg[f], f, what)
        elif op == "vmap_integrate":
            d = exp["delta"]
            assert {f: got[f] for f in DELTA} == {f: d[f] for f in DELTA}, (what, got, d)
            ids = got["updated_ids"]
            ids = ids.cpu().numpy().view(np.uint32) if hasattr(ids, "cpu") else ids
            assert ids.dtype == np.uint32
            np.testing.assert_array_equal(ids, d["updated_ids"], err_msg=what + " updated_ids")
        else:
            assert op == "vmap_carve"
            assert got == exp["totals"], (what, got, exp["totals"])


def run_ops(pkg, oracle, seed, overlap, ops=None):
    """a generated sequence (ops None) or a fixed one (a list of (op, args)); returns the World"""
    r = Run(pkg, oracle, seed, overlap)
    try:
        r.run(cm.generate(seed, r.w) if ops is None else ops)
        return r.w
    finally:
        oracle.params.lambdaG = 8.0
        r.close()


DEFAULT_SEEDS = range(1, 9)
_max_voxels = {}  # seed -> the largest map of its sequence, for the condition over the seed set


@pytest.mark.parametrize("seed", cm.seeds())  # env SDM_FUZZ_FIRST / SDM_FUZZ_SEEDS: deeper one-off runs
@pytest.mark.parametrize("overlap", [False, True])
def test_random_cloud_sequences(pkg, oracle, gpu_ok, seed, overlap):
    w = run_ops(pkg, oracle, seed, overlap)
    print("seed %d overlap %d: %r" % (seed, overlap, w.cov))
    _max_voxels[seed] = w.cov["max_voxels"]
    try:  # the counters tests/test_cloudfuzz_cpu.py asserts: a later edit cannot hollow the sequences
        cm.check_coverage(w, seed)
    except AssertionError as e:
        if seed in DEFAULT_SEEDS:
            raise
        # a deeper one-off run: the engine agreed with the model on every call; that this seed's sequence is short of a
        # coverage condition says nothing about the engine
        print("seed %d is short of coverage: %s" % (seed, str(e)[:300]))


def test_one_map_outgrows_its_first_table(pkg, oracle, gpu_ok):
    """over the default seeds at least one map exceeds 512 voxels, so its table leaves the first 1024 slots and the entries
    and counters compared after every call have survived a rehash (same_info asserts table_slots >= 2 * voxels)"""
    for seed in DEFAULT_SEEDS:
        if seed not in _max_voxels:  # (run alone: the sequences again)
            _max_voxels[seed] = run_ops(pkg, oracle, seed, False).cov["max_voxels"]
    assert max(_max_voxels[seed] for seed in DEFAULT_SEEDS) > 512, _max_voxels
