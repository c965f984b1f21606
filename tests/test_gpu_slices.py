"""GPU: every sliced launch past its first slice, at test sizes.

Every launch whose grid grows with data goes out in slices of at most 2^31 work-items (for_ref_slices and launch_sliced in
csrc/sdm_engine.hip; about 130 call sites, most of them in csrc/sdm_vmap_host.h).  At the sizes a test can afford every one
of them is a single dispatch with first == 0 / b0 == 0.  Here an engine is created under SDM_MAX_DISPATCH_LOG2 = 8 .. 10
(or SDM_MAX_DISPATCH_ITEMS, where the split a case needs is no power of two), so that its launches go out one workgroup,
four workgroups or three reference keyframes at a time, next to a default engine given the same calls.  Every comparison is
for bit equality and three-way: the sliced engine, the default engine, and the CPU expectation the suite already has (the
oracle, cloud_model and map_model, whose checkers are imported, not restated).

sdm_get_dispatch_counts shows that slicing happened: after every call under the knob at least one group of launches took
more than one dispatch, on the default engine none did, and both engines issued the same groups.  The one exception is
stated where it is asserted: extract_points alone has no sliced launch (its passes over the extraction tiles bypass both
helpers; DESIGN.md lists them with their bounds)."""
import contextlib
import os
import time

import numpy as np
import pytest

import cloud_model as cm
import covis_np
import map_model as mm
import test_gpu_cloudfuzz as cf
import test_gpu_mapfuzz as mf
from common import Sequence, assert_bit_equal
from test_gpu_parity import crafted_maps
from test_gpu_priors import scene_observations

pytestmark = pytest.mark.gpu

LOG2, ITEMS = "SDM_MAX_DISPATCH_LOG2", "SDM_MAX_DISPATCH_ITEMS"
BLOCK, K1_PX, TILE_W, TILE_H = 256, 64, 64, 16  # csrc: workgroup size, K1's pixels per workgroup, the stencil tile


@contextlib.contextmanager
def environment(**kv):
    """os.environ with kv set (None: unset) while engines are created: sdm_create reads its knobs once per context"""
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def default_env():
    return environment(**{LOG2: None, ITEMS: None})


# ---- the knob itself --------------------------------------------------------------------------------------------------------
def test_two_engines_hold_different_limits(pkg, gpu_ok):
    """the limit is the context's: a sliced engine, a default engine created after it, and a second sliced one created while
    the first is alive; values below 8 are clamped to 8 (one workgroup per dispatch, not an endless loop)"""
    rng = np.random.default_rng(3)
    W, H = 64, 48
    rho = rng.uniform(0.5, 1.5, (H, W)).astype(np.float32)
    im = rng.integers(0, 256, (H, W)).astype(np.uint8)
    made = []
    for knob in ({LOG2: 8}, {}, {LOG2: 3}, {ITEMS: 3 * 16 * BLOCK}):
        with default_env(), environment(**knob):
            made.append(pkg.Engine(W, H, 7))
    try:
        for eng in made:
            for k in range(7):
                eng.upload_image(k, im, np.float32([60, 60, W / 2, H / 2]), np.eye(4, dtype=np.float32)[:3])
                eng.upload_depth(k, rho, rho)
            assert eng.dispatch_counts(reset=True)[0] == 0  # uploads issue no sliced launch
            eng.pointset(list(range(7)), source=0)
        # k_pointset over 7 planes of 12 workgroups: 7 dispatches of one keyframe; one dispatch; 7; and 4 + 3 (48 // 12)
        assert [e.dispatch_counts() for e in made] == [(1, 7, 1), (1, 1, 0), (1, 7, 1), (1, 2, 1)]
        assert made[0].dispatch_counts(reset=True) == (1, 7, 1) and made[0].dispatch_counts() == (0, 0, 0)
        ref = made[1].download_pointset(6)
        for e in made:
            assert_bit_equal(e.download_pointset(6), ref, "xyz")
    finally:
        for e in made:
            e.close()


# ---- the pipeline ---------------------------------------------------------------------------------------------------------
W, H, N_KF, N = 72, 56, 7, 5  # the shape of test_gpu_fuzz.py
REFS = list(range(N_KF))


def planes(rho=None, sigma=None, chk=None, xyz=None):
    out = {}
    for name, v in (("rho", rho), ("sigma", sigma), ("chk", chk), ("xyz", xyz)):
        if v is not None:
            out.update({(name, k): v[k] for k in REFS})
    return out


class PipelineWorld:
    """the sequence, the calls and, from the oracle, what every call must leave behind; computed once"""

    def __init__(self, pkg, oracle):
        o = oracle
        self.seq = seq = Sequence(pkg, o, W, H, N_KF, 0x511CE5)
        # keyframes 2 and 5 with their baseline stretched by 40 % / shrunk by 30 %: as neighbours (first in the rows of
        # keyframes 1 and 4, in the middle elsewhere) they give consistent-looking but wrong hypotheses, which K1's fusion
        # shortcuts cannot settle (test_gpu_parity.test_search_fuse_with_outlier_hypotheses): the open list is in use
        for k, scale in ((2, 1.4), (5, 0.7)):
            seq.Tcw[k] = seq.Tcw[k].copy()
            seq.Tcw[k][:, 3] = seq.Tcw[k][:, 3] * np.float32(scale)
            seq.okf[k] = o.keyframe(seq.im[k], seq.grad[k], seq.theta[k], seq.istd[k], seq.K, seq.Tcw[k])
        self.nbrs = nbrs = [[int(j) for j in seq.neighbours(k, N)] for k in REFS]
        mind, maxd = seq.min_depth, seq.max_depth
        kfs = lambda row: [seq.okf[j] for j in row]

        def inter(rho, sig):
            return {k: o.inter_check(seq.okf[k], rho[k], kfs(nbrs[k]), [rho[j] for j in nbrs[k]], [sig[j] for j in nbrs[k]])
                    for k in REFS}

        def recon(rows, rot, lo, hi):
            r1, s1, r2, s2, r3, s3 = {}, {}, {}, {}, {}, {}
            for k in REFS:
                r1[k], s1[k], _ = o.recon_search_fuse(seq.okf[k], kfs(rows[k]), None if rot is None else rot[k], float(lo[k]),
                                                      float(hi[k]))
                r2[k], s2[k] = o.intra_check(r1[k], s1[k])
                r3[k], s3[k] = o.intra_grow(r2[k], s2[k], seq.grad[k])
            return (r1, s1), (r2, s2), (r3, s3)

        pset = lambda rho: {k: o.pointset(seq.okf[k], rho[k]) for k in REFS}
        k1, k2, k3 = recon(nbrs, None, [mind] * N_KF, [maxd] * N_KF)
        chk = inter(*k3)
        assert sum(int((chk[k] > 1e-6).sum()) for k in REFS) > 300, "the scene must keep points"
        # maps that are zero off the pixel lists but otherwise adversarial (growing is live), and arbitrary dense maps
        rng = np.random.default_rng(21)
        lst, dense = ({}, {}), ({}, {})
        for k in REFS:
            active = np.zeros((H, W), bool)
            active[2:-2, 2:-2] = seq.grad[k][2:-2, 2:-2] >= 8
            near = lambda r: (seq.gt[k] * (1 + 0.01 * rng.standard_normal((H, W))).astype(np.float32))[r > 0]
            r, s = crafted_maps(rng, H, W, density=0.7)
            r[r > 0] = near(r)
            r[~active] = 0
            s[~active] = 0
            lst[0][k], lst[1][k] = r, s
            r, s = crafted_maps(rng, H, W, density=0.9, orphan_sigma_frac=0.0)
            r[r > 0] = near(r)
            dense[0][k], dense[1][k] = r, s

        def each(fn):
            res = {k: fn(k) for k in REFS}
            return tuple({k: res[k][i] for k in REFS} for i in range(2))

        lst_k2 = each(lambda k: o.intra_check(lst[0][k], lst[1][k]))
        lst_k3 = each(lambda k: o.intra_grow(lst[0][k], lst[1][k], seq.grad[k]))
        assert sum(int((lst_k3[0][k].view(np.uint32) != lst[0][k].view(np.uint32)).sum()) for k in REFS) > 10, "growing is live"
        dense_k2 = each(lambda k: o.intra_check(dense[0][k], dense[1][k]))
        dense_k3 = each(lambda k: o.intra_grow(dense[0][k], dense[1][k], seq.grad[k]))
        dense_chk = inter(*dense)
        # the observations of the keyframes, the priors the host helpers derive from them, the covisible neighbours
        self.obs = obs = scene_observations(seq)
        b = pkg.binding
        bounds = np.float32([b.stereo_search_constraints(obs[k][2]) for k in REFS])
        rot_of = lambda rows: np.float32([[b.median_rot_in_plane(obs[k][0], obs[k][1], obs[j][0], obs[j][1]) for j in rows[k]]
                                          for k in REFS])
        observed = recon(nbrs, rot_of(nbrs), bounds[:, 0], bounds[:, 1])[2]
        cov, weights, cnt = covis_np.neighbours([ob[0] for ob in obs], REFS, REFS, N)
        assert (cnt == N).all() and weights.min() >= 15, "every reference has N covisible neighbours in this scene"
        self.cov_nbrs = cov
        covisible = recon(cov.tolist(), rot_of(cov.tolist()), bounds[:, 0], bounds[:, 1])[2]

        def upload(maps):
            def go(eng):
                for k in REFS:
                    eng.upload_depth(k, maps[0][k], maps[1][k])
            return go

        def declared(eng):
            upload(lst)(eng)
            eng.assume_pipeline_maps(REFS)

        def observations(eng):
            eng.upload_observations_batch(REFS, [ob[0] for ob in obs], [ob[1] for ob in obs], [ob[2] for ob in obs])

        def covisible_call(eng):
            got, done = eng.recon_covisible(REFS, REFS, N)
            assert done.all() and np.array_equal(got, cov)

        depth = lambda m: planes(rho=m[0], sigma=m[1])
        # (label, what comes before it uncounted, the call, the planes it must leave)
        self.steps = [
            ("search_fuse", None, lambda e: e.search_fuse(REFS, nbrs, mind, maxd), depth(k1)),
            ("search_fuse again", None, lambda e: e.search_fuse(REFS, nbrs, mind, maxd), depth(k1)),
            ("intra_check", None, lambda e: e.intra_check(REFS), depth(k2)),
            ("intra_grow", None, lambda e: e.intra_grow(REFS), depth(k3)),
            ("recon", None, lambda e: e.recon(REFS, nbrs, mind, maxd), depth(k3)),
            ("inter_check", None, lambda e: e.inter_check(REFS, nbrs, commit=False), planes(chk=chk, sigma=k3[1])),
            ("pointset1", None, lambda e: e.pointset(REFS, source=1), planes(xyz=pset(chk))),
            ("pointset0", None, lambda e: e.pointset(REFS, source=0), planes(xyz=pset(k3[0]))),
            ("inter_check_pointset", None, lambda e: e.inter_check_pointset(REFS, nbrs), planes(chk=chk, xyz=pset(chk))),
            ("lists intra_check", declared, lambda e: e.intra_check(REFS), depth(lst_k2)),
            ("lists intra_grow", declared, lambda e: e.intra_grow(REFS), depth(lst_k3)),
            ("lists inter_check", declared, lambda e: e.inter_check(REFS, nbrs), planes(chk=inter(*lst))),
            ("generic intra_check", upload(dense), lambda e: e.intra_check(REFS), depth(dense_k2)),
            ("generic intra_grow", upload(dense), lambda e: e.intra_grow(REFS), depth(dense_k3)),
            ("generic inter_check commit", upload(dense), lambda e: e.inter_check(REFS, nbrs, commit=True),
             planes(chk=dense_chk, rho=dense_chk, sigma=dense[1])),
            ("generic pointset1", None, lambda e: e.pointset(REFS, source=1), planes(xyz=pset(dense_chk))),
            ("recon after generic", None, lambda e: e.recon(REFS, nbrs, mind, maxd), depth(k3)),
            ("inter_check commit after generic", None, lambda e: e.inter_check(REFS, nbrs, commit=True),
             planes(chk=chk, rho=chk, sigma=k3[1])),
            ("recon_observed", observations, lambda e: e.recon_observed(REFS, nbrs), depth(observed)),
            ("recon_covisible", None, covisible_call, depth(covisible)),
        ]

    def engine(self, pkg, scan_mode=0, **kw):
        eng = pkg.Engine(W, H, N_KF, max_neighbours=N, **kw)
        eng.set_scan_mode(scan_mode)
        for k in REFS:
            if k % 2:
                eng.upload_image(k, self.seq.im[k], self.seq.K, self.seq.Tcw[k])
            else:
                eng.upload_keyframe(k, self.seq.im[k], self.seq.grad[k], self.seq.theta[k], self.seq.istd[k], self.seq.K,
                                    self.seq.Tcw[k])
        return eng

    def drive(self, eng, sliced):
        """every call on one engine: its planes against the oracle's, its dispatch counters; -> {label: (planes, counts)}"""
        out = {}
        for label, before, call, exp in self.steps:
            if before is not None:
                before(eng)
            eng.dispatch_counts(reset=True)
            call(eng)
            cnt = eng.dispatch_counts()
            got = {}
            for k in REFS:
                if ("rho", k) in exp or ("sigma", k) in exp:
                    got["rho", k], got["sigma", k] = eng.download_depth(k)
                if ("chk", k) in exp:
                    got["chk", k] = eng.download_checked(k)
                if ("xyz", k) in exp:
                    got["xyz", k] = eng.download_pointset(k)
            for key, want in exp.items():
                assert_bit_equal(got[key], want, "%s: %s of keyframe %d (%s engine) against the oracle" %
                                 (label, key[0], key[1], "sliced" if sliced else "default"))
            assert cnt[0] > 0, (label, cnt)
            if sliced:
                assert cnt[2] > 0, "%s under the knob: no group of launches took more than one dispatch %r" % (label, cnt)
            else:
                assert cnt[2] == 0 and cnt[1] == cnt[0], "%s on the default engine: %r" % (label, cnt)
            out[label] = (got, cnt)
        return out


@pytest.fixture(scope="module")
def world(pkg, oracle, gpu_ok):
    w = PipelineWorld(pkg, oracle)
    # the scene's precondition for the open-list cases, counted by K1's statistics variant on a default engine: pixels that
    # neither fusion shortcut settles exist, in more than one keyframe's share of the list
    with default_env():
        eng = w.engine(pkg)
    try:
        eng.enable_stats(True)
        eng.get_stats(reset=True)
        w.steps[0][2](eng)
        w.open_pixels = eng.get_stats()["open_pixels"]
    finally:
        eng.close()
    print("open pixels of the scene: %d" % w.open_pixels)
    assert w.open_pixels > 100, w.open_pixels
    return w


# what carries state over the slices of one call: K1's scan modes, the deferred open list (k_fuse_open runs once behind the
# last slice) with room and without, the grow list, and scratch chunks with slices inside them
CONFIGS = {
    "plain": ({}, {}),
    "scan1": ({}, {"scan_mode": 1}),
    "scan2": ({}, {"scan_mode": 2}),
    "open_deferred": ({"SDM_OPEN_QUOTA": 0, "SDM_OPEN_INPLACE": 65}, {}),
    "open_tiny": ({"SDM_OPEN_QUOTA": 0, "SDM_OPEN_INPLACE": 65, "SDM_OPEN_CAPACITY": 64}, {}),
    "grow4": ({"SDM_GROW_CAPACITY": 4}, {}),
    "batch3": ({}, {"batch_capacity": 3}),
}
_default_runs = {}


def default_run(pkg, world, config):
    """the default engine's run of a configuration, once per module: (results, the longest pixel list)"""
    if config not in _default_runs:
        env, kw = CONFIGS[config]
        with default_env(), environment(**env):
            eng = world.engine(pkg, **kw)
        try:
            act = max(eng.active_count(k) for k in REFS)
            _default_runs[config] = (world.drive(eng, False), act)
        finally:
            eng.close()
    return _default_runs[config]


def blocks_per_ref(site, act):
    """the workgroups per reference keyframe of the launches of a kind, as the host computes them (csrc/sdm_engine.hip)"""
    up = lambda a, b: -(-a // b)
    if site == "k1":      # launch_search_fuse: 64 pixels per workgroup, padded to the 8 XCDs
        return 8 * up(up(act, K1_PX), 8)
    if site == "lists":   # band_grid_per_ref of the list kernels (K2 / K3 / K5: one band; K4: bands of 4 chunks per XCD)
        cpx = up(up(act, BLOCK), 8)
        assert cpx <= 4, "K4's band rounding starts above 4 chunks per XCD: restate it here"
        return 8 * cpx
    if site == "planes":  # blocks_for(P): k_zero_maps, k_rho_copy, k_commit, k_pointset
        return up(W * H, BLOCK)
    assert site == "tiles"  # grid_blocks(geom, 1): the stencil kernels on arbitrary maps
    return 8 * up(up(W, TILE_W) * up(H, TILE_H), 8)


# calls whose groups of launches are all of one kind: (label, groups, stays one group per call with 3-keyframe scratch chunks)
PROBES = {
    "k1": [("search_fuse again", 1, True)],
    "lists": [("inter_check", 1, True), ("pointset1", 1, True), ("intra_check", 2, False), ("intra_grow", 1, False)],
    "planes": [("generic pointset1", 1, True)],
    "tiles": [("generic intra_check", 1, False), ("generic intra_grow", 1, False)],
}
PER_SLICE = {"lists2": 2}  # (else 3) two list references per dispatch: scratch chunks of three go out as 2, 1
CASES = [(c, "one") for c in CONFIGS] + [("plain", s) for s in PROBES] + \
    [(c, "k1") for c in ("scan1", "scan2", "open_deferred", "open_tiny")] + [("grow4", "lists"), ("batch3", "lists2")]


@pytest.mark.parametrize("config,split", CASES, ids=["%s-%s" % c for c in CASES])
def test_pipeline_calls_in_slices(pkg, world, config, split):
    """split "one": limit 2^8, one reference keyframe per dispatch.  Else the limit is three keyframes of the named kind of
    launch, so that its 7 references go out as 3, 3, 1: a full slice at first > 0 and a partial last one.  (No power of
    two does that for 8 or 16 workgroups per keyframe, hence SDM_MAX_DISPATCH_ITEMS.)  With scratch chunks of three
    keyframes a limit of three would leave every chunk whole, so that case takes two: 2, 2, 2, 1, and 2, 1 inside a chunk"""
    ref, act = default_run(pkg, world, config)
    env, kw = CONFIGS[config]
    per = PER_SLICE.get(split, 3)
    knob = {LOG2: 8} if split == "one" else {ITEMS: per * blocks_per_ref(split.rstrip("2"), act) * BLOCK}
    with default_env(), environment(**env), environment(**knob):
        eng = world.engine(pkg, **kw)
    try:
        t0 = time.perf_counter()
        got = world.drive(eng, True)
        print("%s %s: %.2f s for %d calls under %r" % (config, split, time.perf_counter() - t0, len(got), knob))
    finally:
        eng.close()
    for label, (mine, cnt) in got.items():
        theirs, dcnt = ref[label]
        assert cnt[0] == dcnt[0], "%s: %d groups of launches, the default engine %d" % (label, cnt[0], dcnt[0])
        for key in theirs:
            assert_bit_equal(mine[key], theirs[key], "%s: %s of keyframe %d, sliced against default" % (label, key[0], key[1]))
    if split == "one":
        # nothing but whole keyframes: every group of 7 references took 7 dispatches (scratch chunks of 3: 3 + 3 + 1)
        for label in ("search_fuse again", "inter_check", "pointset1", "generic pointset1"):
            assert got[label][1] == (1, N_KF, 1), (label, got[label][1])
    else:
        for label, groups, chunk_free in PROBES[split.rstrip("2")]:
            if chunk_free or "batch_capacity" not in kw:
                assert got[label][1] == (groups, -(-N_KF // per) * groups, groups), \
                    "%s: the 7 references should go out %d at a time: %r" % (label, per, got[label][1])
            elif per == 2:  # chunks of 3, 3, 1 references: 2 + 1, 2 + 1, 1
                assert got[label][1] == (3 * groups, 5 * groups, 2 * groups), (label, got[label][1])


# ---- per-call extraction and the two fuzzed life cycles ----------------------------------------------------------------------
class Counting:
    """mixin over test_gpu_cloudfuzz.Run / test_gpu_mapfuzz.MapRun: the dispatch counters around every engine call by op
    kind, and the raw results of the cloud and map calls"""
    made = []

    def __init__(self, *a, **kw):
        self.counts, self.results, self._depth = {}, [], 0
        super().__init__(*a, **kw)
        self.limit = {k: os.environ.get(k) for k in (LOG2, ITEMS)}
        Counting.made.append(self)

    def _counted(self, op, call, keep=None):
        if self._depth:  # (MapRun.engine_map hands the cloud ops on to engine_cloud)
            return call()
        self._depth += 1
        self.eng.dispatch_counts(reset=True)
        try:
            res = call()
        finally:
            self._depth -= 1
            cnt = self.eng.dispatch_counts()
            tot = self.counts.setdefault(op, [0, 0, 0, 0])
            for i in range(3):
                tot[i] += cnt[i]
            tot[3] += 1
        if keep is not None and res[0] == "ok":
            self.results.append((op, keep, cnt, res[1]))
        return res

    def pipeline(self, op, a, exp):
        return self._counted(op, lambda: super(Counting, self).pipeline(op, a, exp))

    def engine_cloud(self, op, a, exp, refused):
        return self._counted(op, lambda: super(Counting, self).engine_cloud(op, a, exp, refused), a.get("dest", ""))

    def engine_map(self, op, a, exp, refused):
        return self._counted(op, lambda: super(Counting, self).engine_map(op, a, exp, refused), a.get("dest", ""))

    def multi(self):
        return {op: c[2] for op, c in self.counts.items()}


class CloudRun(Counting, cf.Run):
    pass


class MapRun(Counting, mf.MapRun):
    pass


def host_bytes(v):
    if hasattr(v, "cpu"):
        v = v.cpu().numpy()
    return np.ascontiguousarray(v).tobytes() if isinstance(v, np.ndarray) else v


def same_results(got, ref, what):
    """the raw results of two engines' cloud calls, byte for byte"""
    assert [(r[0], r[1]) for r in got] == [(r[0], r[1]) for r in ref], what
    for (op, dest, _, mine), (_, _, _, theirs) in zip(got, ref):
        if isinstance(mine, dict):
            assert set(mine) == set(theirs), (what, op, dest)
            for f in mine:
                assert host_bytes(mine[f]) == host_bytes(theirs[f]), "%s: %s (%s) %s, sliced against default" % (what, op, dest, f)


EXTRACT_SLOTS = [0, 2, 4]
EXTRACT_OPS = ("extract", "extract_support", "voxel", "voxel_cameras", "voxel_freespace")


def extraction_ops(w):
    """96 x 72 (27 workgroups and 3.4 extraction tiles per dense slot): every keyframe reconstructed, arbitrary dense maps over
    slots 0 and 4, so that of the call's three slots two are walked whole and slot 2 from its pixel list; then every
    extraction call with host and with device destinations"""
    seq = w.seq
    ks = list(range(cm.N_KF))
    rows = lambda slots: [[int(j) for j in seq.neighbours(k, cm.N_NBR)] for k in slots]
    yield "recon", {"refs": ks, "nbrs": rows(ks)}
    rng = np.random.default_rng(96)
    for k in (0, 4):
        r = np.where(rng.random((cm.H, cm.W)) < 0.9, rng.uniform(0.5, 1.5, (cm.H, cm.W)), 0).astype(np.float32)
        s = np.where(r > 0, rng.uniform(0.01, 0.2, (cm.H, cm.W)), 0).astype(np.float32)
        yield "upload_depth", {"k": k, "rho": r, "sigma": s}
    yield "pointset0", {"refs": ks}
    assert not w.pipeline_state(0) and not w.pipeline_state(4) and w.pipeline_state(2)
    a = dict(slots=EXTRACT_SLOTS, source=0, max_sigma=0.3, min_rho=1e-6, fields=cm.ALL, nbrs=rows(EXTRACT_SLOTS), voxel=0.05,
             end_margin=1, max_steps=4096)
    for dest in ("host", "device"):
        for op in EXTRACT_OPS:
            yield op, dict(a, dest=dest)


def run_extraction(pkg, oracle):
    r = CloudRun(pkg, oracle, 1, False)
    try:
        r.run(extraction_ops(r.w))
        return r
    finally:
        oracle.params.lambdaG = 8.0
        r.close()


@pytest.fixture(scope="module")
def default_extraction(pkg, oracle, gpu_ok):
    with default_env():
        r = run_extraction(pkg, oracle)
    assert all(v == 0 for v in r.multi().values()), r.counts
    return r


@pytest.mark.parametrize("lg", [8, 10])
def test_extraction_calls_in_slices(pkg, oracle, default_extraction, lg):
    """1 and 4 workgroups per dispatch; 27 is a multiple of neither.  The offsets, the plain-to-kept map, the camera lists
    and the ray counters all cross slice boundaries; Run.run compares every result with cloud_model's"""
    with default_env(), environment(**{LOG2: lg}):
        t0 = time.perf_counter()
        r = run_extraction(pkg, oracle)
        print("extraction under 2^%d: %.2f s, %r" % (lg, time.perf_counter() - t0, r.counts))
    calls = [c for c in r.results if c[0] in EXTRACT_OPS]
    assert [(c[0], c[1]) for c in calls] == [(op, d) for d in ("host", "device") for op in EXTRACT_OPS]
    plain = [c for c in calls if c[0] == "extract"][0][3]
    assert plain["offsets"][-1] > 8 * 1024, "more than 4 tiles of points, so that the tile passes are sliced at 2^10 too"
    for op, dest, cnt, _ in calls:
        if op == "extract":
            # k_extract_count / k_extract_write run over the extraction tiles in one launch each: no sliced launch at all
            assert cnt == (0, 0, 0), (op, dest, cnt)
        else:
            assert cnt[2] > 0, "%s (%s) under 2^%d: no group of launches took more than one dispatch %r" % (op, dest, lg, cnt)
    assert r.counts["recon"][2] > 0 and r.counts["pointset0"][2] > 0
    same_results(r.results, default_extraction.results, "extraction under 2^%d" % lg)
    assert {op: c[0] for op, c in r.counts.items()} == {op: c[0] for op, c in default_extraction.counts.items()}


def fuzzed(monkeypatch, module, name, cls, knob, call):
    """a run of one of the fuzz modules with its Run class (module.name) counting, the engine created under the knob"""
    monkeypatch.setattr(module, name, cls)
    del Counting.made[:]
    with default_env(), environment(**knob):
        t0 = time.perf_counter()
        call()
        dt = time.perf_counter() - t0
    r, = Counting.made
    assert r.limit == dict({LOG2: None, ITEMS: None}, **{k: str(v) for k, v in knob.items()})
    print("%s under %r: %.2f s, multi-dispatch groups by op: %r" % (module.__name__, knob, dt, r.multi()))
    return r


MAP_CALLS = ("vmap_integrate", "vmap_observe", "vmap_carve", "vmap_classify", "vmap_import", "vmap_import_observations",
             "vmap_repose", "vmap_retire", "vmap_recarve") + tuple(mm.FETCHES) + tuple(mm.QUERY_OPS)


@pytest.mark.parametrize("lg", [10, 8])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_map_sequences_in_slices(pkg, oracle, gpu_ok, monkeypatch, seed, lg):
    """test_gpu_mapfuzz's sequence of the seed, the read-only queries of its query stream included, four workgroups per
    dispatch and one: its comparison with map_model after every call is the check (the same sequence on a default engine
    is test_random_map_sequences).  Which map calls reach a second dispatch depends on the seed's map sizes; the calls below
    do for every seed at 2^10 already, and test_online_recipe_in_slices asserts it for every kind"""
    r = fuzzed(monkeypatch, mf, "MapRun", MapRun, {LOG2: lg}, lambda: mf.run_ops(pkg, oracle, seed, False))
    mm.check_coverage(r.w, seed)
    mm.check_query_coverage(r.w, seed)
    assert all(r.counts[op][3] >= 3 for op in mm.QUERY_OPS), r.counts
    # every one of these logs outgrows the observation set's first 1024 slots, seed 2's map its first table as well
    # (tests/test_mapfuzz_cpu.py has the model's sizes): the state compared after every call has survived sliced rehashes
    assert r.w.mcov["max_pairs"] > 512 and r.rehashes["obs"] > 0, (r.w.mcov["max_pairs"], r.rehashes)
    assert (r.w.cov["max_voxels"] > 512) == (seed == 2) and (r.rehashes["map"] > 0 or seed != 2), (r.w.cov, r.rehashes)
    for op in ("recon", "recon+batch", "inter_commit", "pointset0", "vmap_integrate", "vmap_observe"):
        assert r.counts[op][2] > 0, "%s: none of its %d calls took more than one dispatch %r" % (op, r.counts[op][3], r.counts)


def recipe_and_whole_map(w):
    """map_model.online_recipe, then what its sizes leave single-workgroup or without a launch: an import of every record
    (displaced, so that entries are created and updated) and the four fetches by a list of all ids"""
    yield from mm.online_recipe(w)
    vm = w.map.vm
    rec = {f: vm.rec[f].copy() for f in ("xyz", "pixel", "rho_sigma", "intensity", "tag", "multiplicity")}
    rec["xyz"] = (rec["xyz"] + np.float32(2 * w.map.voxel)).astype(np.float32)
    yield "vmap_import", {"records": rec, "extra": True, "dest": "host"}
    ids = np.random.default_rng(8).permutation(w.map.vm.M).astype(np.uint32)
    ids[-1] = ids[0]  # ids may repeat
    for dest in ("host", "device"):
        for op in mm.FETCHES:
            yield op, {"ids": ids, "first": 0, "count": None, "dest": dest}


def test_online_recipe_in_slices(pkg, oracle, gpu_ok, monkeypatch):
    """one workgroup per dispatch: every op kind the recipe issues that launches anything at all had a group of more than
    one dispatch, both rehashes included"""
    r = fuzzed(monkeypatch, mf, "MapRun", MapRun, {LOG2: 8}, lambda: mf.run_ops(pkg, oracle, 1, False, ops=recipe_and_whole_map))
    assert r.w.mcov["recarve_chain"] == 1 and r.w.mcov["repose_merged"] == 1 and r.rehashes["map"] > 0
    print("rehashes %r" % r.rehashes)
    assert max(len(c[3]) for c in r.results if c[0] == "vmap_fetch_published") > 2 * BLOCK
    issued = {op for op, c in r.counts.items() if c[0] > 0}
    assert issued == set(MAP_CALLS) | {"recon", "pointset0"}, sorted(issued)
    assert set(r.counts) - issued == {"vmap_open", "set_pose"}, sorted(set(r.counts) - issued)
    for op in issued:
        assert r.counts[op][2] > 0, "%s: no group of more than one dispatch %r" % (op, r.counts[op])


@pytest.mark.parametrize("lg", [10, 8])
@pytest.mark.parametrize("seed", [1, 2])
def test_cloud_sequences_in_slices(pkg, oracle, gpu_ok, monkeypatch, seed, lg):
    """test_gpu_cloudfuzz's sequence of the seed, four workgroups per dispatch and one, against cloud_model after every call
    (every kind of extraction call reaches a second dispatch in test_extraction_calls_in_slices)"""
    r = fuzzed(monkeypatch, cf, "Run", CloudRun, {LOG2: lg}, lambda: cf.run_ops(pkg, oracle, seed, False))
    cm.check_coverage(r.w, seed)
    for op in ("recon", "recon+batch", "extract_support", "voxel", "vmap_carve"):
        assert r.counts[op][2] > 0, "%s: none of its %d calls took more than one dispatch %r" % (op, r.counts[op][3], r.counts)
