"""Covisible neighbours chosen on the device from resident ORB observations (sdm_covisibility, sdm_covisible_neighbours,
sdm_recon_covisible) against tests/covis_np.py, the restatement of KeyFrame::UpdateConnections and PM.cc:151-160.  Every
comparison is exact integer (or bit) equality."""
import numpy as np
import pytest

import covis_np
from common import Sequence, assert_bit_equal
from test_gpu_priors import _code, rand_angles, scene_observations, synth_kf

pytestmark = pytest.mark.gpu

CAP = 8192
SIZES = [0, 1, 2, 7, 1000, 2000, CAP]
N_SLOTS = 120
MAX_N = 20


def make_corpus(seed=0xC0715):
    """N_SLOTS keyframes' (ids, angles): list sizes from SIZES; ids >= 0 unique per keyframe and drawn from one shared pool,
    about 10 % of the keypoints without a map point; angles as tests/test_gpu_priors.py draws them (negative ones present).
    The last keyframes are made by hand: one base keyframe and 16 that share exactly 0 ... 15 map points with it."""
    rng = np.random.default_rng(seed)
    pool = 12000
    kfs = []
    n_random = N_SLOTS - 17
    for i in range(n_random):
        s = SIZES[i % len(SIZES)] if i < 4 * len(SIZES) else int(rng.choice(SIZES, p=[.05, .1, .1, .2, .3, .2, .05]))
        ids = rng.choice(pool, s, replace=False).astype(np.int32)
        neg = rng.uniform(0, 1, s) < 0.1
        ids[neg] = -rng.integers(1, 5, int(neg.sum()))
        kfs.append((ids, rand_angles(rng, s, bool(rng.integers(0, 2)))))
    base = (100000 + rng.permutation(4000)[:1000]).astype(np.int32)  # ids no random keyframe holds
    kfs.append((base, rand_angles(rng, 1000, False)))
    fresh = 200000
    for k in range(16):
        own = np.arange(fresh, fresh + 40 - k, dtype=np.int32)
        fresh += 100
        ids = rng.permutation(np.concatenate([base[rng.choice(1000, k, replace=False)], own, np.full(5, -1, np.int32)]))
        kfs.append((ids.astype(np.int32), rand_angles(rng, len(ids), False)))
    assert len(kfs) == N_SLOTS
    return kfs


def depths_of(ids):
    return np.ones(max(1, int((ids >= 0).sum())), np.float32)


@pytest.fixture(scope="module")
def corpus():
    return make_corpus()


def upload_corpus(eng, kfs):
    eng.upload_observations_batch(range(len(kfs)), [k[0] for k in kfs], [k[1] for k in kfs], [depths_of(k[0]) for k in kfs])


def corpus_lists(kfs):
    rng = np.random.default_rng(77)
    refs = [int(x) for x in rng.permutation(len(kfs))]
    cands = [int(x) for x in rng.permutation(len(kfs))]  # position != slot: a tie must follow the position
    return refs, cands


def test_random_corpus(pkg, gpu_ok, corpus):
    kfs = corpus
    ids = [k[0] for k in kfs]
    refs, cands = corpus_lists(kfs)
    eng = pkg.Engine(64, 48, N_SLOTS, max_neighbours=MAX_N)
    upload_corpus(eng, kfs)
    want_w = covis_np.weights(ids, refs, cands)
    got_w = eng.covisibility(refs, cands)
    bad = np.argwhere(got_w != want_w)
    assert bad.size == 0, (len(bad), bad[0], got_w[tuple(bad[0])], want_w[tuple(bad[0])])
    # what the corpus must hold for this to mean something
    vals = set(int(x) for x in np.unique(want_w))
    assert set(range(16)) <= vals and max(vals) >= 2000, sorted(vals)[:40]
    with_angle = [k[0][(k[0] >= 0) & (k[1] >= 0)] for k in kfs]
    assert (covis_np.weights(with_angle, refs, cands) != want_w).any(), "weights would pass on the angle-filtered lists"
    assert (want_w.max(axis=1) == 0).any(), "no empty row"
    seen_tie, seen_fallback = set(), set()
    for n in (1, 7, MAX_N):
        for mw in (1, 15, 5000):
            nbrs, w, cnt = eng.covisible_neighbours(refs, cands, n, mw)
            e_nbrs, e_w, e_cnt = covis_np.neighbours(ids, refs, cands, n, mw)
            assert np.array_equal(cnt, e_cnt), (n, mw, np.argwhere(cnt != e_cnt)[:4])
            assert np.array_equal(nbrs, e_nbrs), (n, mw, np.argwhere(nbrs != e_nbrs)[:4])
            assert np.array_equal(w, e_w), (n, mw, np.argwhere(w != e_w)[:4])
            for a in range(len(refs)):
                order = covis_np.connected(want_w[a], mw)
                if len(order) > n and want_w[a, order[n - 1]] == want_w[a, order[n]]:
                    seen_tie.add(n)
                if len(order) == 1 and want_w[a, order[0]] < mw:
                    seen_fallback.add(mw)
    assert seen_tie == {1, 7, MAX_N}, seen_tie          # rows whose equal weights straddle the cut at rank n
    assert seen_fallback == {15, 5000}, seen_fallback   # rows with no candidate at the threshold (none can at 1)
    eng.close()


def test_single_call_equals_batch(pkg, gpu_ok, corpus):
    kfs = corpus
    refs, cands = corpus_lists(kfs)
    eng = pkg.Engine(64, 48, N_SLOTS, max_neighbours=MAX_N)
    upload_corpus(eng, kfs)
    W = eng.covisibility(refs, cands)
    nbrs, w, cnt = eng.covisible_neighbours(refs, cands, 7, 15)
    for a in range(0, len(refs), 7):
        assert np.array_equal(eng.covisibility([refs[a]], cands)[0], W[a]), a
        n1, w1, c1 = eng.covisible_neighbours([refs[a]], cands, 7, 15)
        assert np.array_equal(n1[0], nbrs[a]) and np.array_equal(w1[0], w[a]) and c1[0] == cnt[a], a
    eng.close()


def test_many_candidates(pkg, gpu_ok):
    """more candidates than one pass of the selection's workgroup holds; short lists, so equal weights everywhere"""
    n_kf = 1100
    rng = np.random.default_rng(0xCA7D)
    ids = []
    for _ in range(n_kf):
        x = rng.choice(400, int(rng.integers(0, 60)), replace=False).astype(np.int32)
        x[rng.uniform(0, 1, len(x)) < 0.1] = -1
        ids.append(x)
    eng = pkg.Engine(64, 48, n_kf, max_neighbours=MAX_N)
    for s0 in range(0, n_kf, 100):
        ss = list(range(s0, s0 + 100))
        eng.upload_observations_batch(ss, [ids[s] for s in ss], [np.zeros(len(ids[s]), np.float32) for s in ss],
                                      [np.ones(1, np.float32)] * len(ss))
    cands = [int(x) for x in rng.permutation(n_kf)]
    refs = [int(x) for x in rng.permutation(n_kf)[:48]]
    want_w = covis_np.weights(ids, refs, cands)
    assert np.array_equal(eng.covisibility(refs, cands), want_w)
    late = 0
    for n, mw in ((MAX_N, 1), (MAX_N, 15), (7, 5), (1, 1)):
        got = eng.covisible_neighbours(refs, cands, n, mw)
        want = covis_np.neighbours(ids, refs, cands, n, mw)
        for g, x, what in zip(got, want, ("slots", "weights", "counts")):
            assert np.array_equal(g, x), (n, mw, what, np.argwhere(g != x)[:4])
        pos = {c: p for p, c in enumerate(cands)}
        late += sum(pos[int(s)] >= 1024 for s in want[0].reshape(-1) if s >= 0)
    assert late > 0, "no chosen neighbour lies beyond position 1024"
    eng.close()


def test_hand_made_rows(pkg, gpu_ok):
    eng = pkg.Engine(64, 48, 8, max_neighbours=4)
    one = np.ones(1, np.float32)
    ids = {0: list(range(20)), 1: [0, 1, 2], 2: [3, 4, 5], 3: [6, 7, 8, 9], 4: [10, 11, 12], 5: [], 6: [-1, 50, -2]}
    for s, x in ids.items():
        eng.upload_observations(s, x, [-1.0] * len(x), one)  # no keypoint has an angle: the weights do not look at it
    nbrs, w, cnt = eng.covisible_neighbours([0], [4, 2, 3, 1], 4, 3)
    assert list(nbrs[0]) == [3, 4, 2, 1] and list(w[0]) == [4, 3, 3, 3] and cnt[0] == 4
    nbrs, w, cnt = eng.covisible_neighbours([0], [1, 2, 4, 3], 2, 3)
    assert list(nbrs[0]) == [3, 1] and list(w[0]) == [4, 3] and cnt[0] == 2
    nbrs, w, cnt = eng.covisible_neighbours([0], [4, 2, 3, 1], 4, 15)   # none at 15: the best one alone
    assert list(nbrs[0]) == [3, -1, -1, -1] and list(w[0]) == [4, 0, 0, 0] and cnt[0] == 1
    nbrs, w, cnt = eng.covisible_neighbours([0], [4, 2, 1], 4, 15)      # ... the earliest of the best
    assert list(nbrs[0]) == [4, -1, -1, -1] and cnt[0] == 1
    nbrs, w, cnt = eng.covisible_neighbours([5, 6, 0], [5, 6], 4, 1)    # nothing shared: empty lists
    assert (nbrs == -1).all() and not w.any() and not cnt.any()
    assert eng.covisibility([0, 1], [0, 1, 3]).tolist() == [[0, 3, 4], [3, 0, 0]]  # a reference among its candidates
    eng.close()


def test_refusals(pkg, gpu_ok):
    import ctypes
    K = 10
    eng = pkg.Engine(64, 48, K, max_neighbours=3)
    rng = np.random.default_rng(5)
    good = [synth_kf(rng, 300, 100) for _ in range(6)]
    eng.upload_observations_batch(range(6), [g[0] for g in good], [g[1] for g in good], [g[2] for g in good])
    refs, cands = [0, 1, 2], [1, 2, 3, 4, 5]
    ref_w = eng.covisibility(refs, cands)
    ref_n = eng.covisible_neighbours(refs, cands, 3, 15)
    assert np.array_equal(ref_w, covis_np.weights([g[0] for g in good], refs, cands)) and ref_w.max() >= 15

    def still_good():
        assert np.array_equal(eng.covisibility(refs, cands), ref_w)
        for a, b in zip(eng.covisible_neighbours(refs, cands, 3, 15), ref_n):
            assert np.array_equal(a, b)

    lib, ctx = eng.lib, eng.ctx
    ip = ctypes.POINTER(ctypes.c_int)
    u8p = ctypes.POINTER(ctypes.c_uint8)

    def raw(refs_, cands_, n=3, mw=15, n_ref=None, n_cand=None, null=()):
        """every entry point with the same arguments; each must give the same code and leave its outputs as they were"""
        r = np.asarray(refs_, np.int32)
        c = np.asarray(cands_, np.int32)
        nr = len(r) if n_ref is None else n_ref
        nc = len(c) if n_cand is None else n_cand
        rp = None if "refs" in null else r.ctypes.data_as(ip)
        cp = None if "cands" in null else c.ctypes.data_as(ip)
        m = max(len(r), 1) * max(len(c), 1, abs(n))
        outs = [np.full(m, 12345, np.int32) for _ in range(5)]
        done = np.full(max(len(r), 1), 99, np.uint8)
        codes = [
            lib.sdm_covisibility(ctx, nr, rp, nc, cp, None if "out" in null else outs[0].ctypes.data_as(ip)),
            lib.sdm_covisible_neighbours(ctx, nr, rp, nc, cp, n, mw, None if "out" in null else outs[1].ctypes.data_as(ip),
                                         outs[2].ctypes.data_as(ip), outs[3].ctypes.data_as(ip)),
            lib.sdm_recon_covisible(ctx, nr, rp, nc, cp, n, mw, outs[4].ctypes.data_as(ip),
                                    None if "out" in null else done.ctypes.data_as(u8p)),
        ]
        written = [outs[:1], outs[1:4], outs[4:] + [done.astype(np.int32) - 99 + 12345]]
        for code, arrays in zip(codes, written):
            assert code == 0 or all((o == 12345).all() for o in arrays), "a refused call wrote an output"
        return codes

    EINVAL, ESTATE = 1, 4
    assert raw(refs, cands, null=("refs",)) == [EINVAL] * 3
    assert raw(refs, cands, null=("cands",)) == [EINVAL] * 3
    assert raw(refs, cands, null=("out",)) == [EINVAL] * 3
    assert raw(refs, cands, n_ref=0) == [EINVAL] * 3
    assert raw(refs, cands, n_cand=0) == [EINVAL] * 3
    assert raw(refs, cands, n_cand=-1) == [EINVAL] * 3
    assert raw([0, K], cands) == [EINVAL] * 3                 # slot out of range
    assert raw([0, -1], cands) == [EINVAL] * 3
    assert raw(refs, [1, K]) == [EINVAL] * 3
    assert raw(refs, [1, -1]) == [EINVAL] * 3
    assert raw([0, 1, 0], cands) == [EINVAL] * 3              # a slot twice
    assert raw(refs, [1, 2, 1]) == [EINVAL] * 3
    assert raw(refs, cands, n=0)[1:] == [EINVAL] * 2          # n outside [1, max_neighbours]
    assert raw(refs, cands, n=4)[1:] == [EINVAL] * 2
    assert raw(refs, cands, n=-1)[1:] == [EINVAL] * 2
    assert raw(refs, cands, mw=0)[1:] == [EINVAL] * 2         # min_weight < 1
    assert raw(refs, cands, mw=-3)[1:] == [EINVAL] * 2
    assert raw([0, 7], cands) == [ESTATE] * 3                 # a slot without observations
    assert raw(refs, [1, 7]) == [ESTATE] * 3
    assert lib.sdm_covisibility(None, 1, None, 1, None, None) == EINVAL
    assert lib.sdm_covisible_neighbours(None, 1, None, 1, None, 1, 1, None, None, None) == EINVAL
    assert lib.sdm_recon_covisible(None, 1, None, 1, None, 1, 1, None, None) == EINVAL
    still_good()
    # a keyframe refused at upload (a map point twice) is absent for these calls too
    eng.upload_observations(6, *good[0])
    eng.covisibility([6], cands)
    assert _code(eng, eng.upload_observations, 6, [1, 2, 1], [1.0, 2.0, 3.0], [1.0]) == EINVAL
    assert raw([6], cands) == [ESTATE] * 3
    assert raw(refs, [1, 6]) == [ESTATE] * 3
    still_good()
    # NULL where the header allows it
    r = np.asarray(refs, np.int32)
    c = np.asarray(cands, np.int32)
    out = np.empty((3, 3), np.int32)
    assert lib.sdm_covisible_neighbours(ctx, 3, r.ctypes.data_as(ip), 5, c.ctypes.data_as(ip), 3, 15,
                                        out.ctypes.data_as(ip), None, None) == 0
    assert np.array_equal(out, ref_n[0])
    eng.close()


def test_image_upload_invalidates(pkg, gpu_ok):
    W, H = 64, 48
    eng = pkg.Engine(W, H, 4, max_neighbours=2)
    rng = np.random.default_rng(9)
    im = rng.integers(0, 256, (H, W), dtype=np.uint8)
    K = np.float32([50, 50, 32, 24])
    T = np.eye(3, 4, dtype=np.float32)
    kf = [synth_kf(rng, 200, 80) for _ in range(3)]
    for s in range(3):
        eng.upload_image(s, im, K, T)
        eng.upload_observations(s, *kf[s])
    w = eng.covisibility([0], [1, 2])
    assert np.array_equal(w, covis_np.weights([k[0] for k in kf], [0], [1, 2]))
    eng.upload_image(1, im, K, T)
    assert _code(eng, eng.covisibility, [0], [1, 2]) == 4
    assert _code(eng, eng.covisible_neighbours, [1], [0, 2], 2) == 4
    assert _code(eng, eng.recon_covisible, [0], [1, 2], 2, 1) == 4
    assert np.array_equal(eng.covisibility([0], [2]), w[:, 1:])  # the other slots keep theirs
    eng.upload_observations(1, *kf[1])
    assert np.array_equal(eng.covisibility([0], [1, 2]), w)
    eng.close()


@pytest.mark.parametrize("fixture", [
    ("plane_96x80_n20", 96, 80, 21, 20, 0x5EED0103, 1.5, {}),
    ("strip_roll_160x120_n7", 160, 120, 8, 7, 0x5EED0104, 3.0, {"strip": True, "roll_deg": 5.0}),
], ids=lambda f: f[0])
def test_recon_covisible_end_to_end(pkg, oracle, gpu_ok, fixture):
    name, W, H, n_kf, n, seed, disp, opts = fixture
    seq = Sequence(pkg, oracle, W, H, n_kf, seed, disparity_px=disp, **opts)
    obs = scene_observations(seq)
    refs = list(range(n_kf))
    ids = [o[0] for o in obs]
    nbrs, nbr_w, cnt = covis_np.neighbours(ids, refs, refs, n)
    assert (cnt == n).all() and nbr_w.min() >= 15, "every reference should have n neighbours in this scene"
    if name.startswith("plane"):
        assert sum(len(set(row)) < len(row) for row in nbr_w.tolist()) >= 5, "the scene should exercise the tie rule"
    # the host helpers' priors for the restatement's table, and the oracle fed them
    h_rot = np.float32([[pkg.binding.median_rot_in_plane(obs[k][0], obs[k][1], obs[j][0], obs[j][1]) for j in nbrs[k]]
                        for k in refs])
    h_b = np.float32([pkg.binding.stereo_search_constraints(obs[k][2]) for k in refs])
    o_rho, o_sig = {}, {}
    for k in refs:
        r, s, _ = oracle.recon_search_fuse(seq.okf[k], [seq.okf[j] for j in nbrs[k]], h_rot[k], h_b[k, 0], h_b[k, 1])
        r2, s2 = oracle.intra_check(r, s)
        o_rho[k], o_sig[k] = oracle.intra_grow(r2, s2, seq.grad[k])
    for mode in (0, 1, 2):
        a = pkg.Engine(W, H, n_kf, max_neighbours=n)
        b = pkg.Engine(W, H, n_kf, max_neighbours=n)
        for e in (a, b):
            e.set_scan_mode(mode)
            seq.upload(e)
            e.upload_observations_batch(refs, ids, [o[1] for o in obs], [o[2] for o in obs])
        got_nbrs, done = a.recon_covisible(refs, refs, n)
        assert done.all()
        assert np.array_equal(got_nbrs, nbrs)
        b.recon_observed(refs, nbrs)
        for k in refs:
            ra, sa = a.download_depth(k)
            rb, sb = b.download_depth(k)
            assert_bit_equal(ra, rb, "rho %s mode %d kf %d" % (name, mode, k))
            assert_bit_equal(sa, sb, "sigma %s mode %d kf %d" % (name, mode, k))
            assert_bit_equal(ra, o_rho[k], "rho vs oracle %s mode %d kf %d" % (name, mode, k))
            assert_bit_equal(sa, o_sig[k], "sigma vs oracle %s mode %d kf %d" % (name, mode, k))
            la, ha = a.active_list(k)
            lb, hb = b.active_list(k)
            assert ha == hb and np.array_equal(la, lb)
        a.inter_check(refs, got_nbrs)
        b.inter_check(refs, nbrs)
        for k in refs:
            assert_bit_equal(a.download_checked(k), b.download_checked(k), "checked %s kf %d" % (name, k))
        a.close()
        b.close()


def test_recon_covisible_skips(pkg, oracle, gpu_ok):
    """the camera leaves the point field: keyframes with fewer than n connected keyframes are skipped, their maps left as
    they were (PM.cc:160)"""
    W, H, n_kf, n = 96, 80, 40, 7
    seq = Sequence(pkg, oracle, W, H, n_kf, 0x5EED0105, disparity_px=6.0)
    obs = scene_observations(seq)
    refs = list(range(n_kf))
    ids = [o[0] for o in obs]
    nbrs, _, cnt = covis_np.neighbours(ids, refs, refs, n)
    want_done = cnt == n
    assert want_done.any() and (~want_done).any(), cnt.tolist()
    assert any((o[0] >= 0).sum() == 0 for o in obs), "some keyframe should observe nothing"
    rng = np.random.default_rng(3)
    known = {k: (rng.uniform(0.1, 2.0, (H, W)).astype(np.float32), rng.uniform(0.01, 0.1, (H, W)).astype(np.float32))
             for k in refs if not want_done[k]}
    a = pkg.Engine(W, H, n_kf, max_neighbours=n)
    b = pkg.Engine(W, H, n_kf, max_neighbours=n)
    for e in (a, b):
        seq.upload(e)
        for k, (rho, sig) in known.items():
            e.upload_depth(k, rho, sig)
        # (a keyframe that observes nothing has no point depths either; it is never reconstructed)
        e.upload_observations_batch(refs, ids, [o[1] for o in obs], [o[2] for o in obs])
    got_nbrs, done = a.recon_covisible(refs, refs, n)
    assert np.array_equal(done, want_done)
    assert np.array_equal(got_nbrs, nbrs)
    sub = [k for k in refs if want_done[k]]
    b.recon_observed(sub, nbrs[sub])
    for k in refs:
        ra, sa = a.download_depth(k)
        if want_done[k]:
            rb, sb = b.download_depth(k)
            assert_bit_equal(ra, rb, "rho kf %d" % k)
            assert_bit_equal(sa, sb, "sigma kf %d" % k)
        else:
            assert_bit_equal(ra, known[k][0], "skipped rho kf %d" % k)
            assert_bit_equal(sa, known[k][1], "skipped sigma kf %d" % k)
    # a call that skips everything succeeds and touches nothing
    skipped = [k for k in refs if not want_done[k]]
    _, d2 = a.recon_covisible(skipped, refs, n)
    assert not d2.any()
    for k in skipped:
        ra, sa = a.download_depth(k)
        assert_bit_equal(ra, known[k][0], "skipped again rho kf %d" % k)
    a.close()
    b.close()
