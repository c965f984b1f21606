"""SemiDenseRecon's search priors derived on the device from resident ORB observations (sdm_upload_observations*,
sdm_search_priors, sdm_recon_observed) against the host helpers (sdm_median_rot_in_plane,
sdm_stereo_search_constraints) and the CPU oracle."""
import ctypes

import numpy as np
import pytest

from common import Sequence, assert_bit_equal

pytestmark = pytest.mark.gpu

CAP = 8192
SIZES = [0, 1, 2, 7, 1000, 2000, CAP]


def f32_bits_equal(a, b):
    a, b = np.float32(a), np.float32(b)
    return a.view(np.uint32) == b.view(np.uint32) or (np.isnan(a) and np.isnan(b))


def rand_angles(rng, n, ties):
    a = rng.uniform(0.0, 360.0, n).astype(np.float32)
    if ties:  # few distinct values: many equal differences
        a = (np.floor(a / 45.0) * 45.0).astype(np.float32)
    r = rng.uniform(0, 1, n)
    a[r < 0.1] = -1.0
    a[(r >= 0.1) & (r < 0.15)] = -0.0
    a[(r >= 0.15) & (r < 0.18)] = -rng.uniform(0.5, 90.0, int(((r >= 0.15) & (r < 0.18)).sum()))
    return a


def rand_pair(rng, n1, n2, overlap):
    """two keyframes' (ids, angles): unique ids >= 0 per keyframe, some negative ids, `overlap` of the smaller list's
    map points shared"""
    pool = rng.permutation(1 << 20)[: n1 + n2].astype(np.int32)
    ids1 = pool[:n1].copy()
    ids2 = pool[n1:n1 + n2].copy()
    k = int(round(overlap * min(n1, n2)))
    if k:
        ids2[rng.choice(n2, k, replace=False)] = ids1[rng.choice(n1, k, replace=False)]
    for ids in (ids1, ids2):
        neg = rng.uniform(0, 1, len(ids)) < 0.1
        ids[neg] = -rng.integers(1, 5, int(neg.sum()))
    ties = bool(rng.integers(0, 2))
    return (ids1, rand_angles(rng, n1, ties)), (ids2, rand_angles(rng, n2, ties))


def rand_depths(rng, n, wide):
    if n == 0:
        return np.zeros(0, np.float32)
    if wide:  # mean - 2 sigma <= 0: min_depth negative or infinite, as the reference leaves it
        return rng.exponential(1.0, n).astype(np.float32)
    return rng.uniform(0.5, 2.0, n).astype(np.float32)


@pytest.fixture(scope="module")
def corpus():
    rng = np.random.default_rng(0x9A1)
    pairs = []
    for i in range(300):
        n1 = int(SIZES[rng.integers(0, len(SIZES))]) if i >= len(SIZES) ** 2 // 2 else SIZES[i % len(SIZES)]
        n2 = int(SIZES[rng.integers(0, len(SIZES))])
        if n1 == CAP and n2 == CAP and i % 3:  # (a few cap x cap pairs are enough: the host loop is O(n1 n2))
            n2 = 2000
        overlap = float(rng.choice([0.0, 0.01, 0.3, 0.5, 0.9, 1.0]))
        a, b = rand_pair(rng, n1, n2, overlap)
        d = rand_depths(rng, max(n1, 1), bool(rng.integers(0, 2)))
        pairs.append((a, b, d))
    return pairs


def host_rot(pkg, a, b):
    return pkg.binding.median_rot_in_plane(a[0], a[1], b[0], b[1])


def test_random_pairs_and_bounds(pkg, oracle, gpu_ok, corpus):
    n = len(corpus)
    eng = pkg.Engine(64, 48, 2 * n, max_neighbours=1)
    slots = list(range(2 * n))
    ids = [p[k][0] for p in corpus for k in (0, 1)]
    ang = [p[k][1] for p in corpus for k in (0, 1)]
    dep = [p[2] if k == 0 else np.ones(1, np.float32) for p in corpus for k in (0, 1)]
    eng.upload_observations_batch(slots, ids, ang, dep)
    refs = np.arange(0, 2 * n, 2)
    rot, mn, mx = eng.search_priors(refs, refs[:, None] + 1)
    odd = even = 0
    for i, (a, b, d) in enumerate(corpus):
        want = host_rot(pkg, a, b)
        assert rot[i, 0] == want, (i, len(a[0]), len(b[0]), rot[i, 0], want)
        assert np.float32(oracle.median_rot_in_plane(a[0], a[1], b[0], b[1])) == rot[i, 0], i
        hmn, hmx = pkg.binding.stereo_search_constraints(d)
        assert f32_bits_equal(mn[i], hmn) and f32_bits_equal(mx[i], hmx), (i, mn[i], hmn, mx[i], hmx)
        omn, omx = oracle.stereo_search_constraints(d)
        assert f32_bits_equal(mn[i], omn) and f32_bits_equal(mx[i], omx), i
        s1 = {x: ax for x, ax in zip(a[0], a[1]) if x >= 0 and ax >= 0}
        m = sum(1 for y, by in zip(b[0], b[1]) if y in s1 and by >= 0)
        odd += m % 2 == 1
        even += m > 0 and m % 2 == 0
    assert odd > 20 and even > 20, (odd, even)
    assert (mn <= 0).any() or (~np.isfinite(mn)).any(), "corpus lacks depths with mean - 2 sigma <= 0"
    # the same pairs one call each
    for i in range(0, n, 7):
        r1, a1, b1 = eng.search_priors([2 * i], [[2 * i + 1]])
        assert f32_bits_equal(r1[0, 0], rot[i, 0]) and f32_bits_equal(a1[0], mn[i]) and f32_bits_equal(b1[0], mx[i])
    eng.close()


def synth_kf(rng, n_points, n_kp):
    """a keyframe seeing a random subset of n_points global map points"""
    ids = rng.choice(n_points, n_kp, replace=False).astype(np.int32)
    ids[rng.uniform(0, 1, n_kp) < 0.4] = -1
    ang = rng.uniform(0.0, 360.0, n_kp).astype(np.float32)
    ang[rng.uniform(0, 1, n_kp) < 0.05] = -1.0
    dep = rng.uniform(0.5, 3.0, int((ids >= 0).sum())).astype(np.float32)
    return ids, ang, dep


@pytest.mark.parametrize("n_kp", [1000, 2000])
def test_batch_64x20(pkg, gpu_ok, n_kp):
    rng = np.random.default_rng(n_kp)
    n_kf, n_ref, n = 84, 64, 20
    kfs = [synth_kf(rng, 3 * n_kp, n_kp) for _ in range(n_kf)]
    eng = pkg.Engine(64, 48, n_kf, max_neighbours=n)
    eng.upload_observations_batch(range(n_kf), [k[0] for k in kfs], [k[1] for k in kfs], [k[2] for k in kfs])
    refs = np.arange(n_ref)
    nbrs = np.stack([[(r + 1 + j) % n_kf for j in range(n)] for r in refs])
    rot, mn, mx = eng.search_priors(refs, nbrs)
    for r in refs:
        hmn, hmx = pkg.binding.stereo_search_constraints(kfs[r][2])
        assert f32_bits_equal(mn[r], hmn) and f32_bits_equal(mx[r], hmx)
        for j in range(n):
            s = nbrs[r, j]
            r1, _, _ = eng.search_priors([r], [[s]])
            want = pkg.binding.median_rot_in_plane(kfs[r][0], kfs[r][1], kfs[s][0], kfs[s][1])
            assert rot[r, j] == r1[0, 0] == want, (r, j, rot[r, j], r1[0, 0], want)
    assert (rot != 0).mean() > 0.9
    eng.close()


def test_edge_cases(pkg, gpu_ok):
    eng = pkg.Engine(64, 48, 8, max_neighbours=4)
    one = np.ones(3, np.float32)
    eng.upload_observations(0, [1, 2, 3], [10.0, 20.0, 30.0], one)
    eng.upload_observations(1, [4, 5, 6], [10.0, 20.0, 30.0], one)       # no shared map point
    eng.upload_observations(2, [1, 2, 3], [-1.0, -2.0, -1.0], one)      # every shared point without an angle
    eng.upload_observations(3, [3, -1, 1], [5.0, 7.0, -0.0], one)       # -0 counts as an angle (host: -0 < 0 is false)
    eng.upload_observations(4, [], [], one)                              # no keypoints at all
    rot, _, _ = eng.search_priors([0], [[1, 2, 3, 4]])
    assert rot[0, 0] == 0 and rot[0, 1] == 0 and rot[0, 4 - 1] == 0
    want = pkg.binding.median_rot_in_plane([1, 2, 3], [10.0, 20.0, 30.0], [3, -1, 1], [5.0, 7.0, -0.0])
    assert rot[0, 2] == want == np.float32(-25.0)  # {-25, -10}: rank (2 - 1) / 2 = 0
    rot, mn, mx = eng.search_priors([4], [[0]])  # a reference without keypoints: rot 0, bounds from its depths
    assert rot[0, 0] == 0
    assert f32_bits_equal(mn[0], pkg.binding.stereo_search_constraints(one)[0])
    eng.close()


def _code(eng, fn, *a):
    try:
        fn(*a)
    except pkg_error(eng) as e:
        return e.code
    return 0


def pkg_error(eng):
    import sys
    return sys.modules[type(eng).__module__].SdmError


def test_refusals(pkg, gpu_ok):
    eng = pkg.Engine(64, 48, 8, max_neighbours=2)
    rng = np.random.default_rng(5)
    good = [synth_kf(rng, 300, 100) for _ in range(3)]
    eng.upload_observations_batch([0, 1, 2], [g[0] for g in good], [g[1] for g in good], [g[2] for g in good])
    ref_rot, ref_mn, ref_mx = eng.search_priors([0], [[1, 2]])

    def still_good():
        r, a, b = eng.search_priors([0], [[1, 2]])
        assert_bit_equal(r, ref_rot, "rot")
        assert_bit_equal(a, ref_mn, "min")
        assert_bit_equal(b, ref_mx, "max")

    def refused(slot, ids, ang, dep=np.ones(2, np.float32), code=1):
        eng.upload_observations(3, *good[0])  # present before ...
        assert _code(eng, eng.upload_observations, slot, ids, ang, dep) == code
        if 0 <= slot < 8:
            assert _code(eng, eng.search_priors, [slot], [[0]]) == 4  # ... absent after (SDM_ESTATE)
        still_good()

    refused(3, [1, 2, 1], [1.0, 2.0, 3.0])                        # duplicate id
    refused(3, [1, 2, 1], [-1.0, 2.0, 3.0])                       # duplicate id, one of them without an angle
    refused(3, [1, 2, 3], [1.0, np.nan, 3.0])                     # NaN angle
    refused(3, [1, 2, 3], [1.0, np.inf, 3.0])                     # infinite angle
    refused(3, [-1, 2, 3], [-np.inf, 2.0, 3.0])                   # ... even where no map point is
    refused(3, np.arange(CAP + 1), np.ones(CAP + 1, np.float32))  # over the cap
    refused(3, [1], [1.0], np.ones(CAP + 1, np.float32))          # depths over the cap
    assert _code(eng, eng.upload_observations, 8, [1], [1.0], [1.0]) == 1   # slot out of range
    assert _code(eng, eng.upload_observations, -1, [1], [1.0], [1.0]) == 1
    still_good()
    # the cap itself is accepted
    eng.upload_observations(3, np.arange(CAP), np.ones(CAP, np.float32), np.ones(CAP, np.float32))
    eng.search_priors([3], [[0]])
    # a batch with one bad keyframe stores the others
    b = [synth_kf(rng, 300, 100) for _ in range(3)]
    bad_ids = b[1][0].copy()
    bad_ids[:2] = 7
    assert _code(eng, eng.upload_observations_batch, [4, 5, 6], [b[0][0], bad_ids, b[2][0]], [x[1] for x in b],
                 [x[2] for x in b]) == 1
    r, _, _ = eng.search_priors([4], [[6]])
    assert r[0, 0] == pkg.binding.median_rot_in_plane(b[0][0], b[0][1], b[2][0], b[2][1])
    assert _code(eng, eng.search_priors, [4], [[5]]) == 4
    # no observations; no depths; bad sizes
    assert _code(eng, eng.search_priors, [7], [[0]]) == 4
    assert _code(eng, eng.search_priors, [0], [[7]]) == 4
    eng.upload_observations(7, [1, 2], [1.0, 2.0], [])
    assert _code(eng, eng.search_priors, [7], [[0]]) == 1              # zero depths: the host helper's n <= 0
    rot = np.empty((1, 1), np.float32)
    lib = eng.lib
    rs, ns = (ctypes.c_int * 1)(7), (ctypes.c_int * 1)(0)
    assert lib.sdm_search_priors(eng.ctx, 1, rs, 1, ns, rot.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), None, None) == 0
    assert _code(eng, eng.search_priors, [0], [[1, 2, 0]]) == 1         # n > max_neighbours
    assert _code(eng, eng.search_priors, [8], [[0]]) == 1               # slot out of range
    still_good()
    eng.close()


def test_image_upload_invalidates(pkg, gpu_ok):
    import torch
    W, H = 64, 48
    eng = pkg.Engine(W, H, 8, max_neighbours=1)
    rng = np.random.default_rng(9)
    im = rng.integers(0, 256, (H, W), dtype=np.uint8)
    K = np.float32([50, 50, 32, 24])
    T = np.eye(3, 4, dtype=np.float32)
    g = np.zeros((H, W), np.float32)
    kf = synth_kf(rng, 200, 80)
    dev = torch.from_numpy(im).cuda()
    uploads = [
        lambda s: eng.upload_image(s, im, K, T),
        lambda s: eng.upload_images_batch([s], [im], K, [T]),
        lambda s: eng.upload_image_rgb(s, np.stack([im] * 3, -1), "rgb", K, None, T),
        lambda s: eng.upload_images_rgb_batch([s], [np.stack([im] * 3, -1)], "bgr", K, None, [T]),
        lambda s: eng.upload_image_device(s, dev.data_ptr(), K, T),
        lambda s: eng.upload_keyframe(s, im, g, g, 1.0, K, T),
    ]
    for s in range(8):
        eng.upload_image(s, im, K, T)
    eng.upload_observations(0, *kf)
    for i, up in enumerate(uploads):
        s = 1 + i
        eng.upload_observations(s, *kf)  # image first, then observations: present
        eng.search_priors([s], [[0]])
        up(s)
        torch.cuda.synchronize()
        assert _code(eng, eng.search_priors, [s], [[0]]) == 4, i
        assert _code(eng, eng.search_priors, [0], [[s]]) == 4, i
        eng.search_priors([0], [[0]])  # the other slots keep theirs
    eng.close()


def scene_observations(seq, n_points=1500, seed=11):
    return [seq.scene.observations(k, n_points, seed) for k in range(seq.n_kf)]


@pytest.mark.parametrize("fixture", [
    ("plane_96x80_n20", 96, 80, 21, 20, 0x5EED0103, 1.5, {}),
    ("strip_roll_160x120_n7", 160, 120, 8, 7, 0x5EED0104, 3.0, {"strip": True, "roll_deg": 5.0}),
], ids=lambda f: f[0])
def test_recon_observed_end_to_end(pkg, oracle, gpu_ok, fixture):
    name, W, H, n_kf, n, seed, disp, opts = fixture
    seq = Sequence(pkg, oracle, W, H, n_kf, seed, disparity_px=disp, **opts)
    obs = scene_observations(seq)
    refs = list(range(n_kf))
    nbrs = np.array([seq.neighbours(k, n) for k in refs], np.int32)
    # the host helpers' priors
    h_rot = np.float32([[pkg.binding.median_rot_in_plane(obs[k][0], obs[k][1], obs[j][0], obs[j][1]) for j in nbrs[k]]
                        for k in refs])
    h_b = np.float32([pkg.binding.stereo_search_constraints(obs[k][2]) for k in refs])
    if opts.get("roll_deg"):
        assert (h_rot != 0).all()
        want = np.float32([[seq.scene.rot_deg(k, j) for j in seq.neighbours(k, n)] for k in refs])
        assert np.abs(h_rot - want).max() < 0.05, "synth observations should measure the scene's rotation"
    # the oracle fed the same priors
    o_rho, o_sig = {}, {}
    for k in refs:
        r, s, _ = oracle.recon_search_fuse(seq.okf[k], [seq.okf[j] for j in nbrs[k]], h_rot[k], h_b[k, 0], h_b[k, 1])
        r2, s2 = oracle.intra_check(r, s)
        o_rho[k], o_sig[k] = oracle.intra_grow(r2, s2, seq.grad[k])
    for mode in (0, 1, 2):
        a = pkg.Engine(W, H, n_kf, max_neighbours=n)
        b = pkg.Engine(W, H, n_kf, max_neighbours=n)
        a.set_scan_mode(mode)
        b.set_scan_mode(mode)
        seq.upload(a)
        seq.upload(b)
        a.upload_observations_batch(refs, [o[0] for o in obs], [o[1] for o in obs], [o[2] for o in obs])
        rot, mn, mx = a.search_priors(refs, nbrs)
        assert (rot == h_rot).all()
        assert_bit_equal(mn, h_b[:, 0], "min_depth")
        assert_bit_equal(mx, h_b[:, 1], "max_depth")
        a.recon_observed(refs, nbrs)
        b.recon(refs, nbrs, h_b[:, 0], h_b[:, 1], rot=h_rot)
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
        a.inter_check(refs, nbrs)  # the depth flags are set: the next stage accepts both
        b.inter_check(refs, nbrs)
        for k in refs:
            assert_bit_equal(a.download_checked(k), b.download_checked(k), "checked %s kf %d" % (name, k))
        a.close()
        b.close()
