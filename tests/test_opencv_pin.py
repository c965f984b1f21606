"""CPU: the oracle's OpenCV pieces PINNED against OpenCV 2.4.5 itself -- the prebuilt libraries the reference ships,
staged into oracle/_ref/ by `python __graft_entry__.py` (oracle/ref_opencv.py) and called through their C API.

  N7  cv::fastAtan2 (PM.cc:414 and GradTheta) and the Scharr/32 gradient with cvCartToPolar's magnitude and phase;
      the replicated border of cvSobel, and where cv::Scharr's default BORDER_REFLECT_101 differs (outer ring only);
  N9  cv::undistort (cvUndistort2) and cvtColor(RGB/BGR/RGBA/BGRA -> GRAY) against pmo_ingest;
  N1/N2  every rule of np_pm's mode="cv" (cvGEMM flag combinations PM.cc uses, cvInvert, cvConvertScale).

All bit-exact.  A missing oracle/_ref/ fails these tests (never a skip).  SDM_FUZZ_ATAN_ALL=1 walks all 2^32 float
patterns of fastAtan2(y, 1) and re-derives tests/golden/fastatan2_x1_digest.json (minutes on 16 threads)."""
import os

import numpy as np
import pytest

import cv_pin
import np_pm
import ref_opencv as R
from common import assert_bit_equal

f32, f64 = np.float32, np.float64
ORDERS = ("rgb", "bgr", "rgba", "bgra")
EYE_K = np.float32([500, 500, 0, 0])


@pytest.fixture(scope="module")
def cv():
    return cv_pin.opencv()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return cv_pin.Harness(str(tmp_path_factory.mktemp("cv_pin")))


def _grad_cv(cv, im, border=R.BORDER_REPLICATE):
    """cv::Scharr / 32 then cartToPolar(deg); REFLECT_101 built as copyMakeBorder(1) + cvSobel + crop"""
    if border == R.BORDER_REFLECT_101:
        sx, sy = cv.scharr(cv.copy_make_border(im, 1, 1, 1, 1, border))
        sx, sy = sx[1:-1, 1:-1], sy[1:-1, 1:-1]
    else:
        sx, sy = cv.scharr(im)
    return cv.cart_to_polar(sx * f32(1 / 32), sy * f32(1 / 32))


def _test_images(rng, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    spike = np.zeros((H, W), np.uint8)
    spike[H // 2, W // 2] = 255
    yield "noise", rng.integers(0, 256, (H, W), dtype=np.uint8)
    yield "checker", (((yy + xx) & 1) * 255).astype(np.uint8)
    yield "stripes", ((xx & 1) * 255).astype(np.uint8)
    yield "spike", spike
    yield "flat", np.full((H, W), 77, np.uint8)


# ---- N7: fastAtan2 ---------------------------------------------------------------------------------------------------
def test_fast_atan2_x1_sweep(harness):
    """pmo_fast_atan2(y, 1) == cvFastArctan(y, 1) (PM.cc:414): every float in [-4, 4] (both signs, denormals and zeros)
    plus every 4099th pattern of the rest (Inf, NaN, huge); NaN results match NaN.  SDM_FUZZ_ATAN_ALL=1: all 2^32
    patterns, and their digest must be the recorded one (tests/golden/fastatan2_x1_digest.json)."""
    if os.environ.get("SDM_FUZZ_ATAN_ALL", "0") != "0":
        bad, dig = harness.all_patterns()
        assert bad == 0
        assert "0x%016x" % dig == cv_pin.digest_fixture()["digest"]
        return
    four = 0x40800000  # bits of 4.0f
    for lo, hi, stride in ((0, four + 1, 1), (0x80000000, 0x80000000 + four + 1, 1),
                           (four + 1, 0x80000000, 4099), (0x80000000 + four + 1, 2 ** 32, 4099)):
        bad, _, first = harness.sweep(lo, hi, stride)
        assert bad == 0, "%d mismatches in [%#x, %#x), first at pattern %#x" % (bad, lo, hi, first)


def test_fast_atan2_two_arguments(cv, harness):
    """pmo_fast_atan2(y, x) == cvFastArctan(y, x) on mixed magnitudes, signs, zeros, the diagonal, Inf and NaN"""
    rng = np.random.default_rng(414)
    mag = lambda n: rng.standard_normal(n) * np.exp2(rng.integers(-140, 128, n).astype(f64))
    with np.errstate(all="ignore"):
        y, x = mag(60000).astype(f32), mag(60000).astype(f32)
    special = f32([0.0, -0.0, 1.0, -1.0, 1e-45, -1e-45, 3e38, -3e38, np.inf, -np.inf, np.nan, 0.5, -2.0])
    sy, sx = np.meshgrid(special, special)
    y = np.concatenate([y, sy.ravel(), x[:1000]])
    x = np.concatenate([x, sx.ravel(), x[:1000]])  # y == x: the branch boundary ax >= ay
    want = f32([cv.fast_arctan(a, b) for a, b in zip(y.tolist(), x.tolist())])
    assert_bit_equal(harness.oracle_atan2(y, x), want, "fastAtan2(y, x)")


# ---- N7: GradImg / GradTheta ---------------------------------------------------------------------------------------
def test_gradient_over_every_scharr_sum_pair(cv, harness):
    """GradImg and GradTheta are a pure function of the integer Scharr sums (sx, sy) in [-4080, 4080]^2: the oracle's
    sqrtf(gx*gx + gy*gy) and pmo_fast_atan2(gy, gx) equal cvCartToPolar(deg) on every one of the 66.6 M pairs."""
    s = np.arange(-4080, 4081, dtype=np.int32)
    gy_row = (s.astype(f32) * f32(1 / 32))[None, :]
    for lo in range(0, len(s), 1024):
        gx = np.repeat((s[lo:lo + 1024].astype(f32) * f32(1 / 32))[:, None], len(s), axis=1)
        gy = np.ascontiguousarray(np.broadcast_to(gy_row, gx.shape))
        mag, ang = cv.cart_to_polar(gx, gy)
        assert_bit_equal(np.sqrt(gx * gx + gy * gy), mag, "GradImg, sx from %d" % s[lo])
        assert_bit_equal(harness.oracle_atan2(gy, gx), ang, "GradTheta, sx from %d" % s[lo])


SIZES = [(1, 1), (1, 2), (2, 1), (1, 7), (3, 1), (2, 2), (2, 3), (3, 2), (3, 3), (3, 50), (17, 65), (16, 64),
         (7, 1919), (61, 97), (480, 640)]


@pytest.mark.parametrize("H,W", SIZES)
def test_scharr_replicated_border_equals_prepass(cv, oracle, H, W):
    """cvSobel(CV_SCHARR) (replicated border) / 32 + cvCartToPolar == pmo_gradient_prepass everywhere, border included,
    on noise, 0/255 checkerboards and stripes (|sx|, |sy| = 4080) and a single-pixel spike"""
    rng = np.random.default_rng(H * 1000 + W)
    for what, im in _test_images(rng, H, W):
        mag, ang = _grad_cv(cv, im)
        g, t, _ = oracle.gradient_prepass(im)
        assert_bit_equal(g, mag, "GradImg %s %dx%d" % (what, W, H))
        assert_bit_equal(t, ang, "GradTheta %s %dx%d" % (what, W, H))


@pytest.mark.parametrize("H,W", [s for s in SIZES if min(s) >= 2])
def test_scharr_reflect101_differs_only_on_outer_ring(cv, oracle, H, W):
    """DESIGN N7's deviation, measured: cv::Scharr's default BORDER_REFLECT_101 equals the oracle off the outermost
    ring of pixels; on the ring it differs (reported per size)"""
    rng = np.random.default_rng(W * 1000 + H)
    ring = np.ones((H, W), bool)
    ring[1:-1, 1:-1] = False
    differ = 0
    for what, im in _test_images(rng, H, W):
        mag, ang = _grad_cv(cv, im, R.BORDER_REFLECT_101)
        g, t, _ = oracle.gradient_prepass(im)
        d = (g.view(np.uint32) != mag.view(np.uint32)) | (t.view(np.uint32) != ang.view(np.uint32))
        assert not (d & ~ring).any(), "%s %dx%d: %d interior pixels differ" % (what, W, H, int((d & ~ring).sum()))
        if what == "noise":
            differ = int(d.sum())
    print("REFLECT_101 vs replicated, %dx%d noise: %d of %d ring pixels differ" % (W, H, differ, int(ring.sum())))
    assert 0 < differ <= ring.sum()


# ---- N9: cvtColor and undistort ------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_cvtcolor_every_colour(cv, oracle, order):
    """RGB2Gray<uchar> (4899/9617/1868 >> 14) of all 2^24 colours, per channel order (alpha bytes random)"""
    c = np.arange(2 ** 24, dtype=np.uint32)
    rgb = np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    px = rgb if order in ("rgb", "rgba") else rgb[..., ::-1]
    if len(order) == 4:
        alpha = np.random.default_rng(7).integers(0, 256, (4096, 4096, 1), dtype=np.uint8)
        px = np.concatenate([px, alpha], -1)
    px = np.ascontiguousarray(px)
    want = cv.cvt_gray(px, order)
    got = oracle.ingest(px, order, EYE_K, None)
    assert (got == want).all(), "%s: %d colours differ" % (order, int((got != want).sum()))


def _frame(rng, H, W, ch):
    yy, xx = np.mgrid[0:H, 0:W]
    base = (127 + 100 * np.sin(xx / 9.0) * np.cos(yy / 7.0))[..., None] + rng.integers(-40, 40, (H, W, max(ch, 1)))
    px = np.clip(base, 0, 255).astype(np.uint8)
    return px[..., 0].copy() if ch == 1 else px


def _cv_ingest(cv, px, order, K, dist):
    u = cv.undistort(px, K, dist)
    return u if order == "gray" else cv.cvt_gray(u, order)


def _pin_ingest(cv, oracle, px, order, K, dist, what):
    want = _cv_ingest(cv, px, order, K, dist)
    got = oracle.ingest(px, order, K, dist)
    assert (got == want).all(), "%s %s: %d of %d pixels differ" % (what, order, int((got != want).sum()), got.size)
    return want


@pytest.mark.parametrize("cal", cv_pin.calibrations(), ids=lambda c: c[0].replace("Examples/", ""))
def test_undistort_reference_calibrations(cv, oracle, cal):
    """cvUndistort2 + cvCvtColor == pmo_ingest at every calibration the reference ships, at its native size, for
    1-, 3- and 4-channel frames"""
    src, W, H, K, dist = cal
    rng = np.random.default_rng(W * H)
    for order, ch in (("gray", 1), ("rgb", 3), ("bgra", 4)):
        _pin_ingest(cv, oracle, _frame(rng, H, W, ch), order, K, dist, src)


STRONG = [  # (what, W, H, dist): strong barrel / pincushion, k3, tangential, odd sizes, far outside the frame
    ("barrel k1=-0.9", 640, 480, [-0.9, 0, 0, 0, 0]),
    ("pincushion k1=+0.9", 640, 480, [0.9, 0, 0, 0, 0]),
    ("k3 barrel", 641, 479, [-0.3, 0.1, 0, 0, -0.45]),
    ("k3 pincushion", 97, 61, [0.2, -0.1, 0.003, -0.004, 0.8]),
    ("tangential", 333, 211, [0.0, 0.0, 0.05, -0.04, 0.0]),
    ("mustache", 1281, 719, [-0.6, 1.2, 0, 0, -0.9]),
    ("far 1e4 (short map wraps)", 640, 480, [1e4, 0, 0, 0, 0]),
    ("far 1e6", 640, 480, [1e6, 0, 0, 0, 0.5]),
    ("far 1e9 (cvRound gives INT_MIN)", 640, 480, [1e9, 0, 0, 0, 0]),
    ("far -1e5", 127, 95, [-1e5, 3e4, 0, 0, 0]),
]


@pytest.mark.parametrize("what,W,H,dist", STRONG, ids=[s[0] for s in STRONG])
def test_undistort_strong_and_far(cv, oracle, what, W, H, dist):
    rng = np.random.default_rng(W + H)
    K = np.float32([0.8 * W, 0.8 * W, 0.5 * W - 0.3, 0.5 * H + 0.2])
    dist = np.float32(dist)
    for order, ch in (("gray", 1), ("bgr", 3), ("rgba", 4)):
        want = _pin_ingest(cv, oracle, _frame(rng, H, W, ch), order, K, dist, what)
        assert (want == 0).any() or abs(dist[0]) < 1, what  # the constant border shows up


# ---- N1/N2: cvGEMM, cvInvert, cvConvertScale against np_pm's mode="cv" ----------------------------------------------
def _adversarial_3x3(rng, spread):
    A = (rng.standard_normal((3, 3)) * np.exp2(rng.integers(-spread, spread + 1, (3, 3)))).astype(f32)
    if rng.integers(4) == 0:  # cancellation: a column that nearly cancels against the row it meets
        A[:, 2] = -A[:, 0] * f32(1 + 2 ** -20)
    return A


def _rotation(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q.astype(f32)


@pytest.mark.parametrize("seed", range(4))
def test_gemm_rules_of_np_pm_cv_mode(cv, seed):
    """every cvGEMM call PM.cc makes, against the np_pm helper that states its rounding"""
    rng = np.random.default_rng(seed)
    for it in range(500):
        spread = (0, 6, 30)[it % 3]
        A, B = (_rotation(rng), _rotation(rng)) if it % 2 else (_adversarial_3x3(rng, spread), _adversarial_3x3(rng, spread))
        xp = np.array([[rng.standard_normal()], [rng.standard_normal()], [1]], f32)
        c = (rng.standard_normal((3, 1)) * np.exp2(rng.integers(-spread, spread + 1, (3, 1)))).astype(f32)
        # Rcw2*Rcw1.t() (PM.cc:643,859,890,978): GEMM_2_T, double accumulation
        assert_bit_equal(cv.gemm(A, B, 1.0, None, 0.0, R.CV_GEMM_B_T),
                         np_pm._matmul(A, B.T.copy(), "cv", transposed_operand=True), "A*B.t()")
        # -Rcw2*Rcw1.t(): alpha = -1 folded, == the negated product (np_pm.Pair._rel)
        assert_bit_equal(cv.gemm(A, B, -1.0, None, 0.0, R.CV_GEMM_B_T),
                         -np_pm._matmul(A, B.T.copy(), "cv", transposed_operand=True), "-A*B.t()")
        # plain 3x3*3x3 (F12 chain, PM.cc:986) and 3x3*3x1 (K*temp, PM.cc:679): float left to right
        assert_bit_equal(cv.gemm(A, B), np_pm._matmul(A, B, "cv"), "A*B")
        assert_bit_equal(cv.gemm(A, xp), np_pm._matmul(A, xp, "cv"), "A*xp")
        # (-R)*t + c (PM.cc:644): float dot, then (float)(t*alpha + c*beta) in double (np_pm.Pair._rel)
        neg = -A
        want = f32([[f64(np_pm._dot_f32(neg[i], c[:, 0])) * 1.0 + f64(xp[i, 0]) * 1.0] for i in range(3)])
        assert_bit_equal(cv.gemm(neg, c, 1.0, xp, 1.0), want, "(-R)*t + c")
        # R21*xp*mind + t21 (PM.cc:894) and Rji*xp/depthp + tji (PM.cc:678): alpha folded into the double tail
        for alpha in (f64(f32(rng.uniform(0.01, 20))), 1.0 / f64(f32(rng.uniform(0.01, 20)))):
            want = f32([[f64(np_pm._dot_f32(A[i], xp[:, 0])) * alpha + f64(c[i, 0])] for i in range(3)])
            assert_bit_equal(cv.gemm(A, xp, alpha, c, 1.0), want, "R*xp*alpha + t")
        # R21.row(2)*xp*ucx, fx*(R21.row(0)*xp) (PM.cc:866-868), Rji.row(2)*xp (684, 777): 1x1, double dot, alpha folded
        for r in range(3):
            alpha = f64(f32(rng.uniform(-900, 900)))
            assert_bit_equal(cv.gemm(A[r:r + 1].copy(), xp, alpha), [[f32(np_pm._dot_f64(A[r], xp[:, 0]) * alpha)]],
                             "row*xp*alpha")
            assert_bit_equal(cv.gemm(A[r:r + 1].copy(), xp), [[f32(np_pm._dot_f64(A[r], xp[:, 0]))]], "row*xp")


def test_gemm_jacobian_products(cv):
    """-J.t()*r0 and J.t()*J (PM.cc:788-789) over up to 4 taps x 20 neighbours: GEMM_1_T, double accumulation in
    order, alpha folded, one rounding -- np_pm.inter_check's sum_Jr64 / sum_JJ64"""
    rng = np.random.default_rng(788)
    for it in range(3000):
        n = int(rng.integers(1, 81))
        J = (rng.standard_normal((n, 1)) * np.exp2(rng.integers(-30, 31, (n, 1)))).astype(f32)
        r0 = (rng.standard_normal((n, 1)) * np.exp2(rng.integers(-30, 31, (n, 1)))).astype(f32)
        if it % 5 == 0:
            r0[n // 2:] = -r0[:n - n // 2][: n - n // 2]  # cancellation
        jr, jj = f64(0), f64(0)
        for k in range(n):
            jr = jr + f64(J[k, 0]) * f64(r0[k, 0])
            jj = jj + f64(J[k, 0]) * f64(J[k, 0])
        assert_bit_equal(cv.gemm(J, r0, -1.0, None, 0.0, R.CV_GEMM_A_T), [[f32(jr * -1.0)]], "-J.t()*r0 n=%d" % n)
        assert_bit_equal(cv.gemm(J, J, 1.0, None, 0.0, R.CV_GEMM_A_T), [[f32(jj)]], "J.t()*J n=%d" % n)


def test_invert_rule_of_np_pm_cv_mode(cv):
    """K.inv() and K1.t().inv() (PM.cc:841, 986): cvInvert(CV_LU) of the 3x3 float K == np_pm._kinv(mode="cv"),
    including K with large c/f and wide exponent spreads"""
    rng = np.random.default_rng(986)
    for it in range(4000):
        if it % 4 == 0:
            fx, fy = f32(rng.uniform(0.5, 3)), f32(rng.uniform(0.5, 3))
            cx, cy = f32(rng.uniform(500, 5e4)), f32(rng.uniform(500, 5e4))  # c/f up to 1e5
        else:
            fx, fy = f32(np.exp2(rng.uniform(-10, 14))), f32(np.exp2(rng.uniform(-10, 14)))
            cx, cy = f32(rng.uniform(-2000, 4000)), f32(rng.uniform(-2000, 4000))
        K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], f32)
        assert_bit_equal(cv.invert(K)[0], np_pm._kinv(fx, fy, cx, cy, "cv"), "K.inv()")
        assert_bit_equal(cv.invert(K.T.copy())[0], np_pm._kinv(fx, fy, cx, cy, "cv", transpose=True), "K.t().inv()")


def test_convert_scale_rule_of_np_pm_cv_mode(cv):
    """Xj/Xj(2) (PM.cc:680) is convertTo with alpha = 1./s: x * (float)(1./s) + 0.0f in float (a -0 comes back +0)"""
    rng = np.random.default_rng(680)
    X = (rng.standard_normal((4096, 1)) * np.exp2(rng.integers(-60, 60, (4096, 1)))).astype(f32)
    X[:4, 0] = [0.0, -0.0, 1e-45, -3e38]
    for s in np.concatenate([rng.uniform(-9, 9, 300), [1e-30, -1e30, 3.0]]).astype(f32):
        sc = f32(1.0 / f64(s))
        with np.errstate(over="ignore"):
            want = X * sc + f32(0)
        assert_bit_equal(cv.convert_scale(X, 1.0 / f64(s)), want, "X/%r" % s)
