"""GPU: the device ingest and gradient pre-pass PINNED against OpenCV 2.4.5 directly (loaded from oracle/_ref/, see
oracle/ref_opencv.py) -- no oracle in between:

  * sdm_upload_image_rgb / sdm_upload_images_rgb_batch, all five orders, with and without dist, == cvUndistort2 +
    cvCvtColor, at the reference's calibrations and at 1920x1080 / 1280x720;
  * sdm_upload_image / sdm_upload_images_batch / sdm_upload_image_device == cvSobel(CV_SCHARR)/32 + cvCartToPolar at
    sizes that straddle k_prepass_batch's 64x16 tiles, on images that reach |sx|, |sy| = 4080;
  * sdm_selftest(10): K1's fast_atan2_deg_x1 over all 2^32 inputs == fast_atan2_deg(y, 1), with the digest that
    tests/golden/make_fastatan2_digest.py recorded from OpenCV's cvFastArctan(y, 1).

The gray image, GradImg and GradTheta are read back with download_inputs and compared bit for bit."""
import numpy as np
import pytest

import cv_pin
from common import assert_bit_equal
from test_opencv_pin import _frame, _grad_cv, _test_images

pytestmark = pytest.mark.gpu
EYE = np.float32([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]])
ORDERS = (("rgb", 3), ("bgr", 3), ("rgba", 4), ("bgra", 4), ("gray", 1))


@pytest.fixture(scope="module")
def cv():
    return cv_pin.opencv()


def _cv_inputs(cv, px, order, K, dist):
    im = px if dist is None else cv.undistort(px, K, dist)
    im = im if order == "gray" else cv.cvt_gray(im, order)
    g, t = _grad_cv(cv, im)
    return im, g, t


def _check(eng, slot, want, what):
    im, g, t, _ = eng.download_inputs(slot)
    wi, wg, wt = want
    assert (im == wi).all(), "%s: %d gray pixels differ" % (what, int((im != wi).sum()))
    assert_bit_equal(g, wg, "GradImg " + what)
    assert_bit_equal(t, wt, "GradTheta " + what)


def _rgb_pins(cv, eng, W, H, K, dists, seed, what):
    rng = np.random.default_rng(seed)
    for order, ch in ORDERS:
        frames = [_frame(rng, H, W, ch) for _ in range(2)]
        for dist in dists:
            tag = "%s %dx%d %s dist=%s" % (what, W, H, order, None if dist is None else list(dist))
            want = [_cv_inputs(cv, f, order, K, dist) for f in frames]
            eng.upload_image_rgb(0, frames[0], order, K, dist, EYE)
            _check(eng, 0, want[0], "single " + tag)
            eng.upload_images_rgb_batch([1, 2], frames, order, K, dist, [EYE, EYE])
            _check(eng, 1, want[0], "batch[0] " + tag)
            _check(eng, 2, want[1], "batch[1] " + tag)


def _by_size():
    groups = {}
    for src, W, H, K, dist in cv_pin.calibrations():
        groups.setdefault((W, H), []).append((src, K, dist))
    return sorted(groups.items())


@pytest.mark.parametrize("size,cals", _by_size(), ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else "")
def test_device_ingest_vs_opencv_reference_calibrations(pkg, gpu_ok, cv, size, cals):
    W, H = size
    eng = pkg.Engine(W, H, 3)
    for i, (src, K, dist) in enumerate(cals):
        _rgb_pins(cv, eng, W, H, K, (dist, None) if i == 0 else (dist,), W * H + i, src)
    eng.close()


@pytest.mark.parametrize("W,H", [(1920, 1080), (1280, 720)])
def test_device_ingest_vs_opencv_hd(pkg, gpu_ok, cv, W, H):
    """chris_logic_HD720's calibration (scaled to the frame), a strong barrel and a far pincushion case (positions
    beyond the CV_16SC2 map's short range)"""
    src, _, _, K0, d0 = [c for c in cv_pin.calibrations() if c[0] == "chris_logic_HD720.yaml"][0]
    K = K0 * np.float32(W / 1280.0)
    eng = pkg.Engine(W, H, 3)
    _rgb_pins(cv, eng, W, H, K, (d0, None, np.float32([-0.9, 0.3, 0, 0, -0.05]), np.float32([2e4, 0, 0, 0, 0])),
              W, "HD")
    eng.close()


PREPASS_SIZES = [(63, 15), (64, 16), (65, 17), (129, 16), (64, 15), (65, 16), (63, 17), (129, 17), (67, 31), (97, 61),
                 (131, 19), (8, 8)]


@pytest.mark.parametrize("W,H", PREPASS_SIZES)
def test_device_prepass_vs_opencv(pkg, gpu_ok, cv, W, H):
    import torch
    rng = np.random.default_rng(W * 100 + H)
    ims = [im for _, im in _test_images(rng, H, W)]
    want = [(im,) + tuple(_grad_cv(cv, im)) for im in ims]
    n = len(ims)
    K = np.float32([0.8 * W, 0.8 * W, W / 2, H / 2])
    eng = pkg.Engine(W, H, 2 * n + 1)
    for i, im in enumerate(ims):
        eng.upload_image(i, im, K, EYE)
        _check(eng, i, want[i], "upload_image %dx%d #%d" % (W, H, i))
    eng.upload_images_batch(list(range(n, 2 * n)), ims, K, [EYE] * n)
    for i in range(n):
        _check(eng, n + i, want[i], "upload_images_batch %dx%d #%d" % (W, H, i))
    for i, im in enumerate(ims):
        d = torch.from_numpy(np.ascontiguousarray(im)).cuda()
        torch.cuda.synchronize()
        eng.upload_image_device(2 * n, d.data_ptr(), K, EYE)
        _check(eng, 2 * n, want[i], "upload_image_device %dx%d #%d" % (W, H, i))
        del d
    eng.close()


def test_selftest_fast_atan2_x1_equals_opencv(pkg, gpu_ok):
    """K1's fast_atan2_deg_x1 (PM.cc:414) over every float input: 0 mismatches against fast_atan2_deg(y, 1), and the
    digest of its results equals OpenCV 2.4.5's cvFastArctan(y, 1) over the same 2^32 inputs"""
    eng = pkg.Engine(64, 16, 1)
    bad, digest = eng.selftest(10)
    eng.close()
    assert bad == 0, "%d of 2^32 inputs differ" % bad
    assert "0x%016x" % digest == cv_pin.digest_fixture()["digest"]
