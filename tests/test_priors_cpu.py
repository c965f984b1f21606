"""CPU checks of the device priors' building blocks (csrc/sdm_priors.h): the order-preserving float key map and the
4-pass radix select of rank (m - 1) / 2, restated in NumPy; and the synthetic ORB observations (synth.Scene.observations)
that the GPU tests feed to the engine."""
import numpy as np
import pytest


def f2key(x):
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def key2f(k):
    k = np.uint32(k)
    b = (k & np.uint32(0x7FFFFFFF)) if (k & np.uint32(0x80000000)) else ~k
    return np.array([b], np.uint32).view(np.float32)[0]


def radix_select(x):
    """k_priors' selection: 4 passes of 8-bit histograms over the keys that share the prefix chosen so far"""
    keys = f2key(x)
    m = len(keys)
    if m == 0:
        return np.float32(0)
    k = (m - 1) // 2
    prefix = np.uint32(0)
    for shift in (24, 16, 8, 0):
        hmask = np.uint32(0) if shift == 24 else np.uint32((0xFFFFFFFF << (shift + 8)) & 0xFFFFFFFF)
        live = keys[(keys & hmask) == prefix]
        hist = np.bincount(((live >> np.uint32(shift)) & np.uint32(255)).astype(np.int64), minlength=256)
        excl = np.cumsum(hist) - hist
        b = int(np.nonzero((excl <= k) & (k < excl + hist))[0][0])
        prefix = np.uint32(prefix | np.uint32(b << shift))
        k -= int(excl[b])
    return key2f(prefix)


def nasty_floats(rng, n):
    pick = rng.integers(0, 6, n)
    x = rng.standard_normal(n).astype(np.float32) * np.float32(100)
    x[pick == 0] = 0.0
    x[pick == 1] = -0.0
    sub = (rng.integers(1, 1 << 23, n).astype(np.uint32)).view(np.float32)  # subnormals
    x[pick == 2] = np.where(rng.integers(0, 2, n) == 1, sub, -sub)[pick == 2]
    x[pick == 3] = np.float32(rng.choice([-3.5, 1.25, 7.0], n))[pick == 3]  # ties
    return x


def test_key_map_orders_floats():
    rng = np.random.default_rng(1)
    x = nasty_floats(rng, 20000)
    order = np.argsort(f2key(x), kind="stable")
    xs = x[order]
    assert (xs[1:] >= xs[:-1]).all()
    # -0 sorts just below +0, and the map inverts
    assert f2key(np.float32([-0.0]))[0] + 1 == f2key(np.float32([0.0]))[0]
    for v in x[:2000]:
        assert key2f(f2key(np.float32([v]))[0]).view(np.uint32) == np.float32(v).view(np.uint32)


@pytest.mark.parametrize("m", [1, 2, 3, 4, 7, 64, 65, 999, 1000, 2000, 8192])
def test_radix_select_is_the_sorted_median(m):
    rng = np.random.default_rng(m)
    for _ in range(5):
        x = nasty_floats(rng, m)
        want = np.sort(x)[(m - 1) // 2]
        got = radix_select(x)
        assert got == want, (m, got, want)  # (== : -0 and +0 are equal, as std::sort leaves their order open)


def test_radix_select_empty_is_zero():
    assert radix_select(np.zeros(0, np.float32)) == 0


@pytest.mark.parametrize("strip", [False, True])
def test_synth_observations(pkg, strip):
    synth = pkg.synth
    cam = synth.scaled_intrinsics(synth.TUM1, 160, 120)
    scene = synth.Scene(cam, 0x5EED0104, disparity_px=3.0, strip=strip, roll_deg=5.0)
    seen = []
    for k in range(6):
        ids, ang, dep = scene.observations(k, 1500, 11)
        assert ids.dtype == np.int32 and ang.dtype == np.float32 and dep.dtype == np.float32
        assert len(ids) == len(ang) > 1500
        pos = ids[ids >= 0]
        assert len(np.unique(pos)) == len(pos), "a map point at two keypoints of one keyframe"
        assert (ids[ids < 0] == -1).all() and len(pos) > 900
        assert np.isfinite(ang).all() and ((ang == -1) | ((ang >= 0) & (ang < 360))).all()
        assert 0 < (ang == -1).mean() < 0.2
        assert len(dep) == len(pos) and (dep > 0).all()
        seen.append(set(pos.tolist()))
        again = scene.observations(k, 1500, 11)
        assert all(np.array_equal(a, b) for a, b in zip((ids, ang, dep), again))
    assert len(seen[0] & seen[5]) > 800  # keyframes share most of their map points
