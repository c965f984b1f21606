"""CPU: the per-pair operand boxes behind K1's reciprocal-form quotients (sdm_device.h quot_boxes, SDM_K1_OPT bits 18-20),
through the NumPy restatement in quot_boxes_np.py.

 * soundness by containment: for random and hand-made geometries every operand the search's statements produce at sampled
   pixels (the four corners and the principal point among them), depths and line positions lies inside the box the
   restatement computed;
 * the degenerate pairs are refused;
 * the benchmark's geometry is accepted for all 20 neighbours;
 * quot_fast, modelled with exact rationals and correctly rounded float32 steps, is the correctly rounded quotient on the
   edges of the proved operand ranges."""
import math
from fractions import Fraction

import numpy as np
import pytest

import np_pm
import quot_boxes_np as qb

f32 = np.float32


def rot(rx, ry, rz):
    cx_, sx_, cy_, sy_, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]])
    Rx = np.array([[1.0, 0, 0], [0, cx_, -sx_], [0, sx_, cx_]])
    Ry = np.array([[cy_, 0, sy_], [0, 1.0, 0], [-sy_, 0, cy_]])
    return Ry @ Rx @ Rz


class Cam:
    def __init__(self, K, R, C):
        self.fx, self.fy, self.cx, self.cy = [f32(v) for v in K]
        self.R = np.asarray(R, np.float64).T.astype(f32)  # Rcw
        self.t = (-np.asarray(R, np.float64).T @ np.asarray(C, np.float64)).astype(f32)


def pair_args(k1, k2, istd, mind, maxd, W, H):
    p = np_pm.Pair(k1, k2)  # R21, t21 with float products and left-to-right float sums, as pair_geometry computes them
    return dict(Rx=p.R21[0], Rz=p.R21[2], tx=p.t21[0], tz=p.t21[2], istd=istd, fx=k1.fx, fy=k1.fy, cx=k1.cx, cy=k1.cy,
                mind=mind, maxd=maxd, W=W, H=H)


def inside(v, box, what):
    assert box[0] <= v <= box[1], (what, float(v), [float(b) for b in box])


def check_containment(a, boxes, bits, rng, n_px=12):
    """the statements of epipolar_search / search_range_int1 / pixel_depth in float32 at sampled operands"""
    W, H = a["W"], a["H"]
    fx, fy, cx, cy = a["fx"], a["fy"], a["cx"], a["cy"]
    px = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1),
          (min(max(int(round(float(cx))), 0), W - 1), min(max(int(round(float(cy))), 0), H - 1))]
    px += [(int(rng.integers(0, W)), int(rng.integers(0, H))) for _ in range(n_px)]
    Rx, Rz, tx, tz = [f32(v) for v in a["Rx"]], [f32(v) for v in a["Rz"]], f32(a["tx"]), f32(a["tz"])
    for x, y in px:
        xp0, xp1 = f32(f32(x) - cx) / fx, f32(f32(y) - cy) / fy
        inside(xp0, boxes["xp0"], "xp0")
        inside(xp1, boxes["xp1"], "xp1")
        rxxp = f32(f32(f32(Rx[0] * xp0) + f32(Rx[1] * xp1)) + f32(Rx[2] * f32(1)))
        rzxp = f32(f32(f32(Rz[0] * xp0) + f32(Rz[1] * xp1)) + f32(Rz[2] * f32(1)))
        inside(rxxp, boxes["rxxp"], "rxxp")
        inside(rzxp, boxes["rzxp"], "rzxp")
        for name, d in (("min", f32(a["mind"])), ("max", f32(a["maxd"]))):
            xk, zk = f32(f32(rxxp * d) + tx), f32(f32(rzxp * d) + tz)
            inside(xk, boxes["x_" + name], "x_" + name)
            inside(zk, boxes["z_" + name], "z_" + name)
            inside(f32(fx * xk), boxes["fxx_" + name], "fx*x_" + name)
            if bits & 8:
                assert qb.DIV_LO <= abs(zk) <= qb.DIV_HI
                assert xk == 0 or qb.NUM_LO <= abs(f32(fx * xk)) <= qb.NUM_HI
        us = [f32(-4 * W), f32(5 * W), f32(0), cx, f32(W - 1)] + [f32(u) for u in rng.uniform(-4 * W, 5 * W, 6)]
        for u in us:
            ucx = f32(u - cx)
            inside(ucx, boxes["ucx"], "ucx")
            num = f32(f32(rzxp * ucx) - f32(fx * rxxp))
            den = f32(f32(f32(-tz) * ucx) + f32(fx * tx))
            inside(num, boxes["num"], "num1 - num2")
            inside(den, boxes["den"], "denom1 + denom2")
            if bits & 16:
                assert qb.DIV_LO <= abs(den) <= qb.DIV_HI
                assert (num == 0 and not np.signbit(num)) or qb.NUM_LO <= abs(num) <= qb.NUM_HI


def random_pair(rng, kind):
    W, H = int(rng.integers(16, 1400)), int(rng.integers(16, 1100))
    f = float(rng.uniform(0.4, 2.5)) * W
    K = (f, f * float(rng.uniform(0.9, 1.1)), W * float(rng.uniform(0.3, 0.7)), H * float(rng.uniform(0.3, 0.7)))
    ang = dict(small=0.02, medium=0.3, large=2.0)[kind]
    b = dict(small=0.01, medium=0.2, large=3.0)[kind]
    k1 = Cam(K, rot(*rng.uniform(-ang, ang, 3)), rng.uniform(-b, b, 3))
    k2 = Cam(K, rot(*rng.uniform(-ang, ang, 3)), rng.uniform(-b, b, 3))
    mu, s = float(rng.uniform(0.3, 5.0)), float(rng.uniform(0.02, 0.24))
    return pair_args(k1, k2, f32(rng.uniform(0.5, 120.0)), f32(1 / (mu - 2 * s * mu)), f32(1 / (mu + 2 * s * mu)), W, H)


def test_boxes_contain_every_sampled_operand():
    rng = np.random.default_rng(20260)
    accepted = {8: 0, 16: 0}
    n = 0
    for kind, count in (("small", 1500), ("medium", 1000), ("large", 500)):
        for _ in range(count):
            a = random_pair(rng, kind)
            bits, boxes = qb.quot_boxes(**a)
            n += 1
            if not boxes:
                continue
            check_containment(a, boxes, bits, rng, n_px=3)
            for b in accepted:
                accepted[b] += bool(bits & b)
    assert n == 3000
    assert accepted[8] > 1000 and accepted[16] > 500, accepted  # the sweep exercises accepted pairs, not only refusals


TUM = (517.3, 516.5, 318.6, 255.3)


def handmade():
    """name -> (arguments, bits that must be refused)"""
    W, H = 640, 480
    I = np.eye(3)
    mind, maxd = f32(1.25), f32(1 / 1.2)
    out = {}
    k1 = Cam(TUM, rot(0.002, -0.003, 0.01), (0, 0, 0))
    out["pure_rotation"] = (pair_args(k1, Cam(TUM, rot(0.01, 0.02, -0.01), (0, 0, 0)), 40, mind, maxd, W, H), 24)
    out["baseline_0"] = (pair_args(k1, Cam(TUM, rot(0.002, -0.003, 0.01), (0, 0, 0)), 40, mind, maxd, W, H), 24)
    # the neighbour looks sideways (yaw 0.5 rad) and sits ahead: z_min = rzxp*mind + tz changes sign inside the image
    side = pair_args(Cam(TUM, I, (0, 0, 0)), Cam(TUM, rot(0, 0.5, 0), (0.05, 0, 0.9)), 40, mind, maxd, W, H)
    out["z_min_crosses_zero"] = (side, 8)
    good = pair_args(k1, Cam(TUM, rot(0.004, 0.001, -0.006), (0.02, 0.001, 0.0005)), 40, mind, maxd, W, H)
    out["mind_0"] = (dict(good, mind=f32(0)), 24)
    tiny = dict(good)
    tiny["Rx"] = np.array([good["Rx"][0], 1e-30, good["Rx"][2]], f32)
    out["entry_1e-30"] = (tiny, 24)
    out["tz_1e-30"] = (dict(good, tz=f32(1e-30)), 24)
    out["negative_zero_tz"] = (dict(good, tz=f32(-0.0)), 24)
    out["negative_fx"] = (dict(good, fx=f32(-517.3)), 24)
    out["nan_istd"] = (dict(good, istd=f32("nan")), 16)
    out["inf_tx"] = (dict(good, tx=f32("inf")), 24)
    # forward motion: denom1 + denom2 = -tz*(u - cx) + fx*tx crosses zero for a u inside [-4W, 5W]
    out["forward_motion"] = (pair_args(k1, Cam(TUM, rot(0.002, -0.003, 0.01), (0.001, 0, 0.05)), 40, mind, maxd, W, H), 16)
    return good, out


def test_handmade_degenerate_pairs_are_refused():
    rng = np.random.default_rng(7)
    good, cases = handmade()
    bits, boxes = qb.quot_boxes(**good)
    assert bits & 8 and bits & 16, "the well-conditioned pair next to the degenerate ones must be accepted"
    check_containment(good, boxes, bits, rng)
    for name, (a, refused) in cases.items():
        bits, boxes = qb.quot_boxes(**a)
        assert bits & refused == 0, (name, hex(bits))
        if name == "z_min_crosses_zero":
            z = boxes["z_min"]
            assert z[0] < 0 < z[1]
        if boxes and all(np.isfinite([float(v) for v in (a["tx"], a["tz"], a["istd"])])):
            check_containment(a, boxes, bits, rng)


def test_bench_geometry_is_accepted(pkg):
    """bench.py's headline workload: synth.TUM1 at 640x480, disparity 2.6 px, roll 1 degree, 64 keyframes x 20 neighbours, depth
    prior spread 0.1 (seed: bench.py's for 480p).  Every pair must take the fast quotients, whatever the images' I_stddev"""
    synth = pkg.synth
    sc = synth.Scene(synth.TUM1, 0x5EED0002, disparity_px=2.6, roll_deg=1.0)
    W, H = synth.TUM1["W"], synth.TUM1["H"]
    mind, maxd = sc.depth_prior(0.1)
    K = sc.K()

    class M:
        pass

    def kf(k):
        m = M()
        T = sc.Tcw(k)
        m.R, m.t = T[:, :3].copy(), T[:, 3].copy()
        m.fx, m.fy, m.cx, m.cy = K
        return m

    kfs = [kf(k) for k in range(64)]
    rng = np.random.default_rng(3)
    worst_e = 0
    for k in range(64):
        for j in sc.neighbours(k, 64, 20):
            for istd in (1.0, 45.0, 127.5):
                a = pair_args(kfs[k], kfs[j], istd, mind, maxd, W, H)
                bits, boxes = qb.quot_boxes(**a)
                assert bits & 8 and bits & 16, (k, j, istd, hex(bits))
                worst_e = max(worst_e, (bits >> 8) & 0xFF)
            if (k + j) % 37 == 0:
                check_containment(a, boxes, bits, rng, n_px=2)
    # the per-lane window starts at 2^E <= 0.25: below one quarter of a squared gray level per pixel the refinement has no
    # gradient to work with anyway
    assert worst_e <= 125, worst_e


def edge_values():
    def nb(v, k):  # the float32 k steps above (below) a positive v
        return float((np.array([v], f32).view(np.int32) + np.int32(k)).view(f32)[0])
    nums = [0.0]
    for v in (2.0 ** -66, 2.0 ** 40, 1.0, 3.0, 2.0 ** -20):
        nums += [v, nb(v, 1) if v < 2.0 ** 40 else v, nb(v, -1) if v > 2.0 ** -66 else v]
    dens = []
    for v in (2.0 ** -30, 2.0 ** 30, 1.0, 3.0, 7.0):
        dens += [v, nb(v, 1) if v < 2.0 ** 30 else v, nb(v, -1) if v > 2.0 ** -30 else v]
    dens += [float(np.array([(e << 23) | 0x7FFFFF], np.uint32).view(f32)[0]) for e in (97, 126, 127, 155)]  # all-ones significands
    return sorted(set(nums)), sorted(set(dens))


def test_quot_fast_is_the_rounded_quotient_on_the_box_edges():
    nums, dens = edge_values()
    rng = np.random.default_rng(11)
    pairs = [(sa * a, sb * b) for a in nums for b in dens for sa in (1, -1) for sb in (1, -1) if not (a == 0 and sa < 0)]
    # random operands of the ranges, and numerators next to a multiple of the divisor
    for _ in range(1500):
        b = float(f32(rng.uniform(1, 2) * 2.0 ** int(rng.integers(-30, 30)))) * (1 if rng.integers(2) else -1)
        a = float(f32(rng.uniform(1, 2) * 2.0 ** int(rng.integers(-66, 40)))) * (1 if rng.integers(2) else -1)
        pairs.append((a, b))
        k = int(rng.integers(1, 200))
        near = np.array([f32(k) * f32(b)], f32).view(np.uint32) + np.uint32(rng.integers(0, 3)) - np.uint32(1)
        pairs.append((float(near.view(f32)[0]), b))
    for a, b in pairs:
        got, want = qb.quot_fast_exact(a, b), qb.div_exact(a, b)
        assert got == want, (a, b, float(got), float(want))
        if a != 0:
            assert abs(want) >= Fraction(2) ** -126, "quotients of the proved ranges are normal"
    # a zero numerator takes the divisor's sign under both statements; in float32 arithmetic proper:
    for b in (f32(3.0), f32(-3.0)):
        a = f32(0.0)
        r = f32(1) / b
        q0 = f32(a * r)
        assert np.signbit(q0) == np.signbit(f32(a / b))
    assert len(pairs) > 3000
