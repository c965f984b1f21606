"""NumPy restatement of sdm_device.h quot_boxes: the per-pair operand boxes behind K1's reciprocal-form quotients
(SDM_K1_OPT bits 18-20), float32 statement by statement, plus an exact (fractions.Fraction) model of quot_fast.

quot_boxes() returns the clean bits the device sets (8: search range, 16 | E << 8: sigma and Eq. 8 for lanes whose denom lies in
[2^E, 2^30)) and the boxes it evaluated, so that a test can check soundness by containment."""
from fractions import Fraction

import numpy as np

f32 = np.float32
DIV_LO, DIV_HI, NUM_LO, NUM_HI = f32(2.0 ** -30), f32(2.0 ** 30), f32(2.0 ** -66), f32(2.0 ** 40)
U_SPAN = f32(4)
DWIN_END_EXP = 157
_OUT_REL, _OUT_ABS = f32(2.0 ** -20), f32(2.0 ** -100)


def _out(lo, hi):
    lo, hi = f32(lo), f32(hi)
    return (f32(f32(lo - f32(abs(lo) * _OUT_REL)) - _OUT_ABS), f32(f32(hi + f32(abs(hi) * _OUT_REL)) + _OUT_ABS))


def _pt(v):
    return (f32(v), f32(v))


def _neg(a):
    return (f32(-a[1]), f32(-a[0]))


def _add(a, b):
    return _out(f32(a[0] + b[0]), f32(a[1] + b[1]))


def _mul(a, b):
    p = [f32(a[0] * b[0]), f32(a[0] * b[1]), f32(a[1] * b[0]), f32(a[1] * b[1])]
    return _out(min(p), max(p))


def _mag_hi(a):
    return max(abs(a[0]), abs(a[1]))


def _divisor_ok(a):
    return bool((a[0] > 0 or a[1] < 0) and min(abs(a[0]), abs(a[1])) >= DIV_LO and _mag_hi(a) <= DIV_HI)


def input_ok(v):
    u = int(np.array([v], f32).view(np.uint32)[0])
    mag = u & 0x7FFFFFFF
    return u == 0 or ((127 - 36) << 23) <= mag <= ((127 + 20) << 23)


def quot_boxes(Rx, Rz, tx, tz, istd, fx, fy, cx, cy, mind, maxd, W, H):
    """-> (bits, boxes); boxes is {} when the inputs themselves are refused"""
    Rx, Rz = [f32(v) for v in Rx], [f32(v) for v in Rz]
    tx, tz, istd, fx, fy, cx, cy, mind, maxd = [f32(v) for v in (tx, tz, istd, fx, fy, cx, cy, mind, maxd)]
    ok = all(input_ok(v) for v in (tx, tz, cx, cy, fx, fy, mind, maxd)) and all(input_ok(v) for v in Rx + Rz)
    ok = ok and fx > 0 and fy > 0 and mind > 0 and maxd > 0 and tx != 0 and 2 <= W <= 65536 and 2 <= H <= 65536
    if not ok:
        return 0, {}
    with np.errstate(all="ignore"):
        xp0 = _out(f32(f32(0) - cx) / fx, f32(f32(W - 1) - cx) / fx)
        xp1 = _out(f32(f32(0) - cy) / fy, f32(f32(H - 1) - cy) / fy)
        rxxp = _add(_add(_mul(_pt(Rx[0]), xp0), _mul(_pt(Rx[1]), xp1)), _pt(Rx[2]))
        rzxp = _add(_add(_mul(_pt(Rz[0]), xp0), _mul(_pt(Rz[1]), xp1)), _pt(Rz[2]))
        boxes = dict(xp0=xp0, xp1=xp1, rxxp=rxxp, rzxp=rzxp)
        bits = 0
        good = bool(f32(f32(f32(fx * f32(2.0 ** -25)) * abs(tx)) * f32(1 - 2.0 ** -20)) >= NUM_LO)
        for name, d in (("min", mind), ("max", maxd)):
            xk = _add(_mul(rxxp, _pt(d)), _pt(tx))
            zk = _add(_mul(rzxp, _pt(d)), _pt(tz))
            nk = _mul(_pt(fx), xk)
            boxes["x_" + name], boxes["z_" + name], boxes["fxx_" + name] = xk, zk, nk
            good = good and _divisor_ok(zk) and bool(_mag_hi(nk) <= NUM_HI)
        if good:
            bits |= 8
        w = f32(W)
        ucx = _add((f32(-U_SPAN * w), f32(f32(U_SPAN + f32(1)) * w)), _pt(-cx))
        num = _add(_mul(rzxp, ucx), _neg(_mul(_pt(fx), rxxp)))
        den = _add(_mul(_pt(-tz), ucx), _mul(_pt(fx), _pt(tx)))
        boxes["ucx"], boxes["num"], boxes["den"] = ucx, num, den
        nvar = f32(f32(f32(2) * istd) * istd)
        lb = f32(min(f32(f32(f32(2.0 ** -50) * fx) * abs(Rx[2])), f32(f32(rzxp[0] * f32(2.0 ** -25)) * abs(cx))) * f32(1 - 2.0 ** -20))
        good = (_divisor_ok(den) and bool(_mag_hi(num) <= NUM_HI) and Rx[2] != 0 and cx != 0 and bool(rzxp[0] >= f32(2.0 ** -10)) and
                bool(lb >= NUM_LO) and input_ok(istd) and istd > 0 and bool(NUM_LO <= nvar <= NUM_HI))
        root = f32(f32(f32(f32(1002) + f32(f32(1.4143) * istd)) / f32(U_SPAN * w)) * f32(1 + 2.0 ** -10))
        eb = max((int(np.array([f32(root * root)], f32).view(np.uint32)[0]) >> 23) + 1, 97)
        good = good and eb < DWIN_END_EXP
        boxes["eb"] = eb
        if good:
            bits |= 16 | (eb << 8)
    return bits, boxes


# ---- exact model of quot_fast ---------------------------------------------------------------------------------------------
def rn32(x):
    """a Fraction rounded to the nearest float32 (ties to even, gradual underflow), as a Fraction; no overflow handling"""
    if x == 0:
        return Fraction(0)
    s, a = (1 if x > 0 else -1), abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1  # 2^e <= a < 2^(e+1)
    q = max(e - 23, -149)
    return s * round(a / Fraction(2) ** q) * Fraction(2) ** q


def quot_fast_exact(a, b):
    """quot_fast(a, b, rcp_fast(b)) with every step correctly rounded (rcp_fast delivers RN(1/b): sdm_selftest(6))"""
    a, b = Fraction(float(a)), Fraction(float(b))
    r = rn32(1 / b)
    q0 = rn32(a * r)
    e0 = rn32(a - q0 * b)
    q1 = rn32(q0 + e0 * r)
    e1 = rn32(a - q1 * b)
    return rn32(q1 + e1 * r)


def div_exact(a, b):
    return rn32(Fraction(float(a)) / Fraction(float(b)))
