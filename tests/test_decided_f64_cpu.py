"""CPU: the lemma behind K1's decided f64 roundings (sdm_device.h decided_sum, SDM_K1_OPT bits 21, 22), restated in NumPy.

    x = (float)((double)c + N / d)   is decided, not divided:   Q = N * y,  y ~ 1/d from one Newton step on a float seed,
    lo = (float)fma(Q, 1 - 2^-40, c),  hi = (float)fma(Q, 1 + 2^-40, c);   lo == hi  =>  x = lo.

float64 / float32 operations are NumPy's (IEEE, round to nearest even); the FMAs, which NumPy lacks, are formed exactly in
fractions.Fraction and rounded once by float().  Every decided result must equal the plain statement's bits; operands built
to land next to a float rounding boundary must be left undecided or be right as well."""
from fractions import Fraction

import numpy as np

f32, f64 = np.float32, np.float64
DELTA = Fraction(1, 1 << 40)


def fma(a, b, c):
    """RN64(a * b + c), one rounding"""
    return f64(float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))))


def decided_sum(c, Q):
    with np.errstate(over="ignore"):  # (beyond the float range both sides are the same infinity)
        lo = f32(fma(Q, float(1 - DELTA), c))
        hi = f32(fma(Q, float(1 + DELTA), c))
    return lo, lo == hi


def newton(d, y0):
    e = fma(-d, y0, 1.0)
    return fma(e, y0, y0)


def step64(x, k):
    """the double k steps above x (bit pattern arithmetic; x finite and non-zero)"""
    return (np.array([x], f64).view(np.int64) + np.int64(k)).view(f64)[0]


def same(a, b):
    return f32(a).view(np.uint32) == f32(b).view(np.uint32)


def ustar_forms(c, g, q, pe, ge, inv_theta, N=None):
    """PM.cc:455, 458 -> (statement as written, decided value, decided?)"""
    gg = f32(g * g)
    denom = f32(f64(gg) + inv_theta * f64(q) * f64(q))
    if N is None:
        N = f64(f32(g * pe)) + inv_theta * f64(q) * f64(ge)
    ref = f32(f64(c) + N / f64(denom))
    y0 = f32(1.0) / denom  # rcp_fast: RN32(1 / denom)
    got, ok = decided_sum(f64(c), N * newton(f64(denom), f64(y0)))
    return ref, got, ok, denom


def test_constants_are_doubles():
    assert Fraction(float(1 - DELTA)) == 1 - DELTA and Fraction(float(1 + DELTA)) == 1 + DELTA


def test_ustar_decided_is_the_statement():
    rng = np.random.default_rng(0x75)
    inv_theta = f64(1.0) / f64(0.23)
    undecided = 0
    n = 30000
    for i in range(n):
        c = f64(rng.integers(1, 639))
        if i & 1:
            g = f32(rng.integers(1, 1025) * 0.125 * rng.choice([-1, 1]))
            q = f32(rng.integers(-4096, 4097) * 0.0625)
            pe = f32(rng.integers(-1020, 1021) * 0.25)
            ge = f32(rng.integers(-4096, 4097) * 0.0625)
        else:
            g, q, pe, ge = [f32(rng.choice([-1, 1]) * 2.0 ** rng.uniform(lo, hi)) for lo, hi in ((-6, 7), (-6, 8), (-4, 8), (-4, 8))]
        ref, got, ok, denom = ustar_forms(c, g, q, pe, ge, inv_theta)
        assert 2.0 ** -30 <= denom < 2.0 ** 30
        if ok:
            assert same(got, ref), (c, g, q, pe, ge)
        else:
            undecided += 1
    assert undecided <= n // 1000, undecided  # the lemma predicts about 8e-6


def test_ustar_next_to_rounding_boundaries():
    """N chosen so that c + N/denom sits within a few double steps of the midpoint of two floats, of k * denom, or is +-0"""
    rng = np.random.default_rng(0x76)
    inv_theta = f64(1.0) / f64(0.23)
    decided = 0
    for i in range(6000):
        c = f64(rng.integers(1, 639))
        g, q = [f32(rng.choice([-1, 1]) * 2.0 ** rng.uniform(-6, 7)) for _ in range(2)]
        denom = ustar_forms(c, g, q, f32(1), f32(1), inv_theta)[3]
        kind = i % 3
        if kind == 0:
            f = f32(f32(c) + f32(rng.choice([-1, 1]) * 2.0 ** rng.uniform(-3, 3)))
            mid = (f64(f) + f64(np.nextafter(f, f32(np.inf)))) / 2
            N = (mid - c) * f64(denom)
        elif kind == 1:
            N = f64(rng.integers(1, 1025)) * f64(denom) * rng.choice([-1, 1])
        else:
            N = f64(rng.choice([0.0, -0.0]))
        steps = int(rng.integers(-4, 5))
        if N != 0:
            N = step64(N, steps)
        ref, got, ok, _ = ustar_forms(c, g, q, f32(1), f32(1), inv_theta, N=f64(N))
        if ok:
            decided += 1
            assert same(got, ref), (c, g, q, N)
    assert decided > 2000  # the zero and k * denom numerators are decided


def test_fusion_chains_with_a_perturbed_seed():
    """20-term GetFusion chains (PM.cc:936-937): both sums decided from one Newton step on v_rcp_f32(sigma * sigma), modelled as
    RN32(1 / RN32(sigma^2)) moved by -2 .. +2 float steps (the instruction is good to 1)"""
    rng = np.random.default_rng(0x77)
    undecided = terms = 0
    for chain in range(600):
        base = 2.0 ** rng.uniform(-4, 2)
        pjsj = rsj = f32(0)
        for t in range(1 + chain % 20):
            rho = f32(base * (1 + 0.01 * rng.uniform(-1, 1)))
            sg = f32(2.0 ** rng.uniform(-15, -4))
            s2 = f64(sg) * f64(sg)
            want_p = f32(f64(pjsj) + f64(rho) / s2)
            want_r = f32(f64(rsj) + f64(1.0) / s2)
            seed = f32(1.0) / f32(sg * sg)
            seed = (np.array([seed], f32).view(np.int32) + np.int32(rng.integers(-2, 3))).view(f32)[0]
            assert abs(1 - Fraction(float(s2)) * Fraction(float(seed))) <= Fraction(1, 1 << 21)  # the premise
            y = newton(s2, f64(seed))
            got_p, ok_p = decided_sum(f64(pjsj), f64(rho) * y)
            got_r, ok_r = decided_sum(f64(rsj), y)
            terms += 1
            if ok_p and ok_r:
                assert same(got_p, want_p) and same(got_r, want_r), (rho, sg, pjsj, rsj)
            else:
                undecided += 1
            pjsj, rsj = want_p, want_r
    assert undecided <= terms // 500, (undecided, terms)


def test_lemma_on_arbitrary_terms():
    """any T within 2^-40 |Q| of Q: lo == hi implies RN32(RN64(c + T)) == lo, for both signs, zero and huge values"""
    rng = np.random.default_rng(0x78)
    decided = 0
    for i in range(20000):
        c = f64(f32(rng.choice([-1, 1]) * 2.0 ** rng.uniform(-20, 20))) if i % 5 else f64(0.0)
        Q = f64(rng.choice([-1, 1]) * 2.0 ** rng.uniform(-60, 60))
        if i % 7 == 0:  # next to the midpoint above a float near c
            f = f32(c + Q)
            Q = (f64(f) + f64(np.nextafter(f, f32(np.inf)))) / 2 - c
        if i % 1000 == 0:
            Q = f64(rng.choice([-1, 1]) * 2.0 ** 200)  # beyond the float range: both sides are the same infinity
        rel = Fraction(int(rng.integers(-(1 << 20), (1 << 20) + 1)), 1 << 60)  # |rel| <= 2^-40
        T = f64(float(Fraction(float(Q)) * (1 + rel)))
        if abs(Fraction(float(T)) - Fraction(float(Q))) > DELTA * abs(Fraction(float(Q))):
            continue  # (the rounding of T pushed it out of the band by half a step)
        lo, ok = decided_sum(c, Q)
        if ok:
            decided += 1
            with np.errstate(over="ignore"):
                assert same(lo, f32(c + T)), (c, Q, T)
    assert decided > 10000
