"""GPU: K1's reciprocal-form quotients under per-pair operand boxes (sdm_device.h quot_boxes, SDM_K1_OPT bits 18-20).
search_fuse against the oracle, bit for bit, on (a) a geometry whose pairs are all accepted -- checked through
sdm_selftest(12), which counts the pairs of the call that carry the two PairConst::clean bits -- (b) each degenerate geometry
that must be refused, (c) one call that mixes accepted and refused pairs for the same reference keyframe; and
sdm_selftest(11): quot_fast against the division over 2^32 operand pairs of the proved ranges."""
import math

import numpy as np
import pytest

import np_pm
import quot_boxes_np as qb
from common import Sequence, assert_bit_equal

pytestmark = pytest.mark.gpu

W, H, N_KF = 64, 48, 5


@pytest.fixture(scope="module")
def frames(pkg, oracle):
    """five rendered keyframes of the synthetic scene with their derived planes, shared by every case (never modified)"""
    seq = Sequence(pkg, oracle, W, H, N_KF, 0x5EED0B18)
    return seq


def rot(rx, ry, rz):
    cx_, sx_, cy_, sy_, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]])
    Rx = np.array([[1.0, 0, 0], [0, cx_, -sx_], [0, sx_, cx_]])
    Ry = np.array([[cy_, 0, sy_], [0, 1.0, 0], [-sy_, 0, cy_]])
    return Ry @ Rx @ Rz


def pose(Rwc, C):
    Rcw = np.asarray(Rwc, np.float64).T
    return np.concatenate([Rcw, (-Rcw @ np.asarray(C, np.float64))[:, None]], axis=1).astype(np.float32)


class _Kf:
    def __init__(self, K, T):
        self.fx, self.fy, self.cx, self.cy = [np.float32(v) for v in K]
        self.R, self.t = T[:, :3].copy(), T[:, 3].copy()


def expected_bits(seq, K, Ts, refs, nbrs, mind, maxd):
    """pairs of the call that the restatement accepts: (range, sigma / Eq. 8, pairs)"""
    b3 = b4 = n = 0
    for r, nb in zip(refs, nbrs):
        for j in nb:
            p = np_pm.Pair(_Kf(K, Ts[r]), _Kf(K, Ts[j]))
            bits, _ = qb.quot_boxes(p.R21[0], p.R21[2], p.t21[0], p.t21[2], seq.istd[j], K[0], K[1], K[2], K[3], mind, maxd, W, H)
            b3 += bool(bits & 8)
            b4 += bool(bits & 16)
            n += 1
    return b3, b4, n


def run_case(pkg, oracle, seq, Ts, refs, nbrs, mind, maxd):
    """-> (pairs with the range bit, pairs with the sigma / Eq. 8 bit, pairs, pixels fused, hypotheses); maps and the
    hypothesis count checked against the oracle"""
    okf = [oracle.keyframe(seq.im[k], seq.grad[k], seq.theta[k], seq.istd[k], seq.K, Ts[k]) for k in range(N_KF)]
    eng = pkg.Engine(W, H, N_KF, max_neighbours=len(nbrs[0]))
    for k in range(N_KF):
        eng.upload_keyframe(k, seq.im[k], seq.grad[k], seq.theta[k], seq.istd[k], seq.K, Ts[k])
    eng.enable_stats(True)
    eng.get_stats(reset=True)
    eng.search_fuse(refs, nbrs, mind, maxd)
    hyps = eng.get_stats()["hypotheses"]
    packed, pairs = eng.selftest(12)
    fused = want_hyps = 0
    for r, nb in zip(refs, nbrs):
        want_r, want_s, st = oracle.recon_search_fuse(okf[r], [okf[j] for j in nb], None, mind, maxd)
        got_r, got_s = eng.download_depth(r)
        assert_bit_equal(got_r, want_r, "rho kf %d" % r)
        assert_bit_equal(got_s, want_s, "sigma kf %d" % r)
        fused += int((want_r > 1e-6).sum())
        want_hyps += st["hypotheses"]
    eng.close()
    assert hyps == want_hyps
    return packed & 0xFFFFFFFF, packed >> 32, pairs, fused, hyps


def test_accepted_geometry_takes_the_fast_quotients(pkg, oracle, gpu_ok, frames):
    seq = frames
    refs = list(range(N_KF))
    nbrs = [seq.neighbours(k, 4) for k in refs]
    want = expected_bits(seq, seq.K, seq.Tcw, refs, nbrs, seq.min_depth, seq.max_depth)
    assert want == (20, 20, 20), want  # the restatement accepts every pair of the scene
    b3, b4, pairs, fused, _ = run_case(pkg, oracle, seq, seq.Tcw, refs, nbrs, seq.min_depth, seq.max_depth)
    assert (b3, b4, pairs) == want, "every pair of the call must carry both bits on the device too"
    assert fused > 100, "the case must fuse something"


def degenerate_cases(seq):
    """name -> (poses, min_depth, max_depth): every pair of the call must be refused for the search range (and the inputs-only
    cases for Eq. 8 as well)"""
    I = np.eye(3)
    mind, maxd = seq.min_depth, seq.max_depth
    out = {}
    out["pure_rotation"] = ([pose(rot(0.01 * k, -0.02 * k, 0.015 * k), (0, 0, 0)) for k in range(N_KF)], mind, maxd)
    out["baseline_0"] = ([pose(I, (0, 0, 0)) for k in range(N_KF)], mind, maxd)
    # cameras that look sideways against one another and sit one ahead of the other: z_min changes sign inside the image
    out["z_min_crosses_zero"] = ([pose(rot(0, 0.5 * (k % 2), 0), (0.05 * k, 0, 0.9 * (k % 2))) for k in range(N_KF)], mind, maxd)
    out["mind_0"] = (list(seq.Tcw), 0.0, maxd)
    tiny = []
    for k in range(N_KF):  # the scene's camera centres under an "identity" whose (0,1) entry is 1e-30: R21(0,1) = 1e-30
        T = np.concatenate([np.eye(3), np.asarray(seq.Tcw[k])[:, 3:4]], axis=1).astype(np.float32)
        T[0, 1] = np.float32(1e-30)
        tiny.append(T)
    out["entries_1e-30"] = (tiny, mind, maxd)
    return out


@pytest.mark.parametrize("name", ["pure_rotation", "baseline_0", "z_min_crosses_zero", "mind_0", "entries_1e-30"])
def test_refused_geometry_keeps_the_divisions(pkg, oracle, gpu_ok, frames, name):
    seq = frames
    Ts, mind, maxd = degenerate_cases(seq)[name]
    refs = list(range(N_KF))
    nbrs = [[j for j in range(N_KF) if j != k][:4] for k in refs]
    if name == "z_min_crosses_zero":  # pairs of an even and an odd keyframe
        refs, nbrs = [0, 2, 4], [[1, 3], [1, 3], [3, 1]]
    want = expected_bits(seq, seq.K, Ts, refs, nbrs, mind, maxd)
    assert want[0] == 0, (name, want)
    if name != "z_min_crosses_zero":
        assert want[1] == 0, (name, want)
    b3, b4, pairs, _, _ = run_case(pkg, oracle, seq, Ts, refs, nbrs, mind, maxd)
    assert (b3, b4, pairs) == want, name


def test_accepted_and_refused_pairs_in_one_call(pkg, oracle, gpu_ok, frames):
    """keyframes 0 and 3 both sit at the origin (rotated against each other): the pairs (0,3) and (3,0) are pure rotations,
    every other pair of the same references keeps its baseline"""
    seq = frames
    Ts = list(seq.Tcw)
    Rwc, _ = seq.scene.pose(0)
    Ts[0] = pose(Rwc, (0, 0, 0))
    Ts[3] = pose(Rwc @ rot(0.01, -0.01, 0.02), (0, 0, 0))
    refs = [0, 1, 3]
    nbrs = [[1, 3, 2, 4], [4, 0, 2, 3], [0, 1, 2, 4]]
    want = expected_bits(seq, seq.K, Ts, refs, nbrs, seq.min_depth, seq.max_depth)
    assert 0 < want[0] < want[2] and 0 < want[1] < want[2], want
    b3, b4, pairs, _, hyps = run_case(pkg, oracle, seq, Ts, refs, nbrs, seq.min_depth, seq.max_depth)
    assert (b3, b4, pairs) == want
    assert hyps > 500, "the accepted pairs of the call must still produce hypotheses (three per pixel do not fuse: lambdaN)"


def test_quot_fast_over_the_proved_ranges(pkg, gpu_ok):
    eng = pkg.Engine(W, H, 2, max_neighbours=1)
    bad, tested = eng.selftest(11)
    eng.close()
    assert tested == 1 << 32
    assert bad == 0, "%d of %d quotients differ from the division" % (bad, tested)
