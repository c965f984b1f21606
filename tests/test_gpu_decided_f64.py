"""GPU: K1's decided f64 roundings (sdm_device.h decided_sum, SDM_K1_OPT bits 21-23): the refinement's ustar (PM.cc:458),
GetFusion's two running sums (PM.cc:936-937) and its result pjsj / rsj, sqrtf(1 / rsj) (PM.cc:225-226).

sdm_selftest(13), (14), (15) compare the device functions with the statements as written: no result may differ, and of the
draws INSIDE the operand windows at most 1e-4 may be handed back to the statement (a condition, not a report: a form that
sends everything to its fallback would pass the comparison trivially; the lemma predicts about 8e-6).  End to end, against
the oracle and bit for bit: fuse() on vectors of 2, 4 and 20 hypotheses, epipolar_search() on an accepted and on a refused
pair, and one search_fuse() of three 64x48 keyframes."""
import numpy as np
import pytest

from common import Sequence, assert_bit_equal

pytestmark = pytest.mark.gpu

W, H, N_KF = 64, 48, 5
# draws inside the operand windows per self-test (sdm_c.h; sdm_kernels.h ST_DEC_BLOCKS x BLOCK x ST1x_ITERS)
IN_PREMISE = {13: 1 << 27, 14: 1024 * 256 * 6 * 210, 15: 1 << 28}
MAX_UNDECIDED_SHARE = 1e-4


@pytest.fixture(scope="module")
def frames(pkg, oracle):
    """five rendered 64x48 keyframes with their derived planes, shared by the cases below (never modified)"""
    return Sequence(pkg, oracle, W, H, N_KF, 0x5EED0D64)


@pytest.mark.parametrize("which", [13, 14, 15])
def test_decided_forms_against_the_statements(pkg, gpu_ok, which):
    eng = pkg.Engine(W, H, 2, max_neighbours=1)
    bad, undecided = eng.selftest(which)
    eng.close()
    share = undecided / IN_PREMISE[which]
    print("selftest %d: %d differ, %d of %d undecided (%.3g)" % (which, bad, undecided, IN_PREMISE[which], share))
    assert bad == 0, "%d results differ from the reference statement" % bad
    assert share <= MAX_UNDECIDED_SHARE, "%d of %d draws inside the premise were not decided" % (undecided, IN_PREMISE[which])


def fuse_cases():
    f32 = np.float32
    rng = np.random.default_rng(0xD64)
    out = {}
    out["2_below_lambdaN"] = (f32([1.0, 1.001]), f32([0.01, 0.012]))
    out["4_agree"] = (f32([0.5, 0.5004, 0.4997, 0.5001]), f32([0.004, 0.0051, 0.0037, 0.0045]))
    # sigma log-uniform over [2^-15, 2^-4), rho within 1 % of its base
    sg = np.exp2(rng.uniform(-15, -4, 20)).astype(f32)
    out["20_agree"] = ((0.75 * (1 + 0.01 * rng.uniform(-1, 1, 20))).astype(f32), np.maximum(sg, f32(0.02)).astype(f32))
    out["20_mixed_sigma"] = ((0.75 * (1 + 1e-5 * rng.uniform(-1, 1, 20))).astype(f32), sg)
    # an open pixel: two clusters, neither settles the other, the larger one first in neither order
    rho = np.where(np.arange(20) % 3 == 0, 1.3, 0.8) * (1 + 0.002 * rng.uniform(-1, 1, 20))
    out["20_two_clusters"] = (rho.astype(f32), f32([0.01] * 20))
    # sigma outside [2^-50, 2^50): the terms take the statement as written
    out["4_sigma_tiny"] = (f32([1.0, 1.0, 1.0, 1.0]), f32([1e-20, 2e-20, 1e-20, 3e-20]))
    out["4_sigma_huge"] = (f32([1.0, 1.5, 0.7, 1.2]), f32([1e16, 2e16, 1e16, 3e16]))
    out["4_sigma_window_ends"] = (f32([1.0, 1.0, 1.0, 1.0]), f32([2.0 ** -50, 2.0 ** -50, np.nextafter(f32(2.0 ** -50), f32(0)), 1e-15]))
    out["4_sigma_zero_inf"] = (f32([1, 1, 1, 1, 1]), f32([0.1, 0, 0.1, 0.1, np.inf]))
    out["5_nan"] = (f32([1, np.nan, 1, 1, 1]), f32([0.1, 0.1, 0.1, np.nan, 0.1]))
    # sum of 1/sigma^2 beyond the result's operand window (2^41): the quotient and the root as written
    out["4_sum_beyond_window"] = (f32([0.5, 0.5, 0.5, 0.5]), f32([2.0 ** -21] * 4))
    out["4_rho_zero"] = (f32([0.0, 0.0, 0.0, 0.0]), f32([0.01] * 4))
    out["4_rho_negative"] = (f32([-0.5, -0.5, -0.5, -0.5]), f32([0.01] * 4))
    return out


@pytest.mark.parametrize("name", sorted(fuse_cases()))
def test_fuse_against_the_oracle(pkg, oracle, gpu_ok, name):
    rho, sig = fuse_cases()[name]
    eng = pkg.Engine(W, H, 2, max_neighbours=32)
    got = eng.fuse(rho, sig)
    eng.close()
    ref = oracle.fuse(rho, sig)
    assert got[2] == ref[2], (name, got, ref)
    assert_bit_equal(np.array(got[:2]), np.array(ref[:2]), name)
    if name == "2_below_lambdaN":
        assert ref[2] == 0
    if name in ("4_agree", "20_agree", "20_mixed_sigma", "20_two_clusters"):
        assert ref[2] == 1, name


@pytest.mark.parametrize("mind", ["scene", "zero"])
def test_epipolar_search_accepted_and_refused_pair(pkg, oracle, gpu_ok, frames, mind):
    """min_depth = 0 makes quot_boxes refuse the pair (no denom window: ustar as written); the scene's own bounds accept it"""
    seq = frames
    mn = seq.min_depth if mind == "scene" else 0.0
    eng = pkg.Engine(W, H, N_KF, max_neighbours=4)
    seq.upload(eng)
    ys, xs = np.nonzero(seq.grad[1][2:-2, 2:-2] >= 8)
    pick = np.random.default_rng(5).choice(len(xs), min(80, len(xs)), replace=False)
    n_sup = 0
    for i in pick:
        x, y = int(xs[i]) + 2, int(ys[i]) + 2
        got = eng.epipolar_search(1, 2, x, y, mn, seq.max_depth)
        ref = oracle.epipolar_search(seq.okf[1], seq.okf[2], x, y, mn, seq.max_depth)
        assert got["supported"] == ref["supported"]
        for key in ("rho", "sigma", "best_u", "best_v"):
            assert_bit_equal(np.array([got[key]]), np.array([ref[key]]), "%s at %d,%d" % (key, x, y))
        n_sup += got["supported"]
    eng.close()
    assert n_sup > 10, "the case must produce hypotheses"


def test_search_fuse_three_keyframes(pkg, oracle, gpu_ok, frames):
    seq = frames
    refs = [0, 2, 4]
    nbrs = [seq.neighbours(k, 4) for k in refs]
    eng = pkg.Engine(W, H, N_KF, max_neighbours=4)
    seq.upload(eng)
    eng.search_fuse(refs, nbrs, seq.min_depth, seq.max_depth)
    fused = 0
    for r, nb in zip(refs, nbrs):
        want_r, want_s, _ = oracle.recon_search_fuse(seq.okf[r], [seq.okf[j] for j in nb], None, seq.min_depth, seq.max_depth)
        got_r, got_s = eng.download_depth(r)
        assert_bit_equal(got_r, want_r, "rho kf %d" % r)
        assert_bit_equal(got_s, want_s, "sigma kf %d" % r)
        fused += int((want_r > 1e-6).sum())
    eng.close()
    assert fused > 100, "the case must fuse something"
