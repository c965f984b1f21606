"""CPU: tests/support_np.py (the NumPy restatement of PM.cc:659-765 that also keeps WHICH neighbours were counted) against
the golden fixtures: its checked rho is the oracle's `chk` bit for bit, and its words reproduce the check's decisions."""
import numpy as np
import pytest

import golden_util as gu
import support_np as sn
from common import bits
from np_pm import LAMBDA_N


@pytest.fixture(scope="module", params=gu.fixture_names())
def restated(request):
    g = gu.load(request.param)
    return g, [sn.fixture_support(g, k) for k in range(g["n_kf"])]


def test_checked_rho_is_the_fixtures(restated):
    g, res = restated
    for k, (chk, _) in enumerate(res):
        np.testing.assert_array_equal(bits(chk), bits(g["chk"][k]), err_msg="keyframe %d" % k)


def test_words_reproduce_the_decisions(restated):
    g, res = restated
    H, W, n = g["H"], g["W"], g["n"]
    inset = np.zeros((H, W), bool)
    inset[2:H - 2, 2:W - 2] = True
    pcs, masks, points = [], set(), 0
    for k, (chk, words) in enumerate(res):
        with np.errstate(invalid="ignore"):
            live = inset & ~(g["rho"][k].astype(np.float64) < 0.000001)  # inset and not skipped by PM.cc:662
        pc = sn.popcount(words)
        assert not (words[~live] != 0).any()
        assert not (words >> np.uint64(n)).any()
        # popcount < lambdaN => checked rho == 0, and checked rho != 0 => popcount >= lambdaN: zero exceptions
        assert not (live & (pc < LAMBDA_N) & (chk != 0)).any()
        assert not (live & (chk != 0) & (pc < LAMBDA_N)).any()
        with np.errstate(invalid="ignore"):
            keep = ~(g["sigma"][k].astype(np.float64) > 0.3) & (chk.astype(np.float64) > 0.000001)
        points += int(keep.sum())
        pcs.append(pc[keep])
        masks |= set(int(w) for w in words[keep])
    pcs = np.concatenate(pcs)
    # the extracted points (sigma <= 0.3) carry lists worth testing: all confirmed, not all by everybody
    assert points > 0 and pcs.min() >= LAMBDA_N and pcs.max() == n and len(masks) > 1 and len(set(pcs)) > 1


def test_abi_symbol_and_null_arguments(pkg):
    """sdm_extract_points_support is exported, mirrored in ctypes, and refuses null arguments without a GPU"""
    import ctypes
    import sys
    lib = pkg.load_library()
    b = sys.modules[pkg.__name__ + ".binding"]
    assert hasattr(ctypes.CDLL(pkg.lib_path()), "sdm_extract_points_support")
    assert "sdm_extract_points_support" in {s[0] for s in b.SYMBOLS}
    assert ctypes.sizeof(b.PointBuffers) == 48  # the new array is a separate argument: the struct keeps its layout
    pb = b.PointBuffers()
    offs = (ctypes.c_longlong * 2)()
    slots, nbrs = (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(1)
    sup = (ctypes.c_ulonglong * 1)()
    f = lib.sdm_extract_points_support
    assert f(None, 1, slots, 1, nbrs, 1, 0.01, 1e-6, ctypes.byref(pb), sup, offs) == 1  # SDM_EINVAL
    assert f(None, 1, slots, 1, nbrs, 1, 0.01, 1e-6, None, None, None) == 1
