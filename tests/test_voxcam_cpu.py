"""CPU: tests/voxcam_np.py (the NumPy statement of sdm_extract_points_voxel_cameras' camera lists) against a second
formulation -- Python sets, point by point -- on random clouds and on the golden fixtures, and how much the merged lists
gain over the winner's own list on those fixtures (computed on the CPU: support_np, voxel_np, the fixture cloud)."""
import functools

import numpy as np
import pytest

import golden_util as gu
import support_np as sn
import voxcam_np
import voxel_np
from test_voxel_cpu import _fixture_cloud

N_SHORT = 3  # the fixtures' full rows name every other keyframe, which hides the gain: the tests use three neighbours


def own_set(word, slot, row):
    """C(g)"""
    return {int(slot)} | {int(row[j]) for j in range(len(row)) if int(word) >> j & 1}


def set_lists(support, plain_offsets, slots, nbrs, rep, M):
    """the semantics of include/sdm_c.h, point by point"""
    cams = [set() for _ in range(M)]
    i = 0
    for g, w in enumerate(support):
        while g >= plain_offsets[i + 1]:
            i += 1
        cams[int(rep[g])] |= own_set(w, slots[i], nbrs[i])
    return [sorted(c) for c in cams]


def check(support, plain_offsets, slots, nbrs, rep, M):
    offs, cs = voxcam_np.voxel_cameras(support, plain_offsets, slots, nbrs, rep, M)
    assert offs.dtype == np.int64 and cs.dtype == np.int32
    assert offs[0] == 0 and offs[-1] == len(cs) and len(offs) == M + 1
    got = voxcam_np.lists(offs, cs)
    assert got == set_lists(support, plain_offsets, slots, nbrs, rep, M)
    assert all(len(c) >= 1 and all(a < b for a, b in zip(c, c[1:])) for c in got)
    return got


@pytest.mark.parametrize("seed", range(4))
def test_random_clouds(seed):
    rng = np.random.default_rng(seed)
    n, n_nbr, T, M = 5, (3, 7, 40, 64)[seed], 700, (1, 60, 300, 700)[seed]
    ids = rng.permutation(400)[:90]  # scattered slot ids: slot id != camera index
    slots = ids[:n]
    nbrs = rng.choice(ids, (n, n_nbr))  # repeated neighbours, and some equal to a row's own slot
    nbrs[1, 0] = slots[1]
    nbrs[2, -1] = nbrs[2, 0]
    plain_offsets = np.sort(np.concatenate([[0, T], rng.integers(0, T + 1, n - 1)]))  # (empty slots happen)
    mask = np.uint64((1 << n_nbr) - 1)
    support = rng.integers(0, 2 ** 63, T, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, T, dtype=np.uint64)
    support &= rng.integers(0, 2 ** 63, T, dtype=np.uint64) * np.uint64(2) + np.uint64(1)  # a quarter of the bits
    support &= mask
    support[rng.random(T) < 0.2] = 0  # zero words: the list is the own slot alone if nothing else joins
    rep = rng.integers(0, M, T)
    rep[rng.permutation(T)[:M]] = np.arange(M)  # every kept point stands for someone
    got = check(support, plain_offsets, slots, nbrs, rep, M)
    if M == T:  # nothing merged: every list is its point's own C(g)
        row_of = np.searchsorted(plain_offsets[1:], np.arange(T), side="right")
        for g in range(T):
            assert got[rep[g]] == sorted(own_set(support[g], slots[row_of[g]], nbrs[row_of[g]]))
    if M == 1:
        assert len(got[0]) > n_nbr + 1


@functools.lru_cache(maxsize=None)
def fixture_case(name):
    """(g, xyz, sigma, plain_offsets, support words of the plain points for the short rows, the short rows)"""
    g = gu.load(name)
    xyz, sigma, slot = _fixture_cloud(g)
    offs = np.searchsorted(slot, np.arange(g["n_kf"] + 1))
    rows = np.stack([g["nbrs"][k][:N_SHORT] for k in range(g["n_kf"])])
    words = []
    for k in range(g["n_kf"]):
        with np.errstate(invalid="ignore"):
            keep = ~(g["sigma"][k].astype(np.float64) > 0.3) & (g["chk"][k].astype(np.float64) > 1e-6)  # _fixture_cloud's
        words.append(sn.fixture_support(g, k, nbr_row=rows[k])[1][keep])
    return g, xyz, sigma, offs, np.concatenate(words), rows


@pytest.mark.parametrize("name", gu.fixture_names())
def test_golden_fixtures_gain_cameras(name):
    g, xyz, sigma, offs, support, rows = fixture_case(name)
    T, refs = len(xyz), np.arange(g["n_kf"])
    assert len(support) == T > 1000
    row_of = np.searchsorted(offs[1:], np.arange(T), side="right")
    for voxel in (0.02, 1e-7, 1000.0):
        kept, _, rep, _ = voxel_np.voxel_merge(xyz, sigma, voxel, offs)
        M = len(kept)
        got = check(support, offs, refs, rows, rep, M)
        own = [sorted(own_set(support[q], row_of[q], rows[row_of[q]])) for q in kept]
        assert all(set(o) <= set(c) for o, c in zip(own, got))
        if voxel == 0.02:
            gained = sum(len(c) > len(o) for o, c in zip(own, got))
            beyond = sum(len(c) > N_SHORT + 1 for c in got)
            print("%s: M %d, %d kept points gain a camera, %d hold more than %d" % (name, M, gained, beyond, N_SHORT + 1))
            assert gained >= 500  # 577 .. 779 on the four fixtures
            assert beyond >= 500  # no single support word can express these
        if voxel == 1e-7:
            assert M == T and got == own
        if voxel == 1000.0:
            assert M <= 8
