"""CPU: tests/voxel_np.py (the NumPy statement of sdm_extract_points_voxel's semantics) against a second formulation --
a plain Python dict loop over the points -- on random and crafted clouds, and the redundancy of the golden fixtures the
GPU test relies on."""
import math
import struct

import numpy as np
import pytest

import golden_util as gu
import voxel_np

f32 = np.float32


def _key(s):
    u = struct.unpack("<I", struct.pack("<f", float(s)))[0] if not isinstance(s, int) else s
    return u ^ (0xFFFFFFFF if u >> 31 else 0x80000000)


def dict_merge(xyz, sigma, voxel_size, plain_offsets):
    """the semantics of include/sdm_c.h, point by point"""
    inv = f32(1.0) / f32(voxel_size)
    sig_bits = np.ascontiguousarray(sigma, f32).view(np.uint32)
    best, count, cell_of = {}, {}, []
    for g, p in enumerate(np.asarray(xyz, f32).reshape(-1, 3)):
        cell = []
        for v in p:
            with np.errstate(invalid="ignore", over="ignore"):
                c = float(f32(v) * inv)  # one float32 multiply
            if math.isnan(c) or math.isinf(c) or not (-2.0 ** 20 <= math.floor(c) < 2.0 ** 20):
                cell = None
                break
            cell.append(math.floor(c))
        cell = tuple(cell) if cell is not None else None
        cell_of.append(cell)
        if cell is None:
            continue
        k = (_key(int(sig_bits[g])), g)
        if cell not in best or k < best[cell]:
            best[cell] = k
        count[cell] = count.get(cell, 0) + 1
    kept = [g for g, c in enumerate(cell_of) if c is None or best[c][1] == g]
    rank = {g: k for k, g in enumerate(kept)}
    mult = [1 if cell_of[g] is None else count[cell_of[g]] for g in kept]
    rep = [rank[g] if c is None else rank[best[c][1]] for g, c in enumerate(cell_of)]
    offs = [sum(1 for g in kept if g < o) for o in plain_offsets]
    return np.array(kept, np.int64), np.array(mult, np.int64), np.array(rep, np.int64), np.array(offs, np.int64)


def check(xyz, sigma, voxel, offs):
    a = voxel_np.voxel_merge(xyz, sigma, voxel, offs)
    b = dict_merge(xyz, sigma, voxel, offs)
    for x, y, what in zip(a, b, ("kept", "multiplicity", "representative", "offsets")):
        np.testing.assert_array_equal(x, y, err_msg=what)
    kept, mult, rep, o = a
    assert mult.sum() == len(np.asarray(sigma).reshape(-1)) and (np.diff(kept) > 0).all()
    np.testing.assert_array_equal(rep[kept], np.arange(len(kept)))
    assert o[-1] == len(kept)
    return a


@pytest.mark.parametrize("seed", range(4))
def test_random_clouds(seed):
    rng = np.random.default_rng(seed)
    T = 600
    xyz = rng.uniform(-1, 1, (T, 3)).astype(f32)
    sigma = rng.choice(np.array([0.01, 0.02, 0.05, 0.011], f32), T)  # many ties
    offs = np.sort(np.concatenate([[0, T], rng.integers(0, T + 1, 3)]))
    for voxel in (0.25, 0.3, 0.05, 1e-7, 1000.0):
        kept, mult, _, _ = check(xyz, sigma, voxel, offs)
        if voxel == 1e-7:
            assert len(kept) == T
        if voxel == 1000.0:
            assert len(kept) <= 8
        if voxel == 0.25:
            assert len(kept) < T and mult.max() > 1


def test_crafted_cells():
    v = 0.25  # a power of two: xyz * inv is exact
    big = f32(2.0 ** 20 * v)
    pts = [(-0.25, 0.0, 0.25), (-0.2500001, 0.0, 0.25), (-0.0, 0.0, 0.3), (0.0, -0.0, 0.26),  # faces, -0 / +0
           (-1e-30, 0.1, 0.1), (1e-30, 0.1, 0.1),                                            # either side of zero
           (-big, 0, 0), (np.nextafter(-big, f32(-np.inf)), 0, 0),                             # cell -2^20 and below it
           (np.nextafter(big, f32(0)), 0, 0), (big, 0, 0),                                     # cell 2^20 - 1 and 2^20
           (np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf), (np.nan, 0, 0),                    # never merged, not even equal
           (-big, 0, 0), (np.nextafter(big, f32(0)), 0, 0), (big, 0, 0)]
    xyz = np.array(pts, f32)
    sigma = np.linspace(0.01, 0.02, len(pts)).astype(f32)
    kept, mult, rep, _ = check(xyz, sigma, v, [0, 5, len(pts)])
    c, ok = voxel_np.cells(xyz, v)
    assert list(ok) == [True] * 7 + [False, True, False] + [False] * 4 + [True, True, False]
    assert c[6, 0] == -2.0 ** 20 and c[8, 0] == 2.0 ** 20 - 1 and c[9, 0] == 2.0 ** 20
    assert rep[0] != rep[1] and rep[2] == rep[3] and rep[4] != rep[5]
    assert rep[14] == rep[6] and rep[15] == rep[8] and rep[16] != rep[9] and rep[10] != rep[13]
    assert mult[rep[6]] == 2 and mult[rep[9]] == 1


def test_sigma_order():
    nan_pos = np.array([0x7FC00000], np.uint32).view(f32)[0]
    nan_neg = np.array([0xFFC00000], np.uint32).view(f32)[0]
    ladder = [nan_neg, f32(-np.inf), f32(-1.0), f32(-0.0), f32(0.0), f32(1e-45), f32(0.01), f32(np.inf), nan_pos]
    keys = voxel_np.sigma_key(np.array(ladder, f32)).astype(np.int64)
    assert (np.diff(keys) > 0).all()
    assert [_key(s) for s in ladder] == list(keys)
    xyz = np.zeros((len(ladder), 3), f32) + f32(0.1)
    for perm in (np.arange(len(ladder)), np.arange(len(ladder))[::-1], np.array([4, 3, 8, 0, 1, 2, 5, 6, 7])):
        sig = np.array(ladder, f32)[perm]
        kept, mult, rep, _ = check(xyz, sig, 1.0, [0, len(ladder)])
        assert list(kept) == [int(np.flatnonzero(perm == 0)[0])] and list(mult) == [len(ladder)]
        # without the negative NaN and -Inf .. -1: -0 beats +0
        sub = perm[perm >= 3]
        kept, _, _, _ = check(xyz[:len(sub)], np.array(ladder, f32)[sub], 1.0, [0, len(sub)])
        assert list(kept) == [int(np.flatnonzero(sub == 3)[0])]
    # equal sigmas: the earlier point
    kept, _, _, offs = check(xyz[:6], np.full(6, 0.01, f32), 1.0, [0, 3, 6])
    assert list(kept) == [0] and list(offs) == [0, 1, 1]
    sig = np.full(6, 0.01, f32)
    sig[4] = np.nextafter(f32(0.01), f32(0))
    kept, _, _, offs = check(xyz[:6], sig, 1.0, [0, 3, 6])
    assert list(kept) == [4] and list(offs) == [0, 0, 1]


def _fixture_cloud(g, max_sigma=0.3):
    """the plain cloud of a fixture: chk / sigma through the filter, back-projected with its K and Tcw"""
    fx, fy, cx, cy = [f32(v) for v in g["K"]]
    pts, sig, slot = [], [], []
    for k in range(g["n_kf"]):
        rho, s = g["chk"][k], g["sigma"][k]
        with np.errstate(invalid="ignore"):
            keep = ~(s.astype(np.float64) > max_sigma) & (rho.astype(np.float64) > 1e-6)
        ys, xs = np.nonzero(keep)
        Z = f32(1) / rho[ys, xs]
        cam = np.stack([Z * (xs.astype(f32) - cx) / fx, Z * (ys.astype(f32) - cy) / fy, Z], 1)
        R, t = g["Tcw"][k][:, :3], g["Tcw"][k][:, 3]
        pts.append(((cam - t) @ R).astype(f32))  # Rcw^T (Xc - tcw)
        sig.append(s[ys, xs])
        slot.append(np.full(len(ys), k))
    return np.concatenate(pts), np.concatenate(sig), np.concatenate(slot)


@pytest.mark.parametrize("name", gu.fixture_names())
def test_golden_fixtures_are_redundant_enough(name):
    g = gu.load(name)
    xyz, sigma, slot = _fixture_cloud(g)
    T = len(xyz)
    offs = np.searchsorted(slot, np.arange(g["n_kf"] + 1))
    assert T > 1000
    merged = {v: voxel_np.voxel_merge(xyz, sigma, v, offs) for v in (1e-4, 0.005, 0.02, 1000.0, 1e-7)}
    for kept, mult, rep, o in merged.values():
        assert mult.sum() == T and o[-1] == len(kept)
        np.testing.assert_array_equal(rep[kept], np.arange(len(kept)))
    kept, mult, rep, _ = merged[0.02]
    assert len(kept) < T / 3
    lo, hi = np.full(len(kept), g["n_kf"]), np.full(len(kept), -1)
    np.minimum.at(lo, rep, slot)
    np.maximum.at(hi, rep, slot)
    assert (lo < hi).sum() >= 100  # voxels holding points of more than one keyframe
    assert len(merged[1e-7][0]) == T and (merged[1e-7][1] == 1).all()
    assert len(merged[1000.0][0]) <= 8
    assert len(merged[0.02][0]) < len(merged[0.005][0]) <= len(merged[1e-4][0]) <= T
