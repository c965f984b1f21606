"""NumPy restatement of sdm_extract_points_voxel's semantics (include/sdm_c.h): one point per voxel of a plain cloud.

  inv = float32(1) / float32(voxel_size); cell = floor(xyz * inv) in float32; mergeable iff -2^20 <= cell < 2^20 for all
  three coordinates (NaN, +-Inf fail); within a voxel the kept point minimises (key(sigma), g); an unmergeable point is kept
  with multiplicity 1 and represents itself; the kept points come in plain order."""
import numpy as np

LIM = np.float32(2.0 ** 20)


def sigma_key(sigma):
    """order-preserving map of float32 bit patterns to uint32: u ^ (0xFFFFFFFF if sign else 0x80000000)"""
    u = np.ascontiguousarray(sigma, dtype=np.float32).view(np.uint32)
    return u ^ np.where(u >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def cells(xyz, voxel_size):
    """(float32 cells [T,3], mergeable [T])"""
    inv = np.float32(1.0) / np.float32(voxel_size)
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.floor(np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3) * inv)
        ok = ((c >= -LIM) & (c < LIM)).all(axis=1)
    return c, ok


def voxel_merge(xyz, sigma, voxel_size, plain_offsets):
    """-> kept plain indices [M] (increasing), multiplicity [M], representative [T], offsets [n+1] of the kept points"""
    c, ok = cells(xyz, voxel_size)
    T = len(c)
    g = np.arange(T, dtype=np.int64)
    winner = g.copy()   # the plain index kept for each point (unmergeable: itself)
    count = np.ones(T, np.int64)
    if ok.any():
        gm = g[ok]
        # the integer triple packed into one int64 (21 bits per biased cell: the same partition as np.unique(axis=0) over
        # the three columns), then one sort by (voxel, key(sigma), g): each voxel's first entry is its winner
        ci = c[ok].astype(np.int64) + (1 << 20)
        vox = (ci[:, 0] << 42) | (ci[:, 1] << 21) | ci[:, 2]
        key_g = (sigma_key(np.asarray(sigma, np.float32).reshape(-1)[ok]).astype(np.uint64) << np.uint64(32)) | gm.astype(np.uint64)
        order = np.lexsort((key_g, vox))
        vs, gs = vox[order], gm[order]
        first = np.ones(len(order), bool)
        first[1:] = vs[1:] != vs[:-1]
        start = np.flatnonzero(first)
        vid = np.cumsum(first) - 1  # voxel number of each sorted entry
        winner[gs] = gs[start][vid]
        count[gs] = np.diff(np.append(start, len(order)))[vid]
    kept = np.flatnonzero(winner == g)
    rank = np.full(T, -1, np.int64)
    rank[kept] = np.arange(len(kept))
    offsets = np.searchsorted(kept, np.asarray(plain_offsets, np.int64), side="left").astype(np.int64)
    return kept, count[kept], rank[winner], offsets
