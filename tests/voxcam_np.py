"""NumPy restatement of sdm_extract_points_voxel_cameras' camera lists (include/sdm_c.h): per kept point of the merged
cloud, the cameras that saw the plain points it stands for.

  C(g) = {slots[i(g)]} | {nbrs[i(g)][j] : bit j of support[g]}   (i(g): the call row of plain point g's slot)
  V(k) = union of C(g) over representative[g] == k, as slot ids in ascending order without duplicates

Vectorised: a boolean matrix [M, Cn] over the sorted camera table (the distinct slots of the call), set column by column
of the neighbour table -- the only Python loop runs over n_nbr, never over points."""
import numpy as np


def camera_table(slots, nbrs):
    """the distinct slots among slots and nbrs, ascending"""
    return np.unique(np.concatenate([np.asarray(slots, np.int64).reshape(-1), np.asarray(nbrs, np.int64).reshape(-1)]))


def voxel_cameras(support, plain_offsets, slots, nbrs, representative, M):
    """support uint64[T], plain_offsets [n+1], slots [n], nbrs [n, n_nbr], representative [T] (values < M)
    -> (cam_offsets int64[M+1], cam_slots int32[E])"""
    support = np.asarray(support, np.uint64).reshape(-1)
    T = len(support)
    slots = np.asarray(slots, np.int64).reshape(-1)
    nbrs = np.asarray(nbrs, np.int64).reshape(len(slots), -1)
    rep = np.asarray(representative).astype(np.int64).reshape(-1)
    assert len(rep) == T and int(np.asarray(plain_offsets)[-1]) == T
    table = camera_table(slots, nbrs)
    row_of = np.searchsorted(np.asarray(plain_offsets, np.int64)[1:], np.arange(T), side="right")  # i(g)
    hit = np.zeros((int(M), len(table)), bool)
    hit[rep, np.searchsorted(table, slots)[row_of]] = True  # the observing keyframe, whatever the word
    nbr_cam = np.searchsorted(table, nbrs)
    for j in range(nbrs.shape[1]):
        sel = np.flatnonzero((support >> np.uint64(j)) & np.uint64(1))
        hit[rep[sel], nbr_cam[row_of[sel], j]] = True
    cam_offsets = np.zeros(int(M) + 1, np.int64)
    np.cumsum(hit.sum(axis=1), out=cam_offsets[1:])
    cam_slots = table[np.nonzero(hit)[1]].astype(np.int32)  # row-major: kept points in order, ascending slot id within
    return cam_offsets, cam_slots


def lists(cam_offsets, cam_slots):
    """[list of slot ids] per kept point (small clouds only)"""
    o = np.asarray(cam_offsets, np.int64)
    return [np.asarray(cam_slots[o[k]:o[k + 1]]).tolist() for k in range(len(o) - 1)]
