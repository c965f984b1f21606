"""Covisibility weights and SemiDenseRecon's neighbour choice, restated in Python from the reference's text
(KeyFrame::UpdateConnections, KeyFrame.cc:289-361; the neighbour loop of SemiDenseRecon, PM.cc:151-160).  The expected
value of tests/test_gpu_covis.py; tests/test_covis_cpu.py checks it against a second formulation.

`ids` maps a slot to its keyframe's map-point ids as uploaded (int array; < 0 = the keypoint has no map point).  The
angles play no part: UpdateConnections counts every map point of the keyframe.

The one normative choice: the reference sorts pair<int, KeyFrame*> and so orders equal weights by pointer value; here
equal weights keep the order of `cands`."""
import numpy as np

MIN_WEIGHT = 15  # th, KeyFrame.cc:330


def counters(ids, refs, cands):
    """per reference a dict {candidate slot: shared map points}, built as KeyFrame.cc:302-320 builds KFcounter: for every
    map point of the keyframe, every other keyframe that observes it is counted once"""
    observers = {}  # MapPoint::GetObservations(): map point id -> the candidate keyframes that see it
    for c in cands:
        for mp in set(int(x) for x in ids[c] if x >= 0):
            observers.setdefault(mp, []).append(c)
    out = []
    for r in refs:
        counter = {}
        for mp in set(int(x) for x in ids[r] if x >= 0):
            for c in observers.get(mp, ()):
                if c == r:  # KeyFrame.cc:316
                    continue
                counter[c] = counter.get(c, 0) + 1
        out.append(counter)
    return out


def weights(ids, refs, cands):
    """int32 [n_ref, n_cand]"""
    w = np.zeros((len(refs), len(cands)), np.int32)
    for a, counter in enumerate(counters(ids, refs, cands)):
        for b, c in enumerate(cands):
            w[a, b] = counter.get(c, 0)
    return w


def connected(row, min_weight=MIN_WEIGHT):
    """positions in cands of one reference's connected keyframes, in order (KeyFrame.cc:323-361), from its weights"""
    if not any(w > 0 for w in row):  # KeyFrame.cc:323: the counter is empty
        return []
    pairs = [(int(w), pos) for pos, w in enumerate(row) if w >= min_weight]
    if not pairs:  # KeyFrame.cc:348-352: the keyframe with the largest weight, the earliest among equals
        best = max(range(len(row)), key=lambda pos: (int(row[pos]), -pos))
        return [best]
    pairs.sort(key=lambda p: (-p[0], p[1]))  # by weight descending, position ascending
    return [pos for _, pos in pairs]


def neighbours(ids, refs, cands, n, min_weight=MIN_WEIGHT):
    """(nbr_slots [n_ref, n] padded with -1, nbr_weights [n_ref, n] padded with 0, counts [n_ref]), int32: the first n
    connected keyframes of every reference (PM.cc:151-159)"""
    w = weights(ids, refs, cands)
    nbrs = np.full((len(refs), n), -1, np.int32)
    nw = np.zeros((len(refs), n), np.int32)
    cnt = np.zeros(len(refs), np.int32)
    for a in range(len(refs)):
        order = connected(w[a], min_weight)[:n]
        cnt[a] = len(order)
        for j, pos in enumerate(order):
            nbrs[a, j] = cands[pos]
            nw[a, j] = w[a, pos]
    return nbrs, nw, cnt
