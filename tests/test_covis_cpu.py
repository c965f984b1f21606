"""CPU: tests/covis_np.py (the expected value of the device's covisibility calls) against a second, independent
formulation -- np.intersect1d per pair, np.lexsort for the order -- and on hand-made cases of every rule."""
import numpy as np

import covis_np


def weights2(ids, refs, cands):
    w = np.zeros((len(refs), len(cands)), np.int32)
    for a, r in enumerate(refs):
        x = np.unique(np.asarray(ids[r])[np.asarray(ids[r]) >= 0])
        for b, c in enumerate(cands):
            if c == r:
                continue
            y = np.unique(np.asarray(ids[c])[np.asarray(ids[c]) >= 0])
            w[a, b] = np.intersect1d(x, y).size
    return w


def neighbours2(w, cands, n, min_weight):
    nbrs = np.full((w.shape[0], n), -1, np.int32)
    nw = np.zeros((w.shape[0], n), np.int32)
    cnt = np.zeros(w.shape[0], np.int32)
    pos = np.arange(w.shape[1])
    for a in range(w.shape[0]):
        order = np.lexsort((pos, -w[a].astype(np.int64)))  # last key first: weight descending, then position ascending
        keep = order[w[a][order] >= min_weight]
        if keep.size == 0 and w[a].max() >= 1:
            keep = order[:1]
        keep = keep[:n]
        cnt[a] = keep.size
        nbrs[a, :keep.size] = np.asarray(cands)[keep]
        nw[a, :keep.size] = w[a][keep]
    return nbrs, nw, cnt


def test_restatement_against_second_formulation():
    rng = np.random.default_rng(0xC0715)
    for trial in range(12):
        n_kf = int(rng.integers(2, 40))
        pool = int(rng.choice([40, 300, 3000]))
        ids = []
        for _ in range(n_kf):
            s = int(rng.choice([0, 1, 2, 7, 30, min(pool, 200)]))
            x = rng.choice(pool, s, replace=False).astype(np.int32)
            neg = rng.uniform(0, 1, s) < 0.1
            x[neg] = -rng.integers(1, 5, int(neg.sum()))
            ids.append(x)
        cands = [int(c) for c in rng.permutation(n_kf)[: int(rng.integers(1, n_kf + 1))]]
        refs = [int(r) for r in rng.permutation(n_kf)[: int(rng.integers(1, n_kf + 1))]]
        w = covis_np.weights(ids, refs, cands)
        assert np.array_equal(w, weights2(ids, refs, cands)), trial
        for n in (1, 3, 7, 20):
            for mw in (1, 2, 15, 1000):
                got = covis_np.neighbours(ids, refs, cands, n, mw)
                want = neighbours2(w, cands, n, mw)
                for g, x, what in zip(got, want, ("slots", "weights", "counts")):
                    assert np.array_equal(g, x), (trial, n, mw, what)


def test_all_below_threshold_gives_the_single_fallback():
    ids = {0: [1, 2, 3, 4], 1: [1, 2, 9], 2: [1, 2, 3], 3: [3, 4, 5], 4: [7]}
    nbrs, w, cnt = covis_np.neighbours(ids, [0], [1, 2, 3, 4], 3, 15)
    assert cnt[0] == 1 and list(nbrs[0]) == [2, -1, -1] and list(w[0]) == [3, 0, 0]
    # the largest weight twice: the earlier position
    nbrs, w, cnt = covis_np.neighbours(ids, [0], [4, 3, 1, 2], 3, 15)
    assert cnt[0] == 1 and list(nbrs[0]) == [2, -1, -1]
    ids[1] = [1, 2, 3]
    nbrs, w, cnt = covis_np.neighbours(ids, [0], [4, 3, 1, 2], 3, 15)
    assert cnt[0] == 1 and list(nbrs[0]) == [1, -1, -1] and list(w[0]) == [3, 0, 0]


def test_empty():
    ids = {0: [1, 2, 3], 1: [4, 5], 2: [], 3: [-1, -1]}
    nbrs, w, cnt = covis_np.neighbours(ids, [0, 2, 3], [1, 2, 3], 2, 1)
    assert not cnt.any() and (nbrs == -1).all() and not w.any()
    assert covis_np.connected([0, 0, 0], 1) == []


def test_ties_follow_position():
    ids = {0: list(range(20)), 1: [0, 1, 2], 2: [3, 4, 5], 3: [6, 7, 8, 9], 4: [10, 11, 12]}
    nbrs, w, cnt = covis_np.neighbours(ids, [0], [4, 2, 3, 1], 4, 3)
    assert list(nbrs[0]) == [3, 4, 2, 1] and list(w[0]) == [4, 3, 3, 3] and cnt[0] == 4
    nbrs, w, cnt = covis_np.neighbours(ids, [0], [1, 2, 4, 3], 2, 3)  # the tie runs across the cut at n
    assert list(nbrs[0]) == [3, 1] and cnt[0] == 2


def test_negative_ids_and_angles_do_not_count():
    ids = {0: [-1, -1, 5, -3], 1: [-1, 5, -3, -3]}
    assert covis_np.weights(ids, [0], [1])[0, 0] == 1


def test_reference_among_its_candidates():
    ids = {0: [1, 2, 3], 1: [1, 2, 3], 2: [1, 2]}
    w = covis_np.weights(ids, [0, 1], [0, 1, 2])
    assert w.tolist() == [[0, 3, 2], [3, 0, 2]]
    nbrs, _, cnt = covis_np.neighbours(ids, [0, 1], [0, 1, 2], 3, 1)
    assert nbrs.tolist() == [[1, 2, -1], [0, 2, -1]] and cnt.tolist() == [2, 2]
    assert np.array_equal(w, weights2(ids, [0, 1], [0, 1, 2]))
