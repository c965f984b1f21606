"""NumPy restatement of sdm_vmap_normals (include/sdm_c.h): per-entry surface normals and surface variation of the persistent
voxel map, vectorised over the entries of the range.  Every operation is one IEEE binary32 operation of NumPy (+ - * / sqrt are
correctly rounded there, nothing is fused, denormals are kept), in the order the header gives.

  member      multiplicity[id] >= min_multiplicity and, with require_published, published[id] != 0 (flags None: every flag
              reads 0) -- vmap_comp_np's
  cell        floor(P * inv) in float32, inv = float32(1) / float32(voxel_size) -- vmap_comp_np.cells_of
  samples     the offsets d in {-r..r}^3 in lexicographic order (dx slowest); a cell with a coordinate outside [-2^20, 2^20)
              holds nothing (tested before anything is looked up); the cell's entry j is a sample iff it exists and is a member;
              q = (xyz_j - P) * inv
  sums        k, s_a, m_ab from +0 in visiting order; points = k (0 for a non-member)
  covariance  k >= min_points: kf = float32(k), mu = s / kf, C_ab = m_ab / kf - mu_a * mu_b
  eigen-solve cyclic Jacobi, 6 sweeps of the pairs (0,1), (0,2), (1,2); a pair with A_pq == 0 does nothing
  result      m = the index of the smallest lambda (ties to the lower index); sum = (l0 + l1) + l2; !(sum > 0): not estimated;
              normal = column m of V; variation = max(lambda_m, +0) / sum
  orientation the record's tag in the table: d = O - P, dot = (n0*d0 + n1*d1) + n2*d2, dot < 0 negates; a NaN does not
  otherwise   normal (+0, +0, +0), variation -1
  totals      entries (the size of the range), members, estimated, oriented"""
import numpy as np

from carve_np import camera_centre
from vmap_cast_np import stops
from vmap_comp_np import LIM, cells_of

f32 = np.float32
OUTS = ("entries", "members", "estimated", "oriented")
ARRAYS = ("normal", "variation", "points")
SWEEPS = 6
PAIRS = ((0, 1, 2), (0, 2, 1), (1, 2, 0))   # (p, q, r)
STATS = ("skipped pair", "overflowing theta", "negative lambda_m", "sum not positive", "below min_points", "absent tag", "flip",
         "no flip", "clipped")


def offsets(radius):
    r = range(-radius, radius + 1)
    return [(dx, dy, dz) for dx in r for dy in r for dz in r]


def _pack(c):
    """a lookup key for cells already known to be in range (never formed for a cell outside it)"""
    c = c + LIM
    return (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]


def normals(rec, flags, voxel_size, tags=None, Tcw=None, radius=1, min_points=3, min_multiplicity=0, require_published=False,
            first=0, count=None):
    """rec: the map's records {"xyz" float32[M, 3], "multiplicity" uint32[M], "tag" int32[M]}; flags: uint8[M] or None; tags
    int32[n] and Tcw float32[n, 12] or None -> dict(normal float32[m, 3], variation float32[m], points uint32[m], the four
    totals, stats: how often each kind of case in STATS occurred, lam float32[m, 3]: the eigenvalues (NaN where not reached))"""
    assert radius in (1, 2) and 3 <= min_points <= (2 * radius + 1) ** 3
    xyz = np.ascontiguousarray(rec["xyz"], f32).reshape(-1, 3)
    M = len(xyz)
    count = M - first if count is None else count
    assert 0 <= first and 0 <= count and first + count <= M
    inv = f32(1.0) / f32(voxel_size)
    cell = cells_of(xyz, voxel_size)
    assert ((cell >= -LIM) & (cell < LIM)).all()   # (an entry outside the range does not exist)
    member = stops(rec, flags, min_multiplicity, require_published)
    keys = _pack(cell)
    by_key = np.argsort(keys, kind="stable")
    sorted_keys = keys[by_key]
    assert (sorted_keys[1:] != sorted_keys[:-1]).all()   # one entry per cell
    stats = dict.fromkeys(STATS, 0)

    normal = np.zeros((count, 3), f32)
    variation = np.full(count, -1, f32)
    points = np.zeros(count, np.uint32)
    lam_out = np.full((count, 3), np.nan, f32)
    ids = first + np.flatnonzero(member[first:first + count])   # the members of the range
    res = {"entries": int(count), "members": len(ids), "estimated": 0, "oriented": 0}
    with np.errstate(all="ignore"):
        P = xyz[ids]
        c0 = cell[ids]
        n = len(ids)
        k = np.zeros(n, np.uint32)
        s = [np.zeros(n, f32) for _ in range(3)]
        mm = {ab: np.zeros(n, f32) for ab in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))}
        clipped = np.zeros(n, bool)
        for d in offsets(radius):
            nc = c0 + np.array(d, np.int64)
            inside = ((nc >= -LIM) & (nc < LIM)).all(1)
            clipped |= ~inside
            hit = np.zeros(n, bool)
            j = np.zeros(n, np.int64)
            if M and inside.any():
                kk = _pack(nc[inside])
                pos = np.minimum(np.searchsorted(sorted_keys, kk), M - 1)
                found = sorted_keys[pos] == kk
                jj = by_key[pos]
                hit[inside] = found & member[jj]
                j[inside] = jj
            q = [(xyz[j, a] - P[:, a]) * inv for a in range(3)]
            k = np.where(hit, k + np.uint32(1), k).astype(np.uint32)
            for a in range(3):
                s[a] = np.where(hit, s[a] + q[a], s[a])
            for (a, b) in mm:
                mm[a, b] = np.where(hit, mm[a, b] + q[a] * q[b], mm[a, b])
        stats["clipped"] = int(clipped.sum())
        points[ids - first] = k

        enough = k >= np.uint32(min_points)
        stats["below min_points"] = int((~enough).sum())
        kf = k.astype(f32)
        mu = [s[a] / kf for a in range(3)]
        A = {ab: mm[ab] / kf - mu[ab[0]] * mu[ab[1]] for ab in mm}
        V = [[np.full(n, 1 if i == jx else 0, f32) for jx in range(3)] for i in range(3)]
        one = f32(1)

        def get(a, b):
            return A[(a, b) if a <= b else (b, a)]

        def put(a, b, v):
            A[(a, b) if a <= b else (b, a)] = v

        for _ in range(SWEEPS):
            for p, q_, r in PAIRS:
                apq = get(p, q_)
                act = apq != 0
                theta = (get(q_, q_) - get(p, p)) / (f32(2) * apq)
                tt = theta * theta
                t = np.copysign(one, theta) / (np.abs(theta) + np.sqrt(tt + one))
                c = one / np.sqrt(t * t + one)
                sn = t * c
                h = t * apq
                stats["skipped pair"] += int((enough & ~act).sum())
                stats["overflowing theta"] += int((enough & act & np.isinf(tt)).sum())
                put(p, p, np.where(act, get(p, p) - h, get(p, p)))
                put(q_, q_, np.where(act, get(q_, q_) + h, get(q_, q_)))
                put(p, q_, np.where(act, f32(0), apq))
                x, y = get(r, p), get(r, q_)
                put(r, p, np.where(act, c * x - sn * y, x))
                put(r, q_, np.where(act, sn * x + c * y, y))
                for i in range(3):
                    x, y = V[i][p], V[i][q_]
                    V[i][p] = np.where(act, c * x - sn * y, x)
                    V[i][q_] = np.where(act, sn * x + c * y, y)
        lam = [A[0, 0], A[1, 1], A[2, 2]]
        m = np.zeros(n, np.int64)
        lm = lam[0]
        pick = lam[1] < lm
        m, lm = np.where(pick, 1, m), np.where(pick, lam[1], lm)
        pick = lam[2] < lm
        m, lm = np.where(pick, 2, m), np.where(pick, lam[2], lm)
        total = (lam[0] + lam[1]) + lam[2]
        est = enough & (total > 0)
        stats["sum not positive"] = int((enough & ~(total > 0)).sum())
        stats["negative lambda_m"] = int((est & (lm < 0)).sum())
        nrm = [np.where(m == 0, V[i][0], np.where(m == 1, V[i][1], V[i][2])) for i in range(3)]
        var = np.where(lm < 0, f32(0), lm) / total

        # orientation
        tg = np.asarray([] if tags is None else tags, np.int32).reshape(-1)
        assert len(set(tg.tolist())) == len(tg) and (tg >= 0).all()
        rtag = np.asarray(rec["tag"], np.int32).reshape(-1)[ids]
        ori = np.zeros(n, bool)
        if len(tg):
            T = np.asarray(Tcw, f32).reshape(-1, 12)
            assert len(T) == len(tg)
            O = np.stack([camera_centre(T[i]) for i in range(len(tg))]).astype(f32)
            order = np.argsort(tg, kind="stable")
            pos = np.minimum(np.searchsorted(tg[order], rtag), len(tg) - 1)
            row = order[pos]
            ori = est & (tg[row] == rtag)
            dd = [O[row, a] - P[:, a] for a in range(3)]
            dot = (nrm[0] * dd[0] + nrm[1] * dd[1]) + nrm[2] * dd[2]
            flip = ori & (dot < 0)
            nrm = [np.where(flip, -nrm[a], nrm[a]) for a in range(3)]
            stats["flip"], stats["no flip"] = int(flip.sum()), int((ori & ~flip).sum())
        stats["absent tag"] = int((est & ~ori).sum())

        at = ids - first
        for a in range(3):
            normal[at, a] = np.where(est, nrm[a], f32(0))
            lam_out[at, a] = np.where(enough, lam[a], f32(np.nan))
        variation[at] = np.where(est, var, f32(-1))
        res["estimated"], res["oriented"] = int(est.sum()), int(ori.sum())
    res.update(normal=normal, variation=variation, points=points, stats=stats, lam=lam_out)
    return res
