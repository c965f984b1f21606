"""Which neighbours confirm each pixel: PM.cc:659-765 of InterKeyFrameDepthChecking restated in plain NumPy -- test
infrastructure for sdm_extract_points_support.

The reference keeps only the COUNT of the neighbours whose depth map agrees with a pixel (`nj >= 1` summed over the
neighbours, PM.cc:755, compared with lambdaN at PM.cc:764).  This restatement keeps the set as well: bit j of a pixel's
64-bit word is set iff neighbour j is counted.  It works on maps, intrinsics and poses only, so any device state can be
checked by downloading the maps; no oracle is needed.  Arithmetic: the build's normative N1/N2 choice (np_pm.py), every
operation an elementwise IEEE float32 / float64 NumPy operation in the order the C++ promotion rules give.
"""
import numpy as np

from np_pm import KF, LAMBDA_N, Pair, _ray, _rows_dot_xp

f32, f64 = np.float32, np.float64


def keyframe(K, Tcw, H, W):
    """an np_pm.KF that carries what this check reads: intrinsics, pose and the image size"""
    z = np.zeros((H, W), np.uint8)
    return KF(z, z, z, 0.0, K, Tcw)


def inter_support(cur, cur_rho, nbrs, nbr_rho, nbr_sigma, lambda_n=LAMBDA_N):
    """cur: KF of the reference, cur_rho its depth map [H, W]; nbrs: KFs of its neighbour row (a keyframe may repeat),
    nbr_rho / nbr_sigma their depth maps.  Returns (checked rho [H, W] float32, support [H, W] uint64): the map PM.cc:762-793
    leaves behind, and per pixel the neighbours PM.cc:755 counted (0 outside the 2-px inset and where PM.cc:662 skips)."""
    H, W = cur.H, cur.W
    assert len(nbrs) <= 64
    out = np.array(cur_rho, f32, copy=True)
    words = np.zeros((H, W), np.uint64)
    with np.errstate(all="ignore"):
        sel = ~(out[2:H - 2, 2:W - 2].astype(f64) < 0.000001)  # PM.cc:659-662
    ys, xs = np.nonzero(sel)
    ys, xs = ys + 2, xs + 2
    P = len(xs)
    if not P:
        return out, words
    depthp = out[ys, xs]
    xp0, xp1 = _ray(cur, xs, ys)  # PM.cc:677
    count = np.zeros(P, np.int64)
    word = np.zeros(P, np.uint64)
    sum_Jr, sum_JJ = np.zeros(P, f32), np.zeros(P, f32)
    pairs = {}
    with np.errstate(all="ignore"):
        dp = f32(1) / depthp  # PM.cc:769
        for j, (kj, rj, sj) in enumerate(zip(nbrs, nbr_rho, nbr_sigma)):
            pr = pairs.get(id(kj))
            if pr is None:
                pr = pairs[id(kj)] = Pair(cur, kj)  # Rji, tji: PM.cc:643-644
            rf, _ = _rows_dot_xp(pr, xp0, xp1)
            t = pr.t21
            tmp = [rf[i] / depthp + t[i] for i in range(3)]  # PM.cc:678
            rzxp = rf[2]
            u = kj.fx * tmp[0] + kj.cx * tmp[2]  # PM.cc:679
            v = kj.fy * tmp[1] + kj.cy * tmp[2]
            xj, yj = u / tmp[2], v / tmp[2]  # PM.cc:680
            depthj = depthp / (rzxp + depthp * t[2])  # PM.cc:684-688
            inb = (xj >= 0) & (xj < W - 1) & (yj >= 0) & (yj < H - 1)  # PM.cc:695 (a NaN coordinate is outside)
            x0 = np.floor(np.where(inb, xj, 0)).astype(np.int64)
            y0 = np.floor(np.where(inb, yj, 0)).astype(np.int64)
            nj = np.zeros(P, np.int64)
            for yy, xx in ((y0, x0), (y0 + 1, x0), (y0, x0 + 1), (y0 + 1, x0 + 1)):  # PM.cc:705, 717, 729, 741
                d, sg = rj[yy, xx], sj[yy, xx]
                dd = depthj - d
                test = ((f64(dd) * f64(dd)) / (f64(sg) * f64(sg))).astype(f32)  # PM.cc:709
                ok = inb & (d.astype(f64) > 0.000001) & (test.astype(f64) < 3.84)
                nj += ok
                djn = f32(1) / d  # PM.cc:777-783
                d2s = djn * djn * sg
                J = -rzxp / d2s
                r0 = (djn - dp * rzxp - t[2]) / d2s
                sum_Jr = np.where(ok, sum_Jr + J * r0, sum_Jr)
                sum_JJ = np.where(ok, sum_JJ + J * J, sum_JJ)
            hit = nj >= 1  # PM.cc:755
            count += hit
            word |= hit.astype(np.uint64) << np.uint64(j)
        new = f32(1) / (dp + (-sum_Jr) / sum_JJ)  # PM.cc:788-793
    out[ys, xs] = np.where(count < lambda_n, f32(0), new)  # PM.cc:762-765
    words[ys, xs] = word
    return out, words


def fixture_support(g, k, rho=None, sigma=None, nbr_row=None):
    """the restatement for keyframe k of a golden fixture (tests/golden_util.load), over its `rho` / `sigma` maps unless
    others are given; nbr_row: another neighbour row than the fixture's"""
    rho = g["rho"] if rho is None else rho
    sigma = g["sigma"] if sigma is None else sigma
    row = [int(j) for j in (g["nbrs"][k] if nbr_row is None else nbr_row)]
    kfs = {j: keyframe(g["K"], g["Tcw"][j], g["H"], g["W"]) for j in set(row) | {k}}
    return inter_support(kfs[k], rho[k], [kfs[j] for j in row], [rho[j] for j in row], [sigma[j] for j in row])


def popcount(w):
    w = np.asarray(w, np.uint64)
    return np.unpackbits(np.ascontiguousarray(w).view(np.uint8).reshape(w.shape + (8,)), axis=-1).sum(-1).astype(np.int64)
