"""CPU: tests/vmap_repose_np.py (the NumPy statement of sdm_vmap_repose) -- its own properties (the identity with an empty
table, an unchanged-pose table, survivor order, the epoch rule, the carry sums and the OR, the log collapse), one pinned
small case with literal ids, pointset_pixels against np_pointset_pixel bit for bit, and the synthetic inputs of
tests/test_gpu_vmap_repose.py, defined here, with the assertion that they cover what that test is there for.

The synthetic maps are made by construction, not by luck.  Two tags A and B share one pixel and rho grid; camera B is
camera A translated by ten voxels, so the stored xyz of the B entries lie ten voxels beside the A entries', in voxels of
their own; a table that sets pose B := pose A puts every B entry bit for bit onto an A entry.  The rest of each map are
entries on a lattice far away whose pixel, rho and tag are free: the hostile ones, the ones a NaN pose or a far pose
drops, the ones whose tag no table names.

Coverage: merged > 0, dropped > 0, moved < reposed < examined, a merge won by the higher old id and a collapsed log pair
are asserted for every map of at least 63 entries under the 37-pose table.  A map of 0 or 1 entries cannot merge, and the
tables of 0, 1 and 2 poses hold, by their size, no more than: nothing; the merge; the merge and a dropping pose -- each of
those is asserted for what it can hold."""
import numpy as np
import pytest

import vmap_import_np as vi
import vmap_np
import vmap_obs_np as vo
import vmap_repose_np as vr
import voxel_np
from test_oracle_crosscheck import np_pointset_pixel

F = np.float32
NOID = 0xFFFFFFFF
SAT = (1 << 32) - 1
VOXEL = 0.05
K_CAM = np.array([100.0, 110.0, 31.5, 23.5], F)
TAG_A, TAG_B, TAG_NAN, TAG_FAR, TAG_ZERO, TAG_KEPT = 3, 7, 11, 12, 13, 99   # TAG_KEPT: in no table
SYN_M = (0, 1, 63, 64, 65, 2047, 2048, 2049, 5000)
SYN_POSES = (0, 1, 2, 37)
LOG_TAG = 5


def pose(rx=0.0, ry=0.0, t=(0, 0, 0)):
    """Tcw float32[12]: a rotation about x then y, and a translation"""
    cx, sx, cy, sy = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry)
    R = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    return np.concatenate([R, np.asarray(t, np.float64).reshape(3, 1)], axis=1).astype(F).reshape(12)


POSE_A = pose(0.02, -0.03, (0.1, -0.2, 0.3))
# camera B = camera A moved by ten voxels along the world's z, off the A grid's sheet: Ow_B = Ow_A + shift  <=>  t_B = t_A - R * shift
POSE_B = POSE_A.copy()
POSE_B.reshape(3, 4)[:, 3] = (POSE_A.reshape(3, 4)[:, 3].astype(np.float64) -
                              POSE_A.reshape(3, 4)[:, :3].astype(np.float64) @ np.array([0, 0, 10 * VOXEL])).astype(F)


def synthetic_records(M, seed=0):
    """the records of a map of exactly M entries (every record in a voxel of its own) and the pairs of its log"""
    rng = np.random.default_rng(1000 + M + seed)
    na = (2 * M) // 5 if M >= 5 else 0          # A entries, then as many B entries on the same grid, then the rest
    rest = M - 2 * na
    gi = np.arange(na)
    gx, gy = 4 * (gi % 40), 4 * (gi // 40)       # 4 px apart at Z = 2: 0.08 > VOXEL between neighbours
    grid_pixel = (gx | (gy << 16)).astype(np.uint32)
    grid_rho = np.full(na, 0.5, F)
    pixel = np.concatenate([grid_pixel, grid_pixel, rng.integers(0, 64, rest) | (rng.integers(0, 48, rest) << 16)]).astype(np.uint32)
    rho = np.concatenate([grid_rho, grid_rho, rng.uniform(0.2, 2.0, rest)]).astype(F)
    tag = np.concatenate([np.full(na, TAG_A), np.full(na, TAG_B), rng.integers(20, 60, rest)]).astype(np.int32)
    mult = rng.integers(1, 4, M).astype(np.uint32)
    li = np.arange(rest)
    lattice = (np.stack([li % 64, li // 64, np.full(rest, 1000)], axis=1) + 0.5) * VOXEL   # far from everything projected
    xyz = np.concatenate([vr.pointset_pixels(K_CAM, POSE_A, gx, gy, grid_rho), vr.pointset_pixels(K_CAM, POSE_B, gx, gy, grid_rho),
                          lattice.astype(F)]).astype(F).reshape(-1, 3)
    sigma = rng.uniform(0.01, 0.2, M).astype(F)
    if na:
        sigma[na] = sigma[0]                      # a tie: the lower old id keeps the voxel
        sigma[na + 1:2 * na:2] = sigma[1:na:2] / 2  # every other B entry beats its A entry: the higher old id wins
    r0 = 2 * na
    hostile = {}
    if rest >= 12:   # the hostile entries, at fixed places among the rest
        h = r0 + np.arange(12)
        tag[h[0]], rho[h[0]], mult[h[0]] = TAG_ZERO, 1e-7, SAT - 1       # rho below 1e-6 -> (0, 0, 0), 2^32 - 2 points ...
        tag[h[1]], rho[h[1]], mult[h[1]] = TAG_ZERO, -0.5, 3             # ... merging with 3 of a negative rho: saturates
        tag[h[2]], pixel[h[2]] = TAG_ZERO, 0                             # pixel 0
        tag[h[3]], pixel[h[3]] = TAG_ZERO, 63 | (47 << 16)               # the image's last pixel: outside the inset
        tag[h[4]], pixel[h[4]] = TAG_ZERO, 60000 | (50000 << 16)         # far outside the image
        tag[h[5]] = tag[h[6]] = TAG_NAN                                  # a NaN pose: dropped
        tag[h[7]] = tag[h[8]] = TAG_FAR                                  # beyond +-2^20 cells: dropped
        tag[h[9]], rho[h[9]] = TAG_NAN, 0.0                              # rho 0 under a NaN pose: (0, 0, 0), not dropped
        tag[h[10]] = tag[h[11]] = TAG_KEPT                               # in no table: keeps its bits
        hostile = {"zero": h[:2], "nan": h[5:7], "far": h[7:9], "kept": h[10:12]}
    rec = {"xyz": xyz, "pixel": pixel, "rho_sigma": np.stack([rho, sigma], axis=1).astype(F),
           "intensity": rng.integers(0, 256, M).astype(np.uint8), "tag": tag, "multiplicity": mult}
    # the log: (A_i, LOG_TAG) and (B_i, LOG_TAG) collapse when B_i joins A_i; the rest is random
    P = 3 * M
    entry = np.concatenate([gi, na + gi, rng.integers(0, max(M, 1), P)]).astype(np.uint32)[:2 * na + (P if M else 0)]
    ltag = np.concatenate([np.full(2 * na, LOG_TAG), rng.integers(0, 9, P)]).astype(np.int32)[:len(entry)]
    return rec, {"entry": entry, "tag": ltag}, hostile


def synthetic_table(n_poses, seed=0):
    """(tags int32[n], K float32[n, 4], Tcw float32[n, 12]) in unsorted tag order"""
    rng = np.random.default_rng(77 + n_poses + seed)
    rows = []
    if n_poses >= 1:
        rows.append((TAG_B, K_CAM, POSE_A))                                   # pose B := pose A: the merge
    if n_poses >= 2:
        rows.append((TAG_NAN, K_CAM, np.full(12, np.nan, F)))                 # dropped
    if n_poses >= 3:
        rows.append((TAG_A, K_CAM, POSE_A))                                   # reposed, not moved
        rows.append((TAG_FAR, K_CAM, pose(0.1, 0.2, (1e6, -1e6, 3e6))))       # beyond +-2^20 cells of 0.05
        rows.append((TAG_ZERO, K_CAM * F(1.01), pose(-0.2, 0.1, (0.5, 0.25, -0.125))))
        used = {TAG_A, TAG_B, TAG_NAN, TAG_FAR, TAG_ZERO, TAG_KEPT}
        free = [t for t in list(range(20, 45)) + [0, (1 << 31) - 1] + list(range(200, 260)) if t not in used]  # 45 .. 59 stay out
        for t in free[:n_poses - len(rows)]:   # tags 20 .. 44 of the rest, then tags that no entry carries
            rows.append((t, K_CAM * F(rng.uniform(0.9, 1.1)), pose(*rng.uniform(-0.3, 0.3, 2), rng.uniform(-1, 1, 3))))
    assert len(rows) == n_poses
    order = rng.permutation(n_poses)
    if n_poses > 1 and (np.diff([rows[i][0] for i in order]) > 0).all():
        order = order[::-1]
    tags = np.array([rows[i][0] for i in order], np.int32)
    return tags, np.array([rows[i][1] for i in order], F).reshape(-1, 4), np.array([rows[i][2] for i in order], F).reshape(-1, 12)


def build(M, seed=0):
    """the synthetic map as the restatement makes it: (vm, ol, records, pairs, hostile)"""
    rec, pairs, hostile = synthetic_records(M, seed)
    vm, ol = vmap_np.VoxelMap(VOXEL), vo.ObservationLog()
    d = vi.import_records(vm, rec)
    assert d["created"] == M == vm.M and d["dropped"] == 0, (M, d["created"], d["dropped"])
    if len(pairs["entry"]):
        vi.import_observations(ol, vm.M, pairs["entry"], pairs["tag"])
    return vm, ol, rec, pairs, hostile


def clone(vm, ol):
    v2, o2 = vmap_np.VoxelMap(vm.voxel_size), vo.ObservationLog()
    v2.rec = {f: a.copy() for f, a in vm.rec.items()}
    v2.keys, v2.ids, v2.points, v2.dropped, v2.calls = vm.keys.copy(), vm.ids.copy(), vm.points, vm.dropped, vm.calls
    o2.entry, o2.tag, o2.pairs, o2.calls = ol.entry.copy(), ol.tag.copy(), ol.pairs.copy(), ol.calls
    return v2, o2


def same_map(a, b, skip=()):
    assert a.M == b.M
    for f in vmap_np.FIELDS:
        if f not in skip:
            assert a.rec[f].tobytes() == b.rec[f].tobytes(), f
    assert (a.keys == b.keys).all() and (a.ids == b.ids).all()


def test_pointset_pixels_is_np_pointset_pixel():
    rng = np.random.default_rng(5)
    x, y = rng.integers(0, 65536, 200), rng.integers(0, 65536, 200)
    rho = rng.uniform(-0.1, 2, 200).astype(F)
    rho[:4] = (0, 1e-7, 9.9e-7, 1e-6)
    for T in (POSE_A, POSE_B, pose(0.3, -0.2, (5, 6, 7))):
        got = vr.pointset_pixels(K_CAM, T, x, y, rho)
        for i in range(200):
            want = np_pointset_pixel(K_CAM, T.reshape(3, 4), int(x[i]), int(y[i]), rho[i])
            assert got[i].tobytes() == np.asarray(want, F).tobytes(), (i, got[i], want)


@pytest.mark.parametrize("M", SYN_M)
def test_identity_with_an_empty_table(M):
    vm, ol, *_ = build(M)
    ev = {f: np.arange(M, dtype=np.uint64) * 3 + 1 for f in ("crossings", "ends")}
    flags = (np.arange(M) % 3 == 0).astype(np.uint8)
    v2, o2 = clone(vm, ol)
    d, ev2, fl2 = vr.repose(v2, o2, None, None, None, True, ev, flags)
    assert (d["examined"], d["reposed"], d["moved"], d["dropped"], d["merged"], d["voxels"]) == (M, 0, 0, 0, 0, M)
    assert (d["remap"] == np.arange(M)).all()
    same_map(v2, vm)
    assert v2.calls == vm.calls + 1 and (v2.points, v2.dropped) == (vm.points, vm.dropped)
    assert o2.calls == ol.calls and o2.E == ol.E == d["observations"] == d["observations_before"]
    assert (o2.entry == ol.entry).all() and (o2.tag == ol.tag).all()
    assert all((ev2[f] == ev[f]).all() for f in ev) and (fl2 == flags).all()
    d, ev2, fl2 = vr.repose(v2, o2, [], None, None, False, ev, flags)
    assert not ev2["crossings"].any() and not ev2["ends"].any() and not fl2.any()


def test_unchanged_pose_table():
    vm, ol, *_ = build(2049)
    v2, o2 = clone(vm, ol)
    d, _, _ = vr.repose(v2, o2, [TAG_A, TAG_B], [K_CAM, K_CAM], [POSE_A, POSE_B])
    na = (2 * 2049) // 5
    assert (d["reposed"], d["moved"], d["dropped"], d["merged"]) == (2 * na, 0, 0, 0)
    same_map(v2, vm)


def test_survivor_order_epoch_rule_carry_and_log_collapse():
    M = 2049
    vm, ol, rec, pairs, hostile = build(M)
    vm.rec["epoch"] = (np.arange(M) % 17 + 1).astype(np.uint32)   # as if built by many calls
    ev = {"crossings": np.arange(M, dtype=np.uint64) + 1, "ends": np.full(M, 1 << 63, np.uint64)}
    flags = (np.arange(M) % 5 == 0).astype(np.uint8)
    tags, K, T = synthetic_table(37)
    v2, o2 = clone(vm, ol)
    d, ev2, fl2 = vr.repose(v2, o2, tags, K, T, True, ev, flags)
    remap = d["remap"]
    surv = np.flatnonzero(remap != NOID)
    # survivors keep their relative order: the first old entry of every new one, in increasing old id, has ids 0, 1, 2 ..
    firsts = remap[surv][np.unique(remap[surv], return_index=True)[1]]
    assert (np.sort(np.unique(remap[surv], return_index=True)[1]) == np.unique(remap[surv], return_index=True)[1]).all()
    assert (firsts == np.arange(d["voxels"])).all()
    # every B entry joined its A entry
    na = (2 * M) // 5
    assert (remap[na:2 * na] == remap[:na]).all() and d["merged"] >= na
    # the epoch rule and the winners: B_i wins where its sigma is strictly smaller; a tie goes to A_i
    b_wins = voxel_np.sigma_key(vm.rec["rho_sigma"][na:2 * na, 1]) < voxel_np.sigma_key(vm.rec["rho_sigma"][:na, 1])
    assert b_wins.any() and not b_wins[0] and not b_wins.all()
    win = np.where(b_wins, na + np.arange(na), np.arange(na))
    two = np.flatnonzero(np.bincount(remap[surv])[remap[:na]] == 2)   # (a re-placed entry of the rest may land there too)
    assert len(two) > na // 2 and b_wins[two].any() and not b_wins[two].all()
    assert (v2.rec["epoch"][remap[two]] == vm.rec["epoch"][win[two]]).all()
    assert (v2.rec["rho_sigma"][remap[two]] == vm.rec["rho_sigma"][win[two]]).all()
    assert (v2.rec["multiplicity"][remap[two]].astype(np.int64) ==
            vm.rec["multiplicity"][two].astype(np.int64) + vm.rec["multiplicity"][na + two]).all()
    # saturation: 2^32 - 2 and 3 in voxel (0, 0, 0)
    z = remap[hostile["zero"]]
    assert z[0] == z[1] != NOID and v2.rec["multiplicity"][z[0]] == SAT and not v2.rec["xyz"][z[0]].any()
    assert (remap[hostile["nan"]] == NOID).all() and (remap[hostile["far"]] == NOID).all()
    k = remap[hostile["kept"]]
    assert (v2.rec["xyz"][k] == vm.rec["xyz"][hostile["kept"]]).all()
    # carry: 64-bit sums (wrapping: two ends of 2^63 give 0) and the OR
    for f in ev:
        want = np.zeros(d["voxels"], np.uint64)
        for i in surv:
            want[remap[i]] = np.uint64((int(want[remap[i]]) + int(ev[f][i])) & ((1 << 64) - 1))
        assert (ev2[f] == want).all(), f
    assert (ev2["ends"][remap[two]] == 0).all()
    assert (fl2[remap[two]] == (flags[two] | flags[na + two])).all() and 0 < fl2.sum() < flags.sum()
    # the log: no pair of a dropped entry, equal pairs collapsed, the survivors in their old order
    keys = [(int(remap[e]), int(t)) for e, t in zip(ol.entry, ol.tag) if remap[e] != NOID]
    seen, want = set(), []
    for p in keys:
        if p not in seen:
            seen.add(p)
            want.append(p)
    assert list(zip(o2.entry.tolist(), o2.tag.tolist())) == want
    assert len(want) < len(keys) < ol.E and o2.calls == ol.calls
    assert (d["observations_before"], d["observations"]) == (ol.E, len(want))


def test_pinned_small_case():
    """six entries at voxel 1.0: entries 1 and 4 move into entry 0's voxel, entry 2 is dropped, entry 3 is not named"""
    vm, ol = vmap_np.VoxelMap(1.0), vo.ObservationLog()
    Kc = np.array([1, 1, 0, 0], F)
    ident = pose()
    rec = {"xyz": np.array([[0.5, 0.5, 1.5], [5.5, 0.5, 1.5], [9.5, 0.5, 1.5], [20.5, 0.5, 0.5], [7.5, 7.5, 7.5], [30.5, 0.5, 0.5]], F),
           "pixel": np.array([0, 0, 0, 0, 0, 1 | (1 << 16)], np.uint32),
           "rho_sigma": np.array([[1, 0.2], [1, 0.1], [1, 0.3], [1, 0.4], [1, 0.2], [0.5, 0.5]], F),
           "intensity": np.arange(6, dtype=np.uint8), "tag": np.array([1, 2, 3, 4, 5, 6], np.int32),
           "multiplicity": np.array([1, 2, 3, 4, 5, 6], np.uint32)}
    vi.import_records(vm, rec)
    vi.import_observations(ol, 6, [0, 1, 2, 4, 3, 5], [9, 9, 9, 9, 8, 7])
    # tag 1, 2, 5 -> the identity pose at pixel (0, 0), rho 1: (0, 0, 1); tag 3 -> NaN; tag 6 -> pixel (1, 1), rho 0.5: (2, 2, 2)
    tags = [5, 3, 2, 6, 1]
    T = [ident, np.full(12, np.nan, F), ident, ident, ident]
    d, ev, fl = vr.repose(vm, ol, tags, [Kc] * 5, T, True, {"crossings": np.array([1, 2, 4, 8, 16, 32], np.uint64),
                                                           "ends": np.zeros(6, np.uint64)}, np.array([0, 0, 1, 0, 1, 0], np.uint8))
    assert d["remap"].tolist() == [0, 0, NOID, 1, 0, 2]
    assert {f: d[f] for f in vr.DELTA} == {"examined": 6, "reposed": 5, "moved": 5, "dropped": 1, "merged": 2, "voxels": 3,
                                           "observations_before": 6, "observations": 3}
    assert vm.rec["xyz"].tolist() == [[0, 0, 1], [20.5, 0.5, 0.5], [2, 2, 2]]
    assert vm.rec["tag"].tolist() == [2, 4, 6] and vm.rec["multiplicity"].tolist() == [8, 4, 6]
    assert vm.rec["epoch"].tolist() == [1, 1, 1] and vm.calls == 2 and vm.points == 21
    assert list(zip(ol.entry.tolist(), ol.tag.tolist())) == [(0, 9), (1, 8), (2, 7)]
    assert ev["crossings"].tolist() == [19, 8, 32] and fl.tolist() == [1, 0, 0]


@pytest.mark.parametrize("n_poses", SYN_POSES)
@pytest.mark.parametrize("M", SYN_M)
def test_synthetic_inputs_cover_the_cases(M, n_poses):
    vm, ol, rec, pairs, hostile = build(M)
    tags, K, T = synthetic_table(n_poses)
    assert len(tags) == n_poses and len(set(tags.tolist())) == n_poses
    if n_poses > 1:
        assert (np.diff(tags) < 0).any()   # unsorted
    if n_poses == 37:
        assert not np.isin(tags, vm.rec["tag"]).all() or M < 63   # tags that no entry carries
    sig = vm.rec["rho_sigma"][:, 1].copy()
    d, _, _ = vr.repose(vm, ol, tags, K, T)
    remap = d["remap"]
    na = (2 * M) // 5 if M >= 5 else 0
    if n_poses == 0:
        assert d["reposed"] == d["merged"] == d["dropped"] == 0
        return
    if M < 63:
        return
    assert d["merged"] > 0
    won_by_higher = voxel_np.sigma_key(sig[na:2 * na]) < voxel_np.sigma_key(sig[:na])
    assert (remap[na:2 * na] == remap[:na]).all() and won_by_higher.any()
    assert d["observations"] < d["observations_before"]   # a collapsed pair: (A_i, LOG_TAG) and (B_i, LOG_TAG)
    if n_poses >= 2:
        assert d["dropped"] > 0
    if n_poses == 37:
        assert 0 < d["moved"] < d["reposed"] < d["examined"]
        assert vm.rec["multiplicity"].max() == SAT
