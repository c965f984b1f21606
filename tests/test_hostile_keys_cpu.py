"""CPU: the crafted colliding keys of tests/hostile_keys.py, the linear-probing model, and the hostile map that
tests/test_gpu_hostile_table.py puts into an engine -- its layout conditions, and the restatements against their scalar
twins on it.  Nothing here touches an engine.

The hostile map (voxel 1) is imported in two calls:
  (a) a chain of L colliding cells: their keys all hash to a value ending in twenty ones, so at every capacity up to 2^20
      they home on the table's last slot, occupy it and the slots 0 .. L - 2, and all but one sit below their home;
  (b) geometric pieces near OFF: a two-layer plane patch, a line, isolated cells, and records that share a cell with
      differing sigma and multiplicity.
Of the pieces' entries and of the absent cells their queries probe, about L / capacity home inside the chain's run and are
walked through it; so are the cells sdm_vmap_mesh looks up from its owners, with and without an entry, at every capacity the
GPU test reaches.  OFF is chosen so that the counts below hold; they are conditions on the input, not measurements."""
import functools

import numpy as np
import pytest

import hostile_keys as hk
import vmap_import_np as vi
import vmap_mesh_np as vms
import vmap_normals_np as vn
import vmap_np
import vmap_obs_np as vo
from test_vmap_cast_cpu import both as cast_both
from test_vmap_comp_cpu import both as comp_both
from test_vmap_normals_cpu import both as normals_both
from test_vmap_recarve_cpu import both as recarve_both

F = np.float32
U = np.uint64
VOXEL = 1.0
L = 384                      # the chain of the map's table
SEED = 1
OFF = np.array([-17, 9, 4])   # the pieces' corner, in cells: they straddle zero on x
CHAIN_TAGS = (10, 11, 12, 13)  # the chain's records carry these in turn; the pieces carry PIECE_TAGS
PIECE_TAGS = (0, 1, 2, 3)
CAP_PIECES = 2048            # the table's capacity once (b) is in: 2 (L + records of (b)) > 1024
RECORD_FIELDS = ("xyz", "pixel", "rho_sigma", "intensity", "tag", "multiplicity")
MIN_PIECES_IN_RUN, MIN_ABSENT_IN_RUN = 20, 200
# of the distinct cells the mesh looks up, over the four sets of normals the GPU test gives it, those with their home inside
# the chain's run: with and without an entry.  The mesh looks up some thousands of distinct cells, a few hundred of them
# pieces' entries, and the run is L / capacity of the table: at 8192 slots, with three quarters of the chain left, 3.5 % --
# about 10 and 200; the minima are half of that, and hold at 2048 and 4096 slots all the more
MIN_MESH_PRESENT_IN_RUN, MIN_MESH_ABSENT_IN_RUN = 5, 100
SET_BITS = 12                # the observation set's chain survives up to 4096 slots; the tests reach 2048
SET_HEAD, SET_REST = (3, 60), (20, 3)  # its chain: 60 tags on each of entries 0 .. 2, 3 on each of 20 piece entries
SET_CHAIN = SET_HEAD[0] * SET_HEAD[1] + SET_REST[0] * SET_REST[1]
RETIRED = 13                 # the chain's tag the GPU test retires: entries 3, 7, 11, ... go, entries 0 .. 2 keep their ids
# the plane of 60 x 60 cells at z = 0 in 8192 slots, inserted in raster order: the layout the rest of the suite gives
NATURAL = (18, 0)


def chain_records(n=L, seed=SEED, voxel=VOXEL):
    """(cells, records) of the chain"""
    cells, xyz, _ = hk.colliding_cells(n, seed, voxel=voxel)
    i = np.arange(n)
    rec = {"xyz": xyz, "pixel": ((i % 24) << 16 | (i % 32)).astype(np.uint32),
           "rho_sigma": np.stack([np.ones(n), 0.01 + 0.001 * (i % 7)], 1).astype(F), "intensity": (i * 7 % 256).astype(np.uint8),
           "tag": np.array(CHAIN_TAGS, np.int32)[i % 4], "multiplicity": (1 + i % 3).astype(np.uint32)}
    return cells, rec


def piece_cells():
    """the distinct cells of (b), in entry order: patch, line, isolated"""
    gx, gy, gz = np.meshgrid(np.arange(13), np.arange(10), np.arange(2), indexing="ij")
    patch = np.stack([gx, gy, gz], -1).reshape(-1, 3)
    line = np.stack([16 + np.arange(30), np.full(30, 3), np.full(30, 6)], 1)
    lone = np.stack([-6 + 4 * np.arange(8), np.full(8, -7), -5 + 3 * (np.arange(8) % 2)], 1)
    return np.concatenate([patch, line, lone]) + OFF


def piece_records(voxel=VOXEL):
    """(cells, records) of (b): one record per cell at a point inside it, then 24 records more in patch cells -- lower,
    equal and higher sigma than the cell's first, multiplicities 2 and 3"""
    rng = np.random.default_rng(7)
    cells = piece_cells()
    at = np.concatenate([np.arange(len(cells)), np.arange(0, 240, 10)])
    n = len(at)
    xyz = ((cells[at] + rng.uniform(0.1, 0.9, (n, 3))) * voxel).astype(F)
    sigma = np.full(n, 0.004, F)
    sigma[len(cells):] = np.array([0.002, 0.004, 0.006], F)[np.arange(24) % 3]
    i = np.arange(n)
    mult = np.ones(n, np.uint32)
    mult[len(cells):] = 2 + np.arange(24) % 2
    rec = {"xyz": xyz, "pixel": ((i % 24) << 16 | (i % 32)).astype(np.uint32), "rho_sigma": np.stack([np.ones(n, F), sigma], 1),
           "intensity": (i * 3 % 256).astype(np.uint8), "tag": np.array(PIECE_TAGS, np.int32)[i % 4], "multiplicity": mult}
    assert (hk.restated_key(xyz, voxel) == hk.cell_key(cells[at])).all()
    return cells, rec


def growth_records(k, voxel=VOXEL):
    """further geometric records, far from the pieces: 1100 (k = 0) and 1600 (k = 1) distinct cells of two blocks"""
    n = (1100, 1600)[k]
    i = np.arange(n)
    cells = np.stack([i % 12, (i // 12) % 12, i // 144], 1) + OFF + (100 + 60 * k)
    rec = {"xyz": hk.centres(cells, voxel), "rho_sigma": np.stack([np.ones(n, F), np.full(n, 0.005, F)], 1),
           "tag": np.full(n, 20 + k, np.int32)}
    return cells, rec


def neighbourhood(cells, radius):
    """the distinct cells within `radius` (Chebyshev) of any of `cells`"""
    r = np.arange(-radius, radius + 1)
    d = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    return np.unique((np.asarray(cells)[:, None, :] + d[None]).reshape(-1, 3), axis=0)


def absent_probed(present_cells, about_cells, radius=1):
    """the cells within `radius` of `about_cells` that hold no entry: classify's 26-cell occupancy, components and normals
    at radius 1 probe every one of them"""
    near = neighbourhood(about_cells, radius)
    return near[~np.isin(hk.cell_key(near), hk.cell_key(present_cells))]


def pose_at(centre):
    """Tcw float32[12] of a camera at `centre` looking along +z"""
    T = np.eye(4, dtype=F)[:3].copy()
    T[:, 3] = -np.asarray(centre, F)
    return T.reshape(12)


def camera_table():
    """the pose table of the recarve: the pieces' four tags a few cells from the pieces, and there too the first colliding
    tag of the chain's entry 0 (its ray to that far cell is longer than any max_steps: skipped).  The other colliding tags
    have no pose"""
    tags = list(PIECE_TAGS) + [int(set_chain_pairs()[1][0])]
    at = [(-3.5, 4.5, 6.5), (6.5, -4.5, 9.5), (15.5, 12.5, -4.5), (30.5, 3.5, 1.5), (5.5, 5.5, 12.5)]
    return tags, np.stack([pose_at(np.array(c) + OFF) for c in at])


def piece_pairs(n_pieces, first_id=L):
    """ordinary pairs: every piece entry seen by two of the pieces' tags, a few by all four, and every fifth entry of the
    chain by tag 1 (rays far longer than max_steps; those of the entries a retire drops vanish with them)"""
    e = first_id + np.arange(n_pieces)
    far = np.arange(0, first_id, 5)
    entry = np.concatenate([e, e, e[::9], e[::9], far])
    tag = np.concatenate([e % 4, (e + 1) % 4, (e[::9] + 2) % 4, (e[::9] + 3) % 4, np.ones(len(far), np.int64)])
    return entry.astype(np.uint32), tag.astype(np.int32)


@functools.lru_cache(maxsize=None)
def set_chain_pairs():
    """pairs whose set keys collide: SET_HEAD[1] tags on each of the chain's first SET_HEAD[0] entries, and SET_REST[1] on
    each of SET_REST[0] piece entries.  A retire renumbers the entries behind the first one it drops, and a pair's key holds
    the entry id: only the pairs of entries 0 .. 2, which RETIRED leaves in place, still collide after it."""
    ids = np.concatenate([np.arange(SET_HEAD[0]), L + np.arange(SET_REST[0]) * 11])
    per = np.concatenate([np.full(SET_HEAD[0], SET_HEAD[1]), np.full(SET_REST[0], SET_REST[1])])
    tags = hk.colliding_tags(ids, int(per.max()), SET_BITS)
    entry = np.concatenate([np.full(n, e) for e, n in zip(ids, per)])
    tag = np.concatenate([tags[i, :n] for i, n in enumerate(per)])
    return entry.astype(np.uint32), tag.astype(np.int32)


def cast_rays(chain_cells, pieces, displaced, absent_in_run):
    """short segments ending in chain cells, in displaced piece cells and in absent cells that home inside the run"""
    ends = np.concatenate([chain_cells[:40], displaced[:40], absent_in_run[:120]])
    rng = np.random.default_rng(3)
    step = rng.integers(-3, 4, ends.shape)
    step[(step == 0).all(1)] = (2, -1, 1)
    P = ((ends + rng.uniform(0.2, 0.8, ends.shape))).astype(F)
    O = ((ends + step + rng.uniform(0.2, 0.8, ends.shape))).astype(F)
    return O, P


def axis_normals(M, axis):
    """float32[M, 3]: every entry's normal along +-e_axis, the sign by the id's parity -- sdm_vmap_mesh then stitches along that
    axis whatever the geometry is, so between them the three axes walk every direction through the table"""
    n = np.zeros((M, 3), F)
    n[:, axis] = 1 - 2 * (np.arange(M) % 2)
    return n


def mesh_probes(rec, flags, normal, keys, cap, run, **kw):
    """the distinct cells sdm_vmap_mesh looks up for these normals (vmap_mesh_np.mesh's own lookups: the cell below every
    member, then up to 20 more per owner) whose home at `cap` slots lies inside `run`: (those that hold an entry, those
    that hold none).  Both kinds are walked through the chain."""
    probed = []
    res = vms.mesh(rec, flags, VOXEL, normal, probed=probed, **kw)
    cells = np.unique(np.concatenate(probed), axis=0)
    inside = cells[hk.homes_in_run(hk.cell_key(cells), cap, run)]
    present = np.isin(hk.cell_key(inside), np.asarray(keys, U))
    return inside[present], inside[~present], res


def build_map():
    """the hostile map on the restatement: (VoxelMap, chain cells, piece cells, dst_ids of (a), dst_ids of (b))"""
    vm = vmap_np.VoxelMap(VOXEL)
    cc, ra = chain_records()
    pc, rb = piece_records()
    da = vi.import_records(vm, ra)
    db = vi.import_records(vm, rb)
    assert da["created"] == L and db["created"] == len(pc) and db["dropped"] == 0
    return vm, cc, pc, da["dst_ids"], db["dst_ids"]


def layout(vm, cap):
    """the model of the map's table at `cap` slots and the keys' uint64 form"""
    keys = vm.keys.astype(U)
    return hk.table_model(keys, cap), keys


# ---- the helper -----------------------------------------------------------------------------------------------------------
def test_mix_and_unmix_are_inverse():
    rng = np.random.default_rng(0)
    z = np.concatenate([rng.integers(0, 1 << 64, 100000, dtype=np.uint64),
                        np.array([0, 1, 2, (1 << 63) - 1, 1 << 63, (1 << 64) - 1, (1 << 32) - 1, 1 << 32, 0xFFFFF], U),
                        U(1) << np.arange(64, dtype=U)])
    assert (hk.unmix(hk.mix(z)) == z).all() and (hk.mix(hk.unmix(z)) == z).all()
    assert int(hk.C1) * int(hk.C1_INV) % (1 << 64) == 1 and int(hk.C2) * int(hk.C2_INV) % (1 << 64) == 1
    assert int(hk.mix(np.array([0], U))[0]) == 0 and int(hk.mix(np.array([1], U))[0]) == 0x5692161D100B05E5  # SplitMix64's


@pytest.mark.parametrize("voxel", (1.0, 0.25))
def test_crafted_cells_survive_binary32(voxel):
    cells, xyz, draws = hk.colliding_cells(2000, SEED, voxel=voxel)
    assert 3600 < draws < 4400  # about half of the draws have the top bit set
    keys = hk.cell_key(cells)
    assert len(np.unique(keys)) == 2000 and (np.abs(cells) <= 1 << 20).all()
    assert xyz.dtype == F and (hk.restated_key(xyz, voxel) == keys).all()
    assert (hk.key_cells(keys) == cells).all()
    ones = U((1 << 20) - 1)
    assert ((hk.mix(keys) & ones) == ones).all()


@pytest.mark.parametrize("n,cap", [(2000, 4096), (L, 1024), (L, CAP_PIECES), (L, 1 << 20), (128, 1024)])
def test_model_bounds_on_a_chain(n, cap):
    """a chain of n: one run from the last slot on, displacement >= n - 1 and n - 1 wrapped keys -- for every order"""
    keys = hk.cell_key(hk.colliding_cells(n, SEED)[0])
    m = hk.table_model(keys, cap)
    assert m["run"] == (cap - 1, n) and m["homes_in"] == n and m["min_disp"] == n - 1 and m["min_wraps"] == n - 1
    assert m["occupied"][cap - 1] and m["occupied"][:n - 1].all() and m["occupied"].sum() == n
    rng = np.random.default_rng(n)
    for order in (np.arange(n), np.arange(n)[::-1], rng.permutation(n)):
        slot, seen = hk.table_layout(keys[order], cap)
        assert seen == (n - 1, n - 1)
        occ = np.zeros(cap, bool)
        occ[slot] = True
        assert (occ == m["occupied"]).all()  # the occupied set does not depend on the order


def test_model_against_layouts_of_mixed_keys():
    """random keys mixed with a chain, at a load near 0.5: every order's layout has the model's occupied set and respects
    its two bounds"""
    rng = np.random.default_rng(5)
    keys = np.concatenate([hk.cell_key(hk.colliding_cells(100, 3)[0]), rng.integers(0, 1 << 63, 400, dtype=np.uint64)])
    m = hk.table_model(keys, 1024)
    assert m["run"][1] > 100
    for _ in range(5):
        slot, (disp, wraps) = hk.table_layout(rng.permutation(keys), 1024)
        occ = np.zeros(1024, bool)
        occ[slot] = True
        assert (occ == m["occupied"]).all() and disp >= m["min_disp"] >= 99 and wraps >= m["min_wraps"] >= 99


def test_natural_input_barely_probes():
    """the contrast: the geometric input of the other tests probes a few slots deep and never past the table's end"""
    g = np.stack(np.meshgrid(np.arange(60), np.arange(60), [0], indexing="ij"), -1).reshape(-1, 3)
    assert hk.table_layout(hk.cell_key(g), 8192)[1] == NATURAL
    assert hk.table_layout(hk.cell_key(hk.colliding_cells(2000, SEED)[0]), 4096)[1] == (1999, 1999)


def test_colliding_tags():
    entry, tag = set_chain_pairs()
    keys = hk.pair_key(entry, tag)
    ones = U((1 << SET_BITS) - 1)
    assert len(np.unique(keys)) == len(keys) == SET_CHAIN == 240 and (tag >= 0).all() and RETIRED == CHAIN_TAGS[3]
    assert ((hk.mix(keys) & ones) == ones).all()
    for cap in (1024, 2048, 4096):
        m = hk.table_model(keys, cap)
        assert m["run"] == (cap - 1, len(keys)) and m["min_disp"] == m["min_wraps"] == len(keys) - 1


# ---- the hostile map ------------------------------------------------------------------------------------------------------
def test_hostile_map_conditions():
    """what the GPU test asserts again from the engine's own table_slots: enough of the pieces' entries, and of the absent
    cells the queries probe, home inside the chain's run"""
    vm, cc, pc, da, db = build_map()
    assert vm.M == L + len(pc) and 290 <= len(pc) <= 310 and 2 * (L + len(db)) > 1024
    m, keys = layout(vm, CAP_PIECES)
    start, length = m["run"]
    assert start <= CAP_PIECES - 1 and length >= L and m["min_disp"] >= L - 1 and m["min_wraps"] >= L - 1
    inside = hk.homes_in_run(hk.cell_key(pc), CAP_PIECES, m["run"])
    absent = absent_probed(np.concatenate([cc, pc]), pc)
    absent_in = hk.homes_in_run(hk.cell_key(absent), CAP_PIECES, m["run"])
    print("run", m["run"], "pieces in run", int(inside.sum()), "absent probed", len(absent), "in run", int(absent_in.sum()))
    assert int(inside.sum()) >= MIN_PIECES_IN_RUN and int(absent_in.sum()) >= MIN_ABSENT_IN_RUN


def _records_of(vm):
    return {"xyz": vm.rec["xyz"], "multiplicity": vm.rec["multiplicity"], "tag": vm.rec["tag"], "pixel": vm.rec["pixel"]}


def test_restatements_agree_with_their_scalar_twins_on_the_hostile_map():
    vm, cc, pc, da, db = build_map()
    rec = _records_of(vm)
    flags = (vm.rec["multiplicity"] >= 2).astype(np.uint8)
    m, _ = layout(vm, CAP_PIECES)
    displaced = pc[hk.homes_in_run(hk.cell_key(pc), CAP_PIECES, m["run"])]
    absent = absent_probed(np.concatenate([cc, pc]), pc)
    absent = absent[hk.homes_in_run(hk.cell_key(absent), CAP_PIECES, m["run"])]
    for c in (6, 18, 26):
        res = comp_both(rec, flags, VOXEL, connectivity=c, min_size=4)
        assert res["members"] == vm.M
    comp_both(rec, flags, VOXEL, connectivity=26, min_multiplicity=2, require_published=True)
    O, P = cast_rays(cc, pc, displaced, absent)
    for kw in (dict(), dict(start_margin=1), dict(end_margin=1), dict(start_margin=1, end_margin=1, min_multiplicity=2)):
        res, _ = cast_both(rec, flags, O, P, VOXEL, **kw)
    assert res["rays_total"] == len(O)
    tags, Tcw = camera_table()
    for r in (1, 2):
        normals_both(rec, flags, VOXEL, radius=r, tags=tags, Tcw=Tcw)
    ol = vo.ObservationLog()
    vi.import_observations(ol, vm.M, *set_chain_pairs())
    vi.import_observations(ol, vm.M, *piece_pairs(len(pc)))
    for margin in (0, 1):
        res = recarve_both(vm, ol, tags, Tcw, end_margin=margin)
    assert res["rays_skipped"] > 0 and res["cells_hit"] > 0 and res["pairs_unposed"] > 0


def mesh_normal_sets(M, estimated):
    """the normals the GPU test stitches the hostile map with: the radius-1 normals estimated on it, then one axis after the
    other"""
    return [("estimated", estimated)] + [("axis %d" % ax, axis_normals(M, ax)) for ax in range(3)]


def test_mesh_probes_walk_the_chain():
    """the cells sdm_vmap_mesh looks up from its owners include, at every capacity the GPU test reaches, cells that hold an
    entry and cells that hold none with their home inside the chain's run; every set of normals gives triangles, and the
    restatement agrees with its scalar twin on the hostile map"""
    from test_vmap_mesh_cpu import both as mesh_both
    vm, cc, pc, da, db = build_map()
    rec = _records_of(vm)
    tags, Tcw = camera_table()
    sets = mesh_normal_sets(vm.M, vn.normals(rec, None, VOXEL, radius=1, tags=tags, Tcw=Tcw)["normal"])
    for what, normal in sets:
        res = mesh_both(rec, None, VOXEL, normal)
        assert res["triangles"] > 0 and res["members"] == vm.M, what
    for cap in (CAP_PIECES, 2 * CAP_PIECES, 4 * CAP_PIECES):
        m, keys = layout(vm, cap)
        present, absent = [], []
        for what, normal in sets:
            p, a, _ = mesh_probes(rec, None, normal, keys, cap, m["run"])
            present.append(p)
            absent.append(a)
        have = (len(np.unique(np.concatenate(present), axis=0)), len(np.unique(np.concatenate(absent), axis=0)))
        print("capacity", cap, "run", m["run"], "probed in run: present, absent", have)
        assert have[0] >= MIN_MESH_PRESENT_IN_RUN and have[1] >= MIN_MESH_ABSENT_IN_RUN, (cap, have)


# ---- the keyframe the GPU test integrates into the hostile map --------------------------------------------------------------
KF_TAG = 7
KF_K = np.array([1, 1, 2, 2], F)  # pixel (x, y) at rho = 1 / Z is the point O + (Z (x - 2), Z (y - 2), Z)
KF_W, KF_H = 32, 24


def keyframe():
    """(image, pose, rho, sigma): dense over the patch at Z = 1 and 2 -- its two layers -- and sparse beside it; sigmas below,
    at and above the pieces' 0.004"""
    rng = np.random.default_rng(17)
    pose = np.eye(4, dtype=F)[:3].copy()
    pose[:, 3] = -(OFF + np.array([0.5, 0.5, -0.75])).astype(F)
    dense = np.zeros((KF_H, KF_W), bool)
    dense[2:12, 2:15] = True
    keep = rng.random((KF_H, KF_W)) < np.where(dense, 0.85, 0.08)
    keep[:2], keep[-2:], keep[:, :2], keep[:, -2:] = False, False, False, False  # (a border pixel's stored xyz is the origin,
    # not its back-projection: a repose would move it)
    rho = np.where(keep, rng.choice(np.array([1.0, 1.0, 0.5], F), (KF_H, KF_W)), 0).astype(F)
    sigma = rng.choice(np.array([0.002, 0.004, 0.006], F), (KF_H, KF_W))
    return rng.integers(0, 256, (KF_H, KF_W)).astype(np.uint8), pose, rho, sigma


def test_keyframe_meets_the_pieces_without_growing_the_table():
    import vmap_repose_np as vrp
    vm, cc, pc, da, db = build_map()
    _, pose, rho, sigma = keyframe()
    ys, xs = np.nonzero(rho > 1e-6)
    xyz = vrp.pointset_pixels(KF_K, pose, xs, ys, rho[ys, xs])
    assert not ((xs < 2) | (ys < 2) | (xs >= KF_W - 2) | (ys >= KF_H - 2)).any()
    cloud = {"xyz": xyz, "pixel": (ys << 16 | xs).astype(np.uint32), "rho_sigma": np.stack([rho[ys, xs], sigma[ys, xs]], 1),
             "intensity": np.zeros(len(xs), np.uint8)}
    M = vm.M
    d = vm.integrate(cloud, np.full(len(xs), KF_TAG, np.int32))
    print(d["plain_total"], d["created"], d["updated"])
    assert 100 < d["plain_total"] < 260 and d["created"] > 20 and d["updated"] > 5 and d["dropped"] == 0
    assert 2 * (M + d["plain_total"]) <= CAP_PIECES  # the a-priori bound of the call does not grow the table


# ---- the per-call table of sdm_extract_points_voxel* -----------------------------------------------------------------------
PC_W = PC_H = 8                      # the smallest image an engine accepts
PC_K = np.array([1, 1, 4, 4], F)
PC_CHAIN, PC_EXTRA, PC_SEED = 128, 6, 2


def per_call_case():
    """One point per keyframe on a colliding cell: identity rotation, the one supported pixel at the principal point with
    rho 1, and the camera centre one unit below the cell's centre.  PC_EXTRA further slots put a second point into the
    chain's first cells with a lower, an equal and a higher sigma."""
    cells, centre, _ = hk.colliding_cells(PC_CHAIN, PC_SEED, voxel=VOXEL)
    of = np.concatenate([np.arange(PC_CHAIN), np.arange(PC_EXTRA)])
    S = len(of)
    Tcw = np.zeros((S, 3, 4), F)
    Tcw[:, :, :3] = np.eye(3, dtype=F)
    Tcw[:, :, 3] = np.array([0, 0, 1], F) - centre[of]   # the centre of the camera is the cell's centre - (0, 0, 1)
    rho = np.zeros((PC_H, PC_W), F)
    rho[4, 4] = 1
    sigma = np.zeros((S, PC_H, PC_W), F)
    sigma[:PC_CHAIN, 4, 4] = 0.004
    sigma[PC_CHAIN:, 4, 4] = np.array([0.002, 0.004, 0.006], F)[np.arange(PC_EXTRA) % 3]
    rows = np.stack([(np.arange(S) + 1) % S, (np.arange(S) + 2) % S], 1).astype(np.int32)
    rows[:PC_EXTRA, 1] = PC_CHAIN + np.arange(PC_EXTRA)   # the twins see each other
    rows[PC_CHAIN:, 1] = np.arange(PC_EXTRA)
    return {"S": S, "chain": PC_CHAIN, "cells": cells, "of": of, "Tcw": Tcw.reshape(S, 12), "rho": rho, "sigma": sigma,
            "rows": rows, "im": np.zeros((PC_H, PC_W), np.uint8)}


def per_call_points(oracle, case):
    """the plain cloud the calls must see, from the oracle's point-set pass: float32 [S, 3]"""
    zeros = np.zeros((PC_H, PC_W), F)
    out = np.zeros((case["S"], 3), F)
    for s in range(case["S"]):
        kf = oracle.keyframe(case["im"], zeros, zeros, 1.0, PC_K, case["Tcw"][s].reshape(3, 4))
        out[s] = oracle.pointset(kf, case["rho"]).reshape(PC_H, PC_W, 3)[4, 4]
    return out


def per_call_capacity(T):
    """the slots of the table the host code makes for T plain points: at least 1024, at least 2 T"""
    cap = 1024
    while cap < 2 * T:
        cap *= 2
    return cap


def test_per_call_points_form_the_chain(oracle):
    """binary32 pose arithmetic places every point on its cell's centre over the whole cell range (43 free hash bits): the
    oracle's points, not the intent, have the chain's keys"""
    case = per_call_case()
    xyz = per_call_points(oracle, case)
    assert xyz.tobytes() == hk.centres(case["cells"][case["of"]], VOXEL).tobytes()
    keys = hk.restated_key(xyz, VOXEL)
    assert (keys == hk.cell_key(case["cells"])[case["of"]]).all() and (np.abs(case["cells"]).max(0) > 1 << 19).all()
    cap = per_call_capacity(case["S"])
    m = hk.table_model(np.unique(keys), cap)
    assert cap == 1024 and m["run"] == (cap - 1, PC_CHAIN) and (m["min_disp"], m["min_wraps"]) == (PC_CHAIN - 1, PC_CHAIN - 1)
