"""GPU: every kernel that probes one of the voxel map's hash tables, on colliding keys and long probes that cross the
table's end (tests/hostile_keys.py, tests/test_hostile_keys_cpu.py) -- each call compared for equality (floats as bits) with
its existing restatement fed the engine's own records, through the helpers of the call's own GPU test.  No expectation is
written here; what is new is the input, and the device's witness that the layout happened: sdm_selftest(16) / (17) / (18)
report the largest displacement and the number of keys below their home in the map's table, the observation set and the
per-call table, and must reach the bounds of the CPU model (table_model), which hold for every insertion order.

The map's sequence runs at the capacity the two imports leave (2048 slots, L = 384: the chain's run covers a fifth of the
table), so every later call -- integrate, observations, recarve, casts, classify, components, normals, the mesh, the rebuilds
of repose and retire -- meets it there; the two further growths come last, each followed by the re-import, the witness and the
read-only queries at the new capacity."""
import numpy as np
import pytest

import hostile_keys as hk
import test_hostile_keys_cpu as hm
from test_gpu_carve import centres_of, run as freespace_run
from test_gpu_extract import ALL, ESTATE
from test_gpu_vmap import step as integrate_step
from test_gpu_vmap_cast import cast, render
from test_gpu_vmap_class import Mirror, full_state, step as classify_step
from test_gpu_vmap_comp import comp
from test_gpu_vmap_import import check_import, check_pairs
from test_gpu_vmap_normals import run as normals_run
from test_gpu_vmap_recarve import Model
from test_gpu_vmap_repose import check_repose, pad_evidence
from test_gpu_vmap_retire import check_retire
from test_gpu_voxcam import run as voxcam_run
from test_gpu_voxel import run as voxel_run
from test_vmap_import_cpu import part

pytestmark = pytest.mark.gpu
F = np.float32
L, VOXEL = hm.L, hm.VOXEL
KF_TAG, KF_K = hm.KF_TAG, hm.KF_K
KF_KW = dict(source=0, max_sigma=0.01)
_first_run = {}


class Recarver(Model):
    """test_gpu_vmap_recarve.Model on a mirror that other calls change too"""

    def __init__(self, eng, ref):
        self.eng, self.voxel, self.ref = eng, ref.voxel, ref

    vm = property(lambda self: self.ref.vm)
    ol = property(lambda self: self.ref.ol)
    ev = property(lambda self: self.ref.ev, lambda self, v: setattr(self.ref, "ev", v))


def witness(eng, which, model, what):
    """the device's two figures against the model's bounds, which hold for every order of the compare-and-swaps"""
    disp, wraps = eng.selftest(which)
    print("%s: selftest %d displacement %d wrapped %d; model run %r, bounds %d %d" %
          (what, which, disp, wraps, model["run"], model["min_disp"], model["min_wraps"]))
    assert disp >= model["min_disp"] and wraps >= model["min_wraps"], (what, disp, wraps, model["min_disp"], model["min_wraps"])
    free = np.flatnonzero(~model["occupied"])   # no key is further from home than the longest run of occupied slots
    assert disp < np.diff(np.append(free, free[0] + len(model["occupied"]))).max() - 1 and wraps <= model["run"][1], what
    return disp, wraps


def map_model(eng, ref):
    """the model of the map's table at the engine's own capacity (the occupied set is independent of the insertion order)"""
    return hk.table_model(ref.vm.keys.astype(np.uint64), eng.vmap_info()["table_slots"])


def kf_upload(eng):
    """the small keyframe of tests/test_hostile_keys_cpu.py: about 170 points on and beside the pieces' cells"""
    im, pose, rho, sigma = hm.keyframe()
    eng.upload_image(0, im, KF_K, pose)
    eng.upload_depth(0, rho, sigma)
    eng.pointset([0], source=0)
    return pose


def queries(eng, ref, chain_cells, pieces, what, out, need=(40, 8, 40),
            need_mesh=(hm.MIN_MESH_PRESENT_IN_RUN, hm.MIN_MESH_ABSENT_IN_RUN)):
    """the read-only queries at the table as it stands: casts with both margins, a render, components, normals, the mesh.
    need: the least chain cells, displaced pieces and absent cells the casts end in; need_mesh: the least cells with and
    without an entry, homing inside the chain's run, among those the mesh looks up (tests/test_hostile_keys_cpu.py has the
    model's counts at every capacity)"""
    m = map_model(eng, ref)
    cap = eng.vmap_info()["table_slots"]
    live = chain_cells[np.isin(hk.cell_key(chain_cells), ref.vm.keys.astype(np.uint64))]
    displaced = pieces[hk.homes_in_run(hk.cell_key(pieces), cap, m["run"])]
    present = hk.key_cells(ref.vm.keys.astype(np.uint64))
    absent = hm.absent_probed(present, pieces, 2)
    absent = absent[hk.homes_in_run(hk.cell_key(absent), cap, m["run"])]
    have = (len(live), len(displaced), len(absent))
    assert all(h >= n for h, n in zip(have, need)), (what, have, need)
    O, P = hm.cast_rays(live, pieces, displaced, absent)
    for i, kw in enumerate((dict(), dict(start_margin=1), dict(end_margin=1), dict(start_margin=1, end_margin=1, min_multiplicity=2))):
        got = cast(eng, O, P, "%s cast %r" % (what, kw), device=bool(i & 1), **kw)
        out.append(got["hit_id"] if not hasattr(got["hit_id"], "cpu") else got["hit_id"].cpu().numpy())
    assert got["rays_total"] == len(O)
    at = render(eng, hm.pose_at(hm.OFF + np.array([8.0, 5.0, -1.5])), 9, 7, what + " render")
    assert at["rays_hit"] > 0
    out.append(at["hit_rho"])
    for c in (6, 18, 26):
        out.append(comp(eng, "%s components %d" % (what, c), connectivity=c, min_size=4)["label"])
    tags, Tcw = hm.camera_table()
    estimated = {}
    for r in (1, 2):
        estimated[r] = normals_run(eng, "%s normals %d" % (what, r), radius=r, tags=tags, Tcw=Tcw)["normal"]
        out.append(estimated[r])
    # the mesh: up to 21 lookups per entry, from the radius-1 normals just computed and along each axis in turn; of the
    # cells it looks up, some that hold an entry and some that hold none home inside the chain's run
    from test_gpu_vmap_mesh import host as mesh_host, run as mesh_run   # (that module imports this one)
    rec = {f: ref.vm.rec[f] for f in ("xyz", "multiplicity")}
    flags = ref.cl.flags(ref.vm.M) if ref.cl.calls else None
    inside = [[], []]
    for i, (name, normal) in enumerate(hm.mesh_normal_sets(ref.vm.M, estimated[1])):
        p, a, exp = hm.mesh_probes(rec, flags, normal, ref.vm.keys.astype(np.uint64), cap, m["run"])
        inside[0].append(p)
        inside[1].append(a)
        got = mesh_run(eng, "%s mesh, %s normals" % (what, name), normal, device=bool(i & 1))
        assert got["triangles"] == exp["triangles"] > 0, (what, name, got["triangles"], exp["triangles"])
        out.append(mesh_host(got["tri"]))
    have = tuple(len(np.unique(np.concatenate(x), axis=0)) for x in inside)
    print("%s: of the cells the mesh looks up, %d with and %d without an entry home inside the run %r of %d slots" %
          ((what,) + have + (m["run"], cap)))
    assert all(h >= n for h, n in zip(have, need_mesh)), (what, have, need_mesh)


def reimport(eng, ref, rec, dst, what, chunk):
    """the same records again: every one lands in its old entry, none is created, the multiplicities add up"""
    before = ref.vm.rec["multiplicity"].astype(np.int64).copy()
    n = len(rec["xyz"])
    for a in range(0, n, chunk):
        got, _ = check_import(eng, ref, part(rec, a, min(a + chunk, n)), "%s %d" % (what, a))
        assert got["created"] == 0 and got["dropped"] == 0
        np.testing.assert_array_equal(got["dst_ids"], dst[a:a + chunk])
    add = np.bincount(dst.astype(np.int64), weights=rec["multiplicity"].astype(np.int64), minlength=ref.vm.M).astype(np.int64)
    np.testing.assert_array_equal(ref.vm.rec["multiplicity"].astype(np.int64), before + add)
    pad_evidence(ref)


def sequence(pkg):
    """the whole life of the hostile map; returns every fetched array in order"""
    out = []
    eng = pkg.Engine(32, 24, 1)
    try:
        with pytest.raises(pkg.SdmError) as err:
            eng.selftest(16)
        assert err.value.code == ESTATE
        with pytest.raises(pkg.SdmError) as err:
            eng.selftest(17)
        assert err.value.code == ESTATE
        eng.vmap_open(VOXEL)
        ref = Mirror(VOXEL)
        assert eng.selftest(16) == (0, 0) and eng.selftest(17) == (0, 0)
        chain_cells, ra = hm.chain_records()
        pieces, rb = hm.piece_records()

        # import: (a) the chain alone, then (b) the pieces -- the first growth, with the chain in place
        ga, _ = check_import(eng, ref, ra, "the chain")
        assert ga["created"] == L and eng.vmap_info()["table_slots"] == 1024
        m = map_model(eng, ref)
        assert m["run"] == (1023, L) and (m["min_disp"], m["min_wraps"]) == (L - 1, L - 1)
        assert witness(eng, 16, m, "the chain alone") == (L - 1, L - 1)   # a chain alone: exact for every order
        gb, _ = check_import(eng, ref, rb, "the pieces")
        info = eng.vmap_info()
        assert gb["created"] == len(pieces) and info["table_slots"] == hm.CAP_PIECES and info["rehashes"] == 1
        m = map_model(eng, ref)
        inside = hk.homes_in_run(hk.cell_key(pieces), hm.CAP_PIECES, m["run"])
        absent = hm.absent_probed(np.concatenate([chain_cells, pieces]), pieces)
        absent_in = hk.homes_in_run(hk.cell_key(absent), hm.CAP_PIECES, m["run"])
        assert int(inside.sum()) >= hm.MIN_PIECES_IN_RUN and int(absent_in.sum()) >= hm.MIN_ABSENT_IN_RUN
        assert m["min_disp"] >= L - 1 and m["min_wraps"] >= L - 1
        witness(eng, 16, m, "chain and pieces")
        both = {f: np.concatenate([ra[f], rb[f]]) for f in ra}
        dst = np.concatenate([ga["dst_ids"], gb["dst_ids"]])
        reimport(eng, ref, both, dst, "the same records again", 256)
        assert eng.vmap_info()["table_slots"] == hm.CAP_PIECES
        out.append(full_state(eng))

        # integrate: a small keyframe over the patch
        pose = kf_upload(eng)
        d = integrate_step(eng, ref.vm, [0], [KF_TAG], "the keyframe", **KF_KW)
        pad_evidence(ref)
        assert 100 < d["plain_total"] < 260 and d["created"] > 20 and d["updated"] > 5 and d["dropped"] == 0
        assert eng.vmap_info()["table_slots"] == hm.CAP_PIECES
        witness(eng, 16, map_model(eng, ref), "after the integrate")

        # the observation log: colliding pairs first, then the same again, then ordinary pairs that grow the set
        entry, tag = hm.set_chain_pairs()
        n_chain = len(entry)
        got = check_pairs(eng, ref, entry, tag, None, "colliding pairs")
        assert got["created"] == n_chain and got["rejected"] == 0 and eng.vmap_obs_info()["table_slots"] == 1024
        sm = hk.table_model(hk.pair_key(ref.ol.entry, ref.ol.tag), 1024)
        assert witness(eng, 17, sm, "the set's chain alone") == (n_chain - 1, n_chain - 1)
        got = check_pairs(eng, ref, entry[::-1].copy(), tag[::-1].copy(), None, "the colliding pairs again", device=True)
        assert got["created"] == 0 and got["rejected"] == 0 and eng.vmap_obs_info()["observations"] == n_chain
        got = check_pairs(eng, ref, *hm.piece_pairs(len(pieces)), None, "ordinary pairs")
        oinfo = eng.vmap_obs_info()
        assert got["created"] > 500 and oinfo["table_slots"] == 2048 and oinfo["rehashes"] == 1
        sm = hk.table_model(hk.pair_key(ref.ol.entry, ref.ol.tag), 2048)
        assert sm["min_disp"] >= n_chain - 1 and sm["min_wraps"] >= n_chain - 1
        witness(eng, 17, sm, "the set after its growth")
        check_pairs(eng, ref, ref.ol.entry[::3].copy(), ref.ol.tag[::3].copy(), None, "a third of the log again")
        assert eng.vmap_obs_info()["observations"] == ref.ol.E

        # recarve over the whole log, casts and the render, classify, components, normals
        rc = Recarver(eng, ref)
        tags, Tcw = hm.camera_table()
        for margin in (0, 1):
            got = rc.recarve(tags, Tcw, "recarve margin %d" % margin, reset=True, end_margin=margin)
        assert got["cells_hit"] > 0 and got["rays_skipped"] > 0 and got["pairs_unposed"] > 0 and got["ends_hit"] > 500
        queries(eng, ref, chain_cells, pieces, "first", out)
        got, _ = classify_step(eng, ref, dict(min_neighbours=3), True, "classify")
        assert 0 < got["accepted"] < ref.vm.M
        classify_step(eng, ref, dict(min_neighbours=26, min_multiplicity=2), True, "classify again")
        out.append(full_state(eng))

        # repose with the keyframe's own pose: the rebuild at the same capacity reproduces the map
        M = ref.vm.M
        got, exp = check_repose(eng, ref, [KF_TAG], [KF_K], [pose], 1, "host", "repose")
        assert got["moved"] == 0 and got["voxels"] == M and got["reposed"] > 20 and (got["remap"] == np.arange(M)).all()
        assert eng.vmap_info()["table_slots"] == hm.CAP_PIECES
        witness(eng, 16, map_model(eng, ref), "after the repose")
        witness(eng, 17, hk.table_model(hk.pair_key(ref.ol.entry, ref.ol.tag), eng.vmap_obs_info()["table_slots"]), "the set after the repose")
        rc.recarve(tags, Tcw, "recarve after the repose", reset=True)
        queries(eng, ref, chain_cells, pieces, "after the repose", out)

        # retire one of the chain's four tags, winner mode, committed: a quarter of the chain goes, the rest still wraps.
        # The entries behind the first dropped one are renumbered, so of the set's chain the pairs of entries 0 .. 2 stay
        got, exp = check_retire(eng, ref, [hm.RETIRED], "winner", 1, "host", True, "retire")
        assert got["dropped"] == L // 4 and got["voxels"] == M - L // 4 and got["removed"] == 0
        m = map_model(eng, ref)
        assert m["min_wraps"] >= L - L // 4 - 1
        witness(eng, 16, m, "after the retire")
        sm = hk.table_model(hk.pair_key(ref.ol.entry, ref.ol.tag), eng.vmap_obs_info()["table_slots"])
        assert sm["min_wraps"] >= hm.SET_HEAD[0] * hm.SET_HEAD[1] - 1
        witness(eng, 17, sm, "the set after the retire")
        rc.recarve(tags, Tcw, "recarve after the retire", reset=True)
        queries(eng, ref, chain_cells, pieces, "after the retire", out)
        out.append(full_state(eng))

        # growth: two more rehashes with what is left of the chain in place
        for k in (0, 1):
            before = eng.vmap_info()
            cells, rec = hm.growth_records(k)
            got, _ = check_import(eng, ref, rec, "growth %d" % k)
            info = eng.vmap_info()
            assert got["created"] == len(cells) and info["rehashes"] == before["rehashes"] + 1
            assert info["table_slots"] == 2 * before["table_slots"]
            pad_evidence(ref)
            m = map_model(eng, ref)
            assert m["min_wraps"] >= L - L // 4 - 1
            witness(eng, 16, m, "after growth %d" % k)
        assert eng.vmap_info()["table_slots"] == 8192
        mine = eng.vmap_fetch()
        reimport(eng, ref, {f: np.array(mine[f]) for f in hm.RECORD_FIELDS}, np.arange(ref.vm.M, dtype=np.uint32), "every entry again", 512)
        assert eng.vmap_info()["table_slots"] == 8192
        witness(eng, 16, map_model(eng, ref), "after the last import")
        rc.recarve(tags, Tcw, "recarve after the growth", reset=True)
        queries(eng, ref, chain_cells, pieces, "after the growth", out, need=(40, 1, 10))
        out.append(full_state(eng))
    finally:
        eng.close()
    return out


def flat(x, into):
    if isinstance(x, dict):
        for k in sorted(x):
            flat(x[k], into)
    elif isinstance(x, (tuple, list)):
        for v in x:
            flat(v, into)
    else:
        into.append(np.asarray(x))
    return into


# 1. the persistent map's table and the observation set
def test_hostile_map_sequence(pkg, gpu_ok):
    _first_run["out"] = flat(sequence(pkg), [])
    assert len(_first_run["out"]) > 100


# 2. determinism: the whole sequence again; every fetched array is equal
def test_hostile_map_sequence_is_deterministic(pkg, gpu_ok):
    first = _first_run.get("out") or flat(sequence(pkg), [])
    again = flat(sequence(pkg), [])
    assert len(first) == len(again)
    for i, (a, b) in enumerate(zip(first, again)):
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), i


# 3. the per-call table of sdm_extract_points_voxel, _cameras and _freespace
def test_per_call_table(pkg, oracle, gpu_ok):
    case = hm.per_call_case()
    S, chain = case["S"], case["chain"]
    eng = pkg.Engine(hm.PC_W, hm.PC_H, S, max_neighbours=2)
    try:
        with pytest.raises(pkg.SdmError) as err:
            eng.selftest(18)
        assert err.value.code == ESTATE
        for s in range(S):
            eng.upload_image(s, case["im"], hm.PC_K, case["Tcw"][s])
            eng.upload_depth(s, case["rho"], case["sigma"][s])
        slots = list(range(S))
        eng.pointset(slots, source=0)
        kw = dict(source=0, max_sigma=0.01)
        expect = hm.per_call_points(oracle, case)
        plain = eng.extract_points(slots, fields=ALL, **kw)
        assert plain["xyz"].tobytes() == expect.tobytes() and np.diff(plain["offsets"]).tolist() == [1] * S
        keys = hk.restated_key(plain["xyz"], VOXEL)
        cap = hm.per_call_capacity(S)
        m = hk.table_model(np.unique(keys), cap)
        assert cap == 1024 and m["run"] == (cap - 1, chain) and (m["min_disp"], m["min_wraps"]) == (chain - 1, chain - 1)
        for order, what in ((slots, "in order"), (slots[::-1], "reversed")):
            got, _ = voxel_run(eng, order, VOXEL, "per-call table " + what, **kw)
            assert len(got["source_index"]) == chain and int(got["multiplicity"].max()) == 2
            assert witness(eng, 18, m, "per-call table " + what) == (chain - 1, chain - 1)
        rows = case["rows"]
        got, exp, sup = voxcam_run(eng, slots, rows, VOXEL, "per-call table cameras", **kw)
        assert got["cam_total"] >= S
        witness(eng, 18, m, "per-call table cameras")
        centres = centres_of({s: case["Tcw"][s] for s in range(S)})
        for margin in (0, 1):
            got, _, ref = freespace_run(eng, slots, rows, VOXEL, centres, margin, 4096, "per-call table free space", **kw)
            assert got["rays_total"] >= S
        witness(eng, 18, m, "per-call table free space")
    finally:
        eng.close()
