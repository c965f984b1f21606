"""CPU: tests/vmap_mesh_np.py (the restatement of sdm_vmap_mesh) tied array for array to a scalar loop that takes one owner and
one probe at a time; then the properties of the triangle list, what the mesh is on a plane (a manifold disc), on a crease and
on a shell (the measured edge valences), and pinned totals and digests on keyframe 0 of every golden fixture.
tests/test_gpu_vmap_mesh.py runs the engine on the same maps and normals."""
import functools
import hashlib

import numpy as np
import pytest

import golden_util as gu
import vmap_mesh_np as vm
import vmap_normals_np as vn
from test_vmap_comp_cpu import FILTERS, SMALL, small_case
from test_vmap_normals_cpu import FAR, GOLDEN_MIN_POINTS, GOLDEN_VOXEL, MAPS as NORMAL_MAPS, golden_kf0, tagged

F = np.float32
LIM = 1 << 20
NONE = vm.NONE
# every map the GPU test imports: section 27's crafted map and its random maps, section 28's plane, crease, line and shell
MAPS = {k: v for k, v in NORMAL_MAPS.items() if k != "exact"}
KINDS = ("estimated", "crafted")


@functools.lru_cache(maxsize=None)
def estimated_normals(name, filt=0):
    """the normals vmap_normals_np gives the map under FILTERS[filt], at radius 2, turned towards a camera far above"""
    case, voxel = MAPS[name]
    rec, flags = case()
    return vn.normals(rec, flags, voxel, tags=FAR[0], Tcw=FAR[1], radius=2, min_points=3, **FILTERS[filt])["normal"]


def crafted_normals(M, seed=0):
    """float32[M, 3]: entry i takes pattern (i + seed) % 20 over a random base -- a NaN in each slot and in all, all +0, all
    -0, mixed zeros, three and two equal magnitudes, a denormal alone and a tie of denormals, an infinity in a slot and in
    all, a negative dominant component on each axis, and the base itself"""
    rng = np.random.default_rng(500 + M + seed)
    n = rng.normal(size=(M, 3)).astype(F)
    tiny = np.float32(1e-45)
    for i in range(M):
        p = (i + seed) % 20
        x, y, z = n[i]
        s = abs(x) + F(0.5)
        n[i] = {0: (np.nan, y, z), 1: (x, np.nan, z), 2: (x, y, np.nan), 3: (np.nan, np.nan, np.nan), 4: (0.0, 0.0, 0.0),
                5: (-0.0, -0.0, -0.0), 6: (0.0, -0.0, 0.0), 7: (s, -s, s), 8: (-s, -s, s / 4), 9: (0.0, s, -s),
                10: (0.0, 0.0, tiny), 11: (-tiny, tiny, 0.0), 12: (np.inf, y, z), 13: (x, -np.inf, z),
                14: (np.inf, np.inf, -np.inf), 15: (-s - 1, y / 8, z / 8), 16: (x / 8, -s - 1, z / 8),
                17: (x / 8, y / 8, -s - 1)}.get(p, (x, y, z))
    return n


def normals_of(name, kind, filt=0):
    case, _ = MAPS[name]
    M = len(case()[0]["pixel"])
    return estimated_normals(name, filt) if kind == "estimated" else crafted_normals(M)


def scalar_mesh(rec, flags, voxel_size, normal, min_multiplicity=0, require_published=False, first=0, count=None):
    """the header's semantics once more: one owner, one probe at a time, cells as tuples in a dict"""
    xyz = np.asarray(rec["xyz"], F).reshape(-1, 3)
    M = len(xyz)
    count = M - first if count is None else count
    mult = np.asarray(rec["multiplicity"]).reshape(-1)
    inv = F(1.0) / F(voxel_size)
    member = [int(mult[i]) >= min_multiplicity and (not require_published or (flags is not None and int(flags[i]) != 0))
              for i in range(M)]
    cell = [tuple(int(np.floor(F(xyz[i, k] * inv))) for k in range(3)) for i in range(M)]
    where = {cell[i]: i for i in range(M)}
    probes = [0]

    def at(c):
        """the member of a cell, or None"""
        if min(c) < -LIM or max(c) >= LIM:
            return None
        probes[0] += 1
        j = where.get(c)
        return j if j is not None and member[j] else None

    def moved(c, axis, d):
        return tuple(c[k] + (d if k == axis else 0) for k in range(3))

    def step(c, ax, a):
        t = moved(c, ax, 1)
        for da in (0, -1, 1):
            kc = moved(t, a, da)
            k = at(kc)
            if k is not None:
                for _ in range(2):
                    lower = at(moved(kc, a, -1))
                    if lower is None:
                        break
                    k, kc = lower, moved(kc, a, -1)
                return k, kc
        return None, None

    tri = []
    owner_tris = np.zeros(count, np.uint8)
    corners = np.full((count, 3), NONE, np.int64)
    res = dict.fromkeys(vm.OUTS, 0)
    res["entries"] = count
    most = 0
    with np.errstate(invalid="ignore"):
        for e in range(count):
            i = first + e
            if not member[i]:
                continue
            res["members"] += 1
            n = [F(normal[e][k]) for k in range(3)]
            a = 0
            if abs(n[1]) > abs(n[a]):
                a = 1
            if abs(n[2]) > abs(n[a]):
                a = 2
            if not abs(n[a]) > 0:
                continue
            u, v = (a + 1) % 3, (a + 2) % 3
            probes[0] = 0
            if at(moved(cell[i], a, -1)) is not None:
                continue
            res["owners"] += 1
            Nu, cu = step(cell[i], u, a)
            Nv, cv = step(cell[i], v, a)
            C = None
            if Nu is not None:
                C, _ = step(cu, v, a)
            if C is None and Nv is not None:
                C, _ = step(cv, u, a)
            most = max(most, probes[0])
            corners[e] = [NONE if x is None else x for x in (Nu, Nv, C)]
            if Nu is not None and Nv is not None and C is not None:
                mine = [(i, Nu, C), (i, C, Nv)]
                res["quads"] += 1
            elif Nu is not None and Nv is not None:
                mine = [(i, Nu, Nv)]
            elif Nu is not None and C is not None:
                mine = [(i, Nu, C)]
            elif Nv is not None and C is not None:
                mine = [(i, C, Nv)]
            else:
                mine = []
            if len(mine) == 1:
                res["singles"] += 1
            if n[a] < 0:
                mine = [(p, r, q) for p, q, r in mine]
            owner_tris[e] = len(mine)
            tri.extend(mine)
    tri = np.array(tri, np.uint32).reshape(-1, 3)
    used = np.zeros(M, np.uint8)
    used[tri.reshape(-1)] = 1
    res["triangles"], res["vertices"] = len(tri), int(used.sum())
    res.update(tri=tri, owner_tris=owner_tris, vertex_used=used, corners=corners, most_probes=most)
    return res


def same(a, b, what):
    for f in vm.ARRAYS:
        assert a[f].dtype == b[f].dtype == vm.DTYPES[f] and a[f].shape == b[f].shape, (what, f, a[f].shape, b[f].shape)
        assert a[f].tobytes() == b[f].tobytes(), (what, f)
    assert (a["corners"] == b["corners"]).all(), what
    assert {f: a[f] for f in vm.OUTS} == {f: b[f] for f in vm.OUTS}, what


def both(rec, flags, voxel, normal, **kw):
    a = vm.mesh(rec, flags, voxel, normal, **kw)
    b = scalar_mesh(rec, flags, voxel, normal, **kw)
    same(a, b, repr(kw))
    assert b["most_probes"] <= 21   # 1 + 4 x (3 + 2)
    a["most_probes"] = b["most_probes"]
    return a


@functools.lru_cache(maxsize=None)
def tied(name, kind):
    """the map's mesh without a filter, tied to the scalar loop"""
    case, voxel = MAPS[name]
    rec, flags = case()
    return both(rec, flags, voxel, normals_of(name, kind))


@pytest.mark.parametrize("name", sorted(MAPS))
def test_restatement_is_the_scalar_loop(name):
    case, voxel = MAPS[name]
    rec, flags = case()
    M = len(rec["pixel"])
    for kind in KINDS:
        assert tied(name, kind)["entries"] == M
    both(rec, flags, voxel, estimated_normals(name, 1), **FILTERS[1])
    both(rec, flags, voxel, estimated_normals(name, 3), **FILTERS[3])
    both(rec, flags, voxel, crafted_normals(M, 7), **FILTERS[2])
    none = both(rec, None, voxel, estimated_normals(name), require_published=True)   # no flag: no member
    assert none["members"] == 0
    if M > 3:
        both(rec, flags, voxel, normals_of(name, "estimated")[1:M - 2], first=1, count=M - 3)
        both(rec, flags, voxel, crafted_normals(M, 3)[2:], first=2)


def test_inputs_hold_every_kind_of_case():
    seen = dict.fromkeys(vm.STATS, 0)
    most = 0
    for name in MAPS:
        for kind in KINDS:
            res = tied(name, kind)
            most = max(most, res["most_probes"])
            for k, v in res["stats"].items():
                seen[k] += v
    print(seen, most)
    assert all(v > 0 for v in seen.values()), seen
    # The header's bound is 21 = 1 + 4 x (3 + 2).  No input reaches it: a hit at da = +1 has found the cells at 0 and -1
    # without a member, so its first probe down fails (4 probes); a hit at -1 takes 2 + 2, a hit at 0 takes 1 + 2, a miss 3;
    # and C's second path runs only after a first that missed: 1 + 4 + 4 + 3 + 4 = 16.  Measured over these maps: 15.
    assert 12 <= most <= 16, most
    # and where they are expected: the crafted map's cells at the ends of the range
    rec, _ = tagged(small_case())
    a = SMALL["last cells"][0]
    up = np.tile(np.array([[1, 0, 0]], F), (2, 1))
    assert vm.mesh(rec, None, 1.0, up, first=a, count=2)["stats"]["clipped"] > 0
    a = SMALL["z into y"][0]   # the pair an aliasing key would join: neither sees the other
    res = vm.mesh(rec, None, 1.0, np.tile(np.array([[1, 0, 0]], F), (2, 1)), first=a, count=2)
    assert res["owners"] == 2 and res["triangles"] == 0 and (res["corners"] == NONE).all()
    # the axis by hand
    n = np.array([[1, 1, 1], [1, -2, 2], [0, 1, -1], [np.nan, 5, 1], [1, np.nan, 9], [1e-45, 0, 0], [0, 0, 0], [-0.0, 0, 0],
                  [np.inf, np.inf, 1], [1, 2, -np.inf], [np.nan, np.nan, np.nan], [-3, 1, 2]], F)
    ax, na = vm.axis_of(n)
    assert ax.tolist() == [0, 1, 1, 0, 2, 0, 0, 0, 0, 2, 0, 0]
    with np.errstate(invalid="ignore"):
        assert (np.abs(na) > 0).tolist() == [True, True, True, False, True, True, False, False, True, True, False, True]
        assert (na < 0).tolist() == [False, True, False, False, False, False, False, False, False, True, False, True]


def columns_ok(rec, voxel, res, first=0):
    """the four corners of every owner lie in the four columns (cu, cv), (cu + 1, cv), (cu, cv + 1), (cu + 1, cv + 1)"""
    cell = vm.cells_of(rec["xyz"], voxel)
    for e in np.flatnonzero((res["corners"] != NONE).any(1)):
        a = int(res["axis"][e])
        u, v = (a + 1) % 3, (a + 2) % 3
        c = cell[first + e]
        for k, (du, dv) in zip(res["corners"][e], ((1, 0), (0, 1), (1, 1))):
            if k != NONE:
                assert (cell[k][u], cell[k][v]) == (c[u] + du, c[v] + dv) and abs(cell[k][a] - c[a]) <= 6, (e, k)


@pytest.mark.parametrize("name", sorted(MAPS))
def test_properties(name):
    case, voxel = MAPS[name]
    rec, flags = case()
    M = len(rec["pixel"])
    for kind in KINDS:
        res = tied(name, kind)
        nrm = normals_of(name, kind)
        tri, ot = res["tri"].astype(np.int64), res["owner_tris"]
        assert res["triangles"] == 2 * res["quads"] + res["singles"] == int(ot.sum()) == len(tri)
        assert res["owners"] <= res["members"] <= res["entries"] == M and res["vertices"] == int(res["vertex_used"].sum())
        assert int((ot == 2).sum()) == res["quads"] and int((ot == 1).sum()) == res["singles"]
        # three distinct ids, the owner first, the owners ascending and each with as many rows as owner_tris says
        assert (tri[:, 0] != tri[:, 1]).all() and (tri[:, 0] != tri[:, 2]).all() and (tri[:, 1] != tri[:, 2]).all()
        assert (np.diff(tri[:, 0]) >= 0).all() and (np.bincount(tri[:, 0], minlength=M) == ot).all()
        assert (tri < M).all() and sorted(set(tri.reshape(-1).tolist())) == np.flatnonzero(res["vertex_used"]).tolist()
        columns_ok(rec, voxel, res)
        # a sub-range is the slice: exactly the whole call's triangles whose owner lies in it, in order
        for first, count in ((0, 0), (1, 1), (1, 64), (63, 1), (65, 64), (M // 2, M - M // 2), (M, 0)):
            if first + count > M:
                continue
            sub = vm.mesh(rec, flags, voxel, nrm[first:first + count], first=first, count=count)
            inside = (tri[:, 0] >= first) & (tri[:, 0] < first + count)
            assert sub["tri"].tobytes() == res["tri"][inside].tobytes(), (first, count)
            assert sub["owner_tris"].tobytes() == ot[first:first + count].tobytes() and sub["entries"] == count
            assert (sub["vertex_used"] <= res["vertex_used"]).all()
        # a permutation of the ids relabels the triangle set
        perm = np.random.default_rng(3).permutation(M)
        inv = np.argsort(perm)
        rec2 = {f: a[perm] for f, a in rec.items()}
        other = vm.mesh(rec2, None if flags is None else flags[perm], voxel, nrm[perm])
        assert sorted(map(tuple, inv[tri].tolist())) == sorted(map(tuple, other["tri"].tolist()))
        assert other["vertex_used"].tobytes() == res["vertex_used"][perm].tobytes()
        assert [other[f] for f in vm.OUTS] == [res[f] for f in vm.OUTS]
        # every triangle of a member-filtered call has three members
        for flt in FILTERS[1:]:
            got = vm.mesh(rec, flags, voxel, nrm, **flt)
            ok = vm.stops(rec, flags, **flt)
            assert ok[got["tri"].reshape(-1)].all() and got["members"] == int(ok.sum())
        # a filter nothing passes gives nothing
        none = vm.mesh(rec, flags, voxel, nrm, min_multiplicity=5)
        assert [none[f] for f in vm.OUTS] == [M, 0, 0, 0, 0, 0, 0] and none["tri"].shape == (0, 3)
        assert not none["owner_tris"].any() and not none["vertex_used"].any()


def valences(tri):
    """(triangles per undirected edge, occurrences per directed edge) of a triangle list"""
    t = np.asarray(tri, np.int64)
    d = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    _, directed = np.unique(d, axis=0, return_counts=True)
    _, undirected = np.unique(np.sort(d, axis=1), axis=0, return_counts=True)
    return undirected, directed


def histogram(tri):
    und, _ = valences(tri)
    return {"1": int((und == 1).sum()), "2": int((und == 2).sum()), "3+": int((und >= 3).sum())}


def test_the_plane_is_a_manifold_disc():
    """section 28's tilted plane z = 0.3 x - 0.2 y + 4.25 of 24 x 24 columns: no edge with more than two triangles, no directed
    edge twice (the windings agree), and V - E + F = 1"""
    res = tied("plane", "estimated")
    und, directed = valences(res["tri"])
    print("plane", {f: res[f] for f in vm.OUTS}, histogram(res["tri"]))
    assert und.max() == 2 and directed.max() == 1
    V, E, Fc = res["vertices"], len(und), res["triangles"]
    assert V - E + Fc == 1, (V, E, Fc)
    # one vertex per column, one quad per cell of the 23 x 23 grid between them
    assert res["quads"] == 23 * 23 and res["singles"] == 0 and V == 576
    assert (res["axis"] == 2).all() and res["stats"]["flipped"] == 0
    # turned over, every triangle is wound the other way and the disc is the same
    rec, flags = MAPS["plane"][0]()
    over = vm.mesh(rec, flags, 0.05, -estimated_normals("plane"))
    assert over["tri"][:, [0, 2, 1]].tobytes() == res["tri"].tobytes() and over["stats"]["not flipped"] == 0


# the edge valences the restatement gives where the mesh is no disc: the fold of the crease, the seams between the shell's
# six axis patches.  Measured on these inputs, asserted as measured; the share of edges shared by three or more triangles is
# the figure to watch (crease 0, shell 2.8 % of 1190 edges).
MEASURED = {"crease": {"1": 79, "2": 994, "3+": 0}, "shell": {"1": 175, "2": 982, "3+": 33}}
TWICE = {"crease": 0, "shell": 76}   # directed edges that occur twice: two patches wound against each other along a seam


@pytest.mark.parametrize("name", sorted(MEASURED))
def test_measured_valences(name):
    res = tied(name, "estimated")
    got = histogram(res["tri"])
    _, directed = valences(res["tri"])
    print(name, {f: res[f] for f in vm.OUTS}, got, "directed edges twice", int((directed > 1).sum()))
    assert got == MEASURED[name] and int((directed > 1).sum()) == TWICE[name]
    assert got["3+"] <= 0.05 * sum(got.values()) and got["2"] >= 0.8 * sum(got.values())   # (measured: 0.028 and 0.825 at worst)


def digest(res):
    h = hashlib.sha256()
    for f in vm.ARRAYS:
        h.update(res[f].tobytes())
    return h.hexdigest()


# keyframe 0 of each golden fixture at voxel 0.02, the normals of section 28's recipe (radius 2, min_points 5, oriented by
# keyframe 0's pose): the seven totals and the SHA-256 of tri | owner_tris | vertex_used, as the restatement gives them
PINNED = {"plane_160x120_n7": ((516, 516, 489, 256, 73, 585, 485), "2bbd086eb2f6b2deb05c928e6e73dbb042cd3f90a18eb7ad718109a60960af02"),
          "plane_64x48_n7": ((689, 689, 688, 417, 168, 1002, 685), "878e6ac655fb4bd4782329655d5228ff664e526c6a5bff3cd0beedde561c8383"),
          "plane_96x80_n20": ((345, 345, 321, 149, 56, 354, 318), "fd57828b6f078ce4d1aa86653dd08da1b1d71d3715eba6bd09f4dcdc55fd325c"),
          "strip_roll_160x120_n7": ((599, 599, 517, 196, 102, 494, 485), "69417ff8998a7e5c52252ebf61fc1c18bbcf7b2bb2fbcfc6c4680267fd1378b6")}


@pytest.mark.parametrize("name", gu.fixture_names())
def test_golden_fixture_totals(name):
    rec, (tags, Tcw) = golden_kf0(name)
    nrm = vn.normals(rec, None, GOLDEN_VOXEL, tags, Tcw, radius=2, min_points=GOLDEN_MIN_POINTS)["normal"]
    res = vm.mesh(rec, None, GOLDEN_VOXEL, nrm)
    got = (tuple(res[f] for f in vm.OUTS), digest(res))
    print(name, got, histogram(res["tri"]))
    assert res["triangles"] > 0 and res["vertices"] <= res["members"]
    assert got == PINNED[name]
