"""CPU: tests/vmap_comp_np.py (the restatement of sdm_vmap_components) against an independent flood fill that visits one
entry and one offset at a time, on crafted maps, on random maps, and on keyframe 0 of every golden fixture; then the
properties a partition into components has.  tests/test_gpu_vmap_comp.py runs the engine on the same maps."""
import functools

import numpy as np
import pytest

import golden_util as gu
import vmap_comp_np as vq
from test_vmap_carve_cpu import cloud_of
from test_vmap_recarve_cpu import EQ_VOXEL, fixture_kf0

F = np.float32
LIM = 1 << 20
CONNECTIVITIES = (6, 18, 26)
RANDOM_VOXEL = 0.05
RANDOM_M = ((0, 1), (1, 1), (63, 8), (64, 8), (65, 8), (2049, 24))   # (entries, side of the cube they are drawn from)
FILTERS = (dict(), dict(min_multiplicity=2), dict(require_published=True), dict(min_multiplicity=3, require_published=True))
GOLDEN_MIN_SIZE = 8


def flood_fill(rec, flags, voxel_size, connectivity=26, min_multiplicity=0, require_published=False, min_size=0):
    """the same answer without union-find: a breadth-first fill from every member not yet reached, in id order (so the seed
    is its component's smallest id), one entry and one of the 6, 18 or 26 offsets at a time"""
    xyz = np.asarray(rec["xyz"], F).reshape(-1, 3)
    M = len(xyz)
    inv = F(1.0) / F(voxel_size)
    mult = np.asarray(rec["multiplicity"]).reshape(-1)
    cell, member = [], []
    for i in range(M):
        cell.append(tuple(int(np.floor(F(xyz[i, k] * inv))) for k in range(3)))
        pub = 0 if flags is None else int(flags[i])
        member.append(int(mult[i]) >= min_multiplicity and (not require_published or pub != 0))
    where = {cell[i]: i for i in range(M) if member[i]}
    offs = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)
            if 1 <= abs(dx) + abs(dy) + abs(dz) <= {6: 1, 18: 2, 26: 3}[connectivity]]
    label = [vq.NO_COMPONENT] * M
    size = [0] * M
    for seed in range(M):
        if not member[seed] or label[seed] != vq.NO_COMPONENT:
            continue
        label[seed] = seed
        reached, todo = [seed], [seed]
        while todo:
            i = todo.pop()
            for d in offs:
                n = (cell[i][0] + d[0], cell[i][1] + d[1], cell[i][2] + d[2])
                if min(n) < -LIM or max(n) >= LIM:
                    continue
                j = where.get(n)
                if j is not None and label[j] == vq.NO_COMPONENT:
                    label[j] = seed
                    reached.append(j)
                    todo.append(j)
        for i in reached:
            size[i] = len(reached)
    small = [i for i in range(M) if member[i] and size[i] < min_size]
    roots = [i for i in range(M) if label[i] == i]
    return {"label": np.array(label, np.uint32).reshape(-1), "size": np.array(size, np.uint32).reshape(-1),
            "small_ids": np.array(small, np.uint32).reshape(-1), "entries": M, "members": sum(member), "components": len(roots),
            "largest": max(size, default=0), "small": len(small), "small_components": sum(1 for r in roots if size[r] < min_size)}


def same(a, b, what):
    for f in vq.ARRAYS:
        assert a[f].dtype == b[f].dtype == np.uint32 and a[f].shape == b[f].shape, (what, f)
        np.testing.assert_array_equal(a[f], b[f], err_msg="%s %s" % (what, f))
    assert {f: a[f] for f in vq.OUTS} == {f: b[f] for f in vq.OUTS}, what


def both(rec, flags, voxel, **kw):
    a = vq.components(rec, flags, voxel, **kw)
    same(a, flood_fill(rec, flags, voxel, **kw), repr(kw))
    return a


def records_of(cells, multiplicity=None, voxel=1.0, jitter=None):
    """records as vmap_import takes them, one per cell in the order given: xyz = (cell + 0.5) * voxel, or + jitter"""
    cells = np.asarray(cells, np.float64).reshape(-1, 3)
    M = len(cells)
    xyz = ((cells + (0.5 if jitter is None else jitter)) * voxel).astype(F)
    mult = np.ones(M, np.uint32) if multiplicity is None else np.asarray(multiplicity, np.uint32)
    return dict(cloud_of(xyz), tag=np.zeros(M, np.int32), multiplicity=mult)


def flags_of(M, seed=0):
    return (np.random.default_rng(77 + M + seed).random(M) < 0.7).astype(np.uint8)


def grid(nx, ny, nz):
    return np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)


# where the pieces of the crafted map stand (each at least 3 cells from the next): name -> (first id, entries)
SMALL = {}


@functools.lru_cache(maxsize=None)
def small_case():
    """the crafted pieces at voxel 1, one entry per cell, id = order: the pairs by face, edge and corner; a 3-D checkerboard; a
    hollow shell around a single cell; a bridge of multiplicity 1 between two pieces of multiplicity 2; the pairs the
    aliasing key would join; a face-adjacent pair at each end of the range"""
    cells, mult = [], []

    def add(name, c, m=None):
        c = np.asarray(c, np.int64).reshape(-1, 3)
        SMALL[name] = (len(cells), len(c))
        cells.extend(c.tolist())
        mult.extend([1] * len(c) if m is None else m)

    add("face", [[0, 0, 0], [1, 0, 0]])
    add("edge", [[0, 0, 10], [1, 1, 10]])
    add("corner", [[0, 0, 20], [1, 1, 21]])
    g = grid(6, 6, 6)
    add("checkerboard", g[g.sum(1) % 2 == 0] + [20, 0, 0])
    g = grid(5, 5, 5)
    add("shell", g[(g == 0).any(1) | (g == 4).any(1)] + [40, 0, 0])
    add("inside", [[42, 2, 2]])
    add("bridge", [[60 + i, 0, 0] for i in range(7)], [2, 2, 2, 1, 2, 2, 2])
    add("z into y", [[0, 0, LIM - 1], [0, 1, -LIM]])
    add("y into x", [[100, LIM - 1, 5], [101, -LIM, 5]])
    add("last cells", [[LIM - 1, LIM - 1, LIM - 1], [LIM - 2, LIM - 1, LIM - 1]])
    add("first cells", [[-LIM, -LIM, -LIM], [-LIM, -LIM, -LIM + 1]])
    return records_of(cells, mult), None


@functools.lru_cache(maxsize=None)
def lines_case():
    """three straight lines of 2049 cells: ids ascending along the first, descending along the second, shuffled on the third"""
    rng = np.random.default_rng(5)
    n = 2049
    i = np.arange(n)
    order = [i, i[::-1], rng.permutation(n)]
    cells = np.concatenate([np.stack([o - 1000, np.full(n, 10 * k), np.zeros(n, np.int64)], 1) for k, o in enumerate(order)])
    return records_of(cells, rng.integers(1, 5, 3 * n)), flags_of(3 * n)


@functools.lru_cache(maxsize=None)
def block_case():
    """a solid 17 x 17 x 17 block with shuffled ids: every root is contended"""
    rng = np.random.default_rng(6)
    cells = rng.permutation(grid(17, 17, 17) - 8)
    return records_of(cells, rng.integers(1, 5, len(cells))), flags_of(len(cells))


@functools.lru_cache(maxsize=None)
def random_case(M, side):
    """M cells drawn without replacement from a cube of `side` cells astride the origin, in a random order, each record
    somewhere inside its cell; multiplicities 1 .. 4; random flags"""
    rng = np.random.default_rng(1000 + M)
    pick = rng.choice(side ** 3, M, replace=False)
    cells = np.stack([pick // (side * side), (pick // side) % side, pick % side], 1) - side // 2
    rec = records_of(cells, rng.integers(1, 5, M), RANDOM_VOXEL, rng.uniform(0.1, 0.9, (M, 3)))
    assert (vq.cells_of(rec["xyz"], RANDOM_VOXEL) == cells).all()
    return rec, flags_of(M)


# name -> (case, voxel): every map the GPU test imports
MAPS = dict([("small", (small_case, 1.0)), ("lines", (lines_case, 1.0)), ("block", (block_case, 1.0))] +
            [("random %d" % M, (functools.partial(random_case, M, side), RANDOM_VOXEL)) for M, side in RANDOM_M])


def piece(res, name, f="label"):
    a, n = SMALL[name]
    return res[f][a:a + n]


def partition(res):
    """the components as a set of frozensets of ids"""
    groups = {}
    for i, l in enumerate(res["label"].tolist()):
        if l != vq.NO_COMPONENT:
            groups.setdefault(l, []).append(i)
    return {frozenset(g) for g in groups.values()}


def test_crafted_pieces():
    rec, _ = small_case()
    res = {c: both(rec, None, 1.0, connectivity=c) for c in CONNECTIVITIES}
    joined = lambda c, name: len(set(piece(res[c], name).tolist())) == 1
    assert [joined(c, "face") for c in CONNECTIVITIES] == [True, True, True]
    assert [joined(c, "edge") for c in CONNECTIVITIES] == [False, True, True]
    assert [joined(c, "corner") for c in CONNECTIVITIES] == [False, False, True]
    assert len(partition(res[6])) > len(partition(res[18])) > len(partition(res[26]))   # three different partitions
    n = SMALL["checkerboard"][1]
    assert n == 108 and (piece(res[6], "checkerboard", "size") == 1).all()
    assert joined(18, "checkerboard") and (piece(res[18], "checkerboard", "size") == n).all()
    for c in CONNECTIVITIES:
        assert joined(c, "shell") and (piece(res[c], "shell", "size") == 98).all()
        assert piece(res[c], "inside").tolist() == [SMALL["inside"][0]] and piece(res[c], "inside", "size").tolist() == [1]
        assert joined(c, "bridge") and (piece(res[c], "bridge", "size") == 7).all()
        for name in ("z into y", "y into x"):   # one component under a key that lets a coordinate carry into the next
            assert not joined(c, name) and (piece(res[c], name, "size") == 1).all(), (c, name)
        for name in ("last cells", "first cells"):
            assert joined(c, name) and (piece(res[c], name, "size") == 2).all(), (c, name)
    # the bridge is no member at min_multiplicity 2: it separates the two pieces
    split = both(rec, None, 1.0, min_multiplicity=2)
    a = SMALL["bridge"][0]
    assert piece(split, "bridge").tolist() == [a, a, a, vq.NO_COMPONENT, a + 4, a + 4, a + 4]
    assert piece(split, "bridge", "size").tolist() == [3, 3, 3, 0, 3, 3, 3]
    assert split["members"] == 6 and split["components"] == 2 and split["largest"] == 3


def test_lines_and_block():
    rec, flags = lines_case()
    for c in CONNECTIVITIES:
        res = both(rec, flags, 1.0, connectivity=c)
        assert res["components"] == 3 and res["largest"] == 2049 and (res["size"] == 2049).all()
        assert sorted(set(res["label"].tolist())) == [0, 2049, 4098]
    for kw in FILTERS[1:]:
        res = both(rec, flags, 1.0, min_size=3, **kw)   # the filter cuts the lines into runs
        assert 3 < res["components"] and 0 < res["small"] < res["members"] < res["entries"]
    rec, flags = block_case()
    for c in CONNECTIVITIES:
        res = both(rec, flags, 1.0, connectivity=c)
        assert res["components"] == 1 and res["largest"] == 17 ** 3 and (res["label"] == 0).all()
    for kw in FILTERS[1:]:
        both(rec, flags, 1.0, connectivity=6, min_size=5, **kw)


@pytest.mark.parametrize("M,side", RANDOM_M)
def test_random_maps(M, side):
    rec, flags = random_case(M, side)
    for c in CONNECTIVITIES:
        for fl in (flags, None):
            for kw in FILTERS:
                res = both(rec, fl, RANDOM_VOXEL, connectivity=c, min_size=4, **kw)
                assert res["entries"] == M
                if kw.get("require_published") and fl is None:
                    assert res["members"] == 0


def test_inputs_hold_every_kind_of_case():
    seen = set()
    for name, (case, voxel) in MAPS.items():
        rec, flags = case()
        part = []
        for c in CONNECTIVITIES:
            for kw in FILTERS:
                res = vq.components(rec, flags, voxel, connectivity=c, min_size=4, **kw)
                if (res["size"] == 1).any():
                    seen.add("singleton")
                if res["largest"] >= 64:
                    seen.add("component of 64")
                if res["members"] < res["entries"]:
                    seen.add("non-member")
                seen.add("small positive" if res["small"] else "small zero")
                if res["components"] > 1 and 1 < res["largest"] < res["members"]:
                    seen.add("components of several sizes")
            part.append(partition(vq.components(rec, flags, voxel, connectivity=c)))
        if part[0] != part[1] != part[2] != part[0]:
            seen.add("three partitions")
    rec, _ = small_case()
    a = SMALL["bridge"][0]
    whole, split = vq.components(rec, None, 1.0), vq.components(rec, None, 1.0, min_multiplicity=2)
    if whole["label"][a] == whole["label"][a + 6] and split["label"][a] != split["label"][a + 6] and split["label"][a + 3] == vq.NO_COMPONENT:
        seen.add("a non-member between two components")
    assert seen == {"singleton", "component of 64", "non-member", "small positive", "small zero", "components of several sizes",
                    "three partitions", "a non-member between two components"}


@pytest.mark.parametrize("name", sorted(MAPS))
def test_properties(name):
    case, voxel = MAPS[name]
    rec, flags = case()
    M = len(rec["pixel"])
    ids = np.arange(M, dtype=np.uint32)
    res = {}
    for c in CONNECTIVITIES:
        for kw in FILTERS[:2]:
            r = vq.components(rec, flags, voxel, connectivity=c, **kw)
            # P1: a label is a fixed point no larger than the id; the roots' sizes sum to the members
            mem = r["label"] != vq.NO_COMPONENT
            assert (r["label"][mem] <= ids[mem]).all() and (r["label"][r["label"][mem]] == r["label"][mem]).all()
            roots = r["label"] == ids
            assert int(r["size"][roots].sum()) == r["members"] == int(mem.sum()) and int(roots.sum()) == r["components"]
            assert (r["size"][~mem] == 0).all() and r["small"] == 0 and len(r["small_ids"]) == 0
            # P4: min_size 1 lists nothing, min_size beyond the members lists every member
            assert vq.components(rec, flags, voxel, connectivity=c, min_size=1, **kw)["small"] == 0
            every = vq.components(rec, flags, voxel, connectivity=c, min_size=r["members"] + 1, **kw)
            assert every["small_ids"].tolist() == np.flatnonzero(mem).tolist() and every["small_components"] == r["components"]
            res[c, kw.get("min_multiplicity", 0)] = r
    # P2: the 6-partition refines the 18-partition, which refines the 26-partition
    for m in (0, 2):
        for fine, coarse in ((6, 18), (18, 26)):
            lf, lc = res[fine, m]["label"], res[coarse, m]["label"]
            assert ((lf == vq.NO_COMPONENT) == (lc == vq.NO_COMPONENT)).all()
            mem = lf != vq.NO_COMPONENT
            assert (lc[lf[mem]] == lc[mem]).all()   # an entry and its finer root share the coarser component
            assert res[fine, m]["components"] >= res[coarse, m]["components"]
    # P3: the same cells under a permutation of the ids: the same partition of the cells, the same multiset of sizes
    perm = np.random.default_rng(3).permutation(M)
    rec2 = {f: a[perm] for f, a in rec.items()}
    flags2 = None if flags is None else flags[perm]
    for c in CONNECTIVITIES:
        r1, r2 = vq.components(rec, flags, voxel, connectivity=c, min_size=4), vq.components(rec2, flags2, voxel, connectivity=c, min_size=4)
        back = np.empty(M, np.int64)
        back[np.arange(M)] = perm   # entry j of the permuted map is entry perm[j] of the first
        assert {frozenset(back[list(g)].tolist()) for g in partition(r2)} == partition(r1)
        assert sorted(r1["size"].tolist()) == sorted(r2["size"].tolist())
        assert [r1[f] for f in vq.OUTS] == [r2[f] for f in vq.OUTS]
    # P5: a filter nothing passes
    none = vq.components(rec, flags, voxel, min_multiplicity=5, min_size=4)
    assert (none["label"] == vq.NO_COMPONENT).all() and not none["size"].any() and len(none["small_ids"]) == 0
    assert [none[f] for f in vq.OUTS] == [M, 0, 0, 0, 0, 0]


# keyframe 0 of each golden fixture, integrated alone at voxel 0.005 (tests/test_vmap_recarve_cpu.py's recipe): the six
# totals at connectivity 6 and 26 with min_size 8, from the restatement on the CPU
PINNED = {"plane_160x120_n7": ((2209, 2209, 910, 5, 2209, 910), (2209, 2209, 793, 9, 2192, 791)),
          "plane_64x48_n7": ((720, 720, 720, 1, 720, 720), (720, 720, 720, 1, 720, 720)),
          "plane_96x80_n20": ((678, 678, 678, 1, 678, 678), (678, 678, 677, 2, 678, 677)),
          "strip_roll_160x120_n7": ((2255, 2255, 1024, 17, 2087, 1010), (2255, 2255, 735, 50, 1768, 710))}


@pytest.mark.parametrize("name", gu.fixture_names())
def test_golden_fixture_totals(name):
    vm = fixture_kf0(name)[0]
    rec = {"xyz": vm.rec["xyz"], "multiplicity": vm.rec["multiplicity"]}
    got = []
    for c in (6, 26):
        res = both(rec, None, EQ_VOXEL, connectivity=c, min_size=GOLDEN_MIN_SIZE)
        got.append(tuple(res[f] for f in vq.OUTS))
    print(name, got)
    assert tuple(got) == PINNED[name]
