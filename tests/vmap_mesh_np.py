"""NumPy restatement of sdm_vmap_mesh (include/sdm_c.h): a triangle mesh of the persistent voxel map's entries, vectorised over
the owners.  Nothing here is arithmetic: the normals are only compared, the rest is cells and ids.

  member      multiplicity[id] >= min_multiplicity and, with require_published, published[id] != 0 (flags None: every flag
              reads 0) -- vmap_cast_np.stops
  cell        floor(P * inv) in float32, inv = float32(1) / float32(voxel_size) -- vmap_comp_np.cells_of; a cell with a
              coordinate outside [-2^20, 2^20) holds nothing (tested before anything is looked up); "the member of a cell" is
              the cell's entry if it exists and is a member
  axis        a = 0; |n1| > |n_a|: a = 1; |n2| > |n_a|: a = 2 (ties to the lower index, a NaN never wins, denormals kept);
              u = (a + 1) % 3, v = (a + 2) % 3
  owner       a member of the range with |n_a| > 0 whose cell c - e_a holds no member
  step(j, ax) t = cell(j) + e_ax; for da in 0, -1, +1: the member k of t + da * e_a, then at most twice the member below it
              along -e_a if there is one; no hit: none
  corners     Nu = step(id, u), Nv = step(id, v), C = step(Nu, v) if Nu exists, else / if that is none and Nv exists
              step(Nv, u)
  triangles   all three: (id, Nu, C), (id, C, Nv); Nu and Nv: (id, Nu, Nv); Nu and C: (id, Nu, C); Nv and C: (id, C, Nv);
              n_a < 0 swaps the second and third index of each
  outputs     tri uint32[T, 3] by ascending owner; owner_tris uint8[count] by id - first; vertex_used uint8[M]
  totals      entries (the size of the range), members, owners, quads, singles, triangles, vertices"""
import numpy as np

from vmap_cast_np import stops
from vmap_comp_np import LIM, cells_of

f32 = np.float32
OUTS = ("entries", "members", "owners", "quads", "singles", "triangles", "vertices")
ARRAYS = ("tri", "owner_tris", "vertex_used")
DTYPES = {"tri": np.uint32, "owner_tris": np.uint8, "vertex_used": np.uint8}
STATS = ("axis 0", "axis 1", "axis 2", "tie", "NaN normal", "zero normal", "not the run bottom", "quad", "Nu Nv", "Nu C",
         "Nv C", "no triangle", "descent of 1", "descent of 2", "hit at da 0", "hit at da -1", "hit at da +1",
         "C by the second path", "flipped", "not flipped", "clipped")
NONE = -1


def _pack(c):
    """a lookup key for cells already known to be in range (never formed for a cell outside it)"""
    c = c + LIM
    return (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]


def axis_of(normal):
    """(a int64[n], n_a float32[n]) of normals float32[n, 3]: comparisons of magnitudes only"""
    nrm = np.asarray(normal, f32).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        mag = np.abs(nrm)
        a = np.zeros(len(nrm), np.int64)
        best = mag[:, 0].copy()
        for i in (1, 2):
            pick = mag[:, i] > best          # (False against a NaN on either side)
            a = np.where(pick, i, a)
            best = np.where(pick, mag[:, i], best)
    return a, nrm[np.arange(len(nrm)), a]


def mesh(rec, flags, voxel_size, normal, min_multiplicity=0, require_published=False, first=0, count=None, probed=None):
    """rec: the map's records {"xyz" float32[M, 3], "multiplicity" uint32[M]}; flags: uint8[M] or None; normal float32[count,
    3], indexed by id - first -> dict(tri uint32[T, 3], owner_tris uint8[count], vertex_used uint8[M], the seven totals, stats:
    how often each kind of case in STATS occurred, corners int64[count, 3]: (Nu, Nv, C) of every entry of the range with NONE
    for none, axis int64[count]: a, or NONE for an entry that is no member).  probed: a list that receives the cells int64[n,
    3] of every lookup, for the tests that ask which slots of the table a call walks"""
    xyz = np.ascontiguousarray(rec["xyz"], f32).reshape(-1, 3)
    M = len(xyz)
    count = M - first if count is None else count
    assert 0 <= first and 0 <= count and first + count <= M
    normal = np.asarray(normal, f32).reshape(-1, 3)
    assert len(normal) >= count
    normal = normal[:count]
    cell = cells_of(xyz, voxel_size)
    assert ((cell >= -LIM) & (cell < LIM)).all()   # (an entry outside the range does not exist)
    member = stops(rec, flags, min_multiplicity, require_published)
    keys = _pack(cell)
    by_key = np.argsort(keys, kind="stable")
    sorted_keys = keys[by_key]
    assert (sorted_keys[1:] != sorted_keys[:-1]).all()   # one entry per cell
    stats = dict.fromkeys(STATS, 0)

    def member_of(c, active):
        """int64[n]: the member of every cell c[n, 3] among the active rows, NONE elsewhere"""
        out = np.full(len(c), NONE, np.int64)
        inside = ((c >= -LIM) & (c < LIM)).all(1)
        stats["clipped"] += int((active & ~inside).sum())
        look = active & inside
        if probed is not None:
            probed.append(c[look])
        if M and look.any():
            kk = _pack(c[look])
            pos = np.minimum(np.searchsorted(sorted_keys, kk), M - 1)
            jj = by_key[pos]
            out[look] = np.where((sorted_keys[pos] == kk) & member[jj], jj, NONE)
        return out

    eye = np.eye(3, dtype=np.int64)

    def step(c, ax, a, active):
        """(k int64[n], its cell int64[n, 3]) of step(j, ax) for the active rows, j's cell c"""
        t = c + eye[ax]
        k = np.full(len(c), NONE, np.int64)
        kc = t.copy()
        for da, name in ((0, "hit at da 0"), (-1, "hit at da -1"), (1, "hit at da +1")):
            tc = t + da * eye[a]
            got = member_of(tc, active & (k == NONE))
            hit = got != NONE
            stats[name] += int(hit.sum())
            k = np.where(hit, got, k)
            kc = np.where(hit[:, None], tc, kc)
        moved = np.zeros(len(c), np.int64)
        going = k != NONE
        for _ in range(2):
            tc = kc - eye[a]
            got = member_of(tc, going)
            going = got != NONE
            k = np.where(going, got, k)
            kc = np.where(going[:, None], tc, kc)
            moved += going
        stats["descent of 1"] += int((moved == 1).sum())
        stats["descent of 2"] += int((moved == 2).sum())
        return k, kc

    ids = first + np.flatnonzero(member[first:first + count])   # the members of the range
    a, na = axis_of(normal[ids - first])
    with np.errstate(invalid="ignore"):
        mag = np.abs(normal[ids - first])
        has = np.abs(na) > 0
        stats["NaN normal"] = int(np.isnan(normal[ids - first]).any(1).sum())
        stats["zero normal"] = int((mag == 0).all(1).sum())
        top = np.abs(na)
        stats["tie"] = int((has & ((mag == top[:, None]).sum(1) >= 2)).sum())
    u, v = (a + 1) % 3, (a + 2) % 3
    c0 = cell[ids]
    below = member_of(c0 - eye[a], has)
    own = has & (below == NONE)
    stats["not the run bottom"] = int((has & ~own).sum())
    for i in range(3):
        stats["axis %d" % i] = int((own & (a == i)).sum())

    nu, cu = step(c0, u, a, own)
    nv, cv = step(c0, v, a, own)
    cc, _ = step(cu, v, a, own & (nu != NONE))
    second = own & (cc == NONE) & (nv != NONE)
    c2, _ = step(cv, u, a, second)
    stats["C by the second path"] = int((c2 != NONE).sum())
    cc = np.where(second, c2, cc)
    hu, hv, hc = nu != NONE, nv != NONE, cc != NONE
    have = hu.astype(np.int64) + hv + hc
    nt = np.where(have == 3, 2, np.where(have == 2, 1, 0))
    nt = np.where(own, nt, 0)
    flip = na < 0
    stats["quad"] = int((nt == 2).sum())
    stats["Nu Nv"] = int((own & (nt == 1) & ~hc).sum())
    stats["Nu C"] = int((own & (nt == 1) & ~hv).sum())
    stats["Nv C"] = int((own & (nt == 1) & ~hu).sum())
    stats["no triangle"] = int((own & (nt == 0)).sum())
    stats["flipped"] = int((own & (nt > 0) & flip).sum())
    stats["not flipped"] = int((own & (nt > 0) & ~flip).sum())

    # the first triangle's second and third index, the second triangle's (a quad's only)
    p1 = np.where((nt == 2) | ~hv, nu, np.where(~hc, nu, cc))
    p2 = np.where((nt == 2) | ~hv, cc, nv)
    first_tri = np.stack([ids, np.where(flip, p2, p1), np.where(flip, p1, p2)], 1)
    second_tri = np.stack([ids, np.where(flip, nv, cc), np.where(flip, cc, nv)], 1)
    both = np.stack([first_tri, second_tri], 1)                  # [n, 2, 3]
    keep = np.stack([nt >= 1, nt == 2], 1)
    tri = both[keep].astype(np.uint32).reshape(-1, 3)            # (row-major: by owner, the first before the second)

    owner_tris = np.zeros(count, np.uint8)
    owner_tris[ids - first] = nt
    vertex_used = np.zeros(M, np.uint8)
    vertex_used[tri.reshape(-1)] = 1
    corners = np.full((count, 3), NONE, np.int64)
    corners[ids - first] = np.where(own[:, None], np.stack([nu, nv, cc], 1), NONE)
    axis = np.full(count, NONE, np.int64)
    axis[ids - first] = a
    res = {"entries": int(count), "members": len(ids), "owners": int(own.sum()), "quads": int((nt == 2).sum()),
           "singles": int((nt == 1).sum()), "triangles": len(tri), "vertices": int(vertex_used.sum())}
    res.update(tri=tri, owner_tris=owner_tris, vertex_used=vertex_used, stats=stats, corners=corners, axis=axis)
    return res
