"""NumPy restatement of sdm_vmap_components (include/sdm_c.h): the connected components of the persistent voxel map's entries.

  member      multiplicity[id] >= min_multiplicity and, with require_published, published[id] != 0 (flags None: every flag
              reads 0) -- vmap_cast_np.stops, the filter of the ray queries
  cell        floor(xyz * inv) in float32, inv = float32(1) / float32(voxel_size); every entry has a cell of its own
  adjacency   an offset d in {-1, 0, 1}^3, d != 0, with |dx| + |dy| + |dz| <= 1, 2, 3 for connectivity 6, 18, 26; a cell with a
              coordinate outside [-2^20, 2^20) holds nothing (the cells are looked up as tuples: no key is formed, so nothing
              can alias)
  components  the classes of the transitive closure of "both members, cells adjacent"
  per entry   label = the smallest id of its component, size = its members; (NO_COMPONENT, 0) for a non-member
  small list  min_size > 0: the ascending ids of the members whose component has fewer than min_size members
  totals      entries, members, components, largest, small, small_components

Union-find over a dict of the members' cells: every member visits the lexicographically positive half of the offsets, so each
pair of adjacent cells is met once; the smaller root survives a union, so a root is its component's smallest id."""
import numpy as np

from vmap_cast_np import stops

f32 = np.float32
LIM = 1 << 20
NO_COMPONENT = 0xFFFFFFFF
OUTS = ("entries", "members", "components", "largest", "small", "small_components")
ARRAYS = ("label", "size", "small_ids")
MAX_L1 = {6: 1, 18: 2, 26: 3}


def offsets(connectivity, half=False):
    """the offsets of a connectivity in lexicographic order; half: only those after (0, 0, 0)"""
    out = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)
           if 0 < abs(dx) + abs(dy) + abs(dz) <= MAX_L1[connectivity]]
    return [d for d in out if d > (0, 0, 0)] if half else out


def cells_of(xyz, voxel_size):
    """int64[M, 3]: the cell of every record"""
    xyz = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    inv = f32(1.0) / f32(voxel_size)
    return np.floor(xyz * inv).astype(np.int64)


def components(rec, flags, voxel_size, connectivity=26, min_multiplicity=0, require_published=False, min_size=0):
    """rec: the map's records {"xyz" float32[M, 3], "multiplicity" uint32[M]}; flags: uint8[M] or None ->
    dict(label uint32[M], size uint32[M], small_ids uint32[small], the six totals)"""
    assert connectivity in MAX_L1 and min_size >= 0
    cell = cells_of(rec["xyz"], voxel_size)
    M = len(cell)
    member = stops(rec, flags, min_multiplicity, require_published)
    assert ((cell >= -LIM) & (cell < LIM)).all()   # (an entry outside the range does not exist)
    at = {}
    for i in np.flatnonzero(member):
        c = tuple(cell[i].tolist())
        assert c not in at                          # one entry per cell
        at[c] = int(i)
    parent = list(range(M))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    half = offsets(connectivity, half=True)
    for (cx, cy, cz), i in at.items():
        for dx, dy, dz in half:
            n = (cx + dx, cy + dy, cz + dz)
            if not all(-LIM <= v < LIM for v in n):   # holds nothing
                continue
            j = at.get(n)
            if j is not None:
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    label = np.full(M, NO_COMPONENT, np.uint32)
    size = np.zeros(M, np.uint32)
    ids = np.flatnonzero(member)
    if len(ids):
        roots = np.array([find(int(i)) for i in ids], np.int64)
        label[ids] = roots
        size[ids] = np.bincount(roots, minlength=M)[roots]
    is_root = label == np.arange(M, dtype=np.uint32)
    small = member & (size < min_size)
    return {"label": label, "size": size, "small_ids": np.flatnonzero(small).astype(np.uint32), "entries": M,
            "members": int(member.sum()), "components": int(is_root.sum()), "largest": int(size.max()) if M else 0,
            "small": int(small.sum()), "small_components": int((is_root & small).sum())}
