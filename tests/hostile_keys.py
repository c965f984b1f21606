"""Keys that collide on purpose in the voxel map's hash tables (sdm_voxel.h: vox_key, vox_mix, the probe (h + 1) & mask).

vox_mix is SplitMix64's finaliser, a bijection on 64 bits, and every value below 2^63 is a legal cell key (three 21-bit
biased cells).  A hash value whose low `low_bits` bits are all ones, inverted, is therefore a key that homes on the LAST slot
of every table of up to 2^low_bits slots; the half of those keys whose top bit is clear are cells.  A chain of L such keys
occupies slot cap - 1 and then slots 0 .. L - 2 at every capacity the tests reach, so it survives growth, and every other
key that homes inside that run has to be walked through it.  NumPy only: nothing here touches an engine."""
import numpy as np

U = np.uint64
C1, C2 = U(0xBF58476D1CE4E5B9), U(0x94D049BB133111EB)
C1_INV, C2_INV = U(0x96DE1B173F119089), U(0x319642B2D24D8EC3)  # C1 * C1_INV == C2 * C2_INV == 1 mod 2^64
F = np.float32
BIAS = 1 << 20
EMPTY = 0xFFFFFFFFFFFFFFFF


def _u(z):
    return np.asarray(z).astype(U)


def mix(z):
    """vox_mix of uint64 keys"""
    z = _u(z)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> U(30))) * C1
        z = (z ^ (z >> U(27))) * C2
    return z ^ (z >> U(31))


def unmix(z):
    """the key whose vox_mix is z"""
    z = _u(z)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> U(31)) ^ (z >> U(62))) * C2_INV
        z = (z ^ (z >> U(27)) ^ (z >> U(54))) * C1_INV
    return z ^ (z >> U(30)) ^ (z >> U(60))


def cell_key(cells):
    """vmap_cell_key of int cells [n, 3] in [-2^20, 2^20)"""
    b = (np.asarray(cells, np.int64).reshape(-1, 3) + BIAS).astype(U)
    return (b[:, 0] << U(42)) | (b[:, 1] << U(21)) | b[:, 2]


def key_cells(keys):
    """the int64 cells [n, 3] of cell keys below 2^63"""
    k = _u(keys).reshape(-1)
    m = U((1 << 21) - 1)
    return np.stack([(k >> U(42)) & m, (k >> U(21)) & m, k & m], 1).astype(np.int64) - BIAS


def centres(cells, voxel):
    """xyz = (cell + 0.5) * voxel with every step in binary32"""
    return ((np.asarray(cells).astype(F) + F(0.5)) * F(voxel)).astype(F)


def restated_key(xyz, voxel):
    """vox_key as tests/voxel_np.py states it: uint64 keys, EMPTY for an unmergeable point"""
    import voxel_np
    c, ok = voxel_np.cells(xyz, voxel)
    out = np.full(len(c), EMPTY, U)
    out[ok] = cell_key(c[ok].astype(np.int64))
    return out


def colliding_cells(n, seed, low_bits=20, voxel=1.0, free_bits=43):
    """n distinct cells whose keys' hashes end in low_bits ones, and their binary32 centres at `voxel`: (int64 [n, 3],
    float32 [n, 3], draws).  The hash's bits low_bits .. low_bits + free_bits - 1 are drawn, the rest above are zero; a draw
    whose key has its top bit set is no cell and is discarded, as is a repeat.  draws = how many it took."""
    rng = np.random.default_rng(seed)
    ones = U((1 << low_bits) - 1)
    span = min(free_bits, 64 - low_bits)
    keep, seen, draws = [], set(), 0
    while len(keep) < n:
        hi = rng.integers(0, 1 << span, 2 * n + 16, dtype=np.uint64)
        for k in unmix((hi << U(low_bits)) | ones).tolist():
            draws += 1
            if k < (1 << 63) and k not in seen:
                seen.add(k)
                keep.append(k)
                if len(keep) == n:
                    break
    cells = key_cells(np.array(keep, U))
    return cells, centres(cells, voxel), draws


def pair_key(entry, tag):
    """the observation set's key (u64)id << 32 | tag"""
    return (_u(entry) << U(32)) | (np.asarray(tag).astype(np.int64).astype(U) & U(0xFFFFFFFF))


def colliding_tags(entry_ids, per_entry, low_bits):
    """per entry id the `per_entry` smallest non-negative tags whose pair key's hash ends in low_bits ones: int32
    [len(entry_ids), per_entry].  About 2^low_bits tries per hit, searched in blocks."""
    ones = U((1 << low_bits) - 1)
    block = max(1 << 16, per_entry << (low_bits + 1))
    out = np.zeros((len(entry_ids), per_entry), np.int32)
    for i, e in enumerate(entry_ids):
        got, t0 = [], 0
        while len(got) < per_entry:
            assert t0 + block <= 1 << 31, "no tags left below 2^31"
            t = np.arange(t0, t0 + block, dtype=np.int64)
            got.extend(t[(mix(pair_key(np.full(block, e), t)) & ones) == ones].tolist())
            t0 += block
        out[i] = got[:per_entry]
    return out


def table_model(keys, cap):
    """Linear probing of distinct uint64 `keys` into `cap` slots (a power of two, more than len(keys)).  The set of occupied
    slots does not depend on the order of insertion (which key sits where does), so everything returned holds for every
    order the device's compare-and-swaps can take:
      occupied   bool[cap]
      run        (start, length): the maximal run of occupied slots, taken cyclically, that contains slot cap - 1 (length 0
                 if that slot is empty); it covers slots start .. start + length - 1 mod cap
      homes_in   how many keys home inside the run
      min_disp   a lower bound on the largest displacement.  A key never sits before its home, so the cnt(q) keys that home
                 at the run's positions 0 .. q fill those q + 1 positions and one of them sits at position cnt(q) - 1 or
                 later: it moved by at least cnt(q) - 1 - q.  The maximum over q.
      min_wraps  a lower bound on the keys sitting below their home: of the keys that home at or before slot cap - 1 inside
                 the run, only as many as there are positions up to that slot stay before the table's end"""
    keys = _u(keys).reshape(-1)
    assert cap & (cap - 1) == 0 and len(keys) < cap and len(np.unique(keys)) == len(keys)
    home = (mix(keys) & U(cap - 1)).astype(np.int64)
    occupied = np.zeros(cap, bool)
    free_at = np.arange(cap)  # union-find: the next free slot at or after s, cyclically
    def find(s):
        r = s
        while free_at[r] != r:
            r = free_at[r]
        while free_at[s] != r:
            free_at[s], s = r, free_at[s]
        return r
    for h in home.tolist():
        s = find(h)
        occupied[s] = True
        free_at[s] = find((s + 1) & (cap - 1))
    if not occupied[cap - 1]:
        return {"occupied": occupied, "run": (cap - 1, 0), "homes_in": 0, "min_disp": 0, "min_wraps": 0}
    start = cap - 1
    while occupied[(start - 1) & (cap - 1)]:
        start = (start - 1) & (cap - 1)
    length = 1
    while occupied[(start + length) & (cap - 1)]:
        length += 1
    off = (home - start) & (cap - 1)  # a home's position inside the run
    inside = off < length
    assert int(inside.sum()) == length  # a run holds exactly the keys that home in it
    cnt = np.cumsum(np.bincount(off[inside], minlength=length))  # cnt[q]: keys homing at the run's positions 0 .. q
    q_end = cap - 1 - start                                       # the position of slot cap - 1
    return {"occupied": occupied, "run": (start, length), "homes_in": length,
            "min_disp": int((cnt - 1 - np.arange(length)).max()), "min_wraps": int(cnt[q_end] - (q_end + 1))}


def table_layout(keys, cap):
    """one layout of the table: the slot of each of the distinct `keys` when they are inserted one after the other in the
    order given, and (largest displacement, keys below their home) -- what the device's witness reports for that layout.
    Unlike table_model's figures these depend on the order."""
    keys = _u(keys).reshape(-1)
    home = (mix(keys) & U(cap - 1)).astype(np.int64)
    taken = np.zeros(cap, bool)
    slot = np.zeros(len(keys), np.int64)
    for i, h in enumerate(home.tolist()):
        while taken[h]:
            h = (h + 1) & (cap - 1)
        taken[h] = True
        slot[i] = h
    return slot, (int(((slot - home) & (cap - 1)).max(initial=0)), int((slot < home).sum()))


def homes_in_run(keys, cap, run):
    """which of `keys` (present or absent) home inside the model's run: their probe must walk to the run's end"""
    start, length = run
    home = (mix(keys) & U(cap - 1)).astype(np.int64)
    return ((home - start) & (cap - 1)) < length
