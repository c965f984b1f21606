// sdm_vmap_comp.h -- connected components of the persistent voxel map's entries (sdm_vmap_components; included by
// sdm_engine.hip).  Every filter the map had is local -- one entry's counters, the occupancy of its 26 adjacent cells; this
// call answers the global question: which entries belong to a connected piece of at least k voxels?  A lock-free union-find
// over the hash table; the table, the records and the flags are only read, and the call keeps no per-entry state.
//
// Scratch per call: parent[M] and csize[M], both u32.  One call over the M entries id = 0 .. M-1:
//   k_vcomp_init     one lane per entry: the member test (multiplicity, published flag -- k_vmap_cast's filter); parent[id] =
//                    id for a member, VMAP_NOID otherwise; csize[id] = 0
//   k_vcomp_link     one lane per member: its cell from its record as vcls_neighbours forms it, then the lexicographically
//                    positive half of the offsets (3, 9 or 13 of them for connectivity 6, 18, 26), so each undirected pair of
//                    cells is met once: the range test, the read-only vmap_find, and if the neighbour is a member the two
//                    are united
//   k_vcomp_flatten  (a later launch) parent[id] = root(id), and one u32 atomicAdd(&csize[root], 1) per member: integer adds
//                    commute, so the sizes are the same from run to run
//   k_vcomp_count    (a later launch: it needs every size) tiles of EXT_TILE entries; small(id) = member && csize[label] <
//                    min_size is counted per tile by ballot and popcount; members, components and small components go from
//                    wave sums into one 64-bit atomic per non-zero total, the largest size into an atomicMax
//   k_extract_scan_tiles / k_extract_scan_sums   (sdm_extract.h, unchanged) scan the tile counts
//   k_vcomp_totals   `small` for the host's one wait
//   k_vcomp_write    (queued only if the call is not refused) label, size and small_ids[rank] with the rank from the scan
//                    over id, so the list is ascending without a sort
//
// The union-find.  Find walks parent[] to the node that points to itself and halves the path on its way.  Union takes the two
// roots, hi = the larger and lo = the smaller, and tries atomicCAS(&parent[hi], hi, lo); on a failure it goes on from the
// value the CAS returned.  Invariants:
//   - parent[i] <= i always: init writes i, the CAS writes lo < hi, halving writes a value read further down the chain.
//   - A root is written only by the CAS (which succeeds only on a word that still holds its own index), so a node that has
//     once been seen with parent[x] != x is a non-root for the rest of the call.
//   - A non-root is written only by halving in k_vcomp_link, and in k_vcomp_flatten only by its own lane, which does not
//     halve (see there); both write an ancestor: a node read by walking down from it.  Trees only ever merge, so a node
//     once below x's root stays in x's tree, and the store moves x inside its own tree, never between trees.
//   - The chains strictly descend, so every walk ends after at most its start index many steps, whatever it reads.
//   - The surviving root of a component has every member of the component on a descending chain above it: it is the
//     component's smallest id.
// Correctness does not rest on a read being fresh.  parent[] is read with relaxed agent-scope atomic loads and halved with
// relaxed agent-scope atomic stores, and any value a read returns was stored in that word at some time.  A stale value is
// therefore the word's own index (it was a root then) or an older ancestor: a walk over stale words still ends in x's tree,
// only higher up than it could have.  What it returns is decided by the CAS alone: a stale "hi is a root" makes the CAS fail
// and hand back what parent[hi] really holds, from where the walk goes on; a stale "lo is a root" links hi below a node of
// the other tree, which unites the two just as well.  Two walks that end in one node prove one tree.  No lane waits for
// another: a failed CAS means another lane's CAS on that word succeeded, and at most M - 1 succeed in a call.  No
// wave-level operation stands inside a divergent loop; every lane of a wave reaches every ballot and shuffle; no LDS in the
// union-find.  Union-find is indifferent to the slice a link lands in.  Plain C++ and vector stores only.
#pragma once
#include "sdm_vmap_cast.h"

namespace sdm {

constexpr unsigned VMAP_NO_COMPONENT = VMAP_NOID;  // SDM_VMAP_NO_COMPONENT: the label of a non-member

// the find of k_vcomp_link: with path halving (what ships), or -DSDM_VCOMP_HALVE=false the plain walk, built only to time it
// (tools/build_variants.py); neither can change a result
#ifndef SDM_VCOMP_HALVE
#define SDM_VCOMP_HALVE true
#endif

__device__ __forceinline__ unsigned vcomp_load(const unsigned* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x's tree as far as this lane can see (x a member).  HALVE: it halves the path it walks; otherwise it only reads
template <bool HALVE>
__device__ __forceinline__ unsigned vcomp_root(unsigned* parent, unsigned x)
{
    for (;;) {  // (x strictly descends: at most x rounds)
        const unsigned p = vcomp_load(&parent[x]);
        if (p == x) return x;
        const unsigned g = vcomp_load(&parent[p]);
        if (g == p) return p;
        // x is a non-root, g < p < x below it
        if (HALVE) __hip_atomic_store(&parent[x], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = g;
    }
}

// unites the trees of the members a and b
__device__ __forceinline__ void vcomp_unite(unsigned* parent, unsigned a, unsigned b)
{
    a = vcomp_root<SDM_VCOMP_HALVE>(parent, a);
    b = vcomp_root<SDM_VCOMP_HALVE>(parent, b);
    while (a != b) {  // (a round is repeated only after another lane's CAS on parent[hi] succeeded)
        const unsigned hi = a > b ? a : b, lo = a > b ? b : a;
        const unsigned old = atomicCAS(&parent[hi], hi, lo);
        if (old == hi) break;
        a = vcomp_root<SDM_VCOMP_HALVE>(parent, old);  // hi had a parent already: on from there
        b = vcomp_root<SDM_VCOMP_HALVE>(parent, lo);
    }
}

// one lane per entry id0 + thread
__global__ __launch_bounds__(BLOCK) void k_vcomp_init(const unsigned* __restrict__ multiplicity,
                                                      const unsigned char* __restrict__ published, unsigned min_multiplicity,
                                                      int require_published, long long M, long long id0,
                                                      unsigned* __restrict__ parent, unsigned* __restrict__ csize)
{
    const long long id = id0 + (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (id >= M) return;
    const bool member = multiplicity[id] >= min_multiplicity && (!require_published || (published && published[id] != 0));
    parent[id] = member ? (unsigned)id : VMAP_NOID;
    csize[id] = 0u;
}

// one lane per entry id0 + thread; max_l1 = 1, 2, 3 for connectivity 6, 18, 26
__global__ __launch_bounds__(BLOCK) void k_vcomp_link(VmapTable tb, const float* __restrict__ xyz, float inv, int max_l1,
                                                      long long M, long long id0, unsigned* parent)
{
    const long long id = id0 + (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (id >= M) return;
    if (vcomp_load(&parent[id]) == VMAP_NOID) return;  // (a member's word never holds VMAP_NOID, a non-member's nothing else)
    const int cx = (int)floorf(xyz[id * 3 + 0] * inv), cy = (int)floorf(xyz[id * 3 + 1] * inv),
              cz = (int)floorf(xyz[id * 3 + 2] * inv);  // (in range: the entry exists)
    const int lim = 1 << 20;
    for (int q = 14; q < 27; q++) {  // the offsets after (0, 0, 0) in lexicographic order
        const int dx = q / 9 - 1, dy = (q / 3) % 3 - 1, dz = q % 3 - 1;
        if ((dx != 0) + (dy != 0) + (dz != 0) > max_l1) continue;
        const int nx = cx + dx, ny = cy + dy, nz = cz + dz;
        if (nx < -lim || nx >= lim || ny < -lim || ny >= lim || nz < -lim || nz >= lim) continue;  // holds nothing; no key
        const unsigned nb = vmap_find(tb, vmap_cell_key(nx, ny, nz));
        if (nb < (unsigned)M && vcomp_load(&parent[nb]) != VMAP_NOID) vcomp_unite(parent, (unsigned)id, nb);
    }
}

// one lane per entry id0 + thread: the walk of every member ends in the smallest id of its component.  The walk only reads:
// here a word must end as its entry's root, so it is written by its own lane alone -- a halving store of another lane, begun
// before that write and landing after it, would leave an ancestor that is not the root.  The links are all made, so a word
// that holds its own index is a root for good; a word another lane has flattened already only shortens the walk.
__global__ __launch_bounds__(BLOCK) void k_vcomp_flatten(long long M, long long id0, unsigned* parent, unsigned* __restrict__ csize)
{
    const long long id = id0 + (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (id >= M) return;
    if (vcomp_load(&parent[id]) == VMAP_NOID) return;
    const unsigned r = vcomp_root<false>(parent, (unsigned)id);
    if (r != (unsigned)id) __hip_atomic_store(&parent[id], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    atomicAdd(&csize[r], 1u);
}

// one workgroup per tile tile0 + block of EXT_TILE consecutive entries; label = parent after k_vcomp_flatten;
// totals += {members, components, small components}, totals[3] = max(totals[3], the largest size)
__global__ __launch_bounds__(BLOCK) void k_vcomp_count(const unsigned* __restrict__ label, const unsigned* __restrict__ csize,
                                                       unsigned min_size, long long M, long long tile0,
                                                       unsigned* __restrict__ cnt_small, unsigned long long* __restrict__ totals)
{
    __shared__ unsigned wsum[EXT_WAVES];
    const long long tile = tile0 + blockIdx.x;
    const long long base = tile * EXT_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned sm = 0, mem = 0, comp = 0, smc = 0, big = 0;
#pragma unroll 1
    for (int k = 0; k < EXT_PER; k++) {
        const long long id = base + k * BLOCK + threadIdx.x;
        bool member = false, root = false, small = false;
        if (id < M) {
            const unsigned l = label[id];
            if (l != VMAP_NOID) {
                const unsigned sz = csize[l];
                member = true;
                root = l == (unsigned)id;
                small = sz < min_size;
                if (root && sz > big) big = sz;
            }
        }
        sm += (unsigned)__popcll(__ballot(small));  // (every lane of the wave arrives here)
        mem += (unsigned)__popcll(__ballot(member));
        comp += (unsigned)__popcll(__ballot(root));
        smc += (unsigned)__popcll(__ballot(root && small));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned other = __shfl_xor(big, o, 64);
        big = other > big ? other : big;
    }
    if (lane == 0) {
        wsum[wave] = sm;
        if (mem) atomicAdd(&totals[0], (unsigned long long)mem);
        if (comp) atomicAdd(&totals[1], (unsigned long long)comp);
        if (smc) atomicAdd(&totals[2], (unsigned long long)smc);
        if (big) atomicMax(&totals[3], (unsigned long long)big);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = 0;
        for (int v = 0; v < EXT_WAVES; v++) t += wsum[v];
        cnt_small[tile] = t;
    }
}

// totals[4] = the members of small components
__global__ void k_vcomp_totals(long long nt, const unsigned* __restrict__ off, const unsigned long long* __restrict__ blk,
                               unsigned long long* __restrict__ totals)
{
    if (blockIdx.x || threadIdx.x) return;
    totals[4] = ext_tile_offset(off, blk, nt);
}

// every entry writes its label and size, the small members their id at their rank.  Any destination may be null.
__global__ __launch_bounds__(BLOCK) void k_vcomp_write(const unsigned* __restrict__ label, const unsigned* __restrict__ csize,
                                                       unsigned min_size, long long M, long long tile0,
                                                       const unsigned* __restrict__ off, const unsigned long long* __restrict__ blk,
                                                       unsigned* __restrict__ label_out, unsigned* __restrict__ size_out,
                                                       unsigned* __restrict__ small_ids)
{
    __shared__ unsigned wcnt[EXT_PER][EXT_WAVES];
    const long long tile = tile0 + blockIdx.x;
    const long long base = tile * EXT_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool f[EXT_PER];
    unsigned below[EXT_PER];
#pragma unroll
    for (int k = 0; k < EXT_PER; k++) {
        const long long id = base + k * BLOCK + threadIdx.x;
        f[k] = false;
        if (id < M) {
            const unsigned l = label[id];
            const unsigned sz = l != VMAP_NOID ? csize[l] : 0u;
            f[k] = l != VMAP_NOID && sz < min_size;
            if (label_out) label_out[id] = l;
            if (size_out) size_out[id] = sz;
        }
        const unsigned long long m = __ballot(f[k]);  // (every lane of the wave arrives here)
        below[k] = ext_lanes_below(m);
        if (lane == 0) wcnt[k][wave] = (unsigned)__popcll(m);
    }
    __syncthreads();
    if (!small_ids) return;
    unsigned long long pos = ext_tile_offset(off, blk, tile);
#pragma unroll
    for (int k = 0; k < EXT_PER; k++) {
        unsigned lower = 0, round = 0;
#pragma unroll
        for (int v = 0; v < EXT_WAVES; v++) {
            const unsigned c = wcnt[k][v];
            if (v < wave) lower += c;
            round += c;
        }
        if (f[k]) small_ids[pos + lower + below[k]] = (unsigned)(base + k * BLOCK + threadIdx.x);
        pos += round;
    }
}

}  // namespace sdm
