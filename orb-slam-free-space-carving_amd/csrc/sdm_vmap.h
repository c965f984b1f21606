// sdm_vmap.h -- the persistent voxel map (sdm_vmap_*, included by sdm_engine.hip): one entry per voxel ever seen, kept in
// the context across calls and merged incrementally with each call's plain cloud.
//
// State on the device:
//   table   open-addressed, linear probing, load <= 0.5 (sdm_voxel.h's cell key, vox_mix and probe):
//             keys[cap]   cell key or VOX_EMPTY            id[cap]    the voxel's entry id or VMAP_NOID (claimed this call)
//           and three per-call fields that hold their reduction's identity between calls:
//             cval[cap]   min of f2key(sigma) << 32 | g    cfirst[cap] min of g          ccnt[cap]  points of the call
//   records structure-of-arrays indexed by id: xyz, pixel, rho_sigma, intensity, tag, multiplicity, epoch
//
// One sdm_vmap_integrate over the T staged plain points g = 0 .. T-1 (the host has grown table and records before):
//   k_vmap_insert   one lane per point: claims or finds the key (atomicCAS), reduces the three per-call fields at the table
//                   position (atomicMin, atomicMin, atomicAdd) and notes the position in where[g]; an unmergeable point
//                   gets VOX_NONE and is counted as dropped (one atomicAdd per wave)
//   k_vmap_count    tiles of EXT_TILE points, two flags per point:
//                     creator(g) = g is the first point of a voxel without an id
//                     updater(g) = g is the call's winner of a voxel with an id and its key is strictly below the stored one
//   k_extract_scan_tiles / k_extract_scan_sums   (sdm_extract.h, unchanged) scan both tile counts
//   k_vmap_totals   created, updated, dropped and the overflow flag for the host's one wait
//   k_vmap_ids      creators take id = first_created + rank; every voxel's first-point lane -- the one lane per touched
//                   voxel -- adds the call count to the multiplicity (saturating) or starts it
//   k_vmap_commit   (a later launch: it needs every id) the call's winner of a new or beaten voxel writes the record, the tag
//                   and the epoch at the id; updaters write updated_ids[rank].  The winner lane then puts cval back to its
//                   identity and the first-point lane cfirst and ccnt: no memset over the table, and a lane that still reads
//                   one of them sees either the call's value or the identity, neither of which names it.
//   k_vmap_rehash   (growth only) one lane per old slot re-inserts (key, id) into the new table
//   k_vmap_gather   sdm_vmap_fetch by ids: the requested fields of entries ids[0 .. count) into dense arrays
//
// No lane waits for another; every probe is bounded by the capacity (a lane that exhausts it raises the overflow flag, which
// cannot happen at load <= 0.5).  Which slot a voxel lands in depends on the order of the CAS, so the table's LAYOUT differs
// from run to run; everything that leaves the map does not: the reductions are integer minima and sums, ids and the order
// of updated_ids come from scans over g, and a record is written by exactly one lane.
#pragma once
#include "sdm_voxel.h"

namespace sdm {

constexpr unsigned VMAP_NOID = 0xffffffffu;  // id of a key claimed in the running call (ids stay below 2^30)

struct VmapTable {
    unsigned long long* keys;  // [cap]
    unsigned* id;              // [cap]
    unsigned long long* cval;  // [cap] per call; identity ~0
    unsigned* cfirst;          // [cap] per call; identity ~0
    unsigned* ccnt;            // [cap] per call; identity 0
    unsigned long long mask;   // cap - 1, cap a power of two <= 2^31
};

struct VmapRecords {
    float* xyz;                // [cap][3]
    unsigned* pixel;           // [cap]
    float2* rho_sigma;         // [cap]
    unsigned char* intensity;  // [cap]
    int* tag;                  // [cap]
    unsigned* multiplicity;    // [cap]
    unsigned* epoch;           // [cap]
};

// the position of `key`: claimed if absent.  false: every slot holds another key
__device__ __forceinline__ bool vmap_claim(const VmapTable& tb, unsigned long long key, unsigned long long& h)
{
    h = vox_mix(key) & tb.mask;
    for (unsigned long long probe = 0; probe <= tb.mask; probe++) {  // bounded by the capacity
        const unsigned long long prev = atomicCAS(&tb.keys[h], VOX_EMPTY, key);
        if (prev == VOX_EMPTY || prev == key) return true;
        h = (h + 1) & tb.mask;
    }
    return false;
}

// one lane per plain point g0 + thread; ctr[0] += dropped points, ctr[1] |= overflow
__global__ __launch_bounds__(BLOCK) void k_vmap_insert(const float* __restrict__ xyz, const float2* __restrict__ rho_sigma,
                                                       long long T, long long g0, float inv, VmapTable tb,
                                                       unsigned* __restrict__ where, unsigned* __restrict__ ctr)
{
    const long long g = g0 + (long long)blockIdx.x * BLOCK + threadIdx.x;
    unsigned long long key = VOX_EMPTY;
    if (g < T) key = vox_key(xyz[g * 3 + 0], xyz[g * 3 + 1], xyz[g * 3 + 2], inv);
    const unsigned long long drop = __ballot(g < T && key == VOX_EMPTY);
    if (drop && (threadIdx.x & 63) == 0) atomicAdd(&ctr[0], (unsigned)__popcll(drop));
    if (g >= T) return;
    if (key == VOX_EMPTY) {
        where[g] = VOX_NONE;
        return;
    }
    unsigned long long h;
    if (!vmap_claim(tb, key, h)) {
        atomicOr(&ctr[1], 1u);
        where[g] = VOX_NONE;
        return;
    }
    atomicMin(&tb.cval[h], ((unsigned long long)f2key(rho_sigma[g].y) << 32) | (unsigned long long)g);
    atomicMin(&tb.cfirst[h], (unsigned)g);
    atomicAdd(&tb.ccnt[h], 1u);
    where[g] = (unsigned)h;
}

// the two flags of point g before k_vmap_ids has run (bit 0: creator, bit 1: updater)
__device__ __forceinline__ unsigned vmap_flags(const VmapTable& tb, const VmapRecords& rec, const unsigned* __restrict__ where,
                                               long long g, long long T)
{
    if (g >= T) return 0u;
    const unsigned w = where[g];
    if (w == VOX_NONE) return 0u;
    const unsigned id = tb.id[w];
    if (id == VMAP_NOID) return tb.cfirst[w] == (unsigned)g ? 1u : 0u;
    const unsigned long long v = tb.cval[w];
    return ((unsigned)v == (unsigned)g && (unsigned)(v >> 32) < f2key(rec.rho_sigma[id].y)) ? 2u : 0u;
}

// one workgroup per tile tile0 + block of EXT_TILE consecutive plain points
__global__ __launch_bounds__(BLOCK) void k_vmap_count(VmapTable tb, VmapRecords rec, const unsigned* __restrict__ where,
                                                      long long T, long long tile0, unsigned* __restrict__ cnt_new,
                                                      unsigned* __restrict__ cnt_upd)
{
    __shared__ unsigned wsum[2][EXT_WAVES];
    const long long tile = tile0 + blockIdx.x;
    const long long base = tile * EXT_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned a = 0, b = 0;
#pragma unroll
    for (int k = 0; k < EXT_PER; k++) {
        const unsigned f = vmap_flags(tb, rec, where, base + k * BLOCK + threadIdx.x, T);
        a += (unsigned)__popcll(__ballot(f & 1u));
        b += (unsigned)__popcll(__ballot(f & 2u));
    }
    if (lane == 0) wsum[0][wave] = a, wsum[1][wave] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned ta = 0, tb2 = 0;
        for (int v = 0; v < EXT_WAVES; v++) ta += wsum[0][v], tb2 += wsum[1][v];
        cnt_new[tile] = ta;
        cnt_upd[tile] = tb2;
    }
}

// out = {created, updated, dropped, overflow}
__global__ void k_vmap_totals(long long nt, const unsigned* __restrict__ off_new, const unsigned long long* __restrict__ blk_new,
                              const unsigned* __restrict__ off_upd, const unsigned long long* __restrict__ blk_upd,
                              const unsigned* __restrict__ ctr, unsigned long long* __restrict__ out)
{
    if (blockIdx.x || threadIdx.x) return;
    out[0] = ext_tile_offset(off_new, blk_new, nt);
    out[1] = ext_tile_offset(off_upd, blk_upd, nt);
    out[2] = ctr[0];
    out[3] = ctr[1];
}

// creators take their ids; first-point lanes add the call's count to the multiplicity
__global__ __launch_bounds__(BLOCK) void k_vmap_ids(VmapTable tb, VmapRecords rec, const unsigned* __restrict__ where,
                                                    unsigned first_created, long long T, long long tile0,
                                                    const unsigned* __restrict__ off_new,
                                                    const unsigned long long* __restrict__ blk_new)
{
    __shared__ unsigned wcnt[EXT_PER][EXT_WAVES];
    const long long tile = tile0 + blockIdx.x;
    const long long base = tile * EXT_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned w[EXT_PER], below[EXT_PER];
    bool f[EXT_PER], first[EXT_PER];
#pragma unroll
    for (int k = 0; k < EXT_PER; k++) {
        const long long g = base + k * BLOCK + threadIdx.x;
        w[k] = VOX_NONE;
        if (g < T) w[k] = where[g];
        first[k] = w[k] != VOX_NONE && tb.cfirst[w[k]] == (unsigned)g;
        f[k] = first[k] && tb.id[w[k]] == VMAP_NOID;  // (only this lane changes the id of its voxel)
        const unsigned long long m = __ballot(f[k]);
        below[k] = ext_lanes_below(m);
        if (lane == 0) wcnt[k][wave] = (unsigned)__popcll(m);
    }
    __syncthreads();
    unsigned long long pos = ext_tile_offset(off_new, blk_new, tile);
#pragma unroll
    for (int k = 0; k < EXT_PER; k++) {
        unsigned lower = 0, round = 0;
#pragma unroll
        for (int v = 0; v < EXT_WAVES; v++) {
            const unsigned c = wcnt[k][v];
            if (v < wave) lower += c;
            round += c;
        }
        if (f[k]) {
            const unsigned id = first_created + (unsigned)(pos + lower + below[k]);
            tb.id[w[k]] = id;
            rec.multiplicity[id] = tb.ccnt[w[k]];
        } else if (first[k]) {
            const unsigned id = tb.id[w[k]];
            const unsigned have = rec.multiplicity[id], add = tb.ccnt[w[k]];
            rec.multiplicity[id] = have + add < have ? 0xffffffffu : have + add;  // saturates at 2^32 - 1
        }
        pos += round;
    }
}

// the slot index of plain point g: the last i < n with offsets[i] <= g (an empty slot shares its offset with the next)
__device__ __forceinline__ int vmap_slot_of(const unsigned long long* __restrict__ offsets, int n, unsigned long long g)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (offsets[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// winners of new or beaten voxels write their record; updaters list their id; the per-call fields go back to identity
__global__ __launch_bounds__(BLOCK) void k_vmap_commit(VmapTable tb, VmapRecords rec, const unsigned* __restrict__ where,
                                                       unsigned first_created, unsigned epoch, long long T, long long tile0,
                                                       const unsigned* __restrict__ off_upd,
                                                       const unsigned long long* __restrict__ blk_upd, ExtractOut src,
                                                       const unsigned long long* __restrict__ plain_offsets,
                                                       const int* __restrict__ tags, int n,
                                                       unsigned* __restrict__ updated_ids)
{
    __shared__ unsigned wcnt[EXT_PER][EXT_WAVES];
    const long long tile = tile0 + blockIdx.x;
    const long long base = tile * EXT_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned w[EXT_PER], below[EXT_PER], id[EXT_PER];
    bool upd[EXT_PER], win[EXT_PER], first[EXT_PER];
#pragma unroll
    for (int k = 0; k < EXT_PER; k++) {
        const long long g = base + k * BLOCK + threadIdx.x;
        w[k] = VOX_NONE;
        if (g < T) w[k] = where[g];
        upd[k] = win[k] = first[k] = false;
        id[k] = VMAP_NOID;
        if (w[k] != VOX_NONE) {
            const unsigned long long v = tb.cval[w[k]];
            first[k] = tb.cfirst[w[k]] == (unsigned)g;
            if ((unsigned)v == (unsigned)g) {  // the call's winner of its voxel: the one lane that touches record id
                id[k] = tb.id[w[k]];
                win[k] = id[k] >= first_created;
                upd[k] = !win[k] && (unsigned)(v >> 32) < f2key(rec.rho_sigma[id[k]].y);
                tb.cval[w[k]] = ~0ull;
            }
        }
        const unsigned long long m = __ballot(upd[k]);
        below[k] = ext_lanes_below(m);
        if (lane == 0) wcnt[k][wave] = (unsigned)__popcll(m);
    }
    __syncthreads();
    unsigned long long pos = ext_tile_offset(off_upd, blk_upd, tile);
#pragma unroll
    for (int k = 0; k < EXT_PER; k++) {
        unsigned lower = 0, round = 0;
#pragma unroll
        for (int v = 0; v < EXT_WAVES; v++) {
            const unsigned c = wcnt[k][v];
            if (v < wave) lower += c;
            round += c;
        }
        const long long g = base + k * BLOCK + threadIdx.x;
        if (win[k] || upd[k]) {
            const unsigned e = id[k];
            rec.xyz[(size_t)e * 3 + 0] = src.xyz[g * 3 + 0];
            rec.xyz[(size_t)e * 3 + 1] = src.xyz[g * 3 + 1];
            rec.xyz[(size_t)e * 3 + 2] = src.xyz[g * 3 + 2];
            rec.pixel[e] = src.pixel[g];
            rec.rho_sigma[e] = src.rho_sigma[g];
            rec.intensity[e] = src.intensity[g];
            rec.tag[e] = tags[vmap_slot_of(plain_offsets, n, (unsigned long long)g)];
            rec.epoch[e] = epoch;
            if (upd[k] && updated_ids) updated_ids[pos + lower + below[k]] = e;
        }
        if (first[k]) {
            tb.cfirst[w[k]] = ~0u;
            tb.ccnt[w[k]] = 0u;
        }
        pos += round;
    }
}

// growth: one lane per slot h0 + thread of the old table re-inserts (key, id) into `nw` (its per-call fields were set to
// their identities when it was made)
__global__ __launch_bounds__(BLOCK) void k_vmap_rehash(const unsigned long long* __restrict__ old_keys,
                                                       const unsigned* __restrict__ old_id, unsigned long long old_cap,
                                                       unsigned long long h0, VmapTable nw, unsigned* __restrict__ ctr)
{
    const unsigned long long s = h0 + (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= old_cap) return;
    const unsigned long long key = old_keys[s];
    if (key == VOX_EMPTY) return;
    unsigned long long h;
    if (!vmap_claim(nw, key, h)) {
        atomicOr(&ctr[1], 1u);
        return;
    }
    nw.id[h] = old_id[s];
}

// fetch by ids: entry ids[j] -> position j0 + thread of the dense destinations (any may be null); *bad |= 1 for an id >= M
__global__ __launch_bounds__(BLOCK) void k_vmap_gather(VmapRecords rec, const unsigned* __restrict__ ids, long long count,
                                                       long long j0, unsigned M, VmapRecords dst, unsigned* __restrict__ bad)
{
    const long long j = j0 + (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= count) return;
    const unsigned e = ids[j];
    if (e >= M) {
        atomicOr(bad, 1u);
        return;
    }
    if (dst.xyz) {
        dst.xyz[j * 3 + 0] = rec.xyz[(size_t)e * 3 + 0];
        dst.xyz[j * 3 + 1] = rec.xyz[(size_t)e * 3 + 1];
        dst.xyz[j * 3 + 2] = rec.xyz[(size_t)e * 3 + 2];
    }
    if (dst.pixel) dst.pixel[j] = rec.pixel[e];
    if (dst.rho_sigma) dst.rho_sigma[j] = rec.rho_sigma[e];
    if (dst.intensity) dst.intensity[j] = rec.intensity[e];
    if (dst.tag) dst.tag[j] = rec.tag[e];
    if (dst.multiplicity) dst.multiplicity[j] = rec.multiplicity[e];
    if (dst.epoch) dst.epoch[j] = rec.epoch[e];
}

}  // namespace sdm
