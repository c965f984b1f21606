// sdm_vmap_class.h -- classification of the persistent voxel map's entries on the device (sdm_vmap_classify,
// sdm_vmap_fetch_published; included by sdm_engine.hip).  A rule over the per-entry state -- multiplicity, stored sigma,
// camera-list length, crossings, ends and the occupancy of the 26 adjacent cells -- says which entries are surface; every
// entry keeps a persistent `published` byte, and a call reports exactly the ids whose verdict differs from it.
//
// State on the device (the classification's own; table, records, evidence and observations are only read):
//   published[rec_cap]  one byte per entry, 0 or 1; allocated at the first classify, grown with the records
//   scratch[M]          per call: bit 0 = the entry's LOCAL tests pass, bit 1 = passing (LOCAL and the NEIGHBOUR test)
//
// One sdm_vmap_classify over the M entries id = 0 .. M-1:
//   k_vcls_local    one lane per entry: the five LOCAL tests into scratch[id] (a null ncam / crossings / ends reads as 0:
//                   no observe / carve has run).  The ratio test compares 128-bit products (mul_hi and mul_lo)
//   k_vcls_count    (a later launch: it needs every LOCAL bit) tiles of EXT_TILE entries.  A LOCAL-passing entry, when
//                   min_neighbours > 0, forms its cell from its record as vox_key does and probes the up to 26 adjacent
//                   cells with vmap_find, read-only, adding the neighbours' LOCAL bits until min_neighbours is reached.
//                   It sets bit 1 of its own scratch byte -- the one lane that writes that byte; a lane that reads it as
//                   a neighbour sees the same bit 0 before and after -- and two flags per entry are counted per tile by
//                   ballot and popcount:  accept(id) = passing && !published,  retract(id) = !passing && published
//   k_extract_scan_tiles / k_extract_scan_sums   (sdm_extract.h, unchanged) scan both tile counts
//   k_vcls_totals   accepted, retracted and published_total for the host's one wait
//   k_vcls_commit   (queued only if the call is not refused) no probe again: from bit 1 and the flag the accept lanes write
//                   accepted_ids[rank], the retract lanes retracted_ids[rank]; with commit they flip their own flag
//   k_vcls_gather   sdm_vmap_fetch_published by ids
//
// No atomics: every position is a rank from the scans over id, so both lists are ascending and bitwise the same from run
// to run, whatever the table layout.  No lane waits for another; every probe is bounded by the capacity; every lane of a
// wave reaches every ballot.
#pragma once
#include "sdm_vmap_obs.h"

namespace sdm {

struct VclsRule {
    unsigned min_multiplicity, min_cameras;
    unsigned long long min_ends;
    unsigned ratio_num, ratio_den;
    unsigned max_sigma_key;  // f2key(max_sigma)
    int min_neighbours;      // 0 .. 26
};

struct VclsIn {
    const unsigned* multiplicity;         // [M]
    const float2* rho_sigma;              // [M]
    const unsigned* ncam;                 // [M] or null
    const unsigned long long* crossings;  // [M] or null
    const unsigned long long* ends;       // [M] or null
};

// a * b <= c * d as exact integers (b, d below 2^32: the products have 96 bits)
__device__ __forceinline__ bool vcls_prod_le(unsigned long long a, unsigned b, unsigned long long c, unsigned d)
{
    const unsigned long long lh = __umul64hi(a, (unsigned long long)b), ll = a * (unsigned long long)b;
    const unsigned long long rh = __umul64hi(c, (unsigned long long)d), rl = c * (unsigned long long)d;
    return lh < rh || (lh == rh && ll <= rl);
}

// one lane per entry id0 + thread
__global__ __launch_bounds__(BLOCK) void k_vcls_local(VclsIn in, VclsRule r, long long M, long long id0,
                                                      unsigned char* __restrict__ scratch)
{
    const long long id = id0 + (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (id >= M) return;
    const unsigned nc = in.ncam ? in.ncam[id] : 0u;
    const unsigned long long cr = in.crossings ? in.crossings[id] : 0ull, en = in.ends ? in.ends[id] : 0ull;
    const bool ok = in.multiplicity[id] >= r.min_multiplicity && nc >= r.min_cameras && en >= r.min_ends &&
                    vcls_prod_le(cr, r.ratio_den, en, r.ratio_num) && f2key(in.rho_sigma[id].y) <= r.max_sigma_key;
    scratch[id] = ok ? 1u : 0u;
}

// LOCAL-passing entries among the 26 cells adjacent to the cell of (x, y, z), counted up to `want`
__device__ __forceinline__ int vcls_neighbours(const VmapTable& tb, const unsigned char* scratch, unsigned M, float x, float y,
                                               float z, float inv, int want)
{
    const int cx = (int)floorf(x * inv), cy = (int)floorf(y * inv), cz = (int)floorf(z * inv);  // (in range: the entry exists)
    int nb = 0;
    for (int q = 0; q < 27 && nb < want; q++) {
        if (q == 13) continue;  // the entry's own cell
        const int nx = cx + q / 9 - 1, ny = cy + (q / 3) % 3 - 1, nz = cz + q % 3 - 1;
        const int lim = 1 << 20;
        if (nx < -lim || nx >= lim || ny < -lim || ny >= lim || nz < -lim || nz >= lim) continue;  // holds nothing
        const unsigned id = vmap_find(tb, vmap_cell_key(nx, ny, nz));
        if (id < M) nb += scratch[id] & 1;  // (VMAP_NOID is not below M)
    }
    return nb;
}

// bit 0: accept, bit 1: retract of entry id, from its scratch byte (bit 1 = passing) and its flag
__device__ __forceinline__ unsigned vcls_flags(unsigned s, unsigned pub)
{
    const bool passing = (s & 2u) != 0u;
    return (passing && !pub ? 1u : 0u) | (!passing && pub ? 2u : 0u);
}

// one workgroup per tile tile0 + block of EXT_TILE consecutive entries
__global__ __launch_bounds__(BLOCK) void k_vcls_count(VmapTable tb, const float* __restrict__ xyz, float inv, int min_neighbours,
                                                      long long M, long long tile0, unsigned char* scratch,
                                                      const unsigned char* __restrict__ published,
                                                      unsigned* __restrict__ cnt_acc, unsigned* __restrict__ cnt_ret)
{
    __shared__ unsigned wsum[2][EXT_WAVES];
    const long long tile = tile0 + blockIdx.x;
    const long long base = tile * EXT_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned a = 0, b = 0;
#pragma unroll 1
    for (int k = 0; k < EXT_PER; k++) {
        const long long id = base + k * BLOCK + threadIdx.x;
        unsigned f = 0;
        if (id < M) {
            unsigned s = scratch[id] & 1u;
            if (s && (min_neighbours == 0 ||
                      vcls_neighbours(tb, scratch, (unsigned)M, xyz[id * 3 + 0], xyz[id * 3 + 1], xyz[id * 3 + 2], inv,
                                      min_neighbours) >= min_neighbours)) {
                s |= 2u;
                scratch[id] = (unsigned char)s;
            }
            f = vcls_flags(s, published[id]);
        }
        a += (unsigned)__popcll(__ballot(f & 1u));  // (every lane of the wave arrives here)
        b += (unsigned)__popcll(__ballot(f & 2u));
    }
    if (lane == 0) wsum[0][wave] = a, wsum[1][wave] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned ta = 0, tr = 0;
        for (int v = 0; v < EXT_WAVES; v++) ta += wsum[0][v], tr += wsum[1][v];
        cnt_acc[tile] = ta;
        cnt_ret[tile] = tr;
    }
}

// out = {accepted, retracted, published after the call}
__global__ void k_vcls_totals(long long nt, const unsigned* __restrict__ off_acc, const unsigned long long* __restrict__ blk_acc,
                              const unsigned* __restrict__ off_ret, const unsigned long long* __restrict__ blk_ret,
                              unsigned long long published_before, int commit, unsigned long long* __restrict__ out)
{
    if (blockIdx.x || threadIdx.x) return;
    const unsigned long long acc = ext_tile_offset(off_acc, blk_acc, nt), ret = ext_tile_offset(off_ret, blk_ret, nt);
    out[0] = acc;
    out[1] = ret;
    out[2] = commit ? published_before + acc - ret : published_before;
}

// accept and retract lanes list their id at their rank; with commit they flip their flag (no other lane touches it)
__global__ __launch_bounds__(BLOCK) void k_vcls_commit(const unsigned char* __restrict__ scratch, unsigned char* __restrict__ published,
                                                       int commit, long long M, long long tile0,
                                                       const unsigned* __restrict__ off_acc,
                                                       const unsigned long long* __restrict__ blk_acc,
                                                       const unsigned* __restrict__ off_ret,
                                                       const unsigned long long* __restrict__ blk_ret,
                                                       unsigned* __restrict__ accepted_ids, unsigned* __restrict__ retracted_ids)
{
    __shared__ unsigned wcnt[2][EXT_PER][EXT_WAVES];
    const long long tile = tile0 + blockIdx.x;
    const long long base = tile * EXT_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned f[EXT_PER], below_a[EXT_PER], below_r[EXT_PER];
#pragma unroll
    for (int k = 0; k < EXT_PER; k++) {
        const long long id = base + k * BLOCK + threadIdx.x;
        f[k] = id < M ? vcls_flags(scratch[id], published[id]) : 0u;
        const unsigned long long ma = __ballot(f[k] & 1u), mr = __ballot(f[k] & 2u);
        below_a[k] = ext_lanes_below(ma);
        below_r[k] = ext_lanes_below(mr);
        if (lane == 0) wcnt[0][k][wave] = (unsigned)__popcll(ma), wcnt[1][k][wave] = (unsigned)__popcll(mr);
    }
    __syncthreads();
    unsigned long long pos_a = ext_tile_offset(off_acc, blk_acc, tile), pos_r = ext_tile_offset(off_ret, blk_ret, tile);
#pragma unroll
    for (int k = 0; k < EXT_PER; k++) {
        unsigned lower_a = 0, round_a = 0, lower_r = 0, round_r = 0;
#pragma unroll
        for (int v = 0; v < EXT_WAVES; v++) {
            const unsigned ca = wcnt[0][k][v], cr = wcnt[1][k][v];
            if (v < wave) lower_a += ca, lower_r += cr;
            round_a += ca, round_r += cr;
        }
        const unsigned id = (unsigned)(base + k * BLOCK + threadIdx.x);
        if (f[k] & 1u) {
            if (accepted_ids) accepted_ids[pos_a + lower_a + below_a[k]] = id;
            if (commit) published[id] = 1;
        } else if (f[k] & 2u) {
            if (retracted_ids) retracted_ids[pos_r + lower_r + below_r[k]] = id;
            if (commit) published[id] = 0;
        }
        pos_a += round_a, pos_r += round_r;
    }
}

// fetch by ids: the flag of entry ids[j] -> out[j], j = j0 + thread (a null `published` reads as 0: no classify has run);
// *bad |= 1 for an id >= M
__global__ __launch_bounds__(BLOCK) void k_vcls_gather(const unsigned char* __restrict__ published, const unsigned* __restrict__ ids,
                                                       long long count, long long j0, unsigned M, unsigned char* __restrict__ out,
                                                       unsigned* __restrict__ bad)
{
    const long long j = j0 + (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= count) return;
    const unsigned e = ids[j];
    if (e >= M) {
        atomicOr(bad, 1u);
        return;
    }
    out[j] = published ? published[e] : (unsigned char)0;
}

}  // namespace sdm
