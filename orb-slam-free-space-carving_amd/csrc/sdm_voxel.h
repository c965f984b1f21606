// sdm_voxel.h -- one point per voxel across keyframes (sdm_extract_points_voxel, included by sdm_engine.hip).
//
// The plain extraction (sdm_extract.h) first runs into engine-owned staging: T points g = 0 .. T-1 in its order.  Then,
// over those compacted points:
//   k_voxel_insert    one lane per point: cell = floorf(xyz * inv) per coordinate; a point whose three cells lie in
//                     [-2^20, 2^20) is mergeable and enters an open-addressed hash table (linear probing, load <= 0.5)
//                     under its 63-bit cell key: atomicCAS claims the key slot, atomicMin reduces (f2key(sigma) << 32 | g),
//                     atomicAdd counts.  The lane notes its table position in where[g] (VOX_NONE: unmergeable), so no
//                     later pass probes.  No lane waits for another, and the probe is bounded by the capacity (a lane
//                     that exhausts it raises a flag the host turns into an error; impossible at load <= 0.5).
//   k_voxel_count     tiles of EXT_TILE points: kept(g) = where[g] is VOX_NONE or the table value's low word is g
//   k_extract_scan_tiles / k_extract_scan_sums   (sdm_extract.h, unchanged) scan the tile counts
//   k_voxel_offsets   the kept rank of each slot's first plain point, the kept total M, the overflow flag
//   k_voxel_write     kept again; position as in k_extract_write; gathers the requested fields from the staging, writes
//                     multiplicity and source_index, and leaves the kept rank at the winner's table position
//   k_voxel_rep       representative[g] = the rank left at where[g] (a separate launch: it needs every rank)
//
// Reproducibility: which table slot a voxel lands in depends on the order in which the lanes' CAS arrive, so the table's
// LAYOUT differs from run to run.  The OUTPUT does not: a voxel's value is the minimum of an order-independent integer
// reduction, its count an integer sum, and only the winner's identity (the value's low word) decides what is kept; the
// positions come from a scan.  Every returned array is therefore bitwise the same from run to run.
#pragma once
#include "sdm_extract.h"
#include "sdm_priors.h"  // f2key

namespace sdm {

constexpr unsigned long long VOX_EMPTY = ~0ull;  // key slot not claimed (a cell key has 63 bits)
constexpr unsigned VOX_NONE = 0xffffffffu;       // where[g] of an unmergeable point
constexpr float VOX_CELL_LIM = 1048576.0f;       // 2^20: cells are [-2^20, 2^20), 21 bits each after the bias

struct VoxTable {
    unsigned long long* keys;  // [cap] cell key or VOX_EMPTY
    unsigned long long* vals;  // [cap] min over the voxel's points of f2key(sigma) << 32 | g
    unsigned* cnt;             // [cap] points in the voxel
    unsigned* rank;            // [cap] kept rank of the voxel's winner (k_voxel_write)
    unsigned long long mask;   // cap - 1, cap a power of two <= 2^31
};

__device__ __forceinline__ unsigned long long vox_mix(unsigned long long z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;  // SplitMix64 finaliser (seg_hash_term's)
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the cell key of a point, or VOX_EMPTY if it is unmergeable (a cell outside [-2^20, 2^20), NaN, +-Inf)
__device__ __forceinline__ unsigned long long vox_key(float x, float y, float z, float inv)
{
    const float cx = floorf(x * inv), cy = floorf(y * inv), cz = floorf(z * inv);
    const bool ok = cx >= -VOX_CELL_LIM && cx < VOX_CELL_LIM && cy >= -VOX_CELL_LIM && cy < VOX_CELL_LIM &&
                    cz >= -VOX_CELL_LIM && cz < VOX_CELL_LIM;  // (every compare is false for a NaN)
    if (!ok) return VOX_EMPTY;
    const unsigned long long bx = (unsigned long long)((int)cx + (1 << 20)), by = (unsigned long long)((int)cy + (1 << 20)),
                             bz = (unsigned long long)((int)cz + (1 << 20));
    return (bx << 42) | (by << 21) | bz;
}

// one lane per plain point g0 + thread (g0: the slice's first point)
__global__ __launch_bounds__(BLOCK) void k_voxel_insert(const float* __restrict__ xyz, const float2* __restrict__ rho_sigma,
                                                        long long T, long long g0, float inv, VoxTable tb,
                                                        unsigned* __restrict__ where, unsigned* __restrict__ overflow)
{
    const long long g = g0 + (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= T) return;
    const unsigned long long key = vox_key(xyz[g * 3 + 0], xyz[g * 3 + 1], xyz[g * 3 + 2], inv);
    if (key == VOX_EMPTY) {
        where[g] = VOX_NONE;
        return;
    }
    unsigned long long h = vox_mix(key) & tb.mask;
    bool found = false;
    for (unsigned long long probe = 0; probe <= tb.mask; probe++) {  // bounded by the capacity
        const unsigned long long prev = atomicCAS(&tb.keys[h], VOX_EMPTY, key);
        if (prev == VOX_EMPTY || prev == key) {
            found = true;
            break;
        }
        h = (h + 1) & tb.mask;
    }
    if (!found) {  // every slot holds another key
        atomicOr(overflow, 1u);
        where[g] = VOX_NONE;
        return;
    }
    atomicMin(&tb.vals[h], ((unsigned long long)f2key(rho_sigma[g].y) << 32) | (unsigned long long)g);
    atomicAdd(&tb.cnt[h], 1u);
    where[g] = (unsigned)h;
}

// point g is kept iff it is unmergeable or its voxel's winner; *w = where[g]
__device__ __forceinline__ bool vox_kept(const VoxTable& tb, const unsigned* __restrict__ where, long long g, long long T,
                                         unsigned& w)
{
    if (g >= T) return false;
    w = where[g];
    return w == VOX_NONE || (unsigned)tb.vals[w] == (unsigned)g;
}

// one workgroup per tile tile0 + block of EXT_TILE consecutive plain points; round k covers points k*BLOCK + thread
__global__ __launch_bounds__(BLOCK) void k_voxel_count(VoxTable tb, const unsigned* __restrict__ where, long long T,
                                                       long long tile0, unsigned* __restrict__ tile_cnt)
{
    __shared__ unsigned wsum[EXT_WAVES];
    const long long tile = tile0 + blockIdx.x;
    const long long base = tile * EXT_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned mine = 0;
#pragma unroll
    for (int k = 0; k < EXT_PER; k++) {
        unsigned w;
        const bool f = vox_kept(tb, where, base + k * BLOCK + threadIdx.x, T, w);
        mine += (unsigned)__popcll(__ballot(f));
    }
    if (lane == 0) wsum[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = 0;
        for (int w = 0; w < EXT_WAVES; w++) t += wsum[w];
        tile_cnt[tile] = t;
    }
}

// one workgroup per i <= n + 1: offsets[i] = kept rank of the first plain point of slot i (i < n), offsets[n] = the kept
// total, offsets[n + 1] = the overflow flag.  The rank of plain point g = its tile's offset + the kept points of the tile
// before it.
__global__ __launch_bounds__(BLOCK) void k_voxel_offsets(VoxTable tb, const unsigned* __restrict__ where, long long T,
                                                         const unsigned long long* __restrict__ plain_offsets, int n,
                                                         long long nt, const unsigned* __restrict__ tile_off,
                                                         const unsigned long long* __restrict__ blk_off,
                                                         const unsigned* __restrict__ overflow,
                                                         unsigned long long* __restrict__ offsets)
{
    __shared__ unsigned before;
    const int i = blockIdx.x;
    if (i == n + 1) {
        if (threadIdx.x == 0) offsets[i] = *overflow;
        return;
    }
    if (i == n) {
        if (threadIdx.x == 0) offsets[i] = ext_tile_offset(tile_off, blk_off, nt);
        return;
    }
    const long long g = (long long)plain_offsets[i];  // (<= T)
    const long long tile = g / EXT_TILE;               // (<= nt: tile_off has nt + 1 entries)
    const int r = (int)(g - tile * EXT_TILE);
    if (threadIdx.x == 0) before = 0;
    __syncthreads();
    for (int j0 = 0; j0 < r; j0 += BLOCK) {  // (uniform trip count: the ballot sees whole waves)
        const int j = j0 + threadIdx.x;
        unsigned w;
        const bool f = j < r && vox_kept(tb, where, tile * EXT_TILE + j, T, w);
        const unsigned long long m = __ballot(f);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(&before, (unsigned)__popcll(m));
    }
    __syncthreads();
    if (threadIdx.x == 0) offsets[i] = ext_tile_offset(tile_off, blk_off, tile) + before;
}

// the same walk as k_voxel_count; every kept point learns its rank as in k_extract_write and gathers its fields from the
// staging `src` (the plain extraction) to `dst`
__global__ __launch_bounds__(BLOCK) void k_voxel_write(VoxTable tb, const unsigned* __restrict__ where, long long T,
                                                       long long tile0, const unsigned* __restrict__ tile_off,
                                                       const unsigned long long* __restrict__ blk_off, ExtractOut src,
                                                       ExtractOut dst, unsigned* __restrict__ multiplicity,
                                                       unsigned* __restrict__ source_index,
                                                       unsigned* __restrict__ representative)
{
    __shared__ unsigned wcnt[EXT_PER][EXT_WAVES];
    const long long tile = tile0 + blockIdx.x;
    const long long base = tile * EXT_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned w[EXT_PER], below[EXT_PER];
    bool f[EXT_PER];
#pragma unroll
    for (int k = 0; k < EXT_PER; k++) {
        f[k] = vox_kept(tb, where, base + k * BLOCK + threadIdx.x, T, w[k]);
        const unsigned long long m = __ballot(f[k]);
        below[k] = ext_lanes_below(m);
        if (lane == 0) wcnt[k][wave] = (unsigned)__popcll(m);
    }
    __syncthreads();
    unsigned long long pos = ext_tile_offset(tile_off, blk_off, tile);
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
            const long long g = base + k * BLOCK + threadIdx.x;
            const unsigned long long o = pos + lower + below[k];
            if (dst.xyz) {
                dst.xyz[o * 3 + 0] = src.xyz[g * 3 + 0];
                dst.xyz[o * 3 + 1] = src.xyz[g * 3 + 1];
                dst.xyz[o * 3 + 2] = src.xyz[g * 3 + 2];
            }
            if (dst.pixel) dst.pixel[o] = src.pixel[g];
            if (dst.rho_sigma) dst.rho_sigma[o] = src.rho_sigma[g];
            if (dst.intensity) dst.intensity[o] = src.intensity[g];
            if (multiplicity) multiplicity[o] = w[k] == VOX_NONE ? 1u : tb.cnt[w[k]];
            if (source_index) source_index[o] = (unsigned)g;
            if (w[k] != VOX_NONE) tb.rank[w[k]] = (unsigned)o;
            else if (representative) representative[g] = (unsigned)o;  // (its own; k_voxel_rep fills the mergeable ones)
        }
        pos += round;
    }
}

// one lane per plain point: the rank k_voxel_write left at the point's voxel (an unmergeable point already has its own)
__global__ __launch_bounds__(BLOCK) void k_voxel_rep(VoxTable tb, const unsigned* __restrict__ where, long long T,
                                                     long long g0, unsigned* __restrict__ representative)
{
    const long long g = g0 + (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= T) return;
    const unsigned w = where[g];
    if (w != VOX_NONE) representative[g] = tb.rank[w];
}

}  // namespace sdm
