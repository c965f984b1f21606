// sdm_extract.h -- device-side extraction of the filtered semi-dense point cloud (sdm_extract_points, included by
// sdm_engine.hip).
//
// The filter every consumer of a keyframe applies (SavePointCloudObj PM.cc:100-132, the transcript writer, the adapter's
// finished-keyframe hand-over):
//
//     keep pixel (y, x)  iff  !(sigma > max_sigma) && (rho > min_rho)      in double, raster order
//
// as a stable stream compaction over a batch of slots: keyframes in the order given, pixels in raster order within each.
// A slot's items are either the entries of its active-pixel list (already raster order; used when the rho plane is zero
// outside the list) or all W*H pixels of the plane.  Items are cut into tiles of EXT_TILE consecutive items of one slot:
//   k_extract_count        pass 1: passing items per tile (64-bit ballot + popcount, wave totals summed in LDS)
//   k_extract_scan_tiles   pass 2a: exclusive scan of the tile counts per EXT_SCAN tiles, workgroup totals
//   k_extract_scan_sums    pass 2b: exclusive scan of the workgroup totals (one workgroup, any length)
//   k_extract_offsets      each slot's first point and the total
//   k_extract_write        pass 3: the predicate again; position = tile offset + earlier rounds / waves (LDS) + mbcnt
// No atomics anywhere: every position is a function of the inputs, so the output is the same from run to run.
//
// The double compares are done in float against thresholds derived on the host (ext_float_floor): for a float v and a
// double t, (double)v > t  <=>  v > F(t), F(t) = the largest float <= t (NaN for NaN).
#pragma once
#include "sdm_ingest.h"

namespace sdm {

constexpr int EXT_PER = 8;                  // items per thread and tile round
constexpr int EXT_TILE = BLOCK * EXT_PER;   // items per tile (one workgroup)
constexpr int EXT_SCAN = BLOCK * EXT_PER;   // tile counts one scan workgroup covers
constexpr int EXT_WAVES = BLOCK / 64;

struct ExtractSlot {
    long long tile0;  // first tile of the slot; the tiles of slot i are [tile0, tile0 of slot i + 1)
    int slot;
    int count;        // items: list length (list path) or W*H
    int list;         // 1: items are active-list entries, 0: pixels of the whole plane
    int pad;
};

struct ExtractOut {
    float* xyz;            // [total][3] or null
    unsigned* pixel;       // [total] (y << 16) | x or null
    float2* rho_sigma;     // [total] or null
    unsigned char* intensity;  // [total] or null
};

struct ExtractIn {
    const ExtractSlot* tab;
    int n;
    const float2* pool;   // {rho, sigma}
    const float* chk;     // checked rho (source 1) or null (source 0: rho = pool.x)
    const unsigned* act;  // active lists
    const float* xyz;     // SemiDensePointSets_ planes
    const float4* rec;    // search records (.w low byte = im(y,x))
    long long P;
    int W;
    float sig_max, rho_min;  // ext_float_floor(max_sigma), ext_float_floor(min_rho)
};

// the slot whose tiles contain `tile`: the last entry with tile0 <= tile (an empty slot shares its tile0 with the next
// slot, so the last such entry is never an empty one)
__device__ __forceinline__ int ext_find_slot(const ExtractSlot* __restrict__ tab, int n, long long tile)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].tile0 <= tile) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// item j of slot d: its plane index, pixel code, rho and sigma; true iff it passes the filter
__device__ __forceinline__ bool ext_item(const ExtractIn& in, const ExtractSlot& d, long long j, long long& idx,
                                         unsigned& code, float& rho, float& sigma)
{
    if (j >= d.count) return false;
    const long long plane = (long long)d.slot * in.P;
    if (d.list) {
        code = in.act[plane + j];
        idx = (long long)(code >> 16) * in.W + (code & 0xffffu);
    } else {
        const int i = (int)j;  // (j < count = W*H)
        const int y = i / in.W;
        idx = i;
        code = ((unsigned)y << 16) | (unsigned)(i - y * in.W);
    }
    const float2 v = in.pool[plane + idx];
    rho = in.chk ? in.chk[plane + idx] : v.x;
    sigma = v.y;
    return !(sigma > in.sig_max) && (rho > in.rho_min);  // NaN sigma passes, NaN rho fails (as in double)
}

__device__ __forceinline__ unsigned ext_lanes_below(unsigned long long m)
{
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// pass 1: one workgroup per tile; round k covers items k*BLOCK + threadIdx.x of the tile
__global__ __launch_bounds__(BLOCK) void k_extract_count(ExtractIn in, unsigned* __restrict__ tile_cnt)
{
    __shared__ unsigned wsum[EXT_WAVES];
    const long long tile = blockIdx.x;
    const ExtractSlot d = in.tab[ext_find_slot(in.tab, in.n, tile)];
    const long long base = (tile - d.tile0) * EXT_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned mine = 0;
#pragma unroll
    for (int k = 0; k < EXT_PER; k++) {
        long long idx;
        unsigned code;
        float rho, sigma;
        const bool f = ext_item(in, d, base + k * BLOCK + threadIdx.x, idx, code, rho, sigma);
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

// exclusive scan of one value per thread across the workgroup; *total = the workgroup's sum
template <typename T>
__device__ __forceinline__ T ext_block_scan(T v, T* total)
{
    __shared__ T wtot[EXT_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < EXT_WAVES; w++) {
        if (w < wave) before += wtot[w];
        all += wtot[w];
    }
    __syncthreads();  // wtot may be reused by the caller's next round
    *total = all;
    return before + inc - v;
}

// pass 2a: tile_off[e] = sum of tile_cnt[b0 .. e) for e in [b0, b0 + EXT_SCAN) ∩ [0, nt] (tile_cnt[nt] reads as 0);
// blk_sum[block] = the workgroup's total
__global__ __launch_bounds__(BLOCK) void k_extract_scan_tiles(const unsigned* __restrict__ tile_cnt, long long nt,
                                                              unsigned* __restrict__ tile_off,
                                                              unsigned long long* __restrict__ blk_sum)
{
    const long long e0 = (long long)blockIdx.x * EXT_SCAN + (long long)threadIdx.x * EXT_PER;
    unsigned v[EXT_PER], s = 0;
#pragma unroll
    for (int i = 0; i < EXT_PER; i++) {
        v[i] = e0 + i < nt ? tile_cnt[e0 + i] : 0u;
        s += v[i];
    }
    unsigned total;
    unsigned ex = ext_block_scan<unsigned>(s, &total);  // (at most EXT_SCAN * EXT_TILE per workgroup)
#pragma unroll
    for (int i = 0; i < EXT_PER; i++) {
        if (e0 + i <= nt) tile_off[e0 + i] = ex;
        ex += v[i];
    }
    if (threadIdx.x == 0) blk_sum[blockIdx.x] = total;
}

// pass 2b: one workgroup, exclusive scan of the nb workgroup totals into blk_off, EXT_SCAN at a time with a carry
__global__ __launch_bounds__(BLOCK) void k_extract_scan_sums(const unsigned long long* __restrict__ blk_sum, int nb,
                                                             unsigned long long* __restrict__ blk_off)
{
    unsigned long long carry = 0;
    for (int c0 = 0; c0 < nb; c0 += EXT_SCAN) {
        const int e0 = c0 + threadIdx.x * EXT_PER;
        unsigned long long v[EXT_PER], s = 0;
#pragma unroll
        for (int i = 0; i < EXT_PER; i++) {
            v[i] = e0 + i < nb ? blk_sum[e0 + i] : 0ull;
            s += v[i];
        }
        unsigned long long total;
        unsigned long long ex = carry + ext_block_scan<unsigned long long>(s, &total);
#pragma unroll
        for (int i = 0; i < EXT_PER; i++) {
            if (e0 + i < nb) blk_off[e0 + i] = ex;
            ex += v[i];
        }
        carry += total;
    }
}

__device__ __forceinline__ unsigned long long ext_tile_offset(const unsigned* __restrict__ tile_off,
                                                              const unsigned long long* __restrict__ blk_off,
                                                              long long tile)
{
    return blk_off[tile / EXT_SCAN] + tile_off[tile];
}

// offsets[i] = first point of slot i (i < n), offsets[n] = total
__global__ __launch_bounds__(BLOCK) void k_extract_offsets(const ExtractSlot* __restrict__ tab, int n, long long nt,
                                                           const unsigned* __restrict__ tile_off,
                                                           const unsigned long long* __restrict__ blk_off,
                                                           unsigned long long* __restrict__ offsets)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i > n) return;
    offsets[i] = ext_tile_offset(tile_off, blk_off, i < n ? tab[i].tile0 : nt);
}

// pass 3: the same walk as pass 1; every passing item learns its position from the tile's offset, the counts of the
// earlier rounds and of the lower waves of its round (LDS) and the lanes below it in its wave (mbcnt), then writes the
// requested fields
__global__ __launch_bounds__(BLOCK) void k_extract_write(ExtractIn in, const unsigned* __restrict__ tile_off,
                                                         const unsigned long long* __restrict__ blk_off, ExtractOut out)
{
    __shared__ unsigned wcnt[EXT_PER][EXT_WAVES];
    const long long tile = blockIdx.x;
    const ExtractSlot d = in.tab[ext_find_slot(in.tab, in.n, tile)];
    const long long base = (tile - d.tile0) * EXT_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long idx[EXT_PER];
    unsigned code[EXT_PER], below[EXT_PER];
    float rho[EXT_PER], sigma[EXT_PER];
    bool f[EXT_PER];
#pragma unroll
    for (int k = 0; k < EXT_PER; k++) {
        f[k] = ext_item(in, d, base + k * BLOCK + threadIdx.x, idx[k], code[k], rho[k], sigma[k]);
        const unsigned long long m = __ballot(f[k]);
        below[k] = ext_lanes_below(m);
        if (lane == 0) wcnt[k][wave] = (unsigned)__popcll(m);
    }
    __syncthreads();
    unsigned long long pos = ext_tile_offset(tile_off, blk_off, tile);
    const long long plane = (long long)d.slot * in.P;
#pragma unroll
    for (int k = 0; k < EXT_PER; k++) {
        unsigned lower = 0, round = 0;
#pragma unroll
        for (int w = 0; w < EXT_WAVES; w++) {
            const unsigned c = wcnt[k][w];
            if (w < wave) lower += c;
            round += c;
        }
        if (f[k]) {
            const unsigned long long o = pos + lower + below[k];
            if (out.xyz) {
                const float* s = in.xyz + (plane + idx[k]) * 3;
                out.xyz[o * 3 + 0] = s[0];
                out.xyz[o * 3 + 1] = s[1];
                out.xyz[o * 3 + 2] = s[2];
            }
            if (out.pixel) out.pixel[o] = code[k];
            if (out.rho_sigma) out.rho_sigma[o] = make_float2(rho[k], sigma[k]);
            if (out.intensity) out.intensity[o] = (unsigned char)(__float_as_uint(in.rec[plane + idx[k]].w) & 0xffu);
        }
        pos += round;
    }
}

}  // namespace sdm
