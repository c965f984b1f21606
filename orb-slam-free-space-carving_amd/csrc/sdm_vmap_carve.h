// sdm_vmap_carve.h -- free-space evidence on the persistent voxel map (sdm_vmap_carve / sdm_vmap_fetch_evidence, included
// by sdm_engine.hip): the (camera, plain point) rays of a call are walked through the map's table, read-only, and counted
// into two 64-bit counters per entry that live beside the records (an allocation of their own, made at the first carve and
// grown with the records).
//
// The plain extraction and -- with neighbours -- k_point_support first run into engine-owned staging: T points
// g = 0 .. T-1 with their support words.  The host adds, per slot i of the call, the list of its DISTINCT neighbour slots
// other than slots[i], each with the mask of the table columns that name it (D = the longest list), and the camera centres
// of the call's distinct slots.  Then:
//   k_vmap_carve     one lane per candidate ray (g, d), d = 0 .. D, in camera-major order: index = d * T + g, so a wave
//                    holds 64 consecutive pixels of one keyframe seen from one position of the camera list.  d = 0 is the
//                    point's own camera; d >= 1 is live iff support[g] shares a bit with the mask of distinct neighbour
//                    d - 1 of the point's slot (found by k_vmap_commit's binary search in the plain offsets).  A live lane
//                    forms the cells of the centre and of the point and walks the voxels between them exactly as
//                    k_voxel_carve does (sdm_carve.h: the step COUNT per axis is fixed by the integer cells, the floats
//                    only order the steps).  Every counted cell probes the map's table read-only -- vox_mix, linear
//                    probing, ending at the equal key or at VOX_EMPTY, bounded by the capacity -- and on a hit adds 1 to
//                    crossings[id]; after the walk the end cell is probed once for ends[id].  The wave then reduces its
//                    five totals (ballot / popcount for the flags, 6 shuffle steps for the sums) and lane 0 issues one
//                    64-bit atomic per non-zero total.
//   k_vmap_evidence  sdm_vmap_fetch_evidence by ids: the counters of entries ids[0 .. count) into dense arrays
//
// Reproducibility: every counter and total is a sum of ones, so neither the arrival order of the atomics nor the table's
// layout (which differs from run to run, sdm_vmap.h) can change a bit.  Loops are bounded by max_steps, the table capacity
// and 31 halving steps; no lane waits for another; no LDS.  The map's table and records are only read.
#pragma once
#include "sdm_vmap.h"

namespace sdm {

struct VmapCarveIn {
    const float* xyz;                         // [T][3] the staged plain points
    const unsigned long long* support;        // [T] the support words, or null (D == 0)
    const unsigned long long* plain_offsets;  // [n + 1]
    const int* own_cam;                       // [n] camera index of slots[i]
    const int* nbr_cam;                       // [n][D] camera index of distinct neighbour d of slot i (padding: 0)
    const unsigned long long* nbr_mask;       // [n][D] the columns that name it (padding: 0, never live)
    const float* origin;                      // [Cn][4] camera centres (the fourth value pads)
    long long T;
    int n, D;
    unsigned M;                               // entries of the map
    float voxel, inv;
    int end_margin, max_steps;
};

// the entry of `key`, or VMAP_NOID
__device__ __forceinline__ unsigned vmap_find(const VmapTable& tb, unsigned long long key)
{
    unsigned long long h = vox_mix(key) & tb.mask;
    for (unsigned long long probe = 0; probe <= tb.mask; probe++) {  // bounded by the capacity
        const unsigned long long k = tb.keys[h];
        if (k == key) return tb.id[h];
        if (k == VOX_EMPTY) break;
        h = (h + 1) & tb.mask;
    }
    return VMAP_NOID;
}

__device__ __forceinline__ bool vmap_cell_ok(float c) { return c >= -VOX_CELL_LIM && c < VOX_CELL_LIM; }  // (false for a NaN)

__device__ __forceinline__ unsigned long long vmap_cell_key(int cx, int cy, int cz)
{
    return ((unsigned long long)(cx + (1 << 20)) << 42) | ((unsigned long long)(cy + (1 << 20)) << 21) |
           (unsigned long long)(cz + (1 << 20));
}

// candidates e0 + thread of the slice; totals = {rays, skipped rays, counted cells, counted cells with an entry, walked
// rays whose end cell has an entry}
__global__ __launch_bounds__(BLOCK) void k_vmap_carve(VmapCarveIn in, long long e0, long long E, VmapTable tb,
                                                      unsigned long long* __restrict__ crossings,
                                                      unsigned long long* __restrict__ ends,
                                                      unsigned long long* __restrict__ totals)
{
    const long long e = e0 + (long long)blockIdx.x * BLOCK + threadIdx.x;
    bool live = false, skipped = false, end_hit = false;
    unsigned counted = 0, hit = 0;
    if (e < E) {
        const long long d = e / in.T, g = e - d * in.T;
        const int i = vmap_slot_of(in.plain_offsets, in.n, (unsigned long long)g);
        int cam = in.own_cam[i];
        live = d == 0;
        if (!live) {
            const size_t at = (size_t)i * (size_t)in.D + (size_t)(d - 1);
            live = (in.support[g] & in.nbr_mask[at]) != 0ull;
            cam = in.nbr_cam[at];
        }
        if (live) {
            const float px = in.xyz[g * 3 + 0], py = in.xyz[g * 3 + 1], pz = in.xyz[g * 3 + 2];
            const float ox = in.origin[cam * 4 + 0], oy = in.origin[cam * 4 + 1], oz = in.origin[cam * 4 + 2];
            const float fox = floorf(ox * in.inv), foy = floorf(oy * in.inv), foz = floorf(oz * in.inv);
            const float fpx = floorf(px * in.inv), fpy = floorf(py * in.inv), fpz = floorf(pz * in.inv);
            skipped = !(vmap_cell_ok(fox) && vmap_cell_ok(foy) && vmap_cell_ok(foz) && vmap_cell_ok(fpx) && vmap_cell_ok(fpy) &&
                        vmap_cell_ok(fpz));
            if (!skipped) {
                int cx = (int)fox, cy = (int)foy, cz = (int)foz;
                const int ex = (int)fpx, ey = (int)fpy, ez = (int)fpz;
                const int dx = ex - cx, dy = ey - cy, dz = ez - cz;  // (each below 2^21 in magnitude)
                int rx = dx < 0 ? -dx : dx, ry = dy < 0 ? -dy : dy, rz = dz < 0 ? -dz : dz;
                const int N = rx + ry + rz;
                skipped = N > in.max_steps;
                if (!skipped) {
                    const int sx = dx > 0 ? 1 : -1, sy = dy > 0 ? 1 : -1, sz = dz > 0 ? 1 : -1;  // (read only where r > 0)
                    float tmx = 0.f, tmy = 0.f, tmz = 0.f, tdx = 0.f, tdy = 0.f, tdz = 0.f;
                    if (rx > 0) {
                        const float dd = px - ox;
                        tmx = ((float)(cx + (sx > 0 ? 1 : 0)) * in.voxel - ox) / dd;
                        tdx = in.voxel / fabsf(dd);
                    }
                    if (ry > 0) {
                        const float dd = py - oy;
                        tmy = ((float)(cy + (sy > 0 ? 1 : 0)) * in.voxel - oy) / dd;
                        tdy = in.voxel / fabsf(dd);
                    }
                    if (rz > 0) {
                        const float dd = pz - oz;
                        tmz = ((float)(cz + (sz > 0 ? 1 : 0)) * in.voxel - oz) / dd;
                        tdz = in.voxel / fabsf(dd);
                    }
                    // cells s = 0 .. N - 1 - end_margin are counted; the steps after them change nothing that is returned
                    counted = N > in.end_margin ? (unsigned)(N - in.end_margin) : 0u;
                    for (unsigned s = 0; s < counted; s++) {  // (counted <= N <= max_steps)
                        const unsigned id = vmap_find(tb, vmap_cell_key(cx, cy, cz));
                        if (id < in.M) {
                            atomicAdd(&crossings[id], 1ull);
                            hit++;
                        }
                        // the axis with steps left and the smallest tMax; x, y, z in turn, replaced only by a strictly smaller one
                        int a = -1;
                        float best = 0.f;
                        if (rx > 0) a = 0, best = tmx;
                        if (ry > 0 && (a < 0 || tmy < best)) a = 1, best = tmy;
                        if (rz > 0 && (a < 0 || tmz < best)) a = 2;
                        if (a == 0) cx += sx, rx -= 1, tmx = tmx + tdx;
                        else if (a == 1) cy += sy, ry -= 1, tmy = tmy + tdy;
                        else cz += sz, rz -= 1, tmz = tmz + tdz;
                    }
                    const unsigned id = vmap_find(tb, vmap_cell_key(ex, ey, ez));  // the end cell, whatever end_margin
                    if (id < in.M) {
                        atomicAdd(&ends[id], 1ull);
                        end_hit = true;
                    }
                }
            }
        }
    }
    // the call totals: one atomic per wave and total (every lane of the wave arrives here)
    const unsigned long long lv = __ballot(live), sk = __ballot(skipped), eh = __ballot(end_hit);
    unsigned sum = counted, hits = hit;  // (each at most 64 x 65536)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o, 64);
        hits += __shfl_xor(hits, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (lv) atomicAdd(&totals[0], (unsigned long long)__popcll(lv));
        if (sk) atomicAdd(&totals[1], (unsigned long long)__popcll(sk));
        if (sum) atomicAdd(&totals[2], (unsigned long long)sum);
        if (hits) atomicAdd(&totals[3], (unsigned long long)hits);
        if (eh) atomicAdd(&totals[4], (unsigned long long)__popcll(eh));
    }
}

// fetch by ids: the counters of entry ids[j] -> position j0 + thread of the dense destinations (either may be null; a null
// source reads as 0: no carve has run); *bad |= 1 for an id >= M
__global__ __launch_bounds__(BLOCK) void k_vmap_evidence(const unsigned long long* __restrict__ crossings,
                                                         const unsigned long long* __restrict__ ends,
                                                         const unsigned* __restrict__ ids, long long count, long long j0,
                                                         unsigned M, unsigned long long* __restrict__ dst_crossings,
                                                         unsigned long long* __restrict__ dst_ends, unsigned* __restrict__ bad)
{
    const long long j = j0 + (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= count) return;
    const unsigned e = ids[j];
    if (e >= M) {
        atomicOr(bad, 1u);
        return;
    }
    if (dst_crossings) dst_crossings[j] = crossings ? crossings[e] : 0ull;
    if (dst_ends) dst_ends[j] = ends ? ends[e] : 0ull;
}

}  // namespace sdm
