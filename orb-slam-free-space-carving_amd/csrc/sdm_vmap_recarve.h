// sdm_vmap_recarve.h -- rebuilding the persistent voxel map's free-space evidence from its observation log
// (sdm_vmap_recarve; included by sdm_engine.hip).  sdm_vmap_carve reads the resident slots of a block, so after
// sdm_vmap_repose or sdm_vmap_retire the evidence of everything older could not be made again.  The map holds what that
// takes: the log's (entry, tag) pairs are the rays, the entry's record holds the ray's end point, and the caller holds the
// poses.
//
// One sdm_vmap_recarve over the pairs k = first .. first + count - 1 of the log (the host has formed the camera centre of
// every pose, sorted the table by tag -- which finds a tag listed twice -- and uploaded it once, 20 B per pose; with reset
// it has zeroed both counters of every entry):
//   k_vmap_recarve  one lane per pair, in log order (point-major: a wave mixes cameras).  A binary search of the pair's tag
//                   in the table; a miss counts the pair as unposed and does nothing else.  A hit reads the 12 B of
//                   xyz in the record of the pair's entry and walks the ray from the centre to it exactly as k_vmap_carve
//                   does (sdm_vmap_carve.h; the walk is restated here and that kernel is left alone): a read-only probe
//                   per counted cell, a 64-bit atomic add on a hit, one probe for the end cell.  The wave then reduces its six totals (ballot / popcount for
//                   the flags, 6 shuffle steps for the sums) and lane 0 issues one 64-bit atomic per non-zero total.
//
// Reproducibility: every counter and total is a sum of ones, so neither the arrival order of the atomics nor the table's
// layout can change a bit.  Loops are bounded by max_steps, the table capacity and log2 of the pose table; every lane
// reaches the reduction; no lane waits for another; no LDS.  The table, the records and the log are only read.  Plain C++
// and vector stores only.
#pragma once
#include "sdm_vmap_obs.h"

namespace sdm {

struct VmapRecarveIn {
    const unsigned* obs_entry;  // [E] the log
    const int* obs_tag;         // [E]
    const float* xyz;           // [M][3] the records' xyz
    const int* tags;            // [n] the pose table's tags, ascending
    const float* origin;        // [n][4] their camera centres (the fourth value pads)
    long long first, count;     // the range of the log
    int n;
    unsigned M;                 // entries of the map
    float voxel, inv;
    int end_margin, max_steps;
};

// pairs first + e0 + thread of the slice; totals = {pairs, unposed pairs, skipped rays, counted cells, counted cells with an
// entry, walked rays whose end cell has an entry}
__global__ __launch_bounds__(BLOCK) void k_vmap_recarve(VmapRecarveIn in, long long e0, VmapTable tb,
                                                        unsigned long long* __restrict__ crossings,
                                                        unsigned long long* __restrict__ ends,
                                                        unsigned long long* __restrict__ totals)
{
    const long long e = e0 + (long long)blockIdx.x * BLOCK + threadIdx.x;
    const bool pair = e < in.count;
    bool unposed = false, skipped = false, end_hit = false;
    unsigned counted = 0, hit = 0;
    if (pair) {
        const long long k = in.first + e;
        const unsigned ent = in.obs_entry[k];
        const int t = in.obs_tag[k];
        int lo = 0, hi = in.n;  // the first table position whose tag is not below t
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (in.tags[mid] < t) lo = mid + 1;
            else hi = mid;
        }
        unposed = !(lo < in.n && in.tags[lo] == t && ent < in.M);  // (the log holds entries of the map only)
        if (!unposed) {
            const float px = in.xyz[(size_t)ent * 3 + 0], py = in.xyz[(size_t)ent * 3 + 1], pz = in.xyz[(size_t)ent * 3 + 2];
            const float ox = in.origin[lo * 4 + 0], oy = in.origin[lo * 4 + 1], oz = in.origin[lo * 4 + 2];
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
    const unsigned long long pr = __ballot(pair), up = __ballot(unposed), sk = __ballot(skipped), eh = __ballot(end_hit);
    unsigned sum = counted, hits = hit;  // (each at most 64 x 65536)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o, 64);
        hits += __shfl_xor(hits, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (pr) atomicAdd(&totals[0], (unsigned long long)__popcll(pr));
        if (up) atomicAdd(&totals[1], (unsigned long long)__popcll(up));
        if (sk) atomicAdd(&totals[2], (unsigned long long)__popcll(sk));
        if (sum) atomicAdd(&totals[3], (unsigned long long)sum);
        if (hits) atomicAdd(&totals[4], (unsigned long long)hits);
        if (eh) atomicAdd(&totals[5], (unsigned long long)__popcll(eh));
    }
}

}  // namespace sdm
