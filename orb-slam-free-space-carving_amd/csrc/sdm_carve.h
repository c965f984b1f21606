// sdm_carve.h -- free-space evidence for the merged cloud (sdm_extract_points_voxel_freespace, included by sdm_engine.hip).
//
// sdm_extract_points_voxel_cameras' passes leave, resident: the kept points' xyz, the camera lists (cam_offsets /
// cam_slots: one (camera, kept point) ray per entry) and the voxel table whose claimed positions carry the kept rank of
// the voxel's winner (k_voxel_write).  The host adds the camera centres of the call's distinct slots.  Then:
//   k_voxel_carve    one lane per ray e.  The lane finds its kept point (upper bound of e in cam_offsets, at most 33 halving
//                    steps) and its camera (lower bound of the slot id in slot_of_cam, at most 32), forms the cells of the
//                    centre and of the point as k_voxel_insert forms a point's, and walks the voxels between them
//                    (Amanatides & Woo; the step COUNT per axis is fixed by the integer cells, the floats only order the
//                    steps).  Every counted cell probes the table read-only -- the same vox_mix, linear probing, ending
//                    at the equal key or at VOX_EMPTY, bounded by the capacity -- and on a hit adds 1 to the counter of
//                    the kept point that owns the voxel.  The wave then sums its skipped rays (ballot / popcount) and its
//                    counted cells (6 shuffle steps) and lane 0 issues one 64-bit atomic per total.
//
// Reproducibility: crossings[k] is a sum of ones and the two totals are integer sums, so neither the arrival order of the
// atomics nor the table's layout (which differs from run to run, sdm_voxel.h) can change a bit.  Loops are bounded by
// max_steps, the table capacity, 33 and 32; no lane waits for another; no LDS.
#pragma once
#include "sdm_voxel.h"

namespace sdm {

struct CarveIn {
    const float* xyz;              // [M][3] the kept points
    const long long* cam_offsets;  // [M + 1]
    const int* cam_slots;          // [E]
    const int* slot_of_cam;        // [Cn] ascending slot ids (VoxCamTable's)
    const float* origin;           // [Cn][4] camera centre of slot_of_cam[c] (the fourth value pads)
    long long M, E;
    int Cn;
    float voxel, inv;
    int end_margin, max_steps;
};

__device__ __forceinline__ bool carve_cell_ok(float c) { return c >= -VOX_CELL_LIM && c < VOX_CELL_LIM; }  // (false for a NaN)

// rays e0 + thread of the slice; totals[0] += skipped rays, totals[1] += counted cells
__global__ __launch_bounds__(BLOCK) void k_voxel_carve(CarveIn in, long long e0, VoxTable tb, unsigned* __restrict__ crossings,
                                                       unsigned long long* __restrict__ totals)
{
    const long long e = e0 + (long long)blockIdx.x * BLOCK + threadIdx.x;
    bool skipped = false;
    unsigned counted = 0;
    if (e < in.E) {
        long long lo = 0, hi = in.M;  // the kept point: the last k with cam_offsets[k] <= e
        for (int it = 0; it < 33 && hi - lo > 1; it++) {
            const long long mid = lo + ((hi - lo) >> 1);
            if (in.cam_offsets[mid] <= e) lo = mid;
            else hi = mid;
        }
        const int slot = in.cam_slots[e];
        int ca = 0, cb = in.Cn - 1;  // the camera: slot_of_cam[ca] == slot (every listed slot is in the table)
        for (int it = 0; it < 32 && ca < cb; it++) {
            const int mid = ca + ((cb - ca) >> 1);
            if (in.slot_of_cam[mid] < slot) ca = mid + 1;
            else cb = mid;
        }
        const float px = in.xyz[lo * 3 + 0], py = in.xyz[lo * 3 + 1], pz = in.xyz[lo * 3 + 2];
        const float ox = in.origin[ca * 4 + 0], oy = in.origin[ca * 4 + 1], oz = in.origin[ca * 4 + 2];
        const float fox = floorf(ox * in.inv), foy = floorf(oy * in.inv), foz = floorf(oz * in.inv);
        const float fpx = floorf(px * in.inv), fpy = floorf(py * in.inv), fpz = floorf(pz * in.inv);
        skipped = !(carve_cell_ok(fox) && carve_cell_ok(foy) && carve_cell_ok(foz) && carve_cell_ok(fpx) && carve_cell_ok(fpy) &&
                    carve_cell_ok(fpz));
        if (!skipped) {
            int cx = (int)fox, cy = (int)foy, cz = (int)foz;
            const int dx = (int)fpx - cx, dy = (int)fpy - cy, dz = (int)fpz - cz;  // (each below 2^21 in magnitude)
            int rx = dx < 0 ? -dx : dx, ry = dy < 0 ? -dy : dy, rz = dz < 0 ? -dz : dz;
            const int N = rx + ry + rz;
            skipped = N > in.max_steps;
            if (!skipped) {
                const int sx = dx > 0 ? 1 : -1, sy = dy > 0 ? 1 : -1, sz = dz > 0 ? 1 : -1;  // (read only where r > 0)
                float tmx = 0.f, tmy = 0.f, tmz = 0.f, tdx = 0.f, tdy = 0.f, tdz = 0.f;
                if (rx > 0) {
                    const float d = px - ox;
                    tmx = ((float)(cx + (sx > 0 ? 1 : 0)) * in.voxel - ox) / d;
                    tdx = in.voxel / fabsf(d);
                }
                if (ry > 0) {
                    const float d = py - oy;
                    tmy = ((float)(cy + (sy > 0 ? 1 : 0)) * in.voxel - oy) / d;
                    tdy = in.voxel / fabsf(d);
                }
                if (rz > 0) {
                    const float d = pz - oz;
                    tmz = ((float)(cz + (sz > 0 ? 1 : 0)) * in.voxel - oz) / d;
                    tdz = in.voxel / fabsf(d);
                }
                // cells s = 0 .. N - 1 - end_margin are counted; the steps after them change nothing that is returned
                counted = N > in.end_margin ? (unsigned)(N - in.end_margin) : 0u;
                for (unsigned s = 0; s < counted; s++) {  // (counted <= N <= max_steps)
                    const unsigned long long key = ((unsigned long long)(cx + (1 << 20)) << 42) |
                                                   ((unsigned long long)(cy + (1 << 20)) << 21) |
                                                   (unsigned long long)(cz + (1 << 20));
                    unsigned long long h = vox_mix(key) & tb.mask;
                    for (unsigned long long probe = 0; probe <= tb.mask; probe++) {  // bounded by the capacity
                        const unsigned long long k = tb.keys[h];
                        if (k == key) {
                            const unsigned j = tb.rank[h];
                            if ((long long)j < in.M) atomicAdd(&crossings[j], 1u);
                            break;
                        }
                        if (k == VOX_EMPTY) break;
                        h = (h + 1) & tb.mask;
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
            }
        }
    }
    // the call totals: one atomic per wave and total (every lane of the wave arrives here)
    const unsigned long long sk = __ballot(skipped);
    unsigned sum = counted;  // (at most 64 x 65536)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if ((threadIdx.x & 63) == 0) {
        if (sk) atomicAdd(&totals[0], (unsigned long long)__popcll(sk));
        if (sum) atomicAdd(&totals[1], (unsigned long long)sum);
    }
}

}  // namespace sdm
