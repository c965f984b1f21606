// sdm_vmap_cast.h -- ray queries on the persistent voxel map (sdm_vmap_cast_segments, sdm_vmap_render; included by
// sdm_engine.hip).  Every other sdm_vmap_* call writes the map or lists its entries by id; these two ask it the spatial
// question: along the segment from O to P, which entry comes first?  The walk is k_vmap_carve's with an early exit (the walk
// is restated here and that kernel and k_vmap_recarve are left alone), the probe is its read-only vmap_find.
//
// One call over the rays i = 0 .. n-1:
//   k_vmap_cast<false>  one lane per ray, ray i on lane i: 24 B of (origins[i], ends[i]).
//   k_vmap_cast<true>   one lane per pixel in raster order, ray i = y * W + x on lane i: O is the camera centre the host has
//                       formed, P is pointset_pixel -- the device function of UpdateSemiDensePointSet itself,
//                       sdm_kernels.h -- of (K, Tcw, x, y, rho_far).
//   Both then walk the cells s = 0 .. N - end_margin; a cell of index s >= start_margin is EXAMINED: one probe, and if its
//   key has an entry that passes the filter (multiplicity, published flag) the lane notes (id, s) and leaves the loop.  The
//   lane writes its hit_id, hit_step and -- the render -- hit_rho = 1 / z of the hit entry's stored point in the camera.
//   The wave then reduces its four totals (ballot / popcount for the flags, 6 shuffle steps for the examined cells) and lane 0
//   issues one 64-bit atomic per non-zero total.
//
// Reproducibility: every per-ray output is a function of that ray's walk alone and every total a sum of ones, so neither the
// arrival order of the atomics nor the table's layout can change a bit.  Loops are bounded by max_steps and the table
// capacity; no wave-level operation stands inside the divergent loop; every lane reaches the reduction; no lane waits for
// another; no LDS.  The table, the records and the flags are only read.  Plain C++ and vector stores only.
#pragma once
#include "sdm_vmap_carve.h"

namespace sdm {

constexpr unsigned VMAP_CAST_NO_HIT = 0xffffffffu;   // SDM_VMAP_NO_HIT
constexpr unsigned VMAP_CAST_SKIPPED = 0xfffffffeu;  // SDM_VMAP_RAY_SKIPPED

struct VmapCastIn {
    const float* origins;             // [n][3] (segments)
    const float* ends;                // [n][3] (segments)
    KfMeta pose;                      // (render) fx, fy, cx, cy, Tcw
    float ox, oy, oz;                 // (render) the camera centre, formed on the host
    float rho_far;                    // (render) the inverse depth of the far end of every pixel's ray
    int W;                            // (render) ray i is pixel (i % W, i / W)
    long long n;                      // rays
    const float* xyz;                 // [M][3] the records' xyz (render: hit_rho)
    const unsigned* multiplicity;     // [M]
    const unsigned char* published;   // [M], or null: every flag reads 0
    unsigned M;                       // entries of the map
    float voxel, inv;
    int start_margin, end_margin, max_steps;
    unsigned min_multiplicity;
    int require_published;
};

// rays i0 + thread of the slice; totals = {rays, skipped rays, rays that hit, examined cells}.  Any destination may be null.
template <bool RENDER>
__global__ __launch_bounds__(BLOCK) void k_vmap_cast(VmapCastIn in, long long i0, VmapTable tb, unsigned* __restrict__ hit_id,
                                                     int* __restrict__ hit_step, float* __restrict__ hit_rho,
                                                     unsigned long long* __restrict__ totals)
{
    const long long i = i0 + (long long)blockIdx.x * BLOCK + threadIdx.x;
    const bool ray = i < in.n;
    bool skipped = false, stopped = false;
    unsigned examined = 0, id_out = VMAP_CAST_NO_HIT;
    int step_out = 0;
    if (ray) {
        float ox, oy, oz, px, py, pz;
        if (RENDER) {
            float p[3];
            pointset_pixel(in.pose, (int)(i % in.W), (int)(i / in.W), in.rho_far, p);
            ox = in.ox, oy = in.oy, oz = in.oz;
            px = p[0], py = p[1], pz = p[2];
        } else {
            ox = in.origins[i * 3 + 0], oy = in.origins[i * 3 + 1], oz = in.origins[i * 3 + 2];
            px = in.ends[i * 3 + 0], py = in.ends[i * 3 + 1], pz = in.ends[i * 3 + 2];
        }
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
                // cells s = start_margin .. N - end_margin are examined; the walk stops at the first that stops the ray
                // (N <= max_steps <= 65536 and the margins are >= 0: no overflow; an empty range walks nothing)
                const int last = in.start_margin <= N - in.end_margin ? N - in.end_margin : -1;
                for (int s = 0; s <= last; s++) {    // (at most N + 1 rounds)
                    if (s >= in.start_margin) {
                        examined++;
                        const unsigned id = vmap_find(tb, vmap_cell_key(cx, cy, cz));
                        if (id < in.M && in.multiplicity[id] >= in.min_multiplicity &&
                            (!in.require_published || (in.published && in.published[id] != 0))) {
                            stopped = true;
                            id_out = id;
                            step_out = s;
                            break;
                        }
                    }
                    if (s == last) break;  // (s = N has no step left: every r is 0)
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
        if (skipped) id_out = VMAP_CAST_SKIPPED;
        if (hit_id) hit_id[i] = id_out;
        if (hit_step) hit_step[i] = step_out;
        if (RENDER && hit_rho) {
            float rho = 0.f;
            if (stopped) {
                const float X = in.xyz[(size_t)id_out * 3 + 0], Y = in.xyz[(size_t)id_out * 3 + 1], Z = in.xyz[(size_t)id_out * 3 + 2];
                const float z = ((in.pose.Tcw[8] * X + in.pose.Tcw[9] * Y) + in.pose.Tcw[10] * Z) + in.pose.Tcw[11];
                rho = 1.0f / z;
            }
            hit_rho[i] = rho;
        }
    }
    // the call totals: one atomic per wave and total (every lane of the wave arrives here)
    const unsigned long long rm = __ballot(ray), sk = __ballot(skipped), hm = __ballot(stopped);
    unsigned sum = examined;  // (at most 64 x 65537)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if ((threadIdx.x & 63) == 0) {
        if (rm) atomicAdd(&totals[0], (unsigned long long)__popcll(rm));
        if (sk) atomicAdd(&totals[1], (unsigned long long)__popcll(sk));
        if (hm) atomicAdd(&totals[2], (unsigned long long)__popcll(hm));
        if (sum) atomicAdd(&totals[3], (unsigned long long)sum);
    }
}

}  // namespace sdm
