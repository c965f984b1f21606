// sdm_support.h -- per-point visibility of the extracted cloud (sdm_extract_points_support, included by sdm_engine.hip).
//
// InterKeyFrameDepthChecking tests every pixel against every neighbour (PM.cc:677-755) and keeps only the count
// (`nj >= 1` summed over the neighbours, PM.cc:755, compared with lambdaN at PM.cc:764).  The set behind the count -- the
// neighbour keyframes whose own depth map agrees with the point -- is the point's visibility list, the
// `KF_ind1, ..., KF_indN` of the transcript grammar.  k_point_support evaluates it for the points sdm_extract_points
// compacted: bit j of a point's 64-bit word is set iff neighbour j of its keyframe's row is counted.
//
//   * the statement is K4's: inter_neighbour_fast, and inter_neighbour_exact for the lanes whose guard is raised
//     (sdm_kernels.h); each neighbour is evaluated from a zero K4Sums, so the bit is its kf_count and the Gauss-Newton
//     sums -- which the word does not need -- are dead in the inlined fast form;
//   * rho is the depth map's (the plane sdm_inter_check reads), whatever plane the extraction filtered on; a pixel outside
//     the 2-px inset (PM.cc:659-660) or skipped by PM.cc:662 gets 0; lambdaN plays no part;
//   * one lane per point.  The workgroups are cut per slot on the host from the offsets it has waited for (block0), so
//     every lane of a workgroup shares the reference's RefConst and its PairConst row: those loads are wave-uniform.  The
//     points of a slot are a raster-ordered subset of its pixels, so neighbouring lanes project to neighbouring taps, as
//     in K4's list form;
//   * no atomics: one 8-byte store per lane, consecutive lanes to consecutive words.
#pragma once
#include "sdm_extract.h"
#include "sdm_kernels.h"

namespace sdm {

constexpr int SUP_BLOCK = 256;
static_assert(SDM_MAX_NEIGHBOURS <= 64, "one bit of the support word per neighbour");

// block0[i] = first workgroup of slot i's points (i < n), block0[n] = all workgroups; a slot without points shares its
// block0 with the next one
__device__ __forceinline__ int sup_find_slot(const long long* __restrict__ block0, int n, long long block)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (block0[mid] <= block) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// offsets: sdm_extract_points' (first point of slot i, offsets[n] = total); pixel: the compacted (y << 16) | x codes;
// refs[i] / pairs[i * n_nbr ..] belong to slot i of the call; block_base: first workgroup of this launch
__global__ __launch_bounds__(SUP_BLOCK) void k_point_support(const float2* __restrict__ pool, long long plane,
                                                             const RefConst* __restrict__ refs,
                                                             const PairConst* __restrict__ pairs, int n, int n_nbr, int W,
                                                             int H, const long long* __restrict__ block0,
                                                             long long block_base,
                                                             const unsigned long long* __restrict__ offsets,
                                                             const unsigned* __restrict__ pixel,
                                                             unsigned long long* __restrict__ support)
{
    const long long block = block_base + blockIdx.x;
    const int i = sup_find_slot(block0, n, block);
    const unsigned long long p = offsets[i] + (unsigned long long)(block - block0[i]) * SUP_BLOCK + threadIdx.x;
    if (p >= offsets[i + 1]) return;
    const RefConst rc = refs[i];
    const PairConst* __restrict__ pcs = pairs + (long long)i * n_nbr;
    const unsigned code = pixel[p];
    const int x = (int)(code & 0xffffu), y = (int)(code >> 16);
    unsigned long long word = 0ull;
    if (x >= 2 && x < W - 2 && y >= 2 && y < H - 2) {  // PM.cc:659-660
        const float depthp = pool[(long long)rc.slot * plane + y * W + x].x;
        if (!(lt_1em6(depthp))) {  // PM.cc:662
            const float colsm1 = (float)(W - 1), rowsm1 = (float)(H - 1);
            const float xp0 = ((float)x - rc.cx) / rc.fx, xp1 = ((float)y - rc.cy) / rc.fy;  // PM.cc:677
            const float dp = rcp_exact(depthp);                                                 // PM.cc:769
            const K4Guard g0 = {absbits(depthp), absbits(depthp)};
            const K4Sums zero = {0, 0.f, 0.f};
            for (int j = 0; j < n_nbr; j++) {
                const PairConst* __restrict__ pc = pcs + j;
                const float2* __restrict__ nb = pool + (long long)pc->nbr_slot * plane;
                bool slow;
                K4Sums r = inter_neighbour_fast(nb, pc, W, colsm1, rowsm1, xp0, xp1, depthp, dp, g0, zero, &slow);
                if (__builtin_expect(slow, 0)) r = inter_neighbour_exact(nb, pc, W, colsm1, rowsm1, xp0, xp1, depthp, dp, zero);
                word |= (unsigned long long)(r.kf_count != 0) << j;  // PM.cc:755
            }
        }
    }
    support[p] = word;
}

}  // namespace sdm
