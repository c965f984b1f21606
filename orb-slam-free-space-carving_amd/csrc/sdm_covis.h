// sdm_covis.h -- covisible neighbours from resident ORB observations (sdm_covisibility, sdm_covisible_neighbours,
// sdm_recon_covisible; included by sdm_engine.hip).
//
// A covisibility weight is the number of map points two keyframes share (KeyFrame::UpdateConnections, KeyFrame.cc:302-320).
// Every slot keeps its keyframe's map-point ids >= 0, sorted and unique (ObsStore::cov_ids, written by k_obs_ingest before
// it drops the entries without an angle: the angle is GetRotInPlane's filter, not UpdateConnections').
//   k_covis_weights  grid (n_ref, ceil(n_cand / per_block)): the workgroup copies the reference's ids into LDS once; each
//                    wave takes one candidate at a time, reads its ids 64 per step and binary-searches them in the LDS
//                    copy; ballot + popcount accumulate the count in a wave-uniform register; lane 0 stores one int.
//                    Where the reference's list is much the shorter one, its entries are searched in the candidate's
//                    list instead (ids are unique per keyframe, so both directions count the same intersection).
//   k_covis_select   one workgroup per reference: one 64-bit key per candidate, weight << 32 | ~position, so that a
//                    larger key is (weight descending, position ascending) and no two keys are equal; round i takes
//                    the largest key below round i - 1's winner (wave max through __shfl_xor, then LDS across the
//                    waves).  Round 0's winner carries the largest weight: 0 ends the list (KeyFrame.cc:323), below
//                    min_weight it is the whole list (KeyFrame.cc:348-352), else the rounds stop at min_weight.
// Integer compares and counts only, no atomics: the outputs do not depend on timing.
#pragma once
#include "sdm_priors.h"

namespace sdm {

constexpr int COVIS_SWAP_RATIO = 8;  // search the reference's entries in the candidate's list when it is this much longer

struct CovisArgs {
    ObsStore st;
    const int* refs;    // [n_ref] slots
    const int* cands;   // [n_cand] slots
    int* weights;       // [n_ref][n_cand]
    int* nbr_slots;     // [n_ref][n]  (k_covis_select)
    int* nbr_weights;   // [n_ref][n]
    int* counts;        // [n_ref]
    int n_ref, n_cand;
    int per_block;      // candidates per workgroup of k_covis_weights
    int n, min_weight;
};

// entries of a[0, na) found in the sorted b[0, nb), counted by one wave; the result is wave-uniform
template <typename PA, typename PB>
__device__ __forceinline__ int wave_count_found(PA a, int na, PB b, int nb, int lane)
{
    int got = 0;
    for (int i0 = 0; i0 < na; i0 += 64) {
        const int i = i0 + lane;
        bool hit = false;
        if (i < na) {
            const int x = a[i];
            int lo = 0, hi = nb;  // lower_bound of x in b[0, nb)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (b[mid] < x) lo = mid + 1;
                else hi = mid;
            }
            hit = lo < nb && b[lo] == x;
        }
        got += __popcll(__builtin_amdgcn_ballot_w64(hit));
    }
    return got;
}

// grid: (n_ref, ceil(n_cand / per_block)); dynamic LDS: 4 * (the largest reference list) bytes
__global__ void __launch_bounds__(OBS_BLOCK) k_covis_weights(CovisArgs a)
{
    extern __shared__ int cov_ref[];
    const int r = (int)blockIdx.x;
    const int w = threadIdx.x >> 6, lane = lane_id();
    const int s1 = a.refs[r];
    const int m1 = a.st.cov_cnt[s1];
    const int* id1 = a.st.cov_ids + (long long)s1 * a.st.cap;
    for (int i = (int)threadIdx.x; i < m1; i += OBS_BLOCK) cov_ref[i] = id1[i];
    __syncthreads();
    const int c0 = (int)blockIdx.y * a.per_block, c1 = min(c0 + a.per_block, a.n_cand);
    for (int c = c0 + w; c < c1; c += OBS_WAVES) {
        const int s2 = a.cands[c];
        int got = 0;
        if (s2 != s1) {  // KeyFrame.cc:316: a keyframe is not its own neighbour
            const int m2 = a.st.cov_cnt[s2];
            const int* id2 = a.st.cov_ids + (long long)s2 * a.st.cap;
            if ((long long)m1 * COVIS_SWAP_RATIO < m2) got = wave_count_found(cov_ref, m1, id2, m2, lane);
            else got = wave_count_found(id2, m2, cov_ref, m1, lane);
        }
        if (lane == 0) a.weights[(long long)r * a.n_cand + c] = got;
    }
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long k)
{
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned hi = (unsigned)__shfl_xor((int)(k >> 32), o);
        const unsigned lo = (unsigned)__shfl_xor((int)k, o);
        const unsigned long long t = ((unsigned long long)hi << 32) | lo;
        k = t > k ? t : k;
    }
    return k;
}

// larger = (weight descending, position ascending); unique per position
__device__ __forceinline__ unsigned long long covis_key(int weight, int pos)
{
    return ((unsigned long long)(unsigned)weight << 32) | (unsigned)(~(unsigned)pos);
}

// grid: n_ref workgroups
__global__ void __launch_bounds__(OBS_BLOCK) k_covis_select(CovisArgs a)
{
    __shared__ unsigned long long wmax[2][OBS_WAVES];
    const int r = (int)blockIdx.x;
    const int w = threadIdx.x >> 6, lane = lane_id();
    const int* wt = a.weights + (long long)r * a.n_cand;
    int* out_s = a.nbr_slots + (long long)r * a.n;
    int* out_w = a.nbr_weights + (long long)r * a.n;
    for (int i = (int)threadIdx.x; i < a.n; i += OBS_BLOCK) {
        out_s[i] = -1;
        out_w[i] = 0;
    }
    __syncthreads();  // (thread 0 overwrites the chosen entries below)
    unsigned long long below = ~0ull;  // the previous round's winner: every key is smaller than the first one
    int floor_w = 1;                   // round 0 looks at every weight >= 1, then the threshold applies
    int count = 0;
    for (int round = 0; round < a.n; round++) {
        unsigned long long best = 0;
        for (int c = (int)threadIdx.x; c < a.n_cand; c += OBS_BLOCK) {
            const int wc = wt[c];
            const unsigned long long key = covis_key(wc, c);
            if (wc >= floor_w && key < below && key > best) best = key;
        }
        best = wave_max_u64(best);
        if (lane == 0) wmax[round & 1][w] = best;
        __syncthreads();
        for (int i = 0; i < OBS_WAVES; i++) {
            const unsigned long long t = wmax[round & 1][i];
            best = t > best ? t : best;
        }
        if (best == 0) break;  // (a kept key has weight >= 1, so it is never 0) workgroup-uniform
        const int bw = (int)(best >> 32), pos = (int)~(unsigned)best;
        if (threadIdx.x == 0) {
            out_s[round] = a.cands[pos];
            out_w[round] = bw;
        }
        count = round + 1;
        if (round == 0 && bw < a.min_weight) break;  // KeyFrame.cc:348-352: the best candidate alone
        floor_w = a.min_weight;
        below = best;
    }
    if (threadIdx.x == 0) a.counts[r] = count;
}

}  // namespace sdm
