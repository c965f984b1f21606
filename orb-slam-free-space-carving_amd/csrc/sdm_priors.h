// sdm_priors.h -- SemiDenseRecon's search priors from resident ORB observations (sdm_upload_observations*,
// sdm_search_priors; included by sdm_engine.hip).
//
// A slot's observations are its keyframe's map-point id and keypoint angle per keypoint, and GetAllPointDepths().  At
// upload only the entries that can ever contribute to GetRotInPlane are kept -- id >= 0 && angle >= 0, the host helper's
// filter (PM.cc:467-484) -- sorted by id (beside them the sorted id >= 0 list whatever the angle, for sdm_covis.h):
//   k_obs_ingest   one workgroup per keyframe: compact the id >= 0 entries into LDS, bitonic sort by id, flag a repeated
//                  id and a non-finite angle, then compact the angle >= 0 entries to the slot's arrays; copy the depths
// The priors of a call:
//   k_priors       blocks [0, n_ref) when the bounds are asked for: one wave per reference restates
//                  sdm_stereo_search_constraints step by step (sequential double sums: the same order, the same bits);
//                  the next n_ref * n blocks: one workgroup per (reference, neighbour) pair joins the reference's sorted
//                  list against the neighbour's by a per-lane binary search, forms angle2 - angle1 in float, compacts
//                  the matches into LDS (ballot + mbcnt, one region per wave) and selects the element of rank
//                  (m - 1) / 2 -- what rot[(rot.size() - 1) / 2] after std::sort returns -- by a radix select over
//                  order-preserving 32-bit keys (4 passes of 8-bit LDS histograms; integer counts, so deterministic).
//                  No match gives 0 (PM.cc:174-177).
#pragma once
#include "sdm_ingest.h"

namespace sdm {

constexpr int OBS_BLOCK = 256;
constexpr int OBS_WAVES = OBS_BLOCK / 64;
constexpr unsigned OBS_PAD = 0xffffffffu;  // sorts after every id >= 0

enum : int { OBS_BAD_DUPLICATE = 1, OBS_BAD_ANGLE = 2 };

struct ObsItem {       // one keyframe of an upload batch
    int slot;
    int n_kp;
    int n_depths;
    int sort_n;        // power of two >= n_kp (LDS entries of the sort)
    long long off;     // into the packed block (4-byte units): ids[n_kp] angles[n_kp] depths[n_depths]
};

struct ObsStore {      // resident observations, OBS stride per slot
    int* ids;          // [max_keyframes][cap] sorted, id >= 0 && angle >= 0 entries only
    float* ang;
    float* depth;      // [max_keyframes][cap] GetAllPointDepths() as given
    int* cnt;          // [max_keyframes] kept entries
    int* nd;           // [max_keyframes] depths
    int cap;
    int* cov_ids;      // [max_keyframes][cap] sorted, every id >= 0 whatever its angle (sdm_covis.h)
    int* cov_cnt;      // [max_keyframes]
};

// order-preserving map of a float to a 32-bit unsigned key (-0 sorts just below +0) and back
__device__ __forceinline__ unsigned f2key(float x)
{
    const unsigned b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key2f(unsigned k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__device__ __forceinline__ int lane_id() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// position of this thread's kept item among the workgroup's kept items of one round (thread order), and the round's
// total; wsum: OBS_WAVES ints of LDS.  Every thread of the workgroup calls it (two barriers).
__device__ __forceinline__ int block_keep_pos(bool keep, int* wsum, int& total)
{
    const unsigned long long m = __builtin_amdgcn_ballot_w64(keep);
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const int below = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    if (lane == 0) wsum[w] = __popcll(m);
    __syncthreads();
    int before = 0, all = 0;
    for (int i = 0; i < OBS_WAVES; i++) {
        before += (i < w) ? wsum[i] : 0;
        all += wsum[i];
    }
    __syncthreads();
    total = all;
    return before + below;
}

// grid: one workgroup per keyframe of the batch; dynamic LDS: 2 * max sort_n words
__global__ void __launch_bounds__(OBS_BLOCK) k_obs_ingest(const ObsItem* __restrict__ items, const unsigned char* __restrict__ packed,
                                                         ObsStore st, int* __restrict__ status)
{
    extern __shared__ unsigned obs_lds[];
    __shared__ int wsum[OBS_WAVES];
    __shared__ int bad;
    const ObsItem it = items[blockIdx.x];
    const int* ids = (const int*)packed + it.off;
    const float* ang = (const float*)packed + it.off + it.n_kp;
    const float* dep = (const float*)packed + it.off + 2LL * it.n_kp;
    unsigned* key = obs_lds;
    float* val = (float*)(obs_lds + it.sort_n);
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    // 1. the id >= 0 entries, in keypoint order, into LDS; a NaN or infinite angle anywhere refuses the keyframe
    int m = 0;
    for (int i0 = 0; i0 < it.n_kp; i0 += OBS_BLOCK) {
        const int i = i0 + (int)threadIdx.x;
        int id = -1;
        float a = 0.f;
        if (i < it.n_kp) {
            id = ids[i];
            a = ang[i];
            if (!__builtin_isfinite(a)) atomicOr(&bad, OBS_BAD_ANGLE);
        }
        int total;
        const int pos = block_keep_pos(id >= 0, wsum, total);
        if (id >= 0) {
            key[m + pos] = (unsigned)id;
            val[m + pos] = a;
        }
        m += total;
    }
    for (int i = m + (int)threadIdx.x; i < it.sort_n; i += OBS_BLOCK) key[i] = OBS_PAD;
    __syncthreads();
    // 2. bitonic sort by id (ids are unique in an accepted keyframe, so the order of equal keys does not matter)
    for (int k = 2; k <= it.sort_n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = (int)threadIdx.x; i < it.sort_n; i += OBS_BLOCK) {
                const int p = i ^ j;
                if (p <= i) continue;
                const unsigned ki = key[i], kp = key[p];
                const bool up = (i & k) == 0;
                if (up ? (ki > kp) : (ki < kp)) {
                    key[i] = kp;
                    key[p] = ki;
                    const float t = val[i];
                    val[i] = val[p];
                    val[p] = t;
                }
            }
            __syncthreads();
        }
    // 3. a repeated id: the host helper would emit the cross product of its matches
    for (int i = 1 + (int)threadIdx.x; i < m; i += OBS_BLOCK)
        if (key[i] == key[i - 1]) atomicOr(&bad, OBS_BAD_DUPLICATE);
    const long long base = (long long)it.slot * st.cap;
    // ... and all of them, sorted, for the covisibility weights (KeyFrame::UpdateConnections does not look at the angle)
    for (int i = (int)threadIdx.x; i < m; i += OBS_BLOCK) st.cov_ids[base + i] = (int)key[i];
    // 4. the angle >= 0 entries, still sorted, to the slot
    int kept = 0;
    for (int i0 = 0; i0 < m; i0 += OBS_BLOCK) {
        const int i = i0 + (int)threadIdx.x;
        const bool keep = i < m && val[i] >= 0.f;
        int total;
        const int pos = block_keep_pos(keep, wsum, total);
        if (keep) {
            st.ids[base + kept + pos] = (int)key[i];
            st.ang[base + kept + pos] = val[i];
        }
        kept += total;
    }
    for (int i = (int)threadIdx.x; i < it.n_depths; i += OBS_BLOCK) st.depth[base + i] = dep[i];
    __syncthreads();
    if (threadIdx.x == 0) {
        st.cnt[it.slot] = kept;
        st.nd[it.slot] = it.n_depths;
        st.cov_cnt[it.slot] = m;
        status[blockIdx.x] = bad;
    }
}

// sdm_stereo_search_constraints (PM.cc:370-383) on one wave: every lane walks the same sequence (the chunk's values come
// from readlane), so the double sums run in index order exactly as on the host
__device__ __forceinline__ void depth_bounds(const float* __restrict__ d, int n, float* mind, float* maxd)
{
    const int lane = lane_id();
    double acc = 0.0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const float v = (i0 + lane < n) ? d[i0 + lane] : 0.f;
        const int c = min(64, n - i0);
        for (int l = 0; l < c; l++) acc = acc + (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
    }
    const float sum = (float)acc;
    const float mean = sum / (float)n;
    double acc2 = 0.0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const float v = (i0 + lane < n) ? d[i0 + lane] : 0.f;
        const int c = min(64, n - i0);
        for (int l = 0; l < c; l++) {
            const float diff = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)) - mean;
            const float pr = diff * diff;
            acc2 = acc2 + (double)pr;
        }
    }
    const float variance = (float)(acc2 / (double)n);
    const float stdev = sqrtf(variance);
    if (lane == 0) {
        *maxd = 1.0f / (mean + 2.0f * stdev);  // PM.cc:381
        *mind = 1.0f / (mean - 2.0f * stdev);  // PM.cc:382
    }
}

struct PriorArgs {
    ObsStore st;
    const int* refs;  // [n_ref]
    const int* nbrs;  // [n_ref][n]
    float* rot;       // [n_ref][n] or null
    float* mind;      // [n_ref] or null (then maxd is null too)
    float* maxd;
    int n_ref, n;
    int depth_blocks;  // n_ref when the bounds are asked for, else 0
};

// grid: depth_blocks + (rot ? n_ref * n : 0) workgroups; dynamic LDS: 4 * (the largest reference list) bytes
__global__ void __launch_bounds__(OBS_BLOCK) k_priors(PriorArgs a)
{
    extern __shared__ unsigned pri_keys[];
    __shared__ int cnt[OBS_WAVES];
    __shared__ int hist[256];
    __shared__ int wtot[OBS_WAVES];
    __shared__ int sel_bin, sel_k;
    const int b = (int)blockIdx.x;
    const int w = threadIdx.x >> 6, lane = lane_id();
    if (b < a.depth_blocks) {
        if (w == 0) {
            const int s = a.refs[b];
            depth_bounds(a.st.depth + (long long)s * a.st.cap, a.st.nd[s], a.mind + b, a.maxd + b);
        }
        return;
    }
    const int pair = b - a.depth_blocks, r = pair / a.n;
    const int s1 = a.refs[r], s2 = a.nbrs[pair];
    const int* id1 = a.st.ids + (long long)s1 * a.st.cap;
    const float* an1 = a.st.ang + (long long)s1 * a.st.cap;
    const int* id2 = a.st.ids + (long long)s2 * a.st.cap;
    const float* an2 = a.st.ang + (long long)s2 * a.st.cap;
    const int m1 = a.st.cnt[s1], m2 = a.st.cnt[s2];
    // 1. join: wave w takes the reference entries [w * chunk, (w + 1) * chunk) and appends its matches to its own region
    const int chunk = (m1 + OBS_WAVES - 1) / OBS_WAVES;
    const int lo_w = min(w * chunk, m1), hi_w = min(lo_w + chunk, m1);
    unsigned* reg = pri_keys + lo_w;
    int got = 0;
    for (int i0 = lo_w; i0 < hi_w; i0 += 64) {
        const int i = i0 + lane;
        bool hit = false;
        float d = 0.f;
        if (i < hi_w) {
            const int x = id1[i];
            int lo = 0, hi = m2;  // lower_bound of x in id2[0, m2)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (id2[mid] < x) lo = mid + 1;
                else hi = mid;
            }
            if (lo < m2 && id2[lo] == x) {
                hit = true;
                d = an2[lo] - an1[i];  // PM.cc:477: angle2 - angle1 in float
            }
        }
        const unsigned long long hm = __builtin_amdgcn_ballot_w64(hit);
        const int below = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(hm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)hm, 0u));
        if (hit) reg[got + below] = f2key(d);
        got += __popcll(hm);
    }
    if (lane == 0) cnt[w] = got;
    __syncthreads();
    int m = 0;
    for (int i = 0; i < OBS_WAVES; i++) m += cnt[i];
    if (m == 0) {  // PM.cc:174-177
        if (threadIdx.x == 0) a.rot[pair] = 0.f;
        return;
    }
    // 2. radix select of rank (m - 1) / 2, most significant byte first
    int k = (m - 1) / 2;
    unsigned prefix = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[threadIdx.x] = 0;
        __syncthreads();
        const unsigned hmask = (shift == 24) ? 0u : (0xffffffffu << (shift + 8));
        for (int ww = 0; ww < OBS_WAVES; ww++) {
            const int base = min(ww * chunk, m1);
            for (int i = (int)threadIdx.x; i < cnt[ww]; i += OBS_BLOCK) {
                const unsigned key = pri_keys[base + i];
                if ((key & hmask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
            }
        }
        __syncthreads();
        // exclusive scan of the 256 bins (one per thread): wave scans, then the earlier waves' totals
        const int h = hist[threadIdx.x];
        int inc = h;
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(inc, o);
            if (lane >= o) inc += t;
        }
        if (lane == 63) wtot[w] = inc;
        __syncthreads();
        int excl = inc - h;
        for (int i = 0; i < w; i++) excl += wtot[i];
        if (h > 0 && excl <= k && k < excl + h) {
            sel_bin = (int)threadIdx.x;
            sel_k = k - excl;
        }
        __syncthreads();
        prefix |= (unsigned)sel_bin << shift;
        k = sel_k;
        __syncthreads();
    }
    if (threadIdx.x == 0) a.rot[pair] = key2f(prefix);
}

}  // namespace sdm
