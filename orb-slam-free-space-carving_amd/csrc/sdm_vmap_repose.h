// sdm_vmap_repose.h -- re-placing the persistent voxel map under new keyframe poses (sdm_vmap_repose; included by
// sdm_engine.hip).  Every entry's record carries the winning point's pixel, the rho that passed and the keyframe tag, and
// xyz is a pure function of (pixel, rho, K, Tcw): the call recomputes every entry's xyz from a table of (tag, K, Tcw), bins
// the entries again under sdm_vmap_import's order semantics and carries the observation log, the free-space counters and
// the published flags through the id map.  Nothing crosses the link but the pose table and, if asked for, the id map.
//
// One sdm_vmap_repose over the M old entries i = 0 .. M-1 (the host has sorted the pose table by tag, uploaded it, and made
// a second set of records, and with carry a second set of counters and flags, before anything is written):
//   k_vrep_project  one lane per entry: a binary search of the entry's tag in the table; a hit calls pointset_pixel -- the
//                   device function of UpdateSemiDensePointSet itself, sdm_kernels.h -- with x = pixel & 0xffff,
//                   y = pixel >> 16 and the stored rho, a miss copies the stored bits.  The result goes to a scratch
//                   xyz[M][3]; `reposed` and `moved` (any of the 96 bits differs) are counted by ballot, one atomic per wave
//                   and counter.  Every lane searches for itself: a wave-uniform shortcut for neighbours that share a tag
//                   has not been tried.
//   (memset)        the table goes back to empty keys and the reductions' identities; its size stays
//   k_vimp_insert / k_vmap_count / scans / k_vmap_totals / k_vmap_ids / k_vimp_commit / k_vimp_write   (sdm_vmap_import.h)
//                   exactly one import of the M records {scratch xyz; the OLD record arrays' pixel, rho_sigma, intensity,
//                   tag, multiplicity} into the empty table and the NEW record arrays, with first_created = 0: ids in the
//                   order of first appearance, the smallest key(sigma) wins and a tie goes to the lower old id,
//                   multiplicities add and saturate.  k_vimp_write takes the winner's epoch from the old records instead of
//                   the call's, and its dst_ids is the id map `remap`.
//   k_vrep_carry    (carry == 1) one lane per old entry: two 64-bit atomic adds of its counters and, if it is published, a
//                   store of 1, at remap[i] in the new arrays (which start at 0).  Every lane that stores to a flag stores
//                   the same byte.
//   k_vrep_count    one lane per new entry: the published flags counted by ballot
//   k_vobs_import_insert / k_vobs_count / scans / k_vobs_totals / k_vobs_commit   (sdm_vmap_import.h, sdm_vmap_obs.h) the
//                   observation set and the entries' chains are emptied by memset and the old log is imported through
//                   remap IN PLACE: the insert launch has read every old pair before the commit launch writes the first new
//                   one, and a new index never exceeds the old index of the pair that creates it.
//
// No lane waits for another; every probe is bounded by the capacity and the search by log2 of the table.  Everything
// written is copied bits, an integer reduction, or pointset_pixel's one formula per entry: no output depends on the table
// layout or on the order of the atomics.  Plain C++ and vector stores only.
#pragma once
#include "sdm_vmap_import.h"

namespace sdm {

// one lane per old entry i0 + thread; ctr[0] += entries whose tag is in the table, ctr[1] += those whose xyz changed
__global__ __launch_bounds__(BLOCK) void k_vrep_project(VmapRecords rec, long long M, long long i0,
                                                        const int* __restrict__ tags, const KfMeta* __restrict__ poses, int n,
                                                        float* __restrict__ xyz, unsigned long long* __restrict__ ctr)
{
    const long long i = i0 + (long long)blockIdx.x * BLOCK + threadIdx.x;
    bool hit = false, mov = false;
    if (i < M) {
        float o[3] = {rec.xyz[(size_t)i * 3 + 0], rec.xyz[(size_t)i * 3 + 1], rec.xyz[(size_t)i * 3 + 2]};
        const int t = rec.tag[i];
        int lo = 0, hi = n;  // the first table position whose tag is not below t
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (tags[mid] < t) lo = mid + 1;
            else hi = mid;
        }
        if (lo < n && tags[lo] == t) {
            hit = true;
            const unsigned px = rec.pixel[i];
            float p[3];
            pointset_pixel(poses[lo], (int)(px & 0xffffu), (int)(px >> 16), rec.rho_sigma[i].x, p);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                mov = mov || __float_as_uint(p[k]) != __float_as_uint(o[k]);
                o[k] = p[k];
            }
        }
        xyz[(size_t)i * 3 + 0] = o[0];
        xyz[(size_t)i * 3 + 1] = o[1];
        xyz[(size_t)i * 3 + 2] = o[2];
    }
    const unsigned long long hm = __ballot(hit), mm = __ballot(mov);  // (every lane of the wave arrives here)
    if ((threadIdx.x & 63) == 0) {
        if (hm) atomicAdd(&ctr[0], (unsigned long long)__popcll(hm));
        if (mm) atomicAdd(&ctr[1], (unsigned long long)__popcll(mm));
    }
}

// one lane per old entry i0 + thread: its counters and its flag go to the entry that holds its voxel now (any source array
// may be null with its destination: that evidence was never made)
__global__ __launch_bounds__(BLOCK) void k_vrep_carry(const unsigned* __restrict__ remap, long long M, long long i0,
                                                      const unsigned long long* __restrict__ old_crossings,
                                                      const unsigned long long* __restrict__ old_ends,
                                                      unsigned long long* __restrict__ crossings,
                                                      unsigned long long* __restrict__ ends,
                                                      const unsigned char* __restrict__ old_published,
                                                      unsigned char* __restrict__ published)
{
    const long long i = i0 + (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= M) return;
    const unsigned e = remap[i];
    if (e == VMAP_NOID) return;
    if (old_crossings) {
        const unsigned long long a = old_crossings[i], b = old_ends[i];
        if (a) atomicAdd(&crossings[e], a);
        if (b) atomicAdd(&ends[e], b);
    }
    if (old_published && old_published[i]) published[e] = (unsigned char)1;
}

// one lane per new entry j0 + thread; *total += published flags
__global__ __launch_bounds__(BLOCK) void k_vrep_count(const unsigned char* __restrict__ published, long long M, long long j0,
                                                      unsigned long long* __restrict__ total)
{
    const long long j = j0 + (long long)blockIdx.x * BLOCK + threadIdx.x;
    const unsigned long long m = __ballot(j < M && published[j] != 0);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(total, (unsigned long long)__popcll(m));
}

}  // namespace sdm
