// sdm_vmap_retire.h -- retiring keyframes from the persistent voxel map (sdm_vmap_retire; included by sdm_engine.hip).  A
// set R of keyframe tags leaves the map: its pairs leave the observation log, the entries that do not survive (mode WINNER:
// the record's tag is in R; mode UNOBSERVED: no pair of a live keyframe is left) leave table and records, the survivors
// move up to the rank they have among the survivors, and the call lists what a consumer has to delete.
//
// One sdm_vmap_retire over the M old entries i = 0 .. M-1 and the E old pairs k = 0 .. E-1 (the host has sorted R and
// uploaded it, 4 B per tag).  The marking phase reads the map and writes scratch only:
//   k_vret_pairs     one lane per pair: a binary search of its tag in R into pmark[k] (VRET_REMOVED: retired); in mode
//                    UNOBSERVED a live pair stores the byte 1 to seen[entry].  Every lane that stores there stores the same
//                    byte
//   k_vret_entries   one lane per entry: emark[i] bit 0 = survivor (WINNER: a binary search of the record's tag;
//                    UNOBSERVED: seen[i]), bit 1 = its published flag.  Orphans (survivor whose record's tag is in R),
//                    dropped-and-published and surviving-and-published entries are counted by ballot, one atomic per wave
//                    and counter
//   k_vret_vanish    one lane per pair: a pair of a dropped entry becomes VRET_VANISHED, whatever it was
//   k_vret_count     tiles of EXT_TILE marks, two counts per tile (entries: survivors, dropped; pairs: removed, vanished)
//   k_extract_scan_tiles / k_extract_scan_sums   (sdm_extract.h, unchanged) scan the four tile counts
//   k_vret_totals    the seven counts for the host's first wait
// After the wait the host checks the capacities; a refused call has written no list and changed nothing.  Then:
//   k_vret_remap     tiles of entries: remap[i] = rank among the survivors or VMAP_NOID; a dropped entry lists its OLD id and
//                    its flag at its rank among the dropped
//   k_vret_removed   tiles of pairs: a VRET_REMOVED pair lists its OLD entry id and its tag at its rank (old log order)
// and with commit:
//   k_vret_records   one lane per old entry: a survivor copies the seven fields of its record -- and with carry its two
//                    counters and its flag -- to remap[i] in a SECOND set of arrays, made before anything is written and
//                    swapped in at the end.  Compaction in place is not safe: remap[i] <= i, but the lane of entry remap[i]
//                    may belong to another workgroup that has not read its record yet, and nothing orders workgroups
//   (memset)         the table goes back to empty keys and the reductions' identities; its size stays.  Linear probing has
//                    no tombstones, so nothing is deleted slot by slot and vmap_find stays as it is
//   k_vret_table     one lane per NEW entry: vox_key of its xyz is the cell key it was stored under; (key, new id) is
//                    inserted in the manner of k_vmap_rehash
//   k_vobs_import_insert / k_vobs_count / scans / k_vobs_totals / k_vobs_commit   (sdm_vmap_import.h, sdm_vmap_obs.h) the
//                    observation set and the entries' chains are emptied by memset and the old log is imported through
//                    remap IN PLACE as sdm_vmap_repose does it; k_vobs_import_insert's `skip` is pmark, so a retired pair
//                    is rejected like the pair of a dropped entry.  The insert launch has read every old pair before the
//                    commit launch writes the first new one, and a new index never exceeds the old index of its pair.
//
// No lane waits for another; every probe is bounded by the capacity and every search by log2 of |R|; every lane of a wave
// reaches every ballot.  Everything written is copied bits, an integer count or a rank from a scan: every output is bitwise
// the same from run to run, whatever the table layout.  Plain C++ and vector stores only.
#pragma once
#include "sdm_vmap_repose.h"

namespace sdm {

constexpr unsigned char VRET_KEPT = 0, VRET_REMOVED = 1, VRET_VANISHED = 2;  // pmark[k]

// t is one of the n ascending tags
__device__ __forceinline__ bool vret_retired(const int* __restrict__ tags, int n, int t)
{
    int lo = 0, hi = n;  // the first position whose tag is not below t
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tags[mid] < t) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && tags[lo] == t;
}

// one lane per old pair k0 + thread; seen == null in mode WINNER
__global__ __launch_bounds__(BLOCK) void k_vret_pairs(const unsigned* __restrict__ entry, const int* __restrict__ tag, long long E,
                                                      long long k0, unsigned M, const int* __restrict__ tags, int n,
                                                      unsigned char* __restrict__ pmark, unsigned char* __restrict__ seen)
{
    const long long k = k0 + (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= E) return;
    const bool ret = vret_retired(tags, n, tag[k]);
    pmark[k] = ret ? VRET_REMOVED : VRET_KEPT;
    if (!ret && seen) {
        const unsigned id = entry[k];
        if (id < M) seen[id] = (unsigned char)1;
    }
}

// one lane per old entry i0 + thread; ctr = {orphaned, dropped and published, surviving and published}
__global__ __launch_bounds__(BLOCK) void k_vret_entries(const int* __restrict__ rec_tag, const unsigned char* __restrict__ published,
                                                        const unsigned char* __restrict__ seen, long long M, long long i0,
                                                        const int* __restrict__ tags, int n, unsigned char* __restrict__ emark,
                                                        unsigned long long* __restrict__ ctr)
{
    const long long i = i0 + (long long)blockIdx.x * BLOCK + threadIdx.x;
    bool orphan = false, dpub = false, spub = false;
    if (i < M) {
        const bool ret = vret_retired(tags, n, rec_tag[i]);
        const bool surv = seen ? seen[i] != 0 : !ret;
        const bool pub = published && published[i] != 0;
        emark[i] = (unsigned char)((surv ? 1u : 0u) | (pub ? 2u : 0u));
        orphan = surv && ret;
        dpub = !surv && pub;
        spub = surv && pub;
    }
    const unsigned long long om = __ballot(orphan), dm = __ballot(dpub), sm = __ballot(spub);  // (every lane arrives here)
    if ((threadIdx.x & 63) == 0) {
        if (om) atomicAdd(&ctr[0], (unsigned long long)__popcll(om));
        if (dm) atomicAdd(&ctr[1], (unsigned long long)__popcll(dm));
        if (sm) atomicAdd(&ctr[2], (unsigned long long)__popcll(sm));
    }
}

// one lane per old pair k0 + thread: the pairs of a dropped entry go with it
__global__ __launch_bounds__(BLOCK) void k_vret_vanish(const unsigned* __restrict__ entry, long long E, long long k0, unsigned M,
                                                       const unsigned char* __restrict__ emark, unsigned char* __restrict__ pmark)
{
    const long long k = k0 + (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= E) return;
    const unsigned id = entry[k];
    if (id >= M || !(emark[id] & 1u)) pmark[k] = VRET_VANISHED;
}

// one workgroup per tile tile0 + block of EXT_TILE consecutive marks: cnt_a counts (mark & mask) == a, cnt_b those == b
__global__ __launch_bounds__(BLOCK) void k_vret_count(const unsigned char* __restrict__ mark, unsigned mask, unsigned a, unsigned b,
                                                      long long N, long long tile0, unsigned* __restrict__ cnt_a,
                                                      unsigned* __restrict__ cnt_b)
{
    __shared__ unsigned wsum[2][EXT_WAVES];
    const long long tile = tile0 + blockIdx.x;
    const long long base = tile * EXT_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned na = 0, nb = 0;
#pragma unroll
    for (int k = 0; k < EXT_PER; k++) {
        const long long j = base + k * BLOCK + threadIdx.x;
        const unsigned m = j < N ? (mark[j] & mask) : ~0u;
        na += (unsigned)__popcll(__ballot(m == a));  // (every lane of the wave arrives here)
        nb += (unsigned)__popcll(__ballot(m == b));
    }
    if (lane == 0) wsum[0][wave] = na, wsum[1][wave] = nb;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned ta = 0, tb = 0;
        for (int v = 0; v < EXT_WAVES; v++) ta += wsum[0][v], tb += wsum[1][v];
        cnt_a[tile] = ta;
        cnt_b[tile] = tb;
    }
}

// out = {survivors, dropped, removed, vanished, orphaned, dropped and published, surviving and published} (np == 0: no pair)
__global__ void k_vret_totals(long long ne, const unsigned* __restrict__ off_s, const unsigned long long* __restrict__ blk_s,
                              const unsigned* __restrict__ off_d, const unsigned long long* __restrict__ blk_d, long long np,
                              const unsigned* __restrict__ off_r, const unsigned long long* __restrict__ blk_r,
                              const unsigned* __restrict__ off_v, const unsigned long long* __restrict__ blk_v,
                              const unsigned long long* __restrict__ ctr, unsigned long long* __restrict__ out)
{
    if (blockIdx.x || threadIdx.x) return;
    out[0] = ext_tile_offset(off_s, blk_s, ne);
    out[1] = ext_tile_offset(off_d, blk_d, ne);
    out[2] = np ? ext_tile_offset(off_r, blk_r, np) : 0ull;
    out[3] = np ? ext_tile_offset(off_v, blk_v, np) : 0ull;
    out[4] = ctr[0];
    out[5] = ctr[1];
    out[6] = ctr[2];
}

// survivors take their rank as new id; the dropped list their old id and flag at theirs (either list may be null)
__global__ __launch_bounds__(BLOCK) void k_vret_remap(const unsigned char* __restrict__ emark, long long M, long long tile0,
                                                      const unsigned* __restrict__ off_s, const unsigned long long* __restrict__ blk_s,
                                                      const unsigned* __restrict__ off_d, const unsigned long long* __restrict__ blk_d,
                                                      unsigned* __restrict__ remap, unsigned* __restrict__ dropped_ids,
                                                      unsigned char* __restrict__ dropped_published)
{
    __shared__ unsigned wcnt[2][EXT_PER][EXT_WAVES];
    const long long tile = tile0 + blockIdx.x;
    const long long base = tile * EXT_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned m[EXT_PER], below_s[EXT_PER], below_d[EXT_PER];
#pragma unroll
    for (int k = 0; k < EXT_PER; k++) {
        const long long i = base + k * BLOCK + threadIdx.x;
        m[k] = i < M ? (unsigned)emark[i] : ~0u;
        const unsigned long long ms = __ballot(m[k] != ~0u && (m[k] & 1u)), md = __ballot(m[k] != ~0u && !(m[k] & 1u));
        below_s[k] = ext_lanes_below(ms);
        below_d[k] = ext_lanes_below(md);
        if (lane == 0) wcnt[0][k][wave] = (unsigned)__popcll(ms), wcnt[1][k][wave] = (unsigned)__popcll(md);
    }
    __syncthreads();
    unsigned long long pos_s = ext_tile_offset(off_s, blk_s, tile), pos_d = ext_tile_offset(off_d, blk_d, tile);
#pragma unroll
    for (int k = 0; k < EXT_PER; k++) {
        unsigned lower_s = 0, round_s = 0, lower_d = 0, round_d = 0;
#pragma unroll
        for (int v = 0; v < EXT_WAVES; v++) {
            const unsigned cs = wcnt[0][k][v], cd = wcnt[1][k][v];
            if (v < wave) lower_s += cs, lower_d += cd;
            round_s += cs, round_d += cd;
        }
        const long long i = base + k * BLOCK + threadIdx.x;
        if (m[k] != ~0u) {
            if (m[k] & 1u) {
                if (remap) remap[i] = (unsigned)(pos_s + lower_s + below_s[k]);
            } else {
                const unsigned long long o = pos_d + lower_d + below_d[k];
                if (remap) remap[i] = VMAP_NOID;
                if (dropped_ids) dropped_ids[o] = (unsigned)i;
                if (dropped_published) dropped_published[o] = (unsigned char)((m[k] >> 1) & 1u);
            }
        }
        pos_s += round_s, pos_d += round_d;
    }
}

// the retired pairs of surviving entries list their old entry id and tag at their rank (removed_tag may be null)
__global__ __launch_bounds__(BLOCK) void k_vret_removed(const unsigned char* __restrict__ pmark, const unsigned* __restrict__ entry,
                                                        const int* __restrict__ tag, long long E, long long tile0,
                                                        const unsigned* __restrict__ off_r, const unsigned long long* __restrict__ blk_r,
                                                        unsigned* __restrict__ removed_entry, int* __restrict__ removed_tag)
{
    __shared__ unsigned wcnt[EXT_PER][EXT_WAVES];
    const long long tile = tile0 + blockIdx.x;
    const long long base = tile * EXT_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned below[EXT_PER];
    bool f[EXT_PER];
#pragma unroll
    for (int k = 0; k < EXT_PER; k++) {
        const long long j = base + k * BLOCK + threadIdx.x;
        f[k] = j < E && pmark[j] == VRET_REMOVED;
        const unsigned long long m = __ballot(f[k]);
        below[k] = ext_lanes_below(m);
        if (lane == 0) wcnt[k][wave] = (unsigned)__popcll(m);
    }
    __syncthreads();
    unsigned long long pos = ext_tile_offset(off_r, blk_r, tile);
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
            const long long j = base + k * BLOCK + threadIdx.x;
            const unsigned long long o = pos + lower + below[k];
            removed_entry[o] = entry[j];
            if (removed_tag) removed_tag[o] = tag[j];
        }
        pos += round;
    }
}

// one lane per old entry i0 + thread: a survivor's record, and with carry its counters and flag (any of the three source
// arrays may be null with its destination), go to remap[i] in the second set
__global__ __launch_bounds__(BLOCK) void k_vret_records(VmapRecords old, VmapRecords nw, const unsigned* __restrict__ remap,
                                                        long long M, long long i0,
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
    nw.xyz[(size_t)e * 3 + 0] = old.xyz[(size_t)i * 3 + 0];
    nw.xyz[(size_t)e * 3 + 1] = old.xyz[(size_t)i * 3 + 1];
    nw.xyz[(size_t)e * 3 + 2] = old.xyz[(size_t)i * 3 + 2];
    nw.pixel[e] = old.pixel[i];
    nw.rho_sigma[e] = old.rho_sigma[i];
    nw.intensity[e] = old.intensity[i];
    nw.tag[e] = old.tag[i];
    nw.multiplicity[e] = old.multiplicity[i];
    nw.epoch[e] = old.epoch[i];
    if (old_crossings) {
        crossings[e] = old_crossings[i];
        ends[e] = old_ends[i];
    }
    if (old_published) published[e] = old_published[i];
}

// one lane per new entry j0 + thread re-inserts (cell key, j) into the emptied table; ctr[1] |= overflow
__global__ __launch_bounds__(BLOCK) void k_vret_table(const float* __restrict__ xyz, long long M, long long j0, float inv,
                                                      VmapTable tb, unsigned* __restrict__ ctr)
{
    const long long j = j0 + (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= M) return;
    const unsigned long long key = vox_key(xyz[(size_t)j * 3 + 0], xyz[(size_t)j * 3 + 1], xyz[(size_t)j * 3 + 2], inv);
    unsigned long long h;
    if (key == VOX_EMPTY || !vmap_claim(tb, key, h)) {  // (neither can happen: the entry was stored under this key)
        atomicOr(&ctr[1], 1u);
        return;
    }
    tb.id[h] = (unsigned)j;
}

}  // namespace sdm
