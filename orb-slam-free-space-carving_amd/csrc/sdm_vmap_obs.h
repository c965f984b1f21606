// sdm_vmap_obs.h -- camera lists on the persistent voxel map as an append-only observation log (sdm_vmap_observe,
// sdm_vmap_fetch_observations, sdm_vmap_fetch_cameras; included by sdm_engine.hip).  Every entry of the map accumulates,
// across calls, the set of keyframe tags that saw any point of its voxel; each call appends exactly the (entry, tag)
// pairs that are new.
//
// State on the device (all of it the observations' own; the map's table and records are only read):
//   set      open-addressed, linear probing, load <= 0.5 (vox_mix and the probe of sdm_vmap.h), 20 B per slot:
//              keys[cap]  (u64)id << 32 | tag, or VOX_EMPTY (ids stay below 2^30 and tags below 2^31: no pair is all ones)
//              idx[cap]   the pair's index in the log, or VOBS_NOIDX (claimed in the running call)
//              ord[cap]   per call: min of the candidates' order keys; holds its identity ~0 between calls
//   log      structure of arrays indexed by the observation index k: obs_entry[k], obs_tag[k] and obs_prev[k], the previous
//            observation of the same entry (VOBS_NOIDX: none)
//   entries  last_obs[rec_cap] (head of the entry's chain, VOBS_NOIDX: never observed) and ncam[rec_cap] (its length),
//            allocated at the first observe and grown with the records
//
// One sdm_vmap_observe over the T staged plain points g = 0 .. T-1.  The host has built, per slot i of the call, the
// ascending list of the row's distinct tags (own tag included, padded to Lmax), the mask of the table columns that name
// each, and the position own[i] of the slot's own tag; it has grown set, log and entry arrays for the a-priori bound.
// Candidates are point-major, e = g * Lmax + d, so the candidate index IS the order key of the pair's log position:
//   k_vobs_insert   one lane per candidate.  Live iff d == own[i] or support[g] shares a bit with mask[i][d].  A live lane
//                   (and the d == 0 lane, which counts an unmapped point once) forms the point's cell key and finds the
//                   entry with vmap_find, read-only.  A live lane of a mapped point claims or finds the pair (atomicCAS),
//                   reduces ord (atomicMin) and notes the position in where[e].  Unmapped points and candidates are counted
//                   by ballot, one atomic per wave and counter.
//   k_vobs_count    tiles of EXT_TILE candidates: creator(e) = the slot at where[e] has no index and its ord is e
//   k_extract_scan_tiles / k_extract_scan_sums   (sdm_extract.h, unchanged) scan the tile counts
//   k_vobs_totals   created, unmapped, candidates and the overflow flag for the host's wait
//   k_vobs_commit   the lane whose e is the slot's ord -- one per touched pair -- puts ord back to its identity; if the slot
//                   has no index it is the creator: index = first_created + rank, the log entry, the chain link (atomicExch
//                   on last_obs) and ncam (atomicAdd).  No memset over the table.
//   k_vobs_rehash   (growth only) one lane per old slot re-inserts (key, idx) into the new table
//   k_vobs_list_count / k_vobs_list_offsets / k_vobs_list_fill   sdm_vmap_fetch_cameras: gather ncam of the requested
//                   entries, scan, then one lane per requested entry walks its chain into its segment, inserting each tag
//                   in ascending order
//
// No lane waits for another; every probe is bounded by the capacity, every chain walk by the length gathered before it,
// every sort by that length squared; every lane of a wave reaches every ballot.  The order in which concurrent creators of
// one entry link into its chain differs from run to run, as the table layout does; nothing returned depends on either:
// log indices come from a scan over e, and sdm_vmap_fetch_cameras sorts each list.
#pragma once
#include "sdm_vmap_carve.h"

namespace sdm {

constexpr unsigned VOBS_NOIDX = 0xffffffffu;  // no index yet / end of a chain (indices stay below 2^30)

struct VobsTable {
    unsigned long long* keys;  // [cap]
    unsigned long long* ord;   // [cap] per call; identity ~0
    unsigned* idx;             // [cap]
    unsigned long long mask;   // cap - 1, cap a power of two <= 2^31
};

struct VobsLog {
    unsigned* entry;  // [cap]
    int* tag;         // [cap]
    unsigned* prev;   // [cap]
};

struct VobsIn {
    const float* xyz;                         // [T][3] the staged plain points
    const unsigned long long* support;        // [T] the support words, or null (no neighbour table: Lmax == 1)
    const unsigned long long* plain_offsets;  // [n + 1]
    const int* row_tag;                       // [n][Lmax] ascending distinct tags of row i (padding: 0)
    const unsigned long long* row_mask;       // [n][Lmax] the columns that name each (padding: 0, never live)
    const int* own;                           // [n] position of the slot's own tag in its row
    long long T;
    int n, Lmax;
    float inv;
};

// the position of `key`: claimed if absent.  false: every slot holds another key
__device__ __forceinline__ bool vobs_claim(const VobsTable& ot, unsigned long long key, unsigned long long& h)
{
    h = vox_mix(key) & ot.mask;
    for (unsigned long long probe = 0; probe <= ot.mask; probe++) {  // bounded by the capacity
        const unsigned long long prev = atomicCAS(&ot.keys[h], VOX_EMPTY, key);
        if (prev == VOX_EMPTY || prev == key) return true;
        h = (h + 1) & ot.mask;
    }
    return false;
}

// candidates e0 + thread of the slice; ctr = {unmapped points, candidates, overflow}
__global__ __launch_bounds__(BLOCK) void k_vobs_insert(VobsIn in, long long e0, long long Ec, VmapTable tb, VobsTable ot,
                                                       unsigned* __restrict__ where, unsigned long long* __restrict__ ctr)
{
    const long long e = e0 + (long long)blockIdx.x * BLOCK + threadIdx.x;
    bool unmapped = false, cand = false;
    if (e < Ec) {
        const long long g = e / in.Lmax;
        const int d = (int)(e - g * in.Lmax);
        const int i = vmap_slot_of(in.plain_offsets, in.n, (unsigned long long)g);
        const size_t at = (size_t)i * (size_t)in.Lmax + (size_t)d;
        const bool live = d == in.own[i] || (in.support && (in.support[g] & in.row_mask[at]) != 0ull);
        unsigned w = VOX_NONE;
        if (live || d == 0) {
            const unsigned long long cell = vox_key(in.xyz[g * 3 + 0], in.xyz[g * 3 + 1], in.xyz[g * 3 + 2], in.inv);
            const unsigned id = cell == VOX_EMPTY ? VMAP_NOID : vmap_find(tb, cell);
            unmapped = d == 0 && id == VMAP_NOID;
            if (live && id != VMAP_NOID) {
                cand = true;
                unsigned long long h;
                if (vobs_claim(ot, ((unsigned long long)id << 32) | (unsigned long long)(unsigned)in.row_tag[at], h)) {
                    atomicMin(&ot.ord[h], (unsigned long long)e);
                    w = (unsigned)h;
                } else {
                    atomicOr(&ctr[2], 1ull);
                }
            }
        }
        where[e] = w;
    }
    const unsigned long long um = __ballot(unmapped), cm = __ballot(cand);  // (every lane of the wave arrives here)
    if ((threadIdx.x & 63) == 0) {
        if (um) atomicAdd(&ctr[0], (unsigned long long)__popcll(um));
        if (cm) atomicAdd(&ctr[1], (unsigned long long)__popcll(cm));
    }
}

// candidate e creates its pair: the slot has no index and e is the smallest order key that reached it
__device__ __forceinline__ bool vobs_creator(const VobsTable& ot, const unsigned* __restrict__ where, long long e, long long Ec)
{
    if (e >= Ec) return false;
    const unsigned w = where[e];
    return w != VOX_NONE && ot.idx[w] == VOBS_NOIDX && ot.ord[w] == (unsigned long long)e;
}

// one workgroup per tile tile0 + block of EXT_TILE consecutive candidates
__global__ __launch_bounds__(BLOCK) void k_vobs_count(VobsTable ot, const unsigned* __restrict__ where, long long Ec,
                                                      long long tile0, unsigned* __restrict__ tile_cnt)
{
    __shared__ unsigned wsum[EXT_WAVES];
    const long long tile = tile0 + blockIdx.x;
    const long long base = tile * EXT_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned mine = 0;
#pragma unroll
    for (int k = 0; k < EXT_PER; k++)
        mine += (unsigned)__popcll(__ballot(vobs_creator(ot, where, base + k * BLOCK + threadIdx.x, Ec)));
    if (lane == 0) wsum[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = 0;
        for (int v = 0; v < EXT_WAVES; v++) t += wsum[v];
        tile_cnt[tile] = t;
    }
}

// out = {created, unmapped, candidates, overflow}
__global__ void k_vobs_totals(long long nt, const unsigned* __restrict__ tile_off, const unsigned long long* __restrict__ blk_off,
                              const unsigned long long* __restrict__ ctr, unsigned long long* __restrict__ out)
{
    if (blockIdx.x || threadIdx.x) return;
    out[0] = ext_tile_offset(tile_off, blk_off, nt);
    out[1] = ctr[0];
    out[2] = ctr[1];
    out[3] = ctr[2];
}

// creators take index first_created + rank, write the log entry and link it; every pair's minimum lane restores ord
__global__ __launch_bounds__(BLOCK) void k_vobs_commit(VobsTable ot, VobsLog lg, unsigned* __restrict__ last_obs,
                                                       unsigned* __restrict__ ncam, const unsigned* __restrict__ where,
                                                       unsigned first_created, long long Ec, long long tile0,
                                                       const unsigned* __restrict__ tile_off,
                                                       const unsigned long long* __restrict__ blk_off)
{
    __shared__ unsigned wcnt[EXT_PER][EXT_WAVES];
    const long long tile = tile0 + blockIdx.x;
    const long long base = tile * EXT_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned w[EXT_PER], below[EXT_PER];
    bool f[EXT_PER];
#pragma unroll
    for (int k = 0; k < EXT_PER; k++) {
        const long long e = base + k * BLOCK + threadIdx.x;
        w[k] = VOX_NONE;
        f[k] = false;
        if (e < Ec) w[k] = where[e];
        if (w[k] != VOX_NONE) {
            if (ot.ord[w[k]] == (unsigned long long)e) {  // the one lane that touches this slot in this launch
                f[k] = ot.idx[w[k]] == VOBS_NOIDX;
                ot.ord[w[k]] = ~0ull;
            } else {
                w[k] = VOX_NONE;
            }
        }
        const unsigned long long m = __ballot(f[k]);
        below[k] = ext_lanes_below(m);
        if (lane == 0) wcnt[k][wave] = (unsigned)__popcll(m);
    }
    __syncthreads();
    unsigned long long pos = ext_tile_offset(tile_off, blk_off, tile);
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
            const unsigned idx = first_created + (unsigned)(pos + lower + below[k]);
            const unsigned long long key = ot.keys[w[k]];
            const unsigned id = (unsigned)(key >> 32);
            ot.idx[w[k]] = idx;
            lg.entry[idx] = id;
            lg.tag[idx] = (int)(unsigned)key;
            lg.prev[idx] = atomicExch(&last_obs[id], idx);
            atomicAdd(&ncam[id], 1u);
        }
        pos += round;
    }
}

// growth: one lane per slot h0 + thread of the old table re-inserts (key, idx) into `nw` (its ord holds the identity)
__global__ __launch_bounds__(BLOCK) void k_vobs_rehash(const unsigned long long* __restrict__ old_keys,
                                                       const unsigned* __restrict__ old_idx, unsigned long long old_cap,
                                                       unsigned long long h0, VobsTable nw, unsigned* __restrict__ overflow)
{
    const unsigned long long s = h0 + (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= old_cap) return;
    const unsigned long long key = old_keys[s];
    if (key == VOX_EMPTY) return;
    unsigned long long h;
    if (!vobs_claim(nw, key, h)) {
        atomicOr(overflow, 1u);
        return;
    }
    nw.idx[h] = old_idx[s];
}

// sdm_vmap_fetch_cameras: len[j] = list length of requested entry j0 + thread (ids == null: entry first + j; a null ncam
// reads as 0: nothing has been observed); *bad |= 1 for an id >= M
__global__ __launch_bounds__(BLOCK) void k_vobs_list_count(const unsigned* __restrict__ ncam, const unsigned* __restrict__ ids,
                                                           long long first, long long count, long long j0, unsigned M,
                                                           unsigned* __restrict__ len, unsigned* __restrict__ bad)
{
    const long long j = j0 + (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= count) return;
    const unsigned e = ids ? ids[j] : (unsigned)(first + j);
    if (e >= M) {
        atomicOr(bad, 1u);
        len[j] = 0u;
        return;
    }
    len[j] = ncam ? ncam[e] : 0u;
}

// cam_offsets[j] for j = j0 + thread <= count, and the total
__global__ __launch_bounds__(BLOCK) void k_vobs_list_offsets(const unsigned* __restrict__ tile_off,
                                                             const unsigned long long* __restrict__ blk_off, long long count,
                                                             long long j0, long long* __restrict__ cam_offsets,
                                                             unsigned long long* __restrict__ total)
{
    const long long j = j0 + (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (j > count) return;
    const unsigned long long o = ext_tile_offset(tile_off, blk_off, j);
    if (cam_offsets) cam_offsets[j] = (long long)o;
    if (j == count) *total = o;
}

// requested entry j0 + thread walks its chain and inserts every tag into its segment in ascending order
__global__ __launch_bounds__(BLOCK) void k_vobs_list_fill(VobsLog lg, const unsigned* __restrict__ last_obs,
                                                          const unsigned* __restrict__ ids, long long first, long long count,
                                                          long long j0, unsigned M, const unsigned* __restrict__ len,
                                                          const unsigned* __restrict__ tile_off,
                                                          const unsigned long long* __restrict__ blk_off,
                                                          int* __restrict__ cam_tags)
{
    const long long j = j0 + (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= count) return;
    const unsigned L = len[j];
    if (L == 0u) return;  // (also an id >= M)
    const unsigned e = ids ? ids[j] : (unsigned)(first + j);
    if (e >= M) return;
    int* seg = cam_tags + ext_tile_offset(tile_off, blk_off, j);
    unsigned k = last_obs[e];
    for (unsigned m = 0; m < L && k != VOBS_NOIDX; m++) {  // bounded by the gathered length
        const int t = lg.tag[k];
        unsigned p = m;
        while (p > 0 && seg[p - 1] > t) {  // (at most m steps)
            seg[p] = seg[p - 1];
            p--;
        }
        seg[p] = t;
        k = lg.prev[k];
    }
}

// sdm_selftest(16), (17), (18): how far the table's keys sit from home.  One lane per slot s0 + thread of `keys`, read-only:
// out[0] = max over the occupied slots of (slot - home) & mask, out[1] = occupied slots below their home (the key's probe
// went past the table's end).  Serves the map's table, the observation set and the per-call table: all hash with vox_mix.
__global__ __launch_bounds__(BLOCK) void k_selftest_table_layout(const unsigned long long* __restrict__ keys,
                                                                 unsigned long long cap, unsigned long long s0,
                                                                 unsigned long long* __restrict__ out)
{
    const unsigned long long s = s0 + (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    unsigned long long disp = 0;
    bool wrapped = false;
    if (s < cap) {
        const unsigned long long key = keys[s];
        if (key != VOX_EMPTY) {
            const unsigned long long home = vox_mix(key) & (cap - 1);
            disp = (s - home) & (cap - 1);
            wrapped = s < home;
        }
    }
    if (disp) atomicMax(&out[0], disp);
    const unsigned long long wm = __ballot(wrapped);  // (every lane of the wave arrives here)
    if (wm && (threadIdx.x & 63) == 0) atomicAdd(&out[1], (unsigned long long)__popcll(wm));
}

}  // namespace sdm
