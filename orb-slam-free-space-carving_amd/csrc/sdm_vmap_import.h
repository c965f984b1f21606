// sdm_vmap_import.h -- importing records and observations into the persistent voxel map (sdm_vmap_import,
// sdm_vmap_import_observations; included by sdm_engine.hip).  What sdm_vmap_fetch and sdm_vmap_fetch_observations wrote is
// read back in here: the maps of several ranks merge into one, a saved map is restored, a map is re-binned at another
// voxel size.  The order semantics are sdm_vmap_integrate's and sdm_vmap_observe's; the state is theirs too (sdm_vmap.h,
// sdm_vmap_obs.h): nothing is added to a table slot or a record.
//
// One sdm_vmap_import over the R source records r = 0 .. R-1 (the host has staged host sources and grown table and records):
//   k_vimp_insert   one lane per record: a record with an unmergeable xyz or multiplicity 0 gets VOX_NONE and is counted as
//                   dropped; every other claims or finds its cell key and reduces the three per-call fields exactly as
//                   k_vmap_insert does, with r in the place of g -- except that ccnt receives the record's multiplicity
//                   m_r, not 1.  The call's contribution must saturate, not wrap, and ccnt stays 32 bits (28 B per slot):
//                   vimp_add_sat is a compare-and-swap loop that writes min(2^32 - 1, old + m_r).  min(SAT, sum) does not
//                   depend on the order of the additions, and k_vmap_ids' saturating add of ccnt onto the stored
//                   multiplicity then gives min(SAT, multiplicity + sum of m_r) whatever either clamp did.  The sum of
//                   the stored m_r (64 bits, for `points`) is reduced per wave and added once per wave.
//   k_vmap_count / k_extract_scan_tiles / k_extract_scan_sums / k_vmap_totals / k_vmap_ids   (unchanged) work on where[]
//                   and the table fields alone
//   k_vimp_commit   k_vmap_commit without the record: updaters write updated_ids[rank], the first-record lanes put cfirst
//                   and ccnt back to their identities; cval and the stored sigma are left for the next launch
//   k_vimp_write    one lane per record, no tile: writes dst_ids[r], the entry of its record (every id is known:
//                   k_vmap_ids was an earlier launch) or VMAP_NOID for a dropped one; the call's winner of a new or beaten
//                   voxel writes the record and the TAG OF ITS SOURCE RECORD from the sources and puts cval back.  Two
//                   kernels because one that holds table, records, sources and both lists needs more scalar registers
//                   than there are; the price is one more pass over 16 B per record (where, id, cval).
//
// One sdm_vmap_import_observations over the P pairs k = 0 .. P-1:
//   k_vobs_import_insert   one lane per pair, candidate index e = k: resolves the entry (through entry_map if given),
//                   rejects an entry >= M or a tag < 0 (counted by ballot), claims or finds the pair in the observation
//                   set, reduces ord with k and notes the position in where[k]
//   k_vobs_count / scans / k_vobs_totals / k_vobs_commit   (unchanged) read only where[] and the set
//
// No lane waits for another: a probe is bounded by the capacity, and a round of vimp_add_sat is repeated only when another
// lane's compare-and-swap on the same word succeeded in between (or when the word has reached 2^32 - 1, where it ends), so a
// lane retries at most once per other record of its voxel in the call.  Plain C++ and vector stores only.
#pragma once
#include "sdm_vmap_obs.h"

namespace sdm {

// the sources of sdm_vmap_import on the device: what sdm_vmap_fetch writes (null: pixel, intensity, tag read 0; multiplicity 1)
struct VimpSrc {
    const float* xyz;                // [R][3]
    const float2* rho_sigma;         // [R]
    const unsigned* pixel;           // [R] or null
    const unsigned char* intensity;  // [R] or null
    const int* tag;                  // [R] or null
    const unsigned* multiplicity;    // [R] or null
};

// *p = min(2^32 - 1, *p + m)
__device__ __forceinline__ void vimp_add_sat(unsigned* p, unsigned m)
{
    unsigned old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old != 0xffffffffu) {
        const unsigned sum = old + m < old ? 0xffffffffu : old + m;
        const unsigned prev = atomicCAS(p, old, sum);
        if (prev == old) break;
        old = prev;  // (another lane's addition landed in between)
    }
}

// one lane per source record r0 + thread; ctr[0] += dropped records, ctr[1] |= overflow, *msum += stored multiplicities
__global__ __launch_bounds__(BLOCK) void k_vimp_insert(VimpSrc src, long long R, long long r0, float inv, VmapTable tb,
                                                       unsigned* __restrict__ where, unsigned* __restrict__ ctr,
                                                       unsigned long long* __restrict__ msum)
{
    const long long r = r0 + (long long)blockIdx.x * BLOCK + threadIdx.x;
    unsigned long long key = VOX_EMPTY;
    unsigned m = 0u;
    if (r < R) {
        m = src.multiplicity ? src.multiplicity[r] : 1u;
        if (m) key = vox_key(src.xyz[r * 3 + 0], src.xyz[r * 3 + 1], src.xyz[r * 3 + 2], inv);
    }
    unsigned long long h = 0;
    bool stored = false;
    if (key != VOX_EMPTY) {
        if (vmap_claim(tb, key, h)) {
            stored = true;
            atomicMin(&tb.cval[h], ((unsigned long long)f2key(src.rho_sigma[r].y) << 32) | (unsigned long long)r);
            atomicMin(&tb.cfirst[h], (unsigned)r);
            vimp_add_sat(&tb.ccnt[h], m);
        } else {
            atomicOr(&ctr[1], 1u);
        }
    }
    if (r < R) where[r] = stored ? (unsigned)h : VOX_NONE;
    // (every lane of the wave arrives here)
    const unsigned long long drop = __ballot(r < R && key == VOX_EMPTY);
    unsigned long long add = stored ? (unsigned long long)m : 0ull;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) add += __shfl_down(add, off);
    if ((threadIdx.x & 63) == 0) {
        if (drop) atomicAdd(&ctr[0], (unsigned)__popcll(drop));
        if (add) atomicAdd(msum, add);
    }
}

// updaters list their id; the first-record lanes put cfirst and ccnt back to their identities.  k_vmap_commit without the
// record: cval and the stored sigma stay as they are for k_vimp_write
__global__ __launch_bounds__(BLOCK) void k_vimp_commit(VmapTable tb, VmapRecords rec, const unsigned* __restrict__ where,
                                                       unsigned first_created, long long R, long long tile0,
                                                       const unsigned* __restrict__ off_upd,
                                                       const unsigned long long* __restrict__ blk_upd,
                                                       unsigned* __restrict__ updated_ids)
{
    __shared__ unsigned wcnt[EXT_PER][EXT_WAVES];
    const long long tile = tile0 + blockIdx.x;
    const long long base = tile * EXT_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned w[EXT_PER], below[EXT_PER], id[EXT_PER];
    bool upd[EXT_PER], first[EXT_PER];
#pragma unroll
    for (int k = 0; k < EXT_PER; k++) {
        const long long r = base + k * BLOCK + threadIdx.x;
        w[k] = VOX_NONE;
        if (r < R) w[k] = where[r];
        upd[k] = first[k] = false;
        id[k] = VMAP_NOID;
        if (w[k] != VOX_NONE) {
            const unsigned long long v = tb.cval[w[k]];
            first[k] = tb.cfirst[w[k]] == (unsigned)r;
            if ((unsigned)v == (unsigned)r) {  // the call's winner of its voxel
                id[k] = tb.id[w[k]];
                upd[k] = id[k] < first_created && (unsigned)(v >> 32) < f2key(rec.rho_sigma[id[k]].y);
            }
        }
        const unsigned long long m = __ballot(upd[k]);
        below[k] = ext_lanes_below(m);
        if (lane == 0) wcnt[k][wave] = (unsigned)__popcll(m);
    }
    __syncthreads();
    unsigned long long pos = ext_tile_offset(off_upd, blk_upd, tile);
#pragma unroll
    for (int k = 0; k < EXT_PER; k++) {
        unsigned lower = 0, round = 0;
#pragma unroll
        for (int v = 0; v < EXT_WAVES; v++) {
            const unsigned c = wcnt[k][v];
            if (v < wave) lower += c;
            round += c;
        }
        if (upd[k] && updated_ids) updated_ids[pos + lower + below[k]] = id[k];
        if (first[k]) {
            tb.cfirst[w[k]] = ~0u;
            tb.ccnt[w[k]] = 0u;
        }
        pos += round;
    }
}

// one lane per source record r0 + thread (a later launch than k_vimp_commit): every record learns its entry; the call's
// winner of a new or beaten voxel -- the one lane that touches record id -- writes the record from the sources and puts
// cval back to its identity.  src_epoch (sdm_vmap_repose: the records move, their history stays) replaces the call's epoch
// by the source record's
__global__ __launch_bounds__(BLOCK) void k_vimp_write(VmapTable tb, VmapRecords rec, const unsigned* __restrict__ where,
                                                      unsigned first_created, unsigned epoch, long long R, long long r0,
                                                      VimpSrc src, unsigned* __restrict__ dst_ids,
                                                      const unsigned* __restrict__ src_epoch)
{
    const long long r = r0 + (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= R) return;
    const unsigned w = where[r];
    if (w == VOX_NONE) {
        if (dst_ids) dst_ids[r] = VMAP_NOID;
        return;
    }
    const unsigned e = tb.id[w];
    if (dst_ids) dst_ids[r] = e;
    const unsigned long long v = tb.cval[w];
    if ((unsigned)v != (unsigned)r) return;  // (the identity names no record: its low word is 2^32 - 1)
    tb.cval[w] = ~0ull;
    if (e < first_created && !((unsigned)(v >> 32) < f2key(rec.rho_sigma[e].y))) return;
    rec.xyz[(size_t)e * 3 + 0] = src.xyz[r * 3 + 0];
    rec.xyz[(size_t)e * 3 + 1] = src.xyz[r * 3 + 1];
    rec.xyz[(size_t)e * 3 + 2] = src.xyz[r * 3 + 2];
    rec.pixel[e] = src.pixel ? src.pixel[r] : 0u;
    rec.rho_sigma[e] = src.rho_sigma[r];
    rec.intensity[e] = src.intensity ? src.intensity[r] : (unsigned char)0;
    rec.tag[e] = src.tag ? src.tag[r] : 0;
    rec.epoch[e] = src_epoch ? src_epoch[r] : epoch;
}

// pairs k0 + thread; ctr = {rejected pairs, stored or found pairs, overflow} (k_vobs_totals' layout).  skip
// (sdm_vmap_retire: the pairs that leave the log) rejects pair k where skip[k] != 0
__global__ __launch_bounds__(BLOCK) void k_vobs_import_insert(const unsigned* __restrict__ entry, const int* __restrict__ tag,
                                                              const unsigned* __restrict__ entry_map, long long map_count,
                                                              long long P, long long k0, unsigned M, VobsTable ot,
                                                              unsigned* __restrict__ where, unsigned long long* __restrict__ ctr,
                                                              const unsigned char* __restrict__ skip)
{
    const long long k = k0 + (long long)blockIdx.x * BLOCK + threadIdx.x;
    bool rejected = false, cand = false;
    if (k < P) {
        unsigned id = entry[k];
        if (entry_map) id = (long long)id < map_count ? entry_map[id] : VMAP_NOID;
        if (skip && skip[k]) id = VMAP_NOID;
        const int t = tag[k];
        unsigned w = VOX_NONE;
        if (id >= M || t < 0) {
            rejected = true;
        } else {
            cand = true;
            unsigned long long h;
            if (vobs_claim(ot, ((unsigned long long)id << 32) | (unsigned long long)(unsigned)t, h)) {
                atomicMin(&ot.ord[h], (unsigned long long)k);
                w = (unsigned)h;
            } else {
                atomicOr(&ctr[2], 1ull);
            }
        }
        where[k] = w;
    }
    const unsigned long long rm = __ballot(rejected), cm = __ballot(cand);  // (every lane of the wave arrives here)
    if ((threadIdx.x & 63) == 0) {
        if (rm) atomicAdd(&ctr[0], (unsigned long long)__popcll(rm));
        if (cm) atomicAdd(&ctr[1], (unsigned long long)__popcll(cm));
    }
}

}  // namespace sdm
