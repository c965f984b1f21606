// sdm_voxcam.h -- the cameras that saw each kept point of the merged cloud (sdm_extract_points_voxel_cameras, included by
// sdm_engine.hip).
//
// sdm_extract_points_voxel's passes leave every plain point g its kept rank; k_point_support (sdm_support.h, unchanged)
// leaves it a visibility word whose bit j names neighbour j of ITS slot's row.  The host numbers the distinct slots among
// `slots` and `nbr_slots` in ascending order -- camera index c, Cn of them -- so that a kept point's camera set is a
// bitset of Wd = ceil(Cn / 64) words in which ascending bit order is ascending slot id.  Then:
//   k_voxcam_or      one lane per plain point, workgroups cut per slot as for k_point_support (the same block0), so the
//                    slot's own camera index and its row of neighbour camera indices are wave-uniform loads.  The lane
//                    turns its word into camera bits (its own camera always set) and ORs them into its kept point's
//                    bitset with 64-bit atomicOr, word by word, zero words skipped.  The combining form first ORs the
//                    lanes of a wave that form a run of equal rank (a segmented inclusive OR-scan over shuffles); only
//                    the last lane of each run issues the atomic.
//   k_voxcam_count   tiles of EXT_TILE kept points: popcount of the point's Wd words, block sum per tile
//   k_extract_scan_tiles / k_extract_scan_sums / k_extract_offsets   (sdm_extract.h, unchanged) scan the tile counts and
//                    give the total E
//   k_voxcam_write   block-exclusive scan of the tile's counts: cam_offsets[k], then the slot ids of the set bits in
//                    ascending bit order through slot_of_cam; the lane of the last kept point writes cam_offsets[M] = E
//
// Reproducibility: the bitset of a kept point is the integer OR of the camera bits of the plain points it stands for.  OR
// is associative, commutative and idempotent, so neither the arrival order of the atomics nor the grouping the combining
// form chooses (which depends only on which lanes share a wave) can change a bit; counts and positions come from scans.
// Loops are bounded by n_nbr, Wd, 6 shuffle steps or a word's 64 bits; no lane waits for another.  No LDS beyond
// ext_block_scan's.
#pragma once
#include "sdm_support.h"
#include "sdm_voxel.h"

namespace sdm {

struct VoxCamTable {
    const int* slot_of_cam;  // [Cn] ascending slot ids
    const int* own_cam;      // [n] camera index of slots[i]
    const int* nbr_cam;      // [n][n_nbr] camera index of nbr_slots[i][j]
};

// block0 / offsets / support: as k_point_support got and left them; rank[g]: kept rank of plain point g (k_voxel_write +
// k_voxel_rep); bits[M][Wd], cleared by the host
template <bool COMBINE>
__global__ __launch_bounds__(SUP_BLOCK) void k_voxcam_or(const long long* __restrict__ block0, long long block_base, int n,
                                                         int n_nbr, const unsigned long long* __restrict__ offsets,
                                                         const unsigned long long* __restrict__ support,
                                                         const unsigned* __restrict__ rank, VoxCamTable tab, int Wd,
                                                         unsigned long long* __restrict__ bits)
{
    const long long block = block_base + blockIdx.x;
    const int i = sup_find_slot(block0, n, block);
    const unsigned long long p = offsets[i] + (unsigned long long)(block - block0[i]) * SUP_BLOCK + threadIdx.x;
    const bool valid = p < offsets[i + 1];
    if (!COMBINE && !valid) return;
    const unsigned long long word = valid ? support[p] : 0ull;
    const unsigned k = valid ? rank[p] : VOX_NONE;  // (a rank is below M <= T < 2^32 - 1)
    const int own = tab.own_cam[i];
    const int* __restrict__ row = tab.nbr_cam + (long long)i * n_nbr;
    int start = 0;
    bool tail = true;
    const int lane = threadIdx.x & 63;
    if (COMBINE) {  // runs of equal rank among the wave's lanes: start = the run's first lane, tail = its last
        const unsigned up = __shfl_up(k, 1, 64);
        const unsigned long long heads = __ballot(lane == 0 || up != k);
        start = 63 - __clzll(heads & (~0ull >> (63 - lane)));
        tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
    }
    for (int w = 0; w < Wd; w++) {
        unsigned long long m = (valid && (own >> 6) == w) ? 1ull << (own & 63) : 0ull;
        for (int j = 0; j < n_nbr; j++) {
            const int c = row[j];
            if ((c >> 6) == w && ((word >> j) & 1ull)) m |= 1ull << (c & 63);
        }
        if (COMBINE) {
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {  // after the step, m covers lanes [max(start, lane - 2o + 1), lane]
                const unsigned long long u = __shfl_up(m, o, 64);
                if (lane - o >= start) m |= u;
            }
        }
        if (valid && tail && m) atomicOr(&bits[(unsigned long long)k * Wd + w], m);
    }
}

// kept points base + thread * EXT_PER + r, r < EXT_PER, of tile tile0 + block: cnt[r] = cameras of the point (0 past M)
__device__ __forceinline__ unsigned voxcam_counts(const unsigned long long* __restrict__ bits, int Wd, long long M,
                                                  long long k0, unsigned cnt[EXT_PER])
{
    unsigned s = 0;
#pragma unroll
    for (int r = 0; r < EXT_PER; r++) {
        unsigned c = 0;
        if (k0 + r < M)
            for (int w = 0; w < Wd; w++) c += (unsigned)__popcll(bits[(unsigned long long)(k0 + r) * Wd + w]);
        cnt[r] = c;
        s += c;
    }
    return s;
}

__global__ __launch_bounds__(BLOCK) void k_voxcam_count(const unsigned long long* __restrict__ bits, int Wd, long long M,
                                                        long long tile0, unsigned* __restrict__ tile_cnt)
{
    const long long tile = tile0 + blockIdx.x;
    unsigned cnt[EXT_PER], total;
    const unsigned s = voxcam_counts(bits, Wd, M, tile * EXT_TILE + (long long)threadIdx.x * EXT_PER, cnt);
    ext_block_scan<unsigned>(s, &total);
    if (threadIdx.x == 0) tile_cnt[tile] = total;
}

// cam_offsets / cam_slots: either may be null
__global__ __launch_bounds__(BLOCK) void k_voxcam_write(const unsigned long long* __restrict__ bits, int Wd, long long M,
                                                        long long tile0, const unsigned* __restrict__ tile_off,
                                                        const unsigned long long* __restrict__ blk_off,
                                                        const int* __restrict__ slot_of_cam,
                                                        long long* __restrict__ cam_offsets, int* __restrict__ cam_slots)
{
    const long long tile = tile0 + blockIdx.x;
    const long long k0 = tile * EXT_TILE + (long long)threadIdx.x * EXT_PER;
    unsigned cnt[EXT_PER], total;
    const unsigned s = voxcam_counts(bits, Wd, M, k0, cnt);
    unsigned long long o = ext_tile_offset(tile_off, blk_off, tile) + ext_block_scan<unsigned>(s, &total);
#pragma unroll
    for (int r = 0; r < EXT_PER; r++) {
        const long long k = k0 + r;
        if (k >= M) break;
        if (cam_offsets) {
            cam_offsets[k] = (long long)o;
            if (k == M - 1) cam_offsets[M] = (long long)(o + cnt[r]);
        }
        if (cam_slots) {
            unsigned long long e = o;
            for (int w = 0; w < Wd; w++) {
                unsigned long long b = bits[(unsigned long long)k * Wd + w];
                while (b) {  // (at most 64 rounds)
                    cam_slots[e++] = slot_of_cam[w * 64 + __builtin_ctzll(b)];
                    b &= b - 1;
                }
            }
        }
        o += cnt[r];
    }
}

}  // namespace sdm
