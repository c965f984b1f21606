// sdm_vmap_mesh.h -- a triangle mesh of the persistent voxel map's entries (sdm_vmap_mesh; included by sdm_engine.hip).  Every
// owner -- a member at the bottom of its run of members along the dominant axis of its normal -- stitches the local height
// field over its own cell: itself, its neighbour column along u, along v, and the diagonal one.  The triangles are entry ids.
// The table, the records, the flags and the caller's normals are only read, and the call keeps no per-entry state.
//
// Scratch per call: corner[count][3] u32 and ntri[count] u8 (13 B per entry of the range), used[M] u8, the tile scan's arrays.
// One sdm_vmap_mesh over the entries id = first .. first + count - 1 (used[] has been zeroed):
//   k_vmesh_find      one lane per entry.  The member test (k_vcomp_init's), the axis of the normal by comparisons alone, the
//                     cell from the record as vcls_neighbours forms it, the probe below (the owner test), then the four steps
//                     Nu, Nv, C by Nu and C by Nv: each at most three probes for the column's member and two for its run's
//                     bottom -- 21 read-only vmap_find at the most.  It leaves the three corner ids and the triangle count
//                     (bit 2: the winding is flipped) in the scratch, so no later pass probes; an owner with a triangle sets
//                     used[] of its corners: plain byte stores of the value 1, which any number of lanes may repeat.  The
//                     wave counts entries, members, owners, quads and singles by ballot and popcount and lane 0 issues one
//                     64-bit atomic per non-zero total.
//   k_vmesh_count     tiles of EXT_TILE entries of the range: the triangles of a tile (at most 2 * EXT_TILE) by two ballots
//   k_extract_scan_tiles / k_extract_scan_sums   (sdm_extract.h, unchanged) scan the tile counts
//   k_vmesh_vertices  one lane per byte of used[]: the ones, by ballot and popcount
//   k_vmesh_totals    `triangles` for the host's first wait
//   k_vmesh_write     (queued only if the call is not refused) owner_tris, and the index triples at the rank from the scan
//                     over id, so the list is in owner order without a sort
//
// Reproducibility: every output is an integer decided by comparisons; the totals are sums of ones.  Loops are bounded by the
// table capacity and by constants; every lane reaches every ballot; no lane waits for another; the only LDS is the tile
// kernels' wave counts.  Plain C++ and vector stores only.
#pragma once
#include "sdm_vmap_normals.h"

namespace sdm {

struct VmapMeshIn {
    const float* xyz;                // [M][3] the records' xyz
    const unsigned* multiplicity;    // [M]
    const unsigned char* published;  // [M] or null (every flag reads 0)
    const float* normal;             // [count][3] the caller's normals, indexed by id - first
    long long first, count;          // the range of entries
    unsigned M;                      // entries of the map
    float inv;
    unsigned min_multiplicity;
    int require_published;
};

__device__ __forceinline__ bool vmesh_is_member(const VmapMeshIn& in, unsigned id)
{
    return in.multiplicity[id] >= in.min_multiplicity && (!in.require_published || (in.published && in.published[id] != 0));
}

// the cell moved by d along `axis` (selects: no indexed array of registers)
__device__ __forceinline__ void vmesh_move(int& x, int& y, int& z, int axis, int d)
{
    x += axis == 0 ? d : 0;
    y += axis == 1 ? d : 0;
    z += axis == 2 ? d : 0;
}

// the member of a cell, or VMAP_NOID: vcls_neighbours' range test before the key is formed, then one read-only probe
__device__ __forceinline__ unsigned vmesh_at(const VmapMeshIn& in, const VmapTable& tb, int x, int y, int z)
{
    const int lim = 1 << 20;
    if (x < -lim || x >= lim || y < -lim || y >= lim || z < -lim || z >= lim) return VMAP_NOID;  // holds nothing; no key
    const unsigned j = vmap_find(tb, vmap_cell_key(x, y, z));
    return (j < in.M && vmesh_is_member(in, j)) ? j : VMAP_NOID;  // (VMAP_NOID is not below M)
}

// step(j, ax) in the frame of axis a: (x, y, z) is the cell of j on entry and, on a hit, the cell of the entry returned
__device__ __forceinline__ unsigned vmesh_step(const VmapMeshIn& in, const VmapTable& tb, int& x, int& y, int& z, int ax, int a)
{
    vmesh_move(x, y, z, ax, 1);
    unsigned k = VMAP_NOID;
#pragma unroll 1
    for (int i = 0; i < 3 && k == VMAP_NOID; i++) {  // da = 0, -1, +1
        const int da = i == 0 ? 0 : i == 1 ? -1 : 1;
        int tx = x, ty = y, tz = z;
        vmesh_move(tx, ty, tz, a, da);
        k = vmesh_at(in, tb, tx, ty, tz);
        if (k != VMAP_NOID) x = tx, y = ty, z = tz;
    }
    if (k == VMAP_NOID) return k;
#pragma unroll 1
    for (int r = 0; r < 2; r++) {  // down its run, at most twice
        int tx = x, ty = y, tz = z;
        vmesh_move(tx, ty, tz, a, -1);
        const unsigned b = vmesh_at(in, tb, tx, ty, tz);
        if (b == VMAP_NOID) break;
        k = b, x = tx, y = ty, z = tz;
    }
    return k;
}

// entries first + e0 + thread of the slice; totals += {entries, members, owners, quads, singles}.  corner and ntri are
// indexed by id - first, used by id.
__global__ __launch_bounds__(BLOCK) void k_vmesh_find(VmapMeshIn in, long long e0, VmapTable tb, unsigned* __restrict__ corner,
                                                      unsigned char* __restrict__ ntri, unsigned char* __restrict__ used,
                                                      unsigned long long* __restrict__ totals)
{
    const long long e = e0 + (long long)blockIdx.x * BLOCK + threadIdx.x;
    const bool entry = e < in.count;
    bool member = false, owner = false;
    unsigned nu = VMAP_NOID, nv = VMAP_NOID, cc = VMAP_NOID, nt = 0, flip = 0;
    if (entry) {
        const unsigned id = (unsigned)(in.first + e);  // (below M: the host has checked the range)
        member = vmesh_is_member(in, id);
        if (member) {
            const float n0 = in.normal[e * 3 + 0], n1 = in.normal[e * 3 + 1], n2 = in.normal[e * 3 + 2];
            int a = 0;
            float na = n0;
            if (fabsf(n1) > fabsf(na)) a = 1, na = n1;  // (a NaN never wins; ties go to the lower index)
            if (fabsf(n2) > fabsf(na)) a = 2, na = n2;
            if (fabsf(na) > 0.f) {  // (false for a NaN; a denormal is > 0)
                const int u = a == 2 ? 0 : a + 1, v = a == 0 ? 2 : a - 1;  // (a + 1) mod 3, (a + 2) mod 3
                const int cx = (int)floorf(in.xyz[(size_t)id * 3 + 0] * in.inv), cy = (int)floorf(in.xyz[(size_t)id * 3 + 1] * in.inv),
                          cz = (int)floorf(in.xyz[(size_t)id * 3 + 2] * in.inv);  // (in range: the entry exists)
                int bx = cx, by = cy, bz = cz;
                vmesh_move(bx, by, bz, a, -1);
                owner = vmesh_at(in, tb, bx, by, bz) == VMAP_NOID;  // the bottom of its run
                if (owner) {
                    int ux = cx, uy = cy, uz = cz, vx = cx, vy = cy, vz = cz;
                    nu = vmesh_step(in, tb, ux, uy, uz, u, a);
                    nv = vmesh_step(in, tb, vx, vy, vz, v, a);
                    if (nu != VMAP_NOID) cc = vmesh_step(in, tb, ux, uy, uz, v, a);
                    if (cc == VMAP_NOID && nv != VMAP_NOID) cc = vmesh_step(in, tb, vx, vy, vz, u, a);
                    const int have = (nu != VMAP_NOID) + (nv != VMAP_NOID) + (cc != VMAP_NOID);
                    nt = have == 3 ? 2u : have == 2 ? 1u : 0u;
                    flip = na < 0.f ? 1u : 0u;
                    if (nt) {
                        used[id] = 1;
                        if (nu != VMAP_NOID) used[nu] = 1;
                        if (nv != VMAP_NOID) used[nv] = 1;
                        if (cc != VMAP_NOID) used[cc] = 1;
                    }
                }
            }
        }
        corner[e * 3 + 0] = nu, corner[e * 3 + 1] = nv, corner[e * 3 + 2] = cc;
        ntri[e] = (unsigned char)(nt | (flip << 2));
    }
    // the call totals: one atomic per wave and total (every lane of the wave arrives here)
    const unsigned long long en = __ballot(entry), mb = __ballot(member), ow = __ballot(owner), qd = __ballot(nt == 2u),
                             sg = __ballot(nt == 1u);
    if ((threadIdx.x & 63) == 0) {
        if (en) atomicAdd(&totals[0], (unsigned long long)__popcll(en));
        if (mb) atomicAdd(&totals[1], (unsigned long long)__popcll(mb));
        if (ow) atomicAdd(&totals[2], (unsigned long long)__popcll(ow));
        if (qd) atomicAdd(&totals[3], (unsigned long long)__popcll(qd));
        if (sg) atomicAdd(&totals[4], (unsigned long long)__popcll(sg));
    }
}

// one workgroup per tile tile0 + block of EXT_TILE consecutive entries of the range: cnt[tile] = its triangles
__global__ __launch_bounds__(BLOCK) void k_vmesh_count(const unsigned char* __restrict__ ntri, long long count, long long tile0,
                                                       unsigned* __restrict__ cnt)
{
    __shared__ unsigned wsum[EXT_WAVES];
    const long long tile = tile0 + blockIdx.x;
    const long long base = tile * EXT_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned mine = 0;
#pragma unroll 1
    for (int k = 0; k < EXT_PER; k++) {
        const long long e = base + k * BLOCK + threadIdx.x;
        const unsigned n = e < count ? (ntri[e] & 3u) : 0u;
        mine += (unsigned)(__popcll(__ballot(n >= 1u)) + __popcll(__ballot(n == 2u)));  // (every lane of the wave arrives here)
    }
    if (lane == 0) wsum[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = 0;
        for (int w = 0; w < EXT_WAVES; w++) t += wsum[w];
        cnt[tile] = t;
    }
}

// one lane per byte j0 + thread of used[M]; totals[6] += the ones
__global__ __launch_bounds__(BLOCK) void k_vmesh_vertices(const unsigned char* __restrict__ used, long long M, long long j0,
                                                          unsigned long long* __restrict__ totals)
{
    const long long j = j0 + (long long)blockIdx.x * BLOCK + threadIdx.x;
    const unsigned long long m = __ballot(j < M && used[j] != 0);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(&totals[6], (unsigned long long)__popcll(m));
}

// totals[5] = the triangles
__global__ void k_vmesh_totals(long long nt, const unsigned* __restrict__ off, const unsigned long long* __restrict__ blk,
                               unsigned long long* __restrict__ totals)
{
    if (blockIdx.x || threadIdx.x) return;
    totals[5] = ext_tile_offset(off, blk, nt);
}

// every entry of the range writes its count, the owners their triangles at their rank.  Either destination may be null.
__global__ __launch_bounds__(BLOCK) void k_vmesh_write(const unsigned* __restrict__ corner, const unsigned char* __restrict__ ntri,
                                                       long long first, long long count, long long tile0,
                                                       const unsigned* __restrict__ off, const unsigned long long* __restrict__ blk,
                                                       unsigned* __restrict__ tri, unsigned char* __restrict__ owner_tris)
{
    __shared__ unsigned wcnt[EXT_PER][EXT_WAVES];
    const long long tile = tile0 + blockIdx.x;
    const long long base = tile * EXT_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned code[EXT_PER], below[EXT_PER];
#pragma unroll
    for (int k = 0; k < EXT_PER; k++) {
        const long long e = base + k * BLOCK + threadIdx.x;
        code[k] = 0;
        if (e < count) {
            code[k] = ntri[e];
            if (owner_tris) owner_tris[e] = (unsigned char)(code[k] & 3u);
        }
        const unsigned n = code[k] & 3u;
        const unsigned long long m1 = __ballot(n >= 1u), m2 = __ballot(n == 2u);  // (every lane of the wave arrives here)
        below[k] = ext_lanes_below(m1) + ext_lanes_below(m2);
        if (lane == 0) wcnt[k][wave] = (unsigned)(__popcll(m1) + __popcll(m2));
    }
    __syncthreads();
    if (!tri) return;
    unsigned long long pos = ext_tile_offset(off, blk, tile);
#pragma unroll
    for (int k = 0; k < EXT_PER; k++) {
        unsigned lower = 0, round = 0;
#pragma unroll
        for (int w = 0; w < EXT_WAVES; w++) {
            const unsigned c = wcnt[k][w];
            if (w < wave) lower += c;
            round += c;
        }
        const unsigned n = code[k] & 3u;
        if (n) {
            const long long e = base + k * BLOCK + threadIdx.x;
            const unsigned id = (unsigned)(first + e);
            const unsigned nu = corner[e * 3 + 0], nv = corner[e * 3 + 1], cc = corner[e * 3 + 2];
            const bool flip = (code[k] & 4u) != 0;
            // (id, Nu, C), (id, C, Nv) for a quad; the one of (id, Nu, Nv), (id, Nu, C), (id, C, Nv) otherwise
            unsigned p1, p2;
            if (n == 2u || nv == VMAP_NOID) p1 = nu, p2 = cc;
            else if (cc == VMAP_NOID) p1 = nu, p2 = nv;
            else p1 = cc, p2 = nv;
            unsigned* t = tri + (pos + lower + below[k]) * 3;
            t[0] = id, t[1] = flip ? p2 : p1, t[2] = flip ? p1 : p2;
            if (n == 2u) t[3] = id, t[4] = flip ? nv : cc, t[5] = flip ? cc : nv;
        }
        pos += round;
    }
}

}  // namespace sdm
