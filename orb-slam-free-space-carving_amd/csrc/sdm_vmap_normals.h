// sdm_vmap_normals.h -- per-entry surface normals and surface variation of the persistent voxel map (sdm_vmap_normals;
// included by sdm_engine.hip).  For every entry of a range: the plane through the stored points of the member entries in the
// (2r+1)^3 cells around it, by the covariance of those points and a cyclic Jacobi eigen-solve of a fixed number of sweeps.
// The table, the records and the flags are only read, and the call keeps no per-entry state.
//
// One sdm_vmap_normals over the entries id = first .. first + count - 1 (the host has formed the camera centre of every
// pose, sorted the table by tag and uploaded it once, 20 B per pose):
//   k_vmap_normals<R>  one lane per entry.  The member test (k_vcomp_init's), the cell from the record as vcls_neighbours
//                      forms it, then the (2R+1)^3 offsets in lexicographic order: vcls_neighbours' range test, the
//                      read-only vmap_find, and on a hit 4 B of multiplicity (+ 1 B of flag) and 12 B of xyz.  Nine running
//                      sums (s_a, m_ab) in visiting order; the covariance; 6 sweeps of three rotations, unrolled, the state
//                      (six of A, nine of V) in registers; the smallest eigenvalue's column; k_vmap_recarve's binary search
//                      of the record's tag and the flip towards the camera centre.  The wave then counts its four totals by
//                      ballot and popcount and lane 0 issues one 64-bit atomic per non-zero total.
//
// The arithmetic is normative (sdm_c.h): IEEE binary32, every product rounded before its add (the library is built without
// FMA contraction), the correctly rounded division and sqrtf, denormals kept.  No operation here may be reordered, fused or
// replaced by a reciprocal: tests/vmap_normals_np.py restates each and the outputs are compared bit for bit.
//
// Reproducibility: an entry's sums are accumulated by its own lane in the order of the cells, not of the table; the totals
// are sums of ones.  Loops are bounded by (2R+1)^3, the table capacity and log2 of the pose table; every lane reaches the
// ballots; no lane waits for another; no LDS and no atomics in the estimate.  Plain C++ and vector stores only.
#pragma once
#include "sdm_vmap_comp.h"

namespace sdm {

constexpr int VNRM_SWEEPS = 6;

struct VmapNormalsIn {
    const float* xyz;                // [M][3] the records' xyz
    const unsigned* multiplicity;    // [M]
    const int* rec_tag;              // [M] the winner's tag
    const unsigned char* published;  // [M] or null (every flag reads 0)
    const int* tags;                 // [n] the pose table's tags, ascending
    const float* origin;             // [n][4] their camera centres (the fourth value pads)
    long long first, count;          // the range of entries
    int n;
    unsigned M;                      // entries of the map
    float inv;
    unsigned min_points, min_multiplicity;
    int require_published;
};

__device__ __forceinline__ bool vnrm_member(const VmapNormalsIn& in, unsigned id)
{
    return in.multiplicity[id] >= in.min_multiplicity && (!in.require_published || (in.published && in.published[id] != 0));
}

// one rotation of the pair (p, q) with r the third index: app, aqq, apq the pair's entries of A, arp and arq the third
// row's, v0p .. v2q the two columns of V
__device__ __forceinline__ void vnrm_rotate(float& app, float& aqq, float& apq, float& arp, float& arq, float& v0p, float& v0q,
                                            float& v1p, float& v1q, float& v2p, float& v2q)
{
    if (apq == 0.f) return;  // (-0 too)
    const float theta = (aqq - app) / (2.f * apq);
    const float t = copysignf(1.f, theta) / (fabsf(theta) + sqrtf(theta * theta + 1.f));
    const float c = 1.f / sqrtf(t * t + 1.f);
    const float s = t * c;
    const float h = t * apq;
    app = app - h;
    aqq = aqq + h;
    apq = 0.f;
    float x = arp, y = arq;
    arp = c * x - s * y;
    arq = s * x + c * y;
    x = v0p, y = v0q;
    v0p = c * x - s * y;
    v0q = s * x + c * y;
    x = v1p, y = v1q;
    v1p = c * x - s * y;
    v1q = s * x + c * y;
    x = v2p, y = v2q;
    v2p = c * x - s * y;
    v2q = s * x + c * y;
}

// entries first + e0 + thread of the slice; totals += {entries, members, estimated, oriented}.  Any destination may be null;
// they are indexed by id - first.
template <int R>
__global__ __launch_bounds__(BLOCK) void k_vmap_normals(VmapNormalsIn in, long long e0, VmapTable tb, float* __restrict__ normal,
                                                        float* __restrict__ variation, unsigned* __restrict__ points,
                                                        unsigned long long* __restrict__ totals)
{
    const long long e = e0 + (long long)blockIdx.x * BLOCK + threadIdx.x;
    const bool entry = e < in.count;
    bool member = false, estimated = false, oriented = false;
    unsigned k = 0;
    float n0 = 0.f, n1 = 0.f, n2 = 0.f, var = -1.f;
    if (entry) {
        const unsigned id = (unsigned)(in.first + e);  // (below M: the host has checked the range)
        member = vnrm_member(in, id);
        if (member) {
            const float px = in.xyz[(size_t)id * 3 + 0], py = in.xyz[(size_t)id * 3 + 1], pz = in.xyz[(size_t)id * 3 + 2];
            const int cx = (int)floorf(px * in.inv), cy = (int)floorf(py * in.inv), cz = (int)floorf(pz * in.inv);  // (in range)
            const int lim = 1 << 20;
            float s0 = 0.f, s1 = 0.f, s2 = 0.f, m00 = 0.f, m01 = 0.f, m02 = 0.f, m11 = 0.f, m12 = 0.f, m22 = 0.f;
#pragma unroll 1
            for (int dx = -R; dx <= R; dx++) {
                const int nx = cx + dx;
                if (nx < -lim || nx >= lim) continue;  // holds nothing; no key
#pragma unroll 1
                for (int dy = -R; dy <= R; dy++) {
                    const int ny = cy + dy;
                    if (ny < -lim || ny >= lim) continue;
#pragma unroll 1
                    for (int dz = -R; dz <= R; dz++) {
                        const int nz = cz + dz;
                        if (nz < -lim || nz >= lim) continue;
                        const unsigned j = vmap_find(tb, vmap_cell_key(nx, ny, nz));
                        if (!(j < in.M) || !vnrm_member(in, j)) continue;  // (VMAP_NOID is not below M)
                        const float q0 = (in.xyz[(size_t)j * 3 + 0] - px) * in.inv, q1 = (in.xyz[(size_t)j * 3 + 1] - py) * in.inv,
                                    q2 = (in.xyz[(size_t)j * 3 + 2] - pz) * in.inv;
                        k += 1;
                        s0 = s0 + q0, s1 = s1 + q1, s2 = s2 + q2;
                        m00 = m00 + q0 * q0, m01 = m01 + q0 * q1, m02 = m02 + q0 * q2;
                        m11 = m11 + q1 * q1, m12 = m12 + q1 * q2, m22 = m22 + q2 * q2;
                    }
                }
            }
            if (k >= in.min_points) {
                const float kf = (float)k;
                const float mu0 = s0 / kf, mu1 = s1 / kf, mu2 = s2 / kf;
                float a00 = m00 / kf - mu0 * mu0, a01 = m01 / kf - mu0 * mu1, a02 = m02 / kf - mu0 * mu2;
                float a11 = m11 / kf - mu1 * mu1, a12 = m12 / kf - mu1 * mu2, a22 = m22 / kf - mu2 * mu2;
                float v00 = 1.f, v01 = 0.f, v02 = 0.f, v10 = 0.f, v11 = 1.f, v12 = 0.f, v20 = 0.f, v21 = 0.f, v22 = 1.f;
#pragma unroll
                for (int sweep = 0; sweep < VNRM_SWEEPS; sweep++) {
                    vnrm_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);  // (0, 1), r = 2
                    vnrm_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);  // (0, 2), r = 1
                    vnrm_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);  // (1, 2), r = 0
                }
                int m = 0;
                float lm = a00;
                if (a11 < lm) m = 1, lm = a11;
                if (a22 < lm) m = 2, lm = a22;
                const float sum = (a00 + a11) + a22;
                if (sum > 0.f) {
                    estimated = true;
                    n0 = m == 0 ? v00 : m == 1 ? v01 : v02;
                    n1 = m == 0 ? v10 : m == 1 ? v11 : v12;
                    n2 = m == 0 ? v20 : m == 1 ? v21 : v22;
                    var = (lm < 0.f ? 0.f : lm) / sum;
                    const int t = in.rec_tag[id];
                    int lo = 0, hi = in.n;  // the first table position whose tag is not below t
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (in.tags[mid] < t) lo = mid + 1;
                        else hi = mid;
                    }
                    oriented = lo < in.n && in.tags[lo] == t;
                    if (oriented) {
                        const float d0 = in.origin[lo * 4 + 0] - px, d1 = in.origin[lo * 4 + 1] - py, d2 = in.origin[lo * 4 + 2] - pz;
                        const float dot = (n0 * d0 + n1 * d1) + n2 * d2;
                        if (dot < 0.f) n0 = -n0, n1 = -n1, n2 = -n2;  // (a NaN does not flip)
                    }
                }
            }
        }
        if (normal) normal[e * 3 + 0] = n0, normal[e * 3 + 1] = n1, normal[e * 3 + 2] = n2;
        if (variation) variation[e] = var;
        if (points) points[e] = k;
    }
    // the call totals: one atomic per wave and total (every lane of the wave arrives here)
    const unsigned long long en = __ballot(entry), mb = __ballot(member), es = __ballot(estimated), orr = __ballot(oriented);
    if ((threadIdx.x & 63) == 0) {
        if (en) atomicAdd(&totals[0], (unsigned long long)__popcll(en));
        if (mb) atomicAdd(&totals[1], (unsigned long long)__popcll(mb));
        if (es) atomicAdd(&totals[2], (unsigned long long)__popcll(es));
        if (orr) atomicAdd(&totals[3], (unsigned long long)__popcll(orr));
    }
}

}  // namespace sdm
