// sdm_vmap_normals_check.h -- the argument checks of sdm_vmap_normals, in the order of sdm_c.h.  No HIP and no context:
// tools/vmap_normals_check.cc drives them under the host sanitizers.  A refusal returns its code and leaves the words for
// sdm_last_error in *why.  No pointer is dereferenced but args and, by the pose table's own checks, tags[0 .. n_poses).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "sdm_c.h"
#include "sdm_vmap_poses.h"

namespace sdm {

// the cells a member visits: 0 for a radius the call refuses
inline unsigned normals_cells(int radius) { return radius == 1 ? 27u : radius == 2 ? 125u : 0u; }

// the four outs of a refusal (and of a call before its counts are known)
inline void normals_clear_outs(sdm_vmap_normal_args* a) { a->entries = a->members = a->estimated = a->oriented = 0; }

// sdm_vmap_normals.  map_open: the context has an open voxel map; M: its entries.  On success *count is the size of the
// range (a->count == -1 resolved) and *order the pose table's rows by ascending tag.
inline int normals_check(bool map_open, long long M, int n_poses, const int* tags, const float* Tcw, const sdm_vmap_normal_args* a,
                         long long* count, std::vector<int>* order, std::string* why)
{
    const auto refuse = [why](int code, const char* words) {
        *why = words;
        return code;
    };
    if (!a) return refuse(SDM_EINVAL, "null argument");
    if (!map_open) return refuse(SDM_ESTATE, "no open voxel map");
    const unsigned cells = normals_cells(a->radius);
    if (!cells) return refuse(SDM_EINVAL, "radius must be 1 or 2");
    if (a->min_points < 3u || a->min_points > cells) return refuse(SDM_EINVAL, "min_points outside 3 .. (2*radius+1)^3");
    if (a->require_published != 0 && a->require_published != 1) return refuse(SDM_EINVAL, "require_published must be 0 or 1");
    if (a->first < 0 || a->count < -1 || a->first > M || a->count > M - a->first)
        return refuse(SDM_EINVAL, "range beyond the map's entries (first >= 0, count >= -1, first + count <= M)");
    const long long n = a->count == -1 ? M - a->first : a->count;
    if (a->capacity < 0) return refuse(SDM_EINVAL, "negative capacity");
    if ((a->normal || a->variation || a->points) && a->capacity < n) return refuse(SDM_EINVAL, "capacity below the range");
    if (a->on_device && ((uintptr_t)a->normal | (uintptr_t)a->variation | (uintptr_t)a->points) % 4)
        return refuse(SDM_EINVAL, "device buffer not aligned (normal, variation, points: 4 B)");
    if (n_poses < 0) return refuse(SDM_EINVAL, "negative n_poses");
    if (n_poses > 0 && (!tags || !Tcw)) return refuse(SDM_EINVAL, "null pose table (tags and Tcw are required)");
    const int rc = pose_table_order(n_poses, tags, order, why);
    if (rc) return rc;
    *count = n;
    return SDM_OK;
}

}  // namespace sdm
