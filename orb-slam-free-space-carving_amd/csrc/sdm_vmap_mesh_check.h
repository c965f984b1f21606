// sdm_vmap_mesh_check.h -- the argument checks of sdm_vmap_mesh, in the order of sdm_c.h.  No HIP and no context:
// tools/vmap_mesh_check.cc drives them under the host sanitizers.  A refusal returns its code and leaves the words for
// sdm_last_error in *why.  No pointer is dereferenced but args.
#pragma once
#include <stdint.h>

#include <string>

#include "sdm_c.h"

namespace sdm {

// the seven outs of a refusal (and of a call before its counts are known)
inline void mesh_clear_outs(sdm_vmap_mesh_args* a)
{
    a->entries = a->members = a->owners = a->quads = a->singles = a->triangles = a->vertices = 0;
}

// sdm_vmap_mesh.  map_open: the context has an open voxel map; M: its entries.  On success *count is the size of the range
// (a->count == -1 resolved).
inline int mesh_check(bool map_open, long long M, const sdm_vmap_mesh_args* a, long long* count, std::string* why)
{
    const auto refuse = [why](int code, const char* words) {
        *why = words;
        return code;
    };
    if (!a) return refuse(SDM_EINVAL, "null argument");
    if (!map_open) return refuse(SDM_ESTATE, "no open voxel map");
    if (a->require_published != 0 && a->require_published != 1) return refuse(SDM_EINVAL, "require_published must be 0 or 1");
    if (a->first < 0 || a->count < -1 || a->first > M || a->count > M - a->first)
        return refuse(SDM_EINVAL, "range beyond the map's entries (first >= 0, count >= -1, first + count <= M)");
    const long long n = a->count == -1 ? M - a->first : a->count;
    if (n > 0 && !a->normal) return refuse(SDM_EINVAL, "null normal with a range that is not empty");
    if (a->capacity < 0 || a->tri_capacity < 0 || a->used_capacity < 0) return refuse(SDM_EINVAL, "negative capacity");
    if (a->capacity < n) return refuse(SDM_EINVAL, "capacity below the range (normal and owner_tris hold capacity entries)");
    if (a->vertex_used && a->used_capacity < M) return refuse(SDM_EINVAL, "used_capacity below the map's entries");
    if (a->on_device && ((uintptr_t)a->normal | (uintptr_t)a->tri) % 4)
        return refuse(SDM_EINVAL, "device buffer not aligned (normal, tri: 4 B)");
    *count = n;
    return SDM_OK;
}

// the capacity refusal, once the counts are known: the list is given and does not hold the triangles
inline bool mesh_list_too_small(const sdm_vmap_mesh_args* a, long long triangles) { return a->tri && triangles > a->tri_capacity; }

}  // namespace sdm
