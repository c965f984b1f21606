// sdm_vmap_comp_check.h -- the argument checks of sdm_vmap_components, in the order of sdm_c.h.  No HIP and no context:
// tools/vmap_comp_check.cc drives them under the host sanitizers.  A refusal returns its code and leaves the words for
// sdm_last_error in *why.  No pointer is dereferenced but args.
#pragma once
#include <stdint.h>

#include <string>

#include "sdm_c.h"

namespace sdm {

// the most offsets a member visits: 0 for a connectivity the call refuses
inline int comp_max_l1(int connectivity) { return connectivity == 6 ? 1 : connectivity == 18 ? 2 : connectivity == 26 ? 3 : 0; }

// the six outs of a refusal (and of a call before its counts are known)
inline void comp_clear_outs(sdm_vmap_comp_args* a)
{
    a->entries = a->members = a->components = a->largest = a->small = a->small_components = 0;
}

// sdm_vmap_components.  map_open: the context has an open voxel map; M: its entries.
inline int comp_check(bool map_open, long long M, const sdm_vmap_comp_args* a, std::string* why)
{
    const auto refuse = [why](int code, const char* words) {
        *why = words;
        return code;
    };
    if (!a) return refuse(SDM_EINVAL, "null argument");
    if (!map_open) return refuse(SDM_ESTATE, "no open voxel map");
    if (!comp_max_l1(a->connectivity)) return refuse(SDM_EINVAL, "connectivity must be 6, 18 or 26");
    if (a->require_published != 0 && a->require_published != 1) return refuse(SDM_EINVAL, "require_published must be 0 or 1");
    if (a->capacity < 0 || a->small_capacity < 0) return refuse(SDM_EINVAL, "negative capacity");
    if ((a->label || a->size) && a->capacity < M) return refuse(SDM_EINVAL, "capacity below the map's entries");
    if (a->on_device && ((uintptr_t)a->label | (uintptr_t)a->size | (uintptr_t)a->small_ids) % 4)
        return refuse(SDM_EINVAL, "device buffer not aligned (label, size, small_ids: 4 B)");
    return SDM_OK;
}

// the capacity refusal, once the counts are known: the list is given and does not hold the small members
inline bool comp_list_too_small(const sdm_vmap_comp_args* a, long long small) { return a->small_ids && small > a->small_capacity; }

}  // namespace sdm
