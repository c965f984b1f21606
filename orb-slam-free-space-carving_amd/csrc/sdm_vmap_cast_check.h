// sdm_vmap_cast_check.h -- the argument checks of sdm_vmap_cast_segments and sdm_vmap_render, in the order of sdm_c.h.  No
// HIP and no context: tools/vmap_cast_check.cc drives them under the host sanitizers.  A refusal returns its code and leaves
// the words for sdm_last_error in *why.  No pointer is dereferenced but args.
#pragma once
#include <stdint.h>

#include <string>

#include "sdm_c.h"

namespace sdm {

constexpr long long VMAP_CAST_MAX_RAYS = 1ll << 30;

// what both calls check alike once the number of rays is known: the destinations (hit_rho counts for the render only), the
// capacity, the alignment of device pointers, the margins, max_steps and the filter
inline int cast_check_common(long long n, const sdm_vmap_cast_args* a, bool render, std::string* why)
{
    const auto refuse = [why](const char* words) {
        *why = words;
        return SDM_EINVAL;
    };
    if (!a->hit_id && !a->hit_step && !(render && a->hit_rho)) return refuse("no output requested");
    if (a->capacity < n) return refuse(render ? "capacity below W * H" : "capacity below n");
    if (a->on_device && ((uintptr_t)a->hit_id | (uintptr_t)a->hit_step | (render ? (uintptr_t)a->hit_rho : 0)) % 4)
        return refuse("device buffer not aligned (hit_id, hit_step, hit_rho: 4 B)");
    if (a->start_margin < 0 || a->end_margin < 0) return refuse("negative start_margin or end_margin");
    if (a->max_steps < 1 || a->max_steps > SDM_FREESPACE_MAX_STEPS) return refuse("max_steps outside 1 .. SDM_FREESPACE_MAX_STEPS");
    if (a->require_published != 0 && a->require_published != 1) return refuse("require_published must be 0 or 1");
    return SDM_OK;
}

// sdm_vmap_cast_segments.  map_open: the context has an open voxel map.
inline int cast_segments_check(bool map_open, long long n, const float* origins, const float* ends, const sdm_vmap_cast_args* a,
                               std::string* why)
{
    const auto refuse = [why](int code, const char* words) {
        *why = words;
        return code;
    };
    if (!a) return refuse(SDM_EINVAL, "null argument");
    if (!map_open) return refuse(SDM_ESTATE, "no open voxel map");
    if (n < 0 || n > VMAP_CAST_MAX_RAYS) return refuse(SDM_EINVAL, "n outside 0 .. 2^30");
    if (n > 0 && (!origins || !ends)) return refuse(SDM_EINVAL, "null origins or ends");
    if (a->on_device && ((uintptr_t)origins | (uintptr_t)ends) % 4) return refuse(SDM_EINVAL, "device buffer not aligned (origins, ends: 4 B)");
    return cast_check_common(n, a, false, why);
}

// sdm_vmap_render.  On success *n = W * H.
inline int render_check(bool map_open, const float* K, const float* Tcw, int W, int H, float rho_far, const sdm_vmap_cast_args* a,
                        long long* n, std::string* why)
{
    const auto refuse = [why](int code, const char* words) {
        *why = words;
        return code;
    };
    *n = 0;
    if (!a) return refuse(SDM_EINVAL, "null argument");
    if (!map_open) return refuse(SDM_ESTATE, "no open voxel map");
    if (W < 1 || W > 65535 || H < 1 || H > 65535) return refuse(SDM_EINVAL, "W or H outside 1 .. 65535");
    const long long rays = (long long)W * H;
    if (rays > VMAP_CAST_MAX_RAYS) return refuse(SDM_EINVAL, "W * H above 2^30");
    if (!K || !Tcw) return refuse(SDM_EINVAL, "null K or Tcw");
    const int rc = cast_check_common(rays, a, true, why);
    if (rc) return rc;
    if (!((double)rho_far >= 0.000001)) return refuse(SDM_EINVAL, "rho_far is NaN or below 1e-6");  // (lt_1em6's compare)
    *n = rays;
    return SDM_OK;
}

}  // namespace sdm
