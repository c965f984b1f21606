// sdm_vmap_poses.h -- the host-only steps of sdm_vmap_recarve, which takes a table of keyframe tags and poses: the table's
// order by tag (as sdm_vmap_repose sorts its own), a pose's camera centre, and the call's argument checks.  No HIP and no
// context: tools/vmap_poses_check.cc drives them under the host sanitizers.  A refusal returns its code and leaves the
// words for sdm_last_error in *why.
#pragma once
#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "sdm_c.h"

namespace sdm {

// order[q] = the row of the q-th smallest tag.  Refuses a tag outside [0, 2^31) and a tag listed twice.
inline int pose_table_order(int n, const int* tags, std::vector<int>* order, std::string* why)
{
    const size_t np = (size_t)n;
    try {
        order->resize(np);
    } catch (const std::bad_alloc&) {
        *why = "host allocation for the pose table failed";
        return SDM_EHIP;
    }
    for (size_t p = 0; p < np; p++) {
        if (tags[p] < 0) {
            *why = "tag outside [0, 2^31)";
            return SDM_EINVAL;
        }
        (*order)[p] = (int)p;
    }
    std::sort(order->begin(), order->end(), [tags](int a, int b) { return tags[a] < tags[b]; });
    for (size_t p = 1; p < np; p++)
        if (tags[(*order)[p]] == tags[(*order)[p - 1]]) {
            *why = "tag " + std::to_string(tags[(*order)[p]]) + " listed twice";
            return SDM_EINVAL;
        }
    return SDM_OK;
}

// the camera centre of Tcw[12] as pointset_pixel forms Ow: O = -(Rwc * tcw), Rwc[i][j] = Tcw[j * 4 + i], each row summed
// as (p0 + p1) + p2 (the library is built without FMA contraction)
inline void pose_centre(const float* Tcw, float* O)
{
    const float t0 = Tcw[3], t1 = Tcw[7], t2 = Tcw[11];
    for (int i = 0; i < 3; i++) {
        const float p0 = Tcw[0 * 4 + i] * t0, p1 = Tcw[1 * 4 + i] * t1, p2 = Tcw[2 * 4 + i] * t2;
        O[i] = -((p0 + p1) + p2);
    }
}

// sdm_vmap_recarve's argument checks, in the order of sdm_c.h, against a log of E pairs.  On success *count is the number
// of pairs in the range (rc->count == -1 resolved) and *order the table's rows by ascending tag.
inline int recarve_check(int n_poses, const int* tags, const float* Tcw, const sdm_vmap_recarve_args* rc, long long E,
                         long long* count, std::vector<int>* order, std::string* why)
{
    const auto refuse = [why](const char* words) {
        *why = words;
        return SDM_EINVAL;
    };
    if (n_poses < 0) return refuse("negative n_poses");
    if (n_poses > 0 && (!tags || !Tcw)) return refuse("null pose table (tags and Tcw are required)");
    const int rc_order = pose_table_order(n_poses, tags, order, why);
    if (rc_order) return rc_order;
    if (rc->end_margin < 0) return refuse("negative end_margin");
    if (rc->max_steps < 1 || rc->max_steps > SDM_FREESPACE_MAX_STEPS) return refuse("max_steps outside 1 .. SDM_FREESPACE_MAX_STEPS");
    if (rc->reset != 0 && rc->reset != 1) return refuse("reset must be 0 or 1");
    if (rc->first < 0 || rc->count < -1 || rc->first > E || rc->count > E - rc->first)
        return refuse("range beyond the log's pairs (first >= 0, count >= -1, first + count <= E)");
    *count = rc->count == -1 ? E - rc->first : rc->count;
    return SDM_OK;
}

}  // namespace sdm
