// sdm_extract_host.h -- the host side of the point-cloud calls (sdm_extract_bound, sdm_extract_points*; the kernels are in
// sdm_extract.h, sdm_support.h, sdm_voxel.h, sdm_voxcam.h, sdm_carve.h) and extract_core, on which the voxel map's calls stand
// too.  Included by sdm_engine.hip inside its extern "C" block, after sdm_host_steps.h, in front of sdm_vmap_host.h.  DESIGN.md §24.1.
#pragma once

extern "C++" {
namespace {

// the largest float <= t (NaN for NaN): for every float v, (double)v > t  <=>  v > ext_float_floor(t)
float ext_float_floor(double t)
{
    const float inf = std::numeric_limits<float>::infinity();
    if (t != t) return std::numeric_limits<float>::quiet_NaN();
    if (t >= (double)std::numeric_limits<float>::max()) return t == (double)inf ? inf : std::numeric_limits<float>::max();
    if (t < -(double)std::numeric_limits<float>::max()) return -inf;
    float f = (float)t;
    if ((double)f > t) f = std::nextafterf(f, -inf);
    return f;
}

// The slots' checks and walks, shared by sdm_extract_points and sdm_extract_bound: count[i] = items of slot i -- its list
// length when the list walk covers every pixel that can pass, W*H otherwise.  Waits for list lengths still in flight.
int ext_plan(sdm_ctx* c, int n, const int* slots, int source, double min_rho, std::vector<char>& use_list, std::vector<int>& count)
{
    if (n < 0 || (n > 0 && !slots)) return fail(SDM_EINVAL, "null or negative slot list");
    if (source != 0 && source != 1) return fail(SDM_EINVAL, "source must be 0 (depth map) or 1 (checked plane)");
    std::vector<char> seen((size_t)c->cfg.max_keyframes, 0);
    for (int i = 0; i < n; i++) {
        const int s = slots[i];
        if (s < 0 || s >= c->cfg.max_keyframes) return fail(SDM_EINVAL, "slot out of range");
        if (seen[(size_t)s]) return fail(SDM_EINVAL, "slot listed twice");
        seen[(size_t)s] = 1;
    }
    for (int i = 0; i < n; i++) {
        if (!c->has_depth[slots[i]]) return fail(SDM_ESTATE, "slot has no depth map");
        if (source && !c->has_chk[slots[i]]) return fail(SDM_ESTATE, "slot has not been inter-keyframe checked");
    }
    // per slot: the list path when the rho plane is zero outside the list now in d_act (the flags sdm_pointset decides by;
    // a depth map counts only while the list is the one of the current lambdaG, which this call does not rebuild) and a
    // zero rho cannot pass (min_rho < 0 keeps the zeros off the list: those slots are walked whole)
    const bool zero_fails = !(0.0 > min_rho);
    use_list.assign((size_t)n, 0);
    count.assign((size_t)n, (int)c->P);
    std::vector<int> list_slots;
    for (int i = 0; i < n; i++) {
        const int s = slots[i];
        const bool has_list = c->act_lambdaG[s] == c->act_lambdaG[s];
        use_list[i] = zero_fails && (source ? (c->chk_sparse[s] && has_list)
                                            : (c->recon_lambdaG[s] == c->dprm.lambdaG && c->act_lambdaG[s] == c->dprm.lambdaG));
        if (use_list[i]) list_slots.push_back(s);
    }
    int rc;
    if (!list_slots.empty() && (rc = sync_counts_for(c, (int)list_slots.size(), list_slots.data(), 0, nullptr))) return rc;
    for (int i = 0; i < n; i++)
        if (use_list[i]) count[i] = c->h_act_count[slots[i]];
    return SDM_OK;
}

// extract_core's hand-over to the calls that go on from the plain cloud: it is left in the engine's staging, not yet waited
// for.  d_ext and d_ext_stage stay as they are until the caller's own last wait: every later purpose has its own buffer.
struct ExtractStaged {
    bool pixel, intensity;                 // in: stage these besides xyz and rho_sigma
    bool support;                          // in: stage the pixel codes and the support words too (k_point_support queued)
    long long total;                       // out: plain points
    ExtractOut at;                         // out: where they are (d_ext_stage)
    const unsigned long long* d_offsets;   // out: the plain offsets[n + 1] on the device (d_ext)
    const unsigned long long* d_support;   // out (support): the words (d_ext_stage)
    const long long* d_block0;             // out (support): k_point_support's block0[n + 1] on the device (d_ext)
    long long blocks;                      // out (support): its workgroups
};

// sdm_extract_points (support == nullptr) and sdm_extract_points_support: the three extraction passes, then -- for the
// second -- k_point_support over the compacted pixel codes (sdm_support.h).  With `st` (`out` names no destination then):
// the passes write xyz, rho_sigma and the fields st asks for into the staging whatever the total, and the call returns
// with pass 3 (and, if st asks for the words, k_point_support) queued.
int extract_core(sdm_ctx* c, int n, const int* slots, int n_nbr, const int* nbr_slots, int source, double max_sigma,
                 double min_rho, sdm_point_buffers* out, unsigned long long* support, long long* offsets,
                 ExtractStaged* st = nullptr)
{
    const bool w_xyz = st || out->xyz;
    const bool w_sup = support || (st && st->support);
    if (st) st->total = 0;
    if (out->capacity < 0) return fail(SDM_EINVAL, "negative capacity");
    if (out->on_device && (((uintptr_t)out->xyz | (uintptr_t)out->pixel) % 4 || (uintptr_t)out->rho_sigma % 8))
        return fail(SDM_EINVAL, "device buffer not aligned (xyz, pixel: 4 B; rho_sigma: 8 B)");
    if (out->on_device && (uintptr_t)support % 8) return fail(SDM_EINVAL, "device buffer not aligned (support: 8 B)");
    std::vector<char> use_list;
    std::vector<int> count;
    int rc = ext_plan(c, n, slots, source, min_rho, use_list, count);
    if (rc) return rc;
    if (w_xyz && !c->xyz) return fail(SDM_ESTATE, "context created without with_pointset");
    if (w_sup) {  // sdm_inter_check's checks of the neighbour table (the slots themselves: ext_plan)
        if (n_nbr < 1) return fail(SDM_EINVAL, "need at least one neighbour");
        if (n_nbr > c->cfg.max_neighbours) return fail(SDM_EINVAL, "n_nbr exceeds max_neighbours");
        for (size_t i = 0; i < (size_t)n * (size_t)n_nbr; i++) {
            const int s = nbr_slots[i];
            if (s < 0 || s >= c->cfg.max_keyframes) return fail(SDM_EINVAL, "slot out of range");
            if (!c->has_depth[s])
                return fail(SDM_ESTATE, "neighbour slot has no depth map (sdm_recon, sdm_upload_depth, an sdm_exchange_* "
                                        "call or sdm_mark_depth_present must come first)");
        }
    }
    HIP_TRY(hipSetDevice(c->cfg.device));
    // RefConst / PairConst of the call (the set an sdm_inter_check over the same lists staged serves this call too); the
    // lists are left as they are: this call changes none
    if (w_sup && n > 0 && (rc = stage_tables(c, n, slots, n_nbr, nbr_slots, nullptr, nullptr, nullptr, false, false))) return rc;

    // the slot table, the offsets and (support) the first workgroup per slot, k_point_support's block0: pinned, then on
    // the device with the tile scan between table and offsets
    struct Tables { ExtractSlot* tab; unsigned long long* offs; long long* cut; } h{}, d{};
    Scan scan;
    long long nt = 0;
    const auto tables = [&](Carver& k, Tables& t, bool dev) {
        t.tab = k.take<ExtractSlot>((size_t)std::max(n, 1));
        if (dev) scan = Scan(k, nt);
        t.offs = k.take<unsigned long long>((size_t)n + 1);
        if (w_sup) t.cut = k.take<long long>((size_t)n + 1);
    };
    if ((rc = carve_scratch(&c->h_ext, &c->ext_host_bytes, [&](Carver& k) { tables(k, h, false); }, ext_grow_host))) return rc;
    for (int i = 0; i < n; i++) {
        h.tab[i] = ExtractSlot{nt, slots[i], count[i], use_list[i] ? 1 : 0, 0};  // (tile0, slot, count, list, pad)
        nt += ext_tiles(count[i]);
    }
    if (nt == 0) {  // nothing to walk: every slot is empty
        for (int i = 0; i <= n; i++) offsets[i] = 0;
        HIP_TRY(hipStreamSynchronize(c->stream));
        return SDM_OK;
    }
    if (scan_blocks(nt) > std::numeric_limits<int>::max() || nt > std::numeric_limits<int>::max())
        return fail(SDM_EINVAL, "too many tiles in one call");
    if ((rc = carve_scratch(&c->d_ext, &c->ext_bytes, [&](Carver& k) { tables(k, d, true); }))) return rc;

    const ExtractIn in{d.tab, n, c->pool, source ? c->chk : nullptr, c->d_act, c->xyz, c->rec, c->P, c->W,
                       ext_float_floor(max_sigma), ext_float_floor(min_rho)};  // (sig_max, rho_min)
    HIP_TRY(hipMemcpyAsync(d.tab, h.tab, sizeof(ExtractSlot) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_extract_count, dim3((unsigned)nt), dim3(BLOCK), 0, c->stream, in, scan.cnt);
    scan_counts(c, scan, nt);
    hipLaunchKernelGGL(k_extract_offsets, dim3(blocks_for(n + 1)), dim3(BLOCK), 0, c->stream, d.tab, n, nt, scan.off, scan.boff,
                       d.offs);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h.offs, d.offs, sizeof(unsigned long long) * (size_t)(n + 1), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // the one wait in the middle: the total sizes what follows
    for (int i = 0; i <= n; i++) offsets[i] = (long long)h.offs[i];
    const long long total = offsets[n];
    if (st) st->total = total, st->d_offsets = d.offs;
    if (!st && total > out->capacity) return fail(SDM_EINVAL, "capacity " + std::to_string(out->capacity) + " < " +
                                                           std::to_string(total) + " points (offsets filled)");
    if (total == 0) return SDM_OK;

    // where pass 3 writes: with st one staging region per field it asks for, which stays there; else the caller's fields
    // (and the pixel codes for k_point_support when the caller did not ask for them, which stay there too)
    ExtractOut dst{};
    unsigned long long* d_sup = nullptr;
    OutCopies outs;
    const size_t t = (size_t)total;
    const bool dev = out->on_device != 0;
    if ((rc = carve_scratch(&c->d_ext_stage, &c->ext_stage_bytes, [&](Carver& k) {
             if (st) {
                 dst.xyz = k.take<float>(3 * t);
                 if (st->pixel || st->support) dst.pixel = k.take<unsigned>(t);
                 dst.rho_sigma = k.take<float2>(t);
                 if (st->intensity) dst.intensity = k.take<unsigned char>(t);
                 if (st->support) d_sup = k.take<unsigned long long>(t);
                 return;
             }
             dst.xyz = outs.field(k, out->xyz, 3 * t, dev);
             dst.pixel = (w_sup && !out->pixel) ? k.take<unsigned>(t) : outs.field(k, out->pixel, t, dev);
             dst.rho_sigma = reinterpret_cast<float2*>(outs.field(k, out->rho_sigma, 2 * t, dev));
             dst.intensity = outs.field(k, out->intensity, t, dev);
             d_sup = outs.field(k, support, t, dev);
         })))
        return rc;
    hipLaunchKernelGGL(k_extract_write, dim3((unsigned)nt), dim3(BLOCK), 0, c->stream, in, scan.off, scan.boff, dst);
    HIP_TRY(hipGetLastError());
    if (w_sup) {
        long long blocks = 0;
        for (int i = 0; i < n; i++) {
            h.cut[i] = blocks;
            blocks += (offsets[i + 1] - offsets[i] + SUP_BLOCK - 1) / SUP_BLOCK;
        }
        h.cut[n] = blocks;
        HIP_TRY(hipMemcpyAsync(d.cut, h.cut, sizeof(long long) * (size_t)(n + 1), hipMemcpyHostToDevice, c->stream));
        launch_sliced(c, blocks, [&](long long b0, unsigned g) {
            hipLaunchKernelGGL(k_point_support, dim3(g), dim3(SUP_BLOCK), 0, c->stream, c->pool, c->P, c->d_refs, c->d_pairs, n,
                               n_nbr, c->W, c->H, d.cut, b0, d.offs, dst.pixel, d_sup);
        }, SUP_BLOCK);
        HIP_TRY(hipGetLastError());
        if (st) st->d_support = d_sup, st->d_block0 = d.cut, st->blocks = blocks;
    }
    if (st) {
        st->at = dst;
        return SDM_OK;
    }
    HIP_TRY(outs.flush(c));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SDM_OK;
}

// ---- the cameras of a call (the voxel calls with cameras; sdm_vmap_carve) --------------------------------------------------
// the distinct slots among `slots` and the neighbour table, numbered in ascending order (every slot's range has been checked)
struct CallCameras {
    std::vector<int> cam_of;       // per slot of the context: its camera, -1 where the call does not name the slot
    std::vector<int> slot_of_cam;  // [Cn]
    int Cn = 0;
};

CallCameras call_cameras(const sdm_ctx* c, int n, const int* slots, int n_nbr, const int* nbr_slots)
{
    CallCameras q;
    q.cam_of.assign((size_t)c->cfg.max_keyframes, -1);
    for (int i = 0; i < n; i++) q.cam_of[(size_t)slots[i]] = 0;
    for (size_t i = 0; i < (size_t)n * (size_t)n_nbr; i++) q.cam_of[(size_t)nbr_slots[i]] = 0;
    for (int s = 0; s < c->cfg.max_keyframes; s++)
        if (q.cam_of[(size_t)s] == 0) q.cam_of[(size_t)s] = q.Cn++, q.slot_of_cam.push_back(s);
    return q;
}

// a resident slot's camera centre from its current pose, as pointset_pixel forms Ow: O = -(Rwc * tcw); the fourth value pads
void slot_centre(const sdm_ctx* c, int slot, float* o)
{
    const float* Tcw = c->h_meta[slot].Tcw;
    float Rwc[9], Ow[3];
    const float tcw[3] = {Tcw[3], Tcw[7], Tcw[11]};
    for (int i = 0; i < 3; i++)
        for (int k = 0; k < 3; k++) Rwc[i * 3 + k] = Tcw[k * 4 + i];
    mat3_vec(Rwc, tcw, Ow);
    for (int i = 0; i < 3; i++) o[i] = -Ow[i];
    o[3] = 0.f;
}

// ---- one point per voxel (sdm_voxel.h), with the cameras of each (sdm_voxcam.h) and the rays through it (sdm_carve.h) --------
// What the stages of a voxel call hand on; a stage that fails has set the message and filled what its refusal promises.
struct VoxelCall {
    sdm_ctx* c;
    sdm_point_buffers* out;
    sdm_voxel_buffers* vox;
    long long* offsets;
    int n, n_nbr;  // (the neighbour table: the calls with cameras; 0 and null otherwise)
    const int *slots, *nbr_slots;
    float voxel_size;
    bool cameras, walk;       // the call forms the camera lists; the free-space walk follows them
    sdm_voxel_cameras* cams;  // (cameras) the lists' destinations
    unsigned* crossings;      // (walk) the counters' destination
    unsigned *mult = nullptr, *sidx = nullptr, *repr = nullptr;  // vox's destinations (null: none, or no vox)
    // the merge: plain points, kept points, tiles and workgroups of the plain points
    ExtractStaged st{};
    long long T = 0, M = 0, vt = 0, pblocks = 0;
    VoxTable tb{};
    unsigned *d_where = nullptr, *d_flag = nullptr;
    unsigned long long *d_voffs = nullptr, *h_voffs = nullptr;
    Scan scan, kscan;  // over the plain points' tiles; (cameras) over the kept points'
    // where the kept points go, and every plain point's kept rank (the caller's `representative`, or the cameras' scratch)
    ExtractOut dst{};
    unsigned *d_mult = nullptr, *d_sidx = nullptr, *d_rank = nullptr, *d_cross = nullptr;
    OutCopies outs, cam_outs;
    // the cameras: the table's ints (slot_of_cam[Cn] own_cam[n] nbr_cam[n][n_nbr]), bitset words, kept tiles, list entries
    CallCameras cam;
    size_t cam_tab_n = 0;
    int Wd = 0, *h_ctab = nullptr, *d_cslots = nullptr;
    long long kt = 0, E = 0, *d_coff = nullptr;
    VoxCamTable ctab{};
    unsigned long long *h_E = nullptr, *h_fs_tot = nullptr, *d_bits = nullptr, *d_E = nullptr, *d_fs_tot = nullptr;
    float inv = 0.f, *h_org = nullptr, *d_org = nullptr;  // 1 / voxel_size; (walk) the camera centres
};

// stage 1, the checks, in the order the calls always made them
int voxel_checks(VoxelCall& v)
{
    const sdm_point_buffers* out = v.out;
    if (!v.c || !out || !v.offsets) return fail(SDM_EINVAL, "null argument");
    if (v.n < 0) return fail(SDM_EINVAL, "null or negative slot list");
    if (v.cameras) {
        const sdm_voxel_cameras* cams = v.cams;
        if (!v.nbr_slots) return fail(SDM_EINVAL, "null nbr_slots");
        if (!v.walk && !cams->cam_offsets && !cams->cam_slots) return fail(SDM_EINVAL, "no camera output requested");
        if (cams->cam_slots && cams->cam_capacity < 0) return fail(SDM_EINVAL, "negative capacity");
        if (out->on_device && ((uintptr_t)cams->cam_offsets % 8 || (uintptr_t)cams->cam_slots % 4))
            return fail(SDM_EINVAL, "device buffer not aligned (cam_offsets: 8 B; cam_slots: 4 B)");
    }
    if (v.walk && out->on_device && (uintptr_t)v.crossings % 4) return fail(SDM_EINVAL, "device buffer not aligned (crossings: 4 B)");
    if (!(v.voxel_size > 0.0f) || !std::isfinite(v.voxel_size)) return fail(SDM_EINVAL, "voxel_size must be finite and > 0");
    v.inv = 1.0f / v.voxel_size;
    if (!std::isfinite(v.inv)) return fail(SDM_EINVAL, "1 / voxel_size is not finite");
    if (v.vox) v.mult = v.vox->multiplicity, v.sidx = v.vox->source_index, v.repr = v.vox->representative;
    if (!v.cameras && !out->xyz && !out->pixel && !out->rho_sigma && !out->intensity && !v.mult && !v.sidx && !v.repr)
        return fail(SDM_EINVAL, "no output requested");
    if (out->capacity < 0 || (v.repr && v.vox->rep_capacity < 0)) return fail(SDM_EINVAL, "negative capacity");
    if (out->on_device && (((uintptr_t)out->xyz | (uintptr_t)out->pixel | (uintptr_t)v.mult | (uintptr_t)v.sidx | (uintptr_t)v.repr) % 4 ||
                           (uintptr_t)out->rho_sigma % 8))
        return fail(SDM_EINVAL, "device buffer not aligned (xyz, pixel, multiplicity, source_index, representative: 4 B; "
                                "rho_sigma: 8 B)");
    return SDM_OK;
}

// (cameras) the table, on the host while the merge runs: the cameras of the call, per row the camera of its own slot and of its
// neighbours.  h_vcam = 8 B for the lists' total | at +16 the walk's totals | at +256 the table | (walk) the centres
int voxcam_table(VoxelCall& v)
{
    sdm_ctx* c = v.c;
    const int n = v.n;
    const size_t np = (size_t)n * (size_t)v.n_nbr;
    v.cam = call_cameras(c, n, v.slots, v.n_nbr, v.nbr_slots);
    const int Cn = v.cam.Cn;
    v.cam_tab_n = (size_t)Cn + (size_t)n + np;
    const int rc = carve_scratch(&c->h_vcam, &c->vcam_host_bytes, [&](Carver& k) {
        v.h_E = k.ptr<unsigned long long>(k.at);
        v.h_fs_tot = k.ptr<unsigned long long>(k.at + 16);
        k.take<unsigned char>(256);
        v.h_ctab = k.take<int>(v.cam_tab_n);
        if (v.walk) v.h_org = k.take<float>(4 * (size_t)Cn);
    }, ext_grow_host);
    if (rc) return rc;
    for (int q = 0; q < Cn; q++) v.h_ctab[q] = v.cam.slot_of_cam[(size_t)q];
    for (int i = 0; i < n; i++) v.h_ctab[Cn + i] = v.cam.cam_of[(size_t)v.slots[i]];
    for (size_t i = 0; i < np; i++) v.h_ctab[(size_t)Cn + (size_t)n + i] = v.cam.cam_of[(size_t)v.nbr_slots[i]];
    for (int q = 0; v.walk && q < Cn; q++) slot_centre(c, v.cam.slot_of_cam[(size_t)q], v.h_org + 4 * q);
    return SDM_OK;
}

// stage 2, the merge: the plain cloud into the staging (xyz and rho_sigma feed the merge whatever the caller asks for;
// cameras: the words of k_point_support too), the table, insert, count, offsets, the second wait, and where the kept points
// go.  v.T == 0 on success: no plain point, the offsets -- (cameras) and cam_offsets[0] -- are 0, the stream has been waited for.
int voxel_merge(VoxelCall& v, int source, double max_sigma, double min_rho)
{
    sdm_ctx* c = v.c;
    const sdm_point_buffers* out = v.out;
    const int n = v.n;
    v.st.pixel = out->pixel != nullptr;
    v.st.intensity = out->intensity != nullptr;
    v.st.support = v.cameras;
    sdm_point_buffers none{};
    std::vector<long long> plain((size_t)n + 1, 0);
    int rc = extract_core(c, n, v.slots, v.n_nbr, v.nbr_slots, source, max_sigma, min_rho, &none, nullptr, plain.data(), &v.st);
    if (rc) return rc;
    const long long T = v.T = v.st.total;
    if (v.vox) v.vox->plain_total = T;
    if (T >= 0xffffffffll) return fail(SDM_EINVAL, "2^32 - 1 or more plain points in one call");
    if (T == 0) {
        for (int i = 0; i <= n; i++) v.offsets[i] = 0;
        if (v.cameras && v.cams->cam_offsets) {  // no kept point: the one entry cam_offsets[0] = 0
            if (out->on_device) {
                HIP_TRY(hipMemsetAsync(v.cams->cam_offsets, 0, sizeof(long long), c->stream));
                HIP_TRY(hipStreamSynchronize(c->stream));
            } else {
                v.cams->cam_offsets[0] = 0;
            }
        }
        return SDM_OK;
    }
    unsigned long long cap = 1024;
    while (cap < 2ull * (unsigned long long)T) cap <<= 1;
    if (cap > (1ull << 31)) return fail(SDM_EINVAL, "more than 2^30 plain points: the voxel table would exceed 2^31 slots");

    // keys | values | counts, the overflow flag behind them | ranks | where | the tiles' scan | offsets[n + 1], flag; the
    // offsets' pinned mirror is h_ext, which the plain passes are done with
    v.vt = ext_tiles(T);
    v.pblocks = (T + BLOCK - 1) / BLOCK;
    VoxTable& tb = v.tb;
    c->vox_last_keys = nullptr;  // (the scratch may move)
    if ((rc = carve_scratch(&c->d_vox, &c->vox_bytes, [&](Carver& k) {
             tb.keys = k.take<unsigned long long>((size_t)cap);
             tb.vals = k.take<unsigned long long>((size_t)cap);
             tb.cnt = k.take<unsigned>((size_t)cap);
             v.d_flag = k.take<unsigned>(1);
             tb.rank = k.take<unsigned>((size_t)cap);
             v.d_where = k.take<unsigned>((size_t)T);
             v.scan = Scan(k, v.vt);
             v.d_voffs = k.take<unsigned long long>((size_t)n + 2);
         })) ||
        (rc = carve_scratch(&c->h_ext, &c->ext_host_bytes, [&](Carver& k) { v.h_voffs = k.take<unsigned long long>((size_t)n + 2); },
                            ext_grow_host)))
        return rc;
    tb.mask = cap - 1;
    c->vox_last_keys = tb.keys, c->vox_last_cap = cap;
    const auto bytes_to = [](const void* from, const void* to) { return (size_t)((const unsigned char*)to - (const unsigned char*)from); };
    HIP_TRY(hipMemsetAsync(tb.keys, 0xff, bytes_to(tb.keys, tb.cnt), c->stream));  // keys: VOX_EMPTY; values: the minimum's identity
    HIP_TRY(hipMemsetAsync(tb.cnt, 0, bytes_to(tb.cnt, tb.rank), c->stream));      // counts and the flag
    launch_sliced(c, v.pblocks, [&](long long b0, unsigned g) {
        hipLaunchKernelGGL(k_voxel_insert, dim3(g), dim3(BLOCK), 0, c->stream, v.st.at.xyz, v.st.at.rho_sigma, T, b0 * BLOCK, v.inv, tb,
                           v.d_where, v.d_flag);
    });
    launch_sliced(c, v.vt, [&](long long t0, unsigned g) {
        hipLaunchKernelGGL(k_voxel_count, dim3(g), dim3(BLOCK), 0, c->stream, tb, v.d_where, T, t0, v.scan.cnt);
    });
    scan_counts(c, v.scan, v.vt);
    hipLaunchKernelGGL(k_voxel_offsets, dim3((unsigned)(n + 2)), dim3(BLOCK), 0, c->stream, tb, v.d_where, T, v.st.d_offsets, n, v.vt,
                       v.scan.off, v.scan.boff, v.d_flag, v.d_voffs);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(v.h_voffs, v.d_voffs, 8 * (size_t)(n + 2), hipMemcpyDeviceToHost, c->stream));
    if (v.cameras && (rc = voxcam_table(v))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));  // the second wait: the kept total sizes what follows
    if (v.h_voffs[n + 1]) return fail(SDM_EHIP, "voxel table overflow");
    for (int i = 0; i <= n; i++) v.offsets[i] = (long long)v.h_voffs[i];
    const long long M = v.M = v.offsets[n];
    if (M > out->capacity) return fail(SDM_EINVAL, "capacity " + std::to_string(out->capacity) + " < " + std::to_string(M) +
                                                       " points (offsets and plain_total filled)");
    if (v.repr && T > v.vox->rep_capacity)
        return fail(SDM_EINVAL, "rep_capacity " + std::to_string(v.vox->rep_capacity) + " < " + std::to_string(T) +
                                    " plain points (offsets and plain_total filled)");
    // where the kept points go: the caller's device arrays, or one staging region per requested output
    const size_t m = (size_t)M;
    const bool dev = out->on_device != 0;
    return carve_scratch(&c->d_vox_out, &c->vox_out_bytes, [&](Carver& k) {
        v.dst.xyz = v.outs.field(k, out->xyz, 3 * m, dev);
        v.dst.pixel = v.outs.field(k, out->pixel, m, dev);
        v.dst.rho_sigma = reinterpret_cast<float2*>(v.outs.field(k, out->rho_sigma, 2 * m, dev));
        v.dst.intensity = v.outs.field(k, out->intensity, m, dev);
        v.d_mult = v.outs.field(k, v.mult, m, dev);
        v.d_sidx = v.outs.field(k, v.sidx, m, dev);
        v.d_rank = v.outs.field(k, v.repr, (size_t)T, dev);
    });
}

// stage 3: the kept points' write, and every plain point's kept rank where something takes it
int voxel_write(VoxelCall& v)
{
    sdm_ctx* c = v.c;
    launch_sliced(c, v.vt, [&](long long t0, unsigned g) {
        hipLaunchKernelGGL(k_voxel_write, dim3(g), dim3(BLOCK), 0, c->stream, v.tb, v.d_where, v.T, t0, v.scan.off, v.scan.boff, v.st.at,
                           v.dst, v.d_mult, v.d_sidx, v.d_rank);
    });
    if (v.d_rank)
        launch_sliced(c, v.pblocks, [&](long long b0, unsigned g) {
            hipLaunchKernelGGL(k_voxel_rep, dim3(g), dim3(BLOCK), 0, c->stream, v.tb, v.d_where, v.T, b0 * BLOCK, v.d_rank);
        });
    HIP_TRY(hipGetLastError());
    return SDM_OK;
}

// stage 4, the cameras (sdm_voxcam.h).  Their scratch, ahead of the kept points' write because the ranks live there when the
// caller takes no `representative`: the staged table, the ranks, the bitsets, the kept tiles' scan and the lists' total
int voxcam_prepare(VoxelCall& v)
{
    sdm_ctx* c = v.c;
    const int Cn = v.cam.Cn;
    const long long M = v.M;
    v.Wd = (Cn + 63) / 64;
    v.kt = ext_tiles(M);
    // the scan keeps 32-bit sums per EXT_SCAN tiles (k_extract_scan_tiles): a kept point has at most Cn cameras
    if ((unsigned long long)std::min(M, (long long)EXT_TILE * EXT_SCAN) * (unsigned long long)Cn >= (1ull << 32))
        return fail(SDM_EINVAL, "camera lists of 2^22 kept points could pass 2^32 entries: too many distinct slots in one call");
    int* d_ctab = nullptr;
    const size_t bits = (size_t)M * (size_t)v.Wd;
    int rc = carve_scratch(&c->d_vcam, &c->vcam_bytes, [&](Carver& k) {
        d_ctab = k.take<int>(v.cam_tab_n);
        if (!v.repr) v.d_rank = k.take<unsigned>((size_t)v.T);
        v.d_bits = k.take<unsigned long long>(bits);
        v.kscan = Scan(k, v.kt);
        v.d_E = k.take<unsigned long long>(1);
    });
    if (rc) return rc;
    v.ctab.slot_of_cam = d_ctab;
    v.ctab.own_cam = d_ctab + Cn;
    v.ctab.nbr_cam = d_ctab + Cn + v.n;
    HIP_TRY(hipMemsetAsync(v.d_bits, 0, 8 * bits, c->stream));
    HIP_TRY(stage_in(c, d_ctab, v.h_ctab, 4 * v.cam_tab_n));
    if (!v.walk) return SDM_OK;
    // (walk, sdm_carve.h) the centres, the call totals, and the kept points' xyz when no destination holds them on the device
    const bool own_xyz = !v.dst.xyz;
    if ((rc = carve_scratch(&c->d_carve, &c->carve_bytes, [&](Carver& k) {
             v.d_org = k.take<float>(4 * (size_t)Cn);
             v.d_fs_tot = k.take<unsigned long long>(2);
             if (own_xyz) v.dst.xyz = k.take<float>(3 * (size_t)M);
         })))
        return rc;
    HIP_TRY(stage_in(c, v.d_org, v.h_org, 16 * (size_t)Cn));
    return SDM_OK;
}

// ... and behind the write: bitsets, count, scan, the third wait -- the lists' total, for the capacity check -- and the lists.
// (walk) Both lists are formed on the device whether named or not; the counters stand in front: host copies go in this order.
int voxcam_lists(VoxelCall& v)
{
    sdm_ctx* c = v.c;
    sdm_voxel_cameras* cams = v.cams;
    const int n = v.n, n_nbr = v.n_nbr, Wd = v.Wd;
    const long long M = v.M, kt = v.kt;
    const ExtractStaged& st = v.st;
    // SDM_VOXCAM_PLAIN_OR: one atomic per lane and word instead of one per run of equal rank (A/B; the same bits)
    const bool plain_or = getenv("SDM_VOXCAM_PLAIN_OR") != nullptr;
    launch_sliced(c, st.blocks, [&](long long b0, unsigned g) {
        if (plain_or)
            hipLaunchKernelGGL(k_voxcam_or<false>, dim3(g), dim3(SUP_BLOCK), 0, c->stream, st.d_block0, b0, n, n_nbr, st.d_offsets,
                               st.d_support, v.d_rank, v.ctab, Wd, v.d_bits);
        else
            hipLaunchKernelGGL(k_voxcam_or<true>, dim3(g), dim3(SUP_BLOCK), 0, c->stream, st.d_block0, b0, n, n_nbr, st.d_offsets,
                               st.d_support, v.d_rank, v.ctab, Wd, v.d_bits);
    }, SUP_BLOCK);
    launch_sliced(c, kt, [&](long long t0, unsigned g) {
        hipLaunchKernelGGL(k_voxcam_count, dim3(g), dim3(BLOCK), 0, c->stream, v.d_bits, Wd, M, t0, v.kscan.cnt);
    });
    scan_counts(c, v.kscan, kt);
    // (with no slot, k_extract_offsets writes the one entry offsets[0] = the offset of tile kt: the total)
    hipLaunchKernelGGL(k_extract_offsets, dim3(1), dim3(BLOCK), 0, c->stream, (const ExtractSlot*)nullptr, 0, kt, v.kscan.off,
                       v.kscan.boff, v.d_E);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(v.h_E, v.d_E, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // the third wait
    const long long E = v.E = (long long)*v.h_E;
    cams->cam_total = E;
    if (cams->cam_slots && E > cams->cam_capacity)
        return fail(SDM_EINVAL, "cam_capacity " + std::to_string(cams->cam_capacity) + " < " + std::to_string(E) +
                                    " list entries (offsets, plain_total and cam_total filled)");
    if (v.walk && E >= (1ll << 32)) return fail(SDM_EINVAL, "2^32 or more rays in one call");
    const bool dev = v.out->on_device != 0;
    const int rc = carve_scratch(&c->d_vcam_out, &c->vcam_out_bytes, [&](Carver& k) {
        if (v.walk) v.d_cross = v.cam_outs.field(k, v.crossings, (size_t)M, dev);
        v.d_coff = (v.walk && !cams->cam_offsets) ? k.take<long long>((size_t)M + 1)
                                                   : v.cam_outs.field(k, cams->cam_offsets, (size_t)M + 1, dev);
        v.d_cslots = (v.walk && !cams->cam_slots) ? k.take<int>((size_t)E) : v.cam_outs.field(k, cams->cam_slots, (size_t)E, dev);
    });
    if (rc) return rc;
    launch_sliced(c, kt, [&](long long t0, unsigned g) {
        hipLaunchKernelGGL(k_voxcam_write, dim3(g), dim3(BLOCK), 0, c->stream, v.d_bits, Wd, M, t0, v.kscan.off, v.kscan.boff,
                           v.ctab.slot_of_cam, v.d_coff, v.d_cslots);
    });
    HIP_TRY(hipGetLastError());
    return SDM_OK;
}

// stage 5, the free-space walk (sdm_carve.h), behind the lists: one lane per list entry walks its ray through the table; the
// totals on their way to the host
int voxel_carve(VoxelCall& v, const sdm_voxel_freespace* fs)
{
    sdm_ctx* c = v.c;
    HIP_TRY(hipMemsetAsync(v.d_cross, 0, 4 * (size_t)v.M, c->stream));
    HIP_TRY(hipMemsetAsync(v.d_fs_tot, 0, 16, c->stream));
    const CarveIn in{v.dst.xyz, v.d_coff, v.d_cslots, v.ctab.slot_of_cam, v.d_org, v.M, v.E, v.cam.Cn, v.voxel_size, v.inv,
                     fs->end_margin, fs->max_steps};
    launch_sliced(c, (v.E + BLOCK - 1) / BLOCK, [&](long long b0, unsigned g) {
        hipLaunchKernelGGL(k_voxel_carve, dim3(g), dim3(BLOCK), 0, c->stream, in, b0 * BLOCK, v.tb, v.d_cross, v.d_fs_tot);
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(v.h_fs_tot, v.d_fs_tot, 16, hipMemcpyDeviceToHost, c->stream));
    return SDM_OK;
}

// stage 6: the copies to host destinations and the last wait
int voxel_finish(VoxelCall& v)
{
    HIP_TRY(v.cam_outs.flush(v.c));
    HIP_TRY(v.outs.flush(v.c));
    HIP_TRY(hipStreamSynchronize(v.c->stream));
    return SDM_OK;
}

}  // namespace
}  // extern "C++"

int sdm_extract_bound(sdm_ctx* c, int n, const int* slots, int source, double min_rho, long long* bound)
{
    if (!c || !bound) return fail(SDM_EINVAL, "null argument");
    std::vector<char> use_list;
    std::vector<int> count;
    int rc = ext_plan(c, n, slots, source, min_rho, use_list, count);
    if (rc) return rc;
    long long b = 0;
    for (int i = 0; i < n; i++) b += count[i];
    *bound = b;
    return SDM_OK;
}

int sdm_extract_points(sdm_ctx* c, int n, const int* slots, int source, double max_sigma, double min_rho,
                       sdm_point_buffers* out, long long* offsets)
{
    if (!c || !out || !offsets) return fail(SDM_EINVAL, "null argument");
    if (!out->xyz && !out->pixel && !out->rho_sigma && !out->intensity) return fail(SDM_EINVAL, "no output field requested");
    return extract_core(c, n, slots, 0, nullptr, source, max_sigma, min_rho, out, nullptr, offsets);
}

int sdm_extract_points_support(sdm_ctx* c, int n, const int* slots, int n_nbr, const int* nbr_slots, int source,
                               double max_sigma, double min_rho, sdm_point_buffers* out, unsigned long long* support,
                               long long* offsets)
{
    if (!c || !out || !offsets) return fail(SDM_EINVAL, "null argument");
    if (!support) return fail(SDM_EINVAL, "null support");
    if (!nbr_slots) return fail(SDM_EINVAL, "null nbr_slots");
    return extract_core(c, n, slots, n_nbr, nbr_slots, source, max_sigma, min_rho, out, support, offsets);
}

int sdm_extract_points_voxel(sdm_ctx* c, int n, const int* slots, int source, double max_sigma, double min_rho,
                             float voxel_size, sdm_point_buffers* out, sdm_voxel_buffers* vox, long long* offsets)
{
    VoxelCall v{c, out, vox, offsets, n, 0, slots, nullptr, voxel_size, false, false, nullptr, nullptr};
    int rc;
    if ((rc = voxel_checks(v)) || (rc = voxel_merge(v, source, max_sigma, min_rho)) || v.T == 0) return rc;
    return (rc = voxel_write(v)) ? rc : voxel_finish(v);
}

int sdm_extract_points_voxel_cameras(sdm_ctx* c, int n, const int* slots, int n_nbr, const int* nbr_slots, int source,
                                     double max_sigma, double min_rho, float voxel_size, sdm_point_buffers* out,
                                     sdm_voxel_buffers* vox, sdm_voxel_cameras* cams, long long* offsets)
{
    if (!cams) return fail(SDM_EINVAL, "null cams");
    cams->cam_total = 0;
    VoxelCall v{c, out, vox, offsets, n, n_nbr, slots, nbr_slots, voxel_size, true, false, cams, nullptr};
    int rc;
    if ((rc = voxel_checks(v)) || (rc = voxel_merge(v, source, max_sigma, min_rho)) || v.T == 0) return rc;
    if ((rc = voxcam_prepare(v)) || (rc = voxel_write(v)) || (rc = voxcam_lists(v))) return rc;
    return voxel_finish(v);
}

int sdm_extract_points_voxel_freespace(sdm_ctx* c, int n, const int* slots, int n_nbr, const int* nbr_slots, int source,
                                       double max_sigma, double min_rho, float voxel_size, sdm_point_buffers* out,
                                       sdm_voxel_buffers* vox, sdm_voxel_cameras* cams, sdm_voxel_freespace* fs,
                                       long long* offsets)
{
    if (fs) fs->rays_total = fs->rays_skipped = fs->cells_visited = 0;
    if (!cams) return fail(SDM_EINVAL, "null cams");
    cams->cam_total = 0;
    if (!fs) return fail(SDM_EINVAL, "null fs");
    if (!fs->crossings) return fail(SDM_EINVAL, "null crossings");
    if (fs->end_margin < 0) return fail(SDM_EINVAL, "negative end_margin");
    if (fs->max_steps < 1 || fs->max_steps > SDM_FREESPACE_MAX_STEPS)
        return fail(SDM_EINVAL, "max_steps outside 1 .. SDM_FREESPACE_MAX_STEPS");
    VoxelCall v{c, out, vox, offsets, n, n_nbr, slots, nbr_slots, voxel_size, true, true, cams, fs->crossings};
    int rc;
    if ((rc = voxel_checks(v)) || (rc = voxel_merge(v, source, max_sigma, min_rho)) || v.T == 0) return rc;
    if ((rc = voxcam_prepare(v)) || (rc = voxel_write(v)) || (rc = voxcam_lists(v)) || (rc = voxel_carve(v, fs)) || (rc = voxel_finish(v)))
        return rc;
    fs->rays_total = cams->cam_total;
    fs->rays_skipped = (long long)v.h_fs_tot[0];
    fs->cells_visited = (long long)v.h_fs_tot[1];
    return SDM_OK;
}
