// sdm_vmap_cast_host.h -- the host side of the voxel map's ray queries: sdm_vmap_cast_segments and sdm_vmap_render (the
// kernel is in sdm_vmap_cast.h, the argument checks in sdm_vmap_cast_check.h).  Included by sdm_engine.hip inside its
// extern "C" block, right after sdm_vmap_host.h, whose shared steps it uses.
#pragma once

extern "C++" {
namespace {

// What both calls do once their arguments have passed: scratch, staging and the pinned mirror from the map's own (all of it
// allocated before anything is queued), the copies in, the launch, one copy per requested field of exactly n elements out,
// and the one wait that brings the totals.  in: every field the ray source needs is set; the map's are set here.
template <bool RENDER>
int vmap_cast_run(sdm_ctx* c, VmapCastIn in, const float* origins, const float* ends, sdm_vmap_cast_args* a)
{
    sdm_ctx::Vmap& v = c->vmap;
    HIP_TRY(hipSetDevice(c->cfg.device));
    const long long n = in.n;
    if (n == 0) return SDM_OK;
    const size_t m = (size_t)n;
    const bool dev = a->on_device != 0;
    float* want_rho = RENDER ? a->hit_rho : nullptr;
    ScratchHead head;  // tot: the kernel's four totals
    float *d_org = nullptr, *d_end = nullptr;
    unsigned* d_id = a->hit_id;
    int* d_step = a->hit_step;
    float* d_rho = want_rho;
    int rc;
    if ((rc = carve_scratch(&v.d_scratch, &v.scratch_bytes, [&](Carver& k) {
             head = ScratchHead(k);
             if (RENDER || dev) return;
             d_org = k.take<float>(3 * m);
             d_end = k.take<float>(3 * m);
         })))
        return rc;
    if (!dev && (rc = carve_scratch(&v.d_out, &v.out_bytes, [&](Carver& k) {  // the staging of host destinations
                     if (a->hit_id) d_id = k.take<unsigned>(m);
                     if (a->hit_step) d_step = k.take<int>(m);
                     if (want_rho) d_rho = k.take<float>(m);
                 })))
        return rc;
    if ((rc = ext_grow_host(&v.h_pin, &v.pin_bytes, 256))) return rc;
    unsigned long long* h_tot = reinterpret_cast<unsigned long long*>(v.h_pin);

    if (!RENDER) {
        if (dev) in.origins = origins, in.ends = ends;
        else {
            HIP_TRY(stage_in(c, d_org, origins, 12 * m));
            HIP_TRY(stage_in(c, d_end, ends, 12 * m));
            in.origins = d_org, in.ends = d_end;
        }
    }
    in.xyz = v.rec.xyz;
    in.multiplicity = v.rec.multiplicity;
    in.published = v.cls.d_pub;  // (null: no classify has run, every flag reads 0)
    in.M = (unsigned)v.M;
    in.voxel = v.voxel_size;
    in.inv = v.inv;
    in.start_margin = a->start_margin;
    in.end_margin = a->end_margin;
    in.max_steps = a->max_steps;
    in.min_multiplicity = a->min_multiplicity;
    in.require_published = a->require_published;
    HIP_TRY(hipMemsetAsync(head.tot, 0, 32, c->stream));
    launch_sliced(c, (n + BLOCK - 1) / BLOCK, [&](long long b0, unsigned g) {
        hipLaunchKernelGGL(k_vmap_cast<RENDER>, dim3(g), dim3(BLOCK), 0, c->stream, in, b0 * BLOCK, v.tb, d_id, d_step, d_rho, head.tot);
    });
    HIP_TRY(hipGetLastError());
    if (!dev) {
        if (a->hit_id) HIP_TRY(hipMemcpyAsync(a->hit_id, d_id, 4 * m, hipMemcpyDeviceToHost, c->stream));
        if (a->hit_step) HIP_TRY(hipMemcpyAsync(a->hit_step, d_step, 4 * m, hipMemcpyDeviceToHost, c->stream));
        if (want_rho) HIP_TRY(hipMemcpyAsync(want_rho, d_rho, 4 * m, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipMemcpyAsync(h_tot, head.tot, 32, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // the one wait: the end, with the totals
    a->rays_total = (long long)h_tot[0];
    a->rays_skipped = (long long)h_tot[1];
    a->rays_hit = (long long)h_tot[2];
    a->cells_visited = (long long)h_tot[3];
    return SDM_OK;
}

}  // namespace
}  // extern "C++"

// ---- ray queries on the persistent voxel map (sdm_vmap_cast.h) -----------------------------------------------------------
int sdm_vmap_cast_segments(sdm_ctx* c, long long n, const float* origins, const float* ends, sdm_vmap_cast_args* a)
{
    if (a) a->rays_total = a->rays_skipped = a->rays_hit = a->cells_visited = 0;
    if (!c) return fail(SDM_EINVAL, "null argument");
    std::string why;
    const int r = cast_segments_check(c->vmap.open, n, origins, ends, a, &why);
    if (r) return fail(r, why);
    VmapCastIn in{};
    in.n = n;
    return vmap_cast_run<false>(c, in, origins, ends, a);
}

int sdm_vmap_render(sdm_ctx* c, const float* K, const float* Tcw, int W, int H, float rho_far, sdm_vmap_cast_args* a)
{
    if (a) a->rays_total = a->rays_skipped = a->rays_hit = a->cells_visited = 0;
    if (!c) return fail(SDM_EINVAL, "null argument");
    std::string why;
    long long n = 0;
    const int r = render_check(c->vmap.open, K, Tcw, W, H, rho_far, a, &n, &why);
    if (r) return fail(r, why);
    VmapCastIn in{};
    in.n = n;
    fill_meta(in.pose, K, Tcw);
    float O[3];
    pose_centre(Tcw, O);
    in.ox = O[0], in.oy = O[1], in.oz = O[2];
    in.rho_far = rho_far;
    in.W = W;
    return vmap_cast_run<true>(c, in, nullptr, nullptr, a);
}
