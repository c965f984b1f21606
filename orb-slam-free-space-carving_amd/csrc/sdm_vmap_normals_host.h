// sdm_vmap_normals_host.h -- the host side of sdm_vmap_normals (the kernel is in sdm_vmap_normals.h, the argument checks in
// sdm_vmap_normals_check.h).  Included by sdm_engine.hip inside its extern "C" block, right after sdm_vmap_comp_host.h; put
// together from sdm_vmap_host.h's shared steps.

// ---- per-entry surface normals and variation of the persistent voxel map (sdm_vmap_normals.h) ---------------------------
int sdm_vmap_normals(sdm_ctx* c, int n_poses, const int* tags, const float* Tcw, sdm_vmap_normal_args* a)
{
    if (a) normals_clear_outs(a);
    if (!c) return fail(SDM_EINVAL, "null argument");
    sdm_ctx::Vmap& v = c->vmap;
    std::vector<int> order;  // the table's rows by ascending tag
    std::string why;
    long long count = 0;
    int rc = normals_check(v.open, v.M, n_poses, tags, Tcw, a, &count, &order, &why);
    if (rc) return fail(rc, why);
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (count == 0) return SDM_OK;  // an empty range: nothing queued
    const size_t m = (size_t)count;
    const bool dev = a->on_device != 0;

    // the scratch, the staging of host destinations and the pinned mirror: everything before anything is queued
    const size_t np = (size_t)n_poses;
    const size_t tags_b = ext_align(4 * np), org_b = ext_align(16 * np);
    ScratchHead head;  // tot: {entries, members, estimated, oriented}
    int* d_tags = nullptr;
    float* d_org = nullptr;
    if ((rc = carve_scratch(&v.d_scratch, &v.scratch_bytes, [&](Carver& k) {
             head = ScratchHead(k);
             d_tags = k.take<int>(np);  // (tags | centres: one copy fills both)
             d_org = k.take<float>(4 * np);
         })))
        return rc;
    float *d_normal = a->normal, *d_var = a->variation;
    unsigned* d_points = a->points;
    if (!dev && (a->normal || a->variation || a->points) && (rc = carve_scratch(&v.d_out, &v.out_bytes, [&](Carver& k) {
                                                                 if (a->normal) d_normal = k.take<float>(3 * m);
                                                                 if (a->variation) d_var = k.take<float>(m);
                                                                 if (a->points) d_points = k.take<unsigned>(m);
                                                             })))
        return rc;
    if ((rc = ext_grow_host(&v.h_pin, &v.pin_bytes, 256 + tags_b + org_b))) return rc;
    unsigned long long* h_tot = reinterpret_cast<unsigned long long*>(v.h_pin);
    int* h_tags = reinterpret_cast<int*>(v.h_pin + 256);
    float* h_org = reinterpret_cast<float*>(v.h_pin + 256 + tags_b);
    for (size_t q = 0; q < np; q++) {
        const size_t at = (size_t)order[q];
        h_tags[q] = tags[at];
        pose_centre(Tcw + 12 * at, h_org + 4 * q);
        h_org[4 * q + 3] = 0.f;
    }

    HIP_TRY(hipMemsetAsync(head.tot, 0, 64, c->stream));
    if (np) HIP_TRY(stage_in(c, d_tags, h_tags, tags_b + org_b));
    VmapNormalsIn in;
    in.xyz = v.rec.xyz;
    in.multiplicity = v.rec.multiplicity;
    in.rec_tag = v.rec.tag;
    in.published = v.cls.d_pub;  // (null: no classify has run, every flag reads 0)
    in.tags = d_tags;
    in.origin = d_org;
    in.first = a->first;
    in.count = count;
    in.n = n_poses;
    in.M = (unsigned)v.M;
    in.inv = v.inv;
    in.min_points = a->min_points;
    in.min_multiplicity = a->min_multiplicity;
    in.require_published = a->require_published;
    launch_sliced(c, (count + BLOCK - 1) / BLOCK, [&](long long b0, unsigned g) {
        if (a->radius == 1)
            hipLaunchKernelGGL(k_vmap_normals<1>, dim3(g), dim3(BLOCK), 0, c->stream, in, b0 * BLOCK, v.tb, d_normal, d_var, d_points, head.tot);
        else
            hipLaunchKernelGGL(k_vmap_normals<2>, dim3(g), dim3(BLOCK), 0, c->stream, in, b0 * BLOCK, v.tb, d_normal, d_var, d_points, head.tot);
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_tot, head.tot, 32, hipMemcpyDeviceToHost, c->stream));
    if (!dev) {
        if (a->normal) HIP_TRY(hipMemcpyAsync(a->normal, d_normal, 12 * m, hipMemcpyDeviceToHost, c->stream));
        if (a->variation) HIP_TRY(hipMemcpyAsync(a->variation, d_var, 4 * m, hipMemcpyDeviceToHost, c->stream));
        if (a->points) HIP_TRY(hipMemcpyAsync(a->points, d_points, 4 * m, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));  // the one wait: the end, with the totals
    a->entries = (long long)h_tot[0];
    a->members = (long long)h_tot[1];
    a->estimated = (long long)h_tot[2];
    a->oriented = (long long)h_tot[3];
    return SDM_OK;
}
