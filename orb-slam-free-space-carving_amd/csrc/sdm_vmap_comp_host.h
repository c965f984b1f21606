// sdm_vmap_comp_host.h -- the host side of sdm_vmap_components (the kernels are in sdm_vmap_comp.h, the argument checks in
// sdm_vmap_comp_check.h).  Included by sdm_engine.hip inside its extern "C" block, right after sdm_vmap_cast_host.h; put
// together from sdm_vmap_host.h's shared steps.

// ---- connected components of the persistent voxel map's entries (sdm_vmap_comp.h) ---------------------------------------
int sdm_vmap_components(sdm_ctx* c, sdm_vmap_comp_args* a)
{
    if (a) comp_clear_outs(a);
    if (!c) return fail(SDM_EINVAL, "null argument");
    sdm_ctx::Vmap& v = c->vmap;
    std::string why;
    int rc = comp_check(v.open, v.M, a, &why);
    if (rc) return fail(rc, why);
    HIP_TRY(hipSetDevice(c->cfg.device));
    const long long M = v.M;
    if (M == 0) return SDM_OK;  // nothing to label, nothing queued
    a->entries = M;
    const size_t m = (size_t)M;
    const long long vt = ext_tiles(M);
    const bool dev = a->on_device != 0;
    const size_t list_cap = (size_t)std::min(a->small_capacity, M);  // (no list is longer than the map)

    // the scratch, the staging of host destinations and the pinned totals: everything before anything is queued
    ScratchHead head;  // tot: {members, components, small_components, largest, small}
    unsigned *d_parent = nullptr, *d_csize = nullptr;
    Scan scan;
    if ((rc = carve_scratch(&v.d_scratch, &v.scratch_bytes, [&](Carver& k) {
             head = ScratchHead(k);
             d_parent = k.take<unsigned>(m);
             d_csize = k.take<unsigned>(m);
             scan = Scan(k, vt);
         })))
        return rc;
    unsigned *d_label = a->label, *d_size = a->size, *d_small = a->small_ids;
    if (!dev && (rc = carve_scratch(&v.d_out, &v.out_bytes, [&](Carver& k) {
                     if (a->label) d_label = k.take<unsigned>(m);
                     if (a->size) d_size = k.take<unsigned>(m);
                     if (a->small_ids) d_small = k.take<unsigned>(std::max<size_t>(list_cap, 1));
                 })))
        return rc;
    if ((rc = ext_grow_host(&v.h_pin, &v.pin_bytes, 256))) return rc;
    unsigned long long* h_tot = reinterpret_cast<unsigned long long*>(v.h_pin);

    HIP_TRY(hipMemsetAsync(head.tot, 0, 64, c->stream));
    const long long blocks = (M + BLOCK - 1) / BLOCK;
    launch_sliced(c, blocks, [&](long long b0, unsigned g) {
        hipLaunchKernelGGL(k_vcomp_init, dim3(g), dim3(BLOCK), 0, c->stream, v.rec.multiplicity, v.cls.d_pub, a->min_multiplicity,
                           a->require_published, M, b0 * BLOCK, d_parent, d_csize);
    });
    launch_sliced(c, blocks, [&](long long b0, unsigned g) {
        hipLaunchKernelGGL(k_vcomp_link, dim3(g), dim3(BLOCK), 0, c->stream, v.tb, v.rec.xyz, v.inv, comp_max_l1(a->connectivity), M,
                           b0 * BLOCK, d_parent);
    });
    launch_sliced(c, blocks, [&](long long b0, unsigned g) {
        hipLaunchKernelGGL(k_vcomp_flatten, dim3(g), dim3(BLOCK), 0, c->stream, M, b0 * BLOCK, d_parent, d_csize);
    });
    launch_sliced(c, vt, [&](long long t0, unsigned g) {
        hipLaunchKernelGGL(k_vcomp_count, dim3(g), dim3(BLOCK), 0, c->stream, d_parent, d_csize, a->min_size, M, t0, scan.cnt, head.tot);
    });
    scan_counts(c, scan, vt);
    hipLaunchKernelGGL(k_vcomp_totals, dim3(1), dim3(64), 0, c->stream, vt, scan.off, scan.boff, head.tot);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_tot, head.tot, 40, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // the one wait for the counts
    a->members = (long long)h_tot[0];
    a->components = (long long)h_tot[1];
    a->small_components = (long long)h_tot[2];
    a->largest = (long long)h_tot[3];
    a->small = (long long)h_tot[4];
    if (comp_list_too_small(a, a->small))
        return fail(SDM_EINVAL, "small_capacity " + std::to_string(a->small_capacity) + " < " + std::to_string(a->small) +
                                    " members of small components (the totals are filled)");
    if (!a->label && !a->size && !(a->small_ids && a->small)) return SDM_OK;  // the totals only

    launch_sliced(c, vt, [&](long long t0, unsigned g) {
        hipLaunchKernelGGL(k_vcomp_write, dim3(g), dim3(BLOCK), 0, c->stream, d_parent, d_csize, a->min_size, M, t0, scan.off, scan.boff,
                           d_label, d_size, d_small);
    });
    HIP_TRY(hipGetLastError());
    if (!dev) {
        if (a->label) HIP_TRY(hipMemcpyAsync(a->label, d_label, 4 * m, hipMemcpyDeviceToHost, c->stream));
        if (a->size) HIP_TRY(hipMemcpyAsync(a->size, d_size, 4 * m, hipMemcpyDeviceToHost, c->stream));
        if (a->small_ids && a->small)
            HIP_TRY(hipMemcpyAsync(a->small_ids, d_small, 4 * (size_t)a->small, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));  // the last wait
    return SDM_OK;
}
