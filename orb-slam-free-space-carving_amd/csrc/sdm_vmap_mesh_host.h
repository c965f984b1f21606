// sdm_vmap_mesh_host.h -- the host side of sdm_vmap_mesh (the kernels are in sdm_vmap_mesh.h, the argument checks in
// sdm_vmap_mesh_check.h).  Included by sdm_engine.hip inside its extern "C" block, right after sdm_vmap_normals_host.h; put
// together from sdm_vmap_host.h's shared steps.

// ---- a triangle mesh of the persistent voxel map's entries (sdm_vmap_mesh.h) ---------------------------------------------
int sdm_vmap_mesh(sdm_ctx* c, sdm_vmap_mesh_args* a)
{
    if (a) mesh_clear_outs(a);
    if (!c) return fail(SDM_EINVAL, "null argument");
    sdm_ctx::Vmap& v = c->vmap;
    std::string why;
    long long count = 0;
    int rc = mesh_check(v.open, v.M, a, &count, &why);
    if (rc) return fail(rc, why);
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (count == 0) return SDM_OK;  // an empty range: nothing queued
    const size_t n = (size_t)count, m = (size_t)v.M;
    const long long vt = ext_tiles(count);
    const bool dev = a->on_device != 0;
    const size_t list_cap = (size_t)std::min(a->tri_capacity, 2 * count);  // (no list is longer than two per entry)

    // the scratch, the staging of the host's normals and destinations and the pinned totals: everything before anything is
    // queued
    ScratchHead head;  // tot: {entries, members, owners, quads, singles, triangles, vertices}
    unsigned* d_corner = nullptr;
    unsigned char *d_ntri = nullptr, *d_used = nullptr;
    const float* d_normal = a->normal;
    Scan scan;
    if ((rc = carve_scratch(&v.d_scratch, &v.scratch_bytes, [&](Carver& k) {
             head = ScratchHead(k);
             d_corner = k.take<unsigned>(3 * n);
             d_ntri = k.take<unsigned char>(n);
             d_used = k.take<unsigned char>(m);
             scan = Scan(k, vt);
             if (!dev) d_normal = k.take<float>(3 * n);
         })))
        return rc;
    unsigned* d_tri = a->tri;
    unsigned char* d_owner = a->owner_tris;
    if (!dev && (a->tri || a->owner_tris) && (rc = carve_scratch(&v.d_out, &v.out_bytes, [&](Carver& k) {
                                                  if (a->tri) d_tri = k.take<unsigned>(3 * std::max<size_t>(list_cap, 1));
                                                  if (a->owner_tris) d_owner = k.take<unsigned char>(n);
                                              })))
        return rc;
    if ((rc = ext_grow_host(&v.h_pin, &v.pin_bytes, 256))) return rc;
    unsigned long long* h_tot = reinterpret_cast<unsigned long long*>(v.h_pin);

    HIP_TRY(hipMemsetAsync(head.tot, 0, 64, c->stream));
    HIP_TRY(hipMemsetAsync(d_used, 0, m, c->stream));
    if (!dev) HIP_TRY(stage_in(c, d_normal, a->normal, 12 * n));
    VmapMeshIn in;
    in.xyz = v.rec.xyz;
    in.multiplicity = v.rec.multiplicity;
    in.published = v.cls.d_pub;  // (null: no classify has run, every flag reads 0)
    in.normal = d_normal;
    in.first = a->first;
    in.count = count;
    in.M = (unsigned)v.M;
    in.inv = v.inv;
    in.min_multiplicity = a->min_multiplicity;
    in.require_published = a->require_published;
    launch_sliced(c, (count + BLOCK - 1) / BLOCK, [&](long long b0, unsigned g) {
        hipLaunchKernelGGL(k_vmesh_find, dim3(g), dim3(BLOCK), 0, c->stream, in, b0 * BLOCK, v.tb, d_corner, d_ntri, d_used, head.tot);
    });
    launch_sliced(c, vt, [&](long long t0, unsigned g) {
        hipLaunchKernelGGL(k_vmesh_count, dim3(g), dim3(BLOCK), 0, c->stream, d_ntri, count, t0, scan.cnt);
    });
    scan_counts(c, scan, vt);
    launch_sliced(c, (v.M + BLOCK - 1) / BLOCK, [&](long long b0, unsigned g) {
        hipLaunchKernelGGL(k_vmesh_vertices, dim3(g), dim3(BLOCK), 0, c->stream, d_used, v.M, b0 * BLOCK, head.tot);
    });
    hipLaunchKernelGGL(k_vmesh_totals, dim3(1), dim3(64), 0, c->stream, vt, scan.off, scan.boff, head.tot);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_tot, head.tot, 56, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // the one wait for the counts
    a->entries = (long long)h_tot[0];
    a->members = (long long)h_tot[1];
    a->owners = (long long)h_tot[2];
    a->quads = (long long)h_tot[3];
    a->singles = (long long)h_tot[4];
    a->triangles = (long long)h_tot[5];
    a->vertices = (long long)h_tot[6];
    if (mesh_list_too_small(a, a->triangles))
        return fail(SDM_EINVAL, "tri_capacity " + std::to_string(a->tri_capacity) + " < " + std::to_string(a->triangles) +
                                    " triangles (the totals are filled)");
    if (!(a->tri && a->triangles) && !a->owner_tris && !a->vertex_used) return SDM_OK;  // the totals only

    if ((a->tri && a->triangles) || a->owner_tris) {
        launch_sliced(c, vt, [&](long long t0, unsigned g) {
            hipLaunchKernelGGL(k_vmesh_write, dim3(g), dim3(BLOCK), 0, c->stream, d_corner, d_ntri, a->first, count, t0, scan.off,
                               scan.boff, a->triangles ? d_tri : nullptr, d_owner);
        });
        HIP_TRY(hipGetLastError());
    }
    if (a->vertex_used)  // the plane as the find pass left it, straight from the scratch
        HIP_TRY(hipMemcpyAsync(a->vertex_used, d_used, m, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
    if (!dev) {
        if (a->tri && a->triangles)
            HIP_TRY(hipMemcpyAsync(a->tri, d_tri, 12 * (size_t)a->triangles, hipMemcpyDeviceToHost, c->stream));
        if (a->owner_tris) HIP_TRY(hipMemcpyAsync(a->owner_tris, d_owner, n, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));  // the last wait
    return SDM_OK;
}
