// sdm_vmap_host.h -- the host side of the persistent voxel map: every sdm_vmap_* call of the C ABI (the kernels are in
// sdm_vmap*.h, one header per feature) and the steps the calls share.  Included by sdm_engine.hip inside its extern "C"
// block after sdm_ctx, fail, HIP_TRY, launch_sliced and scan_counts, after sdm_host_steps.h (the ext_* helpers, DevBlock, Carver,
// carve_scratch, Scan, stage_in) and sdm_extract_host.h (extract_core, call_cameras, slot_centre).  DESIGN.md §24 says how a call is built.
#pragma once

extern "C++" {
namespace {

// ---- the shared steps: scratch and layouts (DevBlock, Carver, carve_scratch, Scan, stage_in: sdm_host_steps.h) --------------
// the 512 B every scratch starts with: the counters a call clears and its kernels fill
struct ScratchHead {
    unsigned char* base = nullptr;
    unsigned* ctr = nullptr;             // +0: the map's insert kernels' {dropped, overflow}
    unsigned long long* mid = nullptr;   // +64: a call's own counters; the log's insert kernels' three
    unsigned long long* tot = nullptr;   // +256: what a totals kernel leaves for the read-back
    ScratchHead() = default;
    explicit ScratchHead(Carver& k)
    {
        const size_t at = k.at;
        base = k.take<unsigned char>(512);
        ctr = k.ptr<unsigned>(at);
        mid = k.ptr<unsigned long long>(at + 64);
        tot = k.ptr<unsigned long long>(at + 256);
    }
};

// two of them over the same tiles, interleaved: cnt | cnt | off | off | bsum | boff | bsum | boff
struct ScanPair {
    Scan s[2];
    ScanPair() = default;
    ScanPair(Carver& k, long long tiles, long long counts)  // (counts: `tiles`, or what a call rounds it up to)
    {
        for (Scan& x : s) x.cnt = k.take<unsigned>((size_t)counts);
        for (Scan& x : s) x.off = k.take<unsigned>((size_t)tiles + 1);
        for (Scan& x : s) {
            x.bsum = k.take<unsigned long long>((size_t)scan_blocks(tiles));
            x.boff = k.take<unsigned long long>((size_t)scan_blocks(tiles));
        }
    }
};

// what the scratch of a call that inserts `items` into the map's table starts with (integrate, import, repose): where[items]
// from the insert kernel, then the new ([0]) and updated ([1]) entries per tile
struct VmapScratch {
    ScratchHead head;  // tot: k_vmap_totals' {created, updated, dropped, overflow}, then the import kernels' sum of m
    unsigned* where = nullptr;
    ScanPair scan;
    long long tiles = 0;
    VmapScratch() = default;
    VmapScratch(Carver& k, long long items)
        : head(k), where(k.take<unsigned>((size_t)items)), scan(k, ext_tiles(items), ext_tiles(items)), tiles(ext_tiles(items))
    {
    }
};

// the same for the observation set (observe, import_observations, and the log's rebuild in repose and retire): one count,
// the created pairs.  head.mid: the insert kernels' three counters; head.tot: k_vobs_totals' {created, .., .., overflow}
struct VobsScratch {
    ScratchHead head;
    unsigned* where = nullptr;
    Scan scan;
    long long tiles = 0;
    VobsScratch() = default;
    VobsScratch(Carver& k, long long items)
        : head(k), where(k.take<unsigned>((size_t)items)), scan(k, ext_tiles(items)), tiles(ext_tiles(items))
    {
    }
};

int memset_rc(hipError_t e)
{
    return e == hipSuccess ? SDM_OK : fail(SDM_EHIP, std::string("hipMemsetAsync: ") + hipGetErrorString(e));
}

// The layouts.  Each make_* function lays one block out; the reset beside it restores what the block held when made, from
// the pointers alone, so no other function restates a layout.
// the map's table: keys | cval | id | cfirst | ccnt (28 B per slot); empty keys and the reductions' identities are all
// ones, the counts 0
hipError_t vmap_reset_table(sdm_ctx* c, const VmapTable& tb)
{
    unsigned char *first = reinterpret_cast<unsigned char*>(tb.keys), *ccnt = reinterpret_cast<unsigned char*>(tb.ccnt);
    const hipError_t e = hipMemsetAsync(first, 0xff, (size_t)(ccnt - first), c->stream);
    return e != hipSuccess ? e : hipMemsetAsync(ccnt, 0, sizeof(unsigned) * (size_t)(tb.mask + 1), c->stream);
}

int vmap_make_table(sdm_ctx* c, unsigned long long cap, DevBlock& block, VmapTable* tb)
{
    const size_t n = (size_t)cap;
    const int rc = block.alloc(28 * n);
    if (rc) return rc;
    unsigned char* p = block.p;
    tb->keys = reinterpret_cast<unsigned long long*>(p);
    tb->cval = reinterpret_cast<unsigned long long*>(p + 8 * n);
    tb->id = reinterpret_cast<unsigned*>(p + 16 * n);
    tb->cfirst = reinterpret_cast<unsigned*>(p + 20 * n);
    tb->ccnt = reinterpret_cast<unsigned*>(p + 24 * n);
    tb->mask = cap - 1;
    return memset_rc(vmap_reset_table(c, *tb));
}

// the records of `cap` entries, every array 256-byte aligned (nothing to reset: an entry's record is written when it is made)
int vmap_make_records(long long cap, DevBlock& block, VmapRecords* r)
{
    const size_t n = (size_t)std::max(cap, 1ll);
    const auto lay = [&](Carver& k) {
        r->xyz = k.take<float>(3 * n);
        r->rho_sigma = k.take<float2>(n);
        r->pixel = k.take<unsigned>(n);
        r->tag = k.take<int>(n);
        r->multiplicity = k.take<unsigned>(n);
        r->epoch = k.take<unsigned>(n);
        r->intensity = k.take<unsigned char>(n);
    };
    Carver bytes{nullptr};
    lay(bytes);
    const int rc = block.alloc(bytes.at);
    if (rc) return rc;
    Carver k{block.p};
    lay(k);
    return SDM_OK;
}

// the free-space counters of `cap` entries: crossings | ends, both zero
hipError_t vmap_zero_evidence(sdm_ctx* c, unsigned long long* crossings, unsigned long long* ends)
{
    return hipMemsetAsync(crossings, 0, 2 * sizeof(unsigned long long) * (size_t)(ends - crossings), c->stream);
}

int vmap_make_evidence(sdm_ctx* c, long long cap, DevBlock& block, unsigned long long** crossings, unsigned long long** ends)
{
    const size_t b8 = ext_align(8 * (size_t)std::max(cap, 1ll));
    const int rc = block.alloc(2 * b8);
    if (rc) return rc;
    *crossings = reinterpret_cast<unsigned long long*>(block.p);
    *ends = reinterpret_cast<unsigned long long*>(block.p + b8);
    return memset_rc(vmap_zero_evidence(c, *crossings, *ends));
}

// the observations' per-entry arrays of `cap` entries: last_obs (all ones: no observation) | ncam (0)
hipError_t vobs_reset_entries(sdm_ctx* c, unsigned* last_obs, unsigned* ncam)
{
    const size_t b4 = sizeof(unsigned) * (size_t)(ncam - last_obs);
    const hipError_t e = hipMemsetAsync(last_obs, 0xff, b4, c->stream);
    return e != hipSuccess ? e : hipMemsetAsync(ncam, 0, b4, c->stream);
}

int vmap_make_obs_entries(sdm_ctx* c, long long cap, DevBlock& block, unsigned** last_obs, unsigned** ncam)
{
    const size_t b4 = ext_align(4 * (size_t)std::max(cap, 1ll));
    const int rc = block.alloc(2 * b4);
    if (rc) return rc;
    *last_obs = reinterpret_cast<unsigned*>(block.p);
    *ncam = reinterpret_cast<unsigned*>(block.p + b4);
    return memset_rc(vobs_reset_entries(c, *last_obs, *ncam));
}

// the published flags of `cap` entries, all 0
hipError_t vmap_zero_published(sdm_ctx* c, unsigned char* pub, long long cap)
{
    return hipMemsetAsync(pub, 0, (size_t)std::max(cap, 1ll), c->stream);
}

int vmap_make_published(sdm_ctx* c, long long cap, DevBlock& block)
{
    const int rc = block.alloc((size_t)std::max(cap, 1ll));
    return rc ? rc : memset_rc(vmap_zero_published(c, block.p, cap));
}

// the observation set: keys | ord | idx (20 B per slot), all ones: empty keys, ord's identity, no index
hipError_t vobs_reset_table(sdm_ctx* c, const VobsTable& tb)
{
    unsigned char* first = reinterpret_cast<unsigned char*>(tb.keys);
    return hipMemsetAsync(first, 0xff, (size_t)(reinterpret_cast<unsigned char*>(tb.idx + tb.mask + 1) - first), c->stream);
}

int vobs_make_table(sdm_ctx* c, unsigned long long cap, DevBlock& block, VobsTable* tb)
{
    const size_t n = (size_t)cap;
    const int rc = block.alloc(20 * n);
    if (rc) return rc;
    unsigned char* p = block.p;
    tb->keys = reinterpret_cast<unsigned long long*>(p);
    tb->ord = reinterpret_cast<unsigned long long*>(p + 8 * n);
    tb->idx = reinterpret_cast<unsigned*>(p + 16 * n);
    tb->mask = cap - 1;
    return memset_rc(vobs_reset_table(c, *tb));
}

// A second set of the per-entry arrays -- the records and, where asked for, counters, observation heads and lengths,
// flags -- made whole before anything is written and adopted when everything has succeeded: by vmap_grow (a larger
// capacity) and by repose and retire (the same capacity, the entries re-placed).  An allocation that fails leaves the
// map as it was.
struct VmapSecond {
    long long cap = 0;
    DevBlock rec, evid, ent, pub;
    VmapRecords r{};
    unsigned long long *crossings = nullptr, *ends = nullptr;
    unsigned *last_obs = nullptr, *ncam = nullptr;
};

int vmap_make_second(sdm_ctx* c, long long cap, bool evid, bool ent, bool pub, VmapSecond* s)
{
    int rc;
    s->cap = cap;
    if ((rc = vmap_make_records(cap, s->rec, &s->r))) return rc;
    if (evid && (rc = vmap_make_evidence(c, cap, s->evid, &s->crossings, &s->ends))) return rc;
    if (ent && (rc = vmap_make_obs_entries(c, cap, s->ent, &s->last_obs, &s->ncam))) return rc;
    if (pub && (rc = vmap_make_published(c, cap, s->pub))) return rc;
    return SDM_OK;
}

// the second set becomes the map's (after the wait for whatever filled it); the old blocks leave with `s`
void vmap_adopt_second_sets(sdm_ctx::Vmap& v, VmapSecond& s)
{
    s.rec.install(v.d_rec);
    v.rec = s.r;
    v.rec_cap = s.cap;
    if (s.evid.p) {
        s.evid.install(v.d_evid);
        v.crossings = s.crossings;
        v.ends = s.ends;
    }
    if (s.ent.p) {
        s.ent.install(v.obs.d_ent);
        v.obs.last_obs = s.last_obs;
        v.obs.ncam = s.ncam;
    }
    if (s.pub.p) s.pub.install(v.cls.d_pub);
}

void vmap_free(sdm_ctx* c)
{
    sdm_ctx::Vmap& v = c->vmap;
    (void)hipFree(v.d_table);
    (void)hipFree(v.d_rec);
    (void)hipFree(v.d_evid);
    (void)hipFree(v.d_scratch);
    (void)hipFree(v.d_out);
    (void)hipHostFree(v.h_pin);
    (void)hipFree(v.obs.d_table);
    (void)hipFree(v.obs.d_log);
    (void)hipFree(v.obs.d_ent);
    (void)hipFree(v.obs.d_scratch);
    (void)hipFree(v.obs.d_out);
    (void)hipHostFree(v.obs.h_pin);
    (void)hipFree(v.cls.d_pub);
    v = sdm_ctx::Vmap{};
}

// table and per-entry arrays for `need` entries, made before anything is inserted; the old ones stay intact if an
// allocation fails
int vmap_grow(sdm_ctx* c, long long need)
{
    sdm_ctx::Vmap& v = c->vmap;
    int rc;
    if (2ull * (unsigned long long)need > v.cap) {
        unsigned long long cap = v.cap;
        while (cap < 2ull * (unsigned long long)need) cap <<= 1;
        DevBlock block;
        VmapTable nw{};
        if ((rc = vmap_make_table(c, cap, block, &nw))) return rc;
        HIP_TRY(hipMemsetAsync(v.d_scratch, 0, 8, c->stream));  // (the counters: the caller has sized the scratch)
        launch_sliced(c, (long long)((v.cap + BLOCK - 1) / BLOCK), [&](long long b0, unsigned g) {
            hipLaunchKernelGGL(k_vmap_rehash, dim3(g), dim3(BLOCK), 0, c->stream, v.tb.keys, v.tb.id, v.cap,
                               (unsigned long long)b0 * BLOCK, nw, reinterpret_cast<unsigned*>(v.d_scratch));
        });
        unsigned* h_ctr = reinterpret_cast<unsigned*>(v.h_pin);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(h_ctr, v.d_scratch, 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess || h_ctr[1])
            return fail(SDM_EHIP, e != hipSuccess ? std::string("voxel map rehash: ") + hipGetErrorString(e)
                                                  : std::string("voxel map table overflow while rehashing"));
        block.install(v.d_table);
        v.tb = nw;
        v.cap = cap;
        v.rehashes++;
    }
    if (need > v.rec_cap) {
        VmapSecond s;  // geometric: the copies amortise
        if ((rc = vmap_make_second(c, std::max(need, 2 * v.rec_cap), v.d_evid, v.obs.d_ent, v.cls.d_pub, &s))) return rc;
        // M entries of every array the map has are copied; the rest keeps what its make_* function set
        const struct {
            void* to;  // (null: the map has no such array)
            const void* from;
            size_t bytes;  // per entry
        } copies[] = {{s.pub.p, v.cls.d_pub, 1},
                      {s.last_obs, v.obs.last_obs, 4},
                      {s.ncam, v.obs.ncam, 4},
                      {s.crossings, v.crossings, 8},
                      {s.ends, v.ends, 8},
                      {s.r.xyz, v.rec.xyz, 12},
                      {s.r.rho_sigma, v.rec.rho_sigma, 8},
                      {s.r.pixel, v.rec.pixel, 4},
                      {s.r.tag, v.rec.tag, 4},
                      {s.r.multiplicity, v.rec.multiplicity, 4},
                      {s.r.epoch, v.rec.epoch, 4},
                      {s.r.intensity, v.rec.intensity, 1}};
        const size_t m = (size_t)v.M;
        hipError_t e = hipSuccess;
        for (const auto& cp : copies)
            if (m && cp.to && e == hipSuccess) e = hipMemcpyAsync(cp.to, cp.from, cp.bytes * m, hipMemcpyDeviceToDevice, c->stream);
        // one wait serves every copy; without entries it is for the optional arrays' memsets
        if (e == hipSuccess && (m || s.evid.p || s.ent.p || s.pub.p)) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return fail(SDM_EHIP, std::string("voxel map records: ") + hipGetErrorString(e));
        vmap_adopt_second_sets(v, s);
    }
    return SDM_OK;
}

// After a call's insert kernel has filled s.where for `items`: the new and updated entries per tile, counted against
// `rec` (the map's records or a second set), their scans, k_vmap_totals, and the wait that brings `bytes` of the totals to
// the map's pinned mirror.  Fails on a full table.
int vmap_count_and_total(sdm_ctx* c, const VmapRecords& rec, const VmapScratch& s, long long items, size_t bytes)
{
    sdm_ctx::Vmap& v = c->vmap;
    const Scan &nw = s.scan.s[0], &upd = s.scan.s[1];
    launch_sliced(c, s.tiles, [&](long long t0, unsigned g) {
        hipLaunchKernelGGL(k_vmap_count, dim3(g), dim3(BLOCK), 0, c->stream, v.tb, rec, s.where, items, t0, nw.cnt, upd.cnt);
    });
    scan_counts(c, nw, s.tiles);
    scan_counts(c, upd, s.tiles);
    hipLaunchKernelGGL(k_vmap_totals, dim3(1), dim3(64), 0, c->stream, s.tiles, nw.off, nw.boff, upd.off, upd.boff, s.head.ctr,
                       s.head.tot);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(v.h_pin, s.head.tot, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (reinterpret_cast<const unsigned long long*>(v.h_pin)[3]) return fail(SDM_EHIP, "voxel map table overflow");
    return SDM_OK;
}

// the entries of s.where that k_vmap_count found new get their ids, from `first` on in order of first appearance
void vmap_assign_ids(sdm_ctx* c, const VmapRecords& rec, const VmapScratch& s, unsigned first, long long items)
{
    launch_sliced(c, s.tiles, [&](long long t0, unsigned g) {
        hipLaunchKernelGGL(k_vmap_ids, dim3(g), dim3(BLOCK), 0, c->stream, c->vmap.tb, rec, s.where, first, items, t0,
                           s.scan.s[0].off, s.scan.s[0].boff);
    });
}

// After an insert kernel of the observation set has filled s.where for `items`: the created pairs per tile, their scan and
// k_vobs_totals; then, once the log has room for them, the commit from log index `first` on.
void vobs_count(sdm_ctx* c, const VobsScratch& s, long long items)
{
    sdm_ctx::Vmap::Obs& o = c->vmap.obs;
    launch_sliced(c, s.tiles, [&](long long t0, unsigned g) {
        hipLaunchKernelGGL(k_vobs_count, dim3(g), dim3(BLOCK), 0, c->stream, o.tb, s.where, items, t0, s.scan.cnt);
    });
    scan_counts(c, s.scan, s.tiles);
    hipLaunchKernelGGL(k_vobs_totals, dim3(1), dim3(64), 0, c->stream, s.tiles, s.scan.off, s.scan.boff, s.head.mid, s.head.tot);
}

void vobs_commit(sdm_ctx* c, const VobsScratch& s, unsigned first, long long items)
{
    sdm_ctx::Vmap::Obs& o = c->vmap.obs;
    launch_sliced(c, s.tiles, [&](long long t0, unsigned g) {
        hipLaunchKernelGGL(k_vobs_commit, dim3(g), dim3(BLOCK), 0, c->stream, o.tb, o.log, o.last_obs, o.ncam, s.where, first, items,
                           t0, s.scan.off, s.scan.boff);
    });
}

// The log after the entries moved (repose, retire): its E pairs, in log order, go through remap[M] into the emptied set
// and per-entry arrays, in place; pairs marked in `pmark` (null: none) stay out.  The totals are on their way to the log's
// pinned mirror when this returns: after the caller's wait, [3] is the overflow flag and [0] the new E.
int vobs_rebuild_through_remap(sdm_ctx* c, const unsigned* d_remap, long long M, long long M2, const unsigned char* d_pmark,
                               const VobsScratch& s)
{
    sdm_ctx::Vmap::Obs& o = c->vmap.obs;
    const long long E = o.E;
    HIP_TRY(vobs_reset_table(c, o.tb));
    HIP_TRY(vobs_reset_entries(c, o.last_obs, o.ncam));
    HIP_TRY(hipMemsetAsync(s.head.mid, 0, 24, c->stream));
    launch_sliced(c, (E + BLOCK - 1) / BLOCK, [&](long long b0, unsigned g) {
        hipLaunchKernelGGL(k_vobs_import_insert, dim3(g), dim3(BLOCK), 0, c->stream, (const unsigned*)o.log.entry,
                           (const int*)o.log.tag, d_remap, M, E, b0 * BLOCK, (unsigned)M2, o.tb, s.where, s.head.mid, d_pmark);
    });
    vobs_count(c, s, E);
    vobs_commit(c, s, 0u, E);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(o.h_pin, s.head.tot, 32, hipMemcpyDeviceToHost, c->stream));
    return SDM_OK;
}

// What the fetch calls check alike, in this order: the counts, the range (without ids) or first == 0 (with ids), and a
// host id list against the map's entries (a device list is checked by the gather kernel, which raises `bad`).
int fetch_check(const sdm_ctx::Vmap& v, const unsigned* ids, long long first, long long count, long long capacity, bool dev)
{
    if (count < 0 || capacity < 0) return fail(SDM_EINVAL, "negative count or capacity");
    if (count > capacity) return fail(SDM_EINVAL, "count exceeds capacity");
    if (ids ? first != 0 : (first < 0 || first > v.M || count > v.M - first))
        return fail(SDM_EINVAL, ids ? "first must be 0 with ids" : "range beyond the map's entries");
    if (ids && !dev)
        for (long long j = 0; j < count; j++)
            if ((long long)ids[j] >= v.M) return fail(SDM_EINVAL, "id beyond the map's entries");
    return SDM_OK;
}

// The gathering half of a fetch with ids, in the map's staging: the ids (a host list is copied there), the cleared `bad`
// flag and -- for host destinations -- the dense regions fields(Carver&) describes, one per output.
struct FetchIds {
    const unsigned* d_ids = nullptr;
    unsigned *d_bad = nullptr, *h_bad = nullptr;
};

template <typename F>
int fetch_stage_ids(sdm_ctx* c, const unsigned* ids, size_t m, bool dev, F&& fields, FetchIds* f)
{
    sdm_ctx::Vmap& v = c->vmap;
    unsigned* own = nullptr;
    int rc;
    if ((rc = carve_scratch(&v.d_out, &v.out_bytes,
                            [&](Carver& k) {
                                own = k.take<unsigned>(m);
                                f->d_bad = reinterpret_cast<unsigned*>(k.take<unsigned char>(256));
                                if (!dev) fields(k);
                            })) ||
        (rc = ext_grow_host(&v.h_pin, &v.pin_bytes, 256)))
        return rc;
    f->h_bad = reinterpret_cast<unsigned*>(v.h_pin);
    f->d_ids = ids;
    if (!dev) {
        HIP_TRY(hipMemcpyAsync(own, ids, 4 * m, hipMemcpyHostToDevice, c->stream));
        f->d_ids = own;
    }
    HIP_TRY(hipMemsetAsync(f->d_bad, 0, 4, c->stream));
    return SDM_OK;
}

// behind the gather kernel: the flag on its way to the host
int fetch_read_bad(sdm_ctx* c, const FetchIds& f)
{
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(f.h_bad, f.d_bad, 4, hipMemcpyDeviceToHost, c->stream));
    return SDM_OK;
}

// the one wait of a fetch, and what the flag says (h_bad null: no ids)
int fetch_finish(sdm_ctx* c, const FetchIds& f)
{
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (f.h_bad && *f.h_bad) return fail(SDM_EINVAL, "id beyond the map's entries (the destinations are unspecified)");
    return SDM_OK;
}

}  // namespace
}  // extern "C++"

// ---- the persistent voxel map (sdm_vmap_*, sdm_vmap.h) -------------------------------------------------------------------
int sdm_vmap_open(sdm_ctx* c, float voxel_size, long long reserve_voxels)
{
    if (!c) return fail(SDM_EINVAL, "null argument");
    if (c->vmap.open) return fail(SDM_ESTATE, "the context already has an open voxel map");
    if (!c->xyz) return fail(SDM_ESTATE, "context created without with_pointset");
    if (!(voxel_size > 0.0f) || !std::isfinite(voxel_size)) return fail(SDM_EINVAL, "voxel_size must be finite and > 0");
    const float inv = 1.0f / voxel_size;
    if (!std::isfinite(inv)) return fail(SDM_EINVAL, "1 / voxel_size is not finite");
    if (reserve_voxels < 0 || reserve_voxels > (1ll << 30)) return fail(SDM_EINVAL, "reserve_voxels outside 0 .. 2^30");
    HIP_TRY(hipSetDevice(c->cfg.device));
    sdm_ctx::Vmap& v = c->vmap;
    unsigned long long cap = 1024;
    while (cap < 2ull * (unsigned long long)reserve_voxels) cap <<= 1;
    DevBlock table, rec;
    VmapTable tb{};
    VmapRecords r{};
    int rc;
    if ((rc = vmap_make_table(c, cap, table, &tb)) || (rc = vmap_make_records(reserve_voxels, rec, &r))) return rc;
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(SDM_EHIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    table.install(v.d_table);
    rec.install(v.d_rec);
    v.tb = tb;
    v.rec = r;
    v.cap = cap;
    v.rec_cap = std::max(reserve_voxels, 1ll);
    v.voxel_size = voxel_size;
    v.inv = inv;
    v.open = true;
    return SDM_OK;
}

int sdm_vmap_clear(sdm_ctx* c)
{
    if (!c) return fail(SDM_EINVAL, "null argument");
    sdm_ctx::Vmap& v = c->vmap;
    if (!v.open) return fail(SDM_ESTATE, "no open voxel map");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(vmap_reset_table(c, v.tb));
    if (v.d_evid) HIP_TRY(vmap_zero_evidence(c, v.crossings, v.ends));
    if (v.obs.d_table) HIP_TRY(vobs_reset_table(c, v.obs.tb));
    // (the log keeps its capacity; its content is dead with E = 0)
    if (v.obs.d_ent) HIP_TRY(vobs_reset_entries(c, v.obs.last_obs, v.obs.ncam));
    if (v.cls.d_pub) HIP_TRY(vmap_zero_published(c, v.cls.d_pub, v.rec_cap));
    HIP_TRY(hipStreamSynchronize(c->stream));
    v.cls.published = v.cls.calls = 0;
    v.M = v.points = v.dropped = v.calls = v.rehashes = 0;
    v.obs.E = v.obs.calls = v.obs.rehashes = 0;
    v.obs.seen.clear();
    return SDM_OK;
}

int sdm_vmap_close(sdm_ctx* c)
{
    if (!c) return fail(SDM_EINVAL, "null argument");
    if (!c->vmap.open) return fail(SDM_ESTATE, "no open voxel map");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    vmap_free(c);
    return SDM_OK;
}

int sdm_vmap_get_info(sdm_ctx* c, sdm_vmap_info* info)
{
    if (!c || !info) return fail(SDM_EINVAL, "null argument");
    const sdm_ctx::Vmap& v = c->vmap;
    if (!v.open) return fail(SDM_ESTATE, "no open voxel map");
    std::memset(info, 0, sizeof(*info));
    info->voxels = v.M;
    info->points = v.points;
    info->dropped = v.dropped;
    info->calls = v.calls;
    info->table_slots = (long long)v.cap;
    info->rehashes = v.rehashes;
    info->voxel_size = v.voxel_size;
    return SDM_OK;
}

int sdm_vmap_integrate(sdm_ctx* c, int n, const int* slots, const int* tags, int source, double max_sigma, double min_rho,
                       sdm_vmap_delta* delta)
{
    if (delta) delta->plain_total = delta->dropped = delta->first_created = delta->created = delta->updated = 0;
    if (!c) return fail(SDM_EINVAL, "null argument");
    sdm_ctx::Vmap& v = c->vmap;
    if (!v.open) return fail(SDM_ESTATE, "no open voxel map");
    if (n < 0) return fail(SDM_EINVAL, "null or negative slot list");
    unsigned* upd_dst = delta ? delta->updated_ids : nullptr;
    if (upd_dst && delta->updated_capacity < 0) return fail(SDM_EINVAL, "negative capacity");
    if (upd_dst && delta->on_device && (uintptr_t)upd_dst % 4) return fail(SDM_EINVAL, "device buffer not aligned (updated_ids: 4 B)");

    // the plain cloud, all four fields, into the engine's staging
    ExtractStaged st{};
    st.pixel = st.intensity = true;
    sdm_point_buffers none{};
    std::vector<long long> plain((size_t)n + 1, 0);
    int rc = extract_core(c, n, slots, 0, nullptr, source, max_sigma, min_rho, &none, nullptr, plain.data(), &st);
    if (rc) return rc;
    const long long T = st.total;
    if (delta) delta->plain_total = T, delta->first_created = v.M;
    if (v.M + T > (1ll << 30)) return fail(SDM_EINVAL, "more than 2^30 entries and plain points: the voxel map's table would exceed 2^31 slots");
    if (upd_dst && delta->updated_capacity < std::min(v.M, T))
        return fail(SDM_EINVAL, "updated_capacity " + std::to_string(delta->updated_capacity) + " < min(entries, plain points) = " +
                                    std::to_string(std::min(v.M, T)) + " (plain_total and first_created filled)");
    if (T == 0) {  // (extract_core has waited for the stream)
        v.calls++;
        return SDM_OK;
    }

    // scratch, staging and growth: everything is allocated before anything is inserted
    VmapScratch s;
    int* d_tags = nullptr;
    if ((rc = carve_scratch(&v.d_scratch, &v.scratch_bytes, [&](Carver& k) {
             s = VmapScratch(k, T);
             d_tags = k.take<int>((size_t)n);
         })))
        return rc;
    if ((rc = ext_grow_host(&v.h_pin, &v.pin_bytes, 256 + ext_align(4 * (size_t)n)))) return rc;
    const bool stage_upd = upd_dst && !delta->on_device;
    if (stage_upd && (rc = ext_grow_dev(&v.d_out, &v.out_bytes, 4 * (size_t)std::min(v.M, T)))) return rc;
    if ((rc = vmap_grow(c, v.M + T))) return rc;
    unsigned long long* h_tot = reinterpret_cast<unsigned long long*>(v.h_pin);  // {created, updated, dropped, overflow}
    int* h_tags = reinterpret_cast<int*>(v.h_pin + 256);
    for (int i = 0; i < n; i++) h_tags[i] = tags ? tags[i] : slots[i];

    HIP_TRY(hipMemsetAsync(s.head.ctr, 0, 8, c->stream));
    HIP_TRY(hipMemcpyAsync(d_tags, h_tags, 4 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    launch_sliced(c, (T + BLOCK - 1) / BLOCK, [&](long long b0, unsigned g) {
        hipLaunchKernelGGL(k_vmap_insert, dim3(g), dim3(BLOCK), 0, c->stream, st.at.xyz, st.at.rho_sigma, T, b0 * BLOCK, v.inv, v.tb,
                           s.where, s.head.ctr);
    });
    if ((rc = vmap_count_and_total(c, v.rec, s, T, 32))) return rc;  // the second wait: created and updated
    const long long created = (long long)h_tot[0], updated = (long long)h_tot[1], dropped = (long long)h_tot[2];

    unsigned* d_upd = !upd_dst ? nullptr : stage_upd ? reinterpret_cast<unsigned*>(v.d_out) : upd_dst;
    const unsigned first_created = (unsigned)v.M, epoch = (unsigned)(v.calls + 1);
    vmap_assign_ids(c, v.rec, s, first_created, T);
    launch_sliced(c, s.tiles, [&](long long t0, unsigned g) {
        hipLaunchKernelGGL(k_vmap_commit, dim3(g), dim3(BLOCK), 0, c->stream, v.tb, v.rec, s.where, first_created, epoch, T, t0,
                           s.scan.s[1].off, s.scan.s[1].boff, st.at, st.d_offsets, d_tags, n, d_upd);
    });
    HIP_TRY(hipGetLastError());
    if (stage_upd && updated)
        HIP_TRY(hipMemcpyAsync(upd_dst, d_upd, 4 * (size_t)updated, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    v.M += created;
    v.points += T - dropped;
    v.dropped += dropped;
    v.calls++;
    if (delta) delta->created = created, delta->updated = updated, delta->dropped = dropped;
    return SDM_OK;
}

int sdm_vmap_fetch(sdm_ctx* c, const unsigned* ids, long long first, long long count, sdm_point_buffers* out,
                   sdm_vmap_fields* extra)
{
    if (!c || !out) return fail(SDM_EINVAL, "null argument");
    sdm_ctx::Vmap& v = c->vmap;
    if (!v.open) return fail(SDM_ESTATE, "no open voxel map");
    int* tag = extra ? extra->tag : nullptr;
    unsigned* mult = extra ? extra->multiplicity : nullptr;
    unsigned* epoch = extra ? extra->epoch : nullptr;
    if (!out->xyz && !out->pixel && !out->rho_sigma && !out->intensity && !tag && !mult && !epoch)
        return fail(SDM_EINVAL, "no output requested");
    const bool dev = out->on_device != 0;
    int rc = fetch_check(v, ids, first, count, out->capacity, dev);
    if (rc) return rc;
    if (dev && (((uintptr_t)out->xyz | (uintptr_t)out->pixel | (uintptr_t)tag | (uintptr_t)mult | (uintptr_t)epoch | (uintptr_t)ids) % 4 ||
                (uintptr_t)out->rho_sigma % 8))
        return fail(SDM_EINVAL, "device buffer not aligned (xyz, pixel, tag, multiplicity, epoch, ids: 4 B; rho_sigma: 8 B)");
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (count == 0) return SDM_OK;
    const size_t m = (size_t)count;
    const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    VmapRecords src = v.rec;
    FetchIds f;
    if (!ids) {
        const size_t at = (size_t)first;
        src.xyz += 3 * at, src.pixel += at, src.rho_sigma += at, src.intensity += at, src.tag += at, src.multiplicity += at, src.epoch += at;
    } else {
        VmapRecords dst{};
        if (dev) {
            dst.xyz = out->xyz, dst.pixel = out->pixel, dst.rho_sigma = reinterpret_cast<float2*>(out->rho_sigma);
            dst.intensity = out->intensity, dst.tag = tag, dst.multiplicity = mult, dst.epoch = epoch;
        }
        if ((rc = fetch_stage_ids(c, ids, m, dev, [&](Carver& k) {
                 if (out->xyz) dst.xyz = k.take<float>(3 * m);
                 if (out->pixel) dst.pixel = k.take<unsigned>(m);
                 if (out->rho_sigma) dst.rho_sigma = k.take<float2>(m);
                 if (out->intensity) dst.intensity = k.take<unsigned char>(m);
                 if (tag) dst.tag = k.take<int>(m);
                 if (mult) dst.multiplicity = k.take<unsigned>(m);
                 if (epoch) dst.epoch = k.take<unsigned>(m);
             }, &f)))
            return rc;
        launch_sliced(c, (count + BLOCK - 1) / BLOCK, [&](long long b0, unsigned g) {
            hipLaunchKernelGGL(k_vmap_gather, dim3(g), dim3(BLOCK), 0, c->stream, v.rec, f.d_ids, count, b0 * BLOCK, (unsigned)v.M, dst,
                               f.d_bad);
        });
        if ((rc = fetch_read_bad(c, f))) return rc;
        src = dst;
    }
    if (!ids || !dev) {  // one copy per field of exactly count elements
        if (out->xyz) HIP_TRY(hipMemcpyAsync(out->xyz, src.xyz, 12 * m, kind, c->stream));
        if (out->pixel) HIP_TRY(hipMemcpyAsync(out->pixel, src.pixel, 4 * m, kind, c->stream));
        if (out->rho_sigma) HIP_TRY(hipMemcpyAsync(out->rho_sigma, src.rho_sigma, 8 * m, kind, c->stream));
        if (out->intensity) HIP_TRY(hipMemcpyAsync(out->intensity, src.intensity, m, kind, c->stream));
        if (tag) HIP_TRY(hipMemcpyAsync(tag, src.tag, 4 * m, kind, c->stream));
        if (mult) HIP_TRY(hipMemcpyAsync(mult, src.multiplicity, 4 * m, kind, c->stream));
        if (epoch) HIP_TRY(hipMemcpyAsync(epoch, src.epoch, 4 * m, kind, c->stream));
    }
    return fetch_finish(c, f);
}

// ---- free-space evidence on the persistent voxel map (sdm_vmap_carve.h) --------------------------------------------------
int sdm_vmap_carve(sdm_ctx* c, int n, const int* slots, int n_nbr, const int* nbr_slots, int source, double max_sigma,
                   double min_rho, sdm_vmap_carve_args* cv)
{
    if (cv) cv->plain_total = cv->rays_total = cv->rays_skipped = cv->cells_visited = cv->cells_hit = cv->ends_hit = 0;
    if (!c || !cv) return fail(SDM_EINVAL, "null argument");
    sdm_ctx::Vmap& v = c->vmap;
    if (!v.open) return fail(SDM_ESTATE, "no open voxel map");
    if (n < 0) return fail(SDM_EINVAL, "null or negative slot list");
    if (cv->end_margin < 0) return fail(SDM_EINVAL, "negative end_margin");
    if (cv->max_steps < 1 || cv->max_steps > SDM_FREESPACE_MAX_STEPS)
        return fail(SDM_EINVAL, "max_steps outside 1 .. SDM_FREESPACE_MAX_STEPS");
    if (n_nbr < 0) return fail(SDM_EINVAL, "negative n_nbr");
    if (n_nbr > c->cfg.max_neighbours) return fail(SDM_EINVAL, "n_nbr exceeds max_neighbours");
    if ((n_nbr == 0) != (nbr_slots == nullptr))
        return fail(SDM_EINVAL, n_nbr ? "null nbr_slots" : "n_nbr == 0 with a neighbour table");

    // the plain cloud (xyz and rho_sigma) and, with neighbours, the support words into the engine's staging
    ExtractStaged st{};
    st.support = n_nbr > 0;
    sdm_point_buffers none{};
    std::vector<long long> plain((size_t)n + 1, 0);
    int rc = extract_core(c, n, slots, n_nbr, nbr_slots, source, max_sigma, min_rho, &none, nullptr, plain.data(), &st);
    if (rc) return rc;
    const long long T = st.total;
    cv->plain_total = T;
    if (T == 0) return SDM_OK;  // (extract_core has waited for the stream)

    // the cameras of the call: its distinct slots in ascending order, and per slot i the distinct neighbours other than
    // slots[i], in the order of their first column, each with the mask of the columns that name it (extract_core has
    // checked every slot's range; n_nbr <= 64)
    const CallCameras cam = call_cameras(c, n, slots, n_nbr, nbr_slots);
    std::vector<std::vector<std::pair<int, unsigned long long>>> lists((size_t)n);
    int D = 0;
    for (int i = 0; i < n; i++) {
        auto& l = lists[(size_t)i];
        for (int j = 0; j < n_nbr; j++) {
            const int s = nbr_slots[(size_t)i * (size_t)n_nbr + (size_t)j];
            if (s == slots[i]) continue;
            size_t k = 0;
            while (k < l.size() && l[k].first != s) k++;
            if (k == l.size()) l.emplace_back(s, 0ull);
            l[k].second |= 1ull << j;
        }
        D = std::max(D, (int)l.size());
    }

    // the counters, the scratch and the pinned mirror: everything is allocated before anything is counted
    if (!v.d_evid) {
        DevBlock evid;
        unsigned long long *cr = nullptr, *en = nullptr;
        if ((rc = vmap_make_evidence(c, v.rec_cap, evid, &cr, &en))) return rc;
        evid.install(v.d_evid);
        v.crossings = cr, v.ends = en;
    }
    // the totals at +256 of the scratch's head and of the pinned mirror's; behind each head the same table, which goes over
    // in one copy: the centres | per slot its own camera | per slot and list place the camera | and its columns
    const size_t nd = (size_t)n * (size_t)D;
    struct Table { float* org; int *own, *cam; unsigned long long* mask; size_t bytes; } ht{}, dt{};
    const auto table = [&](Carver& k, Table& t) {
        const size_t first = k.at;
        t.org = k.take<float>(4 * (size_t)cam.Cn);
        t.own = k.take<int>((size_t)n);
        t.cam = k.take<int>(nd);
        t.mask = k.take<unsigned long long>(nd);
        t.bytes = k.at - first;
    };
    ScratchHead head;
    unsigned long long* h_tot = nullptr;
    if ((rc = carve_scratch(&v.d_scratch, &v.scratch_bytes, [&](Carver& k) { head = ScratchHead(k), table(k, dt); })) ||
        (rc = carve_scratch(&v.h_pin, &v.pin_bytes, [&](Carver& k) { h_tot = k.take<unsigned long long>(32), table(k, ht); },
                            ext_grow_host)))
        return rc;
    for (int q = 0; q < cam.Cn; q++) slot_centre(c, cam.slot_of_cam[(size_t)q], ht.org + 4 * q);
    for (int i = 0; i < n; i++) {
        ht.own[i] = cam.cam_of[(size_t)slots[i]];
        const auto& l = lists[(size_t)i];
        for (int d = 0; d < D; d++) {
            const bool have = (size_t)d < l.size();
            ht.cam[(size_t)i * (size_t)D + (size_t)d] = have ? cam.cam_of[(size_t)l[(size_t)d].first] : 0;
            ht.mask[(size_t)i * (size_t)D + (size_t)d] = have ? l[(size_t)d].second : 0ull;
        }
    }
    HIP_TRY(hipMemsetAsync(head.tot, 0, 64, c->stream));
    HIP_TRY(stage_in(c, dt.org, ht.org, dt.bytes));
    const VmapCarveIn in{st.at.xyz, D ? st.d_support : nullptr, st.d_offsets, dt.own, dt.cam, dt.mask, dt.org, T, n, D, (unsigned)v.M,
                         v.voxel_size, v.inv, cv->end_margin, cv->max_steps};
    const long long E = ((long long)D + 1) * T;  // candidates, camera-major
    launch_sliced(c, (E + BLOCK - 1) / BLOCK, [&](long long b0, unsigned g) {
        hipLaunchKernelGGL(k_vmap_carve, dim3(g), dim3(BLOCK), 0, c->stream, in, b0 * BLOCK, E, v.tb, v.crossings, v.ends, head.tot);
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_tot, head.tot, 40, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // the second wait: the end, with the totals
    cv->rays_total = (long long)h_tot[0];
    cv->rays_skipped = (long long)h_tot[1];
    cv->cells_visited = (long long)h_tot[2];
    cv->cells_hit = (long long)h_tot[3];
    cv->ends_hit = (long long)h_tot[4];
    return SDM_OK;
}

int sdm_vmap_fetch_evidence(sdm_ctx* c, const unsigned* ids, long long first, long long count, sdm_vmap_evidence* ev)
{
    if (!c || !ev) return fail(SDM_EINVAL, "null argument");
    sdm_ctx::Vmap& v = c->vmap;
    if (!v.open) return fail(SDM_ESTATE, "no open voxel map");
    if (!ev->crossings && !ev->ends) return fail(SDM_EINVAL, "no output requested");
    const bool dev = ev->on_device != 0;
    int rc = fetch_check(v, ids, first, count, ev->capacity, dev);
    if (rc) return rc;
    if (dev && (((uintptr_t)ev->crossings | (uintptr_t)ev->ends) % 8 || (uintptr_t)ids % 4))
        return fail(SDM_EINVAL, "device buffer not aligned (crossings, ends: 8 B; ids: 4 B)");
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (count == 0) return SDM_OK;
    const size_t m = (size_t)count;
    const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    const unsigned long long *src_cr = v.crossings, *src_en = v.ends;  // (null: no carve has run, every counter reads 0)
    FetchIds f;
    if (!ids) {
        if (src_cr) src_cr += first, src_en += first;
    } else {
        unsigned long long *dst_cr = ev->crossings, *dst_en = ev->ends;
        if ((rc = fetch_stage_ids(c, ids, m, dev, [&](Carver& k) {  // (both regions, whichever is asked for)
                 unsigned long long *cr = k.take<unsigned long long>(m), *en = k.take<unsigned long long>(m);
                 dst_cr = ev->crossings ? cr : nullptr, dst_en = ev->ends ? en : nullptr;
             }, &f)))
            return rc;
        launch_sliced(c, (count + BLOCK - 1) / BLOCK, [&](long long b0, unsigned g) {
            hipLaunchKernelGGL(k_vmap_evidence, dim3(g), dim3(BLOCK), 0, c->stream, src_cr, src_en, f.d_ids, count, b0 * BLOCK,
                               (unsigned)v.M, dst_cr, dst_en, f.d_bad);
        });
        if ((rc = fetch_read_bad(c, f))) return rc;
        src_cr = dst_cr, src_en = dst_en;
    }
    if (!ids || !dev) {  // one copy per counter of exactly count elements (zeros before the first carve)
        unsigned long long* dst[2] = {ev->crossings, ev->ends};
        const unsigned long long* src[2] = {src_cr, src_en};
        for (int k = 0; k < 2; k++) {
            if (!dst[k]) continue;
            if (src[k]) HIP_TRY(hipMemcpyAsync(dst[k], src[k], 8 * m, kind, c->stream));
            else if (dev) HIP_TRY(hipMemsetAsync(dst[k], 0, 8 * m, c->stream));
            else std::memset(dst[k], 0, 8 * m);
        }
    }
    return fetch_finish(c, f);
}

// ---- camera lists on the persistent voxel map: the observation log (sdm_vmap_obs.h) --------------------------------------
// set, log and per-entry arrays for `need` observations, made before anything is inserted; the old ones stay intact if
// an allocation fails
static int vobs_grow(sdm_ctx* c, long long need)
{
    sdm_ctx::Vmap& v = c->vmap;
    sdm_ctx::Vmap::Obs& o = v.obs;
    int rc;
    if (!o.d_ent) {
        DevBlock ent;
        unsigned *last_obs = nullptr, *ncam = nullptr;
        if ((rc = vmap_make_obs_entries(c, v.rec_cap, ent, &last_obs, &ncam))) return rc;
        ent.install(o.d_ent);
        o.last_obs = last_obs, o.ncam = ncam;
    }
    if (!o.d_table || 2ull * (unsigned long long)need > o.cap) {
        unsigned long long cap = std::max(o.cap, 1024ull);
        while (cap < 2ull * (unsigned long long)need) cap <<= 1;
        DevBlock block;
        VobsTable nw{};
        if ((rc = vobs_make_table(c, cap, block, &nw))) return rc;
        if (o.d_table) {
            unsigned* d_flag = reinterpret_cast<unsigned*>(o.d_scratch);  // (the caller has sized the scratch)
            unsigned* h_flag = reinterpret_cast<unsigned*>(o.h_pin);
            hipError_t e = hipMemsetAsync(d_flag, 0, 4, c->stream);
            if (e == hipSuccess) {
                launch_sliced(c, (long long)((o.cap + BLOCK - 1) / BLOCK), [&](long long b0, unsigned g) {
                    hipLaunchKernelGGL(k_vobs_rehash, dim3(g), dim3(BLOCK), 0, c->stream, o.tb.keys, o.tb.idx, o.cap,
                                       (unsigned long long)b0 * BLOCK, nw, d_flag);
                });
                e = hipGetLastError();
            }
            if (e == hipSuccess) e = hipMemcpyAsync(h_flag, d_flag, 4, hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess || *h_flag)
                return fail(SDM_EHIP, e != hipSuccess ? std::string("observation set rehash: ") + hipGetErrorString(e)
                                                      : std::string("observation set overflow while rehashing"));
            o.rehashes++;
        }
        block.install(o.d_table);  // (the old set is freed only after the wait)
        o.tb = nw;
        o.cap = cap;
    }
    if (need > o.log_cap) {
        const long long cap = std::max(need, 2 * o.log_cap);  // geometric: the copies amortise
        const size_t b4 = ext_align(4 * (size_t)cap);
        DevBlock block;
        if ((rc = block.alloc(3 * b4))) return rc;
        VobsLog nl;
        nl.entry = reinterpret_cast<unsigned*>(block.p);
        nl.tag = reinterpret_cast<int*>(block.p + b4);
        nl.prev = reinterpret_cast<unsigned*>(block.p + 2 * b4);
        const size_t m = (size_t)o.E;
        hipError_t e = hipSuccess;
        if (m) {
            e = hipMemcpyAsync(nl.entry, o.log.entry, 4 * m, hipMemcpyDeviceToDevice, c->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(nl.tag, o.log.tag, 4 * m, hipMemcpyDeviceToDevice, c->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(nl.prev, o.log.prev, 4 * m, hipMemcpyDeviceToDevice, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        }
        if (e != hipSuccess) return fail(SDM_EHIP, std::string("observation log: ") + hipGetErrorString(e));
        block.install(o.d_log);
        o.log = nl;
        o.log_cap = cap;
    }
    return SDM_OK;
}

int sdm_vmap_observe(sdm_ctx* c, int n, const int* slots, const int* tags, int n_nbr, const int* nbr_slots, const int* nbr_tags,
                     int source, double max_sigma, double min_rho, sdm_vmap_observe_delta* ob)
{
    if (ob) ob->plain_total = ob->unmapped = ob->candidates = ob->first_created = ob->created = 0;
    if (!c || !ob) return fail(SDM_EINVAL, "null argument");
    sdm_ctx::Vmap& v = c->vmap;
    sdm_ctx::Vmap::Obs& o = v.obs;
    if (!v.open) return fail(SDM_ESTATE, "no open voxel map");
    if (n < 0 || (n > 0 && !slots)) return fail(SDM_EINVAL, "null or negative slot list");
    if (n_nbr < 0) return fail(SDM_EINVAL, "negative n_nbr");
    if (n_nbr > c->cfg.max_neighbours) return fail(SDM_EINVAL, "n_nbr exceeds max_neighbours");
    if ((n_nbr == 0) != (nbr_slots == nullptr))
        return fail(SDM_EINVAL, n_nbr ? "null nbr_slots" : "n_nbr == 0 with a neighbour table");
    if (nbr_tags && !nbr_slots) return fail(SDM_EINVAL, "nbr_tags without nbr_slots");
    const size_t nn = (size_t)n * (size_t)n_nbr;
    if (tags)
        for (int i = 0; i < n; i++)
            if (tags[i] < 0) return fail(SDM_EINVAL, "tag outside [0, 2^31)");
    if (nbr_tags)
        for (size_t i = 0; i < nn; i++)
            if (nbr_tags[i] < 0) return fail(SDM_EINVAL, "tag outside [0, 2^31)");

    // the plain cloud (xyz and rho_sigma) and, with neighbours, the support words into the engine's staging
    ExtractStaged st{};
    st.support = n_nbr > 0;
    sdm_point_buffers none{};
    std::vector<long long> plain((size_t)n + 1, 0);
    int rc = extract_core(c, n, slots, n_nbr, nbr_slots, source, max_sigma, min_rho, &none, nullptr, plain.data(), &st);
    if (rc) return rc;
    const long long T = st.total;
    ob->plain_total = T;

    // per row the ascending list of its distinct tags with the columns that name each; the own tag's position is always
    // live (extract_core has checked every slot's range, so a slot number is a valid tag; n_nbr <= 64)
    std::vector<std::vector<std::pair<int, unsigned long long>>> lists((size_t)n);
    std::vector<int> own((size_t)n, 0);
    int Lmax = 1;
    long long B = 0;
    for (int i = 0; i < n; i++) {
        auto& l = lists[(size_t)i];
        const int mine = tags ? tags[i] : slots[i];
        l.emplace_back(mine, 0ull);
        for (int j = 0; j < n_nbr; j++) {
            const size_t at = (size_t)i * (size_t)n_nbr + (size_t)j;
            const int t = nbr_tags ? nbr_tags[at] : nbr_slots[at];
            size_t k = 0;
            while (k < l.size() && l[k].first != t) k++;
            if (k == l.size()) l.emplace_back(t, 0ull);
            l[k].second |= 1ull << j;
        }
        std::sort(l.begin(), l.end());  // (the tags are distinct: the masks never decide)
        for (size_t k = 0; k < l.size(); k++)
            if (l[k].first == mine) own[(size_t)i] = (int)k;
        Lmax = std::max(Lmax, (int)l.size());
        B += (plain[(size_t)i + 1] - plain[(size_t)i]) * (long long)l.size();
    }
    if (o.E + B > (1ll << 30))
        return fail(SDM_EINVAL, "more than 2^30 observations and candidates: the observation set would exceed 2^31 slots");
    const long long Ec = T * (long long)Lmax;  // candidates, point-major
    if (Ec > (1ll << 40)) return fail(SDM_EINVAL, "more than 2^40 candidates (plain points x the longest row) in one call");
    if (T == 0) {  // (extract_core has waited for the stream)
        ob->first_created = o.E;
        o.calls++;
        return SDM_OK;
    }

    // scratch, pinned mirror and growth: everything is allocated before anything is inserted
    const size_t nl = (size_t)n * (size_t)Lmax;
    const size_t tag_b = ext_align(4 * nl), mask_b = ext_align(8 * nl), own_b = ext_align(4 * (size_t)n), tab_b = mask_b + tag_b + own_b;
    VobsScratch s;  // head.mid: {unmapped, candidates, overflow}; head.tot: {created, unmapped, candidates, overflow}
    unsigned char* d_tab = nullptr;
    if ((rc = carve_scratch(&o.d_scratch, &o.scratch_bytes, [&](Carver& k) {
             s = VobsScratch(k, Ec);
             d_tab = k.take<unsigned char>(tab_b);
         })))
        return rc;
    if ((rc = ext_grow_host(&o.h_pin, &o.pin_bytes, 256 + tab_b))) return rc;
    if ((rc = vobs_grow(c, o.E + B))) return rc;
    unsigned char* h_tab = o.h_pin + 256;
    unsigned long long* h_mask = reinterpret_cast<unsigned long long*>(h_tab);
    int* h_tag = reinterpret_cast<int*>(h_tab + mask_b);
    int* h_own = reinterpret_cast<int*>(h_tab + mask_b + tag_b);
    for (int i = 0; i < n; i++) {
        const auto& l = lists[(size_t)i];
        h_own[i] = own[(size_t)i];
        for (int d = 0; d < Lmax; d++) {
            const bool have = (size_t)d < l.size();
            h_tag[(size_t)i * (size_t)Lmax + (size_t)d] = have ? l[(size_t)d].first : 0;
            h_mask[(size_t)i * (size_t)Lmax + (size_t)d] = have ? l[(size_t)d].second : 0ull;
        }
    }
    HIP_TRY(hipMemsetAsync(s.head.mid, 0, 24, c->stream));
    HIP_TRY(hipMemcpyAsync(d_tab, h_tab, tab_b, hipMemcpyHostToDevice, c->stream));
    VobsIn in;
    in.xyz = st.at.xyz;
    in.support = n_nbr > 0 ? st.d_support : nullptr;
    in.plain_offsets = st.d_offsets;
    in.row_mask = reinterpret_cast<const unsigned long long*>(d_tab);
    in.row_tag = reinterpret_cast<const int*>(d_tab + mask_b);
    in.own = reinterpret_cast<const int*>(d_tab + mask_b + tag_b);
    in.T = T;
    in.n = n;
    in.Lmax = Lmax;
    in.inv = v.inv;
    launch_sliced(c, (Ec + BLOCK - 1) / BLOCK, [&](long long b0, unsigned g) {
        hipLaunchKernelGGL(k_vobs_insert, dim3(g), dim3(BLOCK), 0, c->stream, in, b0 * BLOCK, Ec, v.tb, o.tb, s.where, s.head.mid);
    });
    vobs_count(c, s, Ec);
    HIP_TRY(hipGetLastError());
    unsigned long long* h_tot = reinterpret_cast<unsigned long long*>(o.h_pin);
    HIP_TRY(hipMemcpyAsync(h_tot, s.head.tot, 32, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // the second wait: created
    if (h_tot[3]) return fail(SDM_EHIP, "observation set overflow");
    const long long created = (long long)h_tot[0];
    if (created > B) return fail(SDM_EHIP, "observation log: more pairs created than the a-priori bound");

    vobs_commit(c, s, (unsigned)o.E, Ec);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (const auto& l : lists)  // the tags seen so far bound every list's length (sdm_vmap_fetch_cameras' scan)
        for (const auto& tm : l) {
            const auto it = std::lower_bound(o.seen.begin(), o.seen.end(), tm.first);
            if (it == o.seen.end() || *it != tm.first) o.seen.insert(it, tm.first);
        }
    ob->unmapped = (long long)h_tot[1];
    ob->candidates = (long long)h_tot[2];
    ob->first_created = o.E;
    ob->created = created;
    o.E += created;
    o.calls++;
    return SDM_OK;
}

int sdm_vmap_get_obs_info(sdm_ctx* c, sdm_vmap_obs_info* info)
{
    if (!c || !info) return fail(SDM_EINVAL, "null argument");
    const sdm_ctx::Vmap& v = c->vmap;
    if (!v.open) return fail(SDM_ESTATE, "no open voxel map");
    std::memset(info, 0, sizeof(*info));
    info->observations = v.obs.E;
    info->calls = v.obs.calls;
    info->table_slots = (long long)v.obs.cap;
    info->rehashes = v.obs.rehashes;
    return SDM_OK;
}

int sdm_vmap_fetch_observations(sdm_ctx* c, long long first, long long count, sdm_vmap_observations* out)
{
    if (!c || !out) return fail(SDM_EINVAL, "null argument");
    sdm_ctx::Vmap& v = c->vmap;
    if (!v.open) return fail(SDM_ESTATE, "no open voxel map");
    if (!out->entry && !out->tag) return fail(SDM_EINVAL, "no output requested");
    if (count < 0 || out->capacity < 0) return fail(SDM_EINVAL, "negative count or capacity");
    if (count > out->capacity) return fail(SDM_EINVAL, "count exceeds capacity");
    if (first < 0 || first > v.obs.E || count > v.obs.E - first) return fail(SDM_EINVAL, "range beyond the log's observations");
    const bool dev = out->on_device != 0;
    if (dev && ((uintptr_t)out->entry | (uintptr_t)out->tag) % 4) return fail(SDM_EINVAL, "device buffer not aligned (entry, tag: 4 B)");
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (count == 0) return SDM_OK;
    const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (out->entry) HIP_TRY(hipMemcpyAsync(out->entry, v.obs.log.entry + first, 4 * (size_t)count, kind, c->stream));
    if (out->tag) HIP_TRY(hipMemcpyAsync(out->tag, v.obs.log.tag + first, 4 * (size_t)count, kind, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SDM_OK;
}

int sdm_vmap_fetch_cameras(sdm_ctx* c, const unsigned* ids, long long first, long long count, sdm_vmap_cameras* cams)
{
    if (cams) cams->cam_total = 0;
    if (!c || !cams) return fail(SDM_EINVAL, "null argument");
    sdm_ctx::Vmap& v = c->vmap;
    sdm_ctx::Vmap::Obs& o = v.obs;
    if (!v.open) return fail(SDM_ESTATE, "no open voxel map");
    if (!cams->cam_offsets && !cams->cam_tags) return fail(SDM_EINVAL, "no camera output requested");
    // (this one check of the call's own comes second among fetch_check's, where it has always been)
    if (count >= 0 && cams->capacity >= 0 && cams->cam_tags && cams->cam_capacity < 0) return fail(SDM_EINVAL, "negative cam_capacity");
    const bool dev = cams->on_device != 0;
    int rc = fetch_check(v, ids, first, count, cams->capacity, dev);
    if (rc) return rc;
    if (dev && ((uintptr_t)cams->cam_offsets % 8 || ((uintptr_t)cams->cam_tags | (uintptr_t)ids) % 4))
        return fail(SDM_EINVAL, "device buffer not aligned (cam_offsets: 8 B; cam_tags, ids: 4 B)");
    if ((unsigned long long)std::min(count, (long long)EXT_SCAN) * (unsigned long long)o.seen.size() >= (1ull << 32))
        return fail(SDM_EINVAL, "min(count, 2048) x (distinct tags observed) >= 2^32: the list pass scans 32-bit sums");
    HIP_TRY(hipSetDevice(c->cfg.device));

    // ids, lengths, the scan's arrays and -- for host destinations -- the offsets; the tags' staging follows the total
    const size_t m = (size_t)count;
    unsigned* d_ids_own = nullptr;
    Scan len;  // (cnt: the lists' lengths, one "tile" per requested entry)
    long long* d_offs_own = nullptr;
    if ((rc = carve_scratch(&o.d_scratch, &o.scratch_bytes,
                            [&](Carver& k) {
                                k.take<unsigned char>(256);  // {bad, -, total}
                                d_ids_own = k.take<unsigned>(m);
                                len = Scan(k, count);
                                d_offs_own = k.take<long long>(m + 1);
                            })) ||
        (rc = ext_grow_host(&o.h_pin, &o.pin_bytes, 256)))
        return rc;
    unsigned* d_bad = reinterpret_cast<unsigned*>(o.d_scratch);
    unsigned long long* d_total = reinterpret_cast<unsigned long long*>(o.d_scratch + 8);
    long long* d_offs = dev ? cams->cam_offsets : cams->cam_offsets ? d_offs_own : nullptr;
    const unsigned* d_ids = ids;
    if (ids && !dev && count) {
        HIP_TRY(hipMemcpyAsync(d_ids_own, ids, 4 * m, hipMemcpyHostToDevice, c->stream));
        d_ids = d_ids_own;
    }
    HIP_TRY(hipMemsetAsync(o.d_scratch, 0, 16, c->stream));
    const long long blocks = (count + BLOCK - 1) / BLOCK, oblocks = (count + 1 + BLOCK - 1) / BLOCK;
    launch_sliced(c, blocks, [&](long long b0, unsigned g) {
        hipLaunchKernelGGL(k_vobs_list_count, dim3(g), dim3(BLOCK), 0, c->stream, o.ncam, d_ids, first, count, b0 * BLOCK,
                           (unsigned)v.M, len.cnt, d_bad);
    });
    scan_counts(c, len, count);
    // (the offsets go to a caller's device array only once the total is known to fit: the scan's arrays serve until then)
    hipLaunchKernelGGL(k_vobs_list_offsets, dim3(1), dim3(BLOCK), 0, c->stream, len.off, len.boff, count, count, (long long*)nullptr,
                       d_total);
    HIP_TRY(hipGetLastError());
    unsigned long long* h_tot = reinterpret_cast<unsigned long long*>(o.h_pin);
    HIP_TRY(hipMemcpyAsync(h_tot, o.d_scratch, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // the first wait: the lists' total
    if ((unsigned)h_tot[0]) return fail(SDM_EINVAL, "id beyond the map's entries");
    const long long total = (long long)h_tot[1];
    cams->cam_total = total;
    if (cams->cam_tags && total > cams->cam_capacity)
        return fail(SDM_EINVAL, "cam_capacity " + std::to_string(cams->cam_capacity) + " < " + std::to_string(total) +
                                    " list entries (cam_total filled)");
    int* d_tags = cams->cam_tags;
    if (cams->cam_tags && !dev && total) {
        if ((rc = ext_grow_dev(&o.d_out, &o.out_bytes, 4 * (size_t)total))) return rc;
        d_tags = reinterpret_cast<int*>(o.d_out);
    }
    if (d_offs)
        launch_sliced(c, oblocks, [&](long long b0, unsigned g) {
            hipLaunchKernelGGL(k_vobs_list_offsets, dim3(g), dim3(BLOCK), 0, c->stream, len.off, len.boff, count, b0 * BLOCK, d_offs,
                               d_total);
        });
    if (cams->cam_tags && total)
        launch_sliced(c, blocks, [&](long long b0, unsigned g) {
            hipLaunchKernelGGL(k_vobs_list_fill, dim3(g), dim3(BLOCK), 0, c->stream, o.log, o.last_obs, d_ids, first, count,
                               b0 * BLOCK, (unsigned)v.M, len.cnt, len.off, len.boff, d_tags);
        });
    HIP_TRY(hipGetLastError());
    if (!dev) {
        if (cams->cam_offsets) HIP_TRY(hipMemcpyAsync(cams->cam_offsets, d_offs, 8 * (m + 1), hipMemcpyDeviceToHost, c->stream));
        if (cams->cam_tags && total) HIP_TRY(hipMemcpyAsync(cams->cam_tags, d_tags, 4 * (size_t)total, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SDM_OK;
}

// ---- classification on the persistent voxel map (sdm_vmap_class.h) --------------------------------------------------------
int sdm_vmap_classify(sdm_ctx* c, const sdm_vmap_rule* rule, int commit, sdm_vmap_class_delta* delta)
{
    if (delta) delta->examined = delta->accepted = delta->retracted = delta->published_total = 0;
    if (!c || !rule || !delta) return fail(SDM_EINVAL, "null argument");
    sdm_ctx::Vmap& v = c->vmap;
    if (!v.open) return fail(SDM_ESTATE, "no open voxel map");
    if (rule->ratio_den == 0) return fail(SDM_EINVAL, "ratio_den must be at least 1");
    if (rule->min_neighbours < 0 || rule->min_neighbours > 26) return fail(SDM_EINVAL, "min_neighbours outside 0 .. 26");
    unsigned* acc_dst = delta->accepted_ids;
    unsigned* ret_dst = delta->retracted_ids;
    if ((acc_dst && delta->accepted_capacity < 0) || (ret_dst && delta->retracted_capacity < 0))
        return fail(SDM_EINVAL, "negative capacity");
    const bool dev = delta->on_device != 0;
    if (dev && ((uintptr_t)acc_dst | (uintptr_t)ret_dst) % 4)
        return fail(SDM_EINVAL, "device buffer not aligned (accepted_ids, retracted_ids: 4 B)");
    HIP_TRY(hipSetDevice(c->cfg.device));

    // the flags, the scratch and the pinned totals: everything but the id staging, which follows the counts
    const long long M = v.M;
    const long long vt = ext_tiles(M);
    ScratchHead head;  // tot: {accepted, retracted, published_total}
    unsigned char* d_flag = nullptr;
    ScanPair scan;  // [0] accepted, [1] retracted (sized for at least one entry and tile: M may be 0)
    int rc;
    if ((rc = carve_scratch(&v.d_scratch, &v.scratch_bytes, [&](Carver& k) {
             head = ScratchHead(k);
             d_flag = k.take<unsigned char>((size_t)std::max(M, 1ll));
             scan = ScanPair(k, vt, std::max(vt, 1ll));
         })))
        return rc;
    if ((rc = ext_grow_host(&v.h_pin, &v.pin_bytes, 256))) return rc;
    if (!v.cls.d_pub) {
        DevBlock pub;
        if ((rc = vmap_make_published(c, v.rec_cap, pub))) return rc;
        pub.install(v.cls.d_pub);
    }
    delta->examined = M;
    delta->published_total = v.cls.published;
    if (M == 0) {  // nothing to examine
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (commit) v.cls.calls++;
        return SDM_OK;
    }
    const Scan &acc = scan.s[0], &ret = scan.s[1];

    VclsRule r;
    r.min_multiplicity = rule->min_multiplicity;
    r.min_cameras = rule->min_cameras;
    r.min_ends = rule->min_ends;
    r.ratio_num = rule->ratio_num;
    r.ratio_den = rule->ratio_den;
    unsigned bits;
    std::memcpy(&bits, &rule->max_sigma, 4);
    r.max_sigma_key = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);  // f2key
    r.min_neighbours = rule->min_neighbours;
    VclsIn in;
    in.multiplicity = v.rec.multiplicity;
    in.rho_sigma = v.rec.rho_sigma;
    in.ncam = v.obs.ncam;
    in.crossings = v.crossings;
    in.ends = v.ends;
    launch_sliced(c, (M + BLOCK - 1) / BLOCK, [&](long long b0, unsigned g) {
        hipLaunchKernelGGL(k_vcls_local, dim3(g), dim3(BLOCK), 0, c->stream, in, r, M, b0 * BLOCK, d_flag);
    });
    launch_sliced(c, vt, [&](long long t0, unsigned g) {
        hipLaunchKernelGGL(k_vcls_count, dim3(g), dim3(BLOCK), 0, c->stream, v.tb, v.rec.xyz, v.inv, r.min_neighbours, M, t0, d_flag,
                           v.cls.d_pub, acc.cnt, ret.cnt);
    });
    scan_counts(c, acc, vt);
    scan_counts(c, ret, vt);
    hipLaunchKernelGGL(k_vcls_totals, dim3(1), dim3(64), 0, c->stream, vt, acc.off, acc.boff, ret.off, ret.boff,
                       (unsigned long long)v.cls.published, commit, head.tot);
    HIP_TRY(hipGetLastError());
    unsigned long long* h_tot = reinterpret_cast<unsigned long long*>(v.h_pin);
    HIP_TRY(hipMemcpyAsync(h_tot, head.tot, 24, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // the one wait for the counts
    const long long accepted = (long long)h_tot[0], retracted = (long long)h_tot[1];
    delta->accepted = accepted;
    delta->retracted = retracted;
    if (acc_dst && accepted > delta->accepted_capacity)
        return fail(SDM_EINVAL, "accepted_capacity " + std::to_string(delta->accepted_capacity) + " < " + std::to_string(accepted) +
                                    " accepted entries (the counts are filled)");
    if (ret_dst && retracted > delta->retracted_capacity)
        return fail(SDM_EINVAL, "retracted_capacity " + std::to_string(delta->retracted_capacity) + " < " + std::to_string(retracted) +
                                    " retracted entries (the counts are filled)");
    const bool list_acc = acc_dst && accepted, list_ret = ret_dst && retracted;
    if (commit ? accepted + retracted > 0 : (list_acc || list_ret)) {
        unsigned *d_acc = list_acc ? acc_dst : nullptr, *d_ret = list_ret ? ret_dst : nullptr;
        const size_t acc_b = list_acc ? ext_align(4 * (size_t)accepted) : 0;
        if (!dev && (list_acc || list_ret)) {  // (no flag has changed yet: a failure here leaves the state as it was)
            if ((rc = ext_grow_dev(&v.d_out, &v.out_bytes, acc_b + 4 * (size_t)(list_ret ? retracted : 0)))) return rc;
            if (list_acc) d_acc = reinterpret_cast<unsigned*>(v.d_out);
            if (list_ret) d_ret = reinterpret_cast<unsigned*>(v.d_out + acc_b);
        }
        launch_sliced(c, vt, [&](long long t0, unsigned g) {
            hipLaunchKernelGGL(k_vcls_commit, dim3(g), dim3(BLOCK), 0, c->stream, d_flag, v.cls.d_pub, commit, M, t0, acc.off, acc.boff,
                               ret.off, ret.boff, d_acc, d_ret);
        });
        HIP_TRY(hipGetLastError());
        if (!dev) {
            if (list_acc) HIP_TRY(hipMemcpyAsync(acc_dst, d_acc, 4 * (size_t)accepted, hipMemcpyDeviceToHost, c->stream));
            if (list_ret) HIP_TRY(hipMemcpyAsync(ret_dst, d_ret, 4 * (size_t)retracted, hipMemcpyDeviceToHost, c->stream));
        }
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (commit) {
        v.cls.published = (long long)h_tot[2];
        v.cls.calls++;
    }
    delta->published_total = v.cls.published;
    return SDM_OK;
}

int sdm_vmap_get_class_info(sdm_ctx* c, sdm_vmap_class_info* info)
{
    if (!c || !info) return fail(SDM_EINVAL, "null argument");
    const sdm_ctx::Vmap& v = c->vmap;
    if (!v.open) return fail(SDM_ESTATE, "no open voxel map");
    std::memset(info, 0, sizeof(*info));
    info->published = v.cls.published;
    info->calls = v.cls.calls;
    return SDM_OK;
}

int sdm_vmap_fetch_published(sdm_ctx* c, const unsigned* ids, long long first, long long count, sdm_vmap_published* out)
{
    if (!c || !out) return fail(SDM_EINVAL, "null argument");
    sdm_ctx::Vmap& v = c->vmap;
    if (!v.open) return fail(SDM_ESTATE, "no open voxel map");
    if (!out->published) return fail(SDM_EINVAL, "no output requested");
    const bool dev = out->on_device != 0;
    int rc = fetch_check(v, ids, first, count, out->capacity, dev);
    if (rc) return rc;
    if (dev && (uintptr_t)ids % 4) return fail(SDM_EINVAL, "device buffer not aligned (ids: 4 B)");
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (count == 0) return SDM_OK;
    const size_t m = (size_t)count;
    const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    const unsigned char* src = v.cls.d_pub;  // (null: no classify has run, every flag reads 0)
    FetchIds f;
    if (!ids) {
        if (src) src += first;
    } else {
        unsigned char* dst = out->published;
        if ((rc = fetch_stage_ids(c, ids, m, dev, [&](Carver& k) { dst = k.take<unsigned char>(m); }, &f))) return rc;
        launch_sliced(c, (count + BLOCK - 1) / BLOCK, [&](long long b0, unsigned g) {
            hipLaunchKernelGGL(k_vcls_gather, dim3(g), dim3(BLOCK), 0, c->stream, src, f.d_ids, count, b0 * BLOCK, (unsigned)v.M, dst,
                               f.d_bad);
        });
        if ((rc = fetch_read_bad(c, f))) return rc;
        src = dst;
    }
    if (!ids || !dev) {  // one copy of exactly count flags (zeros before the first classify)
        if (src) HIP_TRY(hipMemcpyAsync(out->published, src, m, kind, c->stream));
        else if (dev) HIP_TRY(hipMemsetAsync(out->published, 0, m, c->stream));
        else std::memset(out->published, 0, m);
    }
    return fetch_finish(c, f);
}

// ---- importing records and observations into the persistent voxel map (sdm_vmap_import.h) --------------------------------
int sdm_vmap_import(sdm_ctx* c, const sdm_point_buffers* src, const sdm_vmap_fields* extra, long long count,
                    sdm_vmap_import_delta* delta)
{
    if (delta) delta->total = delta->dropped = delta->first_created = delta->created = delta->updated = 0;
    if (!c || !src) return fail(SDM_EINVAL, "null argument");
    sdm_ctx::Vmap& v = c->vmap;
    if (!v.open) return fail(SDM_ESTATE, "no open voxel map");
    if (count < 0 || src->capacity < 0) return fail(SDM_EINVAL, "negative count or capacity");
    if (count > src->capacity) return fail(SDM_EINVAL, "count exceeds capacity");
    if (count > 0 && (!src->xyz || !src->rho_sigma)) return fail(SDM_EINVAL, "null source (xyz and rho_sigma are required)");
    const int* s_tag = extra ? extra->tag : nullptr;
    const unsigned* s_mult = extra ? extra->multiplicity : nullptr;
    const bool dev = src->on_device != 0;
    if (dev && (((uintptr_t)src->xyz | (uintptr_t)src->pixel | (uintptr_t)s_tag | (uintptr_t)s_mult) % 4 || (uintptr_t)src->rho_sigma % 8))
        return fail(SDM_EINVAL, "device buffer not aligned (xyz, pixel, tag, multiplicity: 4 B; rho_sigma: 8 B)");
    unsigned* ids_dst = delta ? delta->dst_ids : nullptr;
    unsigned* upd_dst = delta ? delta->updated_ids : nullptr;
    if (upd_dst && delta->updated_capacity < 0) return fail(SDM_EINVAL, "negative capacity");
    if (delta && delta->on_device && ((uintptr_t)ids_dst | (uintptr_t)upd_dst) % 4)
        return fail(SDM_EINVAL, "device buffer not aligned (dst_ids, updated_ids: 4 B)");
    const long long R = count;
    if (delta) delta->total = R, delta->first_created = v.M;
    if (v.M + R > (1ll << 30)) return fail(SDM_EINVAL, "more than 2^30 entries and records: the voxel map's table would exceed 2^31 slots");
    if (upd_dst && delta->updated_capacity < std::min(v.M, R))
        return fail(SDM_EINVAL, "updated_capacity " + std::to_string(delta->updated_capacity) + " < min(entries, records) = " +
                                    std::to_string(std::min(v.M, R)) + " (total and first_created filled)");
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (R == 0) {
        v.calls++;
        return SDM_OK;
    }

    // scratch, the staging of host sources and destinations, and growth: everything is allocated before anything is inserted
    const size_t m = (size_t)R;
    VmapScratch s;
    VimpSrc in{};  // the source on the device: the caller's arrays, or their staging behind the scratch
    if (dev) {
        in.xyz = src->xyz, in.rho_sigma = reinterpret_cast<const float2*>(src->rho_sigma), in.pixel = src->pixel;
        in.intensity = src->intensity, in.tag = s_tag, in.multiplicity = s_mult;
    }
    int rc;
    if ((rc = carve_scratch(&v.d_scratch, &v.scratch_bytes, [&](Carver& k) {
             s = VmapScratch(k, R);
             if (dev) return;
             in.xyz = k.take<float>(3 * m);
             in.rho_sigma = k.take<float2>(m);
             if (src->pixel) in.pixel = k.take<unsigned>(m);
             if (src->intensity) in.intensity = k.take<unsigned char>(m);
             if (s_tag) in.tag = k.take<int>(m);
             if (s_mult) in.multiplicity = k.take<unsigned>(m);
         })))
        return rc;
    if ((rc = ext_grow_host(&v.h_pin, &v.pin_bytes, 256))) return rc;
    const bool stage_out = delta && !delta->on_device;
    const size_t ids_b = stage_out && ids_dst ? ext_align(4 * m) : 0;
    if (stage_out && (ids_dst || upd_dst) && (rc = ext_grow_dev(&v.d_out, &v.out_bytes, ids_b + 4 * (size_t)std::min(v.M, R) + 4))) return rc;
    if ((rc = vmap_grow(c, v.M + R))) return rc;
    unsigned long long* h_tot = reinterpret_cast<unsigned long long*>(v.h_pin);  // {created, updated, dropped, overflow, sum of m_r}
    if (!dev) {
        HIP_TRY(stage_in(c, in.xyz, src->xyz, 12 * m));
        HIP_TRY(stage_in(c, in.rho_sigma, src->rho_sigma, 8 * m));
        if (src->pixel) HIP_TRY(stage_in(c, in.pixel, src->pixel, 4 * m));
        if (src->intensity) HIP_TRY(stage_in(c, in.intensity, src->intensity, m));
        if (s_tag) HIP_TRY(stage_in(c, in.tag, s_tag, 4 * m));
        if (s_mult) HIP_TRY(stage_in(c, in.multiplicity, s_mult, 4 * m));
    }

    HIP_TRY(hipMemsetAsync(s.head.ctr, 0, 8, c->stream));
    HIP_TRY(hipMemsetAsync(s.head.tot + 4, 0, 8, c->stream));
    const long long pblocks = (R + BLOCK - 1) / BLOCK;
    launch_sliced(c, pblocks, [&](long long b0, unsigned g) {
        hipLaunchKernelGGL(k_vimp_insert, dim3(g), dim3(BLOCK), 0, c->stream, in, R, b0 * BLOCK, v.inv, v.tb, s.where, s.head.ctr,
                           s.head.tot + 4);
    });
    if ((rc = vmap_count_and_total(c, v.rec, s, R, 40))) return rc;  // the first wait: created and updated
    const long long created = (long long)h_tot[0], updated = (long long)h_tot[1], dropped = (long long)h_tot[2];
    const long long stored = (long long)h_tot[4];

    unsigned* d_ids = !ids_dst ? nullptr : stage_out ? reinterpret_cast<unsigned*>(v.d_out) : ids_dst;
    unsigned* d_upd = !upd_dst ? nullptr : stage_out ? reinterpret_cast<unsigned*>(v.d_out + ids_b) : upd_dst;
    const unsigned first_created = (unsigned)v.M, epoch = (unsigned)(v.calls + 1);
    vmap_assign_ids(c, v.rec, s, first_created, R);
    launch_sliced(c, s.tiles, [&](long long t0, unsigned g) {
        hipLaunchKernelGGL(k_vimp_commit, dim3(g), dim3(BLOCK), 0, c->stream, v.tb, v.rec, s.where, first_created, R, t0,
                           s.scan.s[1].off, s.scan.s[1].boff, d_upd);
    });
    launch_sliced(c, pblocks, [&](long long b0, unsigned g) {
        hipLaunchKernelGGL(k_vimp_write, dim3(g), dim3(BLOCK), 0, c->stream, v.tb, v.rec, s.where, first_created, epoch, R, b0 * BLOCK,
                           in, d_ids, (const unsigned*)nullptr);
    });
    HIP_TRY(hipGetLastError());
    if (stage_out && ids_dst) HIP_TRY(hipMemcpyAsync(ids_dst, d_ids, 4 * m, hipMemcpyDeviceToHost, c->stream));
    if (stage_out && upd_dst && updated)
        HIP_TRY(hipMemcpyAsync(upd_dst, d_upd, 4 * (size_t)updated, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    v.M += created;
    v.points += stored;
    v.dropped += dropped;
    v.calls++;
    if (delta) delta->created = created, delta->updated = updated, delta->dropped = dropped;
    return SDM_OK;
}

int sdm_vmap_import_observations(sdm_ctx* c, long long count, sdm_vmap_obs_import* io)
{
    if (io) io->total = io->rejected = io->first_created = io->created = 0;
    if (!c || !io) return fail(SDM_EINVAL, "null argument");
    sdm_ctx::Vmap& v = c->vmap;
    sdm_ctx::Vmap::Obs& o = v.obs;
    if (!v.open) return fail(SDM_ESTATE, "no open voxel map");
    if (count < 0) return fail(SDM_EINVAL, "negative count");
    if (io->map_count < 0) return fail(SDM_EINVAL, "negative map_count");
    if (count > 0 && (!io->entry || !io->tag)) return fail(SDM_EINVAL, "null source (entry and tag are required)");
    const bool dev = io->on_device != 0;
    if (dev && ((uintptr_t)io->entry | (uintptr_t)io->tag | (uintptr_t)io->entry_map) % 4)
        return fail(SDM_EINVAL, "device buffer not aligned (entry, tag, entry_map: 4 B)");
    const long long P = count;
    io->total = P;
    io->first_created = o.E;
    if (o.E + P > (1ll << 30))
        return fail(SDM_EINVAL, "more than 2^30 observations and pairs: the observation set would exceed 2^31 slots");
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (P == 0) {
        o.calls++;
        return SDM_OK;
    }

    // scratch, the staging of host sources, pinned mirror and growth: everything is allocated before anything is inserted
    const size_t m = (size_t)P, mm = io->entry_map ? (size_t)io->map_count : 0;
    VobsScratch s;  // head.mid: {rejected, stored or found, overflow}; head.tot: {created, rejected, stored or found, overflow}
    const unsigned* d_entry = io->entry;
    const int* d_tag = io->tag;
    const unsigned* d_map = io->entry_map;
    int rc;
    if ((rc = carve_scratch(&o.d_scratch, &o.scratch_bytes, [&](Carver& k) {
             s = VobsScratch(k, P);
             if (dev) return;
             d_entry = k.take<unsigned>(m);
             d_tag = k.take<int>(m);
             const unsigned* map = k.take<unsigned>(mm);
             if (d_map) d_map = map;  // (map_count == 0: never read)
         })))
        return rc;
    if ((rc = ext_grow_host(&o.h_pin, &o.pin_bytes, 256))) return rc;
    // the tags a list may now hold bound its length (sdm_vmap_fetch_cameras' scan): device tags are read back for that, into
    // a buffer made here, before anything is inserted
    std::vector<int> back;
    if (dev) {
        try {
            back.resize(m);
        } catch (const std::bad_alloc&) {
            return fail(SDM_EHIP, "host allocation of " + std::to_string(4 * m) + " B for the tags failed");
        }
    }
    if ((rc = vobs_grow(c, o.E + P))) return rc;
    if (!dev) {
        HIP_TRY(stage_in(c, d_entry, io->entry, 4 * m));
        HIP_TRY(stage_in(c, d_tag, io->tag, 4 * m));
        if (mm) HIP_TRY(stage_in(c, d_map, io->entry_map, 4 * mm));
    }
    HIP_TRY(hipMemsetAsync(s.head.mid, 0, 24, c->stream));
    launch_sliced(c, (P + BLOCK - 1) / BLOCK, [&](long long b0, unsigned g) {
        hipLaunchKernelGGL(k_vobs_import_insert, dim3(g), dim3(BLOCK), 0, c->stream, d_entry, d_tag, d_map, io->map_count, P,
                           b0 * BLOCK, (unsigned)v.M, o.tb, s.where, s.head.mid, (const unsigned char*)nullptr);
    });
    vobs_count(c, s, P);
    HIP_TRY(hipGetLastError());
    unsigned long long* h_tot = reinterpret_cast<unsigned long long*>(o.h_pin);
    HIP_TRY(hipMemcpyAsync(h_tot, s.head.tot, 32, hipMemcpyDeviceToHost, c->stream));
    const int* h_tag = io->tag;
    if (dev) {
        HIP_TRY(hipMemcpyAsync(back.data(), d_tag, 4 * m, hipMemcpyDeviceToHost, c->stream));
        h_tag = back.data();
    }
    HIP_TRY(hipStreamSynchronize(c->stream));  // the first wait: created
    if (h_tot[3]) return fail(SDM_EHIP, "observation set overflow");
    const long long created = (long long)h_tot[0];

    vobs_commit(c, s, (unsigned)o.E, P);
    HIP_TRY(hipGetLastError());
    // every tag >= 0 of the call counts, a rejected pair's too (its entry is not resolved here): `seen` is an upper bound of
    // the tags the lists hold, which is all sdm_vmap_fetch_cameras' refusal needs, and the header says so
    int last = -1;
    for (size_t k = 0; k < m; k++) {  // (on the host, beside the commit; one binary search per change of tag)
        const int t = h_tag[k];
        if (t < 0 || t == last) continue;
        last = t;
        const auto it = std::lower_bound(o.seen.begin(), o.seen.end(), t);
        if (it == o.seen.end() || *it != t) o.seen.insert(it, t);
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    io->rejected = (long long)h_tot[1];
    io->created = created;
    o.E += created;
    o.calls++;
    return SDM_OK;
}

// ---- re-placing the persistent voxel map under new poses (sdm_vmap_repose.h) ----------------------------------------------
int sdm_vmap_repose(sdm_ctx* c, int n_poses, const int* tags, const float* K, const float* Tcw, sdm_vmap_repose_delta* delta)
{
    if (delta)
        delta->examined = delta->reposed = delta->moved = delta->dropped = delta->merged = delta->voxels =
            delta->observations_before = delta->observations = 0;
    if (!c || !delta) return fail(SDM_EINVAL, "null argument");
    sdm_ctx::Vmap& v = c->vmap;
    sdm_ctx::Vmap::Obs& o = v.obs;
    if (!v.open) return fail(SDM_ESTATE, "no open voxel map");
    if (n_poses < 0) return fail(SDM_EINVAL, "negative n_poses");
    if (n_poses > 0 && (!tags || !K || !Tcw)) return fail(SDM_EINVAL, "null pose table (tags, K and Tcw are required)");
    if (delta->carry != 0 && delta->carry != 1) return fail(SDM_EINVAL, "carry must be 0 or 1");
    const size_t np = (size_t)n_poses;
    std::vector<int> order;  // the table's rows by ascending tag
    try {
        order.resize(np);
    } catch (const std::bad_alloc&) {
        return fail(SDM_EHIP, "host allocation for the pose table failed");
    }
    for (size_t p = 0; p < np; p++) {
        if (tags[p] < 0) return fail(SDM_EINVAL, "tag outside [0, 2^31)");
        order[p] = (int)p;
    }
    std::sort(order.begin(), order.end(), [tags](int a, int b) { return tags[a] < tags[b]; });
    for (size_t p = 1; p < np; p++)
        if (tags[order[p]] == tags[order[p - 1]]) return fail(SDM_EINVAL, "tag " + std::to_string(tags[order[p]]) + " listed twice");
    unsigned* remap_dst = delta->remap;
    const bool remap_dev = remap_dst && delta->on_device;
    if (remap_dev && (uintptr_t)remap_dst % 4) return fail(SDM_EINVAL, "device buffer not aligned (remap: 4 B)");
    const long long M = v.M, E = o.E;
    delta->examined = M;
    if (remap_dst && delta->remap_capacity < M)
        return fail(SDM_EINVAL, "remap_capacity " + std::to_string(delta->remap_capacity) + " < entries = " + std::to_string(M) +
                                    " (examined filled)");
    HIP_TRY(hipSetDevice(c->cfg.device));
    delta->observations_before = delta->observations = E;
    if (M == 0) {  // (no entry: no pair, no counter, no flag)
        v.calls++;
        return SDM_OK;
    }

    // scratch, pose table, the second set of records (with carry: of counters and flags), the log's scratch: everything is
    // allocated before anything is written
    const bool carry = delta->carry == 1;
    const size_t m = (size_t)M;
    const size_t tags_b = ext_align(4 * np), poses_b = ext_align(sizeof(KfMeta) * np);
    VmapScratch s;  // head.mid: {reposed, moved, published}
    float* d_xyz = nullptr;
    int* d_tags = nullptr;
    KfMeta* d_poses = nullptr;
    unsigned* d_remap = remap_dst;
    int rc;
    if ((rc = carve_scratch(&v.d_scratch, &v.scratch_bytes, [&](Carver& k) {
             s = VmapScratch(k, M);
             d_xyz = k.take<float>(3 * m);
             d_tags = k.take<int>(np);  // (tags | poses: one copy fills both)
             d_poses = k.take<KfMeta>(np);
             if (!remap_dev) d_remap = k.take<unsigned>(m);
         })))
        return rc;
    if ((rc = ext_grow_host(&v.h_pin, &v.pin_bytes, 256 + tags_b + poses_b))) return rc;
    VobsScratch os;
    if (E > 0) {
        if ((rc = carve_scratch(&o.d_scratch, &o.scratch_bytes, [&](Carver& k) { os = VobsScratch(k, E); }))) return rc;
        if ((rc = ext_grow_host(&o.h_pin, &o.pin_bytes, 256))) return rc;
    }
    VmapSecond nw;
    if ((rc = vmap_make_second(c, v.rec_cap, carry && v.d_evid, false, carry && v.cls.d_pub, &nw))) return rc;

    unsigned long long* d_rep = s.head.mid;
    unsigned long long* h_tot = reinterpret_cast<unsigned long long*>(v.h_pin);  // [0..5) the import's totals, [8..11) d_rep
    int* h_tags = reinterpret_cast<int*>(v.h_pin + 256);
    KfMeta* h_poses = reinterpret_cast<KfMeta*>(v.h_pin + 256 + tags_b);
    for (size_t q = 0; q < np; q++) {
        const size_t at = (size_t)order[q];
        h_tags[q] = tags[at];
        std::memset(&h_poses[q], 0, sizeof(KfMeta));
        fill_meta(h_poses[q], K + 4 * at, Tcw + 12 * at);
    }

    // the new xyz of every old entry
    HIP_TRY(hipMemsetAsync(s.head.base, 0, 512, c->stream));
    if (np) HIP_TRY(hipMemcpyAsync(d_tags, h_tags, tags_b + poses_b, hipMemcpyHostToDevice, c->stream));
    const long long pblocks = (M + BLOCK - 1) / BLOCK;
    launch_sliced(c, pblocks, [&](long long b0, unsigned g) {
        hipLaunchKernelGGL(k_vrep_project, dim3(g), dim3(BLOCK), 0, c->stream, v.rec, M, b0 * BLOCK, d_tags, d_poses, n_poses, d_xyz,
                           d_rep);
    });
    // one import of the old records, at their new xyz, into the emptied table and the second set of records
    HIP_TRY(vmap_reset_table(c, v.tb));
    VimpSrc in{};
    in.xyz = d_xyz, in.rho_sigma = v.rec.rho_sigma, in.pixel = v.rec.pixel;
    in.intensity = v.rec.intensity, in.tag = v.rec.tag, in.multiplicity = v.rec.multiplicity;
    launch_sliced(c, pblocks, [&](long long b0, unsigned g) {
        hipLaunchKernelGGL(k_vimp_insert, dim3(g), dim3(BLOCK), 0, c->stream, in, M, b0 * BLOCK, v.inv, v.tb, s.where, s.head.ctr,
                           s.head.tot + 4);
    });
    if ((rc = vmap_count_and_total(c, nw.r, s, M, 40))) return rc;  // the first wait: the new M
    const long long M2 = (long long)h_tot[0], dropped = (long long)h_tot[2];

    vmap_assign_ids(c, nw.r, s, 0u, M);
    launch_sliced(c, s.tiles, [&](long long t0, unsigned g) {
        hipLaunchKernelGGL(k_vimp_commit, dim3(g), dim3(BLOCK), 0, c->stream, v.tb, nw.r, s.where, 0u, M, t0, s.scan.s[1].off,
                           s.scan.s[1].boff, (unsigned*)nullptr);
    });
    launch_sliced(c, pblocks, [&](long long b0, unsigned g) {
        hipLaunchKernelGGL(k_vimp_write, dim3(g), dim3(BLOCK), 0, c->stream, v.tb, nw.r, s.where, 0u, 0u, M, b0 * BLOCK, in, d_remap,
                           (const unsigned*)v.rec.epoch);
    });
    // counters and flags: carried through remap into the second set, or back to 0 where they are
    if (carry && (nw.evid.p || nw.pub.p)) {
        launch_sliced(c, pblocks, [&](long long b0, unsigned g) {
            hipLaunchKernelGGL(k_vrep_carry, dim3(g), dim3(BLOCK), 0, c->stream, d_remap, M, b0 * BLOCK,
                               nw.evid.p ? v.crossings : nullptr, nw.evid.p ? v.ends : nullptr, nw.crossings, nw.ends,
                               nw.pub.p ? v.cls.d_pub : nullptr, nw.pub.p);
        });
        if (nw.pub.p)
            launch_sliced(c, (M2 + BLOCK - 1) / BLOCK, [&](long long b0, unsigned g) {
                hipLaunchKernelGGL(k_vrep_count, dim3(g), dim3(BLOCK), 0, c->stream, nw.pub.p, M2, b0 * BLOCK, d_rep + 2);
            });
    } else if (!carry) {
        if (v.d_evid) HIP_TRY(vmap_zero_evidence(c, v.crossings, v.ends));
        if (v.cls.d_pub) HIP_TRY(vmap_zero_published(c, v.cls.d_pub, v.rec_cap));
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_tot + 8, d_rep, 24, hipMemcpyDeviceToHost, c->stream));
    if (remap_dst && !remap_dev) HIP_TRY(hipMemcpyAsync(remap_dst, d_remap, 4 * m, hipMemcpyDeviceToHost, c->stream));

    // the log: the old pairs, in log order, through remap into the emptied set, in place
    const unsigned long long* h_otot = E > 0 ? reinterpret_cast<const unsigned long long*>(o.h_pin) : nullptr;
    if (E > 0 && (rc = vobs_rebuild_through_remap(c, d_remap, M, M2, nullptr, os))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));  // the second wait: the end
    if (h_otot && h_otot[3]) return fail(SDM_EHIP, "observation set overflow");

    vmap_adopt_second_sets(v, nw);
    v.cls.published = carry ? (long long)h_tot[10] : 0;
    v.M = M2;
    v.calls++;
    if (h_otot) o.E = (long long)h_otot[0];
    delta->reposed = (long long)h_tot[8];
    delta->moved = (long long)h_tot[9];
    delta->dropped = dropped;
    delta->voxels = M2;
    delta->merged = M - dropped - M2;
    delta->observations = o.E;
    return SDM_OK;
}

// ---- retiring keyframes from the persistent voxel map (sdm_vmap_retire.h) -------------------------------------------------
namespace {
// the log's scratch of a retire: the rebuild's own, the pairs' marks and the vanished pairs' scan.  The removed pairs' scan
// needs no arrays of its own: it has done its work -- k_vret_totals and k_vret_removed -- before the rebuild counts.
struct VretLogScratch {
    VobsScratch rebuild;
    unsigned char* pmark = nullptr;
    Scan vanished;
    VretLogScratch() = default;
    VretLogScratch(Carver& k, long long E) : rebuild(k, E), pmark(k.take<unsigned char>((size_t)E)), vanished(k, rebuild.tiles) {}
    const Scan& removed() const { return rebuild.scan; }
};
}  // namespace

int sdm_vmap_retire(sdm_ctx* c, int n_tags, const int* tags, int commit, sdm_vmap_retire_delta* delta)
{
    if (delta)
        delta->examined = delta->dropped = delta->dropped_were_published = delta->orphaned = delta->voxels =
            delta->observations_before = delta->observations = delta->removed = delta->published_total = 0;
    if (!c || !delta) return fail(SDM_EINVAL, "null argument");
    sdm_ctx::Vmap& v = c->vmap;
    sdm_ctx::Vmap::Obs& o = v.obs;
    if (!v.open) return fail(SDM_ESTATE, "no open voxel map");
    if (n_tags < 0) return fail(SDM_EINVAL, "negative n_tags");
    if (n_tags > 0 && !tags) return fail(SDM_EINVAL, "null tags");
    if (delta->mode != SDM_VMAP_RETIRE_WINNER && delta->mode != SDM_VMAP_RETIRE_UNOBSERVED)
        return fail(SDM_EINVAL, "mode must be SDM_VMAP_RETIRE_WINNER or SDM_VMAP_RETIRE_UNOBSERVED");
    if (delta->carry != 0 && delta->carry != 1) return fail(SDM_EINVAL, "carry must be 0 or 1");
    if (commit != 0 && commit != 1) return fail(SDM_EINVAL, "commit must be 0 or 1");
    const size_t nt = (size_t)n_tags;
    std::vector<int> sorted;  // R, ascending
    try {
        sorted.assign(tags, tags + nt);
    } catch (const std::bad_alloc&) {
        return fail(SDM_EHIP, "host allocation for the tags failed");
    }
    for (size_t p = 0; p < nt; p++)
        if (sorted[p] < 0) return fail(SDM_EINVAL, "tag outside [0, 2^31)");
    std::sort(sorted.begin(), sorted.end());
    for (size_t p = 1; p < nt; p++)
        if (sorted[p] == sorted[p - 1]) return fail(SDM_EINVAL, "tag " + std::to_string(sorted[p]) + " listed twice");
    unsigned *remap_dst = delta->remap, *drop_dst = delta->dropped_ids, *rem_dst = delta->removed_entry;
    unsigned char* dpub_dst = delta->dropped_published;
    int* rtag_dst = delta->removed_tag;
    if ((remap_dst && delta->remap_capacity < 0) || ((drop_dst || dpub_dst) && delta->dropped_capacity < 0) ||
        ((rem_dst || rtag_dst) && delta->removed_capacity < 0))
        return fail(SDM_EINVAL, "negative capacity");
    if (dpub_dst && !drop_dst) return fail(SDM_EINVAL, "dropped_published without dropped_ids");
    if (rtag_dst && !rem_dst) return fail(SDM_EINVAL, "removed_tag without removed_entry");
    const bool dev = delta->on_device != 0;
    if (dev && ((uintptr_t)remap_dst | (uintptr_t)drop_dst | (uintptr_t)rem_dst | (uintptr_t)rtag_dst) % 4)
        return fail(SDM_EINVAL, "device buffer not aligned (remap, dropped_ids, removed_entry, removed_tag: 4 B)");
    HIP_TRY(hipSetDevice(c->cfg.device));
    const long long M = v.M, E = o.E;
    const bool unobserved = delta->mode == SDM_VMAP_RETIRE_UNOBSERVED, carry = delta->carry == 1;
    delta->examined = M;
    delta->observations_before = E;
    if (M == 0) {  // (no entry: no pair, no counter, no flag)
        if (commit) v.calls++;
        return SDM_OK;
    }

    // the marking phase's scratch and the log's, R on both sides of the link, the second sets: everything but the staging
    // of host lists, which follows the counts, is allocated before anything is written
    const size_t m = (size_t)M;
    const long long vt = ext_tiles(M), ot = ext_tiles(E);
    const size_t tags_b = ext_align(4 * std::max(nt, (size_t)1));
    ScratchHead head;  // ctr: {-, overflow}; mid: k_vret_entries' three counters; tot: k_vret_totals' seven
    int* d_tags = nullptr;
    unsigned char *d_seen = nullptr, *d_emark = nullptr;
    ScanPair scan;  // [0] the entries that stay, [1] the dropped ones
    unsigned* d_remap = remap_dst;
    int rc;
    if ((rc = carve_scratch(&v.d_scratch, &v.scratch_bytes, [&](Carver& k) {
             head = ScratchHead(k);
             d_tags = k.take<int>(std::max(nt, (size_t)1));
             d_seen = k.take<unsigned char>(m);
             d_emark = k.take<unsigned char>(m);
             scan = ScanPair(k, vt, vt);
             if (!(dev && remap_dst)) d_remap = k.take<unsigned>(m);
         })))
        return rc;
    if ((rc = ext_grow_host(&v.h_pin, &v.pin_bytes, 256 + tags_b))) return rc;
    VretLogScratch ls;  // (E == 0: every pointer null, no kernel reads one)
    if (E > 0) {
        if ((rc = carve_scratch(&o.d_scratch, &o.scratch_bytes, [&](Carver& k) { ls = VretLogScratch(k, E); }))) return rc;
        if ((rc = ext_grow_host(&o.h_pin, &o.pin_bytes, 256))) return rc;
    }
    VmapSecond nw;
    if (commit && (rc = vmap_make_second(c, v.rec_cap, carry && v.d_evid, false, carry && v.cls.d_pub, &nw))) return rc;
    const Scan &stay = scan.s[0], &drop = scan.s[1], &rem = ls.removed(), &van = ls.vanished;
    unsigned char* d_pmark = ls.pmark;
    unsigned long long* h_tot = reinterpret_cast<unsigned long long*>(v.h_pin);
    int* h_tags = reinterpret_cast<int*>(v.h_pin + 256);
    if (nt) std::memcpy(h_tags, sorted.data(), 4 * nt);

    // the marking phase: reads the map, writes scratch
    HIP_TRY(hipMemsetAsync(head.base, 0, 512, c->stream));
    if (nt) HIP_TRY(hipMemcpyAsync(d_tags, h_tags, 4 * nt, hipMemcpyHostToDevice, c->stream));
    if (unobserved) HIP_TRY(hipMemsetAsync(d_seen, 0, m, c->stream));
    const long long pblocks = (M + BLOCK - 1) / BLOCK, eblocks = (E + BLOCK - 1) / BLOCK;
    launch_sliced(c, eblocks, [&](long long b0, unsigned g) {
        hipLaunchKernelGGL(k_vret_pairs, dim3(g), dim3(BLOCK), 0, c->stream, (const unsigned*)o.log.entry, (const int*)o.log.tag, E,
                           b0 * BLOCK, (unsigned)M, (const int*)d_tags, n_tags, d_pmark, unobserved ? d_seen : (unsigned char*)nullptr);
    });
    launch_sliced(c, pblocks, [&](long long b0, unsigned g) {
        hipLaunchKernelGGL(k_vret_entries, dim3(g), dim3(BLOCK), 0, c->stream, (const int*)v.rec.tag, (const unsigned char*)v.cls.d_pub,
                           unobserved ? (const unsigned char*)d_seen : (const unsigned char*)nullptr, M, b0 * BLOCK,
                           (const int*)d_tags, n_tags, d_emark, head.mid);
    });
    launch_sliced(c, vt, [&](long long t0, unsigned g) {
        hipLaunchKernelGGL(k_vret_count, dim3(g), dim3(BLOCK), 0, c->stream, (const unsigned char*)d_emark, 1u, 1u, 0u, M, t0,
                           stay.cnt, drop.cnt);
    });
    scan_counts(c, stay, vt);
    scan_counts(c, drop, vt);
    if (E > 0) {
        launch_sliced(c, eblocks, [&](long long b0, unsigned g) {
            hipLaunchKernelGGL(k_vret_vanish, dim3(g), dim3(BLOCK), 0, c->stream, (const unsigned*)o.log.entry, E, b0 * BLOCK,
                               (unsigned)M, (const unsigned char*)d_emark, d_pmark);
        });
        launch_sliced(c, ot, [&](long long t0, unsigned g) {
            hipLaunchKernelGGL(k_vret_count, dim3(g), dim3(BLOCK), 0, c->stream, (const unsigned char*)d_pmark, 3u,
                               (unsigned)VRET_REMOVED, (unsigned)VRET_VANISHED, E, t0, rem.cnt, van.cnt);
        });
        scan_counts(c, rem, ot);
        scan_counts(c, van, ot);
    }
    hipLaunchKernelGGL(k_vret_totals, dim3(1), dim3(64), 0, c->stream, vt, stay.off, stay.boff, drop.off, drop.boff,
                       E > 0 ? ot : 0ll, rem.off, rem.boff, van.off, van.boff, head.mid, head.tot);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_tot, head.tot, 56, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // the first wait: the counts
    const long long M2 = (long long)h_tot[0], dropped = (long long)h_tot[1], removed = (long long)h_tot[2],
                    vanished = (long long)h_tot[3];
    delta->dropped = dropped;
    delta->removed = removed;
    delta->orphaned = (long long)h_tot[4];
    delta->dropped_were_published = (long long)h_tot[5];
    delta->voxels = M2;
    delta->observations = E - removed - vanished;
    delta->published_total = carry ? (long long)h_tot[6] : 0;
    if (remap_dst && delta->remap_capacity < M)
        return fail(SDM_EINVAL, "remap_capacity " + std::to_string(delta->remap_capacity) + " < entries = " + std::to_string(M) +
                                    " (the counts are filled)");
    if (drop_dst && delta->dropped_capacity < dropped)
        return fail(SDM_EINVAL, "dropped_capacity " + std::to_string(delta->dropped_capacity) + " < " + std::to_string(dropped) +
                                    " dropped entries (the counts are filled)");
    if (rem_dst && delta->removed_capacity < removed)
        return fail(SDM_EINVAL, "removed_capacity " + std::to_string(delta->removed_capacity) + " < " + std::to_string(removed) +
                                    " removed pairs (the counts are filled)");

    // the lists (nothing of the map has changed yet: a failure here leaves the state as it was)
    const bool list_drop = drop_dst && dropped, list_rem = rem_dst && removed;
    unsigned *d_drop = list_drop ? drop_dst : nullptr, *d_rem = list_rem ? rem_dst : nullptr;
    unsigned char* d_dpub = list_drop ? dpub_dst : nullptr;
    int* d_rtag = list_rem ? rtag_dst : nullptr;
    if (!dev && (list_drop || list_rem)) {
        const size_t drop_b = list_drop ? ext_align(4 * (size_t)dropped) : 0, dpub_b = list_drop && dpub_dst ? ext_align((size_t)dropped) : 0,
                     rem_b = list_rem ? ext_align(4 * (size_t)removed) : 0;
        if ((rc = ext_grow_dev(&v.d_out, &v.out_bytes, drop_b + dpub_b + 2 * rem_b))) return rc;
        if (list_drop) d_drop = reinterpret_cast<unsigned*>(v.d_out);
        if (list_drop && dpub_dst) d_dpub = v.d_out + drop_b;
        if (list_rem) d_rem = reinterpret_cast<unsigned*>(v.d_out + drop_b + dpub_b);
        if (list_rem && rtag_dst) d_rtag = reinterpret_cast<int*>(v.d_out + drop_b + dpub_b + rem_b);
    }
    if (commit || remap_dst || list_drop)
        launch_sliced(c, vt, [&](long long t0, unsigned g) {
            hipLaunchKernelGGL(k_vret_remap, dim3(g), dim3(BLOCK), 0, c->stream, (const unsigned char*)d_emark, M, t0, stay.off,
                               stay.boff, drop.off, drop.boff, commit || remap_dst ? d_remap : (unsigned*)nullptr, d_drop, d_dpub);
        });
    if (list_rem)
        launch_sliced(c, ot, [&](long long t0, unsigned g) {
            hipLaunchKernelGGL(k_vret_removed, dim3(g), dim3(BLOCK), 0, c->stream, (const unsigned char*)d_pmark,
                               (const unsigned*)o.log.entry, (const int*)o.log.tag, E, t0, rem.off, rem.boff, d_rem, d_rtag);
        });
    HIP_TRY(hipGetLastError());
    if (!dev) {  // (the copies are queued behind the kernels that fill their sources and before anything overwrites them)
        if (remap_dst) HIP_TRY(hipMemcpyAsync(remap_dst, d_remap, 4 * m, hipMemcpyDeviceToHost, c->stream));
        if (list_drop) HIP_TRY(hipMemcpyAsync(drop_dst, d_drop, 4 * (size_t)dropped, hipMemcpyDeviceToHost, c->stream));
        if (list_drop && dpub_dst) HIP_TRY(hipMemcpyAsync(dpub_dst, d_dpub, (size_t)dropped, hipMemcpyDeviceToHost, c->stream));
        if (list_rem) HIP_TRY(hipMemcpyAsync(rem_dst, d_rem, 4 * (size_t)removed, hipMemcpyDeviceToHost, c->stream));
        if (list_rem && rtag_dst) HIP_TRY(hipMemcpyAsync(rtag_dst, d_rtag, 4 * (size_t)removed, hipMemcpyDeviceToHost, c->stream));
    }
    if (!commit) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        return SDM_OK;
    }

    // records (with carry: counters and flags) into the second set; the table emptied and filled from the new records
    launch_sliced(c, pblocks, [&](long long b0, unsigned g) {
        hipLaunchKernelGGL(k_vret_records, dim3(g), dim3(BLOCK), 0, c->stream, v.rec, nw.r, (const unsigned*)d_remap, M, b0 * BLOCK,
                           nw.evid.p ? (const unsigned long long*)v.crossings : nullptr,
                           nw.evid.p ? (const unsigned long long*)v.ends : nullptr, nw.crossings, nw.ends,
                           nw.pub.p ? (const unsigned char*)v.cls.d_pub : nullptr, nw.pub.p);
    });
    if (!carry) {
        if (v.d_evid) HIP_TRY(vmap_zero_evidence(c, v.crossings, v.ends));
        if (v.cls.d_pub) HIP_TRY(vmap_zero_published(c, v.cls.d_pub, v.rec_cap));
    }
    HIP_TRY(vmap_reset_table(c, v.tb));
    launch_sliced(c, (M2 + BLOCK - 1) / BLOCK, [&](long long b0, unsigned g) {
        hipLaunchKernelGGL(k_vret_table, dim3(g), dim3(BLOCK), 0, c->stream, (const float*)nw.r.xyz, M2, b0 * BLOCK, v.inv, v.tb,
                           head.ctr);
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_tot + 8, head.ctr, 8, hipMemcpyDeviceToHost, c->stream));

    // the log: the old pairs that stay, in log order, through remap into the emptied set, in place (from here on the
    // removed pairs' scan is overwritten: VretLogScratch)
    const unsigned long long* h_otot = E > 0 ? reinterpret_cast<const unsigned long long*>(o.h_pin) : nullptr;
    if (E > 0 && (rc = vobs_rebuild_through_remap(c, d_remap, M, M2, d_pmark, ls.rebuild))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));  // the second wait: the end
    if (reinterpret_cast<unsigned*>(h_tot + 8)[1]) return fail(SDM_EHIP, "voxel map table overflow");
    if (h_otot && h_otot[3]) return fail(SDM_EHIP, "observation set overflow");

    vmap_adopt_second_sets(v, nw);
    v.cls.published = delta->published_total;
    v.M = M2;
    v.calls++;
    if (h_otot) o.E = (long long)h_otot[0];
    return SDM_OK;
}

// ---- rebuilding the free-space evidence from the observation log (sdm_vmap_recarve.h) -------------------------------------
int sdm_vmap_recarve(sdm_ctx* c, int n_poses, const int* tags, const float* Tcw, sdm_vmap_recarve_args* rc)
{
    if (rc)
        rc->pairs_total = rc->pairs_unposed = rc->rays_total = rc->rays_skipped = rc->cells_visited = rc->cells_hit = rc->ends_hit = 0;
    if (!c || !rc) return fail(SDM_EINVAL, "null argument");
    sdm_ctx::Vmap& v = c->vmap;
    sdm_ctx::Vmap::Obs& o = v.obs;
    if (!v.open) return fail(SDM_ESTATE, "no open voxel map");
    std::vector<int> order;  // the table's rows by ascending tag
    std::string why;
    long long count = 0;
    int r = recarve_check(n_poses, tags, Tcw, rc, o.E, &count, &order, &why);
    if (r) return fail(r, why);
    HIP_TRY(hipSetDevice(c->cfg.device));

    // the scratch, the pinned mirror and the counters: everything is allocated before anything is written
    const size_t np = (size_t)n_poses;
    const size_t tags_b = ext_align(4 * np), org_b = ext_align(16 * np);
    ScratchHead head;  // tot: the kernel's six totals
    int* d_tags = nullptr;
    float* d_org = nullptr;
    if ((r = carve_scratch(&v.d_scratch, &v.scratch_bytes, [&](Carver& k) {
             head = ScratchHead(k);
             d_tags = k.take<int>(np);  // (tags | centres: one copy fills both)
             d_org = k.take<float>(4 * np);
         })))
        return r;
    if ((r = ext_grow_host(&v.h_pin, &v.pin_bytes, 256 + tags_b + org_b))) return r;
    if (!v.d_evid) {  // (the allocation of the first sdm_vmap_carve)
        DevBlock evid;
        unsigned long long *cr = nullptr, *en = nullptr;
        if ((r = vmap_make_evidence(c, v.rec_cap, evid, &cr, &en))) return r;
        evid.install(v.d_evid);
        v.crossings = cr, v.ends = en;
    }
    unsigned long long* h_tot = reinterpret_cast<unsigned long long*>(v.h_pin);
    int* h_tags = reinterpret_cast<int*>(v.h_pin + 256);
    float* h_org = reinterpret_cast<float*>(v.h_pin + 256 + tags_b);
    for (size_t q = 0; q < np; q++) {
        const size_t at = (size_t)order[q];
        h_tags[q] = tags[at];
        pose_centre(Tcw + 12 * at, h_org + 4 * q);
        h_org[4 * q + 3] = 0.f;
    }

    if (rc->reset) HIP_TRY(vmap_zero_evidence(c, v.crossings, v.ends));
    HIP_TRY(hipMemsetAsync(head.tot, 0, 64, c->stream));
    if (np) HIP_TRY(stage_in(c, d_tags, h_tags, tags_b + org_b));
    VmapRecarveIn in;
    in.obs_entry = o.log.entry;
    in.obs_tag = o.log.tag;
    in.xyz = v.rec.xyz;
    in.tags = d_tags;
    in.origin = d_org;
    in.first = rc->first;
    in.count = count;
    in.n = n_poses;
    in.M = (unsigned)v.M;
    in.voxel = v.voxel_size;
    in.inv = v.inv;
    in.end_margin = rc->end_margin;
    in.max_steps = rc->max_steps;
    launch_sliced(c, (count + BLOCK - 1) / BLOCK, [&](long long b0, unsigned g) {
        hipLaunchKernelGGL(k_vmap_recarve, dim3(g), dim3(BLOCK), 0, c->stream, in, b0 * BLOCK, v.tb, v.crossings, v.ends, head.tot);
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_tot, head.tot, 48, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // the one wait: the end, with the totals
    rc->pairs_total = (long long)h_tot[0];
    rc->pairs_unposed = (long long)h_tot[1];
    rc->rays_total = rc->pairs_total - rc->pairs_unposed;
    rc->rays_skipped = (long long)h_tot[2];
    rc->cells_visited = (long long)h_tot[3];
    rc->cells_hit = (long long)h_tot[4];
    rc->ends_hit = (long long)h_tot[5];
    return SDM_OK;
}
