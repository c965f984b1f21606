// sdm_host_steps.h -- the host steps specific to no call: growing a buffer, describing its layout once, a tile scan's arrays,
// a source into staging, an output out of it.  Included by sdm_engine.hip inside its extern "C" block, after sdm_ctx (for its
// stream), fail, HIP_TRY, EXT_TILE, scan_blocks and the pointer form of scan_counts.  No device code: tools/host_steps_check.cc
// supplies those names itself and drives the layouts under the host sanitizers.
#pragma once

extern "C++" {
namespace {

size_t ext_align(size_t b) { return (b + 255) & ~(size_t)255; }

// grow a device / pinned buffer to at least `bytes` (the previous call ended with a stream sync: nothing uses it)
int ext_grow(unsigned char** p, size_t* have, size_t bytes, bool pinned)
{
    if (*have >= bytes) return SDM_OK;
    HIP_TRY(pinned ? hipHostFree(*p) : hipFree(*p));
    *p = nullptr;
    *have = 0;
    HIP_TRY(pinned ? hipHostMalloc((void**)p, bytes, hipHostMallocDefault) : hipMalloc((void**)p, bytes));
    *have = bytes;
    return SDM_OK;
}
int ext_grow_dev(unsigned char** p, size_t* have, size_t bytes) { return ext_grow(p, have, bytes, false); }
int ext_grow_host(unsigned char** p, size_t* have, size_t bytes) { return ext_grow(p, have, bytes, true); }

// move-only owner of one hipMalloc block.  A call makes its new blocks in owners and installs them in the context once
// everything has succeeded; whatever an owner holds when it leaves -- a block never installed, or the context's old one
// after install -- is freed.
struct DevBlock {
    unsigned char* p = nullptr;
    DevBlock() = default;
    DevBlock(DevBlock&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevBlock(const DevBlock&) = delete;
    DevBlock& operator=(const DevBlock&) = delete;
    ~DevBlock() { (void)hipFree(p); }
    int alloc(size_t bytes) { HIP_TRY(hipMalloc((void**)&p, bytes)); return SDM_OK; }
    void install(unsigned char*& slot) { std::swap(slot, p); }
};

// bump allocator over 256-byte-aligned regions of one buffer.  Over a null base it only adds up the bytes.
struct Carver {
    unsigned char* base;
    size_t at = 0;
    template <typename T>
    T* ptr(size_t offset) const
    {
        return reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(base) + offset);
    }
    template <typename T>
    T* take(size_t count)
    {
        T* r = ptr<T>(at);
        at += ext_align(sizeof(T) * count);
        return r;
    }
};

// A call describes a buffer once, as describe(Carver&): run over a null base for the bytes `buf` must hold, then over the
// grown buffer for the pointers, so the sum and the walk cannot disagree.  `grow`: ext_grow_host for a pinned buffer.
template <typename F>
int carve_scratch(unsigned char** buf, size_t* have, F&& describe, int (*grow)(unsigned char**, size_t*, size_t) = ext_grow_dev)
{
    Carver bytes{nullptr};
    describe(bytes);
    const int rc = grow(buf, have, bytes.at);
    if (rc) return rc;
    Carver k{*buf};
    describe(k);
    return SDM_OK;
}

// tiles of EXT_TILE items: the unit the count and commit kernels work in
long long ext_tiles(long long items) { return (items + EXT_TILE - 1) / EXT_TILE; }

// per-tile counts and the arrays of their scan (scan_counts)
struct Scan {
    unsigned *cnt = nullptr, *off = nullptr;
    unsigned long long *bsum = nullptr, *boff = nullptr;
    Scan() = default;
    Scan(Carver& k, long long tiles)
        : cnt(k.take<unsigned>((size_t)tiles)), off(k.take<unsigned>((size_t)tiles + 1)),
          bsum(k.take<unsigned long long>((size_t)scan_blocks(tiles))), boff(k.take<unsigned long long>((size_t)scan_blocks(tiles))) {}
};
void scan_counts(sdm_ctx* c, const Scan& s, long long tiles) { scan_counts(c, s.cnt, tiles, s.off, s.bsum, s.boff); }

// a host source into its staging region (which the kernels read through pointers to const)
hipError_t stage_in(sdm_ctx* c, const void* dst, const void* src, size_t bytes)
{
    return hipMemcpyAsync(const_cast<void*>(dst), src, bytes, hipMemcpyHostToDevice, c->stream);
}

// The outputs of a call whose destinations are the caller's device arrays or host arrays.  field() is the one statement
// an output needs inside the describe() of its staging buffer: it yields where the kernel writes `count` elements --
// `user` itself when that is on the device (or null: not asked for), else a region of the staging, which flush() then
// copies to `user` ahead of the call's last wait.  (Nothing is noted over a null base: describe() runs twice.)
struct OutCopies {
    struct Copy { void* to; const void* from; size_t bytes; };
    std::vector<Copy> cp;
    template <typename T>
    T* field(Carver& k, T* user, size_t count, bool on_device)
    {
        if (!user || on_device) return user;
        T* r = k.take<T>(count);
        if (k.base) cp.push_back(Copy{user, r, sizeof(T) * count});
        return r;
    }
    hipError_t flush(sdm_ctx* c) const
    {
        hipError_t e = hipSuccess;
        for (const Copy& x : cp)
            if (x.bytes && e == hipSuccess) e = hipMemcpyAsync(x.to, x.from, x.bytes, hipMemcpyDeviceToHost, c->stream);
        return e;
    }
};

}  // namespace
}  // extern "C++"
