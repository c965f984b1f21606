// Drives the generic host steps (csrc/sdm_host_steps.h) without a device and without the HIP runtime, for the host
// sanitizers:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Iorb-slam-free-space-carving_amd/csrc tools/host_steps_check.cc -o host_steps_check && ./host_steps_check
// Exit code 0 and "ok" when every layout walks the same bytes over a null base as over a real buffer, every region starts
// 256-byte aligned and inside the buffer, and an output's staging reaches its destination.  The header asks its includer
// for sdm_ctx, fail, HIP_TRY, EXT_TILE, scan_blocks and the pointer form of scan_counts; here they and the runtime calls
// the header makes (malloc, free, their pinned twins, the copy, the error string) are stand-ins over malloc and memcpy,
// so the sanitizers see every byte the steps touch.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sdm_c.h"

// ---- stand-ins for the runtime ---------------------------------------------------------------------------------------------
enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };
typedef void* hipStream_t;
static const unsigned hipHostMallocDefault = 0;
static int live_blocks = 0;
static const char* hipGetErrorString(hipError_t) { return "stand-in error"; }
static hipError_t hipMalloc(void** p, size_t bytes)
{
    *p = std::aligned_alloc(256, (std::max<size_t>(bytes, 1) + 255) & ~(size_t)255);  // (as the runtime aligns its blocks)
    live_blocks += *p != nullptr;
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
static hipError_t hipFree(void* p)
{
    live_blocks -= p != nullptr;
    std::free(p);
    return hipSuccess;
}
static hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return hipMalloc(p, bytes); }
static hipError_t hipHostFree(void* p) { return hipFree(p); }
static hipError_t hipMemcpyAsync(void* to, const void* from, size_t bytes, hipMemcpyKind, hipStream_t)
{
    std::memcpy(to, from, bytes);
    return hipSuccess;
}

// ---- what the engine defines ahead of the header ---------------------------------------------------------------------------
struct sdm_ctx {
    hipStream_t stream = nullptr;
    const unsigned* scanned = nullptr;  // what the last scan_counts was handed
    long long scanned_tiles = 0;
};
static std::string g_err;
static int fail(int code, const std::string& msg)
{
    g_err = msg;
    return code;
}
#define HIP_TRY(expr)                                                                  \
    do {                                                                               \
        hipError_t e__ = (expr);                                                       \
        if (e__ != hipSuccess) return fail(SDM_EHIP, std::string(#expr) + ": " + hipGetErrorString(e__)); \
    } while (0)
constexpr int EXT_TILE = 2048, EXT_SCAN = 2048;
inline long long scan_blocks(long long tiles) { return (tiles + 1 + EXT_SCAN - 1) / EXT_SCAN; }
inline void scan_counts(sdm_ctx* c, const unsigned* cnt, long long tiles, unsigned*, unsigned long long*, unsigned long long*)
{
    c->scanned = cnt;
    c->scanned_tiles = tiles;
}

#include "sdm_host_steps.h"

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("line %d: %s\n", __LINE__, #cond);              \
            failures++;                                                 \
        }                                                               \
    } while (0)

// every region a describe() names, as [first, first + bytes)
struct Regions {
    std::vector<std::pair<uintptr_t, size_t>> r;
    template <typename T>
    T* note(T* p, size_t count)
    {
        r.emplace_back(reinterpret_cast<uintptr_t>(p), sizeof(T) * count);
        return p;
    }
};

// describe() over a null base, then through carve_scratch over the buffer it grows: the same bytes, every region aligned,
// inside the buffer, disjoint from the others, and writable from end to end
template <typename F>
static size_t walk(F&& describe, bool pinned)
{
    Regions null_pass, real;
    Carver bytes{nullptr};
    describe(bytes, null_pass);
    unsigned char* buf = nullptr;
    size_t have = 0;
    size_t walked = 0;
    const auto both = [&](Carver& k) {
        real.r.clear();
        describe(k, real);
        walked = k.at;
    };
    const int rc = pinned ? carve_scratch(&buf, &have, both, ext_grow_host) : carve_scratch(&buf, &have, both);
    CHECK(rc == SDM_OK);
    CHECK(walked == bytes.at && have >= bytes.at);
    CHECK(bytes.at % 256 == 0);
    CHECK(real.r.size() == null_pass.r.size());
    const uintptr_t base = reinterpret_cast<uintptr_t>(buf);
    for (size_t i = 0; i < real.r.size() && i < null_pass.r.size(); i++) {
        CHECK(real.r[i].first % 256 == 0 && null_pass.r[i].first % 256 == 0);
        CHECK(real.r[i].first - base == null_pass.r[i].first);  // the null walk's pointers are the offsets
        CHECK(real.r[i].second == null_pass.r[i].second);
        CHECK(real.r[i].first >= base && real.r[i].first + real.r[i].second <= base + walked);
        for (size_t j = 0; j < i; j++)
            CHECK(real.r[j].first + real.r[j].second <= real.r[i].first || real.r[i].first + real.r[i].second <= real.r[j].first);
        if (real.r[i].second) std::memset(reinterpret_cast<void*>(real.r[i].first), 0x5a, real.r[i].second);
    }
    // growing is by need only: a second, smaller description keeps the block
    unsigned char* before = buf;
    CHECK(carve_scratch(&buf, &have, [](Carver& k) { k.take<int>(1); }, pinned ? ext_grow_host : ext_grow_dev) == SDM_OK);
    CHECK(buf == before || bytes.at < 256);
    CHECK((pinned ? hipHostFree(buf) : hipFree(buf)) == hipSuccess);
    return walked;
}

int main()
{
    CHECK(ext_align(0) == 0 && ext_align(1) == 256 && ext_align(256) == 256 && ext_align(257) == 512);
    CHECK(ext_tiles(0) == 0 && ext_tiles(1) == 1 && ext_tiles(EXT_TILE) == 1 && ext_tiles(EXT_TILE + 1) == 2);

    // ---- plain regions of odd sizes, an empty one among them; device and pinned
    for (int pinned = 0; pinned < 2; pinned++) {
        const size_t got = walk([](Carver& k, Regions& g) {
            g.note(k.take<unsigned char>(1), 1);
            g.note(k.take<float>(3 * 77), 3 * 77);
            g.note(k.take<int>(0), 0);
            g.note(k.take<unsigned long long>(33), 33);
            g.note(k.take<unsigned char>(256), 256);
        }, pinned != 0);
        CHECK(got == 256 + 1024 + 0 + 512 + 256);
    }
    CHECK(walk([](Carver&, Regions&) {}, false) == 0);  // nothing described: nothing grown, no region

    // ---- the Scan carve: counts, offsets (one more), and the two block arrays, at the sizes where a region's length changes
    for (long long tiles : {0ll, 1ll, 63ll, 64ll, 65ll, (long long)EXT_SCAN - 1, (long long)EXT_SCAN, (long long)EXT_SCAN + 1, 70001ll}) {
        Scan kept;
        const size_t got = walk([&](Carver& k, Regions& g) {
            g.note(k.take<int>(5), 5);  // (a region in front, as every caller has)
            kept = Scan(k, tiles);
            g.note(kept.cnt, (size_t)tiles);
            g.note(kept.off, (size_t)tiles + 1);
            g.note(kept.bsum, (size_t)scan_blocks(tiles));
            g.note(kept.boff, (size_t)scan_blocks(tiles));
            g.note(k.take<unsigned long long>(2), 2);  // (and one behind)
        }, false);
        const size_t nb = (size_t)scan_blocks(tiles);
        CHECK(got == 256 + ext_align(4 * (size_t)tiles) + ext_align(4 * ((size_t)tiles + 1)) + 2 * ext_align(8 * nb) + 256);
        CHECK(nb >= 1 && nb * EXT_SCAN >= (size_t)tiles + 1);
        sdm_ctx ctx;
        Scan s;
        unsigned char block[4096];
        Carver k{block};
        s = Scan(k, 3);
        scan_counts(&ctx, s, 3);  // the overload hands the struct's arrays on
        CHECK(ctx.scanned == s.cnt && ctx.scanned_tiles == 3);
    }

    // ---- the output-field helper: device destinations pass through and carve nothing; host ones get a region each, which
    // flush() copies out; a field not asked for is null either way
    {
        sdm_ctx ctx;
        const size_t m = 301;
        std::vector<float> xyz(3 * m, -1.f);
        std::vector<unsigned char> im(m, 0xee);
        std::vector<unsigned long long> words(m, 7);
        unsigned* const none = nullptr;
        for (int dev = 0; dev < 2; dev++) {
            OutCopies outs;
            float* w_xyz = nullptr;
            unsigned* w_pix = nullptr;
            unsigned char* w_im = nullptr;
            unsigned long long* w_words = nullptr;
            int* w_empty = nullptr;
            int empty_dst = 0;
            unsigned char* buf = nullptr;
            size_t have = 0;
            const auto lay = [&](Carver& k) {
                w_xyz = outs.field(k, xyz.data(), 3 * m, dev != 0);
                w_pix = outs.field(k, none, m, dev != 0);
                w_im = outs.field(k, im.data(), m, dev != 0);
                w_words = outs.field(k, words.data(), m, dev != 0);
                w_empty = outs.field(k, &empty_dst, 0, dev != 0);  // (a list of no entries)
            };
            CHECK(carve_scratch(&buf, &have, lay) == SDM_OK);
            CHECK(w_pix == nullptr);
            if (dev) {
                CHECK(have == 0 && buf == nullptr && outs.cp.empty());
                CHECK(w_xyz == xyz.data() && w_im == im.data() && w_words == words.data() && w_empty == &empty_dst);
            } else {
                CHECK(have == ext_align(12 * m) + ext_align(m) + ext_align(8 * m));
                CHECK(outs.cp.size() == 4);  // one note per host field, though describe() ran twice
                for (const void* p : {(const void*)w_xyz, (const void*)w_im, (const void*)w_words})
                    CHECK(reinterpret_cast<uintptr_t>(p) % 256 == 0 && p >= buf && p < buf + have);
                for (size_t i = 0; i < 3 * m; i++) w_xyz[i] = (float)i;
                for (size_t i = 0; i < m; i++) w_im[i] = (unsigned char)i, w_words[i] = i * i;
                CHECK(outs.flush(&ctx) == hipSuccess);
                bool same = empty_dst == 0;
                for (size_t i = 0; i < 3 * m; i++) same = same && xyz[i] == (float)i;
                for (size_t i = 0; i < m; i++) same = same && im[i] == (unsigned char)i && words[i] == i * i;
                CHECK(same);
            }
            CHECK(hipFree(buf) == hipSuccess);
        }
    }

    // ---- DevBlock: what an owner holds when it leaves is freed, an installed block is the slot's
    {
        unsigned char* slot = nullptr;
        {
            DevBlock a, b;
            CHECK(a.alloc(100) == SDM_OK && b.alloc(100) == SDM_OK && live_blocks == 2);
            a.install(slot);
            DevBlock moved(std::move(b));
            CHECK(b.p == nullptr && moved.p != nullptr);
        }
        CHECK(slot != nullptr && live_blocks == 1);
        {
            DevBlock again;
            CHECK(again.alloc(10) == SDM_OK);
            again.install(slot);  // the old block leaves with the owner
        }
        CHECK(live_blocks == 1 && hipFree(slot) == hipSuccess);
    }
    {
        sdm_ctx ctx;
        int to[4] = {0, 0, 0, 0};
        const int from[4] = {1, 2, 3, 4};
        CHECK(stage_in(&ctx, to, from, sizeof(from)) == hipSuccess && to[3] == 4);
    }
    CHECK(live_blocks == 0);

    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
