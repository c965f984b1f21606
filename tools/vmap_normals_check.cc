// Drives the argument checks of sdm_vmap_normals (csrc/sdm_vmap_normals_check.h) without a device, for the host sanitizers:
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Iorb-slam-free-space-carving_amd/csrc tools/vmap_normals_check.cc -o vmap_normals_check && ./vmap_normals_check
// Exit code 0 and "ok" when every case gives what include/sdm_c.h says.  The checks dereference nothing but the args struct
// and tags[0 .. n_poses): the destinations and Tcw handed in here are addresses only, and the tables are heap arrays of exactly
// n_poses elements, so a read past them is the sanitizer's to report.
#include <climits>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <memory>

#include "sdm_vmap_normals_check.h"

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("line %d: %s\n", __LINE__, #cond);              \
            failures++;                                                 \
        }                                                               \
    } while (0)

static float normal[24], variation[8];
static unsigned points[8];
static const float some_pose[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};

static sdm_vmap_normal_args good()
{
    sdm_vmap_normal_args a{};
    a.radius = 1;
    a.min_points = 3;
    a.count = -1;
    a.capacity = 8;
    a.normal = normal, a.variation = variation, a.points = points;
    return a;
}

struct Result {
    int rc;
    long long count;
    std::vector<int> order;
    std::string why;
};

template <typename F>
static Result call(F&& change, long long M = 8, bool open = true, int n_poses = 0, const int* tags = nullptr, const float* Tcw = nullptr)
{
    sdm_vmap_normal_args a = good();
    change(a);
    const sdm_vmap_normal_args before = a;
    Result r;
    r.count = -7;
    r.rc = sdm::normals_check(open, M, n_poses, tags, Tcw, &a, &r.count, &r.order, &r.why);
    CHECK((r.rc == SDM_OK) == r.why.empty());
    CHECK(r.rc == SDM_OK || r.count == -7);           // a refusal leaves the count alone
    CHECK(std::memcmp(&before, &a, sizeof(a)) == 0);  // the checks write nothing
    return r;
}

typedef sdm_vmap_normal_args A;

int main()
{
    const auto same = [](A&) {};
    std::string why;
    std::vector<int> order;
    long long count = 0;
    Result r = call(same);
    CHECK(r.rc == SDM_OK && r.count == 8 && r.order.empty());
    // NULL args, no open map (and the order: the state comes before the arguments' values)
    CHECK(sdm::normals_check(true, 8, 0, nullptr, nullptr, nullptr, &count, &order, &why) == SDM_EINVAL && why == "null argument");
    CHECK(sdm::normals_check(false, 0, -1, nullptr, nullptr, nullptr, &count, &order, &why) == SDM_EINVAL);
    r = call(same, 8, false);
    CHECK(r.rc == SDM_ESTATE && r.why == "no open voxel map");
    CHECK(call([](A& a) { a.radius = 7; }, 8, false).rc == SDM_ESTATE);
    // radius, and min_points against it
    CHECK(sdm::normals_cells(1) == 27 && sdm::normals_cells(2) == 125 && sdm::normals_cells(0) == 0 && sdm::normals_cells(3) == 0);
    for (int rad : {0, 3, -1, -2, INT_MAX, INT_MIN}) {
        r = call([rad](A& a) { a.radius = rad; });
        CHECK(r.rc == SDM_EINVAL && r.why.find("radius") == 0);
    }
    for (unsigned p : {3u, 4u, 26u, 27u}) CHECK(call([p](A& a) { a.min_points = p; }).rc == SDM_OK);
    for (unsigned p : {3u, 27u, 28u, 124u, 125u}) CHECK(call([p](A& a) { a.radius = 2, a.min_points = p; }).rc == SDM_OK);
    for (unsigned p : {0u, 1u, 2u, 28u, 125u, 0x7fffffffu, 0xffffffffu}) {
        r = call([p](A& a) { a.min_points = p; });
        CHECK(r.rc == SDM_EINVAL && r.why.find("min_points") == 0);
    }
    for (unsigned p : {0u, 2u, 126u, 0x80000000u, 0xffffffffu}) CHECK(call([p](A& a) { a.radius = 2, a.min_points = p; }).rc == SDM_EINVAL);
    // require_published; the filter takes every value
    CHECK(call([](A& a) { a.require_published = 1; }).rc == SDM_OK);
    for (int q : {2, -1, INT_MAX, INT_MIN}) {
        r = call([q](A& a) { a.require_published = q; });
        CHECK(r.rc == SDM_EINVAL && r.why.find("require_published") == 0);
    }
    for (unsigned u : {0u, 1u, 0x7fffffffu, 0xffffffffu}) CHECK(call([u](A& a) { a.min_multiplicity = u; }).rc == SDM_OK);
    // the range: first in [0, M], count in [-1, M - first]; the sum is never formed
    r = call([](A& a) { a.first = 3; });
    CHECK(r.rc == SDM_OK && r.count == 5);
    r = call([](A& a) { a.first = 8; });
    CHECK(r.rc == SDM_OK && r.count == 0);
    r = call([](A& a) { a.first = 8, a.count = 0; });
    CHECK(r.rc == SDM_OK && r.count == 0);
    r = call([](A& a) { a.first = 2, a.count = 6; });
    CHECK(r.rc == SDM_OK && r.count == 6);
    r = call([](A& a) { a.count = 0, a.capacity = 0; });
    CHECK(r.rc == SDM_OK && r.count == 0);
    r = call(same, 0);
    CHECK(r.rc == SDM_OK && r.count == 0);
    r = call([](A& a) { a.normal = nullptr, a.variation = nullptr, a.points = nullptr, a.capacity = 0; }, 1ll << 30);
    CHECK(r.rc == SDM_OK && r.count == 1ll << 30);
    for (auto fc : {std::pair<long long, long long>{-1, -1}, {-1, 1}, {LLONG_MIN, -1}, {0, -2}, {0, LLONG_MIN}, {9, -1}, {9, 0}, {0, 9},
                    {1, 8}, {8, 1}, {LLONG_MAX, -1}, {LLONG_MAX, LLONG_MAX}, {1, LLONG_MAX}, {LLONG_MAX, 1}}) {
        r = call([fc](A& a) { a.first = fc.first, a.count = fc.second, a.capacity = LLONG_MAX; });
        CHECK(r.rc == SDM_EINVAL && r.why.find("range beyond") == 0);
    }
    // the capacity: negative with or without the arrays; against the range only where a destination is given
    r = call([](A& a) { a.capacity = -1; });
    CHECK(r.rc == SDM_EINVAL && r.why == "negative capacity");
    CHECK(call([](A& a) { a.capacity = LLONG_MIN; }).rc == SDM_EINVAL);
    CHECK(call([](A& a) { a.capacity = -1, a.normal = nullptr, a.variation = nullptr, a.points = nullptr; }).rc == SDM_EINVAL);
    r = call(same, 9);
    CHECK(r.rc == SDM_EINVAL && r.why.find("capacity below") == 0);
    CHECK(call([](A& a) { a.variation = nullptr, a.points = nullptr; }, 9).rc == SDM_EINVAL);
    CHECK(call([](A& a) { a.normal = nullptr, a.points = nullptr; }, 9).rc == SDM_EINVAL);
    CHECK(call([](A& a) { a.normal = nullptr, a.variation = nullptr; }, 9).rc == SDM_EINVAL);
    CHECK(call([](A& a) { a.normal = nullptr, a.variation = nullptr, a.points = nullptr; }, 9).rc == SDM_OK);
    CHECK(call([](A& a) { a.first = 1; }, 9).rc == SDM_OK);            // the range, not the map, is what the arrays hold
    CHECK(call([](A& a) { a.count = 8; }, 1000).rc == SDM_OK);
    CHECK(call([](A& a) { a.count = 9; }, 1000).rc == SDM_EINVAL);
    CHECK(call([](A& a) { a.capacity = LLONG_MAX; }, 1ll << 30).rc == SDM_OK);
    // alignment counts on the device only
    for (int off = 1; off < 4; off++) {
        const auto bumpf = [off](float* p) { return reinterpret_cast<float*>(reinterpret_cast<uintptr_t>(p) + off); };
        const auto bumpu = [off](unsigned* p) { return reinterpret_cast<unsigned*>(reinterpret_cast<uintptr_t>(p) + off); };
        CHECK(call([&](A& a) { a.normal = bumpf(normal); }).rc == SDM_OK);
        r = call([&](A& a) { a.on_device = 1, a.normal = bumpf(normal); });
        CHECK(r.rc == SDM_EINVAL && r.why.find("device buffer not aligned") == 0);
        CHECK(call([&](A& a) { a.on_device = 1, a.variation = bumpf(variation); }).rc == SDM_EINVAL);
        CHECK(call([&](A& a) { a.on_device = 1, a.points = bumpu(points); }).rc == SDM_EINVAL);
    }
    CHECK(call([](A& a) { a.on_device = 1; }).rc == SDM_OK);
    CHECK(call([](A& a) { a.on_device = 1, a.normal = nullptr, a.variation = nullptr, a.points = nullptr; }).rc == SDM_OK);
    // the pose table: heap arrays of exactly n_poses tags
    {
        r = call(same, 8, true, -1);
        CHECK(r.rc == SDM_EINVAL && r.why == "negative n_poses");
        CHECK(call(same, 8, true, INT_MIN).rc == SDM_EINVAL);
        CHECK(call(same, 8, true, 0, nullptr, nullptr).rc == SDM_OK);
        std::unique_ptr<int[]> t(new int[5]{40, 7, 0, INT_MAX, 12});
        r = call(same, 8, true, 5, t.get(), some_pose);
        CHECK(r.rc == SDM_OK && r.order == (std::vector<int>{2, 1, 4, 0, 3}));
        r = call(same, 8, true, 5, nullptr, some_pose);
        CHECK(r.rc == SDM_EINVAL && r.why.find("null pose table") == 0);
        CHECK(call(same, 8, true, 5, t.get(), nullptr).rc == SDM_EINVAL);
        CHECK(call(same, 8, true, 0, t.get(), nullptr).rc == SDM_OK);   // n_poses == 0 reads no table
        t[4] = 7;
        r = call(same, 8, true, 5, t.get(), some_pose);
        CHECK(r.rc == SDM_EINVAL && r.why == "tag 7 listed twice");
        t[4] = -1;
        r = call(same, 8, true, 5, t.get(), some_pose);
        CHECK(r.rc == SDM_EINVAL && r.why.find("tag outside") == 0);
        t[4] = INT_MIN;
        CHECK(call(same, 8, true, 5, t.get(), some_pose).rc == SDM_EINVAL);
        std::unique_ptr<int[]> one(new int[1]{0});
        r = call(same, 8, true, 1, one.get(), some_pose);
        CHECK(r.rc == SDM_OK && r.order == (std::vector<int>{0}));
        // the arguments' own refusals come before the table's
        r = call([](A& a) { a.radius = 0; }, 8, true, 5, t.get(), some_pose);
        CHECK(r.rc == SDM_EINVAL && r.why.find("radius") == 0);
    }
    // a camera centre (the host forms it with sdm_vmap_recarve's function): O = -(Rwc * tcw)
    {
        const float T[12] = {0, -1, 0, 2, 1, 0, 0, 3, 0, 0, 1, 5};
        float O[3];
        sdm::pose_centre(T, O);
        CHECK(O[0] == -3.f && O[1] == 2.f && O[2] == -5.f);
    }
    // the outs of a refusal
    {
        sdm_vmap_normal_args a = good();
        a.entries = a.members = a.estimated = a.oriented = 7;
        sdm::normals_clear_outs(&a);
        CHECK(!a.entries && !a.members && !a.estimated && !a.oriented);
        CHECK(a.radius == 1 && a.min_points == 3 && a.count == -1 && a.capacity == 8 && a.normal == normal);
    }
    std::printf(failures ? "%d failures\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
