// lane_plan (cppserver_amd/csrc/wsg_lane_plan.h): how a host batch is cut
// into the lane's frame groups.  A pure function of (n, want, limit, strict,
// bound); no device.  Small cases enumerated, every group checked; built with
// AddressSanitizer + UndefinedBehaviorSanitizer (make sanitize).
#include "wsg_lane_plan.h"

#include <cstdio>
#include <vector>

namespace {

int failures = 0;

#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        if (!(cond)) {                                                                                       \
            ++failures;                                                                                      \
            std::printf("FAIL %s:%d: %s  [%s]\n", __FILE__, __LINE__, #cond, what);                          \
        }                                                                                                    \
    } while (0)

constexpr uint32_t T = wsg::LANE_THREADS, G = wsg::LANE_GROUPS_MAX;

// bounds[i] = b(i), i in [0, n]; returns the group count
uint32_t plan(const std::vector<uint64_t>& bounds, uint32_t want, uint64_t limit, bool strict, LaneGroup* g)
{
    const uint32_t n = uint32_t(bounds.size() - 1);
    return lane_plan(n, want, limit, strict, [&](uint32_t i) -> uint64_t { return bounds[i]; }, g);
}

// Every property of a plan that was made (k > 0).
void check_groups(const std::vector<uint64_t>& bounds, uint64_t limit, bool strict, const LaneGroup* g, uint32_t k,
                  const char* what)
{
    const uint32_t n = uint32_t(bounds.size() - 1);
    CHECK(k >= 1 && k <= G);
    uint32_t f = 0;
    for (uint32_t q = 0; q < k; ++q) {
        CHECK(g[q].f == f);                           // contiguous
        CHECK(g[q].cnt >= 1 && g[q].cnt <= T);
        CHECK(uint64_t(g[q].f) + g[q].cnt <= n);
        if (uint64_t(g[q].f) + g[q].cnt > n)
            return;
        CHECK(g[q].lo == bounds[g[q].f]);
        CHECK(g[q].hi == bounds[g[q].f + g[q].cnt]);
        if (strict)
            CHECK(g[q].hi - g[q].lo <= limit);
        else
            CHECK(g[q].hi - g[q].lo <= limit || g[q].cnt == 1);
        f += g[q].cnt;
    }
    CHECK(f == n);                                    // cover [0, n)
}

std::vector<uint64_t> bounds_of(const std::vector<uint64_t>& sizes)
{
    std::vector<uint64_t> b(sizes.size() + 1, 0);
    for (size_t i = 0; i < sizes.size(); ++i)
        b[i + 1] = b[i] + sizes[i];
    return b;
}

// Does any plan exist?  Strict: every frame within the limit.  The greedy
// cut into groups of at most T frames and `limit` bytes is the fewest groups
// possible, so more than G of them means none.
bool fits(const std::vector<uint64_t>& sizes, uint64_t limit, bool strict)
{
    uint32_t groups = 0;
    for (size_t i = 0; i < sizes.size();) {
        if (strict && sizes[i] > limit)
            return false;
        uint64_t bytes = sizes[i];
        size_t e = i + 1;
        while (e < sizes.size() && e - i < T && bytes + sizes[e] <= limit)
            bytes += sizes[e++];
        ++groups;
        i = e;
    }
    return groups <= G;
}

void enumerate_small()
{
    const char* what = "enumerate";
    LaneGroup g[G];
    const uint64_t limit = 10;
    const uint64_t sizes_of[] = {0, 1, 4, 10, 11};
    // every sequence of up to five frames over those sizes
    for (uint32_t n = 1; n <= 5; ++n) {
        uint32_t combos = 1;
        for (uint32_t i = 0; i < n; ++i)
            combos *= 5;
        for (uint32_t c = 0; c < combos; ++c) {
            std::vector<uint64_t> sizes(n);
            bool over = false;
            for (uint32_t i = 0, r = c; i < n; ++i, r /= 5) {
                sizes[i] = sizes_of[r % 5];
                over = over || sizes[i] > limit;
            }
            const std::vector<uint64_t> b = bounds_of(sizes);
            for (uint32_t want : {1u, 3u, 32u})
                for (bool strict : {false, true}) {
                    const uint32_t k = plan(b, want, limit, strict, g);
                    if (strict && over) {
                        CHECK(k == 0);
                        continue;
                    }
                    CHECK(k >= 1);
                    if (k)
                        check_groups(b, limit, strict, g, k, what);
                }
        }
    }
}

void uniform_cases()
{
    LaneGroup g[G];
    const uint64_t limit = 1000;
    for (uint32_t n : {1u, 2u, T, T + 1, 3 * T + 7, G * T}) {
        for (uint64_t size : {uint64_t(0), uint64_t(1), uint64_t(7), limit / 2 + 1, limit}) {
            const std::vector<uint64_t> sizes(n, size);
            const std::vector<uint64_t> b = bounds_of(sizes);
            for (uint32_t want : {1u, 3u, 32u})
                for (bool strict : {false, true}) {
                    char what[96];
                    std::snprintf(what, sizeof what, "uniform n=%u size=%llu want=%u strict=%d", n,
                                  (unsigned long long)size, want, int(strict));
                    const uint32_t k = plan(b, want, limit, strict, g);
                    if (!fits(sizes, limit, strict)) {
                        CHECK(k == 0);
                        continue;
                    }
                    if (k)   // (a request that would fit in other groups than the planner's may still be refused)
                        check_groups(b, limit, strict, g, k, what);
                    if (size == 0 || n <= 2)
                        CHECK(k >= 1);   // zero-length frames, tiny requests: always planned
                }
        }
    }
}

void refusals()
{
    const char* what = "refusals";
    LaneGroup g[G];
    // a frame larger than the limit under strict (alone, and between others)
    CHECK(plan(bounds_of({11}), 3, 10, true, g) == 0);
    CHECK(plan(bounds_of({1, 2, 11, 3}), 3, 10, true, g) == 0);
    CHECK(plan(bounds_of({1, 2, 11, 3}), 3, 10, false, g) != 0);
    // more than LANE_GROUPS_MAX groups of LANE_THREADS frames
    for (uint32_t want : {1u, 3u, 32u})
        for (bool strict : {false, true}) {
            CHECK(plan(bounds_of(std::vector<uint64_t>(G * T + 1, 0)), want, 10, strict, g) == 0);
            CHECK(plan(bounds_of(std::vector<uint64_t>(G * T + 1, 1)), want, 1 << 30, strict, g) == 0);
        }
    // more than 32 frames of exactly `limit` bytes: one group each
    for (uint32_t want : {1u, 3u, 32u}) {
        CHECK(plan(bounds_of(std::vector<uint64_t>(G + 1, 10)), want, 10, true, g) == 0);
        CHECK(plan(bounds_of(std::vector<uint64_t>(G, 10)), want, 10, true, g) == G);
    }
}

} // namespace

int main()
{
    enumerate_small();
    uniform_cases();
    refusals();
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
