// wsg_lane_plan.h — how a host batch is cut into the lane's frame groups: plain
// host arithmetic, apart from the HIP headers so that a stand-alone program
// can include it (tests/cpp/test_lane_plan.cpp).
#pragma once

#include <algorithm>
#include <cstdint>

namespace wsg {
constexpr uint32_t LANE_THREADS = 1024;        // one workgroup of the lane; frames per group (lane per frame)
constexpr uint32_t LANE_GROUPS_MAX = 32;       // frame groups of a request (<= 32 Ki frames)
} // namespace wsg

// A request's frame groups: runs of whole frames [f, f + cnt), each at most
// LANE_THREADS frames over the byte range [lo, hi) of its boundaries b(f) ..
// b(f + cnt) (b(0) = 0, b(n) = the request's end), about equal in bytes and
// about `want` of them (lane_want).  A group's range is at most `limit`
// bytes: strict (decode: the range is staged in LDS) a frame larger than that
// does not fit the lane; otherwise (encode: the payload span is staged when it
// fits, read in place when not) such a frame is a group alone.
// Returns the group count; 0 when the request does not fit the lane (more
// than LANE_GROUPS_MAX groups, or a frame too large for a strict stage).
struct LaneGroup {
    uint32_t f, cnt;
    uint64_t lo, hi;
};

template <class Bound>
uint32_t lane_plan(uint32_t n, uint32_t want, uint64_t limit, bool strict, Bound b, LaneGroup* g)
{
    const uint64_t total = b(n);
    const uint64_t target = std::max<uint64_t>(1, (total + want - 1) / want);
    // b is non-decreasing: the first index in [a, z] whose bound is >= v (z if none)
    const auto first_at_least = [&b](uint32_t a, uint32_t z, uint64_t v) {
        while (a < z) {
            const uint32_t m = a + (z - a) / 2;
            if (b(m) >= v)
                z = m;
            else
                a = m + 1;
        }
        return a;
    };
    uint32_t k = 0;
    for (uint32_t f = 0; f < n;) {
        if (k == wsg::LANE_GROUPS_MAX)
            return 0;
        const uint64_t lo = b(f);
        if (strict && b(f + 1) - lo > limit)
            return 0;
        // the group ends at the first bound reaching the target, before the
        // first past the limit, after at most LANE_THREADS frames, and holds
        // at least one frame
        const uint32_t z = uint32_t(std::min<uint64_t>(n, uint64_t(f) + wsg::LANE_THREADS));
        const uint32_t e_target = first_at_least(f + 1, z, lo + target);
        uint32_t e_limit = first_at_least(f + 1, z, lo + limit + 1);
        if (b(e_limit) - lo > limit)
            --e_limit;
        const uint32_t e = std::max(f + 1, std::min(e_target, e_limit));
        g[k++] = LaneGroup{f, e - f, lo, b(e)};
        f = e;
    }
    return k;
}

// Requests of at most this many frames fit the lane (groups of at most
// LANE_THREADS frames, at most LANE_GROUPS_MAX groups).
constexpr uint32_t kLaneMaxFrames = wsg::LANE_GROUPS_MAX * wsg::LANE_THREADS;
