// sphx_contour_chain.hpp — stitching contour segments into polylines (sphx_contour_chain, include/sphx.h "free-surface extraction").
// Pure host code without a HIP dependency: compiled into libsphx (sphx_contour.inc) and restated by tests/contour_reference.py.
// A point is matched by its fp32 bits with -0 folded onto +0 (fp32 == on both coordinates); a point with a NaN matches nothing and is
// kept out of the tables.  The start points are sorted by (point, segment index): the segments that start at one point are a run in
// ascending index, and a cursor per run skips the used ones (used never reverts: every entry is skipped once) — O(n log n) in all.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

namespace sphx_contour_host {

inline bool point_key(const float* p, uint64_t* key) {
    if (p[0] != p[0] || p[1] != p[1]) return false;
    uint32_t bx, by;
    const float x = p[0] + 0.0f, y = p[1] + 0.0f;  // (-0 + 0 = +0 in round-to-nearest)
    std::memcpy(&bx, &x, 4);
    std::memcpy(&by, &y, 4);
    *key = ((uint64_t)bx << 32) | by;
    return true;
}

// -> number of lines.  order [n], line_first [n + 1], closed [n]; segments [n][4] = x0, y0, x1, y1.
inline uint32_t chain(const float* seg, uint32_t n, uint32_t* order, uint32_t* line_first, uint8_t* closed) {
    std::vector<std::pair<uint64_t, uint32_t>> starts;  // (point, segment) sorted: runs of equal points in ascending index
    std::vector<uint64_t> ends;
    starts.reserve(n);
    ends.reserve(n);
    uint64_t k;
    for (uint32_t s = 0; s < n; ++s) {
        if (point_key(seg + 4 * (size_t)s, &k)) starts.emplace_back(k, s);
        if (point_key(seg + 4 * (size_t)s + 2, &k)) ends.push_back(k);
    }
    std::sort(starts.begin(), starts.end());
    std::sort(ends.begin(), ends.end());
    std::vector<uint32_t> cursor(starts.size(), 0u);  // at a run's first entry: entries of the run already found used
    std::vector<uint8_t> used(n, 0);
    // the lowest-index unused segment that starts at the end of s, or n
    auto successor = [&](uint32_t s) -> uint32_t {
        uint64_t e;
        if (!point_key(seg + 4 * (size_t)s + 2, &e)) return n;
        const size_t g = std::lower_bound(starts.begin(), starts.end(), std::make_pair(e, 0u)) - starts.begin();
        size_t at = g + (g < starts.size() ? cursor[g] : 0u);
        while (at < starts.size() && starts[at].first == e && used[starts[at].second]) ++at;
        if (g < starts.size()) cursor[g] = (uint32_t)(at - g);
        return at < starts.size() && starts[at].first == e ? starts[at].second : n;
    };
    uint32_t lines = 0, pos = 0;
    auto follow = [&](uint32_t first, bool may_close) {
        line_first[lines] = pos;
        uint32_t s = first, last = first;
        while (s != n) {
            used[s] = 1;
            order[pos++] = s;
            last = s;
            s = successor(s);
        }
        const float *a = seg + 4 * (size_t)first, *b = seg + 4 * (size_t)last + 2;
        closed[lines++] = may_close && a[0] == b[0] && a[1] == b[1] ? 1 : 0;
    };
    for (uint32_t s = 0; s < n; ++s) {  // pass 1: a start that is nobody's end
        if (used[s]) continue;
        if (point_key(seg + 4 * (size_t)s, &k) && std::binary_search(ends.begin(), ends.end(), k)) continue;
        follow(s, false);
    }
    for (uint32_t s = 0; s < n; ++s)  // pass 2: what is left lies on cycles (or behind one)
        if (!used[s]) follow(s, true);
    line_first[lines] = n;
    return lines;
}

}  // namespace sphx_contour_host
