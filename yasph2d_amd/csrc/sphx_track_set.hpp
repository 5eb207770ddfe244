// sphx_track_set.hpp — the host side of a tracked id set (sphx_track_set, include/sphx.h): the sorted, de-duplicated table the look-up
// pass binary-searches, the map from the caller's order to it, the bit filter in front of it, and the argument checks that need no
// device.  Plain C++ (no HIP include): tests/track_set_driver.cpp compiles it with the sanitizers.  The device look-up
// (sphx_track.inc) uses track_hash() and the constants, so that filter and probe can never disagree.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace sphx {

constexpr uint32_t TRACK_MAX_IDS = 16384;          // == SPHX_TRACK_MAX_IDS
constexpr uint32_t TRACK_ABSENT = 0xFFFFFFFFu;     // == SPHX_TRACK_ABSENT
constexpr uint32_t TRACK_ABSENT_WORD = 0x7FC00000u;  // every float of an absent id
// The filter: 2^L bits, L = ceil(log2(16 * unique ids)) clamped to [10, 18]: 16 bits per id, ~6 % of the particles that are NOT in the
// set pass it (1 - exp(-1/16)).  At the full 16 384 ids it is 2^18 bits = 32 KiB of LDS; a small set gets a small filter, so that the
// staging cost per workgroup follows the set.
constexpr uint32_t TRACK_FILTER_LOG2_MIN = 10, TRACK_FILTER_LOG2_MAX = 18;
constexpr uint64_t TRACK_RECORD_MAX_BYTES = 1ull << 30;  // recording buffer: max_frames * m * 16 bytes

// the filter bit of an id: multiplicative hash (the high bits of id * 2^32 / phi), L in [1, 32]
constexpr uint32_t track_hash(uint32_t id, uint32_t log2_bits) { return (id * 0x9E3779B1u) >> (32u - log2_bits); }

constexpr uint32_t track_filter_log2(uint32_t unique) {
    uint32_t l = TRACK_FILTER_LOG2_MIN;
    while (l < TRACK_FILTER_LOG2_MAX && (1ull << l) < 16ull * unique) ++l;
    return l;
}

struct TrackSet {
    std::vector<uint32_t> table;   // the unique ids, ascending
    std::vector<uint32_t> map;     // [m]: index into table of the caller's k-th id
    std::vector<uint32_t> filter;  // 2^log2_bits bits, 32 to a word
    uint32_t log2_bits = TRACK_FILTER_LOG2_MIN;

    uint32_t m() const { return (uint32_t)map.size(); }
    uint32_t unique() const { return (uint32_t)table.size(); }
    bool passes(uint32_t id) const {
        const uint32_t b = track_hash(id, log2_bits);
        return (filter[b >> 5] >> (b & 31u)) & 1u;
    }
    // index into table, or TRACK_ABSENT (the search the device does for a lane that passed the filter)
    uint32_t find(uint32_t id) const {
        uint32_t lo = 0, hi = unique();
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (table[mid] < id) lo = mid + 1u;
            else hi = mid;
        }
        return lo < unique() && table[lo] == id ? lo : TRACK_ABSENT;
    }
};

// nullptr = fine, else what is wrong with the argument (the message names it)
inline const char* track_check_ids(const uint32_t* ids, uint32_t m) {
    if (m > TRACK_MAX_IDS) return "m is larger than SPHX_TRACK_MAX_IDS";
    if (m && !ids) return "ids is NULL with m > 0";
    return nullptr;
}
inline const char* track_check_record(uint32_t m, uint32_t max_frames, uint32_t every, bool* capacity) {
    *capacity = false;
    if (every == 0) return "every is 0";
    if ((uint64_t)max_frames * m * 16ull > TRACK_RECORD_MAX_BYTES) {
        *capacity = true;
        return "max_frames * m * 16 bytes is more than 1 GiB";
    }
    return nullptr;
}
// the ids first_id + k, k < count, must end at 2^32 at the latest
inline const char* track_check_range(uint32_t first_id, uint32_t count) {
    if ((uint64_t)first_id + count > (1ull << 32)) return "first_id + count is larger than 2^32";
    return nullptr;
}

// ids already checked (track_check_ids).  m == 0 gives the empty set (an all-zero filter of the smallest size).
inline TrackSet track_build(const uint32_t* ids, uint32_t m) {
    TrackSet s;
    s.table.assign(ids, ids + m);
    std::sort(s.table.begin(), s.table.end());
    s.table.erase(std::unique(s.table.begin(), s.table.end()), s.table.end());
    s.log2_bits = track_filter_log2(s.unique());
    s.filter.assign((size_t)1u << (s.log2_bits - 5u), 0u);
    for (uint32_t id : s.table) {
        const uint32_t b = track_hash(id, s.log2_bits);
        s.filter[b >> 5] |= 1u << (b & 31u);
    }
    s.map.resize(m);
    for (uint32_t k = 0; k < m; ++k) s.map[k] = (uint32_t)(std::lower_bound(s.table.begin(), s.table.end(), ids[k]) - s.table.begin());
    return s;
}

}  // namespace sphx
