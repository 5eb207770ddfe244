// Stand-alone driver for the host half of a tracked id set (yasph2d_amd/csrc/sphx_track_set.hpp): plain C++, compiled by
// tests/test_track_host.py with the address and undefined-behaviour sanitizers (any report aborts the program).
//   track_set_driver <check>      check = empty | one | duplicates | maximum | extremes | filter | checks
// prints "ok <assertions>" and returns 0, or names the first failed assertion and returns 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "sphx_track_set.hpp"

using namespace sphx;

static long g_checks = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        ++g_checks;                                                            \
        if (!(cond)) {                                                         \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
            std::exit(1);                                                      \
        }                                                                      \
    } while (0)

// the invariants of any built set, against the ids it was built from
static void check_set(const TrackSet& s, const std::vector<uint32_t>& ids) {
    CHECK(s.m() == ids.size());
    CHECK(s.unique() <= s.m());
    for (uint32_t k = 1; k < s.unique(); ++k) CHECK(s.table[k - 1] < s.table[k]);  // ascending, no repeats
    CHECK(s.log2_bits >= TRACK_FILTER_LOG2_MIN && s.log2_bits <= TRACK_FILTER_LOG2_MAX);
    CHECK(s.filter.size() == ((size_t)1 << s.log2_bits) / 32);
    CHECK(s.filter.size() * 4 <= 32768);  // the LDS the look-up stages it in
    for (uint32_t k = 0; k < s.m(); ++k) {
        CHECK(s.map[k] < s.unique());
        CHECK(s.table[s.map[k]] == ids[k]);  // the caller's order comes back through the map
        CHECK(s.passes(ids[k]));             // no member is ever filtered out
        CHECK(s.find(ids[k]) == s.map[k]);
    }
    size_t bits = 0;
    for (uint32_t w : s.filter) bits += (size_t)__builtin_popcount(w);
    CHECK(bits <= s.unique());
    CHECK(s.unique() == 0 || bits > 0);
}

static uint32_t lcg(uint32_t& x) { return x = x * 1664525u + 1013904223u; }

int main(int argc, char** argv) {
    const std::string c = argc > 1 ? argv[1] : "";
    if (c == "empty") {
        const TrackSet s = track_build(nullptr, 0);
        check_set(s, {});
        CHECK(s.unique() == 0 && s.find(0) == TRACK_ABSENT && s.find(0xFFFFFFFFu) == TRACK_ABSENT);
        for (uint32_t w : s.filter) CHECK(w == 0);
        CHECK(!s.passes(0) && !s.passes(12345));
    } else if (c == "one") {
        for (uint32_t id : {0u, 1u, 4049u, 0x80000000u, 0xFFFFFFFFu}) {
            const std::vector<uint32_t> ids{id};
            const TrackSet s = track_build(ids.data(), 1);
            check_set(s, ids);
            CHECK(s.unique() == 1 && s.table[0] == id && s.find(id) == 0 && s.find(id ^ 1u) == TRACK_ABSENT);
        }
    } else if (c == "duplicates") {
        const std::vector<uint32_t> all(1000, 77u);
        TrackSet s = track_build(all.data(), 1000);
        check_set(s, all);
        CHECK(s.unique() == 1);
        for (uint32_t k = 0; k < 1000; ++k) CHECK(s.map[k] == 0);
        const std::vector<uint32_t> mixed{5, 3, 5, 9, 3, 3, 0, 9};
        s = track_build(mixed.data(), (uint32_t)mixed.size());
        check_set(s, mixed);
        CHECK(s.unique() == 4 && s.map[0] == s.map[2] && s.map[1] == s.map[4] && s.map[4] == s.map[5] && s.map[3] == s.map[7] && s.map[6] == 0);
    } else if (c == "maximum") {
        std::vector<uint32_t> ids(TRACK_MAX_IDS);
        std::iota(ids.begin(), ids.end(), 100u);
        TrackSet s = track_build(ids.data(), TRACK_MAX_IDS);
        check_set(s, ids);
        CHECK(s.unique() == TRACK_MAX_IDS && s.log2_bits == TRACK_FILTER_LOG2_MAX && s.filter.size() * 4 == 32768);
        uint32_t x = 99;
        for (auto& v : ids) v = lcg(x);
        s = track_build(ids.data(), TRACK_MAX_IDS);
        check_set(s, ids);
        for (uint32_t k = 0; k < TRACK_MAX_IDS; ++k) ids[k] = 0xFFFFFFFFu - 16u * k;  // descending, stride 16
        s = track_build(ids.data(), TRACK_MAX_IDS);
        check_set(s, ids);
        CHECK(s.table.front() == 0xFFFFFFFFu - 16u * (TRACK_MAX_IDS - 1) && s.table.back() == 0xFFFFFFFFu);
    } else if (c == "extremes") {
        const std::vector<uint32_t> ids{0xFFFFFFFFu, 0u, 0xFFFFFFFEu, 1u, 0x7FFFFFFFu, 0x80000000u, 0u, 0xFFFFFFFFu};
        const TrackSet s = track_build(ids.data(), (uint32_t)ids.size());
        check_set(s, ids);
        CHECK(s.unique() == 6 && s.table.front() == 0 && s.table.back() == 0xFFFFFFFFu);
        CHECK(s.find(2) == TRACK_ABSENT && s.find(0xFFFFFFFDu) == TRACK_ABSENT);
        for (uint32_t l = 1; l <= 32; ++l) {  // the hash stays inside the filter for every size
            CHECK(l == 32 || track_hash(0xFFFFFFFFu, l) < (1u << l));
            CHECK(track_hash(0u, l) == 0u);
        }
    } else if (c == "filter") {
        // every member passes, whatever the size; the share of non-members that pass stays near 1 - exp(-1/16) ~ 6 % (16 bits per id)
        uint32_t x = 7;
        for (uint32_t m : {1u, 2u, 16u, 63u, 64u, 65u, 1000u, 1024u, 4097u, TRACK_MAX_IDS}) {
            std::vector<uint32_t> ids(m);
            for (auto& v : ids) v = lcg(x);
            const TrackSet s = track_build(ids.data(), m);
            check_set(s, ids);
            CHECK(s.log2_bits == track_filter_log2(s.unique()));
            CHECK(((uint64_t)1 << s.log2_bits) >= 16ull * s.unique() || s.log2_bits == TRACK_FILTER_LOG2_MAX);
            uint32_t pass = 0, probes = 200000;
            for (uint32_t k = 0; k < probes; ++k) {
                const uint32_t id = lcg(x);
                if (s.find(id) == TRACK_ABSENT && s.passes(id)) ++pass;
            }
            CHECK(pass < probes / 10);  // < 10 %
        }
        // consecutive ids (what sphx_upload hands out) spread as well
        std::vector<uint32_t> run(TRACK_MAX_IDS);
        std::iota(run.begin(), run.end(), 0u);
        const TrackSet s = track_build(run.data(), TRACK_MAX_IDS);
        uint32_t pass = 0;
        for (uint32_t id = TRACK_MAX_IDS; id < TRACK_MAX_IDS + 200000u; ++id) pass += s.passes(id) ? 1u : 0u;
        CHECK(pass < 20000u);
    } else if (c == "checks") {
        const uint32_t one = 1;
        bool cap = false;
        CHECK(track_check_ids(nullptr, 0) == nullptr && track_check_ids(&one, 1) == nullptr && track_check_ids(&one, TRACK_MAX_IDS) == nullptr);
        CHECK(std::strstr(track_check_ids(nullptr, 1), "ids") != nullptr);
        CHECK(std::strstr(track_check_ids(&one, TRACK_MAX_IDS + 1), "SPHX_TRACK_MAX_IDS") != nullptr);
        CHECK(std::strstr(track_check_ids(nullptr, 0xFFFFFFFFu), "SPHX_TRACK_MAX_IDS") != nullptr);
        CHECK(track_check_record(16, 100, 1, &cap) == nullptr && !cap);
        CHECK(std::strstr(track_check_record(16, 100, 0, &cap), "every") != nullptr && !cap);
        CHECK(track_check_record(TRACK_MAX_IDS, 4096, 1, &cap) == nullptr && !cap);        // exactly 1 GiB
        CHECK(track_check_record(TRACK_MAX_IDS, 4097, 1, &cap) != nullptr && cap);
        CHECK(track_check_record(TRACK_MAX_IDS, 0xFFFFFFFFu, 0xFFFFFFFFu, &cap) != nullptr && cap);  // (no 32-bit overflow in the product)
        CHECK(track_check_range(0, 0) == nullptr && track_check_range(0, 0xFFFFFFFFu) == nullptr && track_check_range(1, 0xFFFFFFFFu) == nullptr);
        CHECK(track_check_range(0xFFFFFFFFu, 1) == nullptr && track_check_range(0xFFFFFFFFu, 0) == nullptr);
        CHECK(std::strstr(track_check_range(2, 0xFFFFFFFFu), "first_id + count") != nullptr);
        CHECK(track_check_range(0xFFFFFFFFu, 2) != nullptr && track_check_range(0xFFFFFFFFu, 0xFFFFFFFFu) != nullptr);
        CHECK(TRACK_MAX_IDS == 16384 && TRACK_ABSENT == 0xFFFFFFFFu && TRACK_ABSENT_WORD == 0x7FC00000u);
    } else {
        std::printf("usage: track_set_driver empty|one|duplicates|maximum|extremes|filter|checks\n");
        return 2;
    }
    std::printf("ok %ld\n", g_checks);
    return 0;
}
