// sphx_query_merge.hpp — the host side of sphx_multi_query_radius and sphx_query_merge (include/sphx.h, "neighbour queries of a tiled
// run"): the parts of several tiles (or ranks) folded into ONE CSR list in the caller's point order.  Pure host code, no HIP include
// (tests/query_merge_driver.cpp compiles it alone), like sphx_sample_window.hpp and sphx_contour_merge.hpp.
//
// A part comes in one of two forms:
//   full     (a rank's answer, as sphx_multi_query_radius returns it): record k IS point k — offsets[m + 1], tile[m] and the nearest
//            arrays [m]; a point the part does not answer has tile < 0 and an empty range;
//   compact  (a tile's answer, as sphx_tile_query_fetch returns it): n records in ascending point index — point[n], the exclusive
//            offset[n] of each record's entries, the part's total, the nearest arrays [n]; every record is answered by tile `rank`.
// In both the entries of consecutive records follow each other, and the part HOLDS only the first `held` of them (its own capacity).
// Per point the part with tile >= 0 answers, the lowest tile if several have one; nobody: an empty range, tile -1, nearest NONE / +inf.
// Maximal runs of consecutive points that one part answers with consecutive records are copied with one memcpy per array.  Nothing at or
// behind out.cap is ever written; an entry that has to be copied and that its part does not hold is SPHX_ERR_CAPACITY.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

namespace sphx_query_host {

constexpr int OK = 0, ERR_CAPACITY = 7;  // SPHX_OK, SPHX_ERR_CAPACITY (checked against sphx.h where both are visible)
constexpr uint32_t NONE = 0xFFFFFFFFu, INF_WORD = 0x7F800000u;

struct Part {
    const uint32_t* point = nullptr;    // compact form: [n] ascending point indices; nullptr: full form (n == m)
    uint32_t n = 0;                     // records
    const uint64_t* offset = nullptr;   // [n] (+ [n] = total in the full form) first entry of record k
    uint64_t total = 0;                 // compact form: the end of the last record
    const int32_t* tile = nullptr;      // full form: [n] who answered; nullptr: every record by `rank`
    int32_t rank = 0;
    const uint32_t* nearest_id = nullptr;    // [n] each, or nullptr
    const uint32_t* nearest_slot = nullptr;
    const uint32_t* nearest_d2 = nullptr;    // (the float's word)
    const uint32_t* id = nullptr;            // [held] each, or nullptr
    const uint32_t* d2 = nullptr;
    const uint32_t* slot = nullptr;
    uint64_t held = 0;                       // entries the arrays hold: min(the part's count, its capacity)
    const uint32_t* id_map = nullptr;        // boundary ids: id -> id_map[id] on the way out (a tile's clipped set -> the caller's order)
    uint32_t id_map_n = 0;

    uint64_t begin(uint32_t k) const { return offset[k]; }
    uint64_t end(uint32_t k) const { return (point == nullptr || k + 1u < n) ? offset[k + 1u] : total; }
};

struct Out {
    uint64_t* offsets = nullptr;  // [m + 1] or nullptr
    uint32_t* id = nullptr;       // [cap] each, or nullptr
    uint32_t* d2 = nullptr;
    uint32_t* slot = nullptr;
    uint32_t* nearest_id = nullptr;  // [m] each, or nullptr
    uint32_t* nearest_slot = nullptr;
    uint32_t* nearest_d2 = nullptr;
    int32_t* tile = nullptr;         // [m] or nullptr
    uint64_t* count = nullptr;       // [1]
    uint64_t cap = 0;
};

inline uint32_t map_id(const Part& p, uint32_t id) { return (p.id_map && id < p.id_map_n) ? p.id_map[id] : id; }

inline int merge(uint32_t m, const Part* parts, uint32_t n_parts, const Out& out) {
    // who answers each point: (part, record), the lowest tile winning
    std::vector<uint32_t> who(m, NONE), rec(m, 0u);
    std::vector<int32_t> who_tile(m, -1);
    for (uint32_t p = 0; p < n_parts; ++p) {
        const Part& q = parts[p];
        for (uint32_t k = 0; k < q.n; ++k) {
            const uint32_t i = q.point ? q.point[k] : k;
            const int32_t t = q.tile ? q.tile[k] : q.rank;
            if (i >= m || t < 0) continue;
            if (who[i] == NONE || t < who_tile[i]) who[i] = p, rec[i] = k, who_tile[i] = t;
        }
    }
    const bool lists = out.id || out.d2 || out.slot;
    uint64_t pos = 0;
    int rc = OK;
    uint32_t i = 0;
    while (i < m) {
        const uint32_t p = who[i];
        if (p == NONE) {
            if (out.offsets) out.offsets[i] = pos;
            if (out.tile) out.tile[i] = -1;
            if (out.nearest_id) out.nearest_id[i] = NONE;
            if (out.nearest_slot) out.nearest_slot[i] = NONE;
            if (out.nearest_d2) out.nearest_d2[i] = INF_WORD;
            ++i;
            continue;
        }
        const Part& q = parts[p];
        const uint32_t k0 = rec[i];
        uint32_t len = 1;  // the run: points i .. i + len - 1 are records k0 .. k0 + len - 1 of part p
        while (i + len < m && who[i + len] == p && rec[i + len] == k0 + len && q.end(k0 + len - 1u) == q.begin(k0 + len)) ++len;
        const uint64_t src = q.begin(k0), n_ent = q.end(k0 + len - 1u) - src;
        for (uint32_t j = 0; j < len; ++j) {
            if (out.offsets) out.offsets[i + j] = pos + (q.begin(k0 + j) - src);
            if (out.tile) out.tile[i + j] = who_tile[i + j];
        }
        if (out.nearest_id && q.nearest_id) {
            std::memcpy(out.nearest_id + i, q.nearest_id + k0, (size_t)len * 4);
            if (q.id_map)
                for (uint32_t j = 0; j < len; ++j)
                    if (out.nearest_id[i + j] != NONE) out.nearest_id[i + j] = map_id(q, out.nearest_id[i + j]);
        }
        if (out.nearest_slot && q.nearest_slot) std::memcpy(out.nearest_slot + i, q.nearest_slot + k0, (size_t)len * 4);
        if (out.nearest_d2 && q.nearest_d2) std::memcpy(out.nearest_d2 + i, q.nearest_d2 + k0, (size_t)len * 4);
        if (lists && pos < out.cap && n_ent) {
            uint64_t n_copy = n_ent < out.cap - pos ? n_ent : out.cap - pos;
            if (src + n_copy > q.held) {  // the part truncated an entry this result needs
                rc = ERR_CAPACITY;
                n_copy = src < q.held ? q.held - src : 0u;
            }
            if (n_copy) {
                if (out.id && q.id) {
                    std::memcpy(out.id + pos, q.id + src, (size_t)n_copy * 4);
                    if (q.id_map)
                        for (uint64_t e = 0; e < n_copy; ++e) out.id[pos + e] = map_id(q, out.id[pos + e]);
                }
                if (out.d2 && q.d2) std::memcpy(out.d2 + pos, q.d2 + src, (size_t)n_copy * 4);
                if (out.slot && q.slot) std::memcpy(out.slot + pos, q.slot + src, (size_t)n_copy * 4);
            }
        }
        pos += n_ent;
        i += len;
    }
    if (out.offsets) out.offsets[m] = pos;
    if (out.count) out.count[0] = pos;
    return rc;
}

}  // namespace sphx_query_host
