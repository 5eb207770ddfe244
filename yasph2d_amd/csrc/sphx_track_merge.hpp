// sphx_track_merge.hpp — the host side of following particles in a tiled run (sphx_multi_track_*, sphx_multi_download_by_id,
// sphx_track_merge, sphx_track_merge_frames: sphx_tiles.cpp): the rule of include/sphx.h that folds the parts of several tiles (or ranks)
// into one answer, and the scatter of a tile's packed window records into id-ordered arrays.  Plain C++ without a GPU call, shared by
// the library and tests/track_merge_driver.cpp.
//   An entry of the answer is held by at most one part in a run whose ids are unique.  If several parts hold it (a state loaded with
// repeated ids), the greatest (tile rank, slot) wins — the single context's "highest slot" carried across tiles; an equal pair (parts
// that are not tiles of one run) keeps the earlier part, so the fold is deterministic whatever it is given.  Presence is the tile word
// (a part) or the slot word (a tile's own output), never the float bits: a particle may carry 0x7FC00000.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/sphx.h"

namespace sphx_track_host {

constexpr uint32_t ABSENT = 0xFFFFFFFFu;      // == SPHX_TRACK_ABSENT
constexpr uint32_t ABSENT_WORD = 0x7FC00000u;  // every float of an absent id
constexpr uint32_t WINDOW = 1u << 22;          // ids per pass of the by-id download (== TRACK_WINDOW of sphx_track.inc)
constexpr uint32_t RECORD_WORDS = 8;           // a packed window record: {index, slot, x, y, vx, vy, density, 0}
constexpr uint32_t HEADER_WORDS = 4;           // ... behind the tile's counter (16 bytes: the records stay 16-byte aligned)
constexpr uint64_t RECORD_MAX_BYTES = 1ull << 30;  // a tile's recording: max_frames * unique * FRAME_ENTRY_BYTES
constexpr uint32_t FRAME_ENTRY_BYTES = 20;     // {x, y, vx, vy} + the presence word

static_assert(ABSENT == SPHX_TRACK_ABSENT, "the absent word of sphx.h");

// the accumulated answer: n entries; tile and slot are always there (the fold compares them), the float arrays as the caller asked
struct Acc {
    uint32_t* tile;
    uint32_t* slot;
    uint32_t* pos;      // [2n] or null
    uint32_t* vel;      // [2n] or null
    uint32_t* density;  // [n] or null
};

inline void fill_words(uint32_t* p, size_t n, uint32_t w) {
    for (size_t k = 0; k < n; ++k) p[k] = w;
}
// every entry absent
inline void fill_absent(const Acc& a, size_t n) {
    fill_words(a.tile, n, ABSENT);
    fill_words(a.slot, n, ABSENT);
    if (a.pos) fill_words(a.pos, 2 * n, ABSENT_WORD);
    if (a.vel) fill_words(a.vel, 2 * n, ABSENT_WORD);
    if (a.density) fill_words(a.density, n, ABSENT_WORD);
}

// does (tile, slot) of a candidate replace what entry k of acc holds?
inline bool replaces(const Acc& a, size_t k, uint32_t tile, uint32_t slot) {
    if (a.tile[k] == ABSENT) return true;
    return tile > a.tile[k] || (tile == a.tile[k] && slot > a.slot[k]);
}

// One tile's fetch (per distinct id j < unique: slot word, {x, y, vx, vy}, density) into the answer over the distinct ids.
inline void fold_unique(const Acc& a, uint32_t tile, uint32_t unique, const uint32_t* slot, const uint32_t* xyvv, const uint32_t* density) {
    for (uint32_t j = 0; j < unique; ++j) {
        if (slot[j] == ABSENT || !replaces(a, j, tile, slot[j])) continue;
        a.tile[j] = tile;
        a.slot[j] = slot[j];
        if (a.pos) std::memcpy(a.pos + 2 * (size_t)j, xyvv + 4 * (size_t)j, 8);
        if (a.vel) std::memcpy(a.vel + 2 * (size_t)j, xyvv + 4 * (size_t)j + 2, 8);
        if (a.density) a.density[j] = density[j];
    }
}

// One tile's packed window records (any order) into the answer of a window of `count` ids.  A record whose index is not below count
// is skipped and counted in the return value (a sound tile never writes one).
inline uint32_t scatter_records(const Acc& a, uint32_t tile, uint32_t count, const uint32_t* records, uint32_t n_records) {
    uint32_t bad = 0;
    for (uint32_t r = 0; r < n_records; ++r) {
        const uint32_t* w = records + (size_t)r * RECORD_WORDS;
        const uint32_t k = w[0];
        if (k >= count) {
            bad += 1u;
            continue;
        }
        if (!replaces(a, k, tile, w[1])) continue;
        a.tile[k] = tile;
        a.slot[k] = w[1];
        if (a.pos) std::memcpy(a.pos + 2 * (size_t)k, w + 2, 8);
        if (a.vel) std::memcpy(a.vel + 2 * (size_t)k, w + 4, 8);
        if (a.density) a.density[k] = w[6];
    }
    return bad;
}

// The answer over the distinct ids (src, `unique` entries) in the caller's order: entry k of dst = entry map[k] of src.
inline void expand(const Acc& dst, const Acc& src, const uint32_t* map, uint32_t m) {
    for (uint32_t k = 0; k < m; ++k) {
        const size_t j = map[k];
        dst.tile[k] = src.tile[j];
        dst.slot[k] = src.slot[j];
        if (dst.pos) std::memcpy(dst.pos + 2 * (size_t)k, src.pos + 2 * j, 8);
        if (dst.vel) std::memcpy(dst.vel + 2 * (size_t)k, src.vel + 2 * j, 8);
        if (dst.density) dst.density[k] = src.density[j];
    }
}

inline uint32_t count_present(const uint32_t* tile, size_t n) {
    uint32_t c = 0;
    for (size_t k = 0; k < n; ++k) c += tile[k] != ABSENT;
    return c;
}

// ---- sphx_track_merge: parts that are answers themselves (what the ranks of a run returned) --------------------------------------
inline const char* merge_error(uint32_t m, const sphx_multi_track_out* parts, uint32_t n_parts, const sphx_multi_track_out* out) {
    if (!out) return "out is NULL";
    if (!out->tile && !out->slot && !out->pos && !out->vel && !out->density) return "out requests no output (every pointer is NULL)";
    if (n_parts && !parts) return "parts is NULL with n_parts > 0";
    if (!m) return nullptr;
    for (uint32_t p = 0; p < n_parts; ++p) {
        if (!parts[p].tile || !parts[p].slot) return "a part lacks tile or slot (the fold compares them)";
        if ((out->pos && !parts[p].pos) || (out->vel && !parts[p].vel) || (out->density && !parts[p].density)) return "out asks for an array a part lacks";
    }
    return nullptr;
}
// acc: tile and slot non-null (the caller lends scratch where out has none); arguments checked by merge_error
inline void merge(uint32_t m, const sphx_multi_track_out* parts, uint32_t n_parts, const Acc& acc) {
    fill_absent(acc, m);
    for (uint32_t p = 0; p < n_parts; ++p) {
        const sphx_multi_track_out& s = parts[p];
        for (uint32_t k = 0; k < m; ++k) {
            if (s.tile[k] == ABSENT || !replaces(acc, k, s.tile[k], s.slot[k])) continue;
            acc.tile[k] = s.tile[k];
            acc.slot[k] = s.slot[k];
            if (acc.pos) std::memcpy(acc.pos + 2 * (size_t)k, s.pos + 2 * (size_t)k, 8);
            if (acc.vel) std::memcpy(acc.vel + 2 * (size_t)k, s.vel + 2 * (size_t)k, 8);
            if (acc.density) std::memcpy(acc.density + k, s.density + k, 4);
        }
    }
}

// ---- frames: n entries of {x, y, vx, vy} and their tile words; the greatest tile wins, an equal tile keeps the earlier part --------
inline const char* merge_frames_error(uint64_t n, const float* const* parts, const uint32_t* const* parts_tile, uint32_t n_parts, const float* out) {
    if (n && !out) return "out is NULL";
    if (n_parts && (!parts || !parts_tile)) return "parts or parts_tile is NULL with n_parts > 0";
    for (uint32_t p = 0; n && p < n_parts; ++p)
        if (!parts[p] || !parts_tile[p]) return "a part or its tile array is NULL";
    return nullptr;
}
// out_tile non-null (the caller lends scratch)
inline void merge_frames(uint64_t n, const float* const* parts, const uint32_t* const* parts_tile, uint32_t n_parts, float* out, uint32_t* out_tile) {
    uint32_t* const o = (uint32_t*)out;
    fill_words(o, 4 * (size_t)n, ABSENT_WORD);
    fill_words(out_tile, (size_t)n, ABSENT);
    for (uint32_t p = 0; p < n_parts; ++p)
        for (size_t k = 0; k < n; ++k) {
            const uint32_t t = parts_tile[p][k];
            if (t == ABSENT || (out_tile[k] != ABSENT && t <= out_tile[k])) continue;
            out_tile[k] = t;
            std::memcpy(o + 4 * k, parts[p] + 4 * k, 16);
        }
}

// One tile's frames (per frame: [unique] {x, y, vx, vy}, [unique] presence words) into frames over the distinct ids
inline void fold_frames_unique(uint32_t* xyvv, uint32_t* tile_w, uint32_t* slot_w, uint32_t tile, size_t n, const uint32_t* t_xyvv, const uint32_t* t_slot) {
    for (size_t k = 0; k < n; ++k) {
        if (t_slot[k] == ABSENT) continue;
        if (tile_w[k] != ABSENT && !(tile > tile_w[k] || (tile == tile_w[k] && t_slot[k] > slot_w[k]))) continue;
        tile_w[k] = tile;
        slot_w[k] = t_slot[k];
        std::memcpy(xyvv + 4 * k, t_xyvv + 4 * k, 16);
    }
}

}  // namespace sphx_track_host
