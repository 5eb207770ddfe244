// sphx_multi_edit.hpp — the host side of an edit of a tiled run (sphx_multi_append / sphx_multi_remove: sphx_tiles.cpp, the contract is in
// include/sphx.h, "emitting and draining fluid in a tiled run"): which tile owns a new record, the rules of the multi's id counter and the
// check of the caller's positions.  Plain C++ without a GPU call, shared by the library and tests/multi_edit_driver.cpp.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

namespace sphx_multi_edit {

constexpr uint64_t ID_LIMIT = 1ull << 31;  // bit 31 of a tile's id word is the owner bit: ids stay below it

struct CellRect {
    uint32_t x0, x1, y0, y1;  // cells, half-open
};

// GridProperties::position_to_mortoncellpos (neighborhood_search.rs:52-58) along one axis: the f32 operations of the device and of the
// set-up's decomposition (sphx_tiles.cpp)
inline uint32_t cell_coord(float v, float grid_min, float cell_inv) {
    const float c = (v - grid_min) * cell_inv;
    if (!(c > 0.0f)) return 0;  // NaN -> 0 like Rust's saturating cast
    if (c >= 65535.0f) return 65535;
    return (uint32_t)c;
}
inline bool in_rect(uint32_t cx, uint32_t cy, const CellRect& r) { return cx >= r.x0 && cx < r.x1 && cy >= r.y0 && cy < r.y1; }

// the tile whose rectangle holds the cell: the first in ascending rank, as the set-up takes it (the rectangles of a layout are disjoint and
// cover the u16 cell range, so there is exactly one); -1 for rectangles that leave the cell out
inline int owner_of(uint32_t cx, uint32_t cy, const CellRect* rects, int world) {
    for (int r = 0; r < world; ++r)
        if (in_rect(cx, cy, rects[r])) return r;
    return -1;
}

// owner[k] = the tile that record k goes to.  A record exactly on a cut belongs to the tile on the high side (its cell is the cut's).
inline void route(const float* pos_xy, uint32_t n_new, const float grid_min[2], float cell_inv, const CellRect* rects, int world, std::vector<int>& owner) {
    owner.resize(n_new);
    int last = 0;  // (neighbouring records of a block mostly share their owner: try that rectangle first)
    for (uint32_t k = 0; k < n_new; ++k) {
        const uint32_t cx = cell_coord(pos_xy[2 * (size_t)k], grid_min[0], cell_inv), cy = cell_coord(pos_xy[2 * (size_t)k + 1], grid_min[1], cell_inv);
        int a = world > 0 && in_rect(cx, cy, rects[last]) ? last : owner_of(cx, cy, rects, world);
        owner[k] = a;
        if (a >= 0) last = a;
    }
}

// the index of the first record with a non-finite coordinate, or n_new.  (A NaN x is the mark of a retired record; an infinite position
// has no cell.)
inline uint32_t first_nonfinite(const float* pos_xy, uint32_t n_new) {
    for (uint32_t k = 0; k < n_new; ++k)
        if (!std::isfinite(pos_xy[2 * (size_t)k]) || !std::isfinite(pos_xy[2 * (size_t)k + 1])) return k;
    return n_new;
}

// The id counter = the id the next appended record gets.  After an upload of n particles without ids: n (they are numbered 0 .. n - 1);
// with ids, and after a checkpoint's load: 1 + the greatest id (0 for an empty set).
inline uint64_t counter_after(const uint32_t* ids, uint64_t n) {
    if (!ids) return n;
    uint64_t next = 0;
    for (uint64_t i = 0; i < n; ++i) next = next > (uint64_t)ids[i] + 1u ? next : (uint64_t)ids[i] + 1u;
    return next;
}
// n_new ids from the counter: false (and nothing taken) if one of them would reach ID_LIMIT.  *first_id is reported either way, and for
// n_new == 0.
inline bool take_ids(uint64_t& counter, uint32_t n_new, uint32_t* first_id) {
    if (first_id) *first_id = (uint32_t)(counter < ID_LIMIT ? counter : ID_LIMIT);
    if (n_new && counter + n_new > ID_LIMIT) return false;
    counter += n_new;
    return true;
}

}  // namespace sphx_multi_edit
