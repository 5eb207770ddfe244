// sphx_contour_merge.hpp — the host half of sphx_multi_surface_contour (include/sphx.h, "free surface of a tiled run"): which border word
// of which tile fills each apron node of a tile's padded window, and the stable K-way merge of the tiles' segment lists by cell word.
// Plain C++ without a GPU call: compiled into sphx_tiles.cpp and into tests/contour_merge_driver.cpp, which checks both without a GPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "sphx_sample_window.hpp"

namespace sphx_contour_host {

using sphx_sample_host::Window;

// ---- borders and aprons ----------------------------------------------------------------------------------------------------------------
// The BORDER of a window is its row 0 (w words) followed by its column 0 (h words) — node (ix0, iy0) is in both.  The borders of all tiles
// in rank order form one vector; off[k] is where tile k's starts, off[n] its length.
inline std::vector<size_t> border_offsets(const Window* wins, uint32_t n) {
    std::vector<size_t> off(n + 1u, 0);
    for (uint32_t k = 0; k < n; ++k) off[k + 1u] = off[k] + (wins[k].points() ? (size_t)wins[k].w() + wins[k].h() : 0);
    return off;
}

enum { NODE_OK = 0, NODE_IN_NO_WINDOW = 1, NODE_IN_SEVERAL = 2, NODE_NOT_ON_A_BORDER = 3 };

// where node (ix, iy) stands in the vector of borders; the node must lie in exactly one window, in its first row or first column
inline int border_index(const Window* wins, const size_t* off, uint32_t n, uint32_t ix, uint32_t iy, size_t* at) {
    uint32_t found = 0;
    int rc = NODE_IN_NO_WINDOW;
    for (uint32_t k = 0; k < n; ++k) {
        const Window& w = wins[k];
        if (ix < w.ix0 || ix >= w.ix1 || iy < w.iy0 || iy >= w.iy1) continue;
        if (++found > 1u) return NODE_IN_SEVERAL;
        if (iy == w.iy0) *at = off[k] + (ix - w.ix0), rc = NODE_OK;
        else if (ix == w.ix0) *at = off[k] + w.w() + (iy - w.iy0), rc = NODE_OK;
        else rc = NODE_NOT_ON_A_BORDER;
    }
    return rc;
}

// ax / ay of window w in a lattice of nx x ny nodes: an apron column / row exists (the window does not end at the lattice's edge)
inline uint32_t apron_ax(const Window& w, uint32_t nx) { return w.points() && w.ix1 < nx ? 1u : 0u; }
inline uint32_t apron_ay(const Window& w, uint32_t ny) { return w.points() && w.iy1 < ny ? 1u : 0u; }
inline uint32_t apron_words(const Window& w, uint32_t nx, uint32_t ny) {
    const uint32_t ax = apron_ax(w, nx), ay = apron_ay(w, ny);
    return (ax ? w.h() : 0u) + (ay ? w.w() : 0u) + (ax & ay);
}
// cells tile k cuts: those whose node 0 lies in its window
inline uint64_t window_cells(const Window& w, uint32_t nx, uint32_t ny) {
    if (!w.points()) return 0;
    return (uint64_t)(w.w() - 1u + apron_ax(w, nx)) * (w.h() - 1u + apron_ay(w, ny));
}

// The apron of tile k in the order k_contour_apron_unpack reads it — column ix1 of rows [iy0, iy1) if ax, row iy1 of columns [ix0, ix1) if
// ay, the corner (ix1, iy1) if both — as indices into the vector of borders.  NODE_OK, or what is wrong with the first bad node (*bad_ix,
// *bad_iy): a missing node is an error of the windows, never a zero.
inline int apron_indices(const Window* wins, const size_t* off, uint32_t n, uint32_t nx, uint32_t ny, uint32_t k, std::vector<size_t>& idx, uint32_t* bad_ix,
                         uint32_t* bad_iy) {
    idx.clear();
    const Window& w = wins[k];
    const uint32_t ax = apron_ax(w, nx), ay = apron_ay(w, ny);
    auto add = [&](uint32_t ix, uint32_t iy) {
        size_t at = 0;
        const int rc = border_index(wins, off, n, ix, iy, &at);
        if (rc) *bad_ix = ix, *bad_iy = iy;
        else idx.push_back(at);
        return rc;
    };
    int rc;
    if (ax)
        for (uint32_t iy = w.iy0; iy < w.iy1; ++iy)
            if ((rc = add(w.ix1, iy))) return rc;
    if (ay)
        for (uint32_t ix = w.ix0; ix < w.ix1; ++ix)
            if ((rc = add(ix, w.iy1))) return rc;
    if (ax & ay)
        if ((rc = add(w.ix1, w.iy1))) return rc;
    return NODE_OK;
}

// do the windows partition the lattice?  (disjoint by construction of the layouts; the sum of their points says whether a node is missed)
inline bool windows_cover(const Window* wins, uint32_t n, uint32_t nx, uint32_t ny) {
    uint64_t covered = 0;
    for (uint32_t k = 0; k < n; ++k) {
        if (wins[k].ix1 > nx || wins[k].iy1 > ny) return false;
        covered += wins[k].points();
    }
    return covered == (uint64_t)nx * ny;
}

// ---- the merge ------------------------------------------------------------------------------------------------------------------------
struct MergePart {
    const float* segments;  // [stored][4] or NULL
    const uint32_t* cell;   // [stored] ascending (equal words: a saddle cell's two segments, whose order is kept)
    const int32_t* tile;    // [stored] or NULL
    int32_t tile_const;     // ... then this for every entry
    uint32_t stored;
};
struct MergeOut {
    float* segments;
    uint32_t* cell;
    int32_t* tile;
};
// Stable K-way merge by cell word: of equal words the entry of the earlier part comes first, within a part the stored order is kept.
// Writes the first min(cap, sum of stored) entries and returns that number; nothing at or behind cap is written.  The outputs must not
// alias a part.
inline uint32_t merge(const MergePart* parts, uint32_t n_parts, uint32_t cap, const MergeOut& out) {
    std::vector<uint32_t> head(n_parts, 0u);
    uint32_t written = 0;
    while (written < cap) {
        uint32_t best = n_parts;
        for (uint32_t p = 0; p < n_parts; ++p)
            if (head[p] < parts[p].stored && (best == n_parts || parts[p].cell[head[p]] < parts[best].cell[head[best]])) best = p;
        if (best == n_parts) break;
        const MergePart& q = parts[best];
        const uint32_t j = head[best]++;
        if (out.segments && q.segments) std::memcpy(out.segments + 4 * (size_t)written, q.segments + 4 * (size_t)j, 16);
        if (out.cell) out.cell[written] = q.cell[j];
        if (out.tile) out.tile[written] = q.tile ? q.tile[j] : q.tile_const;
        ++written;
    }
    return written;
}

}  // namespace sphx_contour_host
