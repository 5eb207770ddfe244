// sphx_render_merge.hpp — the host side of the tiled picture (sphx_render_merge, sphx_multi_render, sphx_multi_render_layer:
// sphx_tiles.cpp): the composite rule of include/sphx.h that folds the layers of tiles (or ranks) into the picture of the whole run.
// Plain C++ without a GPU call, shared by the library and tests/render_merge_driver.cpp.
//   Per pixel a layer says who it shows: a fluid particle (class 2: owner = its id, key = the Morton code of its cell), the boundary
// (class 1) or nothing (class 0).  A later layer replaces what has accumulated only if its class is higher, or if both are fluid and its
// key is STRICTLY greater: between the tiles of one run two fluid owners of a pixel lie in different cells (every cell belongs to one
// tile), and the one in the cell with the greater code comes later in a single context's array.  Equal keys (layers that are not tiles
// of one run) keep the earlier layer, so the fold is deterministic whatever it is given.  key, owner and rgba travel together.
#pragma once
#include <cstdint>
#include <cstring>

#include "../../include/sphx.h"

namespace sphx_render_host {

constexpr uint64_t MAX_PIXELS = 1ull << 28;  // (sphx_render's limit)

inline uint32_t cls(uint32_t owner) { return owner == (uint32_t)SPHX_RENDER_NONE ? 0u : owner == (uint32_t)SPHX_RENDER_BOUNDARY ? 1u : 2u; }
// does (owner_b, key_b) of a later layer replace (owner_a, key_a)?
inline bool replaces(uint32_t owner_a, uint32_t key_a, uint32_t owner_b, uint32_t key_b) {
    const uint32_t ca = cls(owner_a), cb = cls(owner_b);
    return cb > ca || (cb == 2u && ca == 2u && key_b > key_a);
}

// Folds the rectangle [x0, x1) x [y0, y1) of a later layer into the accumulated picture `acc` (full size, `width` pixels per row; rgba
// may be null in both or in src alone — then acc.rgba must be null too).  src is COMPACT: its arrays hold only the rectangle, row after
// row, (x1 - x0) pixels per row.  The caller guarantees x0 <= x1 <= width and y1 <= height.
inline void fold_window(const sphx_render_layer& acc, uint32_t width, const sphx_render_layer& src, uint32_t x0, uint32_t x1, uint32_t y0, uint32_t y1) {
    const uint32_t w = x1 - x0;
    for (uint32_t iy = y0; iy < y1; ++iy) {
        const size_t a0 = (size_t)iy * width + x0, s0 = (size_t)(iy - y0) * w;
        for (uint32_t k = 0; k < w; ++k) {
            const size_t a = a0 + k, s = s0 + k;
            if (!replaces(acc.owner[a], acc.key[a], src.owner[s], src.key[s])) continue;
            acc.owner[a] = src.owner[s];
            acc.key[a] = src.key[s];
            if (acc.rgba) std::memcpy(acc.rgba + 4 * a, src.rgba + 4 * s, 4);
        }
    }
}

// the argument rules of sphx_render_merge: the message behind "sphx_render_merge: ", or nullptr
inline const char* merge_error(uint32_t width, uint32_t height, const sphx_render_layer* layers, uint32_t n_layers, const sphx_render_layer* out) {
    if (!out) return "out is NULL";
    if (!out->key && !out->owner && !out->rgba) return "out requests no output (key, owner and rgba are NULL)";
    if ((uint64_t)width * height >= MAX_PIXELS) return "width * height must be < 2^28";
    if (n_layers && !layers) return "layers is NULL with n_layers > 0";
    if (n_layers == 0 && out->rgba) return "n_layers is 0 and out->rgba is requested (no layer supplies the background colour)";
    for (uint32_t k = 0; k < n_layers; ++k) {
        if (!layers[k].key || !layers[k].owner) return "a layer's key or owner is NULL";
        if (out->rgba && !layers[k].rgba) return "out->rgba is requested and a layer has no rgba";
    }
    return nullptr;
}

// The fold of the layers in the order given, pixel by pixel: what layers[0] shows, replaced by every later layer that beats what has
// accumulated.  Every array of out that is not null is written; out may alias any of the layers (a pixel of every layer is read before
// that pixel of out is written).  Arguments as checked by merge_error.
inline void merge(uint32_t width, uint32_t height, const sphx_render_layer* layers, uint32_t n_layers, const sphx_render_layer* out) {
    const size_t npix = (size_t)width * height;
    for (size_t p = 0; p < npix; ++p) {
        uint32_t owner = (uint32_t)SPHX_RENDER_NONE, key = 0u, from = 0u;
        if (n_layers) owner = layers[0].owner[p], key = layers[0].key[p];
        for (uint32_t k = 1; k < n_layers; ++k)
            if (replaces(owner, key, layers[k].owner[p], layers[k].key[p])) owner = layers[k].owner[p], key = layers[k].key[p], from = k;
        if (out->rgba) {
            uint8_t px[4];
            std::memcpy(px, layers[from].rgba + 4 * p, 4);
            std::memcpy(out->rgba + 4 * p, px, 4);
        }
        if (out->key) out->key[p] = key;
        if (out->owner) out->owner[p] = owner;
    }
}

}  // namespace sphx_render_host
