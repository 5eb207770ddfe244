// sphx_stats_merge.hpp — the host side of the tiled fluid statistics (sphx_multi_fluid_stats, sphx_multi_stats_read: sphx_tiles.cpp):
// a (+) b of two sphx_stats_rec as the device forms it (stats_merge, sphx_stats.inc), the fold of the tiles' records in ascending tile
// rank, and the encoding that carries a record across ranks through a transport that only sums doubles.  Plain C++ without a GPU call,
// shared by the library and tests/stats_merge_driver.cpp.  Compile without value-changing floating-point options (no -ffast-math).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>

#include "../../include/sphx.h"

namespace sphx_stats_host {

// key(f) is monotone in f over the floats without NaN and puts -0 below +0 (stats_key of sphx_stats.inc); key is its own inverse
inline int32_t key(float f) {
    int32_t i;
    std::memcpy(&i, &f, 4);
    return i ^ ((i >> 31) & 0x7FFFFFFF);
}
inline float unkey(int32_t k) {
    const int32_t i = k ^ ((k >> 31) & 0x7FFFFFFF);
    float f;
    std::memcpy(&f, &i, 4);
    return f;
}
inline float key_min(float a, float b) { return unkey(key(a) < key(b) ? key(a) : key(b)); }  // among zeros: -0 if one is present
inline float key_max(float a, float b) { return unkey(key(a) > key(b) ? key(a) : key(b)); }  // ... +0 if one is present

// what a tile without an owned particle returns: the neutral element of (+) but for the sign of a zero sum
inline sphx_stats_rec empty(uint32_t density_valid) {
    sphx_stats_rec r;
    std::memset(&r, 0, sizeof(r));
    r.density_valid = density_valid;
    const float inf = std::numeric_limits<float>::infinity();
    r.min_pos[0] = r.min_pos[1] = r.min_density = inf;
    r.max_pos[0] = r.max_pos[1] = r.max_density = -inf;
    return r;
}

// a (+) b: every sum a + b in this order, integer addition for the counts, key-min / key-max for the extremes, fmax for max_speed_sq;
// density_valid only if both have it
inline sphx_stats_rec merge(const sphx_stats_rec& a, const sphx_stats_rec& b) {
    sphx_stats_rec r;
    std::memset(&r, 0, sizeof(r));
    r.count = a.count + b.count;
    r.nonfinite = a.nonfinite + b.nonfinite;
    r.density_count = a.density_count + b.density_count;
    r.density_valid = (a.density_valid && b.density_valid) ? 1u : 0u;
    for (int j = 0; j < 2; ++j) {
        r.sum_pos[j] = a.sum_pos[j] + b.sum_pos[j];
        r.sum_vel[j] = a.sum_vel[j] + b.sum_vel[j];
        r.min_pos[j] = key_min(a.min_pos[j], b.min_pos[j]);
        r.max_pos[j] = key_max(a.max_pos[j], b.max_pos[j]);
    }
    r.sum_speed_sq = a.sum_speed_sq + b.sum_speed_sq;
    r.sum_angular = a.sum_angular + b.sum_angular;
    r.sum_density = a.sum_density + b.sum_density;
    r.sum_density_sq = a.sum_density_sq + b.sum_density_sq;
    r.max_speed_sq = std::fmax(a.max_speed_sq, b.max_speed_sq);
    r.min_density = key_min(a.min_density, b.min_density);
    r.max_density = key_max(a.max_density, b.max_density);
    return r;
}

// record `r` of the whole fluid from tiles[t * stride + r], t = 0 .. world - 1: ((tile 0 (+) tile 1) (+) tile 2) ... — ascending rank
inline sphx_stats_rec fold(const sphx_stats_rec* tiles, uint32_t world, size_t stride, uint32_t r) {
    sphx_stats_rec acc = tiles[r];
    for (uint32_t t = 1; t < world; ++t) acc = merge(acc, tiles[(size_t)t * stride + r]);
    return acc;
}

// Transport: a record is sixteen 64-bit words.  A transport that moves a double by adding it to zeros (Comm::allgather8) turns -0 into +0
// and need not preserve an arbitrary bit pattern (a NaN payload), so each word travels as two integers below 2^32, low half first: such
// values and their sums with zeros are exact in float64.
constexpr int WORDS = (int)(sizeof(sphx_stats_rec) / 8);  // 16
constexpr int HALVES = 2 * WORDS;                          // 32 doubles per record
inline void encode_word(uint64_t w, double out[2]) {
    out[0] = (double)(uint32_t)(w & 0xFFFFFFFFull);
    out[1] = (double)(uint32_t)(w >> 32);
}
inline uint64_t decode_word(const double in[2]) { return (uint64_t)(uint32_t)in[0] | ((uint64_t)(uint32_t)in[1] << 32); }
inline void encode(const sphx_stats_rec& r, double out[HALVES]) {
    uint64_t w[WORDS];
    std::memcpy(w, &r, sizeof(r));
    for (int k = 0; k < WORDS; ++k) encode_word(w[k], out + 2 * k);
}
inline sphx_stats_rec decode(const double in[HALVES]) {
    uint64_t w[WORDS];
    for (int k = 0; k < WORDS; ++k) w[k] = decode_word(in + 2 * k);
    sphx_stats_rec r;
    std::memcpy(&r, w, sizeof(r));
    return r;
}
static_assert(sizeof(sphx_stats_rec) == 128, "the layout of sphx.h");

}  // namespace sphx_stats_host
