// sphx_gauge_merge.hpp — the fold of the tiles' gauge partials (sphx_multi_gauge_levels, sphx_multi_probe_read, sphx_gauge_merge;
// include/sphx.h, "gauges and probes of a tiled run").  Plain C++ without a GPU call, compiled into the kernels' translation unit, into
// sphx_tiles.cpp and into tests/gauge_merge_driver.cpp.
//
// A tile reduces the samples of a gauge it owns — ONE contiguous interval [lo, lo + count), fact 1 of sphx_gauge_window.hpp — to a
// 32-byte sphx_gauge_part on its device; the values never cross to the host.  The fold checks that the parts with count > 0, ordered by
// lo, tile [0, n) exactly, and then forms the record:
//   first = the minimum, last = the maximum, inside = the sum over the parts that have something inside;
//   f_last = the f_last of the part that holds `last`;
//   f_next = that part's f_next where it owns last + 1, otherwise the f_lo of the part whose lo == last + 1 — fact 2 of
//            sphx_gauge_window.hpp: the intervals are contiguous and disjoint, so the owner of last + 1 begins there.
// sphx_gauge_host::record() of sphx_gauge_rule.hpp makes the record, here as in sphx_gauge_reduce and in k_gauge_reduce: the result is
// bit for bit sphx_gauge_reduce over the concatenated values.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

#include "sphx_gauge_rule.hpp"
#include "sphx_gauge_window.hpp"

namespace sphx_gauge_host {

static_assert(sizeof(sphx_gauge_part) == 32, "a partial is 32 bytes");

SPHX_GAUGE_FN float qnan_value() {
    const uint32_t u = QNAN_WORD;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// The partial of the interval iv of a gauge whose n values are f[0 .. n): what a tile's reduce pass stores (tests and the driver; the
// device forms the same members from ballots).
inline sphx_gauge_part make_part(const float* f, Interval iv, float iso) {
    sphx_gauge_part p;
    p.lo = iv.lo, p.count = iv.count;
    p.first = p.last = SPHX_GAUGE_NONE, p.inside = 0u;
    p.f_lo = p.f_last = p.f_next = qnan_value();
    for (uint32_t k = iv.lo; k < iv.lo + iv.count; ++k)
        if (f[k] >= iso) {
            if (!p.inside) p.first = k;
            p.last = k;
            p.inside += 1u;
        }
    if (iv.count) p.f_lo = f[iv.lo];
    if (p.inside) {
        p.f_last = f[p.last];
        if (p.last + 1u < iv.lo + iv.count) p.f_next = f[p.last + 1u];
    }
    return p;
}

// The record of gauge g from its parts parts[0], parts[stride], ... (n_parts of them; parts with count == 0 own nothing).  nullptr: *out is
// the record; otherwise the message of the refusal and *out is untouched.
inline const char* fold(const sphx_gauge& g, float iso, const sphx_gauge_part* parts, uint32_t n_parts, size_t stride, Words* out) {
    std::vector<uint32_t> order;
    order.reserve(n_parts);
    for (uint32_t p = 0; p < n_parts; ++p) {
        const sphx_gauge_part& q = parts[(size_t)p * stride];
        if (q.count == 0u) {
            if (q.inside != 0u) return "a part that owns no sample reports samples inside";
            continue;
        }
        if ((uint64_t)q.lo + q.count > g.n) return "a part reaches behind the gauge's last sample";
        if (q.inside > q.count) return "a part reports more samples inside than it owns";
        if (q.inside && (q.first < q.lo || q.last >= q.lo + q.count || q.first > q.last || q.last - q.first + 1u < q.inside))
            return "a part's first / last lie outside its own interval";
        order.push_back(p);
    }
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        const sphx_gauge_part &x = parts[(size_t)a * stride], &y = parts[(size_t)b * stride];
        return x.lo != y.lo ? x.lo < y.lo : a < b;
    });
    uint64_t at = 0;
    for (uint32_t p : order) {
        const sphx_gauge_part& q = parts[(size_t)p * stride];
        if (q.lo > at) return "the parts leave a gap (a sample nobody owns, or a count below the interval)";
        if (q.lo < at) return "the parts overlap (a sample owned twice, or a count above the interval)";
        at += q.count;
    }
    if (at != g.n) return "the parts leave a gap at the end of the gauge";
    uint32_t first = SPHX_GAUGE_NONE, last = SPHX_GAUGE_NONE, inside = 0u;
    const sphx_gauge_part* holder = nullptr;
    for (uint32_t p : order) {  // (ascending lo: the first part with something inside holds the minimum, the last one the maximum)
        const sphx_gauge_part& q = parts[(size_t)p * stride];
        if (!q.inside) continue;
        if (!inside) first = q.first;
        last = q.last;
        inside += q.inside;
        holder = &q;
    }
    float f_last = 0.0f, f_next = 0.0f;
    if (holder) {
        f_last = holder->f_last;
        if (last + 1u < g.n) {
            if (last + 1u < holder->lo + holder->count) {
                f_next = holder->f_next;
            } else {
                for (uint32_t p : order)
                    if (parts[(size_t)p * stride].lo == last + 1u) f_next = parts[(size_t)p * stride].f_lo;  // (exists: the parts tile [0, n))
            }
        }
    }
    *out = record(g, iso, first, last, inside, f_last, f_next);
    return nullptr;
}

// sphx_gauge_merge: parts[p * n_gauges + k] is part p of gauge k.  nullptr, or the message of the first refusal (no record is written
// for any gauge then).
inline const char* merge(const sphx_gauge* gauges, uint32_t n_gauges, float iso, const sphx_gauge_part* parts, uint32_t n_parts, sphx_gauge_rec* out) {
    std::vector<Words> rec(n_gauges);
    for (uint32_t k = 0; k < n_gauges; ++k)
        if (const char* bad = fold(gauges[k], iso, parts + k, n_parts, n_gauges, &rec[k])) return bad;
    if (n_gauges) memcpy(out, rec.data(), (size_t)n_gauges * sizeof(Words));
    return nullptr;
}

// The point probes of a frame: entry i is the record of the first part (lowest tile first) whose "answered" mark — reserved[0] — is set,
// with the mark stripped; nobody answered: zeros and tile -1.  tile_of[p]: the tile number of part p.
inline void fold_points(uint32_t m, const sphx_probe_rec* const* parts, const int32_t* tile_of, uint32_t n_parts, sphx_probe_rec* out, int32_t* out_tile) {
    for (uint32_t i = 0; i < m; ++i) {
        sphx_probe_rec r;
        memset(&r, 0, sizeof(r));
        int32_t t = -1;
        for (uint32_t p = 0; p < n_parts; ++p)
            if (parts[p][i].reserved[0] != 0u && (t < 0 || tile_of[p] < t)) {
                r = parts[p][i];
                t = tile_of[p];
            }
        r.reserved[0] = 0u;
        if (out) out[i] = r;
        if (out_tile) out_tile[i] = t;
    }
}

}  // namespace sphx_gauge_host
