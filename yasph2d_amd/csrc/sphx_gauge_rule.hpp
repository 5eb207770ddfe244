// sphx_gauge_rule.hpp — the gauge rule of include/sphx.h ("gauges and probes"): from the inside test over a ray's values to one
// sphx_gauge_rec.  One function forms the record on the host (sphx_gauge_reduce) and on the device (k_gauge_reduce, sphx_gauge.inc), so
// the two agree by construction; tests/gauge_rule_driver.cpp compiles this file alone and holds it to the numpy restatement
// (tests/gauge_reference.py).  Every fp32 operation is rounded once: compile with -ffp-contract=off and without value-changing options.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/sphx.h"

#if defined(__HIPCC__)
#define SPHX_GAUGE_FN __host__ __device__ inline
#else
#define SPHX_GAUGE_FN inline
#endif

namespace sphx_gauge_host {

constexpr uint32_t QNAN_WORD = 0x7FC00000u;     // what the members that have no value hold
constexpr uint32_t MAX_SAMPLES = 1u << 20;      // per gauge
constexpr uint64_t MAX_TOTAL = 1ull << 24;      // per call

struct Words {
    uint32_t w[8];  // the members of sphx_gauge_rec in order
};
static_assert(sizeof(sphx_gauge_rec) == 32 && sizeof(Words) == 32 && sizeof(sphx_gauge) == 32 && sizeof(sphx_probe_rec) == 32 &&
                  sizeof(sphx_probe_status) == 32,
              "the records of include/sphx.h are 32 bytes");

SPHX_GAUGE_FN uint32_t word_of(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

// The record of a gauge g whose inside test gave first / last / inside (inside == 0: none).  f_last = the value at `last`, f_next = the
// value at last + 1; either is read only where the rule uses it.
// (f_next - f_last is never zero where it divides: b_last != b_(last+1), and equal values compare alike with iso.)
SPHX_GAUGE_FN Words record(const sphx_gauge& g, float iso, uint32_t first, uint32_t last, uint32_t inside, float f_last, float f_next) {
    Words r;
    if (inside == 0u) {
        r.w[0] = r.w[1] = SPHX_GAUGE_NONE;
        r.w[2] = 0u;
        r.w[3] = r.w[4] = r.w[5] = r.w[6] = r.w[7] = QNAN_WORD;
        return r;
    }
    r.w[0] = first, r.w[1] = last, r.w[2] = inside;
    const float xa = g.x0 + (float)last * g.dx, ya = g.y0 + (float)last * g.dy;
    r.w[6] = word_of(f_last);
    if (last == g.n - 1u) {  // the ray ends wet
        r.w[3] = word_of(0.0f);
        r.w[4] = word_of(xa), r.w[5] = word_of(ya);
        r.w[7] = QNAN_WORD;
        return r;
    }
    const float xb = g.x0 + (float)(last + 1u) * g.dx, yb = g.y0 + (float)(last + 1u) * g.dy;
    const float t = (iso - f_last) / (f_next - f_last);
    r.w[3] = word_of(t);
    r.w[4] = word_of(xa + t * (xb - xa)), r.w[5] = word_of(ya + t * (yb - ya));
    r.w[7] = word_of(f_next);
    return r;
}

// NULL gauges with n_gauges > 0, too many gauges or samples, a non-finite number -> the message; nullptr: fine.  *total = the sum of n.
inline const char* check(const sphx_gauge* gauges, uint32_t n_gauges, float iso, uint64_t* total) {
    *total = 0;
    if (n_gauges > SPHX_GAUGE_MAX) return "n_gauges exceeds SPHX_GAUGE_MAX";
    if (n_gauges && !gauges) return "gauges is NULL with n_gauges > 0";
    if (!std::isfinite(iso)) return "iso must be finite";
    uint64_t sum = 0;
    for (uint32_t k = 0; k < n_gauges; ++k) {
        const sphx_gauge& g = gauges[k];
        if (g.n == 0u || g.n > MAX_SAMPLES) return "gauges holds a gauge with n == 0 or n > 2^20";
        if (!std::isfinite(g.x0) || !std::isfinite(g.y0) || !std::isfinite(g.dx) || !std::isfinite(g.dy))
            return "gauges holds a non-finite x0, y0, dx or dy";
        sum += g.n;
    }
    if (sum > MAX_TOTAL) return "gauges holds more than 2^24 samples in all";
    *total = sum;
    return nullptr;
}

// the rule over the values of one gauge
inline Words reduce_one(const sphx_gauge& g, const float* f, float iso) {
    uint32_t first = SPHX_GAUGE_NONE, last = SPHX_GAUGE_NONE, inside = 0;
    for (uint32_t k = 0; k < g.n; ++k) {
        if (f[k] >= iso) {  // (NaN: outside)
            if (!inside) first = k;
            last = k;
            inside += 1u;
        }
    }
    const float f_last = inside ? f[last] : 0.0f;
    const float f_next = inside && last + 1u < g.n ? f[last + 1u] : 0.0f;
    return record(g, iso, first, last, inside, f_last, f_next);
}

// sphx_gauge_reduce
inline int reduce(const float* values, const sphx_gauge* gauges, uint32_t n_gauges, float iso, sphx_gauge_rec* out) {
    if (!out) return SPHX_ERR_INVALID_ARGUMENT;
    uint64_t total;
    if (check(gauges, n_gauges, iso, &total)) return SPHX_ERR_INVALID_ARGUMENT;
    if (total && !values) return SPHX_ERR_INVALID_ARGUMENT;
    size_t at = 0;
    for (uint32_t k = 0; k < n_gauges; ++k) {
        const Words r = reduce_one(gauges[k], values + at, iso);
        memcpy(&out[k], &r, sizeof(r));
        at += gauges[k].n;
    }
    return SPHX_OK;
}

}  // namespace sphx_gauge_host
