// sphx_state_format.hpp — layout and validation of the state blob (sphx_state_save / sphx_state_load, include/sphx.h) and of the solver
// file around it (sphx_solver_save / sphx_solver_load).  Pure host C++: no HIP include, so that the library's two translation units that
// write and read blobs and a stand-alone program (tests/state_format_driver.cpp) compile the same text.
//
// The blob, little-endian, every offset in bytes from its first byte:
//     0  char[8]  magic "SPHXSTAT"
//     8  u32      format version (1)
//    12  u32      endianness tag 0x01020304 (a reader on the wrong byte order sees 0x04030201)
//    16  u64      total size of the blob
//    24  u32      size of everything in front of the sections (HEADER_BYTES = 392)
//    28  u32      number of sections (SPHX_STATE_SECTIONS = 9)
//    32  u32      sizeof(sphx_params) (80)
//    36  u32      0
//    40  sphx_params the context was created with; `device` is stored as 0 (the blob does not say where it was made)
//   120  u32 N, u32 B, u32 cached_n, u32 wcsph_n
//   136  u64 ids_issued
//   144  u32 num_density_iters, u32 num_divergence_iters
//   152  u32 set_changed, u32 tiling_invariant, u32 lists_current, u32 sampling_allowed      (each 0 or 1)
//   168  section table: 9 x {u64 offset, u64 bytes, u64 digest}, in the order of the SPHX_STATE_SEC_* codes
//   384  u64      digest (the section digest of sphx.h) of the 96 words in front of it: no field of the header can change unnoticed
//   392  the sections in that order, each at the next multiple of 8 behind its predecessor; padding bytes are zero
// Sections (W = min(N, cached_n)): positions 8N, velocities 8N, particle_id 4N, density 4N, alpha 4W, kappa 4W, stiffness 4W,
// accel 8 wcsph_n, boundary (caller order) 8B.  The layout is a function of the five counts: a valid blob has exactly one form.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/sphx.h"

namespace sphx_state {

constexpr char MAGIC[8] = {'S', 'P', 'H', 'X', 'S', 'T', 'A', 'T'};
constexpr uint32_t VERSION = 1;
constexpr uint32_t ENDIAN_TAG = 0x01020304u;
constexpr uint32_t NSEC = SPHX_STATE_SECTIONS;
constexpr uint64_t MAX_SLOTS = 1ull << 28;  // fluid + boundary slots of one context (the kernels' 32-bit byte offsets)

struct Section {
    uint64_t offset, bytes, digest;
};
struct Scalars {
    uint32_t n, b, cached_n, wcsph_n;
    uint64_t ids_issued;
    uint32_t num_density_iters, num_divergence_iters;
    uint32_t set_changed, tiling_invariant, lists_current, sampling_allowed;
};
struct Header {
    char magic[8];
    uint32_t version, endian_tag;
    uint64_t total_bytes;
    uint32_t header_bytes, n_sections, params_bytes, zero;
    sphx_params params;
    Scalars s;
    Section sec[NSEC];
    uint64_t header_digest;
};
constexpr uint32_t HEADER_BYTES = 392, HEADER_DIGEST_AT = 384;
static_assert(sizeof(sphx_params) == 80, "sphx_params is part of the blob format");
static_assert(sizeof(Scalars) == 48 && sizeof(Section) == 24 && sizeof(Header) == HEADER_BYTES, "the blob header has no implicit padding");

inline const char* section_name(uint32_t k) {
    static const char* const names[NSEC] = {"positions", "velocities", "particle_id", "density", "alpha", "kappa", "stiffness", "accel", "boundary"};
    return k < NSEC ? names[k] : "?";
}

// The digest of sphx.h over W 32-bit words (host form; the device kernel of sphx_state.inc computes the same number).
constexpr uint64_t DIGEST_MUL = 0x9E3779B97F4A7C15ull, DIGEST_LEN = 0xD6E8FEB86659FD93ull;
inline uint64_t digest_words(const void* words, uint64_t W) {
    const unsigned char* p = (const unsigned char*)words;
    uint64_t sum = 0, k = DIGEST_MUL;  // k = (2 i + 1) * DIGEST_MUL
    for (uint64_t i = 0; i < W; ++i, k += 2 * DIGEST_MUL) {
        uint32_t w;
        std::memcpy(&w, p + 4 * i, 4);
        sum += (uint64_t)w * k;
    }
    return sum + W * DIGEST_LEN;
}

// bytes of section k under these counts (counts are 32-bit: no product overflows 64 bits)
inline uint64_t section_bytes(const Scalars& s, uint32_t k) {
    const uint64_t n = s.n, w = s.n < s.cached_n ? s.n : s.cached_n;
    switch (k) {
        case SPHX_STATE_SEC_POSITIONS:
        case SPHX_STATE_SEC_VELOCITIES: return 8 * n;
        case SPHX_STATE_SEC_PARTICLE_ID:
        case SPHX_STATE_SEC_DENSITY: return 4 * n;
        case SPHX_STATE_SEC_ALPHA:
        case SPHX_STATE_SEC_KAPPA:
        case SPHX_STATE_SEC_STIFFNESS: return 4 * w;
        case SPHX_STATE_SEC_ACCEL: return 8 * (uint64_t)s.wcsph_n;
        case SPHX_STATE_SEC_BOUNDARY: return 8 * (uint64_t)s.b;
        default: return 0;
    }
}

inline uint64_t header_digest_of(const Header& h) { return digest_words(&h, HEADER_DIGEST_AT / 4u); }

// fills the fixed fields, the section offsets and byte counts and the total from h.params / h.s (digests are left alone: the writer
// sets the sections' and then seal()s the header)
inline void layout(Header& h) {
    std::memcpy(h.magic, MAGIC, 8);
    h.version = VERSION;
    h.endian_tag = ENDIAN_TAG;
    h.header_bytes = HEADER_BYTES;
    h.n_sections = NSEC;
    h.params_bytes = (uint32_t)sizeof(sphx_params);
    h.zero = 0;
    uint64_t at = HEADER_BYTES;
    for (uint32_t k = 0; k < NSEC; ++k) {
        h.sec[k].offset = at;
        h.sec[k].bytes = section_bytes(h.s, k);
        at = (at + h.sec[k].bytes + 7u) & ~7ull;
    }
    h.total_bytes = at;
}
inline void seal(Header& h) { h.header_digest = header_digest_of(h); }

// the first physics field in which two parameter sets differ bit for bit (device and list_span_limit are free), or nullptr
inline const char* params_mismatch(const sphx_params& a, const sphx_params& b) {
#define SPHX_STATE_FIELD(f) \
    if (std::memcmp(&a.f, &b.f, sizeof(a.f)) != 0) return #f;
    SPHX_STATE_FIELD(smoothing_length) SPHX_STATE_FIELD(particle_mass) SPHX_STATE_FIELD(fluid_density) SPHX_STATE_FIELD(particle_radius)
    SPHX_STATE_FIELD(gravity) SPHX_STATE_FIELD(grid_min) SPHX_STATE_FIELD(xsph_epsilon) SPHX_STATE_FIELD(max_avg_density_error)
    SPHX_STATE_FIELD(max_density_iterations) SPHX_STATE_FIELD(max_divergence_error) SPHX_STATE_FIELD(max_divergence_iterations)
    SPHX_STATE_FIELD(fixed_density_iterations) SPHX_STATE_FIELD(fixed_divergence_iterations) SPHX_STATE_FIELD(viscosity_model)
    SPHX_STATE_FIELD(fluid_viscosity) SPHX_STATE_FIELD(reserved)
#undef SPHX_STATE_FIELD
    return nullptr;
}

// Everything about a blob that can be checked without a context: `avail` bytes at `buf` (the header is copied out, so buf needs no
// alignment).  Reads at most HEADER_BYTES bytes.  On success *out holds the header; on failure *err says what is wrong.
inline bool validate(const void* buf, uint64_t avail, Header* out, std::string* err) {
    auto bad = [&](const std::string& what) {
        if (err) *err = what;
        return false;
    };
    if (!buf) return bad("the buffer is NULL");
    if (avail < HEADER_BYTES) return bad("truncated: shorter than the header");
    Header h;
    std::memcpy(&h, buf, HEADER_BYTES);
    if (std::memcmp(h.magic, MAGIC, 8) != 0) return bad("bad magic: not a state blob");
    if (h.endian_tag != ENDIAN_TAG) return bad("endianness tag mismatch: written on a machine of the other byte order, or damaged");
    if (h.version != VERSION) return bad("format version " + std::to_string(h.version) + " is not supported (this library reads version " + std::to_string(VERSION) + ")");
    if (h.header_bytes != HEADER_BYTES) return bad("header size field is wrong");
    if (h.n_sections != NSEC) return bad("section count field is wrong");
    if (h.params_bytes != sizeof(sphx_params)) return bad("sizeof(sphx_params) field is wrong");
    if (h.zero != 0) return bad("reserved header word is not zero");
    if (h.params.device != 0) return bad("params.device is not stored as 0");
    if (h.header_digest != header_digest_of(h)) return bad("the header's digest does not match its fields: damaged");
    if (h.total_bytes != avail) return bad(h.total_bytes > avail ? "truncated: the blob says it is longer than the buffer" : "the buffer is longer than the blob says it is");
    // the scalars, every count against every other
    const Scalars& s = h.s;
    if ((uint64_t)s.n + s.b >= MAX_SLOTS) return bad("N + B is beyond the 2^28 slots of a context");
    if (s.wcsph_n >= MAX_SLOTS || s.cached_n >= MAX_SLOTS) return bad("cached_n or wcsph_n is beyond the 2^28 slots of a context");
    if (s.ids_issued > (1ull << 32)) return bad("ids_issued is beyond 2^32");
    if (s.ids_issued < s.n) return bad("ids_issued is smaller than N (every particle holds an id of its own)");
    if (s.set_changed > 1 || s.tiling_invariant > 1 || s.lists_current > 1 || s.sampling_allowed > 1) return bad("a flag scalar is neither 0 nor 1");
    if (s.sampling_allowed && !s.lists_current) return bad("sampling allowed without current neighbour lists");
    const uint64_t cap_den = (uint64_t)(h.params.max_density_iterations > h.params.fixed_density_iterations ? h.params.max_density_iterations : h.params.fixed_density_iterations) + 1;
    const uint64_t cap_div = (uint64_t)(h.params.max_divergence_iterations > h.params.fixed_divergence_iterations ? h.params.max_divergence_iterations : h.params.fixed_divergence_iterations) + 1;
    if (s.num_density_iters > cap_den || s.num_divergence_iters > cap_div) return bad("an iteration count is beyond the iteration cap of the params");
    // the section table: generic checks first (they name what a damaged table breaks), then the one canonical layout
    for (uint32_t k = 0; k < NSEC; ++k) {
        const Section& a = h.sec[k];
        const std::string nm = section_name(k);
        if (a.offset + a.bytes < a.offset) return bad("section " + nm + ": offset + size overflows 64 bits");
        if (a.offset < HEADER_BYTES || a.offset + a.bytes > h.total_bytes) return bad("section " + nm + " is out of range");
        if (a.offset % 8) return bad("section " + nm + " is not 8-byte aligned");
        if (a.bytes != section_bytes(s, k)) return bad("section " + nm + ": size disagrees with the counts");
        for (uint32_t j = 0; j < k; ++j) {
            const Section& b = h.sec[j];
            if (a.bytes && b.bytes && a.offset < b.offset + b.bytes && b.offset < a.offset + a.bytes) return bad("sections " + std::string(section_name(j)) + " and " + nm + " overlap");
        }
    }
    Header want = h;
    layout(want);
    for (uint32_t k = 0; k < NSEC; ++k)
        if (h.sec[k].offset != want.sec[k].offset) return bad("section " + std::string(section_name(k)) + " is not where the layout puts it");
    if (h.total_bytes != want.total_bytes) return bad("total size disagrees with the counts");
    if (out) *out = h;
    return true;
}

// are the padding bytes between the sections zero?  (needs the whole blob in host memory)
inline bool padding_is_zero(const void* buf, const Header& h) {
    const unsigned char* p = (const unsigned char*)buf;
    for (uint32_t k = 0; k < NSEC; ++k) {
        const uint64_t end = h.sec[k].offset + h.sec[k].bytes, next = k + 1 < NSEC ? h.sec[k + 1].offset : h.total_bytes;
        for (uint64_t i = end; i < next; ++i)
            if (p[i]) return false;
    }
    return true;
}

// ---- the solver file: {SolverFileHeader, blob} -----------------------------------------------------------------------------------------
constexpr char SOLVER_MAGIC[8] = {'S', 'P', 'H', 'X', 'S', 'O', 'L', 'V'};
struct SolverFileHeader {
    char magic[8];
    uint32_t version, endian_tag;
    uint64_t blob_bytes;
    sphx_timer_state timer;
};
static_assert(sizeof(sphx_timer_state) == 56 && sizeof(SolverFileHeader) == 80, "the solver file header has no implicit padding");

inline bool timer_state_valid(const sphx_timer_state& t) {
    return t.fixed <= 1 && t.reserved == 0 && t.cfl_factor == t.cfl_factor;  // (a NaN factor is the one value no constructor accepts and keeps)
}

inline bool validate_solver_file(const void* buf, uint64_t avail, SolverFileHeader* out, std::string* err) {
    auto bad = [&](const char* what) {
        if (err) *err = what;
        return false;
    };
    if (!buf || avail < sizeof(SolverFileHeader)) return bad("truncated: shorter than the solver file header");
    SolverFileHeader h;
    std::memcpy(&h, buf, sizeof(h));
    if (std::memcmp(h.magic, SOLVER_MAGIC, 8) != 0) return bad("bad magic: not a solver state file");
    if (h.endian_tag != ENDIAN_TAG) return bad("endianness tag mismatch");
    if (h.version != VERSION) return bad("unsupported solver file version");
    if (h.blob_bytes != avail - sizeof(SolverFileHeader)) return bad("truncated: the file's length disagrees with the blob size it states");
    if (!timer_state_valid(h.timer)) return bad("the timer state is not one a TimeManager can hold");
    if (out) *out = h;
    return true;
}

}  // namespace sphx_state
