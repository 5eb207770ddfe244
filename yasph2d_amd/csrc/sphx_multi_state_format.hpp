// sphx_multi_state_format.hpp — layout and validation of one PART of a tiled run's checkpoint (sphx_multi_state_save / _load,
// include/sphx.h) and of the file around a set of parts (sphx_solver_multi_checkpoint).  Pure host C++: no HIP include, so that
// sphx_tiles.cpp and a stand-alone program (tests/multi_state_format_driver.cpp) compile the same text.
//
// A checkpoint is n_parts parts; a part holds the particles some tiles OWN, in those tiles' device order, tile after tile in ascending
// rank.  An in-process sphx_multi writes part 0 of 1; in rank mode rank r writes part r of W.  What a part says does not depend on the
// tiling beyond the order of its particles and the saver's layout, which is kept as a hint only.
//
// One part, little-endian, every offset in bytes from its first byte:
//     0  char[8]  magic "SPHXMULT"
//     8  u32      format version (1)
//    12  u32      endianness tag 0x01020304
//    16  u64      total size of the part
//    24  u32      size of everything in front of the sections (HEADER_BYTES = 1176)
//    28  u32      number of sections (8)
//    32  u32      sizeof(sphx_params) (80)
//    36  u32      0
//    40  sphx_params the multi was created with; `device` is stored as 0
//   120  u64      N_total: owned particles of the whole run
//   128  u32 N_part (particles in this part), u32 B (boundary particles, the GLOBAL boundary)
//   136  u32 part, u32 n_parts
//   144  u32 num_density_iters, u32 num_divergence_iters      (dfsph.rs:199 / :354: do the warm starts fire)
//   152  u32 last_div_iters, u32 last_div_warm                (the tile loop's ring budget of the step that follows)
//   160  u64      steps finished since the upload
//   168  u32 tiling_invariant (0 or 1), u32 world (tiles of the saver, 1 .. 64)
//   176  i32 axis (0 / 1: strips along it; -1: grid), u32 nx, u32 ny (grid: nx * ny = world; strips: both 1), u32 n_cuts
//   192  u32 cuts[196]: strips: the world + 1 cuts; grid: the nx + 1 column cuts, then ny + 1 cuts for each column; unused entries 0
//   976  section table: 8 x {u64 offset, u64 bytes, u64 digest}
//  1168  u64      digest (the section digest of sphx.h) of the 292 words in front of it
//  1176  the sections, each at the next multiple of 8 behind its predecessor; padding bytes are zero
// Sections: positions 8 N_part, velocities 8 N_part, particle_id 4 N_part (bit 31 clear), density, alpha, kappa, stiffness 4 N_part each,
// boundary 8 B (caller order; the same in every part).  The first seven carry the ID-KEYED digest of sphx.h — the word c of the particle
// with id `id` has the index id * k + c, k the words per particle — so the digests of the parts of a checkpoint ADD UP (mod 2^64) to
// those of the whole run, however it is tiled; the boundary carries the positional digest.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "sphx_state_format.hpp"

namespace sphx_multi_state {

constexpr char MAGIC[8] = {'S', 'P', 'H', 'X', 'M', 'U', 'L', 'T'};
constexpr uint32_t VERSION = 1;
constexpr uint32_t ENDIAN_TAG = sphx_state::ENDIAN_TAG;
constexpr uint32_t NSEC = 8, NPARTICLE_SEC = 7, SEC_BOUNDARY = 7;
constexpr uint32_t MAX_TILES = 64, MAX_CUTS = 196;  // grid: nx + 1 + nx (ny + 1) = world + 2 nx + 1 <= 193
constexpr uint64_t MAX_PART = 1ull << 28, MAX_TOTAL = 1ull << 31;  // (ids carry the owner mark in bit 31)
constexpr uint64_t DIGEST_MUL = sphx_state::DIGEST_MUL, DIGEST_LEN = sphx_state::DIGEST_LEN;

using sphx_state::Section;
struct Scalars {
    uint64_t n_total;
    uint32_t n_part, b;
    uint32_t part, n_parts;
    uint32_t num_density_iters, num_divergence_iters;
    uint32_t last_div_iters, last_div_warm;
    uint64_t steps;
    uint32_t tiling_invariant, world;
    int32_t axis;
    uint32_t nx, ny, n_cuts;
    uint32_t cuts[MAX_CUTS];
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
constexpr uint32_t HEADER_BYTES = 1176, HEADER_DIGEST_AT = 1168;
static_assert(sizeof(Scalars) == 856 && sizeof(Header) == HEADER_BYTES, "the part header has no implicit padding");

inline const char* section_name(uint32_t k) {
    static const char* const names[NSEC] = {"positions", "velocities", "particle_id", "density", "alpha", "kappa", "stiffness", "boundary"};
    return k < NSEC ? names[k] : "?";
}
// 32-bit words per particle of section k (0 for the boundary)
inline uint32_t section_words(uint32_t k) { return k < 2 ? 2u : (k < NPARTICLE_SEC ? 1u : 0u); }

// The id-keyed digest of sphx.h over n particles with k words each (host form; the device pass of sphx_multi_state.inc computes the
// same number): sum over the particles of (u64) w[c] * ((2 (id k + c) + 1) * DIGEST_MUL), plus (n k) * DIGEST_LEN.
inline uint64_t digest_by_id(const void* words, const uint32_t* ids, uint64_t n, uint32_t k) {
    const unsigned char* p = (const unsigned char*)words;
    uint64_t sum = 0;
    for (uint64_t i = 0; i < n; ++i)
        for (uint32_t c = 0; c < k; ++c) {
            uint32_t w;
            std::memcpy(&w, p + 4 * (i * k + c), 4);
            sum += (uint64_t)w * ((2ull * ((uint64_t)ids[i] * k + c) + 1ull) * DIGEST_MUL);
        }
    return sum + n * k * DIGEST_LEN;
}

inline uint64_t section_bytes(const Scalars& s, uint32_t k) {
    return k < NPARTICLE_SEC ? 4ull * section_words(k) * s.n_part : (k == SEC_BOUNDARY ? 8ull * s.b : 0ull);
}
inline uint64_t header_digest_of(const Header& h) { return sphx_state::digest_words(&h, HEADER_DIGEST_AT / 4u); }

// fills the fixed fields, the section offsets and byte counts and the total from h.s (digests are the writer's, who then seal()s)
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

// the saver's layout: is it one sphx_multi could have had?  (cut lists start at 0, end at 65536 and increase strictly)
inline const char* layout_problem(const Scalars& s) {
    if (s.world < 1 || s.world > MAX_TILES) return "the saver's tile count is not in 1 .. 64";
    auto list_ok = [&](uint32_t from, uint32_t cnt) {
        if (s.cuts[from] != 0 || s.cuts[from + cnt - 1] != 65536u) return false;
        for (uint32_t i = 1; i < cnt; ++i)
            if (s.cuts[from + i] <= s.cuts[from + i - 1]) return false;
        return true;
    };
    if (s.axis == 0 || s.axis == 1) {
        if (s.nx != 1 || s.ny != 1) return "a strip layout with nx or ny other than 1";
        if (s.n_cuts != s.world + 1) return "a strip layout needs world + 1 cuts";
        if (!list_ok(0, s.n_cuts)) return "the cuts do not run from 0 to 65536 strictly increasing";
    } else if (s.axis == -1) {
        if (s.nx < 1 || s.ny < 1 || s.nx > MAX_TILES || s.ny > MAX_TILES || s.nx * s.ny != s.world) return "a grid layout whose nx * ny is not the tile count";
        if (s.n_cuts != s.nx + 1 + s.nx * (s.ny + 1)) return "a grid layout needs nx + 1 + nx (ny + 1) cuts";
        if (!list_ok(0, s.nx + 1)) return "the column cuts do not run from 0 to 65536 strictly increasing";
        for (uint32_t ix = 0; ix < s.nx; ++ix)
            if (!list_ok(s.nx + 1 + ix * (s.ny + 1), s.ny + 1)) return "a column's cuts do not run from 0 to 65536 strictly increasing";
    } else {
        return "axis is none of 0, 1, -1";
    }
    for (uint32_t i = s.n_cuts; i < MAX_CUTS; ++i)
        if (s.cuts[i]) return "an unused cut entry is not zero";
    return nullptr;
}

// Everything about ONE part that can be checked without a multi: `avail` bytes at `buf` (the header is copied out: buf needs no
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
    if (std::memcmp(h.magic, MAGIC, 8) != 0)
        return bad(std::memcmp(h.magic, sphx_state::MAGIC, 8) == 0 ? "bad magic: a single-context state blob (sphx_state_load reads it), not a part of a tiled checkpoint"
                                                                   : "bad magic: not a part of a tiled checkpoint");
    if (h.endian_tag != ENDIAN_TAG) return bad("endianness tag mismatch: written on a machine of the other byte order, or damaged");
    if (h.version != VERSION) return bad("format version " + std::to_string(h.version) + " is not supported (this library reads version " + std::to_string(VERSION) + ")");
    if (h.header_bytes != HEADER_BYTES) return bad("header size field is wrong");
    if (h.n_sections != NSEC) return bad("section count field is wrong");
    if (h.params_bytes != sizeof(sphx_params)) return bad("sizeof(sphx_params) field is wrong");
    if (h.zero != 0) return bad("reserved header word is not zero");
    if (h.params.device != 0) return bad("params.device is not stored as 0");
    if (h.header_digest != header_digest_of(h)) return bad("the header's digest does not match its fields: damaged");
    if (h.total_bytes != avail) return bad(h.total_bytes > avail ? "truncated: the part says it is longer than the buffer" : "the buffer is longer than the part says it is");
    const Scalars& s = h.s;
    if (s.n_total > MAX_TOTAL) return bad("N_total is beyond 2^31 (ids carry the owner mark in bit 31)");
    if (s.n_part >= MAX_PART || s.b >= MAX_PART) return bad("N_part or B is beyond the 2^28 slots of a context");
    if (s.n_part > s.n_total) return bad("N_part is larger than N_total");
    if (s.n_parts < 1 || s.n_parts > MAX_TILES) return bad("n_parts is not in 1 .. 64");
    if (s.part >= s.n_parts) return bad("the part index is not below n_parts");
    if (s.n_parts == 1 && s.n_part != s.n_total) return bad("the only part does not hold N_total particles");
    if (s.tiling_invariant > 1 || s.last_div_warm > 1) return bad("a flag scalar is neither 0 nor 1");
    const uint64_t cap_den = (uint64_t)(h.params.max_density_iterations > h.params.fixed_density_iterations ? h.params.max_density_iterations : h.params.fixed_density_iterations) + 1;
    const uint64_t cap_div = (uint64_t)(h.params.max_divergence_iterations > h.params.fixed_divergence_iterations ? h.params.max_divergence_iterations : h.params.fixed_divergence_iterations) + 1;
    if (s.num_density_iters > cap_den || s.num_divergence_iters > cap_div || s.last_div_iters > cap_div) return bad("an iteration count is beyond the iteration cap of the params");
    if (const char* lp = layout_problem(s)) return bad(std::string("the saver's layout: ") + lp);
    if (s.n_parts != 1 && s.n_parts != s.world) return bad("n_parts is neither 1 nor the saver's tile count");
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

// A SET of validated headers: one checkpoint?  Every index once; scalars, params, flag, the saver's layout and the boundary digest equal
// across the parts; the parts' particles add up to N_total.
inline bool validate_set(const Header* h, uint32_t n, std::string* err) {
    auto bad = [&](const std::string& what) {
        if (err) *err = what;
        return false;
    };
    if (!h || n == 0) return bad("no parts");
    if (n > MAX_TILES) return bad("more than 64 parts");
    if (h[0].s.n_parts != n) return bad(n < h[0].s.n_parts ? "a part is missing: the checkpoint has " + std::to_string(h[0].s.n_parts) + " parts, " + std::to_string(n) + " were given"
                                                           : "more parts were given than the checkpoint has");
    uint64_t seen = 0, total = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const Scalars &a = h[0].s, &b = h[i].s;
        if (b.n_parts != n) return bad("the parts disagree about n_parts");
        if (seen >> b.part & 1u) return bad("part " + std::to_string(b.part) + " appears twice (another one is missing)");
        seen |= 1ull << b.part;
        total += b.n_part;
        if (std::memcmp(&h[i].params, &h[0].params, sizeof(sphx_params)) != 0) return bad("the parts were saved under different params");
        if (b.n_total != a.n_total || b.b != a.b) return bad("the parts disagree about N_total or B");
        if (b.num_density_iters != a.num_density_iters || b.num_divergence_iters != a.num_divergence_iters || b.last_div_iters != a.last_div_iters ||
            b.last_div_warm != a.last_div_warm)
            return bad("the parts disagree about the iteration counts");
        if (b.steps != a.steps) return bad("the parts were saved at different steps");
        if (b.tiling_invariant != a.tiling_invariant) return bad("the parts disagree about tiling-invariant mode");
        if (b.world != a.world || b.axis != a.axis || b.nx != a.nx || b.ny != a.ny || b.n_cuts != a.n_cuts || std::memcmp(b.cuts, a.cuts, sizeof(a.cuts)) != 0)
            return bad("the parts disagree about the saver's layout");
        if (h[i].sec[SEC_BOUNDARY].digest != h[0].sec[SEC_BOUNDARY].digest) return bad("the parts hold different boundaries");
    }
    if (total != h[0].s.n_total) return bad("the parts' particle counts do not add up to N_total");
    return true;
}

// are the padding bytes between the sections zero?  (needs the whole part in host memory)
inline bool padding_is_zero(const void* buf, const Header& h) {
    const unsigned char* p = (const unsigned char*)buf;
    for (uint32_t k = 0; k < NSEC; ++k) {
        const uint64_t end = h.sec[k].offset + h.sec[k].bytes, next = k + 1 < NSEC ? h.sec[k + 1].offset : h.total_bytes;
        for (uint64_t i = end; i < next; ++i)
            if (p[i]) return false;
    }
    return true;
}

// ---- the checkpoint file of the solver object: {CheckpointFileHeader, the parts one after the other} -------------------------------------
constexpr char CHECKPOINT_MAGIC[8] = {'S', 'P', 'H', 'X', 'M', 'C', 'K', 'P'};
struct CheckpointFileHeader {
    char magic[8];
    uint32_t version, endian_tag;
    uint64_t parts_bytes;  // everything behind this header
    sphx_timer_state timer;
};
static_assert(sizeof(CheckpointFileHeader) == 80, "the checkpoint file header has no implicit padding");

inline bool validate_checkpoint_file(const void* buf, uint64_t avail, CheckpointFileHeader* out, std::string* err) {
    auto bad = [&](const char* what) {
        if (err) *err = what;
        return false;
    };
    if (!buf || avail < sizeof(CheckpointFileHeader)) return bad("truncated: shorter than the checkpoint file header");
    CheckpointFileHeader h;
    std::memcpy(&h, buf, sizeof(h));
    if (std::memcmp(h.magic, CHECKPOINT_MAGIC, 8) != 0) return bad("bad magic: not a tiled solver checkpoint");
    if (h.endian_tag != ENDIAN_TAG) return bad("endianness tag mismatch");
    if (h.version != VERSION) return bad("unsupported checkpoint file version");
    if (h.parts_bytes != avail - sizeof(CheckpointFileHeader)) return bad("truncated: the file's length disagrees with the size it states");
    if (!sphx_state::timer_state_valid(h.timer)) return bad("the timer state is not one a TimeManager can hold");
    if (out) *out = h;
    return true;
}

// Splits `avail` bytes that hold parts back to back (each part states its own length) into {offset, bytes}; false if they do not tile it.
inline bool split_parts(const void* buf, uint64_t avail, std::vector<std::pair<uint64_t, uint64_t>>* out, std::string* err) {
    const unsigned char* p = (const unsigned char*)buf;
    uint64_t at = 0;
    out->clear();
    while (at < avail) {
        if (avail - at < HEADER_BYTES || out->size() >= MAX_TILES) {
            if (err) *err = "truncated: what follows the last whole part is not a part";
            return false;
        }
        uint64_t total;
        std::memcpy(&total, p + at + 16, 8);
        if (total < HEADER_BYTES || total > avail - at) {
            if (err) *err = "truncated: a part says it is longer than what is left of the file";
            return false;
        }
        out->push_back({at, total});
        at += total;
    }
    return true;
}

}  // namespace sphx_multi_state
