// state_format_driver — the state blob's layout and validation (yasph2d_amd/csrc/sphx_state_format.hpp) as a stand-alone host program,
// built by tests/test_state_host.py with -fsanitize=address,undefined.  It builds a valid blob header, checks that validate() accepts it,
// and then that it refuses every damaged variant without reading outside the buffer it was given.
//   state_format_driver <check>     prints "ok <cases>" and exits 0, or prints what was wrongly accepted / refused and exits 1
//   state_format_driver digest <hex word>...   prints the digest of the words (for the comparison with tests/state_reference.py)
#include <cinttypes>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "sphx_state_format.hpp"

using namespace sphx_state;

static long cases = 0;
static int failures = 0;

static Header good_header() {
    Header h;
    std::memset(&h, 0, sizeof(h));
    h.params.smoothing_length = 0.02f;
    h.params.max_density_iterations = 200;
    h.params.max_divergence_iterations = 400;
    h.s.n = 1001;  // (odd: the 4-byte sections are followed by padding)
    h.s.b = 33;
    h.s.cached_n = 900;
    h.s.wcsph_n = 7;
    h.s.ids_issued = 1200;
    h.s.num_density_iters = 3;
    h.s.num_divergence_iters = 2;
    h.s.lists_current = 1;
    h.s.sampling_allowed = 1;
    layout(h);
    for (uint32_t k = 0; k < NSEC; ++k) h.sec[k].digest = 0x1111111111111111ull * (k + 1);
    seal(h);
    return h;
}

// the header in a heap buffer of exactly `len` bytes (AddressSanitizer then sees every read past it)
static bool check(const Header& h, uint64_t len, uint64_t avail, std::string* err) {
    std::unique_ptr<unsigned char[]> buf(new unsigned char[len]);  // (non-NULL also for len 0)
    std::memcpy(buf.get(), &h, len < sizeof(h) ? len : sizeof(h));
    Header out;
    return validate(buf.get(), avail, &out, err);
}

static void expect_refused(const Header& h, uint64_t len, uint64_t avail, const char* what, const char* needle = nullptr) {
    std::string err;
    cases += 1;
    if (check(h, len, avail, &err)) {
        std::printf("ACCEPTED: %s\n", what);
        failures += 1;
    } else if (needle && err.find(needle) == std::string::npos) {
        std::printf("REFUSED FOR ANOTHER REASON: %s: \"%s\" does not mention \"%s\"\n", what, err.c_str(), needle);
        failures += 1;
    }
}

// a forgery that keeps the header's own digest right, so that the structural checks behind it are what refuses
static void expect_refused_resealed(Header h, const char* what, const char* needle) {
    seal(h);
    expect_refused(h, sizeof(h), good_header().total_bytes, what, needle);
}

static int run_valid() {
    const Header h = good_header();
    std::string err;
    cases += 1;
    if (!check(h, sizeof(h), h.total_bytes, &err)) {
        std::printf("REFUSED a valid header: %s\n", err.c_str());
        return 1;
    }
    // the layout: sections in order, 8-byte aligned, sizes from the counts
    uint64_t at = HEADER_BYTES;
    for (uint32_t k = 0; k < NSEC; ++k) {
        if (h.sec[k].offset != at || h.sec[k].offset % 8) {
            std::printf("section %u at %" PRIu64 ", expected %" PRIu64 "\n", k, h.sec[k].offset, at);
            return 1;
        }
        at = (at + h.sec[k].bytes + 7) & ~7ull;
    }
    if (h.total_bytes != at || h.sec[SPHX_STATE_SEC_ALPHA].bytes != 4 * 900 || h.sec[SPHX_STATE_SEC_ACCEL].bytes != 8 * 7) return 1;
    // an empty state is a valid blob of exactly the header
    Header e;
    std::memset(&e, 0, sizeof(e));
    layout(e);
    seal(e);
    cases += 1;
    if (e.total_bytes != HEADER_BYTES || !check(e, sizeof(e), e.total_bytes, &err)) {
        std::printf("REFUSED the empty state: %s\n", err.c_str());
        return 1;
    }
    return 0;
}

// every byte of the header, several damaged values each: nothing in it can change unnoticed (the header's digest sees to that)
static void run_corrupt_bytes() {
    const Header h = good_header();
    for (size_t i = 0; i < sizeof(Header); ++i)
        for (unsigned char x : {(unsigned char)0x01, (unsigned char)0x80, (unsigned char)0xFF}) {
            Header d = h;
            ((unsigned char*)&d)[i] ^= x;
            char what[64];
            std::snprintf(what, sizeof(what), "byte %zu ^ 0x%02x", i, x);
            expect_refused(d, sizeof(d), h.total_bytes, what);
        }
}

// every field, with the header's digest recomputed: the field checks themselves
static void run_corrupt_fields() {
    Header d;
#define FORGE(stmt, what, needle) \
    d = good_header();            \
    stmt;                         \
    expect_refused_resealed(d, what, needle);
    FORGE(d.magic[0] = 's', "magic", "magic")
    FORGE(d.magic[7] = 0, "magic tail", "magic")
    FORGE(d.version = 2, "future version", "version")
    FORGE(d.version = 0, "version 0", "version")
    FORGE(d.endian_tag = 0x04030201u, "byte-swapped endianness tag", "endian")
    FORGE(d.header_bytes = 384, "header size", "header size")
    FORGE(d.n_sections = 8, "section count", "section count")
    FORGE(d.params_bytes = 76, "params size", "sphx_params")
    FORGE(d.zero = 1, "reserved word", "reserved")
    FORGE(d.params.device = 1, "params.device", "device")
    FORGE(d.total_bytes += 8, "total size + 8", "truncated")
    FORGE(d.total_bytes -= 8, "total size - 8", "longer")
    // counts that disagree
    FORGE(d.s.n += 1, "N + 1", "disagrees")
    FORGE(d.s.n -= 1, "N - 1", "disagrees")
    FORGE(d.s.n = 0, "N = 0", nullptr)
    FORGE(d.s.b += 1, "B + 1", "disagrees")
    FORGE(d.s.cached_n += 1, "cached_n + 1", "disagrees")
    FORGE(d.s.cached_n = 0, "cached_n = 0", "disagrees")
    FORGE(d.s.wcsph_n += 1, "wcsph_n + 1", "disagrees")
    FORGE(d.s.ids_issued = 1000, "ids_issued < N", "ids_issued")
    FORGE(d.s.ids_issued = (1ull << 32) + 1, "ids_issued > 2^32", "ids_issued")
    FORGE(d.s.n = 0xFFFFFFFFu, "N = 2^32 - 1", "2^28")
    FORGE(d.s.b = 0xFFFFFFFFu, "B = 2^32 - 1", "2^28")
    FORGE(d.s.n = (1u << 28) - 33, "N + B = 2^28", "2^28")
    FORGE(d.s.cached_n = 1u << 28, "cached_n = 2^28", "2^28")
    FORGE(d.s.wcsph_n = 0xFFFFFFFFu, "wcsph_n = 2^32 - 1", "2^28")
    FORGE(d.s.set_changed = 2, "set_changed = 2", "flag")
    FORGE(d.s.tiling_invariant = 0x100, "tiling_invariant = 256", "flag")
    FORGE(d.s.lists_current = 0, "sampling allowed without lists", "sampling")
    FORGE(d.s.sampling_allowed = 7, "sampling_allowed = 7", "flag")
    FORGE(d.s.num_density_iters = 202, "density iterations beyond the cap", "iteration")
    FORGE(d.s.num_divergence_iters = 0xFFFFFFFFu, "divergence iterations beyond the cap", "iteration")
    // sections: out of range, overlapping, misaligned, overflowing, misplaced
    for (uint32_t k = 0; k < NSEC; ++k) {
        FORGE(d.sec[k].offset = d.total_bytes, "section offset = total", nullptr)
        FORGE(d.sec[k].offset = 0, "section offset = 0 (inside the header)", "out of range")
        FORGE(d.sec[k].offset += 4, "section offset + 4", nullptr)
        FORGE(d.sec[k].offset += 8, "section offset + 8", nullptr)
        FORGE(d.sec[k].bytes += 4, "section bytes + 4", nullptr)
        FORGE(d.sec[k].bytes = d.total_bytes, "section bytes = total", "out of range")
        FORGE(d.sec[k].offset = 0xFFFFFFFFFFFFFFF8ull, "section offset near 2^64", "overflows")
        FORGE(d.sec[k].bytes = 0xFFFFFFFFFFFFFFFFull, "section bytes = 2^64 - 1", "overflows")
        FORGE(d.sec[k].offset = 0x8000000000000000ull; d.sec[k].bytes = 0x8000000000000000ull, "offset + bytes = 2^64", "overflows")
        if (k) {
            FORGE(d.sec[k].offset = d.sec[k - 1].offset, "section on top of its predecessor", nullptr)
        }
    }
    FORGE(std::swap(d.sec[0].offset, d.sec[1].offset), "two sections swapped", "not where")
    FORGE(d.sec[1].offset = d.sec[0].offset + 8, "velocities inside positions", "overlap")
#undef FORGE
}

// every truncation length: the buffer holds `len` bytes and the caller says so; and the buffer is complete but the caller passes less
static void run_truncations() {
    const Header h = good_header();
    for (uint64_t len = 0; len < sizeof(Header); ++len) expect_refused(h, len, len, "header cut short", "truncated");
    // (behind the header validate() reads nothing: the lengths are a claim it compares with the header's)
    for (uint64_t len = sizeof(Header); len < h.total_bytes; ++len) expect_refused(h, sizeof(Header), len, "sections cut short", "truncated");
    expect_refused(h, sizeof(Header), h.total_bytes + 1, "one byte too many", "longer");
    expect_refused(h, sizeof(Header), 0xFFFFFFFFFFFFFFFFull, "2^64 - 1 bytes claimed", "longer");
}

static void run_solver_file() {
    SolverFileHeader f;
    std::memset(&f, 0, sizeof(f));
    std::memcpy(f.magic, SOLVER_MAGIC, 8);
    f.version = VERSION;
    f.endian_tag = ENDIAN_TAG;
    f.blob_bytes = 1000;
    f.timer.cfl_factor = 1.5f;
    f.timer.timestep_max_ns = 2777778;
    f.timer.timestep_min_ns = 41667;
    f.timer.simulation_step_ns = 41667;
    std::string err;
    auto ok = [&](const SolverFileHeader& g, uint64_t len, uint64_t avail) {
        std::unique_ptr<unsigned char[]> buf(new unsigned char[len]);
        std::memcpy(buf.get(), &g, len < sizeof(g) ? len : sizeof(g));
        SolverFileHeader out;
        cases += 1;
        return validate_solver_file(buf.get(), avail, &out, &err);
    };
    if (!ok(f, sizeof(f), sizeof(f) + 1000)) std::printf("REFUSED a valid solver file header: %s\n", err.c_str()), failures += 1;
    for (uint64_t len = 0; len < sizeof(f); ++len)
        if (ok(f, len, len)) std::printf("ACCEPTED a solver file header cut to %" PRIu64 "\n", len), failures += 1;
    if (ok(f, sizeof(f), sizeof(f) + 999)) std::printf("ACCEPTED a solver file one byte short\n"), failures += 1;
    SolverFileHeader g = f;
    g.magic[4] = 'T';
    if (ok(g, sizeof(g), sizeof(g) + 1000)) std::printf("ACCEPTED a solver file with the blob's magic\n"), failures += 1;
    g = f;
    g.version = 9;
    if (ok(g, sizeof(g), sizeof(g) + 1000)) std::printf("ACCEPTED a future solver file version\n"), failures += 1;
    g = f;
    g.timer.fixed = 2;
    if (ok(g, sizeof(g), sizeof(g) + 1000)) std::printf("ACCEPTED timer.fixed = 2\n"), failures += 1;
    g = f;
    g.timer.reserved = 1;
    if (ok(g, sizeof(g), sizeof(g) + 1000)) std::printf("ACCEPTED timer.reserved = 1\n"), failures += 1;
    g = f;
    uint32_t nan_bits = 0x7FC00000u;
    std::memcpy(&g.timer.cfl_factor, &nan_bits, 4);
    if (ok(g, sizeof(g), sizeof(g) + 1000)) std::printf("ACCEPTED a NaN cfl factor\n"), failures += 1;
    g = f;
    g.blob_bytes = 0xFFFFFFFFFFFFFFFFull;
    if (ok(g, sizeof(g), sizeof(g) + 1000)) std::printf("ACCEPTED a blob size of 2^64 - 1\n"), failures += 1;
}

static void run_params() {
    sphx_params a;
    std::memset(&a, 0, sizeof(a));
    a.smoothing_length = 0.02f;
    a.fluid_viscosity = 0.001f;
    sphx_params b = a;
    cases += 3;
    if (params_mismatch(a, b)) std::printf("equal params reported as different\n"), failures += 1;
    b.device = 3;
    b.list_span_limit = 77;
    if (params_mismatch(a, b)) std::printf("device / list_span_limit are not free\n"), failures += 1;
    b.fluid_viscosity = 0.002f;
    const char* f = params_mismatch(a, b);
    if (!f || std::strcmp(f, "fluid_viscosity") != 0) std::printf("fluid_viscosity mismatch not named (%s)\n", f ? f : "null"), failures += 1;
    // every byte of the struct belongs to a compared field or to one of the two free ones
    for (size_t i = 0; i < sizeof(sphx_params); ++i) {
        b = a;
        ((unsigned char*)&b)[i] ^= 0x40;
        const bool is_free = (i >= offsetof(sphx_params, device) && i < offsetof(sphx_params, device) + 4) ||
                             (i >= offsetof(sphx_params, list_span_limit) && i < offsetof(sphx_params, list_span_limit) + 4);
        cases += 1;
        if ((params_mismatch(a, b) != nullptr) == is_free) std::printf("params byte %zu: wrong verdict\n", i), failures += 1;
    }
}

int main(int argc, char** argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "digest") {
        std::vector<uint32_t> w;
        for (int a = 2; a < argc; ++a) w.push_back((uint32_t)std::strtoul(argv[a], nullptr, 16));
        std::printf("%016" PRIx64 "\n", digest_words(w.data(), w.size()));
        return 0;
    }
    if (what == "header") {  // the valid header as hex, for the Python parser of tests/state_reference.py
        const Header h = good_header();
        for (size_t i = 0; i < sizeof(h); ++i) std::printf("%02x", ((const unsigned char*)&h)[i]);
        std::printf("\n");
        return 0;
    }
    if (run_valid()) return 1;
    if (what == "valid") {
    } else if (what == "corrupt_bytes") {
        run_corrupt_bytes();
    } else if (what == "corrupt_fields") {
        run_corrupt_fields();
    } else if (what == "truncations") {
        run_truncations();
    } else if (what == "solver_file") {
        run_solver_file();
    } else if (what == "params") {
        run_params();
    } else {
        std::fprintf(stderr, "usage: state_format_driver valid|corrupt_bytes|corrupt_fields|truncations|solver_file|params|header|digest <hex>...\n");
        return 2;
    }
    if (failures) return 1;
    std::printf("ok %ld\n", cases);
    return 0;
}
