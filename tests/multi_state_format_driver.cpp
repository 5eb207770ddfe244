// multi_state_format_driver — the layout and validation of a tiled checkpoint's parts (yasph2d_amd/csrc/sphx_multi_state_format.hpp) as a
// stand-alone host program, built by tests/test_multi_state_host.py with -fsanitize=address,undefined.  It builds well-formed parts, checks
// that validate() / validate_set() accept them, and that every damaged variant is refused without a read outside the buffer given.
//   multi_state_format_driver <check>                    prints "ok <cases>" and exits 0, or prints what went wrong and exits 1
//   multi_state_format_driver digest <k> <id:hexword[,hexword]>...   the id-keyed digest of the particles (k words each)
//   multi_state_format_driver header                     a valid header in hex (for the parser of tests/multi_state_reference.py)
#include <cinttypes>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "sphx_multi_state_format.hpp"

using namespace sphx_multi_state;

static long cases = 0;
static int failures = 0;

// part `part` of `n_parts` of a 2 x 2 run (n_parts 1 or 4) holding n_part of 1001 particles
static Header good_header(uint32_t part = 0, uint32_t n_parts = 1, uint32_t n_part = 1001) {
    Header h;
    std::memset(&h, 0, sizeof(h));
    h.params.smoothing_length = 0.02f;
    h.params.max_density_iterations = 200;
    h.params.max_divergence_iterations = 400;
    h.s.n_total = 1001;  // (odd: the 4-byte sections are followed by padding)
    h.s.n_part = n_part;
    h.s.b = 33;
    h.s.part = part;
    h.s.n_parts = n_parts;
    h.s.num_density_iters = 3;
    h.s.num_divergence_iters = 2;
    h.s.last_div_iters = 2;
    h.s.last_div_warm = 1;
    h.s.steps = 40;
    h.s.tiling_invariant = 1;
    h.s.world = 4;
    h.s.axis = -1;
    h.s.nx = h.s.ny = 2;
    const uint32_t cuts[9] = {0, 40, 65536, 0, 17, 65536, 0, 23, 65536};
    std::memcpy(h.s.cuts, cuts, sizeof(cuts));
    h.s.n_cuts = 9;
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
static void expect_accepted(Header h, const char* what) {
    layout(h);
    seal(h);
    std::string err;
    cases += 1;
    if (!check(h, sizeof(h), h.total_bytes, &err)) {
        std::printf("REFUSED %s: %s\n", what, err.c_str());
        failures += 1;
    }
}

static void run_valid() {
    const Header h = good_header();
    expect_accepted(h, "a valid header");
    uint64_t at = HEADER_BYTES;
    for (uint32_t k = 0; k < NSEC; ++k) {
        if (h.sec[k].offset != at || h.sec[k].offset % 8) {
            std::printf("section %u at %" PRIu64 ", expected %" PRIu64 "\n", k, h.sec[k].offset, at);
            failures += 1;
        }
        at = (at + h.sec[k].bytes + 7) & ~7ull;
    }
    if (h.total_bytes != at || h.sec[0].bytes != 8 * 1001 || h.sec[5].bytes != 4 * 1001 || h.sec[SEC_BOUNDARY].bytes != 8 * 33) failures += 1;
    // an empty run on one tile: exactly the header
    Header e;
    std::memset(&e, 0, sizeof(e));
    e.s.n_parts = e.s.world = 1;
    e.s.nx = e.s.ny = 1;
    e.s.cuts[1] = 65536;
    e.s.n_cuts = 2;
    expect_accepted(e, "the empty run");
    layout(e);
    if (e.total_bytes != HEADER_BYTES) failures += 1;
    // strips, 64 of them; a 64 x 1 grid (the most cuts a layout can have)
    Header s = good_header();
    s.s.world = 64;
    s.s.axis = 1;
    s.s.nx = s.s.ny = 1;
    std::memset(s.s.cuts, 0, sizeof(s.s.cuts));
    for (uint32_t i = 0; i <= 64; ++i) s.s.cuts[i] = i < 64 ? i * 100 : 65536;
    s.s.n_cuts = 65;
    expect_accepted(s, "64 strips");
    Header g = good_header();
    g.s.world = 64;
    g.s.nx = 64;
    g.s.ny = 1;
    std::memset(g.s.cuts, 0, sizeof(g.s.cuts));
    for (uint32_t i = 0; i <= 64; ++i) g.s.cuts[i] = i < 64 ? i * 100 : 65536;
    for (uint32_t ix = 0; ix < 64; ++ix) g.s.cuts[65 + 2 * ix + 1] = 65536;
    g.s.n_cuts = 65 + 128;
    expect_accepted(g, "a 64 x 1 grid");
    // a part of a set
    expect_accepted(good_header(2, 4, 300), "part 2 of 4");
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

static void run_corrupt_fields() {
    const Header h = good_header();
    Header d;
#define FORGE(stmt, what, needle) \
    d = h;                        \
    stmt;                         \
    expect_refused_resealed(d, what, needle)
    FORGE(d.magic[7] = 'X', "magic", "bad magic");
    FORGE(std::memcpy(d.magic, sphx_state::MAGIC, 8), "the single-context magic", "single-context");
    FORGE(d.version = 2, "version", "format version");
    FORGE(d.endian_tag = 0x04030201u, "endianness", "endianness");
    FORGE(d.header_bytes = 392, "header size", "header size");
    FORGE(d.n_sections = 9, "section count", "section count");
    FORGE(d.params_bytes = 76, "params size", "sizeof(sphx_params)");
    FORGE(d.zero = 1, "reserved word", "reserved");
    FORGE(d.params.device = 1, "device", "device");
    FORGE(d.total_bytes += 8, "total size", "longer than the buffer");
    FORGE(d.total_bytes -= 8, "total size (short)", "longer than the part says");
    // counts that disagree
    FORGE(d.s.n_total = (1ull << 31) + 1, "N_total", "N_total");
    FORGE(d.s.n_part = 1u << 28, "N_part", "2^28");
    FORGE(d.s.b = 1u << 28, "B", "2^28");
    FORGE(d.s.n_part = 1002, "N_part > N_total", "larger than N_total");
    FORGE(d.s.n_part = 1000, "N_part != N_total in the only part", "only part");
    FORGE(d.s.n_parts = 0, "n_parts 0", "n_parts");
    FORGE(d.s.n_parts = 65, "n_parts 65", "n_parts");
    FORGE(d.s.part = 1, "part >= n_parts", "part index");
    FORGE(d.s.n_parts = 3; d.s.n_part = 10, "n_parts neither 1 nor world", "neither 1 nor");
    FORGE(d.s.tiling_invariant = 2, "flag", "neither 0 nor 1");
    FORGE(d.s.last_div_warm = 2, "last_div_warm", "neither 0 nor 1");
    FORGE(d.s.num_density_iters = 202, "density iterations", "iteration cap");
    FORGE(d.s.num_divergence_iters = 402, "divergence iterations", "iteration cap");
    FORGE(d.s.last_div_iters = 402, "last divergence iterations", "iteration cap");
    // the saver's layout
    FORGE(d.s.world = 0, "world 0", "tile count");
    FORGE(d.s.world = 65, "world 65", "tile count");
    FORGE(d.s.axis = 2, "axis", "axis");
    FORGE(d.s.nx = 3, "nx * ny != world", "nx * ny");
    FORGE(d.s.n_cuts = 8, "n_cuts", "cuts");
    FORGE(d.s.cuts[0] = 1, "first cut", "column cuts");
    FORGE(d.s.cuts[2] = 65535, "last cut", "column cuts");
    FORGE(d.s.cuts[4] = 0, "a column's cuts not increasing", "a column's cuts");
    FORGE(d.s.cuts[9] = 5, "an unused cut", "unused cut");
    FORGE(d.s.axis = 0, "strips with a grid's cuts", "nx or ny");
    FORGE(d.s.axis = 0; d.s.nx = d.s.ny = 1, "strips with too many cuts", "world + 1 cuts");
    FORGE(d.s.nx = 0xFFFFFFFFu; d.s.ny = 0xFFFFFFFCu, "nx * ny wraps to the tile count", "nx * ny");
    // the section table
    FORGE(d.sec[3].offset = ~0ull - 7, "offset + size overflows", "overflows");
    FORGE(d.sec[2].offset = 8, "section inside the header", "out of range");
    FORGE(d.sec[7].offset = d.total_bytes, "section past the end", "out of range");
    FORGE(d.sec[1].offset += 4, "misaligned section", "aligned");
    FORGE(d.sec[4].bytes -= 4, "size disagrees", "disagrees with the counts");
    FORGE(d.sec[1].offset = d.sec[0].offset, "overlap", "overlap");
    FORGE(std::swap(d.sec[3].offset, d.sec[4].offset), "misplaced sections", "not where the layout puts it");
#undef FORGE
}

static void run_truncations() {
    const Header h = good_header();
    for (uint64_t len = 0; len < sizeof(Header); ++len) expect_refused(h, len, len, "shorter than the header", "truncated");
    for (uint64_t len : {(uint64_t)sizeof(Header), h.total_bytes - 1, h.total_bytes - 8, h.sec[3].offset, h.sec[7].offset})
        expect_refused(h, sizeof(h), len, "shorter than the part", "truncated");
    expect_refused(h, sizeof(h), h.total_bytes + 8, "longer than the part", "longer than the part says");
    std::string err;
    cases += 1;
    if (validate(nullptr, 100, nullptr, &err)) failures += 1;
}

static void set_case(std::vector<Header> hs, bool want_ok, const char* what, const char* needle = nullptr) {
    for (Header& h : hs) {  // every part is valid on its own: the SET is what is wrong
        seal(h);
        std::string e;
        if (!check(h, sizeof(h), h.total_bytes, &e)) {
            std::printf("a part of the set case '%s' is not valid on its own: %s\n", what, e.c_str());
            failures += 1;
        }
    }
    std::string err;
    cases += 1;
    const bool ok = validate_set(hs.data(), (uint32_t)hs.size(), &err);
    if (ok != want_ok) {
        std::printf("%s: %s (%s)\n", ok ? "ACCEPTED" : "REFUSED", what, err.c_str());
        failures += 1;
    } else if (!ok && needle && err.find(needle) == std::string::npos) {
        std::printf("REFUSED FOR ANOTHER REASON: %s: \"%s\" does not mention \"%s\"\n", what, err.c_str(), needle);
        failures += 1;
    }
}

static void run_sets() {
    const uint32_t np[4] = {300, 0, 401, 300};
    std::vector<Header> good;
    for (uint32_t r = 0; r < 4; ++r) good.push_back(good_header(r, 4, np[r]));
    set_case(good, true, "four parts");
    set_case({good[2], good[0], good[3], good[1]}, true, "four parts in another order");
    set_case({good_header()}, true, "the one part");
    set_case({good[0], good[1], good[2]}, false, "a missing part", "missing");
    set_case({good[0], good[1], good[2], good[2]}, false, "a duplicated part", "twice");
    set_case({good[0], good[1], good[2], good[3], good[3]}, false, "one part too many", "more parts");
    std::string err;
    cases += 1;
    if (validate_set(nullptr, 0, &err) || validate_set(good.data(), 0, &err)) failures += 1;
    std::vector<Header> v;
#define VARY(stmt, what, needle) \
    v = good;                    \
    stmt;                        \
    set_case(v, false, what, needle)
    VARY(v[1].s.n_part = 1; layout(v[1]), "counts that do not add up", "add up");
    VARY(v[2].s.b = 34; layout(v[2]), "another boundary count", "N_total or B");
    VARY(v[2].s.n_total = 1002, "another N_total", "N_total or B");
    VARY(v[3].s.num_density_iters = 1, "another density iteration count", "iteration counts");
    VARY(v[3].s.num_divergence_iters = 1, "another divergence iteration count", "iteration counts");
    VARY(v[3].s.last_div_iters = 1, "another last_div_iters", "iteration counts");
    VARY(v[3].s.last_div_warm = 0, "another last_div_warm", "iteration counts");
    VARY(v[1].s.steps = 41, "another step", "different steps");
    VARY(v[1].s.tiling_invariant = 0, "another mode", "tiling-invariant");
    VARY(v[1].s.cuts[1] = 41, "another layout", "layout");
    VARY(v[2].sec[SEC_BOUNDARY].digest ^= 1, "another boundary digest", "different boundaries");
    VARY(v[2].params.particle_mass = 1.0f, "other params", "params");
#undef VARY
}

// the params rule of the loader: every field but device and list_span_limit, the first that differs is named
static void run_params() {
    const Header h = good_header();
    sphx_params p = h.params;
    cases += 1;
    if (sphx_state::params_mismatch(h.params, p)) failures += 1;
    p.device = 3;
    p.list_span_limit = 77;
    cases += 1;
    if (sphx_state::params_mismatch(h.params, p)) failures += 1;
#define FIELD(f, lv, value)                                                           \
    p = h.params;                                                                   \
    p.lv = value;                                                                   \
    cases += 1;                                                                     \
    {                                                                               \
        const char* m = sphx_state::params_mismatch(h.params, p);                   \
        if (!m || std::strcmp(m, #f) != 0) {                                        \
            std::printf("params differing in %s: reported %s\n", #f, m ? m : "-"); \
            failures += 1;                                                          \
        }                                                                           \
    }
    FIELD(smoothing_length, smoothing_length, 0.03f)
    FIELD(particle_mass, particle_mass, 2.0f)
    FIELD(fluid_density, fluid_density, 999.0f)
    FIELD(particle_radius, particle_radius, 0.5f)
    FIELD(gravity, gravity[1], -1.0f)
    FIELD(grid_min, grid_min[0], -3.0f)
    FIELD(xsph_epsilon, xsph_epsilon, 0.5f)
    FIELD(max_avg_density_error, max_avg_density_error, 0.5f)
    FIELD(max_density_iterations, max_density_iterations, 7)
    FIELD(max_divergence_error, max_divergence_error, 0.5f)
    FIELD(max_divergence_iterations, max_divergence_iterations, 7)
    FIELD(fixed_density_iterations, fixed_density_iterations, 2)
    FIELD(fixed_divergence_iterations, fixed_divergence_iterations, 2)
    FIELD(viscosity_model, viscosity_model, 1)
    FIELD(fluid_viscosity, fluid_viscosity, 0.5f)
    FIELD(reserved, reserved[0], 1)
#undef FIELD
}

// the checkpoint file of the solver object and the splitting of parts that lie back to back
static void run_file() {
    const Header a = good_header(0, 4, 300), b = good_header(1, 4, 0);
    std::vector<unsigned char> body(a.total_bytes + b.total_bytes, 0);
    std::memcpy(body.data(), &a, sizeof(a));
    std::memcpy(body.data() + a.total_bytes, &b, sizeof(b));
    std::vector<std::pair<uint64_t, uint64_t>> pieces;
    std::string err;
    cases += 1;
    if (!split_parts(body.data(), body.size(), &pieces, &err) || pieces.size() != 2 || pieces[1].first != a.total_bytes || pieces[1].second != b.total_bytes) {
        std::printf("split_parts: %s\n", err.c_str());
        failures += 1;
    }
    for (uint64_t len = 1; len < body.size(); len += 97) {  // every truncated length: exact heap copy, refused or split into fewer parts
        std::unique_ptr<unsigned char[]> buf(new unsigned char[len]);
        std::memcpy(buf.get(), body.data(), len);
        cases += 1;
        if (split_parts(buf.get(), len, &pieces, &err) && len != a.total_bytes) {
            std::printf("split_parts accepted %" PRIu64 " bytes\n", len);
            failures += 1;
        }
    }
    CheckpointFileHeader fh;
    std::memset(&fh, 0, sizeof(fh));
    std::memcpy(fh.magic, CHECKPOINT_MAGIC, 8);
    fh.version = VERSION;
    fh.endian_tag = ENDIAN_TAG;
    fh.parts_bytes = 1000;
    fh.timer.cfl_factor = 0.4f;
    CheckpointFileHeader out;
    cases += 1;
    if (!validate_checkpoint_file(&fh, sizeof(fh) + 1000, &out, &err)) failures += 1;
    for (uint64_t len = 0; len < sizeof(fh); ++len) {
        std::unique_ptr<unsigned char[]> buf(new unsigned char[len ? len : 1]);
        std::memcpy(buf.get(), &fh, len);
        cases += 1;
        if (validate_checkpoint_file(buf.get(), len, &out, &err)) failures += 1;
    }
    CheckpointFileHeader d = fh;
    d.magic[0] = 'X';
    cases += 5;
    if (validate_checkpoint_file(&d, sizeof(d) + 1000, &out, &err)) failures += 1;
    d = fh, d.version = 2;
    if (validate_checkpoint_file(&d, sizeof(d) + 1000, &out, &err)) failures += 1;
    d = fh, d.timer.fixed = 2;
    if (validate_checkpoint_file(&d, sizeof(d) + 1000, &out, &err)) failures += 1;
    if (validate_checkpoint_file(&fh, sizeof(fh) + 999, &out, &err)) failures += 1;
    if (validate_checkpoint_file(&fh, sizeof(fh) + 1001, &out, &err)) failures += 1;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string what = argv[1];
    if (what == "digest") {  // digest <k> <id:hex[,hex]>...
        if (argc < 3) return 2;
        const uint32_t k = (uint32_t)std::strtoul(argv[2], nullptr, 10);
        if (k != 1 && k != 2) return 2;
        std::vector<uint32_t> ids, words;
        for (int i = 3; i < argc; ++i) {
            char* end = nullptr;
            ids.push_back((uint32_t)std::strtoul(argv[i], &end, 10));
            for (uint32_t c = 0; c < k; ++c) {
                if (!end || (*end != ':' && *end != ',')) return 2;
                words.push_back((uint32_t)std::strtoul(end + 1, &end, 16));
            }
        }
        std::printf("%" PRIx64 "\n", digest_by_id(words.data(), ids.data(), ids.size(), k));
        return 0;
    }
    if (what == "header") {
        const Header h = good_header();
        const unsigned char* p = (const unsigned char*)&h;
        for (size_t i = 0; i < sizeof(h); ++i) std::printf("%02x", p[i]);
        std::printf("\n");
        return 0;
    }
    if (what == "valid")
        run_valid();
    else if (what == "corrupt_bytes")
        run_corrupt_bytes();
    else if (what == "corrupt_fields")
        run_corrupt_fields();
    else if (what == "truncations")
        run_truncations();
    else if (what == "sets")
        run_sets();
    else if (what == "params")
        run_params();
    else if (what == "file")
        run_file();
    else
        return 2;
    if (failures) return 1;
    std::printf("ok %ld\n", cases);
    return 0;
}
