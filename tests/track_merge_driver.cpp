// track_merge_driver.cpp — the host merge of following particles in a tiled run (csrc/sphx_track_merge.hpp) as a stand-alone program,
// compiled by tests/test_track_multi_host.py with -fsanitize=address,undefined.
//   track_merge_driver <check>    check = random | empty | absent | two | scatter | capacity | nanbits | frames | checks
// Prints "ok <number of comparisons>" and exits 0, or says what differed and exits 1.  The expected values come from a brute-force
// restatement of the rule in include/sphx.h: an entry belongs to the part with the greatest (tile, slot) that holds it.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "sphx_track_merge.hpp"

namespace th = sphx_track_host;

static long g_checks = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        ++g_checks;                                                         \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

static float as_float(uint32_t w) {
    float f;
    std::memcpy(&f, &w, 4);
    return f;
}
static uint32_t as_word(float f) {
    uint32_t w;
    std::memcpy(&w, &f, 4);
    return w;
}

// an answer of m entries that owns its arrays
struct Answer {
    std::vector<uint32_t> tile, slot;
    std::vector<float> pos, vel, density;
    explicit Answer(uint32_t m) : tile(m, th::ABSENT), slot(m, th::ABSENT), pos(2 * (size_t)m, as_float(th::ABSENT_WORD)), vel(pos), density(m, as_float(th::ABSENT_WORD)) {}
    sphx_multi_track_out view() { return sphx_multi_track_out{tile.data(), slot.data(), pos.data(), vel.data(), density.data()}; }
    th::Acc acc() { return th::Acc{tile.data(), slot.data(), (uint32_t*)pos.data(), (uint32_t*)vel.data(), (uint32_t*)density.data()}; }
};
static bool same(Answer& a, Answer& b) {
    if (a.tile.empty() || b.tile.empty()) return a.tile.size() == b.tile.size();  // (no bytes to compare: memcmp takes no null pointer)
    return a.tile == b.tile && a.slot == b.slot && !std::memcmp(a.pos.data(), b.pos.data(), a.pos.size() * 4) &&
           !std::memcmp(a.vel.data(), b.vel.data(), a.vel.size() * 4) && !std::memcmp(a.density.data(), b.density.data(), a.density.size() * 4);
}

// the rule restated: scan every part for every entry
static Answer brute(uint32_t m, std::vector<Answer>& parts) {
    Answer r(m);
    for (uint32_t k = 0; k < m; ++k) {
        int best = -1;
        for (size_t p = 0; p < parts.size(); ++p) {
            if (parts[p].tile[k] == th::ABSENT) continue;
            if (best < 0 || parts[p].tile[k] > parts[best].tile[k] || (parts[p].tile[k] == parts[best].tile[k] && parts[p].slot[k] > parts[best].slot[k])) best = (int)p;
        }
        if (best < 0) continue;
        Answer& s = parts[best];
        r.tile[k] = s.tile[k];
        r.slot[k] = s.slot[k];
        for (int j = 0; j < 2; ++j) {
            r.pos[2 * k + j] = s.pos[2 * k + j];
            r.vel[2 * k + j] = s.vel[2 * k + j];
        }
        r.density[k] = s.density[k];
    }
    return r;
}

static Answer run_merge(uint32_t m, std::vector<Answer>& parts) {
    std::vector<sphx_multi_track_out> views;
    for (auto& p : parts) views.push_back(p.view());
    Answer out(m);
    const sphx_multi_track_out o = out.view();
    if (m) EXPECT(th::merge_error(m, views.data(), (uint32_t)views.size(), &o) == nullptr);  // (m == 0: the empty vectors have no address to name an output with)
    // (start from garbage: merge fills the absent words itself)
    std::fill(out.tile.begin(), out.tile.end(), 12345u);
    std::fill(out.pos.begin(), out.pos.end(), 1.0f);
    th::merge(m, views.data(), (uint32_t)views.size(), out.acc());
    return out;
}

static void fill_entry(Answer& a, uint32_t k, uint32_t tile, uint32_t slot, std::mt19937& g) {
    a.tile[k] = tile;
    a.slot[k] = slot;
    for (int j = 0; j < 2; ++j) {
        a.pos[2 * k + j] = as_float((uint32_t)g());
        a.vel[2 * k + j] = as_float((uint32_t)g());
    }
    a.density[k] = as_float((uint32_t)g());
}

static void check_random() {
    std::mt19937 g(20261020u);
    for (int round = 0; round < 200; ++round) {
        const uint32_t m = g() % 300u, n_parts = 1u + g() % 6u;
        std::vector<Answer> parts;
        for (uint32_t p = 0; p < n_parts; ++p) {
            parts.emplace_back(m);
            const uint32_t tile = g() % 4u;  // (several parts may claim one tile rank: the slot decides then)
            for (uint32_t k = 0; k < m; ++k)
                if (g() % 3u == 0u) fill_entry(parts.back(), k, tile, g() % 5u, g);
        }
        Answer want = brute(m, parts), got = run_merge(m, parts);
        EXPECT(same(want, got));
        uint32_t present = 0;
        for (uint32_t k = 0; k < m; ++k) present += want.tile[k] != th::ABSENT;
        EXPECT(th::count_present(got.tile.data(), m) == present);
    }
}

static void check_empty() {
    std::vector<Answer> none;
    Answer got = run_merge(7, none), want(7);
    EXPECT(same(want, got));
    std::vector<Answer> zero;
    zero.emplace_back(0);
    zero.emplace_back(0);
    Answer g0 = run_merge(0, zero), w0(0);
    EXPECT(same(w0, g0));
    // a tile without an owned particle: no records, nothing folded
    Answer a(5), b(5);
    EXPECT(th::scatter_records(a.acc(), 3, 5, nullptr, 0) == 0u);
    EXPECT(same(a, b));
    th::fold_unique(a.acc(), 3, 0, nullptr, nullptr, nullptr);
    EXPECT(same(a, b));
}

static void check_absent() {
    std::vector<Answer> parts;
    for (int p = 0; p < 3; ++p) parts.emplace_back(40);
    // floats of an absent entry are ignored whatever they hold
    parts[1].pos[6] = 3.0f;
    parts[2].density[5] = -1.0f;
    Answer got = run_merge(40, parts), want(40);
    EXPECT(same(want, got));
    EXPECT(th::count_present(got.tile.data(), 40) == 0u);
    for (uint32_t k = 0; k < 40; ++k) EXPECT(as_word(got.density[k]) == 0x7FC00000u && as_word(got.vel[2 * k + 1]) == 0x7FC00000u);
}

static void check_two() {
    std::mt19937 g(7u);
    std::vector<Answer> parts;
    for (int p = 0; p < 3; ++p) parts.emplace_back(4);
    fill_entry(parts[0], 0, 2, 9, g);  // entry 0: tile 2 beats tile 1 whatever the slots and the order of the parts
    fill_entry(parts[1], 0, 1, 100, g);
    fill_entry(parts[0], 1, 1, 5, g);  // entry 1: the same tile, the greater slot (a later part)
    fill_entry(parts[2], 1, 1, 6, g);
    fill_entry(parts[1], 2, 3, 8, g);  // entry 2: the same tile, the greater slot (an earlier part)
    fill_entry(parts[2], 2, 3, 7, g);
    fill_entry(parts[0], 3, 0, 4, g);  // entry 3: an equal pair keeps the earlier part
    fill_entry(parts[1], 3, 0, 4, g);
    Answer got = run_merge(4, parts);
    EXPECT(got.tile[0] == 2u && got.slot[0] == 9u && as_word(got.pos[0]) == as_word(parts[0].pos[0]));
    EXPECT(got.tile[1] == 1u && got.slot[1] == 6u && as_word(got.density[1]) == as_word(parts[2].density[1]));
    EXPECT(got.tile[2] == 3u && got.slot[2] == 8u && as_word(got.vel[5]) == as_word(parts[1].vel[5]));
    EXPECT(got.tile[3] == 0u && got.slot[3] == 4u && as_word(got.density[3]) == as_word(parts[0].density[3]));
    Answer want = brute(4, parts);
    EXPECT(same(want, got));
    // the same through the window scatter: two tiles hold index 1
    const uint32_t r0[8] = {1, 50, 11, 12, 13, 14, 15, 0}, r1[8] = {1, 3, 21, 22, 23, 24, 25, 0};
    Answer a(2), b(2);
    th::scatter_records(a.acc(), 1, 2, r1, 1);
    th::scatter_records(a.acc(), 0, 2, r0, 1);
    th::scatter_records(b.acc(), 0, 2, r0, 1);
    th::scatter_records(b.acc(), 1, 2, r1, 1);
    EXPECT(same(a, b) && a.tile[1] == 1u && a.slot[1] == 3u && as_word(a.pos[2]) == 21u && as_word(a.density[1]) == 25u && a.tile[0] == th::ABSENT);
}

// `n` records for distinct indices below count, in a shuffled order
static std::vector<uint32_t> make_records(uint32_t count, uint32_t n, std::mt19937& g, std::vector<uint32_t>* index_out) {
    std::vector<uint32_t> idx(count);
    for (uint32_t k = 0; k < count; ++k) idx[k] = k;
    std::shuffle(idx.begin(), idx.end(), g);
    idx.resize(n);
    std::vector<uint32_t> rec((size_t)n * th::RECORD_WORDS);
    for (uint32_t r = 0; r < n; ++r) {
        uint32_t* w = rec.data() + (size_t)r * th::RECORD_WORDS;
        w[0] = idx[r];
        w[1] = (uint32_t)g() % 1000u;
        for (int j = 2; j < 7; ++j) w[j] = (uint32_t)g();
        w[7] = 0;
    }
    *index_out = idx;
    return rec;
}
static void expect_scattered(Answer& a, uint32_t tile, uint32_t count, const std::vector<uint32_t>& rec, const std::vector<uint32_t>& idx) {
    std::vector<int> from(count, -1);
    for (size_t r = 0; r < idx.size(); ++r) from[idx[r]] = (int)r;
    for (uint32_t k = 0; k < count; ++k) {
        if (from[k] < 0) {
            EXPECT(a.tile[k] == th::ABSENT && a.slot[k] == th::ABSENT && as_word(a.pos[2 * k]) == 0x7FC00000u && as_word(a.density[k]) == 0x7FC00000u);
            continue;
        }
        const uint32_t* w = rec.data() + (size_t)from[k] * th::RECORD_WORDS;
        EXPECT(a.tile[k] == tile && a.slot[k] == w[1]);
        EXPECT(as_word(a.pos[2 * k]) == w[2] && as_word(a.pos[2 * k + 1]) == w[3] && as_word(a.vel[2 * k]) == w[4] && as_word(a.vel[2 * k + 1]) == w[5] &&
               as_word(a.density[k]) == w[6]);
    }
}

static void check_scatter() {
    std::mt19937 g(99u);
    for (int round = 0; round < 50; ++round) {
        const uint32_t count = 1u + g() % 500u, n = g() % (count + 1u);
        std::vector<uint32_t> idx;
        const std::vector<uint32_t> rec = make_records(count, n, g, &idx);
        Answer a(count);
        std::fill(a.tile.begin(), a.tile.end(), 77u);  // (absent fill first, as the library does)
        th::fill_absent(a.acc(), count);
        EXPECT(th::scatter_records(a.acc(), 5, count, rec.data(), n) == 0u);
        expect_scattered(a, 5, count, rec, idx);
        // a subset of the outputs gives the same bits
        Answer b(count);
        th::Acc sub = b.acc();
        sub.vel = nullptr;
        th::scatter_records(sub, 5, count, rec.data(), n);
        EXPECT(b.tile == a.tile && b.slot == a.slot && !std::memcmp(b.pos.data(), a.pos.data(), a.pos.size() * 4) &&
               !std::memcmp(b.density.data(), a.density.data(), a.density.size() * 4));
        for (float v : b.vel) EXPECT(as_word(v) == 0x7FC00000u);
    }
    // a record outside the window is skipped and counted, never written
    const uint32_t bad[16] = {4, 1, 2, 3, 4, 5, 6, 0, 0xFFFFFFFFu, 1, 2, 3, 4, 5, 6, 0};
    Answer c(4), d(4);
    EXPECT(th::scatter_records(c.acc(), 0, 4, bad, 2) == 2u);
    EXPECT(same(c, d));
}

static void check_capacity() {
    std::mt19937 g(5u);
    // the tile's buffer is exactly full: as many records as the capacity, every index of the window taken
    const uint32_t cap = 257;
    std::vector<uint32_t> idx;
    const std::vector<uint32_t> rec = make_records(cap, cap, g, &idx);
    std::vector<uint32_t> buf(th::HEADER_WORDS + (size_t)cap * th::RECORD_WORDS);  // as a tile returns it: the counter, then the records
    buf[0] = cap;
    std::copy(rec.begin(), rec.end(), buf.begin() + th::HEADER_WORDS);
    Answer a(cap);
    EXPECT(th::scatter_records(a.acc(), 1, cap, buf.data() + th::HEADER_WORDS, buf[0]) == 0u);
    expect_scattered(a, 1, cap, rec, idx);
    EXPECT(th::count_present(a.tile.data(), cap) == cap);
}

static void check_nanbits() {
    // a particle whose floats are all 0x7FC00000 is present: presence is the tile / slot word
    const uint32_t W = th::ABSENT_WORD;
    const uint32_t rec[8] = {1, 6, W, W, W, W, W, 0};
    Answer a(3);
    th::scatter_records(a.acc(), 2, 3, rec, 1);
    EXPECT(a.tile[1] == 2u && a.slot[1] == 6u && as_word(a.pos[2]) == W && th::count_present(a.tile.data(), 3) == 1u);
    const uint32_t slot[2] = {th::ABSENT, 9}, xyvv[8] = {1, 2, 3, 4, W, W, W, W}, den[2] = {5, W};
    Answer b(2);
    th::fold_unique(b.acc(), 4, 2, slot, xyvv, den);
    EXPECT(b.tile[0] == th::ABSENT && as_word(b.pos[0]) == W);  // (slot absent: the floats 1..4 are not taken)
    EXPECT(b.tile[1] == 4u && b.slot[1] == 9u && as_word(b.vel[3]) == W);
    std::vector<Answer> parts;
    parts.push_back(a);
    parts.emplace_back(3);
    Answer got = run_merge(3, parts);
    EXPECT(got.tile[1] == 2u && th::count_present(got.tile.data(), 3) == 1u);
    // frames: the tile word decides
    const float f0[8] = {as_float(W), as_float(W), as_float(W), as_float(W), 1, 2, 3, 4};
    const uint32_t t0[2] = {0, th::ABSENT};
    const float* fp[1] = {f0};
    const uint32_t* tp[1] = {t0};
    float out[8];
    uint32_t out_tile[2];
    th::merge_frames(2, fp, tp, 1, out, out_tile);
    EXPECT(out_tile[0] == 0u && out_tile[1] == th::ABSENT && as_word(out[0]) == W && as_word(out[4]) == W && as_word(out[7]) == W);
}

static void check_frames() {
    std::mt19937 g(31u);
    for (int round = 0; round < 100; ++round) {
        const size_t n = g() % 200u;
        const uint32_t n_parts = g() % 5u;
        std::vector<std::vector<float>> f(n_parts, std::vector<float>(4 * n));
        std::vector<std::vector<uint32_t>> t(n_parts, std::vector<uint32_t>(n, th::ABSENT));
        for (uint32_t p = 0; p < n_parts; ++p)
            for (size_t k = 0; k < n; ++k) {
                for (int j = 0; j < 4; ++j) f[p][4 * k + j] = as_float((uint32_t)g());
                if (g() % 3u == 0u) t[p][k] = g() % 4u;
            }
        std::vector<const float*> fp;
        std::vector<const uint32_t*> tp;
        for (uint32_t p = 0; p < n_parts; ++p) fp.push_back(f[p].data()), tp.push_back(t[p].data());
        std::vector<float> out(4 * n + 1, 0.5f);
        std::vector<uint32_t> out_tile(n + 1, 9u);
        EXPECT(th::merge_frames_error(n, fp.data(), tp.data(), n_parts, out.data()) == nullptr);
        th::merge_frames(n, fp.data(), tp.data(), n_parts, out.data(), out_tile.data());
        for (size_t k = 0; k < n; ++k) {
            int best = -1;
            for (uint32_t p = 0; p < n_parts; ++p)
                if (t[p][k] != th::ABSENT && (best < 0 || t[p][k] > t[best][k])) best = (int)p;
            EXPECT(out_tile[k] == (best < 0 ? th::ABSENT : t[best][k]));
            for (int j = 0; j < 4; ++j) EXPECT(as_word(out[4 * k + j]) == (best < 0 ? 0x7FC00000u : as_word(f[best][4 * k + j])));
        }
        EXPECT(out[4 * n] == 0.5f && out_tile[n] == 9u);
    }
    // a tile's own frames into the frames over the distinct ids: (tile, slot) decides, absent slots are skipped
    uint32_t xyvv[8], tile_w[2] = {th::ABSENT, th::ABSENT}, slot_w[2] = {th::ABSENT, th::ABSENT};
    th::fill_words(xyvv, 8, th::ABSENT_WORD);
    const uint32_t a_x[8] = {1, 2, 3, 4, 5, 6, 7, 8}, a_s[2] = {3, th::ABSENT}, b_x[8] = {11, 12, 13, 14, 15, 16, 17, 18}, b_s[2] = {1, 2};
    th::fold_frames_unique(xyvv, tile_w, slot_w, 1, 2, b_x, b_s);
    th::fold_frames_unique(xyvv, tile_w, slot_w, 0, 2, a_x, a_s);
    EXPECT(tile_w[0] == 1u && slot_w[0] == 1u && xyvv[0] == 11u && tile_w[1] == 1u && xyvv[7] == 18u);
}

static void check_checks() {
    uint32_t t[2] = {0, 0}, s[2] = {0, 0};
    float p[4] = {0, 0, 0, 0};
    const sphx_multi_track_out full{t, s, p, p, p}, none{nullptr, nullptr, nullptr, nullptr, nullptr}, no_tile{nullptr, s, p, p, p}, no_pos{t, s, nullptr, p, p};
    const sphx_multi_track_out only_pos{nullptr, nullptr, p, nullptr, nullptr};
    EXPECT(th::merge_error(2, &full, 1, nullptr) != nullptr);
    EXPECT(th::merge_error(2, &full, 1, &none) != nullptr);
    EXPECT(th::merge_error(2, nullptr, 1, &full) != nullptr);
    EXPECT(th::merge_error(2, &no_tile, 1, &full) != nullptr);
    EXPECT(th::merge_error(2, &no_pos, 1, &full) != nullptr);
    EXPECT(th::merge_error(2, &no_pos, 1, &no_pos) == nullptr);
    EXPECT(th::merge_error(2, &full, 1, &only_pos) == nullptr);
    EXPECT(th::merge_error(2, nullptr, 0, &full) == nullptr);
    const float* fp[1] = {p};
    const uint32_t* tp[1] = {t};
    const float* fnull[1] = {nullptr};
    EXPECT(th::merge_frames_error(1, fp, tp, 1, nullptr) != nullptr);
    EXPECT(th::merge_frames_error(1, nullptr, tp, 1, p) != nullptr);
    EXPECT(th::merge_frames_error(1, fnull, tp, 1, p) != nullptr);
    EXPECT(th::merge_frames_error(0, nullptr, nullptr, 0, nullptr) == nullptr);
    EXPECT(th::merge_frames_error(1, fp, tp, 1, p) == nullptr);
}

int main(int argc, char** argv) {
    const std::string c = argc > 1 ? argv[1] : "";
    if (c == "random") check_random();
    else if (c == "empty") check_empty();
    else if (c == "absent") check_absent();
    else if (c == "two") check_two();
    else if (c == "scatter") check_scatter();
    else if (c == "capacity") check_capacity();
    else if (c == "nanbits") check_nanbits();
    else if (c == "frames") check_frames();
    else if (c == "checks") check_checks();
    else {
        std::printf("usage: track_merge_driver random|empty|absent|two|scatter|capacity|nanbits|frames|checks\n");
        return 2;
    }
    std::printf("ok %ld\n", g_checks);
    return 0;
}
