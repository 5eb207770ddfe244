// query_merge_driver.cpp — stand-alone program over csrc/sphx_query_merge.hpp (no HIP, no library): tests/test_query_multi_host.py writes
// a case file (parts in the full or the compact form), this program folds it with sphx_query_host::merge into arrays that end in guard
// words and writes everything back; the test compares with its numpy restatement of the fold.  Built with the sanitizers.
//   query_merge_driver IN OUT
// IN  (64-bit words unless said): m, n_parts, cap, want_entries; per part: compact, n, total, rank, held, n_map, then point[n] (u32,
//      compact only), offset[n + 1 - compact] (u64), tile[n] (i32, full only), nearest_id / nearest_slot / nearest_d2 [n] (u32),
//      id / d2 / slot [held] (u32, if want_entries), id_map[n_map] (u32)
// OUT (64-bit words): rc, count, offsets[m + 1]; then u32: tile[m], nearest_id[m], nearest_slot[m], nearest_d2[m] and, if
//      want_entries, id / d2 / slot [cap + GUARD] each
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sphx_query_merge.hpp"

namespace qh = sphx_query_host;
static constexpr size_t GUARD = 8;
static constexpr uint32_t GUARD_WORD = 0xDEADBEEFu;

template <class T>
static std::vector<T> rd(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && std::fread(v.data(), sizeof(T), n, f) != n) {
        std::fprintf(stderr, "short case file\n");
        std::exit(2);
    }
    return v;
}
template <class T>
static void wr(FILE* f, const std::vector<T>& v) {
    if (!v.empty() && std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) std::exit(3);
}

struct Held {
    std::vector<uint32_t> point, near_id, near_slot, near_d2, id, d2, slot, map;
    std::vector<uint64_t> offset;
    std::vector<int32_t> tile;
};

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    const auto head = rd<uint64_t>(in, 4);
    const uint32_t m = (uint32_t)head[0], n_parts = (uint32_t)head[1];
    const uint64_t cap = head[2];
    const bool entries = head[3] != 0;
    std::vector<Held> held(n_parts);
    std::vector<qh::Part> parts(n_parts);
    for (uint32_t p = 0; p < n_parts; ++p) {
        const auto h = rd<uint64_t>(in, 6);
        const bool compact = h[0] != 0;
        const size_t n = (size_t)h[1];
        Held& s = held[p];
        if (compact) s.point = rd<uint32_t>(in, n);
        s.offset = rd<uint64_t>(in, n + (compact ? 0 : 1));
        if (!compact) s.tile = rd<int32_t>(in, n);
        s.near_id = rd<uint32_t>(in, n);
        s.near_slot = rd<uint32_t>(in, n);
        s.near_d2 = rd<uint32_t>(in, n);
        if (entries) {
            s.id = rd<uint32_t>(in, (size_t)h[4]);
            s.d2 = rd<uint32_t>(in, (size_t)h[4]);
            s.slot = rd<uint32_t>(in, (size_t)h[4]);
        }
        s.map = rd<uint32_t>(in, (size_t)h[5]);
        qh::Part& q = parts[p];
        q.point = compact ? s.point.data() : nullptr;
        q.n = (uint32_t)n;
        q.offset = s.offset.data();
        q.total = h[2];
        q.tile = compact ? nullptr : s.tile.data();
        q.rank = (int32_t)h[3];
        q.nearest_id = s.near_id.data();
        q.nearest_slot = s.near_slot.data();
        q.nearest_d2 = s.near_d2.data();
        if (entries) q.id = s.id.data(), q.d2 = s.d2.data(), q.slot = s.slot.data();
        q.held = h[4];
        q.id_map = h[5] ? s.map.data() : nullptr;
        q.id_map_n = (uint32_t)h[5];
    }
    std::fclose(in);

    // exactly sized heap arrays: the sanitizer sees a write one word behind any of them; the guard words catch one inside
    std::vector<uint64_t> offsets((size_t)m + 1, ~0ull), count(1, ~0ull);
    std::vector<uint32_t> near_id(m, GUARD_WORD), near_slot(m, GUARD_WORD), near_d2(m, GUARD_WORD);
    std::vector<int32_t> tile(m, -7);
    std::vector<uint32_t> id, d2, slot;
    if (entries) id.assign((size_t)cap + GUARD, GUARD_WORD), d2 = id, slot = id;
    qh::Out out;
    out.offsets = offsets.data();
    out.count = count.data();
    out.nearest_id = near_id.data();
    out.nearest_slot = near_slot.data();
    out.nearest_d2 = near_d2.data();
    out.tile = tile.data();
    if (entries) out.id = id.data(), out.d2 = d2.data(), out.slot = slot.data();
    out.cap = cap;
    const int rc = qh::merge(m, parts.data(), n_parts, out);

    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    wr(o, std::vector<uint64_t>{(uint64_t)rc, count[0]});
    wr(o, offsets);
    wr(o, std::vector<uint32_t>(tile.begin(), tile.end()));
    wr(o, near_id);
    wr(o, near_slot);
    wr(o, near_d2);
    wr(o, id);
    wr(o, d2);
    wr(o, slot);
    std::fclose(o);
    std::printf("ok %u %u\n", m, n_parts);
    return 0;
}
