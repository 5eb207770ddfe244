// Stand-alone driver for the gauge rule (yasph2d_amd/csrc/sphx_gauge_rule.hpp): plain C++, compiled by tests/test_gauge_host.py with the
// address and undefined-behaviour sanitizers (any report aborts the program) and without value-changing floating-point options.
//   gauge_rule_driver IN OUT
// IN:  uint32 n_gauges, float iso, n_gauges x sphx_gauge (32 bytes each), then the values (float32, gauges[k].n per gauge).
// OUT: n_gauges x sphx_gauge_rec as sphx_gauge_host::reduce wrote them.  Prints "rc <status>" and returns 0; 2 on a malformed file.
// The value and record arrays are heap blocks of exactly the needed size, so a read or write behind either is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sphx_gauge_rule.hpp"

static bool read_all(const char* path, std::vector<unsigned char>& out) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    unsigned char buf[4096];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) out.insert(out.end(), buf, buf + n);
    std::fclose(f);
    return true;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::vector<unsigned char> in;
    if (!read_all(argv[1], in) || in.size() < 8) return 2;
    uint32_t n_gauges;
    float iso;
    std::memcpy(&n_gauges, in.data(), 4);
    std::memcpy(&iso, in.data() + 4, 4);
    if (n_gauges > 4096u || in.size() < 8 + (size_t)n_gauges * sizeof(sphx_gauge)) return 2;
    std::vector<sphx_gauge> gauges(n_gauges);
    if (n_gauges) std::memcpy(gauges.data(), in.data() + 8, (size_t)n_gauges * sizeof(sphx_gauge));
    const size_t at = 8 + (size_t)n_gauges * sizeof(sphx_gauge);
    if ((in.size() - at) % 4) return 2;
    const size_t n_values = (in.size() - at) / 4;
    uint64_t total;
    if (!sphx_gauge_host::check(gauges.data(), n_gauges, iso, &total) && total != n_values) return 2;  // (a valid table reads `total` values)
    float* values = n_values ? (float*)std::malloc(n_values * 4) : nullptr;
    if (n_values) std::memcpy(values, in.data() + at, n_values * 4);
    sphx_gauge_rec* out = n_gauges ? (sphx_gauge_rec*)std::malloc((size_t)n_gauges * sizeof(sphx_gauge_rec)) : nullptr;
    if (n_gauges) std::memset(out, 0xAB, (size_t)n_gauges * sizeof(sphx_gauge_rec));
    sphx_gauge_rec none;
    const int rc = sphx_gauge_host::reduce(values, gauges.data(), n_gauges, iso, n_gauges ? out : &none);
    std::printf("rc %d\n", rc);
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    if (n_gauges) std::fwrite(out, sizeof(sphx_gauge_rec), n_gauges, f);
    std::fclose(f);
    std::free(values);
    std::free(out);
    return 0;
}
