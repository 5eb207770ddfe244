// sphx_xcd.hpp — the XCD-aware workgroup -> particle-block mapping (xcd_bid in sphx_kernels.hip), its chunk-shift clamp and the
// packing of direction + shift that the scatter and the gather receive as one kernel argument.  Shared by the kernels, the host
// side (sphx_launch.inc) and the exhaustive host test (tests/test_block_mapping.py): ONE definition, plain C++ as well as HIP.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define SPHX_XCD_FN __host__ __device__ __forceinline__
#else
#define SPHX_XCD_FN inline
#endif

namespace sphx {

// Largest chunk shift (log2 of the chunk length in blocks).  xcd_map shifts 32-bit operands by shift + 3: anything at or above 29 is
// undefined; 20 (2^20 blocks per chunk) is already far beyond the largest grid a context can launch (2^28 slots / 256 = 2^20 blocks),
// where the mapping is the contiguous-eighths one anyway.
constexpr int XCD_SHIFT_MAX = 20;
SPHX_XCD_FN uint32_t xcd_shift_clamp(int s) { return s < 0 ? 0u : s > XCD_SHIFT_MAX ? (uint32_t)XCD_SHIFT_MAX : (uint32_t)s; }

// Block `block` of a grid of `grid` workgroups (a multiple of 8) -> the particle block it works on.  A bijection of [0, grid).
// rev: sweep from the top down.  shift: log2 of the chunk length in blocks; 0 — XCD x owns the x-th contiguous eighth; otherwise
// XCD x owns every eighth chunk of 2^shift blocks, and a last, shorter group of chunks of r = per mod 2^shift blocks each is dealt
// like eighths (so a grid of fewer than 8 << shift blocks gets the contiguous-eighths map).
SPHX_XCD_FN uint32_t xcd_map(uint32_t block, uint32_t grid, uint32_t rev, uint32_t shift) {
    const uint32_t per = grid >> 3, q0 = block >> 3, x = block & 7u;
    const uint32_t q = rev ? per - 1u - q0 : q0;
    if (shift == 0u) return x * per + q;
    const uint32_t full = per >> shift, g = q >> shift;
    if (g < full) return (g << (shift + 3u)) + (x << shift) + (q - (g << shift));
    const uint32_t r = per - (full << shift);  // the last, shorter group of chunks
    return (full << (shift + 3u)) + x * r + (q - (full << shift));
}

// Direction and chunk shift in one kernel argument: bit 0 the direction, bits 8 and up the shift.
SPHX_XCD_FN uint32_t xcd_pack(uint32_t rev, uint32_t shift) { return (rev & 1u) | (shift << 8); }
SPHX_XCD_FN uint32_t xcd_packed_rev(uint32_t packed) { return packed & 1u; }
SPHX_XCD_FN uint32_t xcd_packed_shift(uint32_t packed) { return packed >> 8; }
// The scatter's blocks hold 1 024 particles (256 lanes x SCATTER_PER_LANE = 4): its chunks are 4x shorter in blocks, so that one
// chunk covers the particles of one chunk of the 256-particle kernels.
SPHX_XCD_FN uint32_t xcd_scatter_shift(uint32_t shift) { return shift > 2u ? shift - 2u : 0u; }
SPHX_XCD_FN uint32_t xcd_scatter_pack(uint32_t rev, uint32_t shift) { return xcd_pack(rev, xcd_scatter_shift(shift)); }

}  // namespace sphx
