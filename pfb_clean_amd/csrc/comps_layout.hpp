// comps_layout.hpp -- the bit-mask work layout that the mask passes of comps.hip and spi.hip write and k_comps_compact
// reads: [mask: one 64-bit word per 64 pixels | per-workgroup counts, scanned in place, nblocks + 1 int64].
#pragma once
#include "common.hpp"

namespace pfb {

typedef unsigned long long u64;
typedef long long i64;

constexpr int CP_BLOCK = 256;
constexpr int CP_WAVES = CP_BLOCK / 64;
// mask words (of 64 pixels) per wave.  Measured on 4096^2 x 8 fp32 with non-temporal loads (the cube is read once
// and is larger than the Infinity Cache): 4 / 8 / 16 / 32 words stream 4.7 / 5.4 / 5.7 / 5.3 TB/s; with plain loads
// 4.1 / 4.8 / 4.9 / 4.6
constexpr int CP_WAVE_WORDS = 16;
constexpr int CP_WORDS = CP_WAVES * CP_WAVE_WORDS;          // ... and per workgroup: 4096 pixels

// bit i of x -> bit 4 i (16 bits in) / bit 2 i (32 bits in)
__device__ __forceinline__ u64 spread4(u64 x) {
    x &= 0xFFFFull;
    x = (x | (x << 24)) & 0x000000FF000000FFull;
    x = (x | (x << 12)) & 0x000F000F000F000Full;
    x = (x | (x << 6)) & 0x0303030303030303ull;
    x = (x | (x << 3)) & 0x1111111111111111ull;
    return x;
}
__device__ __forceinline__ u64 spread2(u64 x) {
    x &= 0xFFFFFFFFull;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}

// Word j < V of the 64 V pixels whose flags the V ballots hold (ballot k: element k of every lane): bit V i + k of the
// word is bit 64 j / V + i of ballot k
template <int V>
__device__ __forceinline__ u64 mask_word(const u64 (&b)[V], int j) {
    static_assert(V == 2 || V == 4, "16-byte packs of double or float");
    if constexpr (V == 2) {
        return spread2(b[0] >> (32 * j)) | (spread2(b[1] >> (32 * j)) << 1);
    } else {
        return spread4(b[0] >> (16 * j)) | (spread4(b[1] >> (16 * j)) << 1) | (spread4(b[2] >> (16 * j)) << 2) |
               (spread4(b[3] >> (16 * j)) << 3);
    }
}

static inline size_t comps_nwords(size_t npix) { return (npix + 63) / 64; }
static inline size_t comps_nblocks(size_t npix) { return (comps_nwords(npix) + CP_WORDS - 1) / CP_WORDS; }
constexpr size_t CP_MAX_PIX = (size_t)1 << 40;              // 2^28 workgroups

}  // namespace pfb
