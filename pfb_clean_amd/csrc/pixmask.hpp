// pixmask.hpp -- the mask pass that comps.hip (fit_image_cube) and spi.hip (fit_spi) open with, and its work layout
// [mask: one 64-bit word per 64 pixels | per-workgroup counts, scanned in place, nblocks + 1 int64
//  | with a maximum: per-workgroup maxima, nblocks doubles | the maximum], which k_comps_compact (comps.hip) reads:
//   load_own      a lane's V pixels of one plane; PEEL: for planes off the 16-byte grid, shifted in from the lane below
//   k_pixmask     one streaming pass over the cube(s) of a Rule: one bit per pixel, the set bits per workgroup and,
//                 if the rule tracks one, the workgroup's NaN-propagating maximum
//   k_count_scan  exclusive scan of the workgroup counts, the total behind them, the maximum of the maxima
//   pixmask_run   the host side of both: argument checks, aligned or PEEL form, the two launches
// A Rule is a small struct, passed to the kernel by value, that states the per-pixel logic:
//   NCUBE                    cubes of (nplane, npix) it reads, 1 or 2
//   START                    a pixel's flag before the first plane
//   x = value(e0, e1)        what one plane contributes, from the pixel's element of the first and of the last cube
//   flag = update(flag, x)   ... and how it changes the flag
//   HAS_MAX                  keep the maximum of x (a double) over all planes and in-range pixels, NaN if any x is
//   UNROLL_ITS, PLANE_UNROLL full unrolling of a wave's iterations, unroll count of the plane loop
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
constexpr int CP_SCAN_BLOCK = 256;

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

// The lane's own V pixels [pix, pix + V) of one plane; elements at or beyond npix are 0.
// PEEL = false: plane + pix is on a 16-byte boundary and pix + V <= npix whenever pix < npix.
// PEEL = true: the plane starts a elements past a boundary, so its aligned vectors begin at pixel h = (V - a) mod V
// (wave-uniform).  A lane loads the vector h pixels AFTER its own; its first h pixels are the last h elements of the
// vector of the lane below (lane 0 reads them one by one).  A vector that would straddle npix is read by element.
// Every lane of the wave must call this (shuffles).
template <int H, typename T, int V>
__device__ __forceinline__ Pack<T, V> shift_in(const Pack<T, V>& v, const Pack<T, V>& below) {
    Pack<T, V> own;
#pragma unroll
    for (int k = 0; k < V; ++k) own.e[k] = k >= H ? v.e[k >= H ? k - H : 0] : below.e[k < H ? V - H + k : 0];
    return own;
}

template <typename T, int V, bool PEEL>
__device__ __forceinline__ Pack<T, V> load_own(const T* __restrict__ plane, size_t pix, size_t npix, int h, int lane) {
    Pack<T, V> v;
#pragma unroll
    for (int k = 0; k < V; ++k) v.e[k] = (T)0;
    if constexpr (!PEEL) {
        if (pix < npix) v = ld_nt<T, V>(plane, pix / V);
        return v;
    } else {
        const size_t p0 = pix + h;
        if (p0 + V <= npix) {
            v = ld_nt<T, V>(plane + h, pix / V);
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k)
                if (p0 + k < npix) v.e[k] = plane[p0 + k];
        }
        if (h == 0) return v;
        Pack<T, V> below;
#pragma unroll
        for (int k = 0; k < V; ++k) below.e[k] = __shfl_up(v.e[k], 1, 64);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < V; ++k) {
                // below.e[V - h + k] is pixel pix + k, k < h
                const int kk = k - (V - h);
                below.e[k] = (kk >= 0 && pix + kk < npix) ? plane[pix + kk] : (T)0;
            }
        }
        if constexpr (V == 2) {
            return shift_in<1>(v, below);
        } else {
            return h == 1 ? shift_in<1>(v, below) : h == 2 ? shift_in<2>(v, below) : shift_in<3>(v, below);
        }
    }
}

// Workgroup g owns mask words [64 g, 64 g + 64), wave w of it the 16 words from 64 g + 16 w.  A lane holds V consecutive
// pixels (V = 16 bytes of T), so one iteration of a wave covers V words.  The aligned form needs every plane of every
// cube on a 16-byte boundary (then npix % V == 0 and no vector straddles npix); PEEL takes the rest, each plane of each
// cube with its own head.  counts[g] = set bits of the workgroup's words, maxpart[g] = the workgroup's maximum.
template <typename T, int V, bool PEEL, typename Rule>
__global__ void __launch_bounds__(CP_BLOCK)
k_pixmask(const Rule rule, const T* __restrict__ c0, const T* __restrict__ c1, int nplane, size_t npix, size_t nwords,
          u64* __restrict__ mask, i64* __restrict__ counts, double* __restrict__ maxpart) {
    constexpr int NC = Rule::NCUBE;
    constexpr int IT_UNROLL = Rule::UNROLL_ITS ? CP_WAVE_WORDS / V : 1;
    constexpr int PLANE_UNROLL = PEEL ? 1 : Rule::PLANE_UNROLL;  // the shuffles do not unroll at a run-time count
    __shared__ int cnt[CP_WAVES];
    __shared__ double wmax[CP_WAVES];
    __shared__ int wnan[CP_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t w0 = (size_t)blockIdx.x * CP_WORDS + (size_t)wave * CP_WAVE_WORDS;
    const T* const cube[2] = {c0, c1};
    unsigned a[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) a[q] = (unsigned)((reinterpret_cast<uintptr_t>(cube[q]) / sizeof(T)) % V);
    const unsigned step = (unsigned)(npix % V);
    int c = 0;
    double mx = -INFINITY;
    bool nan = false;
#pragma unroll IT_UNROLL
    for (int it = 0; it < CP_WAVE_WORDS / V; ++it) {
        const size_t wbase = w0 + (size_t)it * V;
        const size_t pix = wbase * 64 + (size_t)lane * V;
        bool flag[V];
#pragma unroll
        for (int k = 0; k < V; ++k) flag[k] = Rule::START && pix + k < npix;
        // load_own shuffles under PEEL, so the test is wave-uniform.  An aligned form that unrolls its planes tests the
        // lane here instead: with the test left to load_own the loop does not unroll (23 instead of 52 VGPRs); one
        // that keeps them rolled measured 2 % slower that way
        if ((!PEEL && PLANE_UNROLL > 1) ? pix < npix : wbase * 64 < npix) {
#pragma unroll PLANE_UNROLL
            for (int p = 0; p < nplane; ++p) {
                Pack<T, V> v[NC];
#pragma unroll
                for (int q = 0; q < NC; ++q) {
                    const int h = PEEL ? (int)((V - (a[q] + p * step) % V) % V) : 0;
                    v[q] = load_own<T, V, PEEL>(cube[q] + (size_t)p * npix, pix, npix, h, lane);
                }
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const auto x = rule.value(v[0].e[k], v[NC - 1].e[k]);
                    flag[k] = rule.update(flag[k], x);
                    if constexpr (Rule::HAS_MAX) {
                        const bool in = pix + k < npix;
                        nan = nan || (in && x != x);
                        mx = (in && x > mx) ? x : mx;
                    }
                }
            }
        }
        u64 b[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            b[k] = __ballot(flag[k]);
            c += __popcll(b[k]);
        }
        if (lane < V && wbase + lane < nwords) mask[wbase + lane] = mask_word<V>(b, lane);
    }
    if constexpr (Rule::HAS_MAX) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double o = __shfl_down(mx, off, 64);
            mx = o > mx ? o : mx;
        }
        const bool anynan = __ballot(nan) != 0;
        if (lane == 0) {
            wmax[wave] = mx;
            wnan[wave] = anynan;
        }
    }
    if (lane == 0) cnt[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0, n = 0;
        double m = -INFINITY;
#pragma unroll
        for (int w = 0; w < CP_WAVES; ++w) {
            s += cnt[w];
            if constexpr (Rule::HAS_MAX) {
                n |= wnan[w];
                m = wmax[w] > m ? wmax[w] : m;
            }
        }
        counts[blockIdx.x] = s;
        if constexpr (Rule::HAS_MAX) maxpart[blockIdx.x] = n ? (double)NAN : m;
    }
}

// one workgroup: offs[g] <- sum_{h < g} offs[h] in place, offs[n] <- the total; WITH_MAX: *mxout <- max of
// maxpart[0 .. n), NaN if any of them is
template <bool WITH_MAX>
__global__ void __launch_bounds__(CP_SCAN_BLOCK)
k_count_scan(i64* __restrict__ offs, const double* __restrict__ maxpart, int n, double* __restrict__ mxout) {
    __shared__ i64 wsum[CP_SCAN_BLOCK / 64];
    __shared__ double wmax[CP_SCAN_BLOCK / 64];
    __shared__ int wnan[CP_SCAN_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    i64 carry = 0;
    double mx = -INFINITY;
    bool nan = false;
    for (int base = 0; base < n; base += CP_SCAN_BLOCK) {
        const int i = base + threadIdx.x;
        const i64 c = i < n ? offs[i] : 0;
        if constexpr (WITH_MAX) {
            if (i < n) {
                const double m = maxpart[i];
                nan = nan || (m != m);
                mx = m > mx ? m : mx;
            }
        }
        i64 inc = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const i64 t = __shfl_up(inc, off, 64);
            if (lane >= off) inc += t;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        i64 before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < CP_SCAN_BLOCK / 64; ++w) {
            const i64 s = wsum[w];
            if (w < wave) before += s;
            total += s;
        }
        if (i < n) offs[i] = carry + before + inc - c;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) offs[n] = carry;
    if constexpr (WITH_MAX) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double o = __shfl_down(mx, off, 64);
            mx = o > mx ? o : mx;
        }
        const bool anynan = __ballot(nan) != 0;
        if (lane == 0) {
            wmax[wave] = mx;
            wnan[wave] = anynan;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int nn = 0;
            double m = -INFINITY;
#pragma unroll
            for (int w = 0; w < CP_SCAN_BLOCK / 64; ++w) {
                nn |= wnan[w];
                m = wmax[w] > m ? wmax[w] : m;
            }
            *mxout = nn ? (double)NAN : m;
        }
    }
}

template <typename T, typename Rule>
static void pixmask_launch(const Rule& rule, const void* c0, const void* c1, int nplane, size_t npix, u64* mask,
                           i64* offs, double* maxpart, hipStream_t st) {
    constexpr int V = V16<T>::N;
    const dim3 grid((unsigned)comps_nblocks(npix)), block(CP_BLOCK);
    // every plane of every cube starts on a 16-byte boundary
    if (aligned16(c0) && aligned16(c1) && (npix * sizeof(T)) % 16 == 0)
        hipLaunchKernelGGL((k_pixmask<T, V, false, Rule>), grid, block, 0, st, rule, (const T*)c0, (const T*)c1, nplane,
                           npix, comps_nwords(npix), mask, offs, maxpart);
    else
        hipLaunchKernelGGL((k_pixmask<T, V, true, Rule>), grid, block, 0, st, rule, (const T*)c0, (const T*)c1, nplane,
                           npix, comps_nwords(npix), mask, offs, maxpart);
}

// What pfb_comps_mask and pfb_spi_mask do, `who` being the caller's name in the messages: the checks, the mask pass in
// its aligned or PEEL form, the scan.  c1 is null for a rule of one cube.
template <typename Rule>
static int pixmask_run(const char* who, const Rule& rule, int max_planes, int dtype, const void* c0, const void* c1,
                       int nplane, size_t npix, void* work, void* stream) {
    PFB_REQUIRE(c0 && (c1 || Rule::NCUBE == 1) && work, PFB_ERR_INVALID, "%s: null argument", who);
    PFB_REQUIRE(dtype == PFB_F32 || dtype == PFB_F64, PFB_ERR_INVALID, "%s: bad dtype %d", who, dtype);
    PFB_REQUIRE(nplane >= 1 && npix >= 1 && npix <= CP_MAX_PIX, PFB_ERR_INVALID,
                "%s: nplane %d / npix %zu out of range", who, nplane, npix);
    PFB_REQUIRE(nplane <= max_planes, PFB_ERR_UNSUPPORTED, "%s: %d planes beyond the supported %d", who, nplane,
                max_planes);
    PFB_REQUIRE(((uintptr_t)work & 7u) == 0, PFB_ERR_INVALID, "%s: work must be 8-byte aligned", who);
    const unsigned el = dtype == PFB_F32 ? 4 : 8;
    PFB_REQUIRE((uintptr_t)c0 % el == 0 && (uintptr_t)c1 % el == 0, PFB_ERR_INVALID,
                "%s: a cube is not aligned to its element size", who);
    hipStream_t st = as_stream(stream);
    const size_t nblocks = comps_nblocks(npix);
    u64* mask = (u64*)work;
    i64* offs = (i64*)work + comps_nwords(npix);
    double* maxpart = Rule::HAS_MAX ? (double*)(offs + nblocks + 1) : nullptr;
    if (dtype == PFB_F32) pixmask_launch<float>(rule, c0, c1, nplane, npix, mask, offs, maxpart, st);
    else                  pixmask_launch<double>(rule, c0, c1, nplane, npix, mask, offs, maxpart, st);
    hipLaunchKernelGGL(k_count_scan<Rule::HAS_MAX>, dim3(1), dim3(CP_SCAN_BLOCK), 0, st, offs, maxpart, (int)nblocks,
                       Rule::HAS_MAX ? maxpart + nblocks : nullptr);
    PFB_HIP_CHECK(hipGetLastError());
    return PFB_OK;
}

}  // namespace pfb
