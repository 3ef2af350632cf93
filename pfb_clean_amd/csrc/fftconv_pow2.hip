// fftconv_pow2.hip -- the fast PSF-convolution path: images whose axes are 2^k, 3 2^k or 5 2^k long with the
// standard 2x PSF oversampling (nx_psf = 2 nx, ny_psf = 2 ny; pfb's default
// psf-oversize 2.0, parser/grid.yaml:65-67).  All BASELINE configs take this path.
//
// Lengths.  Columns (nx): 64 .. 8192 (2^k), 96 .. 6144 (3 2^k), 160 .. 5120 (5 2^k).  Rows (ny / 2): 64 .. 8192 (fp64:
// 4096), 96 .. 6144 (fp64: 3072), 80 .. 5120 (fp64: 2560).  The axes mix freely.  The persistent kernels serve
// power-of-two lengths only; a 3 2^k or 5 2^k axis runs the plain kernel of its pass (k_col_pow2, k_col_fwd_pow2,
// k_row_fwd_pow2, k_row_inv_pow2) on a RegFft whose last pass has radix 3 or 5 (fft_pow2.hpp).
//
// Pruned transforms.  A length-2H FFT whose input is zero beyond H splits exactly into
//     A_e = FFT_H(a)            (even output bins)
//     A_o = FFT_H(a .* w_2H^n)  (odd  output bins)
// and the inverse restricted to the first H samples is
//     b = IFFT_H(B_e) + conj(w_2H^n) .* IFFT_H(B_o)
// so neither the zero half of the padded image nor the discarded half of the result
// is ever computed, loaded or stored.  The same identity is used on the packed-real
// row transform (z[n] = x[2n] + i x[2n+1]).
//
// Layout (16-byte blocking).  Frequency columns are grouped NVB at a time (2 for fp32,
// 1 for fp64: NVB complex values = 16 bytes) WITHIN a parity class of the row transform
// (even bins v = 2m, odd bins v = 2m+1), L = ny/2, NBE = ceil((L+1)/NVB), NBO = L/NVB:
//     block b <  NBE : even bins m = NVB b + c   (fp32: the last block holds m = L + a dummy)
//     block b >= NBE : odd  bins m = NVB (b - NBE) + c
//     T[band][b][i][c]                 c < NVB, i < nx        -> blocks of nx*16 B
//     psf_l[band][b][pu][mu][c]        psfhat[2 mu + pu][v(b,c)], mu < H = nx
// so that (measured, tools/micro/piece_bw.hip: 64-B pieces 3.1 TB/s, 128-B pieces
// 5.5 TB/s from HBM) every strided access is a full 128-byte line: 8 rows x 2 columns.
//
// Kernels:
//   k_row_fwd_pow2  G = 8 image rows per workgroup -> X[v]; per parity the bins are
//                   LDS-transposed and written as 128-byte pieces T[b][i0..i0+8)[0..1]
//   k_col_pow2      one block (two columns) per thread group, 16-byte/lane streams:
//                   a -> FFT -> *psf_e -> IFFT, a*w -> FFT -> *psf_o -> IFFT, combine,
//                   store in place; the two columns share barriers (RegFft NV = 2)
//   k_row_inv_pow2  mirror image of row_fwd with the fused epilogue
//                   (1/(PQ wsum), beam, + sigmainv x, <dot_with, out> partials)
// Host side (below the kernels): which variant serves a class and what it needs is stated once -- ColCfg / ColKernels,
// RowFwdK, RowInvK -- and read by the launchers, the LDS-attribute set-up and the table set-up.  An axis is served
// through ONE seam, a record of function pointers (ColPass for nx, RowPass for ny / 2), whichever object owns its classes.
//
// This file is compiled into THREE objects (csrc/Makefile, FLAGS_fftconv_pow2 / _col / _mix).  Everything up to the entry
// blocks at the end of the file -- configuration, kernels, class descriptions, table set-up, launchers: all templates or
// inlines -- is seen by all three; an object holds the kernels its own entry block instantiates and no others:
//   PFB_POW2_PART=1  the fast path's public entry points (pow2_*) and the power-of-two rows
//   PFB_POW2_PART=2  the power-of-two columns, built with LLVM's max-ILP machine scheduler (-mllvm
//                    -amdgpu-sched-strategy=max-ilp).  Their occupancy is pinned by the launch bounds, so the default
//                    occupancy-driven scheduling only costs them instruction-level parallelism: col 0.977 -> 0.904 ms fp32
//                    and 1.152 -> 1.078 ms fp64 at 4096^2; the row kernels LOSE 5-25 % under the same switch, hence the split
//   PFB_POW2_PART=3  the columns and rows of the lengths 3 2^k and 5 2^k (plain kernels; an object of their own: see
//                    ColKernels::all on what a new instantiation does to its object's other kernels)
#include "conv_plan.hpp"
#include "fft_pow2.hpp"
#include <vector>
#include <cstdlib>
#include <type_traits>

namespace pfb {

// ---- diagnostic build (make stamp: -DPFB_STAMP=1 -> libpfb_hip_stamp.so; never in the product): thread 0 of
// every workgroup of the three persistent kernels records the 100 MHz wall clock at its phase boundaries for
// the tiles / items PFB_STAMP_FIRST .. +PFB_STAMP_ITS of its loop; tools/stamp_report.py turns the buffer into
// a per-phase time table.  Layout: buf[((kernel * 1024 + workgroup) * PFB_STAMP_ITS + it) * 16 + slot].
#ifndef PFB_STAMP
#define PFB_STAMP 0
#endif
#if PFB_STAMP
#define PFB_STAMP_ITS 4
#define PFB_STAMP_FIRST 2
static __device__ unsigned long long* g_stamp_buf = nullptr;
#define STAMP(KID, it, slot)                                                                              \
    do {                                                                                                  \
        const unsigned _si = (unsigned)((it) - PFB_STAMP_FIRST);                                          \
        if (threadIdx.x == 0 && g_stamp_buf && _si < PFB_STAMP_ITS && blockIdx.x < 1024)                  \
            g_stamp_buf[(((size_t)(KID) * 1024 + blockIdx.x) * PFB_STAMP_ITS + _si) * 16 + (slot)] = wall_clock64(); \
    } while (0)
#else
#define STAMP(KID, it, slot) do { (void)(it); } while (0)
#endif

// elements per thread: the column kernel favours occupancy (small register arrays, it
// is the HBM-streaming kernel), the row kernels favour few threads per row so that 8
// rows (64-byte transposed pieces) fit one 1024-thread workgroup.
template <typename T> struct FastCfg;
// NVB: frequency columns per block of the T / psf_l layout = columns per 16-byte access
// (2 x complex64, 1 x complex128), so that 8 rows of a block form one 128-byte line.
template <> struct FastCfg<float>  { static constexpr int ECOL = 8; static constexpr int EROWMAX = 32; static constexpr int WCOL = 4; static constexpr int NVB = 2; };
template <> struct FastCfg<double> { static constexpr int ECOL = 8; static constexpr int EROWMAX = 16; static constexpr int WCOL = 2; static constexpr int NVB = 1; };

// Row kernels: one WAVE per image row whenever the row transform fits 64 lanes x E registers
// (E <= 32 fp32 / 16 fp64): the FFT exchanges are then wave-local (no s_barrier, the 8 waves
// of a workgroup drift freely and overlap each other's memory phases) and nothing spills.
// Measured on MI355X at 4096^2 x 8 bands (ms per launch, fwd / inv):
//   E=16 G=8 (16 waves/CU, 128-B pieces): 0.570 / 1.420     E=16 G=4: 0.569 / 1.312
//   E=8  G=4 (32 waves/CU,  64-B pieces): 0.622 / 1.116     E=32 G=8 (wave per row): 0.603 / 1.673
// -> occupancy beats piece size for the latency-bound inverse kernel; the forward kernel
// keeps 8 rows per workgroup (its strided side is the WRITE, full 128-byte lines).
template <typename T, int L, int E, int GMAX> constexpr int row_groups();
// Elements per thread at the lengths 3 2^k and 5 2^k: the odd factor times the radix of the power-of-two passes, so that a
// row is at least 8 threads (the row tiles then have at most 32 rows, which divides every supported nx).
//   3 2^k: 12 (radix-4 passes)      5 2^k: 20 (radix 4), 10 at L = 80 (radix 2)
// Register counts of the alternatives: profiles/mixed_kernel_resources.md.
constexpr int mix_row_e(int L) { return L % 3 == 0 ? 12 : (L >= 160 ? 20 : 10); }
template <typename T, int L, bool INVK> struct RowCfg {
    // fp32 inverse rows: 8 elements per thread, except 16 at L = 4096: 4 rows / 64-byte pieces instead of 2 / 32, operands
    // read in the epilogue (no registers left to prefetch them): 1.054 against 1.188 ms per 2 x 8192^2.  (16 at L = 2048,
    // 8-row tiles with 128-byte pieces: 128 VGPRs + 232 B of scratch, 0.792 against 0.609 ms per 8-band launch.)
    // fp64: 8 elements per thread (the persistent inverse kernel has its own: InvPE)
    static constexpr int EMAX = sizeof(T) == 4 ? (INVK ? (L == 4096 ? 16 : 8) : 16) : 8;
    static constexpr int E = odd_part(L) > 1 ? mix_row_e(L) : (L / 64 < 8) ? 8 : (L / 64 > EMAX ? EMAX : L / 64);
    static constexpr int TPB = L / E;
    static constexpr bool WAVE = TPB <= 64;
    static constexpr int GMAX = INVK ? 4 : 8;
};
constexpr int LDS_MAX = 160 * 1024;       // dynamic LDS a workgroup may ask for (hipFuncAttributeMaxDynamicSharedMemorySize)
constexpr int LDS_BUDGET = 152 * 1024;    // what the row tiles are sized to

// inverse row kernel: second exchange buffer (one barrier per exchange instead of two)
// whenever 2 x G rows fit the LDS
template <typename T, int L> struct InvDb {
    using C = RowCfg<T, L, true>;
    static constexpr int G = row_groups<T, L, C::E, C::GMAX>();
    static constexpr int STRIDE = RegFft<T, L, C::E>::LDS_ELEMS + 4;
    static constexpr bool ON = (size_t)(2 * G * STRIDE + L) * sizeof(cplx<T>) + 384 <= (size_t)LDS_BUDGET;
    static constexpr int OFF = ON ? G * STRIDE : 0;
};

// elements per thread of the column transform: 8, but 16 for fp64 at H = 8192 -- with E = 8 that
// size needs a 1024-thread workgroup (128-VGPR cap) and spilled ~200 bytes per lane: 4.32 -> 3.29 ms
// per 2 bands.  (fp32 at 8192 is the other way round: E = 16 under its 4-waves/SIMD launch bound
// spills 788 bytes, 2.22 -> 3.58 ms, and still 2.66 ms with a 2-waves/SIMD bound and 84 bytes.)
// ... and 4 up to H = 1024 (the plain, non-persistent column kernel): at these sizes a launch is ONE wave of workgroups, each a
// serial chain of four transforms; twice the threads per column halve the chain (1024^2 x 8 fp32: col 93.8 -> 73.2 us,
// 1024^2 x 1: 23.6 -> 18.1, fp64 27.6 -> 24.1; profiles/r03_ab_col_e4_small.md)
constexpr int COL_E4_MAXH = 1024;
// ... and at the lengths 3 2^k / 5 2^k (plain kernel): 12 (radix-4 passes) / 10 (radix 2).  vv, aw and ev are 3 NVB E complex
// registers whatever the type (144 / 120), which is why these run under the two-waves-per-SIMD launch bound
// (col_waves); 24 / 20 elements do not fit 256 registers (profiles/mixed_kernel_resources.md)
constexpr int mix_col_e(int H) { return H % 3 == 0 ? 12 : 10; }
template <typename T, int H> constexpr int ecol() { return odd_part(H) > 1 ? mix_col_e(H) : (H >= 8192 && sizeof(T) == 8) ? 16 : (H <= COL_E4_MAXH && H >= 64 ? 4 : FastCfg<T>::ECOL); }
// waves per SIMD the plain column kernels are bounded to
template <typename T> constexpr int col_waves(int E) { return (E >= 16 || odd_part(E) > 1) ? 2 : FastCfg<T>::WCOL; }

// rows per workgroup for the row kernels
template <typename T, int L, int E, int GMAX>
constexpr int row_groups() {
    constexpr int TPB = L / E;
    int G = 256 / TPB > GMAX ? 256 / TPB : GMAX;
    const int stride = RegFft<T, L, E>::LDS_ELEMS + 4;
    while (G > 1 && (G * TPB > 1024 || (size_t)G * stride * sizeof(cplx<T>) + 384 > LDS_BUDGET)) G /= 2;
    return G;
}
template <int H, int E>
constexpr int col_groups() { return (H / E) >= 256 ? 1 : 256 / (H / E); }
constexpr int ECOLX = 8;      // elements per thread of the two-level column kernel's sub-transforms (k_col_pow2x)

// NVB adjacent complex values as one aligned 16-byte access
template <typename T, int NVB> struct alignas(16) Blk { cplx<T> c[NVB]; };
template <typename T, int NVB>
__device__ __forceinline__ Blk<T, NVB> loadb(const cplx<T>* src) {
    return *reinterpret_cast<const Blk<T, NVB>*>(src);
}
// the same, marked non-temporal (global_load ... nt): for streams that are read exactly once per launch and are far
// larger than the 256 MiB Infinity Cache (the PSF spectrum: 268 MB per 4096^2 fp32 band) -- they should not push
// the half-spectrum T, which the NEXT kernel re-reads, out of it
template <typename T, int NVB>
__device__ __forceinline__ Blk<T, NVB> loadb_nt(const cplx<T>* src) {
    typedef float v4f __attribute__((ext_vector_type(4)));
    static_assert(sizeof(Blk<T, NVB>) == 16, "16-byte blocks");
    const v4f v = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(src));
    Blk<T, NVB> b;
    __builtin_memcpy(&b, &v, 16);
    return b;
}

template <typename T, int NVB>
__device__ __forceinline__ void storeb(cplx<T>* dst, const Blk<T, NVB>& b) {
    *reinterpret_cast<Blk<T, NVB>*>(dst) = b;
}

// Make a pointer opaque to the optimiser: loads through the result cannot be CSE'd with /
// hoisted above earlier loads of the same address (used where a value is deliberately
// RE-READ from L2 instead of being kept live in 32 VGPRs across an FFT).
template <typename P>
__device__ __forceinline__ P* opaque(P* p) {
    asm volatile("" : "+v"(p));
    return p;
}

// LAUNDER_EARLY: see the comment at the row kernels -- values derived from the thread index are loop invariant, and
// the optimiser keeps whatever it can compute from them live across a persistent kernel's whole loop
__device__ __forceinline__ int launder(int v) {
    asm volatile("" : "+v"(v));
    return v;
}

// exp(-2 pi i k / 32) for the kernels that rebuild a long twiddle table from a short one: w^(t + c j) = w^t x (a 32nd root
// of unity that is a compile-time constant once the loop over j is unrolled)
template <typename T>
__device__ __forceinline__ cplx<T> root32(int k) {              // exp(-2 pi i k / 32); folds to constants for constant k
    constexpr T C[9] = {T(1), T(0.98078528040323044912618223613423903697L), T(0.92387953251128675612818318939678828682L),
                        T(0.83146961230254523707878837761790575673L), T(0.70710678118654752440084436210484903928L),
                        T(0.55557023301960222474283081394853287438L), T(0.38268343236508977172845998403039886676L),
                        T(0.19509032201612826784828486847702224093L), T(0)};
    auto cs = [&](int q) -> T {                                 // cos(2 pi q / 32)
        q &= 31;
        return q <= 8 ? C[q] : q <= 16 ? -C[16 - q] : q <= 24 ? -C[q - 16] : C[32 - q];
    };
    return cplx<T>(cs(k), -cs(k - 8));
}

// XCD-aware order of the row groups (plain row kernels: workgroups; persistent ones: tiles of a band).  A group of G rows
// touches T in G x 16-byte pieces; 8 rows make a 128-byte line.  Workgroups are dealt round-robin over the 8 XCDs (blocks
// b and b + 8 share an L2), so the SH = 8 / G row groups of one line are given to blocks b, b + 8, .. b + 8 (SH - 1):
// their pieces meet in ONE L2 and leave it (or are fetched into it) as a full line (speed only: any bijection is
// correct; on whenever the `n` groups are a multiple of 8 SH).
__device__ __forceinline__ int xcd_paired(int rg, int SH) {
    const int q = rg / (8 * SH), rem = rg % (8 * SH);
    return SH * (q * 8 + (rem & 7)) + (rem >> 3);
}
__device__ __forceinline__ int xcd_line_pair(int rg, int n, int SH) {
    return SH > 1 && n % (8 * SH) == 0 ? xcd_paired(rg, SH) : rg;
}
template <int G>
__device__ __forceinline__ int xcd_row_group(int bx, int nbx) { return xcd_line_pair(bx, nbx, 8 / G); }

struct FastDims {
    int nx, ny, M;              // M = ny (packed length), nv = M + 1 columns
    size_t T_band, psf_band;
    size_t xpitch, xband;       // forward row kernels: elements between rows / bands of x and beam (ny, nx ny for
                                // an image cube; the PSFHAT producer reads quadrants of the (P, Q) PSF: pitch Q)
};

// ---------------------------------------------------------------- psfhat re-layout
// blocks of the even bins (m <= L: L + 1 of them) and of the odd bins (m < L) of a half spectrum of L + 1 + L columns
__host__ __device__ constexpr int nblocks_even(int L, int nvb) { return (L + nvb) / nvb; }
__host__ __device__ constexpr int nblocks_odd(int L, int nvb) { return L / nvb; }
// column v of the half spectrum -> (block, slot) of the pair layout
__host__ __device__ inline void block_of_bin(int v, int L, int nvb, int* blk, int* c) {
    const int m = v >> 1;
    const int nbe = nblocks_even(L, nvb);
    *blk = ((v & 1) ? nbe : 0) + m / nvb;
    *c = m % nvb;
}
inline int fast_nblocks(int L, int nvb) { return nblocks_even(L, nvb) + nblocks_odd(L, nvb); }
// element offset of psfhat[u][v(blk, c)] inside a band of psf_l (H = nx = P / 2 rows per parity).
//   four = 0: parity-major  psf_l[blk][u & 1][u >> 1][c]     (k_col_pow2, k_col_pow2p)
//   four = 1: class-major   psf_l[blk][u & 3][u >> 2][c]     (k_col_pow2x: the two-level column transform)
__host__ __device__ inline size_t psf_off(int blk, int u, int c, int H, int nvb, int four) {
    return four ? (((size_t)blk * 4 + (u & 3)) * (size_t)(H / 2) + (u >> 2)) * nvb + c
                : (((size_t)blk * 2 + (u & 1)) * (size_t)H + (u >> 1)) * nvb + c;
}

// psf_l[band][blk][pu][mu][c] = psfhat[band][2 mu + pu][v]
template <typename T>
__global__ void k_relayout_psf_pow2(const cplx<T>* __restrict__ psfhat, cplx<T>* __restrict__ psf_l,
                                    int P, int nv, int L, int nvb, size_t psf_band, int four) {
    // tile transpose through LDS: block handles 32 u x 32 v
    __shared__ cplx<T> tile[32][33];
    const int band = blockIdx.z;
    const int u0 = blockIdx.y * 32, v0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;      // 256 threads: ty < 8
    for (int r = ty; r < 32; r += 8) {
        const int u = u0 + r, v = v0 + tx;
        if (u < P && v < nv) tile[r][tx] = psfhat[((size_t)band * P + u) * nv + v];
    }
    __syncthreads();
    const int H = P / 2;
    for (int r = ty; r < 32; r += 8) {
        const int v = v0 + r, u = u0 + tx;
        if (u < P && v < nv) {
            int blk, c;
            block_of_bin(v, L, nvb, &blk, &c);
            psf_l[(size_t)band * psf_band + psf_off(blk, u, c, H, nvb, four)] = tile[tx][r];
        }
    }
}

// psfhat[band][u][v] = psf_l[band][blk][u & 1][u >> 1][c]: the reference's layout back out of the plan's
template <typename T>
__global__ void k_unrelayout_psf_pow2(const cplx<T>* __restrict__ psf_l, cplx<T>* __restrict__ psfhat,
                                      int P, int nv, int L, int nvb, size_t psf_band, int four) {
    __shared__ cplx<T> tile[32][33];
    const int band = blockIdx.z;
    const int u0 = blockIdx.y * 32, v0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int H = P / 2;
    for (int r = ty; r < 32; r += 8) {
        const int v = v0 + r, u = u0 + tx;
        if (u < P && v < nv) {
            int blk, c;
            block_of_bin(v, L, nvb, &blk, &c);
            tile[tx][r] = psf_l[(size_t)band * psf_band + psf_off(blk, u, c, H, nvb, four)];
        }
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int u = u0 + r, v = v0 + tx;
        if (u < P && v < nv) psfhat[((size_t)band * P + u) * nv + v] = tile[r][tx];
    }
}

// ------------------------------------------------------------------------ column
template <typename T, int H, int E>
__global__ void __launch_bounds__((col_groups<H, E>() * (H / E)), (col_waves<T>(E)))
k_col_pow2(cplx<T>* __restrict__ Tw, const cplx<T>* __restrict__ psf_l,
           const cplx<T>* __restrict__ twP, const cplx<T>* __restrict__ ptw,
           int nblk, size_t T_band, size_t psf_band, int band0) {
    using F = RegFft<T, H, E>;
    constexpr int TPB = F::TPB;
    constexpr int NVB = FastCfg<T>::NVB;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int g = threadIdx.x / TPB, t = threadIdx.x % TPB;
    cplx<T>* lds = reinterpret_cast<cplx<T>*>(smem) + (size_t)g * (NVB * F::LDS_ELEMS);
    const int blk = blockIdx.x * col_groups<H, E>() + g;
    const int band = band0 + blockIdx.y;
    const bool active = blk < nblk;
    const size_t b = active ? blk : 0;
    cplx<T>* col = Tw + (size_t)band * T_band + (b * (size_t)H + t) * NVB;             // [i][c]
    const cplx<T>* pe = psf_l + (size_t)band * psf_band + (b * (2 * (size_t)H) + t) * NVB;
    const cplx<T>* po = pe + (size_t)H * NVB;

    // a is read from HBM exactly once (rocprofv3 FETCH_SIZE showed the former "re-read from
    // L2" going to HBM: +1 GB per 8-band launch).  aw = a .* w_P^n is formed at load time and
    // parked in registers; its live range (first FFT pair) does not overlap ev's (second pair),
    // so the peak register demand is unchanged.
    cplx<T> vv[NVB][E], aw[NVB][E];
    {
        const cplx<T>* tw2 = twP + t;
#pragma unroll
        for (int j = 0; j < E; ++j) {
            Blk<T, NVB> a;
            if (active) a = loadb<T, NVB>(col + NVB * TPB * j);
            const cplx<T> w = tw2[TPB * j];
#pragma unroll
            for (int c = 0; c < NVB; ++c) {
                vv[c][j] = active ? a.c[c] : cplx<T>(0, 0);
                aw[c][j] = vv[c][j] * w;
            }
        }
    }
    // (Requesting psf_e before the first transform and psf_o before the second in the 8192-point fp64 columns: vv + aw + q
    // are 192 registers before the radix-16 butterfly's own 64, 84 -> 556 bytes of scratch per lane.)
    // MIXL: the 3 2^k / 5 2^k columns launder the thread index per transform (LAUNDER_EARLY): with up to ten passes per
    // transform the LDS addresses of all of them, computed once and kept across the four transforms, cost 130 registers
    // (5120-point fp32 columns: 256 VGPRs + 132 B of scratch -> 132 VGPRs).  (Spelled as a branch per call: behind a
    // helper -- a lambda or launder_if<MIXL>(t), both tried -- the power-of-two instantiations of this object compile to a
    // different register allocation and schedule than the one all its measurements were taken with.)
    constexpr bool MIXL = odd_part(H) > 1;
    // ---- even bins of the column transform
    if constexpr (MIXL) F::template runN<false, NVB>(vv, lds, launder(t), ptw);
    else
    F::template runN<false, NVB>(vv, lds, t, ptw);
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const Blk<T, NVB> p = loadb<T, NVB>(pe + NVB * TPB * j);
#pragma unroll
        for (int c = 0; c < NVB; ++c) vv[c][j] = vv[c][j] * p.c[c];
    }
    if constexpr (MIXL) F::template runN<true, NVB>(vv, lds, launder(t), ptw);
    else
    F::template runN<true, NVB>(vv, lds, t, ptw);
    cplx<T> ev[NVB][E];
#pragma unroll
    for (int j = 0; j < E; ++j) {
#pragma unroll
        for (int c = 0; c < NVB; ++c) { ev[c][j] = vv[c][j]; vv[c][j] = aw[c][j]; }
    }
    // ---- odd bins
    if constexpr (MIXL) F::template runN<false, NVB>(vv, lds, launder(t), ptw);
    else
    F::template runN<false, NVB>(vv, lds, t, ptw);
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const Blk<T, NVB> p = loadb<T, NVB>(po + NVB * TPB * j);
#pragma unroll
        for (int c = 0; c < NVB; ++c) vv[c][j] = vv[c][j] * p.c[c];
    }
    if constexpr (MIXL) F::template runN<true, NVB>(vv, lds, launder(t), ptw);
    else
    F::template runN<true, NVB>(vv, lds, t, ptw);
    if (active) {
        const cplx<T>* tw3 = opaque(twP + t);
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const cplx<T> w = tw3[TPB * j];
            Blk<T, NVB> o;
#pragma unroll
            for (int c = 0; c < NVB; ++c) o.c[c] = ev[c][j] + mulc(vv[c][j], w);
            storeb<T, NVB>(col + NVB * TPB * j, o);
        }
    }
}

// --------------------------------------------------- column, persistent + prefetching
// The plain column kernel above is latency bound (rocprofv3: 58 % of wave-cycles parked in
// s_waitcnt / s_barrier, VALU 18 %): every block pays the HBM latency of a, psf_e and psf_o
// one after the other.  This version keeps ONE workgroup per CU resident (256 VGPRs per
// thread), loops over the (band, block) items, and has at all times in flight
//   * psf_e and psf_o of the CURRENT item (issued before the first FFT), and
//   * a (the T block) of the NEXT item,
// so that in steady state no load latency is exposed; the column twiddles w_P^n are
// loaded once per kernel and stay in registers.
// DB: a second set of exchange buffers (when the LDS holds it) -- one barrier per exchange instead of two.
// The loads are not issued in two bursts (top of the trip / after the first FFT) but a few per FFT PASS
// (RegFft pass hook): a burst of 16 x 16-byte loads per thread blocks every wave of the workgroup at issue for ~3.8 us
// of a 16 us trip (profiles/r02_a_phase_stamps_*), with nothing computing meanwhile.  Per trip:
//     FFT (even)   <- first half of the NEXT item's a          multiply by psf_e (requested during the last IFFT)
//     IFFT (even)  <- psf_o of this item
//     FFT (odd)    <- second half of the next item's a         multiply by psf_o
//     IFFT (odd)   <- psf_e of the NEXT item
template <typename T, int H, int E, bool DB, bool NT>
__global__ void __launch_bounds__((col_groups<H, E>() * (H / E)), 2)
k_col_pow2p(cplx<T>* __restrict__ Tw, const cplx<T>* __restrict__ psf_l,
            const cplx<T>* __restrict__ twP, const cplx<T>* __restrict__ ptwc,
            int nblk, int nitems, size_t T_band, size_t psf_band, int band0, int bstep) {
    constexpr int NVB = FastCfg<T>::NVB;
    constexpr int XB = NVB * RegFft<T, H, E>::LDS_ELEMS;  // one set of exchange buffers (elements)
    using F = RegFft<T, H, E, false, DB ? XB : 0, true>;  // twiddles from LDS: no vmcnt wait in the passes
    constexpr int X1 = (DB && (F::template nxch<1>() & 1)) ? 1 : 0;   // start parity of every other transform
    constexpr int TPB = F::TPB;
    constexpr int GC = col_groups<H, E>();
    constexpr int NP = F::NPASS;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int g = threadIdx.x / TPB, t = threadIdx.x % TPB;
    cplx<T>* ltw = reinterpret_cast<cplx<T>*>(smem);
    cplx<T>* lds = ltw + ((F::PTWC + 1) & ~1) + (size_t)g * ((DB ? 2 : 1) * XB);
    const int stride = gridDim.x * GC;
    const int niter = (nitems + stride - 1) / stride;           // same for every workgroup

    cplx<T> tw[E];
#pragma unroll
    for (int j = 0; j < E; ++j) tw[j] = twP[t + TPB * j];
    for (int k = threadIdx.x; k < F::PTWC; k += GC * TPB) ltw[k] = ptwc[k];

    auto col_of = [&](int item) -> cplx<T>* {
        const int bl = item / nblk, blk = item - bl * nblk;
        return Tw + (size_t)(band0 + bstep * bl) * T_band + ((size_t)blk * H + t) * NVB;
    };
    auto psf_of = [&](int item) -> const cplx<T>* {
        const int bl = item / nblk, blk = item - bl * nblk;
        return psf_l + (size_t)(band0 + bstep * bl) * psf_band + ((size_t)blk * 2 * H + t) * NVB;
    };

    auto item_of = [&](int it) -> int { return blockIdx.x * GC + g + it * stride; };
    int item = item_of(0);
    Blk<T, NVB> an[E];
    Blk<T, NVB> q[E];
    {
        const bool act = item < nitems;
        const cplx<T>* c0 = col_of(act ? item : 0);
#pragma unroll
        for (int j = 0; j < E; ++j) {
            if (act) an[j] = loadb<T, NVB>(c0 + NVB * TPB * j);
            else {
#pragma unroll
                for (int c = 0; c < NVB; ++c) an[j].c[c] = cplx<T>(0, 0);
            }
        }
        {
            const cplx<T>* pe0 = psf_of(act ? item : 0);
#pragma unroll
            for (int j = 0; j < E; ++j) q[j] = NT ? loadb_nt<T, NVB>(pe0 + NVB * TPB * j) : loadb<T, NVB>(pe0 + NVB * TPB * j);
        }
    }
    __syncthreads();                                            // twiddle table visible
#pragma unroll 1
    for (int it = 0; it < niter; ++it, item = item_of(it)) {
        STAMP(1, it, 0);
        const bool active = item < nitems;
        cplx<T>* col = col_of(active ? item : 0);
        const cplx<T>* pe = psf_of(active ? item : 0);
        const cplx<T>* po = pe + (size_t)H * NVB;
        // next item (clamped: a trip past the end re-reads a valid block and drops it)
        const int nxt = item_of(it + 1);
        const bool nact = nxt < nitems;
        const cplx<T>* cn = col_of(nact ? nxt : (active ? item : 0));
        const cplx<T>* pen = psf_of(nact ? nxt : (active ? item : 0));
        cplx<T> vv[NVB][E], aw[NVB][E];
#pragma unroll
        for (int j = 0; j < E; ++j) {
#pragma unroll
            for (int c = 0; c < NVB; ++c) { vv[c][j] = an[j].c[c]; aw[c][j] = vv[c][j] * tw[j]; }
        }
        // loads [lo, hi) of a group of CNT, slice k of NP
        auto ld_an = [&](auto k, int base) {
            constexpr int K = decltype(k)::value;
            constexpr int CNT = E / 2;
#pragma unroll
            for (int j = (K * CNT) / NP; j < ((K + 1) * CNT) / NP; ++j)
                an[base + j] = loadb<T, NVB>(cn + NVB * TPB * (base + j));
        };
        STAMP(1, it, 1);
        // ---- even bins
        F::template runN<false, NVB, 0>(vv, lds, t, ltw, [&](auto k) { ld_an(k, 0); });
        STAMP(1, it, 2);
#pragma unroll
        for (int j = 0; j < E; ++j) {
#pragma unroll
            for (int c = 0; c < NVB; ++c) vv[c][j] = vv[c][j] * q[j].c[c];
        }
        STAMP(1, it, 3);
        F::template runN<true, NVB, X1>(vv, lds, t, ltw, [&](auto k) {
            constexpr int K = decltype(k)::value;
#pragma unroll
            for (int j = (K * E) / NP; j < ((K + 1) * E) / NP; ++j) q[j] = NT ? loadb_nt<T, NVB>(po + NVB * TPB * j) : loadb<T, NVB>(po + NVB * TPB * j);
        });
        STAMP(1, it, 4);
        cplx<T> ev[NVB][E];
#pragma unroll
        for (int j = 0; j < E; ++j) {
#pragma unroll
            for (int c = 0; c < NVB; ++c) { ev[c][j] = vv[c][j]; vv[c][j] = aw[c][j]; }
        }
        // ---- odd bins
        F::template runN<false, NVB, 0>(vv, lds, t, ltw, [&](auto k) { ld_an(k, E / 2); });
        STAMP(1, it, 5);
#pragma unroll
        for (int j = 0; j < E; ++j) {
#pragma unroll
            for (int c = 0; c < NVB; ++c) vv[c][j] = vv[c][j] * q[j].c[c];
        }
        STAMP(1, it, 6);
        F::template runN<true, NVB, X1>(vv, lds, t, ltw, [&](auto k) {
            constexpr int K = decltype(k)::value;
#pragma unroll
            for (int j = (K * E) / NP; j < ((K + 1) * E) / NP; ++j) q[j] = NT ? loadb_nt<T, NVB>(pen + NVB * TPB * j) : loadb<T, NVB>(pen + NVB * TPB * j);
        });
        STAMP(1, it, 7);
        if (active) {
#pragma unroll
            for (int j = 0; j < E; ++j) {
                Blk<T, NVB> o;
#pragma unroll
                for (int c = 0; c < NVB; ++c) o.c[c] = ev[c][j] + mulc(vv[c][j], tw[j]);
                storeb<T, NVB>(col + NVB * TPB * j, o);
            }
        }
        STAMP(1, it, 8);
    }
}

// ------------------------------------------- column, two-level (four residue classes), persistent
// Long columns (H = 8192: one 16-byte block of a column is 128 KB, the whole register file of a CU holds four of them)
// do not fit the kernel above: its exchange buffers fill the LDS, the tables do not fit next to them, 1024 threads cap
// the registers at 128 -- the plain kernel then runs one workgroup per CU barrier to barrier with every load latency
// exposed (1.1 TB/s of traffic at 8192^2 fp32 against 5.4 TB/s at 4096^2) and spills.  Here the padded length-4 HS
// transform (H = 2 HS samples, zero beyond) is split by the residue of the output bin modulo 4:
//     X[4m + r] = FFT_HS( (a[n] + (-i)^r a[n + HS]) w_P^(r n) )[m]                      r = 0..3,  n, m < HS
//     b[n + s HS] = sum_r  i^(s r) conj(w_P^(r n)) IFFT_HS( X[4 . + r] psf[4 . + r] )[n]        s = 0, 1
// i.e. FOUR rounds of (combine, FFT_HS, multiply, IFFT_HS, accumulate) on the persistent, spill-free HS-point tile:
// half the threads, half the exchange buffer, and the loads ride inside the transforms (RegFft pass hooks), in issue
// order per trip
//     round r:      IFFT passes  <- psf slice of the NEXT round (last round: class 0 of the next item)
//     rounds 1, 3:  FFT passes   <- upper / lower half of the next item's column (into the registers a just left)
// Rounds run in the order 0, 2, 1, 3: after round 0 both output halves are the same array, two accumulators exist from
// the end of the second round only -- and the upper one lives in the LDS (`park`: the exchange buffer is half the
// usual size), so that at most FIVE arrays of E blocks are live in registers at any time (the 4096-point persistent
// kernel: five).  The twiddles w_P^n, n = t + TPB j, are w_P^t (LDS table of TPB entries) times the compile-time
// constants exp(-2 pi i j / 4E).  The PSF spectrum is stored class-major for this kernel (psf_l[blk][r][m][c] =
// psfhat[4 m + r], see psf_off), so that every slice is a contiguous 16-byte-per-lane stream.
template <typename T, int H, int E>
struct ColX {
    static constexpr int HS = H / 2;
    using F = RegFft<T, HS, E, false, 0, true>;
    static constexpr int NVB = FastCfg<T>::NVB;
    static constexpr int GC = col_groups<HS, E>();
    static constexpr int NT = GC * F::TPB;
    static constexpr int XB = NVB * F::LDS_ELEMS;
    static constexpr int PTWP = (F::PTWC + 1) & ~1;
    static constexpr size_t LDS = sizeof(cplx<T>) * ((size_t)PTWP + F::TPB + (size_t)GC * XB + (size_t)NT * E * NVB);
    static_assert(E == 8, "root32: the twiddle constants are the 4E-th roots of unity");
};

template <typename T, int H, int E, bool NT = false>
__global__ void __launch_bounds__((ColX<T, H, E>::NT), 2)
k_col_pow2x(cplx<T>* __restrict__ Tw, const cplx<T>* __restrict__ psf_l,
            const cplx<T>* __restrict__ twP, const cplx<T>* __restrict__ ptwc,
            int nblk, int nitems, size_t T_band, size_t psf_band, int band0, int bstep) {
    using X = ColX<T, H, E>;
    using F = typename X::F;
    constexpr int NVB = X::NVB, HS = X::HS, TPB = F::TPB, GC = X::GC, NP = F::NPASS, NTH = X::NT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int g = threadIdx.x / TPB, t = threadIdx.x % TPB;
    cplx<T>* ltw = reinterpret_cast<cplx<T>*>(smem);
    cplx<T>* ltx = ltw + X::PTWP;                               // w_P^n, n < TPB
    cplx<T>* lds = ltx + TPB + (size_t)g * X::XB;
    Blk<T, NVB>* park = reinterpret_cast<Blk<T, NVB>*>(ltx + TPB + (size_t)GC * X::XB) + threadIdx.x;   // [j][thread]
    const int stride = gridDim.x * GC;
    const int niter = (nitems + stride - 1) / stride;           // same for every workgroup

    for (int k = threadIdx.x; k < F::PTWC; k += NTH) ltw[k] = ptwc[k];
    for (int k = threadIdx.x; k < TPB; k += NTH) ltx[k] = twP[k];

    auto col_of = [&](int item) -> cplx<T>* {
        const int bl = item / nblk, blk = item - bl * nblk;
        return Tw + (size_t)(band0 + bstep * bl) * T_band + ((size_t)blk * H + t) * NVB;
    };
    auto psf_of = [&](int item) -> const cplx<T>* {             // class 0 of the item; class r: + r HS NVB
        const int bl = item / nblk, blk = item - bl * nblk;
        return psf_l + (size_t)(band0 + bstep * bl) * psf_band + ((size_t)blk * 2 * H + t) * NVB;
    };
    auto ldq = [&](const cplx<T>* p) __attribute__((always_inline)) { return NT ? loadb_nt<T, NVB>(p) : loadb<T, NVB>(p); };

    int item = blockIdx.x * GC + g;
    Blk<T, NVB> al[E], ah[E], q[E];
    {
        const bool act = item < nitems;
        const cplx<T>* c0 = col_of(act ? item : 0);
#pragma unroll
        for (int j = 0; j < E; ++j) {
            al[j] = loadb<T, NVB>(c0 + NVB * TPB * j);
            ah[j] = loadb<T, NVB>(c0 + NVB * (HS + TPB * j));
        }
    }
    __syncthreads();                                            // tables visible
#pragma unroll 1
    for (int it = 0; it < niter; ++it, item += stride) {
        const bool active = item < nitems;
        cplx<T>* col = col_of(active ? item : 0);
        const cplx<T>* ps = psf_of(active ? item : 0);
        const int nxt = item + stride;
        const bool nact = nxt < nitems;                         // a trip past the end re-reads a valid block and drops it
        const cplx<T>* cn = col_of(nact ? nxt : (active ? item : 0));
        cplx<T> vv[NVB][E], ol[NVB][E];
        // w_P^t, laundered at every use: t and the table are loop invariant, and the optimiser would otherwise keep
        // w, w^2, w^3 of all E samples live across the whole item loop
        auto wt = [&]() __attribute__((always_inline)) { return ltx[launder(t)]; };
        auto mulq = [&]() __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < E; ++j) {
#pragma unroll
                for (int c = 0; c < NVB; ++c) vv[c][j] = vv[c][j] * q[j].c[c];
            }
        };
        // PSF slices: the slice of round r is requested inside the FORWARD transform of round r (one transform of
        // lead), not inside the inverse transform of the round before (two): q is then dead across every
        // accumulate / combine step, which is where the registers run out (fp64: 140 B of scratch per lane = 2.35 GB of
        // spill traffic per 2-band launch, a quarter of the kernel's HBM bytes -- profiles/r03_m_c5_hbm_traffic.json)
        auto qslice = [&](auto k, const cplx<T>* pq) __attribute__((always_inline)) {
            constexpr int K = decltype(k)::value;
#pragma unroll
            for (int j = (K * E) / NP; j < ((K + 1) * E) / NP; ++j) q[j] = ldq(pq + NVB * TPB * j);
        };
        auto fft_q = [&](const cplx<T>* pq) __attribute__((always_inline)) {     // forward transform of a round
            F::template runN<false, NVB>(vv, lds, t, ltw, [&](auto k) { qslice(k, pq); });
        };
        auto ifft_q = [&](auto&& extra) __attribute__((always_inline)) {        // inverse transform
            F::template runN<true, NVB>(vv, lds, t, ltw, [&](auto k) { extra(k); });
        };
        auto none = [](auto) {};
        STAMP(1, it, 0);
        // ---- round r = 0:  a_lo + a_hi
#pragma unroll
        for (int j = 0; j < E; ++j) {
#pragma unroll
            for (int c = 0; c < NVB; ++c) vv[c][j] = al[j].c[c] + ah[j].c[c];
        }
        fft_q(ps);
        STAMP(1, it, 1);
        mulq();
        ifft_q(none);
        STAMP(1, it, 2);
#pragma unroll
        for (int j = 0; j < E; ++j) {
#pragma unroll
            for (int c = 0; c < NVB; ++c) ol[c][j] = vv[c][j];
        }
        // ---- round r = 2:  (a_lo - a_hi) w^2n
        {
            const cplx<T> w1 = wt(), wt2 = w1 * w1;
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const cplx<T> w2 = wt2 * root32<T>(2 * j);
#pragma unroll
                for (int c = 0; c < NVB; ++c) vv[c][j] = (al[j].c[c] - ah[j].c[c]) * w2;
            }
        }
        STAMP(1, it, 3);
        fft_q(ps + (size_t)2 * HS * NVB);
        STAMP(1, it, 4);
        mulq();
        ifft_q(none);
        STAMP(1, it, 5);
        {
            const cplx<T> w1 = wt(), wt2 = w1 * w1;
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const cplx<T> w2 = wt2 * root32<T>(2 * j);
                Blk<T, NVB> hi;
#pragma unroll
                for (int c = 0; c < NVB; ++c) {
                    const cplx<T> u = mulc(vv[c][j], w2);
                    hi.c[c] = ol[c][j] - u;
                    ol[c][j] = ol[c][j] + u;
                }
                park[j * NTH] = hi;
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // ---- round r = 1:  (a_lo - i a_hi) w^n.  The input of round 3, (a_lo + i a_hi) w^3n, is formed here as well and
        // parked in a_lo's registers: the column dies one round early and a_hi's registers take the upper half of the
        // next item's column during this round's forward transform
        {
            const cplx<T> w1t = wt(), w3t = w1t * (w1t * w1t);
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const cplx<T> w1 = w1t * root32<T>(j), w3 = w3t * root32<T>(3 * j);
#pragma unroll
                for (int c = 0; c < NVB; ++c) {
                    const cplx<T> lo = al[j].c[c], hi = ah[j].c[c];
                    vv[c][j] = addrot<false>(lo, hi) * w1;
                    al[j].c[c] = addrot<true>(lo, hi) * w3;
                }
                __builtin_amdgcn_sched_barrier(0);          // one sample at a time: the temporaries of all E at once spill
            }
        }
        STAMP(1, it, 6);
        // the next item's column: upper half into a_hi's registers (free since the inputs of rounds 1 and 3 were formed),
        // lower half into a_lo's (free once round 3's input has moved to vv).  The forward transforms of rounds 1 / 3 carry
        // the PSF slices and the column rides in the inverse transforms, so that no transform has more than five arrays
        // of E blocks live.
        auto ld_ah = [&](auto k) __attribute__((always_inline)) {
            constexpr int K = decltype(k)::value;
#pragma unroll
            for (int j = (K * E) / NP; j < ((K + 1) * E) / NP; ++j) ah[j] = loadb<T, NVB>(cn + NVB * (HS + TPB * j));
        };
        auto ld_al = [&](auto k) __attribute__((always_inline)) {
            constexpr int K = decltype(k)::value;
#pragma unroll
            for (int j = (K * E) / NP; j < ((K + 1) * E) / NP; ++j) al[j] = loadb<T, NVB>(cn + NVB * TPB * j);
        };
        fft_q(ps + (size_t)1 * HS * NVB);
        STAMP(1, it, 7);
        mulq();
        ifft_q(ld_ah);
        STAMP(1, it, 8);
        {
            const cplx<T> w1t = wt();
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const cplx<T> w1 = w1t * root32<T>(j);
                Blk<T, NVB> hi = park[j * NTH];
#pragma unroll
                for (int c = 0; c < NVB; ++c) {
                    const cplx<T> u = mulc(vv[c][j], w1);
                    ol[c][j] = ol[c][j] + u;
                    hi.c[c] = addrot<true>(hi.c[c], u);              // + i u
                }
                park[j * NTH] = hi;
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // ---- round r = 3: its input leaves a_lo's registers, which take the lower half of the next item's column
#pragma unroll
        for (int j = 0; j < E; ++j) {
#pragma unroll
            for (int c = 0; c < NVB; ++c) vv[c][j] = al[j].c[c];
        }
        STAMP(1, it, 9);
        fft_q(ps + (size_t)3 * HS * NVB);
        STAMP(1, it, 10);
        mulq();
        ifft_q(ld_al);
        STAMP(1, it, 11);
        if (active) {
            const cplx<T> w1t = wt(), w3t = w1t * (w1t * w1t);
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const cplx<T> w3 = w3t * root32<T>(3 * j);
                const Blk<T, NVB> hi = park[j * NTH];
                Blk<T, NVB> o0, o1;
#pragma unroll
                for (int c = 0; c < NVB; ++c) {
                    const cplx<T> u = mulc(vv[c][j], w3);
                    o0.c[c] = ol[c][j] + u;
                    o1.c[c] = addrot<false>(hi.c[c], u);         // - i u
                }
                storeb<T, NVB>(col + NVB * TPB * j, o0);
                storeb<T, NVB>(col + NVB * (HS + TPB * j), o1);
            }
        }
        STAMP(1, it, 12);
    }
}

// ------------------------------------------------- column, forward only: the PSFHAT producer
// psfhat = r2c(ifftshift(psf)) (gridder.py:712-714) on the fast path's own kernels.  The (P, Q) = (2 nx, 2 ny)
// shifted PSF s is cut into its four (nx, ny) quadrants s_ab (a: top / bottom, b: left / right); the PRUNED
// forward row kernel turns each into a half spectrum T_ab (same layout as the convolution's T), and with
// sigma = (-1)^v (+ for the even-bin blocks, - for the odd-bin blocks)
//     R_top = T_00 + sigma T_01,   R_bot = T_10 + sigma T_11            (un-pruned row transform of length Q)
//     psfhat[2k]   = FFT_nx(R_top + R_bot)[k]
//     psfhat[2k+1] = FFT_nx((R_top - R_bot) .* w_P^n)[k]                 (un-pruned column transform of length P)
// written straight into the plan's psf_l[blk][pu][mu][c] layout.
template <typename T, int H, int E>
__global__ void __launch_bounds__((col_groups<H, E>() * (H / E)), (col_waves<T>(E)))
k_col_fwd_pow2(const cplx<T>* __restrict__ Tq, cplx<T>* __restrict__ psf_b,
               const cplx<T>* __restrict__ twP, const cplx<T>* __restrict__ ptw,
               int nblk, int nbe, size_t T_band, int four) {
    using F = RegFft<T, H, E>;
    constexpr int TPB = F::TPB;
    constexpr int NVB = FastCfg<T>::NVB;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int g = threadIdx.x / TPB, t = threadIdx.x % TPB;
    cplx<T>* lds = reinterpret_cast<cplx<T>*>(smem) + (size_t)g * (NVB * F::LDS_ELEMS);
    const int blk = blockIdx.x * col_groups<H, E>() + g;
    const bool active = blk < nblk;
    const size_t b = active ? blk : 0;
    const T sg = b >= (size_t)nbe ? T(-1) : T(1);
    const cplx<T>* c00 = Tq + (b * (size_t)H + t) * NVB;
    cplx<T> ve[NVB][E], vo[NVB][E];
    {
        const cplx<T>* tw2 = twP + t;
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const Blk<T, NVB> a00 = loadb<T, NVB>(c00 + NVB * TPB * j);
            const Blk<T, NVB> a01 = loadb<T, NVB>(c00 + T_band + NVB * TPB * j);
            const Blk<T, NVB> a10 = loadb<T, NVB>(c00 + 2 * T_band + NVB * TPB * j);
            const Blk<T, NVB> a11 = loadb<T, NVB>(c00 + 3 * T_band + NVB * TPB * j);
            const cplx<T> w = tw2[TPB * j];
#pragma unroll
            for (int c = 0; c < NVB; ++c) {
                const cplx<T> top = a00.c[c] + sg * a01.c[c], bot = a10.c[c] + sg * a11.c[c];
                ve[c][j] = top + bot;
                vo[c][j] = (top - bot) * w;
            }
        }
    }
    // psfhat[2 k + pu] of this block: parity-major or class-major (psf_off), k = t + TPB j
    // (MIXL: the 3 2^k / 5 2^k columns launder the thread index per transform, as k_col_pow2 does)
    constexpr bool MIXL = odd_part(H) > 1;
    if constexpr (MIXL) F::template runN<false, NVB>(ve, lds, launder(t), ptw);
    else
    F::template runN<false, NVB>(ve, lds, t, ptw);
    if (active) {
#pragma unroll
        for (int j = 0; j < E; ++j) {
            Blk<T, NVB> o;
#pragma unroll
            for (int c = 0; c < NVB; ++c) o.c[c] = ve[c][j];
            storeb<T, NVB>(psf_b + psf_off((int)b, 2 * (t + TPB * j), 0, H, NVB, four), o);
        }
    }
    if constexpr (MIXL) F::template runN<false, NVB>(vo, lds, launder(t), ptw);
    else
    F::template runN<false, NVB>(vo, lds, t, ptw);
    if (active) {
#pragma unroll
        for (int j = 0; j < E; ++j) {
            Blk<T, NVB> o;
#pragma unroll
            for (int c = 0; c < NVB; ++c) o.c[c] = vo[c][j];
            storeb<T, NVB>(psf_b + psf_off((int)b, 2 * (t + TPB * j) + 1, 0, H, NVB, four), o);
        }
    }
}

// ------------------------------------------------------------------- row forward
// Hermitian post-processing of one parity: the group's transform Z (registers, natural order)
// goes to LDS, then every lane produces the NVB bins of one block for one row and the G lanes
// of a block lane-group write one contiguous G*16-byte piece of T.
template <typename T, int L, int E, int PAR, typename F>
__device__ __forceinline__ void row_fwd_post(const cplx<T> (&z)[E], const cplx<T>* __restrict__ twQ,
                                             cplx<T>* lds0, cplx<T>* lds, cplx<T>* __restrict__ Tb,
                                             int nx, int i0, int t) {
    constexpr int TPB = F::TPB;
    constexpr int G = row_groups<T, L, E, RowCfg<T, L, false>::GMAX>();
    constexpr int NT = G * TPB;
    constexpr int STRIDE = F::LDS_ELEMS + 4;
    const int rr = threadIdx.x % G, bi = threadIdx.x / G;
    const cplx<T>* zr = lds0 + (size_t)rr * STRIDE;
    __syncthreads();                             // earlier readers of the row buffers are done
    {
        cplx<T>* wp = lds + F::pad(t);
#pragma unroll
        for (int j = 0; j < E; ++j) wp[F::cpad(TPB * j)] = z[j];
    }
    __syncthreads();
    // X[v] = 1/2 [ (Z[v] + conj Z[M-v]) - i w_Q^v (Z[v] - conj Z[M-v]) ]
    //   even v = 2m   : Z -> Ze[m mod L], Ze[(L-m) mod L]      m = 0..L
    //   odd  v = 2m+1 : Z -> Zo[m],       Zo[L-1-m]            m = 0..L-1
    constexpr int NVB = FastCfg<T>::NVB;
    constexpr int NBE = nblocks_even(L, NVB), NBO = nblocks_odd(L, NVB);
    constexpr int NBP = PAR ? NBO : NBE;                     // blocks of this parity
    constexpr int BSTEP = NT / G;
    cplx<T>* Tp = Tb + ((size_t)(PAR ? NBE : 0) * nx + i0 + rr) * NVB;
    constexpr int MS = NVB * BSTEP;               // m advances by MS per trip
    // (fp32: 0.0564 -> 0.0547 ms at 2048^2 x 4; the fp64 sweeps measured 1-2 % slower with it and keep the plain form)
    if constexpr (sizeof(T) == 4 && NBO % BSTEP == 0 && MS % 16 == 0) {
        // incremental addressing (see fwdp_post): the trip advances every index by a multiple of 16, so the two
        // padded LDS streams, the twiddle stream and the store address move by constants instead of being rebuilt
        // from the block index (selects, two pad()s, a 64-bit multiply per trip); the Nyquist block of the even
        // bins -- the one trip only bi = 0 makes -- is handled after the loop.
        constexpr int NREG = NBO / BSTEP;
        const int m0 = NVB * bi;
        const cplx<T>* za = zr + F::pad(m0);
        const cplx<T>* zb[NVB];
#pragma unroll
        for (int h = 0; h < NVB; ++h) zb[h] = zr + F::pad(L - PAR - m0 - h);
        const cplx<T>* tq = twQ + 2 * m0 + PAR;
        cplx<T>* st = Tp + (size_t)bi * nx * NVB;
        const size_t ustep = (size_t)BSTEP * nx * NVB;
        const bool first0 = PAR == 0 && bi == 0;
        for (int k = 0; k < NREG; ++k) {
            Blk<T, NVB> o;
#pragma unroll
            for (int h = 0; h < NVB; ++h) {
                const cplx<T> w = tq[2 * h];
                const cplx<T> zv = za[h];                      // pad(m0 + h) = pad(m0) + h: m0 is a multiple of NVB <= 2
                cplx<T> zm = *zb[h];
                if (first0 && h == 0 && k == 0) zm = zv;      // m = 0: both are z[0]
                o.c[h] = T(0.5) * addrot<false>(addc(zv, zm), w * subc(zv, zm));
                zb[h] -= F::cpad(MS);
            }
            storeb<T, NVB>(st, o);
            za += F::cpad(MS);
            tq += 2 * MS;
            st += ustep;
        }
        if (PAR == 0 && bi == 0) {                 // block NBE - 1: bin m = L (partner z[0]), beyond it zeros
            const cplx<T> z0 = zr[F::pad(0)];
            Blk<T, NVB> o;
            o.c[0] = T(0.5) * addrot<false>(addc(z0, z0), twQ[2 * L] * subc(z0, z0));
#pragma unroll
            for (int h = 1; h < NVB; ++h) o.c[h] = cplx<T>(0, 0);
            storeb<T, NVB>(Tp + (size_t)(NBE - 1) * nx * NVB, o);
        }
        return;
    }
    for (int b = bi; b < NBP; b += BSTEP) {       // (unrolling this loop spills: 0.52 -> 0.84 ms)
        Blk<T, NVB> o;
#pragma unroll
        for (int h = 0; h < NVB; ++h) {
            const int m = NVB * b + h;
            const bool valid = PAR || m <= L;
            const int ia = PAR ? m : (m >= L ? 0 : m);
            const int ib = PAR ? (L - 1 - m) : ((m == 0 || m > L) ? 0 : L - m);
            const cplx<T> w = twQ[valid ? 2 * m + PAR : 0];
            const cplx<T> zv = zr[F::pad(ia)];
            const cplx<T> zm = zr[F::pad(ib)];
            o.c[h] = T(0.5) * addrot<false>(addc(zv, zm), w * subc(zv, zm));
            if (!valid) o.c[h] = cplx<T>(0, 0);
        }
        storeb<T, NVB>(Tp + (size_t)b * nx * NVB, o);
    }
}

template <typename T, int L, int E>
__global__ void __launch_bounds__((row_groups<T, L, E, RowCfg<T, L, false>::GMAX>() * (L / E)))
k_row_fwd_pow2(const T* __restrict__ x, const T* __restrict__ beam, cplx<T>* __restrict__ Tw,
               const cplx<T>* __restrict__ twQ, const cplx<T>* __restrict__ twM,
               const cplx<T>* __restrict__ ptw, FastDims d, int band0) {
    // the even-bin and odd-bin transforms advance together (NV = 2) through ONE row buffer
    // (SEQX): the image row is read from HBM once instead of once per parity
    using F = RegFft<T, L, E, RowCfg<T, L, false>::WAVE, 0, false, true>;
    constexpr int TPB = F::TPB;
    constexpr int G = row_groups<T, L, E, RowCfg<T, L, false>::GMAX>();
    constexpr int STRIDE = F::LDS_ELEMS + 4;
    using V2 = typename vec2<T>::type;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cplx<T>* lds0 = reinterpret_cast<cplx<T>*>(smem);
    const int g = threadIdx.x / TPB, t = threadIdx.x % TPB;
    cplx<T>* lds = lds0 + (size_t)g * STRIDE;
    const int i0 = xcd_row_group<G>(blockIdx.x, gridDim.x) * G;      // 8192-point fp64 rows: G = 2, 32-byte pieces
    const int bl = blockIdx.y, band = band0 + bl;
    const size_t rowoff = (size_t)bl * d.xband + (size_t)(i0 + g) * d.xpitch;
    const V2* xr = reinterpret_cast<const V2*>(x + rowoff) + t;
    const V2* br = beam ? reinterpret_cast<const V2*>(beam + rowoff) + t : nullptr;
    cplx<T>* Tb = Tw + (size_t)band * d.T_band;

    cplx<T> vv[2][E];
    {
        const cplx<T>* tm = twM + t;
#pragma unroll
        for (int j = 0; j < E; ++j) {
            V2 a = xr[TPB * j];
            if (br) { V2 b = br[TPB * j]; a.x *= b.x; a.y *= b.y; }
            vv[0][j] = cplx<T>(a.x, a.y);                    // z[n] = x[2n] + i x[2n+1]
            vv[1][j] = vv[0][j] * tm[TPB * j];               // z .* w_M^n  (odd bins)
        }
    }
    F::template runN<false, 2>(vv, lds, t, ptw);
    row_fwd_post<T, L, E, 0, F>(vv[0], twQ, lds0, lds, Tb, d.nx, i0, t);
    row_fwd_post<T, L, E, 1, F>(vv[1], twQ, lds0, lds, Tb, d.nx, i0, t);
}

// Values derived from the thread index are loop invariant, so the optimiser computes every
// LDS / global address of the tile loop once, keeps ~40 of them live across it and spills:
// scratch reloads are vector-memory operations, and one of them inside an FFT (in-order
// vmcnt) waits for the prefetch it was supposed to overlap with.  Laundering the index at
// the top of each iteration makes the (cheap) address arithmetic part of the loop body.
// (launder() itself is defined near the top of the file)

// ------------------------------------------------- row forward, persistent + pipelined
// Same recipe as k_row_inv_pow2p below (read its comment first): one resident 1024-thread
// workgroup per CU walks the 8-row tiles; the NEXT tile's image rows are requested into
// registers as soon as the even-bin spectrum sits in the LDS and land while the two
// Hermitian post-processing sweeps of the current tile run; every twiddle comes from the
// LDS (pass table, w_M^n, w_Q^(2m+1) = w_M^m w_Q) so that nothing else queues behind the
// in-order vmcnt; the post-processing sweep is fully unrolled with clamped block indices
// (static store count -> the compiler's vmcnt for the prefetched rows is exact).
template <typename T, int L>
struct FwdP {
    // 128 threads per row, 8 rows per workgroup -- and for the 4096-point rows of 8192-pixel lines (BIG) 256 threads per
    // row, 4 rows (64-byte pieces, XCD-paired to full lines), with the twiddle table w_M^n cut down to the 512 entries a
    // sweep step spans: the full table (32 KB) does not fit next to four 4096-point rows.  Both transforms use 16
    // elements per thread, and with M = 2 L = 32 TPR every other twiddle is a table entry times a 32nd root of unity:
    //     w_M^(t + TPR j)      = w_M^t       root32(j)        (odd-bin pre-multiply, j = register index)
    //     w_M^(m0 + h + MS K)  = w_M^(m0+h)  root32(2 K)      (sweep step K, MS = NVB BSTEP = M / 16)
    // The kernel serves fp32 rows of 2048 and 4096 points (OK; the alternatives and their timings: DESIGN 8).  RowFwdK
    // reads OK for every class, so every member is well-formed at every power-of-two L.
    static constexpr bool BIG = L >= 4096;
    static constexpr int E = L >= 2048 ? 16 : 8;
    using F = RegFft<T, L, E, false, 0, true, true>;
    static constexpr int TPR = L / E;                 // threads per row
    static constexpr int NT = 1024;
    static constexpr int G = NT / TPR;
    static constexpr int STRIDE = F::LDS_ELEMS + 4;
    static constexpr int NVB = FastCfg<T>::NVB;
    static constexpr int NBE = nblocks_even(L, NVB);
    static constexpr int NBO = nblocks_odd(L, NVB);
    static constexpr int BSTEP = NT / G;
    static constexpr int NTM = BIG ? NVB * BSTEP : L; // entries of the w_M table kept in the LDS
    static constexpr int PTWP = (F::PTWC + 1) & ~1;
    static constexpr size_t LDS = sizeof(cplx<T>) * ((size_t)PTWP + NTM + (size_t)G * STRIDE);
    // sweep step K advances the bin index by MS = NVB BSTEP: w_M^(MS K) = root32(KR K)
    static constexpr int KR = (32 * NVB * BSTEP) / (2 * L);
    static constexpr bool OK = E == 16 && LDS <= (size_t)LDS_MAX && !(BIG && sizeof(T) == 8) &&
                               (!BIG || (32 * TPR == 2 * L && KR * 2 * L == 32 * NVB * BSTEP && NTM >= TPR));
    // w_M^(t + TPR j) from the table in the LDS
    __device__ __forceinline__ static cplx<T> tw_row(const cplx<T>* ltm, int t, int j) {
        if constexpr (BIG) return j == 0 ? ltm[t] : ltm[t] * root32<T>(j);
        else return ltm[t + TPR * j];
    }
    // tile rg of a band -> first row (xcd_line_pair: tiles b and b + 8 take the pieces of ONE 128-byte line)
    __device__ __forceinline__ static int tile_row(int rg, int tiles_per_band) {
        return xcd_line_pair(rg, tiles_per_band, 8 / G) * G;
    }
};

// ---- the sweep with strength-reduced addressing.
// The plain form of the sweep (removed, the code is at commit e9a762c) recomputed for every step the clamped block
// index, two padded LDS indices per value and a 64-bit `block * nx` product for the store: per tile and thread 18
// v_mad_u64_u32 / v_mul_lo_u32 (quarter-rate on CDNA) and ~150 index instructions next to ~230 of arithmetic (ISA count).  A step advances m by NVB * BSTEP, a multiple of 16:
// pad(m + 16 c) = pad(m) + 17 c, so each LDS stream is ONE base register with compile-time offsets; the store address
// is a workgroup-uniform base (band + step, scalar unit) plus a 32-bit per-thread offset that never changes.
// The irregular items -- m = 0 in the first even-bin step, and the last even-bin step, which holds only block NBE - 1
// (the Nyquist column) -- are handled apart.
template <typename T, int L, int PAR, int K, int NREG, typename Hook>
__device__ __forceinline__ void post_steps_lin(const cplx<T>* const (&za)[FastCfg<T>::NVB], const cplx<T>* const (&zb)[FastCfg<T>::NVB],
                                               const cplx<T>* lw, cplx<T> wq1, cplx<T>* ub, size_t ustep, unsigned voff,
                                               bool first0, const Hook& hook) {
    using P = FwdP<T, L>;
    using F = typename P::F;
    constexpr int NVB = P::NVB, MS = NVB * P::BSTEP;
    if constexpr (K < NREG) {
        hook(PassIdx<K>{});
        Blk<T, NVB> o;
#pragma unroll
        for (int h = 0; h < NVB; ++h) {
            cplx<T> w;
            if constexpr (P::BIG) w = K == 0 ? lw[h] : lw[h] * root32<T>(P::KR * K);  // w_M^(m0 + h + MS K), MS = KR M / 32
            else w = lw[MS * K + h];
            if (PAR) w = w * wq1;
            const cplx<T> zv = za[h][F::cpad(MS * K)];
            cplx<T> zm = zb[h][F::cpad(MS * (NREG - 1 - K))];
            if constexpr (PAR == 0 && K == 0) { if (first0 && h == 0) zm = zv; }      // m = 0: both are z[0]
            o.c[h] = T(0.5) * addrot<false>(addc(zv, zm), w * subc(zv, zm));
        }
        storeb<T, NVB>(ub + (size_t)K * ustep + voff, o);
        __builtin_amdgcn_sched_barrier(0);
        post_steps_lin<T, L, PAR, K + 1, NREG, Hook>(za, zb, lw, wq1, ub, ustep, voff, first0, hook);
    }
}

// hook(PassIdx<k>): called at the top of sweep step k (the kernel issues a slice of the next tile's loads there)
template <typename T, int L, int PAR, typename Hook = NoPassHook>
__device__ __forceinline__ void fwdp_post(const cplx<T>* zr, const cplx<T>* ltm, cplx<T> wq1,
                                          cplx<T>* __restrict__ Tb, int nx, int i0, int rr, int bi,
                                          const Hook& hook = Hook()) {
    using P = FwdP<T, L>;
    using F = typename P::F;
    constexpr int NVB = P::NVB, BS = P::BSTEP, MS = NVB * BS;
    constexpr int NBP = PAR ? P::NBO : P::NBE;
    constexpr int NIT = (NBP + BS - 1) / BS;
    constexpr int NREG = PAR ? NIT : NIT - 1;
    static_assert(MS % 16 == 0, "a step keeps the padding phase");
    static_assert(PAR ? (NBP == NIT * BS) : (NBP == (NIT - 1) * BS + 1), "block counts of the two sweeps");
    cplx<T>* ub = Tb + (size_t)(PAR ? P::NBE : 0) * nx * NVB;                         // workgroup-uniform
    const size_t ustep = (size_t)BS * nx * NVB;
    const unsigned voff = ((unsigned)bi * (unsigned)nx + (unsigned)(i0 + rr)) * NVB;  // elements; < 2^32
    const int m0 = NVB * bi;
    const cplx<T>* za[NVB];
    const cplx<T>* zb[NVB];
#pragma unroll
    for (int h = 0; h < NVB; ++h) {
        za[h] = zr + F::pad(m0 + h);
        // partner index of the LAST regular step (the lowest address of the stream): L - PAR - m - MS (NREG - 1)
        // (m = 0 makes step 0 read index L: inside the row's padded allotment, and the value is replaced there)
        zb[h] = zr + F::pad(L - PAR - (m0 + h) - MS * (NREG - 1));
    }
    post_steps_lin<T, L, PAR, 0, NREG, Hook>(za, zb, ltm + m0, wq1, ub, ustep, voff, bi == 0, hook);
    if constexpr (PAR == 0) {
        // the last even-bin step: block NBE - 1 = bins m = L (Nyquist: w_Q^(2L) = -1, partner z[0]) and, for NVB = 2,
        // m = L + 1 (beyond the spectrum: zero).  Every thread stores it, like the clamped step it replaces.
        hook(PassIdx<NREG>{});
        const cplx<T> z0 = zr[F::pad(0)];
        Blk<T, NVB> o;
        o.c[0] = T(0.5) * addrot<false>(addc(z0, z0), cplx<T>(T(-1), T(0)) * subc(z0, z0));
#pragma unroll
        for (int h = 1; h < NVB; ++h) o.c[h] = cplx<T>(0, 0);
        storeb<T, NVB>(ub + (size_t)(NBP - 1) * nx * NVB + (unsigned)(i0 + rr) * NVB, o);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// ------------------------------------------- row forward, persistent, parities in sequence
// The first persistent forward kernel (k_row_fwd_pow2p; removed, the code is at commit e9a762c) ran the even-bin and
// the odd-bin transform of a tile together and then the two post-processing sweeps; the next tile's rows were requested
// in one burst between them, which parks all 16 waves at
// issue (profiles/r02_a_phase_stamps_*: 8.0 of 28 us per trip, and the 9.3 us of the transforms run with NOTHING in
// flight).  Here the parities run one after the other:
//     z = x [* beam]              -> FFT  -> LDS -> even-bin sweep (stores)
//     z .* w_M^n  (x now dead)    -> FFT  -> LDS -> odd-bin sweep  (stores)
// and the next tile's rows are requested a few per PASS of the second transform INTO THE REGISTERS THE CURRENT ROWS
// JUST LEFT (no extra registers): the even-bin sweep's stores drain and the next rows arrive while the second
// transform computes, the odd-bin sweep's stores drain during the next tile's first transform.
template <typename T, int L, bool BEAM>
__global__ void __launch_bounds__((FwdP<T, L>::NT))
k_row_fwd_pow2q(const T* __restrict__ x, const T* __restrict__ beam, cplx<T>* __restrict__ Tw, const cplx<T>* __restrict__ twM,
                const cplx<T>* __restrict__ ptwc, FastDims d, int band0, int tiles_per_band, int ntiles,
                cplx<T> wq1) {
    using P = FwdP<T, L>;
    constexpr int E = P::E;
    using F = RegFft<T, L, E, false, 0, true, false>;        // one transform at a time, twiddles from LDS
    constexpr int TPB = F::TPB, G = P::G, NT = P::NT, NP = F::NPASS;
    using V2 = typename vec2<T>::type;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cplx<T>* ltw = reinterpret_cast<cplx<T>*>(smem);
    cplx<T>* ltm = ltw + P::PTWP;
    cplx<T>* lds0 = ltm + P::NTM;
    int vb = blockIdx.x;
    if (vb >= ntiles) return;
    for (int k = threadIdx.x; k < F::PTWC; k += NT) ltw[k] = ptwc[k];
    for (int k = threadIdx.x; k < P::NTM; k += NT) ltm[k] = twM[k];
    V2 xa[E], ba[BEAM ? E : 1];
    {
        const int bl = vb / tiles_per_band, i0 = P::tile_row(vb - bl * tiles_per_band, tiles_per_band);
        const int g = threadIdx.x / TPB, t = threadIdx.x % TPB;
        const size_t off = (size_t)bl * d.xband + (size_t)(i0 + g) * d.xpitch;
        const V2* xr = reinterpret_cast<const V2*>(x + off) + t;
#pragma unroll
        for (int j = 0; j < E; ++j) xa[j] = xr[TPB * j];
        if constexpr (BEAM) {
            const V2* br = reinterpret_cast<const V2*>(beam + off) + t;
#pragma unroll
            for (int j = 0; j < E; ++j) ba[j] = br[TPB * j];
        }
    }
    __syncthreads();                                    // tables visible
    for (int sit = 0;; ++sit) {
        STAMP(0, sit, 0);
        const int vbn = vb + (int)gridDim.x < ntiles ? vb + (int)gridDim.x : vb;   // last tile: harmless repeat
        const int bl = vb / tiles_per_band, i0 = P::tile_row(vb - bl * tiles_per_band, tiles_per_band);
        cplx<T>* Tb = Tw + (size_t)(band0 + bl) * d.T_band;
        cplx<T> vv[E];
        // ---- even bins: z[n] = x[2n] + i x[2n+1]
        {
            const int tid = launder((int)threadIdx.x);
            const int g = tid / TPB, t = tid % TPB;
            cplx<T>* lds = lds0 + (size_t)g * P::STRIDE;
#pragma unroll
            for (int j = 0; j < E; ++j) {
                if constexpr (BEAM) { xa[j].x *= ba[j].x; xa[j].y *= ba[j].y; }
                vv[j] = cplx<T>(xa[j].x, xa[j].y);
            }
            STAMP(0, sit, 1);
            F::template run<false>(vv, lds, t, ltw);
            STAMP(0, sit, 2);
        }
        {
            const int tid = launder((int)threadIdx.x);
            const int g = tid / TPB, t = tid % TPB;
            __syncthreads();                                     // last exchange's readers are done
            cplx<T>* wp = lds0 + (size_t)g * P::STRIDE + F::pad(t);
#pragma unroll
            for (int j = 0; j < E; ++j) wp[F::cpad(TPB * j)] = vv[j];
            __syncthreads();
        }
        STAMP(0, sit, 3);
        {
            const int tid = launder((int)threadIdx.x);
            fwdp_post<T, L, 0>(lds0 + (size_t)(tid % G) * P::STRIDE, ltm, wq1, Tb, d.nx, i0, tid % G, tid / G);
        }
        STAMP(0, sit, 4);
        // ---- odd bins: z .* w_M^n; the rows die here and their registers take the NEXT tile's rows
        {
            const int tid = launder((int)threadIdx.x);
            const int g = tid / TPB, t = tid % TPB;
            cplx<T>* lds = lds0 + (size_t)g * P::STRIDE;
#pragma unroll
            for (int j = 0; j < E; ++j) {
                vv[j] = cplx<T>(xa[j].x, xa[j].y) * P::tw_row(ltm, t, j);
                if ((j & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
            const int bln = vbn / tiles_per_band, i0n = P::tile_row(vbn - bln * tiles_per_band, tiles_per_band);
            const size_t offn = (size_t)bln * d.xband + (size_t)(i0n + g) * d.xpitch;
            const V2* xr = reinterpret_cast<const V2*>(x + offn) + t;
            const V2* br = BEAM ? reinterpret_cast<const V2*>(beam + offn) + t : nullptr;
            // the first exchange of this transform waits (barrier) for the even-bin sweep's LDS reads
            F::template run<false>(vv, lds, t, ltw, [&](auto k) {
                constexpr int K = decltype(k)::value;
#pragma unroll
                for (int j = (K * E) / NP; j < ((K + 1) * E) / NP; ++j) {
                    xa[j] = xr[TPB * j];
                    if constexpr (BEAM) ba[j] = br[TPB * j];
                }
            });
            STAMP(0, sit, 5);
        }
        {
            const int tid = launder((int)threadIdx.x);
            const int g = tid / TPB, t = tid % TPB;
            cplx<T>* wp = lds0 + (size_t)g * P::STRIDE + F::pad(t);
            __syncthreads();
#pragma unroll
            for (int j = 0; j < E; ++j) wp[F::cpad(TPB * j)] = vv[j];
            __syncthreads();
            fwdp_post<T, L, 1>(lds0 + (size_t)(tid % G) * P::STRIDE, ltm, wq1, Tb, d.nx, i0, tid % G, tid / G);
            STAMP(0, sit, 6);
            __syncthreads();                                     // rows free for the next transform
        }
        STAMP(0, sit, 7);
        if (vbn == vb) break;
        vb = vbn;
    }
}

// ------------------------------------------------------------------- row inverse
// one parity of the inverse row transform: gathers Y[2m + PAR][i0 .. i0+G) (G*8-byte
// pieces), LDS-transposes them to per-row order, builds the packed spectrum and runs
// the inverse FFT; result in vv (register j <-> sample t + TPB j of IFFT_L)
template <typename T, int L, int E, int PAR, typename PF>
__device__ __forceinline__ void row_inv_phase(PF&& after_loads_issued, const cplx<T>* __restrict__ Tb,
                                              const cplx<T>* __restrict__ twQ,
                                              const cplx<T>* __restrict__ ptw, cplx<T>* lds0,
                                              cplx<T>* lds, int nx, int i0, int t,
                                              cplx<T> (&vv)[E]) {
    using F = RegFft<T, L, E, RowCfg<T, L, true>::WAVE, InvDb<T, L>::OFF, true>;
    constexpr int TPB = F::TPB;
    constexpr int G = row_groups<T, L, E, RowCfg<T, L, true>::GMAX>();
    constexpr int NT = G * TPB;
    constexpr int STRIDE = F::LDS_ELEMS + 4;
    const int rr = threadIdx.x % G, bi = threadIdx.x / G;
    cplx<T>* yr = lds0 + (size_t)rr * STRIDE;
    __syncthreads();                            // previous phase done with the LDS
    constexpr int NVB = FastCfg<T>::NVB;
    constexpr int NBE = nblocks_even(L, NVB);
    constexpr int NBP = PAR ? nblocks_odd(L, NVB) : NBE;
    constexpr int BSTEP = NT / G;
    const cplx<T>* Tp = Tb + ((size_t)(PAR ? NBE : 0) * nx + i0 + rr) * NVB;
    // issue ALL strided loads of this thread before the first LDS write: a rolled loop
    // (load, wait, store, next) pays the HBM latency once per trip
    constexpr int NIT = (NBP + BSTEP - 1) / BSTEP;
    Blk<T, NVB> y[NIT];
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
        const int b = bi + k * BSTEP;
        if (b < NBP) y[k] = loadb<T, NVB>(Tp + (size_t)b * nx * NVB);    // bins of block b, row rr
    }
    // vmcnt is in order: loads issued from here on are YOUNGER than the strided loads above,
    // so waiting for those does not wait for these (prefetch hook of the kernel).  (Also
    // hoisting the w_Q twiddle loads of the unpacking loop up here would keep the prefetch in
    // flight longer, but costs 16 more live registers: measured slower, 1.01 vs 0.93 ms.)
    after_loads_issued();
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
        const int b = bi + k * BSTEP;
        if (b < NBP) {
#pragma unroll
            for (int h = 0; h < NVB; ++h)
                if (PAR || NVB * b + h <= L) yr[F::pad(NVB * b + h)] = y[k].c[h];
        }
    }
    __syncthreads();
    // Z[v] = (Y[v] + conj Y[M-v]) + i conj(w_Q^v) (Y[v] - conj Y[M-v]),  v = 2m + PAR
    //   even: Y[2m], Y[M-2m] = Yl[m], Yl[L-m]   (m = 0: DC and Nyquist, imag ignored)
    //   odd : Y[2m+1], Y[M-2m-1] = Yl[m], Yl[L-1-m]
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const int m = t + TPB * j;
        cplx<T> yv = lds[F::pad(m)];
        cplx<T> ym = lds[F::pad(PAR ? (L - 1 - m) : (L - m))];
        if (!PAR && m == 0) { yv.y = 0; ym.y = 0; }
        const cplx<T> w = twQ[2 * m + PAR];
        vv[j] = addrot<true>(addc(yv, ym), mulc(subc(yv, ym), w));
        // bound the number of LDS / twiddle loads in flight (else all 3 E are hoisted: spills)
        if ((j & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
    F::template run<true>(vv, lds, t, ptw);
}

template <typename T, int L, int E>
__global__ void __launch_bounds__((row_groups<T, L, E, RowCfg<T, L, true>::GMAX>() * (L / E)))
k_row_inv_pow2(const cplx<T>* __restrict__ Tw, const cplx<T>* __restrict__ twQ,
               const cplx<T>* __restrict__ twM, const cplx<T>* __restrict__ ptw,
               const T* __restrict__ x, const T* __restrict__ beam,
               const T* __restrict__ dot_with, const T* __restrict__ dot_with2, T* __restrict__ out,
               double* __restrict__ partials, FastDims d, int band0, T scale, T sigmainv) {
    using F = RegFft<T, L, E, RowCfg<T, L, true>::WAVE, InvDb<T, L>::OFF, true>;
    constexpr int TPB = F::TPB;
    constexpr int G = row_groups<T, L, E, RowCfg<T, L, true>::GMAX>();
    constexpr int NT = G * TPB;
    constexpr int STRIDE = F::LDS_ELEMS + 4;
    constexpr int HP = G / 2;
    using V2 = typename vec2<T>::type;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* red = reinterpret_cast<double*>(smem);                 // 3 sums * 16 waves * 8 B
    cplx<T>* ltw = reinterpret_cast<cplx<T>*>(smem + 384);          // compact twiddle table (LDS)
    cplx<T>* lds0 = ltw + ((F::PTWC + 1) & ~1);
    const int g = threadIdx.x / TPB, t = threadIdx.x % TPB;
    cplx<T>* lds = lds0 + (size_t)g * STRIDE;
    for (int k = threadIdx.x; k < F::PTWC; k += NT) ltw[k] = ptw[k];   // visible after the first barrier
    // XCD-aware row-group order: with G = 4 a 128-byte line of T is shared by two row groups;
    // workgroups are dealt round-robin over the 8 XCDs, so blocks b and b+8 share an L2 --
    // give THEM the two halves of a line (speed only, any mapping is correct).
    const int rg = xcd_row_group<G>(blockIdx.x, gridDim.x);
    const int i0 = rg * G;
    const int bl = blockIdx.y, band = band0 + bl;
    const cplx<T>* Tb = Tw + (size_t)band * d.T_band;
    cplx<T> vv[E], ev[E];
    row_inv_phase<T, L, E, 0>([] {}, Tb, twQ, ltw, lds0, lds, d.nx, i0, t, ev);
    // The kernel's phases do not overlap inside one workgroup (ablation: T loads 0.23 ms +
    // epilogue loads 0.31 ms + FFTs 0.20 ms + rest 0.22 ms = the 1.06 ms total at 4096^2 x 8),
    // and registers allow only one workgroup per CU: so the epilogue operands x and dot_with2
    // are requested right after the odd-bin strided loads and arrive while that transform runs.
    const size_t rowoff = ((size_t)bl * d.nx + (i0 + g)) * d.ny;
    const V2* xr = reinterpret_cast<const V2*>(x + rowoff) + t;
    const V2* br = beam ? reinterpret_cast<const V2*>(beam + rowoff) + t : nullptr;
    const V2* dr = dot_with ? reinterpret_cast<const V2*>(dot_with + rowoff) + t : nullptr;
    const V2* dr2 = dot_with2 ? reinterpret_cast<const V2*>(dot_with2 + rowoff) + t : nullptr;
    V2* orow = reinterpret_cast<V2*>(out + rowoff) + t;
    const bool dot_is_x = dot_with == x;            // PCG: <p, A p> with x = p
    // fp64: 2 x 32 more registers for the prefetched operands do not exist under the 128-VGPR cap of
    // a 1024-thread workgroup (it spilled 80-94 registers); they are read in the epilogue instead.  The same for fp32 at
    // 16 elements per thread (L >= 4096): x / x and r prefetched there cost 188 / 492 B of scratch, 1.29 / 1.63 ms
    constexpr bool BIG32 = sizeof(T) == 4 && E >= 16 && L >= 4096;
    // ... and the 3 2^k / 5 2^k rows at 1024 threads or 16+ elements (profiles/mixed_kernel_resources.md)
    constexpr bool MIXBIG = odd_part(L) > 1 && (NT >= 1024 || E >= 16 || (sizeof(T) == 8 && NT >= 512));
    constexpr bool PREF = !BIG32 && !MIXBIG && (sizeof(T) == 4 || NT < 1024);
    V2 xq[PREF ? E : 1], rq[PREF ? E : 1];
    row_inv_phase<T, L, E, 1>([&] {
        if constexpr (PREF) {
#pragma unroll
            for (int j = 0; j < E; ++j) {
                xq[j] = xr[TPB * j];
                if (dr2) rq[j] = dr2[TPB * j];
            }
        }
    }, Tb, twQ, ltw, lds0, lds, d.nx, i0, t, vv);
    // z[n] = e[n] + conj(w_M^n) o[n] ;  y[2n] = Re z, y[2n+1] = Im z
    double acc[3] = {0.0, 0.0, 0.0};       // <dot_with,out>, <dot_with2,out>, <out,out>
    const cplx<T>* tm = twM + t;
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const cplx<T> zz = ev[j] + mulc(vv[j], tm[TPB * j]);
        V2 val;
        val.x = zz.x * scale;
        val.y = zz.y * scale;
        if (br) { const V2 b = br[TPB * j]; val.x *= b.x; val.y *= b.y; }
        V2 xx;
        if constexpr (PREF) xx = xq[j]; else xx = xr[TPB * j];
        val.x += sigmainv * xx.x;
        val.y += sigmainv * xx.y;
        orow[TPB * j] = val;
        if (dr) {
            V2 dw = xx;
            if (!dot_is_x) dw = dr[TPB * j];
            acc[0] += (double)dw.x * (double)val.x + (double)dw.y * (double)val.y;
            if (dr2) {
                V2 d2;
                if constexpr (PREF) d2 = rq[j]; else d2 = dr2[TPB * j];
                acc[1] += (double)d2.x * (double)val.x + (double)d2.y * (double)val.y;
            }
            acc[2] += (double)val.x * (double)val.x + (double)val.y * (double)val.y;
        }
    }
    if (dot_with) {
        __syncthreads();
        block_sum<3>(acc, red);
        if (threadIdx.x == 0) {
            const size_t np = (size_t)gridDim.x * gridDim.y, k = (size_t)bl * gridDim.x + rg;
            partials[k] = acc[0]; partials[np + k] = acc[1]; partials[2 * np + k] = acc[2];
        }
    }
}

// ------------------------------------------------- row inverse, persistent + pipelined
// The plain kernel above keeps ONE 1024-thread workgroup per CU (registers), so its phases
// (strided T loads, FFT, epilogue loads, stores) run strictly one after the other.  This
// variant keeps the workgroup resident, loops over its row tiles and software-pipelines the
// strided loads: the 16-byte pieces of the NEXT phase (odd bins of this tile / even bins of
// the next tile) are requested into registers right after the current phase's pieces were
// scattered into the LDS and land while that phase's FFT runs.  For this to work no other
// global load may sit between the request and the FFT's end (s_waitcnt vmcnt retires in
// order), so w_M^n lives in the LDS as well (w_Q^(2m+1) = w_M^m * w_Q), and the even-bin
// result is parked in the LDS (not registers) while the odd-bin transform runs.
// INV_ROT: the workgroup -> tile map of k_row_inv_pow2p rotates by that many workgroups per trip.  With the static map
// (tile = workgroup + trip x grid) a workgroup -- and its whole XCD, workgroup b runs on XCD b mod 8 -- reads the SAME 128 bytes
// of every 1-KB stretch of a column block for the whole launch, and one XCD ran 13-15 % behind the others from the first trip to
// the last (profiles/r03_z_phase_stamps_4096x8_f32.md, per-XCD table): the launch lasts as long as its slowest workgroup.
// Rotating gives every workgroup every row residue in turn: 8 x 4096^2 fp32 0.614 -> 0.541 ms, 4 x 4096^2 fp64 0.716 -> 0.581,
// 2 x 8192^2 fp64 1.644 -> 1.450, fp32 0.749 -> 0.679, with beam 0.720 -> 0.635; bit-identical results
// (profiles/r03_ab_tile_rotation.md).  The forward rows and the column kernel show no such spread and no effect.
constexpr int INV_ROT = 3;
constexpr int INV_HOIST_B = 8;      // operand samples per batch of the batched epilogue (InvP::NXE)
// The persistent tiles that exist (OK, with E = InvPE<T, L>::E) and what tells them apart:
//   class             E   PARK OPF SMT NXT   next tile's even-bin pieces                 epilogue operands
//   fp32 1024 / 2048   8    1    1   0   1    prefetched across the epilogue              prefetched into registers; even-bin result
//                                                                                         parked in LDS; stores deferred
//   fp64 1024 / 2048   8    0    1   0   1    prefetched across the epilogue              prefetched into registers; even-bin result
//                                                                                         kept in registers
//   fp64 4096         16    0    0   1   1    prefetched across the epilogue              read in place
//   fp32 4096         16    0    0   1   0    requested behind the last operand batch     read in batches of INV_HOIST_B samples
//                                             (beam + two inner products: at the top of
//                                             the tile's own trip)
template <typename T, int L, int E>
struct InvP {
    using C = RowCfg<T, L, true>;
    using F = RegFft<T, L, E, C::WAVE, 0, true>;
    // fp32: always a full 1024-thread workgroup: 4 rows at L = 2048, 8 rows (128-byte pieces) at L = 1024.
    // fp64: two rows = 512 threads (the exchange buffers of four complex128 rows alone fill the LDS): with
    // one such workgroup per CU every thread may use 256 VGPRs, so the even-bin result stays in registers
    // (PARK = false) and the prefetched pieces / operands fit as well.
    static constexpr bool PARK = sizeof(T) == 4 && E < 16;     // (E = 16: four rows fill the LDS, the even-bin result stays in registers)
    static constexpr int G = (sizeof(T) == 4 ? 1024 : 512) / F::TPB;
    static constexpr int NT = G * F::TPB;
    static constexpr int STRIDE = F::LDS_ELEMS + 4;
    static constexpr int NVB = FastCfg<T>::NVB;
    static constexpr int NBE = nblocks_even(L, NVB);
    static constexpr int NBO = nblocks_odd(L, NVB);
    static constexpr int BSTEP = NT / G;
    static constexpr int NITE = (NBE + BSTEP - 1) / BSTEP;
    static constexpr int NITO = (NBO + BSTEP - 1) / BSTEP;
    static constexpr int PTWP = (F::PTWC + 1) & ~1;
    // 16 elements per thread (4096-point rows): the exchange buffers of the tile's rows leave no room for the full table
    // w_M^n (32 KB) nor for the parked even-bin result.  SMT: only w_M^t, t < TPB, is kept and
    // w_M^(t + TPB j) = w_M^t root32(j) (M = 2 L = 32 TPB).  OPF = false: the epilogue operands (x, dot_with2, beam) are
    // NOT prefetched into registers (fp32: vv + ev + the strided pieces already take 100 of the 128) but read where they
    // are used; what the persistent kernel still buys over the plain one are the tables loaded once and the strided
    // pieces of the next phase / next tile in flight during every transform.
    static constexpr bool SMT = E >= 16;
    static constexpr bool OPF = E < 16;
    // NXT: the NEXT tile's even-bin pieces are requested during the odd-bin transform and stay in flight across the
    // epilogue (always with OPF; without it only where registers remain: the 512-thread fp64 tiles have 256).
    // 2 x 8192^2 fp64: 1.376 -> 1.195 ms (239 VGPRs, no scratch).  It had measured a tie (1.612 / 1.618) while one XCD set
    // the pace of every variant (INV_ROT).  With it the barrier between the odd-bin transform's last exchange and the
    // next tile's scatter sits right behind that transform instead of at the top of the next trip (8 x 4096^2 fp32
    // 0.6293 -> 0.6229 ms, 2 x 8192^2 fp64 1.673 -> 1.643); not without it -- there the barrier was the only thing the
    // loads requested at the top of the trip were in flight across (0.706 -> 0.732)
    static constexpr bool NXT = OPF || sizeof(T) == 8;
    // NXE (the fp32 16-element tile, the only one without NXT): the operand rows are read in batches of INV_HOIST_B
    // samples behind the combine loop (the even-bin result is dead by then), and the next tile's even-bin pieces are
    // requested behind the last batch, in the registers the loop has freed, instead of at the top of the next trip,
    // where they were waited for right away (profiles/r03_q_phase_stamps_8192x2_*: 8.4 us of a 45 us trip):
    // 2 x 8192^2 fp32 0.682 -> 0.665 ms (no change with beam).  fp64 measured 1.955 vs 1.639 ms per 2 x 8192^2 with
    // the request at the start of the epilogue (the pieces queue behind the epilogue's own loads)
    static constexpr bool NXE = !NXT;
    static constexpr int NTM = SMT ? F::TPB : L;
    static constexpr size_t LDS = 384 + sizeof(cplx<T>) * ((size_t)PTWP + NTM + (size_t)G * STRIDE + (PARK ? (size_t)G * L : 0));
    static constexpr bool OK = odd_part(L) == 1 && LDS <= (size_t)LDS_MAX && !C::WAVE && (!SMT || 32 * F::TPB == 2 * L) &&
                               (sizeof(T) == 4 ? (NT == 1024 && G >= 4 && G <= 16) : (NT == 512 && (G == 2 || G == 4) && L >= 1024));
    __device__ __forceinline__ static cplx<T> tw_row(const cplx<T>* ltm, int t, int j) {     // w_M^(t + TPB j)
        if constexpr (SMT) return j == 0 ? ltm[t] : ltm[t] * root32<T>(j);
        else return ltm[t + F::TPB * j];
    }
};

// elements per thread of the PERSISTENT inverse row kernel: RowCfg's, except fp64 rows of 4096 points (C5) -- there the
// plain kernel is a 2-row, 1024-thread, 8-elements tile under the 128-VGPR cap, the persistent one a 2-row, 512-thread,
// 16-elements tile (174-199 VGPRs, no scratch; small tables, operands read in place): 2.30 -> 1.61 ms per 2 x 8192^2.
// (The plain kernel at 16 elements spills 648 B and takes 3.0 ms: the two kernels keep separate pass tables.)
template <typename T, int L> struct InvPE {
    static constexpr int MINL64 = 4096;       // smallest fp64 row length that takes the 16-element persistent tile
    static constexpr int E = (sizeof(T) == 8 && L >= MINL64) ? 16 : RowCfg<T, L, true>::E;
};

// the per-band variant (PB) of k_row_inv_pow2p exists for every persistent tile but the 4096-point fp32 one (SMT, 16
// elements per thread): that tile is at the 128-VGPR cap already, and its per-band flush kept 20-136 B of scratch however
// it was written.  There the launcher runs the whole-cube kernel once per band instead (launch_row_inv).
// the rows of the table above InvP.  SMT = (E >= 16), NXE = !NXT, the barrier that moves with NXT and the batched
// epilogue that comes with NXE were separate, type- and length-dependent flags once (commit 4085cbe) that coincide over
// these classes: a new class that needs them apart does not compile until it has a row here
template <typename T, int L>
constexpr bool invp_class(int e, bool park, bool opf, bool smt, bool nxt) {
    using P = InvP<T, L, InvPE<T, L>::E>;
    return P::OK && InvPE<T, L>::E == e && P::PARK == park && P::OPF == opf && P::SMT == smt && P::NXT == nxt &&
           P::NXE == !nxt && P::SMT == !opf && (nxt || sizeof(T) == 4);
}
static_assert(invp_class<float, 1024>(8, true, true, false, true) && invp_class<float, 2048>(8, true, true, false, true));
static_assert(invp_class<double, 1024>(8, false, true, false, true) && invp_class<double, 2048>(8, false, true, false, true));
static_assert(invp_class<double, 4096>(16, false, false, true, true) && invp_class<float, 4096>(16, false, false, true, false));

template <typename T, int L, int E>
constexpr bool inv_pb_ok() { return odd_part(L) == 1 && !(sizeof(T) == 4 && InvP<T, L, E>::SMT); }

// strength-reduced addressing of the strided pieces (see fwdp_post): the blocks of a thread are BSTEP apart, so the
// load address is a workgroup-uniform base (band, parity, step) + a 32-bit per-thread offset that never changes, and
// the padded LDS index of the scatter is one base + compile-time offsets.  Regular whenever BSTEP divides the odd-bin
// block count; the even bins then have exactly one more block (the Nyquist column), fetched by every thread in the last step.
template <typename T, int L, int E>
constexpr bool inv_lin_ok() {
    using P = InvP<T, L, E>;
    // (fp32 only: 1902 instead of 2147 instructions per thread and tile, 0.613 vs 0.616 ms -- the inverse kernel is not
    // issue bound the way the forward sweep was; the fp64 tiles measured 1 % slower with it)
    return sizeof(T) == 4 && P::NBO % P::BSTEP == 0 && P::NBE == P::NBO + 1 && P::NITO * P::BSTEP == P::NBO &&
           P::NITE == P::NITO + 1 && (P::NVB * P::BSTEP) % 16 == 0 && P::F::TPB % 16 == 0;
}
template <typename T, int L, int E, int PAR, int K0, int K1>
__device__ __forceinline__ void inv_issue_slice(const cplx<T>* __restrict__ Tb, int nx, int i0, int rr, int bi,
                                                Blk<T, FastCfg<T>::NVB> (&y)[InvP<T, L, E>::NITE]);
template <typename T, int L, int E, int PAR>
__device__ __forceinline__ void inv_issue(const cplx<T>* __restrict__ Tb, int nx, int i0, int rr, int bi,
                                          Blk<T, FastCfg<T>::NVB> (&y)[InvP<T, L, E>::NITE]) {
    using P = InvP<T, L, E>;
    constexpr int NBP = PAR ? P::NBO : P::NBE, NIT = PAR ? P::NITO : P::NITE;
    if constexpr (inv_lin_ok<T, L, E>()) {
        inv_issue_slice<T, L, E, PAR, 0, NIT>(Tb, nx, i0, rr, bi, y);
        return;
    }
    const cplx<T>* Tp = Tb + ((size_t)(PAR ? P::NBE : 0) * nx + i0 + rr) * P::NVB;
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
        int b = bi + k * P::BSTEP;
        if (b >= NBP) b = NBP - 1;                 // clamped (not skipped): the load count stays static
        y[k] = loadb<T, P::NVB>(Tp + (size_t)b * nx * P::NVB);
    }
}

// loads [K0, K1) of the same set (a compile-time slice: one FFT pass issues a few of them, see RegFft's pass hook)
template <typename T, int L, int E, int PAR, int K0, int K1>
__device__ __forceinline__ void inv_issue_slice(const cplx<T>* __restrict__ Tb, int nx, int i0, int rr, int bi,
                                                Blk<T, FastCfg<T>::NVB> (&y)[InvP<T, L, E>::NITE]) {
    using P = InvP<T, L, E>;
    constexpr int NBP = PAR ? P::NBO : P::NBE;
    if constexpr (inv_lin_ok<T, L, E>()) {
        const cplx<T>* ub = Tb + (size_t)(PAR ? P::NBE : 0) * nx * P::NVB;                    // workgroup-uniform
        const size_t ustep = (size_t)P::BSTEP * nx * P::NVB;
        const unsigned vrow = (unsigned)(i0 + rr) * P::NVB, voff = (unsigned)bi * (unsigned)nx * P::NVB + vrow;
#pragma unroll
        for (int k = K0; k < K1; ++k) {
            if (PAR == 0 && k == P::NITE - 1) y[k] = loadb<T, P::NVB>(ub + (size_t)(NBP - 1) * nx * P::NVB + vrow);   // Nyquist block
            else y[k] = loadb<T, P::NVB>(ub + (size_t)k * ustep + voff);
        }
        return;
    }
    const cplx<T>* Tp = Tb + ((size_t)(PAR ? P::NBE : 0) * nx + i0 + rr) * P::NVB;
#pragma unroll
    for (int k = K0; k < K1; ++k) {
        int b = bi + k * P::BSTEP;
        if (b >= NBP) b = NBP - 1;
        y[k] = loadb<T, P::NVB>(Tp + (size_t)b * nx * P::NVB);
    }
}

template <typename T, int L, int E, int PAR>
__device__ __forceinline__ void inv_scatter(const Blk<T, FastCfg<T>::NVB> (&y)[InvP<T, L, E>::NITE],
                                            cplx<T>* yr, int bi) {
    using P = InvP<T, L, E>;
    constexpr int NBP = PAR ? P::NBO : P::NBE, NIT = PAR ? P::NITO : P::NITE;
    if constexpr (inv_lin_ok<T, L, E>()) {
        cplx<T>* y0 = yr + P::F::pad(P::NVB * bi);          // pad(NVB bi + h + 16 c) = pad(NVB bi) + h + 17 c
#pragma unroll
        for (int k = 0; k < NIT; ++k) {
            if (PAR == 0 && k == NIT - 1) yr[P::F::pad(L)] = y[k].c[0];      // bin m = L; every thread holds the same value
            else {
#pragma unroll
                for (int h = 0; h < P::NVB; ++h) y0[P::F::cpad(P::NVB * P::BSTEP * k) + h] = y[k].c[h];
            }
        }
        return;
    }
    // no `if (b < NBP)` here: a conditional use lets the compiler SINK the load into the branch
    // (load + vmcnt(0) back to back).  Out-of-range threads hold a copy of the last block
    // (inv_issue clamps the same way) and store the same values to the same place.
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
        int b = bi + k * P::BSTEP;
        if (b >= NBP) b = NBP - 1;
#pragma unroll
        for (int h = 0; h < P::NVB; ++h)
            if (PAR || P::NVB * b + h <= L) yr[P::F::pad(P::NVB * b + h)] = y[k].c[h];
    }
}

template <typename T, int L, int E, int PAR>
__device__ __forceinline__ void inv_build(const cplx<T>* lds, const cplx<T>* ltm, cplx<T> wq1, int t,
                                          cplx<T> (&vv)[E]) {
    using F = typename InvP<T, L, E>::F;
    if constexpr (inv_lin_ok<T, L, E>()) {
        const cplx<T>* pa = lds + F::pad(t);                                  // Y[t + TPB j]      = pa[cpad(TPB j)]
        const cplx<T>* pb = lds + F::pad(L - PAR - t - F::TPB * (E - 1));     // partner of step j = pb[cpad(TPB (E-1-j))]
#pragma unroll
        for (int j = 0; j < E; ++j) {
            cplx<T> yv = pa[F::cpad(F::TPB * j)];
            cplx<T> ym = pb[F::cpad(F::TPB * (E - 1 - j))];
            if (!PAR && j == 0) { if (t == 0) { yv.y = 0; ym.y = 0; } }
            cplx<T> w = InvP<T, L, E>::tw_row(ltm, t, j);
            if (PAR) w = w * wq1;
            vv[j] = addrot<true>(addc(yv, ym), mulc(subc(yv, ym), w));
            if ((j & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const int m = t + F::TPB * j;
        cplx<T> yv = lds[F::pad(m)];
        cplx<T> ym = lds[F::pad(PAR ? (L - 1 - m) : (L - m))];
        if (!PAR && m == 0) { yv.y = 0; ym.y = 0; }
        cplx<T> w = InvP<T, L, E>::tw_row(ltm, t, j);          // w_M^m, m = t + TPB j
        if (PAR) w = w * wq1;
        vv[j] = addrot<true>(addc(yv, ym), mulc(subc(yv, ym), w));
        if ((j & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
}

// MODE 0: no inner products; 1: <x, out>, <out, out>; 2: also <dot_with2, out> (the PCG call)
// The strided pieces and the epilogue operands are requested a few per FFT PASS (RegFft pass hook) instead of
// in two bursts behind the scatters: a burst of 21 loads per thread parks all 16 waves at issue for 7.6 us of a
// 22.6 us trip (profiles/r02_a_phase_stamps_*).  Per trip, in issue order (vmcnt retires in order):
//     IFFT (even)  <- y(odd bins of this tile), then x [, beam]   of this tile's rows
//     IFFT (odd)   <- dot_with2 rows, then y(even bins of the NEXT tile)
// The first pass's slice of each (odd-bin pieces / dot_with2 rows) is requested right behind the scatter instead, so that
// something is in flight across the barrier and inv_build: 0.6075 -> 0.5999 ms per 8 x 4096^2 fp32, 0.7415 -> 0.7216 per
// 4 x 4096^2 fp64 (requesting more there measured no better: profiles/r03_ab_inv_ablation.md).
// PB (per band, MODE >= 1): the inner products are flushed whenever the next tile lies in another band, so that every
// partial belongs to one band: partials[(q * nbands + band) * grid + workgroup], zero for a band the workgroup never
// visits.  The tiles of trip s are [s grid, (s + 1) grid) under the rotated map, so a workgroup's band never decreases
// along its trips: one flush per band boundary it crosses.  PB = false compiles to the whole-cube kernel unchanged.
template <typename T, int L, int E, int MODE, bool BEAM, bool PB = false>
__global__ void __launch_bounds__((InvP<T, L, E>::NT), (InvP<T, L, E>::NT / 256))
k_row_inv_pow2p(const cplx<T>* __restrict__ Tw, const cplx<T>* __restrict__ twM,
                const cplx<T>* __restrict__ ptw, const T* __restrict__ x, const T* __restrict__ beam,
                const T* __restrict__ dot_with2, T* __restrict__ out,
                double* __restrict__ partials, FastDims d, int band0, int tiles_per_band, int ntiles,
                T scale, T sigmainv, cplx<T> wq1) {
    using P = InvP<T, L, E>;
    using F = typename P::F;
    constexpr int TPB = F::TPB, G = P::G, NT = P::NT;
    // (the batched-operand variant of the fp32 16-element tiles keeps 12 B of scratch with beam + two inner products: that
    // instantiation stays on the plain order -- a tile's pieces requested at the top of its own trip)
    constexpr bool BATCH = P::NXE && !(BEAM && MODE == 2);
    constexpr int NP = F::NPASS, NPA = NP / 2 > 0 ? NP / 2 : 1, NPB = NP - NPA > 0 ? NP - NPA : 1;
    using V2 = typename vec2<T>::type;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* red = reinterpret_cast<double*>(smem);
    cplx<T>* ltw = reinterpret_cast<cplx<T>*>(smem + 384);
    cplx<T>* ltm = ltw + P::PTWP;
    cplx<T>* lds0 = ltm + P::NTM;
    cplx<T>* park = lds0 + (size_t)G * P::STRIDE;
    int vb = blockIdx.x;
    if (vb >= ntiles) return;
    for (int k = threadIdx.x; k < F::PTWC; k += NT) ltw[k] = ptw[k];
    for (int k = threadIdx.x; k < P::NTM; k += NT) ltm[k] = twM[k];
    constexpr int SH = 128 / (G * (int)sizeof(cplx<T>) * P::NVB) > 1 ? 128 / (G * (int)sizeof(cplx<T>) * P::NVB) : 1;
    // (xcd_line_pair with its condition evaluated here, once: tested inside `tile` the kernel compiles to another schedule)
    const bool pairing = SH > 1 && (tiles_per_band % (8 * SH)) == 0;
    auto tile = [&](int v, int& bl, int& i0) {
        bl = v / tiles_per_band;
        int rg = v - bl * tiles_per_band;
        if (pairing) rg = xcd_paired(rg, SH);
        i0 = rg * G;
    };
    int bl, i0;
    tile(vb, bl, i0);
    Blk<T, P::NVB> y[P::NITE];
    // OPF kernels keep the NEXT tile's even-bin pieces in flight across the epilogue; without the registers for that
    // (!OPF: 16 elements per thread) a tile's even-bin pieces are requested at the top of its own trip instead
    if constexpr (P::NXT || BATCH)
        inv_issue<T, L, E, 0>(Tw + (size_t)(band0 + bl) * d.T_band, d.nx, i0, threadIdx.x % G, threadIdx.x / G, y);
    double acc[3] = {0.0, 0.0, 0.0};
    if constexpr (PB && MODE >= 1) {      // every slot of this workgroup starts at zero: a band it never visits reads 0
        if (threadIdx.x == 0) {           // (the same thread writes the visited bands' sums later: program order)
            const int n = 3 * (ntiles / tiles_per_band);
            for (int k = 0; k < n; ++k) partials[(size_t)k * gridDim.x + blockIdx.x] = 0.0;
        }
    }
    // deferred stores (fp32): a tile's output rows stay in registers and are written two per pass of the NEXT
    // tile's even-bin transform instead of in one burst behind the epilogue
    V2 ov[P::PARK ? E : 1];
    V2* oprev = nullptr;
    for (int sit = 0;; ++sit) {
        STAMP(2, sit, 0);
        // the workgroup -> tile map rotates by INV_ROT workgroups per trip: over its trips a workgroup sees the row
        // groups of every XCD, not always the same 128 bytes of each 1-KB stretch of a column block
        const int s1 = sit + 1;
        const int cand = (int)(((unsigned)blockIdx.x + (unsigned)s1 * (unsigned)INV_ROT) % gridDim.x) + s1 * (int)gridDim.x;
        const int vbn = cand < ntiles ? cand : vb;   // last tile: harmless repeat
        int bln, i0n;
        tile(vbn, bln, i0n);
        const cplx<T>* Tb = Tw + (size_t)(band0 + bl) * d.T_band;
        if constexpr (!P::NXT && !BATCH) {
            const int tid = launder((int)threadIdx.x);
            inv_issue<T, L, E, 0>(Tb, d.nx, i0, tid % G, tid / G, y);
        }
        cplx<T> vv[E], ev[P::PARK ? 1 : E];
        constexpr bool OPF = P::OPF;             // epilogue operands prefetched into registers
        V2 xq[OPF ? E : 1], rq[(OPF && MODE == 2) ? E : 1], bq[(OPF && BEAM) ? E : 1];
        // ---- even bins
        {
            const int tid = launder((int)threadIdx.x);
            const int g = tid / TPB, t = tid % TPB, rr = tid % G, bi = tid / G;
            cplx<T>* lds = lds0 + (size_t)g * P::STRIDE;
            if (!P::NXT || sit == 0) __syncthreads();        // (NXT: the barrier that protects lds0 sits behind the odd-bin transform)
            STAMP(2, sit, 1);
            inv_scatter<T, L, E, 0>(y, lds0 + (size_t)rr * P::STRIDE, bi);
            STAMP(2, sit, 2);
            inv_issue_slice<T, L, E, 1, 0, P::NITO / NPA>(Tb, d.nx, i0, rr, bi, y);   // pass 0's slice: in flight across the barrier and inv_build
            __syncthreads();
            STAMP(2, sit, 3);
            inv_build<T, L, E, 0>(lds, ltm, wq1, t, vv);
            STAMP(2, sit, 4);
            {
                const size_t rowoff = ((size_t)bl * d.nx + (i0 + g)) * d.ny;
                const V2* xr = reinterpret_cast<const V2*>(x + rowoff) + t;
                const V2* br = BEAM ? reinterpret_cast<const V2*>(beam + rowoff) + t : nullptr;
                F::template run<true>(vv, lds, t, ltw, [&](auto k) {
                    constexpr int K = decltype(k)::value;
                    if constexpr (P::PARK) {
                        if (oprev) {
#pragma unroll
                            for (int j = (K * E) / NP; j < ((K + 1) * E) / NP; ++j) oprev[TPB * j] = ov[j];
                        }
                    }
                    if constexpr (K < NPA) {            // first passes: the odd-bin pieces (needed first; pass 0's slice is out)
                        if constexpr (K != 0)
                        inv_issue_slice<T, L, E, 1, (K * P::NITO) / NPA, ((K + 1) * P::NITO) / NPA>(Tb, d.nx, i0, rr, bi, y);
                    } else if constexpr (OPF) {         // then this tile's x (and beam) rows for the epilogue
                        constexpr int KK = K - NPA;
#pragma unroll
                        for (int j = (KK * E) / NPB; j < ((KK + 1) * E) / NPB; ++j) {
                            xq[j] = xr[TPB * j];
                            if constexpr (BEAM) bq[j] = br[TPB * j];
                        }
                    }
                });
            }
            STAMP(2, sit, 5);
#pragma unroll
            for (int j = 0; j < E; ++j) {
                if constexpr (P::PARK) park[j * NT + tid] = vv[j]; else ev[j] = vv[j];
            }
        }
        // ---- odd bins
        {
            const int tid = launder((int)threadIdx.x);
            const int g = tid / TPB, t = tid % TPB, rr = tid % G, bi = tid / G;
            cplx<T>* lds = lds0 + (size_t)g * P::STRIDE;
            __syncthreads();
            STAMP(2, sit, 6);
            inv_scatter<T, L, E, 1>(y, lds0 + (size_t)rr * P::STRIDE, bi);
            STAMP(2, sit, 7);
            const size_t rowoff = ((size_t)bl * d.nx + (i0 + g)) * d.ny;
            const V2* dr2 = reinterpret_cast<const V2*>(dot_with2 + rowoff) + t;
            const cplx<T>* Tbn = Tw + (size_t)(band0 + bln) * d.T_band;
            if constexpr (MODE == 2 && OPF) {           // pass 0's slice of the dot_with2 rows: in flight across the barrier
#pragma unroll
                for (int j = 0; j < E / NPA; ++j) rq[j] = dr2[TPB * j];
            }
            __syncthreads();
            STAMP(2, sit, 8);
            inv_build<T, L, E, 1>(lds, ltm, wq1, t, vv);
            STAMP(2, sit, 9);
            F::template run<true>(vv, lds, t, ltw, [&](auto k) {
                constexpr int K = decltype(k)::value;
                if constexpr (MODE == 2 && OPF) {
                    if constexpr (K < NPA) {        // dot_with2 rows first: the epilogue waits for them
                        if constexpr (K != 0)
#pragma unroll
                        for (int j = (K * E) / NPA; j < ((K + 1) * E) / NPA; ++j) rq[j] = dr2[TPB * j];
                    } else {                        // the next tile's even-bin pieces stay in flight past the epilogue
                        constexpr int KK = K - NPA;
                        inv_issue_slice<T, L, E, 0, (KK * P::NITE) / NPB, ((KK + 1) * P::NITE) / NPB>(Tbn, d.nx, i0n, rr, bi, y);
                    }
                } else if constexpr (P::NXT) {
                    inv_issue_slice<T, L, E, 0, (K * P::NITE) / NP, ((K + 1) * P::NITE) / NP>(Tbn, d.nx, i0n, rr, bi, y);
                }
            });
            STAMP(2, sit, 10);
            // the last exchange's readers are done BEFORE the epilogue instead of at the top of the next trip: the waves are
            // still in step here (cheap), and a wave that is through with its epilogue scatters the next tile's pieces while
            // the others finish theirs -- the skew is absorbed by the barrier behind the scatter
            if constexpr (P::NXT) __syncthreads();
        }
        // ---- z[n] = e[n] + conj(w_M^n) o[n] ;  y[2n] = Re z, y[2n+1] = Im z
        {
            const int tid = launder((int)threadIdx.x);
            int g = tid / TPB;
            const int t = tid % TPB;
            // a row is shared by whole waves (TPB a multiple of 64): its index is wave-uniform -- said explicitly, the
            // row bases live in SGPRs and the 2-KB steps of the unrolled operand / result streams cost scalar adds instead
            // of a 64-bit VGPR address per stream and sample
            if constexpr (TPB % 64 == 0 && !P::OPF) g = __builtin_amdgcn_readfirstlane(g);
            const size_t rowoff = ((size_t)bl * d.nx + (i0 + g)) * d.ny;
            V2* orow = reinterpret_cast<V2*>(out + rowoff) + t;
            [[maybe_unused]] const V2* xr_e = reinterpret_cast<const V2*>(x + rowoff) + t;
            [[maybe_unused]] const V2* br_e = BEAM ? reinterpret_cast<const V2*>(beam + rowoff) + t : nullptr;
            [[maybe_unused]] const V2* dr_e = MODE == 2 ? reinterpret_cast<const V2*>(dot_with2 + rowoff) + t : nullptr;
            if constexpr (!OPF) {
                // operands read in place: combine the two parities FIRST (no load involved), so that the even-bin result
                // is dead before the operand streams start -- 32 registers less across the loop below
#pragma unroll
                for (int j = 0; j < E; ++j) vv[j] = ev[j] + mulc(vv[j], P::tw_row(ltm, t, j));
                __builtin_amdgcn_sched_barrier(0);
            }
            [[maybe_unused]] V2 xh[BATCH ? E : 1], rh[(BATCH && MODE == 2) ? E : 1], bh[(BATCH && BEAM) ? E : 1];

#pragma unroll
            for (int j = 0; j < E; ++j) {
                cplx<T> zz;
                if constexpr (!OPF) zz = vv[j];
                else {
                    cplx<T> e0;
                    if constexpr (P::PARK) e0 = park[j * NT + tid]; else e0 = ev[j];
                    zz = e0 + mulc(vv[j], P::tw_row(ltm, t, j));
                }
                if constexpr (BATCH) {
                    // operand rows in batches of HB samples; behind the LAST batch the next tile's even-bin pieces (in order:
                    // nothing the epilogue still waits for is queued behind them)
                    constexpr int HB = INV_HOIST_B;
                    if (j % HB == 0) {
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int q = j; q < j + HB && q < E; ++q) {
                            xh[q] = xr_e[TPB * q];
                            if constexpr (MODE == 2) rh[q] = dr_e[TPB * q];
                            if constexpr (BEAM) bh[q] = br_e[TPB * q];
                        }
                        if (j + HB >= E)
                            inv_issue<T, L, E, 0>(Tw + (size_t)(band0 + bln) * d.T_band, d.nx, i0n, tid % G, tid / G, y);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                V2 val;
                V2 xx;
                [[maybe_unused]] V2 bb;
                if constexpr (OPF) { xx = xq[j]; if constexpr (BEAM) bb = bq[j]; }
                else if constexpr (BATCH) { xx = xh[j]; if constexpr (BEAM) bb = bh[j]; }
                else { xx = xr_e[TPB * j]; if constexpr (BEAM) bb = br_e[TPB * j]; }
                if constexpr (BEAM) {
                    val.x = zz.x * scale * bb.x + sigmainv * xx.x;
                    val.y = zz.y * scale * bb.y + sigmainv * xx.y;
                } else {
                    val.x = zz.x * scale + sigmainv * xx.x;
                    val.y = zz.y * scale + sigmainv * xx.y;
                }
                if constexpr (P::PARK) ov[j] = val; else orow[TPB * j] = val;
                // operands read in place (!OPF): a few samples at a time, or every x / dot_with2 load of the tile is
                // hoisted to the top of the loop and spills
                if constexpr (!OPF && !BATCH) { if (sizeof(T) == 4 && (j & 3) == 3) __builtin_amdgcn_sched_barrier(0); }
                if constexpr (MODE >= 1) {
                    acc[0] += (double)xx.x * (double)val.x + (double)xx.y * (double)val.y;
                    if constexpr (MODE == 2) {
                        V2 d2;
                        if constexpr (OPF) d2 = rq[j]; else if constexpr (BATCH) d2 = rh[j];
                        else d2 = dr_e[TPB * j];
                        acc[1] += (double)d2.x * (double)val.x + (double)d2.y * (double)val.y;
                    }
                    acc[2] += (double)val.x * (double)val.x + (double)val.y * (double)val.y;
                }
            }
        }
        STAMP(2, sit, 11);
        if constexpr (P::PARK) {
            const int tid = launder((int)threadIdx.x);
            const int g = tid / TPB, t = tid % TPB;
            oprev = reinterpret_cast<V2*>(out + ((size_t)bl * d.nx + (i0 + g)) * d.ny) + t;
        }
        if constexpr (PB && MODE >= 1) {
            if (vbn == vb || bln != bl) {     // band bl is done for this workgroup (the last tile is not repeated)
                block_sum<3>(acc, red);
                if (threadIdx.x == 0) {
                    const size_t np = (size_t)(ntiles / tiles_per_band) * gridDim.x, k = (size_t)bl * gridDim.x + blockIdx.x;
                    partials[k] = acc[0]; partials[np + k] = acc[1]; partials[2 * np + k] = acc[2];
                }
                acc[0] = 0.0; acc[1] = 0.0; acc[2] = 0.0;
            }
        }
        if (vbn == vb) break;
        vb = vbn; bl = bln; i0 = i0n;
    }
    if constexpr (P::PARK) {
        if (oprev) {
#pragma unroll
            for (int j = 0; j < E; ++j) oprev[TPB * j] = ov[j];
        }
    }
    if constexpr (!PB && MODE >= 1) {
        __syncthreads();
        block_sum<3>(acc, red);
        if (threadIdx.x == 0) {           // one slot per WORKGROUP (launcher: last_npartials = grid)
            const size_t np = gridDim.x;
            partials[blockIdx.x] = acc[0]; partials[np + blockIdx.x] = acc[1]; partials[2 * np + blockIdx.x] = acc[2];
        }
    }
}

// -------------------------------------------------------------------- host side
// Every fact about which kernel variant serves a size / type class and what it needs is stated ONCE below: ColCfg /
// ColKernels for the column pass (nx), RowFwdK / RowInvK for the row passes (ny / 2).  The launchers, the LDS-attribute
// set-up and the table set-up all read those; a new or retuned variant is entered there and nowhere else.

// f(std::integral_constant<int, N>) for the transform length N == n; false if the fast path has no such length
template <typename Fn>
static inline bool for_pow2_size(int n, Fn&& f) {
    switch (n) {
#define X(NN) case NN: f(std::integral_constant<int, NN>{}); return true;
        X(64) X(128) X(256) X(512) X(1024) X(2048) X(4096) X(8192)
#undef X
        default: return false;
    }
}

// the same for the lengths 3 2^k (96 .. 6144) and 5 2^k (80 .. 5120) of the third object
template <typename Fn>
static inline bool for_mix_size(int n, Fn&& f) {
    switch (n) {
#define X(NN) case NN: f(std::integral_constant<int, NN>{}); return true;
        X(96) X(192) X(384) X(768) X(1536) X(3072) X(6144)
        X(80) X(160) X(320) X(640) X(1280) X(2560) X(5120)
#undef X
        default: return false;
    }
}
// which of them an axis may have: columns (H = nx) from 96, rows (L = ny / 2) from 80 and, like the power-of-two rows, up
// to what one row's transform of that type takes in the LDS
constexpr int MIX_COL_MIN = 96, MIX_ROW_MIN = 80;
constexpr int mix_row_max(bool f32) { return f32 ? 6144 : 3072; }
inline bool mix_len(int n, int lo, int hi) { return (odd_part(n) == 3 || odd_part(n) == 5) && n >= lo && n <= hi; }
inline bool mix_col_len(int nx) { return mix_len(nx, MIX_COL_MIN, 6144); }
inline bool mix_row_len(int L, bool f32) { return mix_len(L, MIX_ROW_MIN, mix_row_max(f32)); }
// rows per workgroup of every row kernel divide this, and it divides every supported nx
constexpr int ROW_TILE_MAX = 32;

// the two-level column kernel k_col_pow2x and its class-major psf_l (the `four` of psf_off) serve nx >= 8192
constexpr bool col_two_level(int nx) { return odd_part(nx) == 1 && nx >= 8192; }

enum Tab {                     // device tables owned by the plan
    PTW_COL,                   // pass table of the one-level column transform (plain kernel, PSFHAT producer)
    PTWC_COL,                  // compact (w only) table of the persistent / two-level column kernel, copied to LDS (ColCfg)
    PTW_ROW,                   // plain forward row kernel
    PTWC_ROW_FWD,              // compact pass table of the persistent forward row kernel (its own E)
    PTWC_ROW_INV,              // inverse row kernel: COMPACT table, copied to LDS
    PTWC_ROW_INV_P,            // the persistent inverse kernel's, where its elements per thread differ (InvPE); else an ALIAS of PTWC_ROW_INV
    TW_M,                      // exp(-2 pi i n / M), n < L
    NTAB
};
struct FastTables {            // stored behind p->fast_tables
    void* tab[NTAB];
    int num_cu;
};

// The seam between the objects: what serves an axis, as a record of functions.  Each object defines the tables of the
// classes it owns (its entry block at the end of the file); the two selectors are the only place that maps a length to
// its family, and a length that the family has no class for is reported by the family's class dispatch (unsupported_len).
struct ColPass {               // the column pass (nx)
    int (*prepare)(pfb_conv_plan* p, FastTables* ft);                        // tables and LDS attributes
    int (*launch)(pfb_conv_plan* p, const FastTables* ft, int band0, int nb, hipStream_t st);
    int (*fwd_launch)(pfb_conv_plan* p, const FastTables* ft, const void* Tq, int band, hipStream_t st);   // PSFHAT producer
};
struct RowPass {               // the two row passes (ny / 2)
    int (*prepare)(pfb_conv_plan* p, FastTables* ft);
    int (*rows_per_wg)(const pfb_conv_plan* p);                              // of the plain inverse kernel (0: no such class)
    int (*fwd_launch)(pfb_conv_plan* p, const FastTables* ft, void* Tbuf, int band0, int nb, const void* x,
                      const void* beam, size_t xpitch, size_t xband, hipStream_t st);
    int (*inv_launch)(pfb_conv_plan* p, const FastTables* ft, const ApplyArgs& a);
};
// (reached through functions: a namespace-scope constant would also be emitted, host addresses and all, into the code object)
const ColPass& col_pass_pow2();     // object 2
const RowPass& row_pass_pow2();     // object 1
const ColPass& col_pass_mix();      // object 3
const RowPass& row_pass_mix();
inline const ColPass& col_pass(const pfb_conv_plan* p) { return mix_col_len(p->nx) ? col_pass_mix() : col_pass_pow2(); }
inline const RowPass& row_pass(const pfb_conv_plan* p) {
    return mix_row_len(p->ny / 2, p->dtype == PFB_F32) ? row_pass_mix() : row_pass_pow2();
}
static int unsupported_len(const char* axis, int n) {
    set_error("pow2: unsupported %s %d", axis, n);
    return PFB_ERR_UNSUPPORTED;
}

// n table entries written by fill(cplx<T>*) -> a new device array
template <typename T, typename Fill>
static int upload_table(void** dev, int n, Fill&& fill) {
    std::vector<cplx<T>> h(n > 0 ? n : 1);
    if (n > 0) fill(h.data());
    PFB_HIP_CHECK(hipMalloc(dev, sizeof(cplx<T>) * h.size()));
    PFB_HIP_CHECK(hipMemcpy(*dev, h.data(), sizeof(cplx<T>) * h.size(), hipMemcpyHostToDevice));
    return PFB_OK;
}
template <typename T, int N, int E>
static int upload_ptw(void** dev) { return upload_table<T>(dev, ptw_total<N, E>(), fill_ptw<T, N, E>); }
template <typename T, int N, int E>
static int upload_ptwc(void** dev) { return upload_table<T>(dev, ptw_total<N, E>() / 4, fill_ptw_compact<T, N, E>); }

template <typename K>
static int set_lds_max(K* kernel) {
    PFB_HIP_CHECK(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX));
    return PFB_OK;
}

// Grid of the persistent column kernel k_col_pow2p: not all `maxgrid` resident workgroups but as many as give every one of them the same number
// of trips.  `need` is rarely a multiple of the CU count (a band is 2^k + 1 column blocks), and a last trip with a handful
// of workgroups runs at their latency while the rest of the chip idles -- the same work on slightly fewer workgroups is
// bandwidth bound to the end: col 0.816 -> 0.800 ms at 8 x 4096^2 fp32 (253 instead of 256 workgroups), 45.5 -> 42.6 us
// at 1 x 2048^2 (342 instead of 512), 129.3 -> 126.5 us at 1 x 4096^2 (228), 0.889 -> 0.861 ms at 4 x 4096^2 fp64.  Only for
// that kernel (the row kernels' grids divide evenly at the usual sizes, the two-level column kernel loses).
static inline int balanced_grid(int need, int maxgrid) {
    if (need <= maxgrid) return need;
    const int trips = (need + maxgrid - 1) / maxgrid;
    return (need + trips - 1) / trips;
}

// The column pass of class (T, H = nx): which kernel serves it and what that kernel needs.
enum class ColKind { Plain, Persistent, TwoLevel };
// workgroups per CU of the persistent and the two-level kernel: one resident set, 8 waves per CU at 256 VGPRs
constexpr int col_resident(int threads) { return (8 * 64) / threads > 0 ? (8 * 64) / threads : 1; }
template <typename T, int H> struct ColCfg {
    static constexpr int NVB = FastCfg<T>::NVB;
    // the one-level transform (plain and persistent kernel, PSFHAT producer)
    static constexpr int E1 = ecol<T, H>();
    using F1 = RegFft<T, H, E1>;
    static constexpr int GC1 = col_groups<H, E1>(), NT1 = GC1 * F1::TPB;
    static constexpr size_t XB1 = sizeof(cplx<T>) * (size_t)GC1 * NVB * F1::LDS_ELEMS;   // one set of exchange buffers
    static constexpr size_t TAB1 = sizeof(cplx<T>) * (size_t)((F1::PTWC + 1) & ~1);       // the compact table in the LDS
    // persistent kernel: needs its LDS (exchange buffers + twiddle table) to fit; measured faster
    // for H >= 2048 (fp32, packed arithmetic: 1.07 vs 1.32 ms at 4096^2 x 8, 0.276 vs 0.347 at 2048^2 x 8;
    // fp64: 1.19 vs 1.41 and 0.266 vs 0.333 at x 4; a tie or a small loss at H <= 1024)
    // (the lengths 3 2^k and 5 2^k: the plain kernel, whatever their size)
    static constexpr ColKind KIND = odd_part(H) > 1 ? ColKind::Plain : col_two_level(H) ? ColKind::TwoLevel
                                  : H >= 2048 && XB1 + TAB1 <= (size_t)LDS_MAX ? ColKind::Persistent : ColKind::Plain;
    // second exchange buffer set when ONE workgroup per CU is resident anyway and it fits: col 0.98 ->
    // 0.96 ms at 8 x 4096^2 fp32, 1.16 -> 1.10 ms at 4 x 4096^2 fp64; with two workgroups per CU (H = 2048)
    // the doubled LDS costs residency (fp64 0.245 -> 0.304 ms)
    static constexpr bool DB = KIND == ColKind::Persistent && col_resident(NT1) == 1 && 2 * XB1 + TAB1 <= (size_t)LDS_MAX;

    // the serving kernel's launch shape; TAB_N, TAB_E: the transform whose pass table it reads (PTW_COL for the plain
    // kernel, the compact PTWC_COL otherwise)
    struct Shape { int gc, threads; size_t lds; int wg_per_cu, tab_n, tab_e; };
    static constexpr Shape shape() {
        if constexpr (KIND == ColKind::TwoLevel) {
            // HS = H / 2 point sub-transforms, one resident workgroup set (2 waves per SIMD)
            using CX = ColX<T, H, ECOLX>;
            const int wg_lds = (int)((size_t)LDS_MAX / CX::LDS);
            int wg_per_cu = col_resident(CX::NT);
            if (wg_per_cu > wg_lds) wg_per_cu = wg_lds > 0 ? wg_lds : 1;
            return {CX::GC, CX::NT, CX::LDS, wg_per_cu, CX::HS, ECOLX};
        } else if constexpr (KIND == ColKind::Persistent) {
            return {GC1, NT1, (DB ? 2 : 1) * XB1 + TAB1, col_resident(NT1), H, E1};
        } else {
            return {GC1, NT1, XB1, 0, H, E1};
        }
    }
};

// The column-kernel instantiations of class (T, H).
template <typename T, int H> struct ColKernels {
    using C = ColCfg<T, H>;
    static constexpr auto plain() { return k_col_pow2<T, H, C::E1>; }
    static constexpr auto fwd() { return k_col_fwd_pow2<T, H, C::E1>; }
    // the serving persistent / two-level kernel: f(kernel, NT) for its plain and its non-temporal PSF reads
    template <typename Fn> static void serving(Fn&& f) {
        if constexpr (C::KIND == ColKind::Persistent) {
            f(k_col_pow2p<T, H, C::E1, C::DB, false>, false);
            f(k_col_pow2p<T, H, C::E1, C::DB, true>, true);
        } else if constexpr (C::KIND == ColKind::TwoLevel) {
            f(k_col_pow2x<T, H, ECOLX, false>, false);
            f(k_col_pow2x<T, H, ECOLX, true>, true);
        }
    }
    // all of them, f(kernel)
    template <typename Fn> static void all(Fn&& f) {
        // (the plain kernel exists only where it is launched: without its six never-launched instantiations of the
        // persistent and two-level classes every other kernel of the object compiles to the same instructions)
        if constexpr (C::KIND == ColKind::Plain) f(plain());
        f(fwd());
        serving([&](auto* k, bool) { f(k); });
        // KEPT INSTANTIATED, NEVER LAUNCHED: k_col_pow2x<double, 4096> -- the one-level kernel serves 4096-point columns -- shares
        // the 2048-point RegFft with k_col_pow2p<double, 2048>: without it the compiler contracts some products of that kernel
        // differently and 2048^2 fp64 results change in the last bits
        if constexpr (H == 4096 && sizeof(T) == 8) {
            f(k_col_pow2x<T, H, ECOLX, false>);
            f(k_col_pow2x<T, H, ECOLX, true>);
        }
    }
};

template <typename T, int H>
static int launch_col(pfb_conv_plan* p, const FastTables* ft, int band0, int nb, hipStream_t st) {
    using C = ColCfg<T, H>;
    using CK = ColKernels<T, H>;
    constexpr auto S = C::shape();
    const int nblk = fast_nblocks(p->ny / 2, FastCfg<T>::NVB);
    if constexpr (C::KIND == ColKind::Plain) {
        hipLaunchKernelGGL(CK::plain(), dim3((nblk + S.gc - 1) / S.gc, nb), dim3(S.threads), S.lds, st,
                           (cplx<T>*)p->T, (const cplx<T>*)p->psf_l, (const cplx<T>*)p->twP,
                           (const cplx<T>*)ft->tab[PTW_COL], nblk, p->T_elems_per_band, p->psf_elems_per_band, band0);
    } else {
        // bands in DESCENDING order (persistent kernels): the row pass before and after run ascending, so each pass starts on
        // the band whose T the previous one touched last (part of it still in the 256 MiB Infinity Cache):
        // col 0.995 -> 0.987 ms, row_inv 0.666 -> 0.660 ms at 8 x 4096^2 fp32
        const int band_first = band0 + nb - 1;
        // psf read with non-temporal loads (see loadb_nt) only when this launch's share of the PSF spectrum is itself of the
        // Infinity Cache's size or larger: a smaller one is RE-READ from that cache by the next apply and must stay allocatable
        const bool psf_nt = sizeof(cplx<T>) * p->psf_elems_per_band * (size_t)nb >= ((size_t)200 << 20);
        const int nitems = nblk * nb, need = (nitems + S.gc - 1) / S.gc, maxgrid = ft->num_cu * S.wg_per_cu;
        // (the two-level kernel without balanced_grid: it is bound by the issue of its transforms, every workgroup counts --
        // 2.003 -> 2.047 ms fp64, 1.110 -> 1.128 fp32 with 253 / 249 instead of 256)
        const int grid = C::KIND == ColKind::Persistent ? balanced_grid(need, maxgrid) : (need < maxgrid ? need : maxgrid);
        CK::serving([&](auto* k, bool nt) {
            if (nt != psf_nt) return;
            hipLaunchKernelGGL(k, dim3(grid), dim3(S.threads), S.lds, st,
                               (cplx<T>*)p->T, (const cplx<T>*)p->psf_l, (const cplx<T>*)p->twP,
                               (const cplx<T>*)ft->tab[PTWC_COL], nblk, nitems, p->T_elems_per_band,
                               p->psf_elems_per_band, band_first, -1);
        });
    }
    return PFB_OK;
}

// PSFHAT producer: the four quadrant spectra in Tq (slots of T_elems_per_band) -> psf_l of `band`
template <typename T, int H>
static int launch_col_fwd(pfb_conv_plan* p, const FastTables* ft, const void* Tq, int band, hipStream_t st) {
    using C = ColCfg<T, H>;
    using CK = ColKernels<T, H>;
    const int L = p->ny / 2;
    const int nblk = fast_nblocks(L, C::NVB), nbe = nblocks_even(L, C::NVB);
    hipLaunchKernelGGL(CK::fwd(), dim3((nblk + C::GC1 - 1) / C::GC1), dim3(C::NT1), C::XB1, st,
                       (const cplx<T>*)Tq, (cplx<T>*)p->psf_l + (size_t)band * p->psf_elems_per_band,
                       (const cplx<T>*)p->twP, (const cplx<T>*)ft->tab[PTW_COL], nblk, nbe, p->T_elems_per_band,
                       col_two_level(H));
    return PFB_OK;
}

// tables and LDS attributes of class (T, H)
template <typename T, int H>
static int col_prepare(FastTables* ft) {
    constexpr auto S = ColCfg<T, H>::shape();
    int rc = upload_ptw<T, H, ColCfg<T, H>::E1>(&ft->tab[PTW_COL]);
    if constexpr (ColCfg<T, H>::KIND != ColKind::Plain)
        if (rc == PFB_OK) rc = upload_ptwc<T, S.tab_n, S.tab_e>(&ft->tab[PTWC_COL]);
    ColKernels<T, H>::all([&](auto* k) { if (rc == PFB_OK) rc = set_lds_max(k); });
    return rc;
}

// The ColPass of a class family.  D::each(p, f) is the family's class dispatch: f(T{}, std::integral_constant<int, H>) -> int
// for the plan's type and nx, or unsupported_len.
template <typename D> struct ColPassOf {
    static int prepare(pfb_conv_plan* p, FastTables* ft) {
        return D::each(p, [&](auto t, auto h) { return col_prepare<decltype(t), h()>(ft); });
    }
    static int launch(pfb_conv_plan* p, const FastTables* ft, int band0, int nb, hipStream_t st) {
        return D::each(p, [&](auto t, auto h) { return launch_col<decltype(t), h()>(p, ft, band0, nb, st); });
    }
    static int fwd_launch(pfb_conv_plan* p, const FastTables* ft, const void* Tq, int band, hipStream_t st) {
        return D::each(p, [&](auto t, auto h) { return launch_col_fwd<decltype(t), h()>(p, ft, Tq, band, st); });
    }
    static constexpr ColPass table = {prepare, launch, fwd_launch};
};

// The forward row kernels of class (T, L = ny / 2): the persistent one where FwdP::OK, else the plain one.
// (FwdP is written for power-of-two rows and is not even instantiated for the others)
template <typename T, int L> constexpr bool fwdp_ok() {
    if constexpr (odd_part(L) > 1) return false;
    else return FwdP<T, L>::OK;
}
template <typename T, int L> struct RowFwdK {
    using FP = FwdP<T, L>;
    static constexpr bool PERSISTENT = fwdp_ok<T, L>();
    static constexpr int E = [] { if constexpr (PERSISTENT) return FP::E; else return RowCfg<T, L, false>::E; }();
    static constexpr auto plain() { return k_row_fwd_pow2<T, L, E>; }
    // the instantiations launch_row_fwd can reach: f(kernel, beam) (the plain kernel takes `beam` at run time)
    template <typename Fn> static void reachable(Fn&& f) {
        if constexpr (PERSISTENT) {
            f(k_row_fwd_pow2q<T, L, false>, false);
            f(k_row_fwd_pow2q<T, L, true>, true);
        } else {
            f(plain(), false);
        }
    }
};

// The inverse row kernels of class (T, L): the plain one, and where InvP::OK the persistent one by mode (0: no inner
// product, 1: <x, out>, 2: + <dot_with2, out>), beam and -- where inv_pb_ok -- its per-band form.
template <typename T, int L> struct RowInvK {
    static constexpr int E = RowCfg<T, L, true>::E, EP = InvPE<T, L>::E;
    using IP = InvP<T, L, EP>;
    static constexpr bool PERSISTENT = IP::OK;
    static constexpr bool PER_BAND = PERSISTENT && inv_pb_ok<T, L, EP>();
    static constexpr auto plain() { return k_row_inv_pow2<T, L, E>; }
    template <int MODE, bool PB, typename Fn> static void beam_pair(Fn&& f) {
        f(k_row_inv_pow2p<T, L, EP, MODE, false, PB>, MODE, false, PB);
        f(k_row_inv_pow2p<T, L, EP, MODE, true, PB>, MODE, true, PB);
    }
    // the persistent instantiations launch_row_inv can reach: f(kernel, mode, beam, per_band)
    template <typename Fn> static void persistent(Fn&& f) {
        if constexpr (PERSISTENT) {
            beam_pair<0, false>(f);
            beam_pair<1, false>(f);
            beam_pair<2, false>(f);
            if constexpr (PER_BAND) beam_pair<2, true>(f);
        }
    }
    template <typename Fn> static void reachable(Fn&& f) {       // all of them, f(kernel)
        f(plain());
        persistent([&](auto* k, int, bool, bool) { f(k); });
    }
};

// tables and LDS attributes of the row class (T, L)
template <typename T, int L>
static int row_prepare(FastTables* ft) {
    using FK = RowFwdK<T, L>;
    using IK = RowInvK<T, L>;
    int rc;
    if constexpr (FK::PERSISTENT) rc = upload_ptwc<T, L, FK::E>(&ft->tab[PTWC_ROW_FWD]);
    else rc = upload_ptw<T, L, FK::E>(&ft->tab[PTW_ROW]);
    if (rc == PFB_OK) rc = upload_ptwc<T, L, IK::E>(&ft->tab[PTWC_ROW_INV]);
    if constexpr (IK::EP != IK::E) {
        if (rc == PFB_OK) rc = upload_ptwc<T, L, IK::EP>(&ft->tab[PTWC_ROW_INV_P]);
    } else {
        ft->tab[PTWC_ROW_INV_P] = ft->tab[PTWC_ROW_INV];
    }
    FK::reachable([&](auto* k, bool) { if (rc == PFB_OK) rc = set_lds_max(k); });
    IK::reachable([&](auto* k) { if (rc == PFB_OK) rc = set_lds_max(k); });
    return rc;
}

template <typename T, int L>
static int rows_per_wg() { return row_groups<T, L, RowCfg<T, L, true>::E, RowCfg<T, L, true>::GMAX>(); }

static FastDims fast_dims(const pfb_conv_plan* p, size_t xpitch, size_t xband) {
    return FastDims{p->nx, p->ny, p->M, p->T_elems_per_band, p->psf_elems_per_band, xpitch, xband};
}
// w_Q = exp(-2 pi i / Q), Q = 2 ny: the persistent row kernels' odd-bin twiddles are w_M^m w_Q
template <typename T>
static cplx<T> wq1_of(const pfb_conv_plan* p) {
    const long double a = 6.283185307179586476925286766559005768L / (2.0L * (long double)p->ny);
    return cplx<T>((T)cosl(a), (T)(-sinl(a)));
}

// Tbuf: the half-spectrum buffer to fill (the plan's T, or the PSFHAT producer's quadrant scratch: `band0`
// is then the slot); xpitch / xband: elements between rows / bands of x (and beam)
template <typename T, int L>
static int launch_row_fwd(pfb_conv_plan* p, const FastTables* ft, void* Tbuf, int band0, int nb, const void* x,
                          const void* beam, size_t xpitch, size_t xband, hipStream_t st) {
    using K = RowFwdK<T, L>;
    const FastDims d = fast_dims(p, xpitch, xband);
    if constexpr (K::PERSISTENT) {
        // persistent kernel: parities in sequence, next rows requested inside the second transform
        using FP = typename K::FP;
        const int tiles_per_band = p->nx / FP::G, ntiles = tiles_per_band * nb;
        const int grid = ntiles < ft->num_cu ? ntiles : ft->num_cu;            // one resident workgroup per CU
        const cplx<T> wq1 = wq1_of<T>(p);
        K::reachable([&](auto* k, bool bm) {
            if (bm != (beam != nullptr)) return;
            hipLaunchKernelGGL(k, dim3(grid), dim3(FP::NT), FP::LDS, st, (const T*)x,
                               (const T*)beam, (cplx<T>*)Tbuf, (const cplx<T>*)ft->tab[TW_M],
                               (const cplx<T>*)ft->tab[PTWC_ROW_FWD], d, band0, tiles_per_band, ntiles, wq1);
        });
    } else {
        constexpr int E = K::E;
        using F = RegFft<T, L, E, RowCfg<T, L, false>::WAVE>;
        constexpr int G = row_groups<T, L, E, RowCfg<T, L, false>::GMAX>();
        static_assert(ROW_TILE_MAX % G == 0, "pow2_supported: the row tile divides nx");
        const size_t lds = sizeof(cplx<T>) * (size_t)G * (F::LDS_ELEMS + 4);
        hipLaunchKernelGGL(K::plain(), dim3(p->nx / G, nb), dim3(G * F::TPB), lds, st,
                           (const T*)x, (const T*)beam, (cplx<T>*)Tbuf, (const cplx<T>*)p->twQ,
                           (const cplx<T>*)ft->tab[TW_M], (const cplx<T>*)ft->tab[PTW_ROW], d, band0);
    }
    return PFB_OK;
}

template <typename T, int L>
static int launch_row_inv(pfb_conv_plan* p, const FastTables* ft, const ApplyArgs& a) {
    using K = RowInvK<T, L>;
    const FastDims d = fast_dims(p, (size_t)p->ny, (size_t)p->nx * p->ny);
    const int band0 = a.band0, nb = a.nb;
    if constexpr (K::PERSISTENT) {
        // pipelined persistent kernel: inner products only against x itself (+ dot_with2)
        const bool plain_dots = !a.dot_with || (a.dot_with == a.x);
        if (plain_dots && !(a.dot_with2 && !a.dot_with)) {
            using IP = typename K::IP;
            const cplx<T> wq1 = wq1_of<T>(p);
            // the (mode, beam given, pb) instantiation over bands [b0, b0 + nbl) on `grid` workgroups; the operands of
            // band b0 lie `off` elements into x / beam / dot_with2 / out
            auto launch = [&](int mode, bool pb, int b0, int nbl, int grid, size_t off, double* part) {
                K::persistent([&](auto* k, int m, bool bm, bool pbv) {
                    if (m != mode || bm != (a.beam != nullptr) || pbv != pb) return;
                    hipLaunchKernelGGL(k, dim3(grid), dim3(IP::NT), IP::LDS, a.st,
                                       (const cplx<T>*)p->T, (const cplx<T>*)ft->tab[TW_M],
                                       (const cplx<T>*)ft->tab[PTWC_ROW_INV_P], (const T*)a.x + off,
                                       a.beam ? (const T*)a.beam + off : nullptr,
                                       a.dot_with2 ? (const T*)a.dot_with2 + off : nullptr, (T*)a.out + off, part, d,
                                       b0, p->nx / IP::G, p->nx / IP::G * nbl, (T)a.scale, (T)a.sigmainv, wq1);
                });
            };
            const int mode = !a.dot_with ? 0 : !a.dot_with2 ? 1 : 2;
            const int tiles_per_band = p->nx / IP::G, ntiles = tiles_per_band * nb;
            int grid = ntiles < ft->num_cu ? ntiles : ft->num_cu;                  // one resident workgroup per CU
            if (a.per_band && a.dot_with) {
                if constexpr (K::PER_BAND) {
                    if (a.dot_with2) {            // one launch, partials [3][nb][grid]
                        if ((size_t)grid * nb > (size_t)p->nx * p->nband) grid = p->nx * p->nband / nb;   // partials: nx x nband
                        launch(2, true, band0, nb, grid, 0, p->partials);
                        p->last = {grid * nb, grid, grid * nb, grid};
                        return PFB_OK;
                    }
                }
                // the whole-cube kernel once per band (the same launches a band-by-band solve makes): band bl's
                // partials land at [bl][3][grid1]
                const int grid1 = tiles_per_band < ft->num_cu ? tiles_per_band : ft->num_cu;
                const size_t bandel = (size_t)p->nx * p->ny;
                for (int bl = 0; bl < nb; ++bl)
                    launch(mode, false, band0 + bl, 1, grid1, bl * bandel, p->partials + (size_t)bl * 3 * grid1);
                p->last = {grid1 * nb, grid1, grid1, 3 * grid1};
                return PFB_OK;
            }
            p->last = {grid, nb == 1 ? grid : 0, grid, grid};
            launch(mode, false, band0, nb, grid, 0, p->partials);
            return PFB_OK;
        }
    }
    constexpr int E = K::E;
    using F = RegFft<T, L, E, RowCfg<T, L, true>::WAVE>;
    constexpr int G = row_groups<T, L, E, RowCfg<T, L, true>::GMAX>();
    static_assert(ROW_TILE_MAX % G == 0, "pow2_supported: the row tile divides nx");
    const size_t lds = 384 + sizeof(cplx<T>) * ((size_t)((F::PTWC + 1) & ~1) + (size_t)G * (F::LDS_ELEMS + 4) * (InvDb<T, L>::ON ? 2 : 1));
    hipLaunchKernelGGL(K::plain(), dim3(p->nx / G, nb), dim3(G * F::TPB), lds, a.st,
                       (const cplx<T>*)p->T, (const cplx<T>*)p->twQ, (const cplx<T>*)ft->tab[TW_M],
                       (const cplx<T>*)ft->tab[PTWC_ROW_INV], (const T*)a.x, (const T*)a.beam, (const T*)a.dot_with,
                       (const T*)a.dot_with2, (T*)a.out, p->partials, d, band0, (T)a.scale, (T)a.sigmainv);
    return PFB_OK;
}

// The RowPass of a class family; D::each(p, f): f(T{}, std::integral_constant<int, L>) -> int for the plan's type and ny / 2
template <typename D> struct RowPassOf {
    static int prepare(pfb_conv_plan* p, FastTables* ft) {
        return D::each(p, [&](auto t, auto l) { return row_prepare<decltype(t), l()>(ft); });
    }
    static int rows_per_wg(const pfb_conv_plan* p) {
        int g = 0;
        (void)D::each(p, [&](auto t, auto l) { g = pfb::rows_per_wg<decltype(t), l()>(); return PFB_OK; });
        return g;
    }
    static int fwd_launch(pfb_conv_plan* p, const FastTables* ft, void* Tbuf, int band0, int nb, const void* x,
                          const void* beam, size_t xpitch, size_t xband, hipStream_t st) {
        return D::each(p, [&](auto t, auto l) {
            return launch_row_fwd<decltype(t), l()>(p, ft, Tbuf, band0, nb, x, beam, xpitch, xband, st);
        });
    }
    static int inv_launch(pfb_conv_plan* p, const FastTables* ft, const ApplyArgs& a) {
        return D::each(p, [&](auto t, auto l) { return launch_row_inv<decltype(t), l()>(p, ft, a); });
    }
    static constexpr RowPass table = {prepare, rows_per_wg, fwd_launch, inv_launch};
};

// ---------------------------------------------------------------------------------------------- the objects' entry blocks
// (the order in which a class dispatch walks types and lengths is the order in which its object's kernels are instantiated
// and laid out: all of fp32 before fp64 for the rows, length by length for the columns -- kept as the objects were measured)
#if PFB_POW2_PART == 1
// ------------------------------------------------- object 1: the power-of-two rows and the fast path's public entry points
struct for_row_class {
    template <typename T, typename Fn> static int lengths(const pfb_conv_plan* p, Fn& f) {
        int rc = PFB_OK;
        return for_pow2_size(p->ny / 2, [&](auto l) { rc = f(T{}, l); }) ? rc : unsupported_len("ny / 2", p->ny / 2);
    }
    template <typename Fn> static int each(const pfb_conv_plan* p, Fn&& f) {
        return p->dtype == PFB_F32 ? lengths<float>(p, f) : lengths<double>(p, f);
    }
};
const RowPass& row_pass_pow2() { return RowPassOf<for_row_class>::table; }

bool pow2_supported(const pfb_conv_plan* p) {
    const bool f32 = p->dtype == PFB_F32;
    if (p->P != 2 * p->nx || p->Q != 2 * p->ny || p->ny % 2) return false;
    if (!(is_pow2(p->nx) && p->nx >= 64 && p->nx <= 8192) && !mix_col_len(p->nx)) return false;
    // rows: one length-ny/2 complex transform per image row in LDS: 8192 complex64 (ny = 16384) fit, complex128 do not
    if (!(is_pow2(p->ny) && p->ny >= 128 && p->ny <= (f32 ? 16384 : 8192)) && !mix_row_len(p->ny / 2, f32)) return false;
    // the row launchers run nx / G workgroups of G rows, G <= ROW_TILE_MAX a power of two: G must divide nx (this is what
    // keeps nx = 80 out: the shortest rows are tiled 32 to a workgroup)
    return p->nx % ROW_TILE_MAX == 0;
}
int pow2_rows_per_wg(const pfb_conv_plan* p) { return row_pass(p).rows_per_wg(p); }
int pow2_nblocks(const pfb_conv_plan* p) {
    return fast_nblocks(p->ny / 2, p->dtype == PFB_F32 ? FastCfg<float>::NVB : FastCfg<double>::NVB);
}
int pow2_nvb(const pfb_conv_plan* p) {
    return p->dtype == PFB_F32 ? FastCfg<float>::NVB : FastCfg<double>::NVB;
}

template <typename T>
static int prep_tables(pfb_conv_plan* p, FastTables* ft) {
    const int L = p->ny / 2;
    if (int rc = col_pass(p).prepare(p, ft); rc != PFB_OK) return rc;
    if (int rc = row_pass(p).prepare(p, ft); rc != PFB_OK) return rc;
    // twM[n] = exp(-2 pi i n / M), n < L  (M = ny)
    return upload_table<T>(&ft->tab[TW_M], L, [&](cplx<T>* h) {
        const long double two_pi = 6.283185307179586476925286766559005768L;
        for (int n = 0; n < L; ++n) {
            long double a = two_pi * (long double)n / (long double)p->ny;
            h[n] = cplx<T>((T)cosl(a), (T)(-sinl(a)));
        }
    });
}
int pow2_prepare(pfb_conv_plan* p) {
    FastTables* ft = (FastTables*)calloc(1, sizeof(FastTables));
    PFB_REQUIRE(ft != nullptr, PFB_ERR_ALLOC, "pow2_prepare: host alloc failed");
    p->fast_tables = ft;
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
        ft->num_cu = prop.multiProcessorCount;
    if (ft->num_cu <= 0) ft->num_cu = 256;
    return p->dtype == PFB_F32 ? prep_tables<float>(p, ft) : prep_tables<double>(p, ft);
}
void pow2_release(pfb_conv_plan* p) {
    FastTables* ft = (FastTables*)p->fast_tables;
    if (!ft) return;
    if (ft->tab[PTWC_ROW_INV_P] == ft->tab[PTWC_ROW_INV]) ft->tab[PTWC_ROW_INV_P] = nullptr;      // the alias
    for (void* t : ft->tab)
        if (t) (void)hipFree(t);
    free(ft);
    p->fast_tables = nullptr;
}

template <typename T>
static int set_psfhat_t(pfb_conv_plan* p, const void* psfhat, hipStream_t st) {
    const int nv = p->M + 1;
    // the dummy partner of the last even bin (and nothing else) is never written: zero all
    PFB_HIP_CHECK(hipMemsetAsync(p->psf_l, 0, sizeof(cplx<T>) * p->psf_elems_per_band * p->nband, st));
    dim3 grid((nv + 31) / 32, (p->P + 31) / 32, p->nband);
    hipLaunchKernelGGL((k_relayout_psf_pow2<T>), grid, dim3(256), 0, st, (const cplx<T>*)psfhat,
                       (cplx<T>*)p->psf_l, p->P, nv, p->ny / 2, FastCfg<T>::NVB, p->psf_elems_per_band,
                       col_two_level(p->nx));
    PFB_HIP_CHECK(hipGetLastError());
    return PFB_OK;
}
int pow2_set_psfhat(pfb_conv_plan* p, const void* psfhat, hipStream_t st) {
    return p->dtype == PFB_F32 ? set_psfhat_t<float>(p, psfhat, st) : set_psfhat_t<double>(p, psfhat, st);
}

// psfhat = r2c(ifftshift(psf)) with the fast path's own kernels (see k_col_fwd_pow2), band by band:
// four pruned row passes over the PSF quadrants (ifftshift = which quadrant goes where), one forward column pass
// straight into psf_l; psfhat_out (optional) receives the reference's (P, M+1) layout.  Synchronous (plan time).
template <typename T>
static int set_psf_t(pfb_conv_plan* p, const void* psf, void* psfhat_out, hipStream_t st) {
    const FastTables* ft = (const FastTables*)p->fast_tables;
    const int nx = p->nx, ny = p->ny, P = p->P, Q = p->Q, L = ny / 2;
    void* Tq = nullptr;
    if (hipMalloc(&Tq, sizeof(cplx<T>) * 4 * p->T_elems_per_band) != hipSuccess) {
        set_error("pow2_set_psf: device allocation failed (%zu B)", sizeof(cplx<T>) * 4 * p->T_elems_per_band);
        return PFB_ERR_ALLOC;
    }
    int rc = PFB_OK;
    for (int band = 0; band < p->nband && rc == PFB_OK; ++band) {
        const T* pb = (const T*)psf + (size_t)band * P * Q;
        for (int q = 0; q < 4 && rc == PFB_OK; ++q) {
            // quadrant (a, b) of the SHIFTED PSF = quadrant (1 - a, 1 - b) of the centred one
            const int a = q >> 1, b = q & 1;
            const T* src = pb + (size_t)((1 - a) * nx) * Q + (size_t)(1 - b) * ny;
            rc = row_pass(p).fwd_launch(p, ft, Tq, q, 1, src, nullptr, (size_t)Q, (size_t)0, st);
        }
        if (rc == PFB_OK) rc = col_pass(p).fwd_launch(p, ft, Tq, band, st);
    }
    if (rc == PFB_OK && psfhat_out) {
        const int nv = p->M + 1;
        dim3 grid((nv + 31) / 32, (P + 31) / 32, p->nband);
        hipLaunchKernelGGL((k_unrelayout_psf_pow2<T>), grid, dim3(256), 0, st, (const cplx<T>*)p->psf_l,
                           (cplx<T>*)psfhat_out, P, nv, L, FastCfg<T>::NVB, p->psf_elems_per_band, col_two_level(nx));
    }
    if (rc == PFB_OK && (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess)) {
        set_error("pow2_set_psf: kernel launch failed");
        rc = PFB_ERR_HIP;
    }
    (void)hipFree(Tq);
    return rc;
}
int pow2_set_psf(pfb_conv_plan* p, const void* psf, void* psfhat_out, hipStream_t st) {
    return p->dtype == PFB_F32 ? set_psf_t<float>(p, psf, psfhat_out, st) : set_psf_t<double>(p, psf, psfhat_out, st);
}

// forward rows, columns, inverse rows: each axis through its seam
int pow2_apply(pfb_conv_plan* p, const ApplyArgs& a) {
    const FastTables* ft = (const FastTables*)p->fast_tables;
    const RowPass& rows = row_pass(p);
    prof_mark(p, a.st, 0);
    if (int rc = rows.fwd_launch(p, ft, p->T, a.band0, a.nb, a.x, a.beam, (size_t)p->ny, (size_t)p->nx * p->ny, a.st); rc != PFB_OK)
        return rc;
    prof_mark(p, a.st, 1);
    if (int rc = col_pass(p).launch(p, ft, a.band0, a.nb, a.st); rc != PFB_OK) return rc;
    prof_mark(p, a.st, 2);
    if (int rc = rows.inv_launch(p, ft, a); rc != PFB_OK) return rc;
    prof_mark(p, a.st, 3);
    PFB_HIP_CHECK(hipGetLastError());
    return PFB_OK;
}

#if PFB_STAMP
// diagnostic build only: buf = 3 * 1024 * PFB_STAMP_ITS * 16 device uint64 (NULL switches the stamps off); this object's
// copy of g_stamp_buf and the column object's
int pow2_col_set_stamp(unsigned long long* buf);
extern "C" int pfb_debug_set_stamps(void* buf) {
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_buf), &buf, sizeof(buf)) != hipSuccess) return PFB_ERR_HIP;
    return pow2_col_set_stamp((unsigned long long*)buf);
}
#endif

#elif PFB_POW2_PART == 2
// ------------------------------------------------- object 2: the power-of-two columns
struct for_col_class {
    template <typename Fn> static int each(const pfb_conv_plan* p, Fn&& f) {
        int rc = PFB_OK;
        const bool ok = for_pow2_size(p->nx, [&](auto h) { rc = p->dtype == PFB_F32 ? f(float{}, h) : f(double{}, h); });
        return ok ? rc : unsupported_len("nx", p->nx);
    }
};
const ColPass& col_pass_pow2() { return ColPassOf<for_col_class>::table; }

#if PFB_STAMP
int pow2_col_set_stamp(unsigned long long* buf) {
    return hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_buf), &buf, sizeof(buf)) == hipSuccess ? PFB_OK : PFB_ERR_HIP;
}
#endif

#elif PFB_POW2_PART == 3
// ------------------------------------------------- object 3: the columns and rows of the lengths 3 2^k and 5 2^k
// The classes are those of for_mix_size; a class is described by the same ColCfg / ColKernels / RowFwdK / RowInvK as a
// power-of-two one (every one of them Plain / not PERSISTENT by construction) and launched by the same templates.
// f(T{}, std::integral_constant<int, N>) -> int for the plan's type and axis length; rows: fp64 up to mix_row_max only
template <bool ROWS> struct for_mix_class {
    template <typename Fn> static int each(const pfb_conv_plan* p, Fn&& f) {
        const bool f32 = p->dtype == PFB_F32;
        const int n = ROWS ? p->ny / 2 : p->nx;
        int rc = PFB_OK;
        bool ok = false;                                  // stays where (type, n) has no class
        for_mix_size(n, [&](auto c) {
            constexpr int N = decltype(c)::value;
            auto plain = [&](auto t) {
                using T = decltype(t);
                if constexpr (ROWS)
                    static_assert(!RowFwdK<T, N>::PERSISTENT && !RowInvK<T, N>::PERSISTENT && !RowInvK<T, N>::PER_BAND, "plain row kernels");
                else
                    static_assert(ColCfg<T, N>::KIND == ColKind::Plain && !col_two_level(N), "plain column kernel");
                ok = true;
                return f(t, c);
            };
            if constexpr (ROWS) {
                if (f32) rc = plain(float{});
                else if constexpr (N <= mix_row_max(false)) rc = plain(double{});
            } else if constexpr (N >= MIX_COL_MIN) {
                rc = f32 ? plain(float{}) : plain(double{});
            }
        });
        return ok ? rc : unsupported_len(ROWS ? "ny / 2" : "nx", n);
    }
};
const ColPass& col_pass_mix() { return ColPassOf<for_mix_class<false>>::table; }
const RowPass& row_pass_mix() { return RowPassOf<for_mix_class<true>>::table; }

#else
#error "PFB_POW2_PART must be 1, 2 or 3 (csrc/Makefile: FLAGS_fftconv_pow2 / _col / _mix)"
#endif

}  // namespace pfb
