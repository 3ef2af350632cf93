// cycle.hip -- what the workers' major-cycle loops do between the solver calls (pfb/workers/klean.py:190-339,
// spotless.py:155-363, fluxmop.py:129-199): the band sum of a cube with the statistics that set the threshold and the
// stopping test, the mop mask, and the masked right-hand side / start point / beam of the flux mop.
//   k_bandsum_stats        one streaming pass over the (nband, nset, npix) cube: per pixel the band sum in the cube's
//                          dtype and band order (np.sum(axis=0)), written out on request; per set and workgroup the
//                          moments (count, mean, M2) of the sums over the quiet pixels (no model band != 0) in fp64 and
//                          the NaN-propagating max |sum| over all pixels
//   k_bandsum_stats_final  the workgroups' partials of a set in a fixed order -> the set's record
//   k_mask_close           support of a cube (any band != 0, or > a threshold) or a given uint8 mask, one binary
//                          dilation and one erosion by the 5-point cross or the full 3 x 3, a tile with a 2-pixel halo
//                          in LDS; outside the image is 0 in both steps (scipy's border_value=0)
//   k_masked_problem       beam_eff = beam * mask, b = beam_eff * residual, x0 = mask ? seed : 0 in one pass
//
// The moments are never formed as sum x, sum x^2: a thread accumulates sum (x - K), sum (x - K)^2 about a pivot K, its
// own first quiet value, which leaves differences of the size of the spread however far the mean is from zero.  Threads,
// waves, workgroups and the final launch merge (n, mean, M2) with
//     M2 = M2a + M2b + d^2 na nb / (na + nb),   mean = mean_a + d nb / (na + nb),   d = mean_b - mean_a,
// always lower index on the left: the same input gives the same bits.  A partial with n == 0 is the identity.
//
// The 16-byte forms need every plane on a 16-byte boundary (npix a multiple of the vector width and aligned bases);
// anything else (odd npix in fp32, a base offset by 1-3 elements) runs the same kernels one element per lane.
//
// No FMA contraction in this file: the products of k_masked_problem and the band sums round like numpy's.
#pragma clang fp contract(off)
#include "common.hpp"

namespace pfb {

typedef unsigned char u8;

constexpr int CY_BLOCK = 256;
constexpr int CY_WAVES = CY_BLOCK / 64;
constexpr int CY_REC = PFB_CYCLE_RECORD;
// workgroups per set of the statistics pass: one pack per thread up to here, a grid-stride loop beyond.  A constant, not
// a multiple of the CU count, because pfb_cycle_work_bytes sizes the partials on the host from nset alone; 1024 is 4
// workgroups per CU of an MI355X.  Measured with a model, 8 x 4096^2 fp32 / 2 x 8192^2 fp64: 1024 with the
// band loops unrolled by 4 streams 5.27 / 5.50 TB/s, 2048 with unroll 8 4.69 / 4.75
constexpr int CY_MAX_GRID = 1024;
constexpr int CY_MAX_SETS = 65535;
constexpr size_t CY_MAX_PIX = (size_t)1 << 40;
// output tile of the closing, rows x columns.  tests/golden/make_golden_cycle.py (TILE_ROWS, TILE_COLS) places its
// "either side of the tile edge" cases by these two numbers: change them together
constexpr int MC_TH = 32, MC_TW = 64;
constexpr int MP_MAX_GRID = 4096;

struct Mom { double n, mean, m2; };

__device__ __forceinline__ Mom mom_merge(const Mom& a, const Mom& b) {
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    const double n = a.n + b.n, d = b.mean - a.mean;
    return {n, a.mean + d * (b.n / n), a.m2 + b.m2 + (d * d) * (a.n * b.n / n)};
}
__device__ __forceinline__ Mom mom_shfl_down(const Mom& a, int off) {
    return {__shfl_down(a.n, off, 64), __shfl_down(a.mean, off, 64), __shfl_down(a.m2, off, 64)};
}

// ndarray.max's combination: a NaN on either side wins
template <typename T>
__device__ __forceinline__ T nanmax(T a, T b) { return (b > a || b != b) ? b : a; }

static inline int cy_grid(size_t nvec) {
    const size_t g = (nvec + CY_BLOCK - 1) / CY_BLOCK;
    return (int)(g < 1 ? 1 : (g > (size_t)CY_MAX_GRID ? CY_MAX_GRID : g));
}

// grid (G, nset).  x[(band * nset + set) * npix + p]; model[band * npix + p] (nset == 1 only) or NULL; sum_out
// [set * npix + p] or NULL.  A thread takes the packs i = its global index, + G * CY_BLOCK, ...; part[(set * G + g) * 4]
// = (n, mean, M2, max |sum|) of workgroup g.
template <typename T, int V>
__global__ void __launch_bounds__(CY_BLOCK)
k_bandsum_stats(const T* __restrict__ x, int nband, int nset, size_t npix, const T* __restrict__ model, int nband_m,
                T* __restrict__ sum_out, double* __restrict__ part) {
    __shared__ Mom wmom[CY_WAVES];
    __shared__ T wmax[CY_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int set = blockIdx.y;
    const size_t nvec = npix / V;                           // V > 1 only when npix % V == 0
    const size_t bstride = (size_t)nset * npix;
    const T* xs = x + (size_t)set * npix;
    T* so = sum_out ? sum_out + (size_t)set * npix : nullptr;
    const size_t stride = (size_t)gridDim.x * CY_BLOCK;
    double K = 0.0, n = 0.0, s1 = 0.0, s2 = 0.0;
    T amax = (T)0;
    for (size_t i = (size_t)blockIdx.x * CY_BLOCK + threadIdx.x; i < nvec; i += stride) {
        Pack<T, V> s = ld_nt<T, V>(xs, i);
#pragma unroll 4
        for (int b = 1; b < nband; ++b) {
            const Pack<T, V> v = ld_nt<T, V>(xs + (size_t)b * bstride, i);
#pragma unroll
            for (int k = 0; k < V; ++k) s.e[k] = s.e[k] + v.e[k];
        }
        bool loud[V];
#pragma unroll
        for (int k = 0; k < V; ++k) loud[k] = false;
#pragma unroll 4
        for (int b = 0; b < nband_m; ++b) {
            const Pack<T, V> v = ld_nt<T, V>(model + (size_t)b * npix, i);
#pragma unroll
            for (int k = 0; k < V; ++k) loud[k] |= (v.e[k] != (T)0);
        }
        if (so) st<T, V>(so, i, s);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            amax = nanmax(amax, (T)fabs(s.e[k]));
            if (!loud[k]) {
                const double d = (double)s.e[k];
                K = n == 0.0 ? d : K;
                const double e = d - K;
                n += 1.0;
                s1 += e;
                s2 += e * e;
            }
        }
    }
    Mom m = {0.0, 0.0, 0.0};
    if (n > 0.0) {
        const double v = s2 - s1 * (s1 / n);
        m = {n, K + s1 / n, v < 0.0 ? 0.0 : v};
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        m = mom_merge(m, mom_shfl_down(m, off));
        amax = nanmax(amax, __shfl_down(amax, off, 64));
    }
    if (lane == 0) {
        wmom[wave] = m;
        wmax[wave] = amax;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        Mom r = wmom[0];
        T a = wmax[0];
#pragma unroll
        for (int w = 1; w < CY_WAVES; ++w) {
            r = mom_merge(r, wmom[w]);
            a = nanmax(a, wmax[w]);
        }
        double* p = part + CY_REC * ((size_t)set * gridDim.x + blockIdx.x);
        p[0] = r.n;
        p[1] = r.mean;
        p[2] = r.m2;
        p[3] = (double)a;
    }
}

// grid (nset), one wave: lane l merges the partials g = l, l + 64, ... in order, then the shuffle tree
__global__ void __launch_bounds__(64)
k_bandsum_stats_final(const double* __restrict__ part, int G, double* __restrict__ out) {
    const int set = blockIdx.x;
    const double* p = part + CY_REC * (size_t)set * G;
    Mom m = {0.0, 0.0, 0.0};
    double a = 0.0;
    for (int g = threadIdx.x; g < G; g += 64) {
        m = mom_merge(m, Mom{p[CY_REC * g], p[CY_REC * g + 1], p[CY_REC * g + 2]});
        a = nanmax(a, p[CY_REC * g + 3]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        m = mom_merge(m, mom_shfl_down(m, off));
        a = nanmax(a, __shfl_down(a, off, 64));
    }
    if (threadIdx.x == 0) {
        double* r = out + CY_REC * (size_t)set;
        r[0] = m.n;
        r[1] = m.mean;
        r[2] = m.m2;
        r[3] = a;
    }
}

// S = float / double: a (nband, nx, ny) cube, a pixel is in the support iff any band != 0 (a NaN counts, -0.0 does
// not), or iff any band > thr when above != 0 (a NaN does not count).  S = u8: a mask, nband = 1, in iff != 0.
template <typename S>
__device__ __forceinline__ u8 in_support(const S* __restrict__ src, int nband, size_t npix, size_t q, int above, S thr) {
    bool on = false;
    for (int b = 0; b < nband; ++b) {
        const S v = src[(size_t)b * npix + q];
        on |= above ? (v > thr) : (v != (S)0);
    }
    return on ? 1 : 0;
}

// grid (ceil(ny / MC_TW), ceil(nx / MC_TH)).  sup: the support on the tile grown by 2 pixels, dil: its dilation on the
// tile grown by 1; both are 0 outside the image, so a pixel whose structure reaches outside never survives the erosion.
// conn <= 0: the support itself; 1: the cross; >= 2: the full 3 x 3.
template <typename S>
__global__ void __launch_bounds__(CY_BLOCK)
k_mask_close(const S* __restrict__ src, int nband, int nx, int ny, int above, S thr, int conn, u8* __restrict__ out) {
    constexpr int SH = MC_TH + 4, SW = MC_TW + 4, DH = MC_TH + 2, DW = MC_TW + 2;
    __shared__ u8 sup[SH][SW];
    __shared__ u8 dil[DH][DW];
    const size_t npix = (size_t)nx * ny;
    const long long i0 = (long long)blockIdx.y * MC_TH, j0 = (long long)blockIdx.x * MC_TW;
    for (int idx = threadIdx.x; idx < SH * SW; idx += CY_BLOCK) {
        const int r = idx / SW, c = idx % SW;
        const long long i = i0 - 2 + r, j = j0 - 2 + c;
        u8 v = 0;
        if (i >= 0 && i < nx && j >= 0 && j < ny) v = in_support<S>(src, nband, npix, (size_t)i * ny + (size_t)j, above, thr);
        sup[r][c] = v;
    }
    __syncthreads();
    if (conn <= 0) {
        for (int idx = threadIdx.x; idx < MC_TH * MC_TW; idx += CY_BLOCK) {
            const int r = idx / MC_TW, c = idx % MC_TW;
            const long long i = i0 + r, j = j0 + c;
            if (i < nx && j < ny) out[(size_t)i * ny + (size_t)j] = sup[r + 2][c + 2];
        }
        return;
    }
    const bool full = conn >= 2;
    for (int idx = threadIdx.x; idx < DH * DW; idx += CY_BLOCK) {
        const int r = idx / DW, c = idx % DW;
        const long long i = i0 - 1 + r, j = j0 - 1 + c;
        u8 v = 0;
        if (i >= 0 && i < nx && j >= 0 && j < ny) {
            const int a = r + 1, b = c + 1;                 // the same pixel in sup
            v = sup[a][b] | sup[a - 1][b] | sup[a + 1][b] | sup[a][b - 1] | sup[a][b + 1];
            if (full) v |= sup[a - 1][b - 1] | sup[a - 1][b + 1] | sup[a + 1][b - 1] | sup[a + 1][b + 1];
        }
        dil[r][c] = v;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < MC_TH * MC_TW; idx += CY_BLOCK) {
        const int r = idx / MC_TW, c = idx % MC_TW;
        const long long i = i0 + r, j = j0 + c;
        if (i >= nx || j >= ny) continue;
        const int a = r + 1, b = c + 1;                     // the same pixel in dil
        u8 v = dil[a][b] & dil[a - 1][b] & dil[a + 1][b] & dil[a][b - 1] & dil[a][b + 1];
        if (full) v &= dil[a - 1][b - 1] & dil[a - 1][b + 1] & dil[a + 1][b - 1] & dil[a + 1][b + 1];
        out[(size_t)i * ny + (size_t)j] = v;
    }
}

// V mask bytes from byte offset i * V (aligned to V on the 16-byte path) as 0 / 1 flags
template <int V>
__device__ __forceinline__ void ld_mask(const u8* __restrict__ mask, size_t i, bool (&on)[V]) {
    if constexpr (V == 1) {
        on[0] = mask[i] != 0;
    } else if constexpr (V == 2) {
        const unsigned short w = reinterpret_cast<const unsigned short*>(mask)[i];
        on[0] = (w & 0xFFu) != 0;
        on[1] = (w >> 8) != 0;
    } else {
        static_assert(V == 4, "16-byte packs of double or float");
        const unsigned w = reinterpret_cast<const unsigned*>(mask)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) on[k] = ((w >> (8 * k)) & 0xFFu) != 0;
    }
}

// grid (G).  A thread keeps the mask and the seed of its pack and walks the bands: one read of the residual and the beam,
// one write of each output that is asked for.  beam: nbeam = nband or 1 planes, or NULL; beam_eff has nbe planes (nbeam
// with a beam, 1 without).
template <typename T, int V>
__global__ void __launch_bounds__(CY_BLOCK)
k_masked_problem(const T* __restrict__ res, const u8* __restrict__ mask, const T* __restrict__ beam, int nbeam,
                 const T* __restrict__ seed, int nband, size_t npix, T* __restrict__ b, T* __restrict__ x0,
                 T* __restrict__ beam_eff, int nbe) {
    const size_t nvec = npix / V;
    const size_t stride = (size_t)gridDim.x * CY_BLOCK;
    const int nwalk = (b || x0) ? nband : nbe;              // beam_eff alone: only its own planes
    for (size_t i = (size_t)blockIdx.x * CY_BLOCK + threadIdx.x; i < nvec; i += stride) {
        bool on[V];
        ld_mask<V>(mask, i, on);
        Pack<T, V> mk, sd;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            mk.e[k] = on[k] ? (T)1 : (T)0;
            sd.e[k] = (T)0;
        }
        if (seed && x0) {
            const Pack<T, V> s = ld<T, V>(seed, i);
#pragma unroll
            for (int k = 0; k < V; ++k) sd.e[k] = on[k] ? s.e[k] : (T)0;
        }
        for (int band = 0; band < nwalk; ++band) {
            const size_t off = (size_t)band * npix;
            Pack<T, V> be = mk;
            if (beam) {
                const Pack<T, V> bm = ld<T, V>(beam + (nbeam == 1 ? 0 : off), i);
#pragma unroll
                for (int k = 0; k < V; ++k) be.e[k] = bm.e[k] * mk.e[k];
            }
            if (beam_eff && band < nbe) st<T, V>(beam_eff + off, i, be);
            if (b) {
                const Pack<T, V> r = ld_nt<T, V>(res + off, i);
                Pack<T, V> o;
#pragma unroll
                for (int k = 0; k < V; ++k) o.e[k] = be.e[k] * r.e[k];
                st<T, V>(b + off, i, o);
            }
            if (x0) st<T, V>(x0 + off, i, sd);
        }
    }
}

static bool cy_elem_aligned(const void* p, int dtype) { return (uintptr_t)p % (dtype == PFB_F32 ? 4 : 8) == 0; }

template <typename T>
static void launch_bandsum(const void* x, int nband, int nset, size_t npix, const void* model, int nband_m, void* sum_out,
                           double* part, double* out, hipStream_t st) {
    constexpr int V = V16<T>::N;
    const bool vec = can_vec<T>(npix, {x, model, sum_out});
    const int G = cy_grid(vec ? npix / V : npix);
    const dim3 grid(G, nset);
    if (vec)
        hipLaunchKernelGGL((k_bandsum_stats<T, V>), grid, dim3(CY_BLOCK), 0, st, (const T*)x, nband, nset, npix,
                           (const T*)model, nband_m, (T*)sum_out, part);
    else
        hipLaunchKernelGGL((k_bandsum_stats<T, 1>), grid, dim3(CY_BLOCK), 0, st, (const T*)x, nband, nset, npix,
                           (const T*)model, nband_m, (T*)sum_out, part);
    hipLaunchKernelGGL(k_bandsum_stats_final, dim3(nset), dim3(64), 0, st, part, G, out);
}

template <typename S>
static void launch_close(const void* src, int nband, int nx, int ny, int above, double thr, int conn, u8* out,
                         hipStream_t st) {
    const dim3 grid((ny + MC_TW - 1) / MC_TW, (nx + MC_TH - 1) / MC_TH);
    hipLaunchKernelGGL(k_mask_close<S>, grid, dim3(CY_BLOCK), 0, st, (const S*)src, nband, nx, ny, above, (S)thr, conn,
                       out);
}

template <typename T>
static void launch_masked(const void* res, const u8* mask, const void* beam, int nbeam, const void* seed, int nband,
                          size_t npix, void* b, void* x0, void* beam_eff, hipStream_t st) {
    constexpr int V = V16<T>::N;
    const bool vec = can_vec<T>(npix, {res, beam, seed, b, x0, beam_eff}) && (uintptr_t)mask % V == 0;
    const size_t nvec = vec ? npix / V : npix;
    size_t g = (nvec + CY_BLOCK - 1) / CY_BLOCK;
    g = g < 1 ? 1 : (g > (size_t)MP_MAX_GRID ? MP_MAX_GRID : g);
    const int nbe = beam ? nbeam : 1;
    if (vec)
        hipLaunchKernelGGL((k_masked_problem<T, V>), dim3((unsigned)g), dim3(CY_BLOCK), 0, st, (const T*)res, mask,
                           (const T*)beam, nbeam, (const T*)seed, nband, npix, (T*)b, (T*)x0, (T*)beam_eff, nbe);
    else
        hipLaunchKernelGGL((k_masked_problem<T, 1>), dim3((unsigned)g), dim3(CY_BLOCK), 0, st, (const T*)res, mask,
                           (const T*)beam, nbeam, (const T*)seed, nband, npix, (T*)b, (T*)x0, (T*)beam_eff, nbe);
}

}  // namespace pfb

using namespace pfb;

extern "C" {

size_t pfb_cycle_work_bytes(int nset) {
    if (nset < 1 || nset > CY_MAX_SETS) return 0;
    return 8 * (size_t)CY_REC * CY_MAX_GRID * (size_t)nset;
}

int pfb_bandsum_stats(int dtype, const void* x, int nband, int nset, size_t npix, const void* model, int nband_m,
                      void* sum_out, void* work, double* out, void* stream) {
    PFB_REQUIRE(x && work && out, PFB_ERR_INVALID, "bandsum_stats: null argument");
    PFB_REQUIRE(dtype == PFB_F32 || dtype == PFB_F64, PFB_ERR_INVALID, "bandsum_stats: bad dtype %d", dtype);
    PFB_REQUIRE(nband >= 1 && nset >= 1 && nset <= CY_MAX_SETS && npix >= 1 && npix <= CY_MAX_PIX, PFB_ERR_INVALID,
                "bandsum_stats: nband %d / nset %d / npix %zu out of range", nband, nset, npix);
    PFB_REQUIRE(model ? (nset == 1 && nband_m >= 1) : true, PFB_ERR_INVALID,
                "bandsum_stats: a model needs nset == 1 (got %d) and nband_m >= 1 (got %d)", nset, nband_m);
    PFB_REQUIRE(((uintptr_t)work & 7u) == 0 && ((uintptr_t)out & 7u) == 0, PFB_ERR_INVALID,
                "bandsum_stats: work and out must be 8-byte aligned");
    PFB_REQUIRE(cy_elem_aligned(x, dtype) && cy_elem_aligned(model, dtype) && cy_elem_aligned(sum_out, dtype),
                PFB_ERR_INVALID, "bandsum_stats: an array is not aligned to its element size");
    hipStream_t st = as_stream(stream);
    if (!model) nband_m = 0;
    if (dtype == PFB_F32)
        launch_bandsum<float>(x, nband, nset, npix, model, nband_m, sum_out, (double*)work, out, st);
    else
        launch_bandsum<double>(x, nband, nset, npix, model, nband_m, sum_out, (double*)work, out, st);
    PFB_HIP_CHECK(hipGetLastError());
    return PFB_OK;
}

int pfb_mask_close(int dtype, const void* cube, int nband, const unsigned char* mask, int nx, int ny, int has_min,
                   double min_value, int connectivity, unsigned char* out, void* stream) {
    PFB_REQUIRE(out && ((cube != nullptr) != (mask != nullptr)), PFB_ERR_INVALID,
                "mask_close: exactly one of cube and mask, and an output");
    PFB_REQUIRE(nx >= 1 && ny >= 1 && (size_t)nx * ny <= CY_MAX_PIX && (nx + MC_TH - 1) / MC_TH <= 65535,
                PFB_ERR_INVALID, "mask_close: shape (%d,%d) out of range", nx, ny);
    hipStream_t st = as_stream(stream);
    if (mask) {
        PFB_REQUIRE(mask != out, PFB_ERR_INVALID, "mask_close: out must not be the input mask");
        launch_close<u8>(mask, 1, nx, ny, 0, 0.0, connectivity, out, st);
    } else {
        PFB_REQUIRE(dtype == PFB_F32 || dtype == PFB_F64, PFB_ERR_INVALID, "mask_close: bad dtype %d", dtype);
        PFB_REQUIRE(nband >= 1, PFB_ERR_INVALID, "mask_close: nband %d out of range", nband);
        PFB_REQUIRE(cy_elem_aligned(cube, dtype), PFB_ERR_INVALID, "mask_close: cube is not aligned to its element size");
        if (dtype == PFB_F32)
            launch_close<float>(cube, nband, nx, ny, has_min != 0, min_value, connectivity, out, st);
        else
            launch_close<double>(cube, nband, nx, ny, has_min != 0, min_value, connectivity, out, st);
    }
    PFB_HIP_CHECK(hipGetLastError());
    return PFB_OK;
}

int pfb_masked_problem(int dtype, const void* residual, const unsigned char* mask, const void* beam, int nband_beam,
                       const void* seed, int nband, size_t npix, void* b, void* x0, void* beam_eff, void* stream) {
    PFB_REQUIRE(mask && (residual || !b), PFB_ERR_INVALID, "masked_problem: null mask, or b without a residual");
    PFB_REQUIRE(dtype == PFB_F32 || dtype == PFB_F64, PFB_ERR_INVALID, "masked_problem: bad dtype %d", dtype);
    PFB_REQUIRE(nband >= 1 && npix >= 1 && npix <= CY_MAX_PIX, PFB_ERR_INVALID,
                "masked_problem: nband %d / npix %zu out of range", nband, npix);
    PFB_REQUIRE(!beam || nband_beam == 1 || nband_beam == nband, PFB_ERR_INVALID,
                "masked_problem: a beam of %d bands for a cube of %d", nband_beam, nband);
    for (const void* p : {residual, beam, seed, (const void*)b, (const void*)x0, (const void*)beam_eff})
        PFB_REQUIRE(cy_elem_aligned(p, dtype), PFB_ERR_INVALID, "masked_problem: an array is not aligned to its element size");
    if (!b && !x0 && !beam_eff) return PFB_OK;
    hipStream_t st = as_stream(stream);
    if (dtype == PFB_F32)
        launch_masked<float>(residual, mask, beam, nband_beam, seed, nband, npix, b, x0, beam_eff, st);
    else
        launch_masked<double>(residual, mask, beam, nband_beam, seed, nband, npix, b, x0, beam_eff, st);
    PFB_HIP_CHECK(hipGetLastError());
    return PFB_OK;
}

}  // extern "C"
