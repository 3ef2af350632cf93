// comps.hip -- the component model: what pfb/utils/misc.py:1084-1313 (fit_image_cube, eval_coeffs_to_cube,
// eval_coeffs_to_slice) do on image-sized arrays.  The design matrix, its LU factors, the basis values and the
// coordinate arrays are tiny and come from the host (utils/comps.py); these kernels do the rest:
//   k_pixmask        (pixmask.hpp, with the rule AnyNonzero) one pass over the (nplane, npix) cube: np.any over the
//                    planes as a bit mask (one 64-bit word per 64 pixels) and the number of set bits per workgroup
//   k_count_scan     (pixmask.hpp) exclusive scan of the workgroup counts, the total behind them (one workgroup)
//   k_comps_compact  Ix, Iy in row-major order (np.where) from the mask, the scanned offsets and a popcount
//   k_comps_fit      one component per lane: gather, rhs = (Xfit^T diag(w)) beta, LU substitution, all fp64
//   k_comps_eval     scatter of sum_p E[plane][p] coeffs[p][c] to (Ix[c], Iy[c])
//   k_comps_interp   RegularGridInterpolator(method='linear') of a rendered plane, np.pad read as zeros
//
// No FMA contraction in this file: the interpolation must take scipy's weights on grid-aligned points (a distance of
// exactly 0 or 1 returns the corner value itself), and the dot products round like numpy's multiply-then-add.
#pragma clang fp contract(off)
#include "pixmask.hpp"

namespace pfb {

constexpr int CP_FIT_BLOCK = 64;
constexpr int CP_MAX_ROWS = 64;
constexpr int CP_MAX_PARAMS = 32;

// The mask rule of np.any: a pixel is set iff any plane value != 0, compared in T: NaN counts, -0.0 does not.  The
// aligned form streams with a wave's iterations unrolled and the planes by 8.
struct AnyNonzero {
    static constexpr int NCUBE = 1, PLANE_UNROLL = 8;
    static constexpr bool START = false, HAS_MAX = false, UNROLL_ITS = true;
    template <typename T> __device__ __forceinline__ T value(T e, T) const { return e; }
    template <typename T> __device__ __forceinline__ bool update(bool flag, T x) const { return flag | (x != (T)0); }
};

// same ownership of words as k_pixmask; pixel q = 64 word + bit is component offs[g] + (set bits before it in the
// workgroup's words), i.e. components are numbered in pixel order: the order of np.where on the (nx, ny) mask
__global__ void __launch_bounds__(CP_BLOCK)
k_comps_compact(const u64* __restrict__ mask, const i64* __restrict__ offs, size_t nwords, i64 ny,
                i64* __restrict__ Ix, i64* __restrict__ Iy) {
    __shared__ u64 words[CP_WORDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t w0 = (size_t)blockIdx.x * CP_WORDS;
    if (threadIdx.x < CP_WORDS) words[threadIdx.x] = w0 + threadIdx.x < nwords ? mask[w0 + threadIdx.x] : 0;
    __syncthreads();
    i64 base = offs[blockIdx.x];
    for (int j = 0; j < wave * CP_WAVE_WORDS; ++j) base += __popcll(words[j]);
#pragma unroll
    for (int k = 0; k < CP_WAVE_WORDS; ++k) {
        const int j = wave * CP_WAVE_WORDS + k;
        const u64 bits = words[j];
        if ((bits >> lane) & 1) {
            const i64 pos = base + __popcll(bits & ((1ull << lane) - 1));
            const i64 q = (i64)((w0 + j) * 64 + lane);
            Ix[pos] = q / ny;
            Iy[pos] = q % ny;
        }
        base += __popcll(bits);
    }
}

// One component per lane, one wave per workgroup.  sys = [A (nparam, nrow) | LU (nparam, nparam) | piv (nparam)], all
// doubles, is staged in LDS, followed by the lanes' vectors v[p][lane]: every dynamically indexed array lives in LDS.
// LU / piv are LAPACK getrf's (unit lower triangle below the diagonal; row i was exchanged with row piv[i], in order).
template <typename T>
__global__ void __launch_bounds__(CP_FIT_BLOCK)
k_comps_fit(const T* __restrict__ img, int nrow, size_t npix, i64 ny, const i64* __restrict__ Ix,
            const i64* __restrict__ Iy, i64 ncomps, const double* __restrict__ sys, int nparam,
            double* __restrict__ coeffs) {
    extern __shared__ double cp_lds[];
    const int nsys = nparam * nrow + nparam * nparam + nparam;
    for (int i = threadIdx.x; i < nsys; i += CP_FIT_BLOCK) cp_lds[i] = sys[i];
    __syncthreads();
    const double* A = cp_lds;
    const double* LU = A + nparam * nrow;
    const double* piv = LU + nparam * nparam;
    const int lane = threadIdx.x;
    double* v = cp_lds + nsys + lane;                         // v[p * CP_FIT_BLOCK]
    const i64 c = (i64)blockIdx.x * CP_FIT_BLOCK + lane;
    if (c >= ncomps) return;
    const size_t q = (size_t)(Ix[c] * ny + Iy[c]);
    for (int p = 0; p < nparam; ++p) v[p * CP_FIT_BLOCK] = 0.0;
    for (int r = 0; r < nrow; ++r) {
        const double b = (double)img[(size_t)r * npix + q];
        for (int p = 0; p < nparam; ++p) v[p * CP_FIT_BLOCK] += A[p * nrow + r] * b;
    }
    for (int i = 0; i < nparam; ++i) {
        const int pi = (int)piv[i];
        if (pi != i) {
            const double t = v[i * CP_FIT_BLOCK];
            v[i * CP_FIT_BLOCK] = v[pi * CP_FIT_BLOCK];
            v[pi * CP_FIT_BLOCK] = t;
        }
    }
    for (int i = 1; i < nparam; ++i) {
        double s = v[i * CP_FIT_BLOCK];
        for (int j = 0; j < i; ++j) s -= LU[i * nparam + j] * v[j * CP_FIT_BLOCK];
        v[i * CP_FIT_BLOCK] = s;
    }
    for (int i = nparam - 1; i >= 0; --i) {
        double s = v[i * CP_FIT_BLOCK];
        for (int j = i + 1; j < nparam; ++j) s -= LU[i * nparam + j] * v[j * CP_FIT_BLOCK];
        v[i * CP_FIT_BLOCK] = s / LU[i * nparam + i];
    }
    for (int p = 0; p < nparam; ++p) coeffs[(size_t)p * ncomps + c] = v[p * CP_FIT_BLOCK];
}

// grid (ceil(ncomps / block), nplane): out[plane, Ix[c], Iy[c]] = sum_p E[plane, p] coeffs[p, c]; a component outside
// the (nx, ny) plane is skipped
template <typename TO>
__global__ void __launch_bounds__(CP_BLOCK)
k_comps_eval(const double* __restrict__ E, const double* __restrict__ coeffs, const i64* __restrict__ Ix,
             const i64* __restrict__ Iy, i64 ncomps, int nparam, i64 nx, i64 ny, TO* __restrict__ out) {
    const i64 c = (i64)blockIdx.x * CP_BLOCK + threadIdx.x;
    if (c >= ncomps) return;
    const int plane = blockIdx.y;
    const i64 ix = Ix[c], iy = Iy[c];
    if (ix < 0 || ix >= nx || iy < 0 || iy >= ny) return;
    double acc = 0.0;
    for (int p = 0; p < nparam; ++p) acc += E[(size_t)plane * nparam + p] * coeffs[(size_t)p * ncomps + c];
    out[((size_t)plane * nx + ix) * ny + iy] = (TO)acc;
}

// np.searchsorted(grid, x) - 1 clipped to [0, n - 2]
__device__ __forceinline__ int interval(const double* __restrict__ grid, int n, double x) {
    int lo = 0, hi = n;                        // first index with grid[index] >= x
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (grid[mid] < x) lo = mid + 1; else hi = mid;
    }
    int i = lo - 1;
    if (i < 0) i = 0;
    if (i > n - 2) i = n - 2;
    return i;
}

struct InterpGeom {
    int nxi, nyi;        // the stored plane
    int padx, pady;      // zeros np.pad puts in front of it
    int nxp, nyp;        // lengths of the (padded) coordinate arrays
    int nxo, nyo;
};

// grid (ceil(nyo / block), min(nxo, 65535)): scipy's _evaluate_linear on the padded plane, which is never stored
template <typename TO>
__global__ void __launch_bounds__(CP_BLOCK)
k_comps_interp(const double* __restrict__ img, InterpGeom g, const double* __restrict__ xin,
               const double* __restrict__ yin, const double* __restrict__ xo, const double* __restrict__ yo,
               TO* __restrict__ out) {
    const int j = blockIdx.x * CP_BLOCK + threadIdx.x;
    if (j >= g.nyo) return;
    const double y = yo[j];
    const int jj = interval(yin, g.nyp, y);
    const double dy = (y - yin[jj]) / (yin[jj + 1] - yin[jj]);
    for (int i = blockIdx.y; i < g.nxo; i += gridDim.y) {
        const double x = xo[i];
        const int ii = interval(xin, g.nxp, x);
        const double dx = (x - xin[ii]) / (xin[ii + 1] - xin[ii]);
        auto at = [&](int a, int b) -> double {
            a -= g.padx;
            b -= g.pady;
            return (a >= 0 && a < g.nxi && b >= 0 && b < g.nyi) ? img[(size_t)a * g.nyi + b] : 0.0;
        };
        double val = 0.0;
        val = val + at(ii, jj) * ((1.0 - dx) * (1.0 - dy));
        val = val + at(ii, jj + 1) * ((1.0 - dx) * dy);
        val = val + at(ii + 1, jj) * (dx * (1.0 - dy));
        val = val + at(ii + 1, jj + 1) * (dx * dy);
        out[(size_t)i * g.nyo + j] = (TO)val;
    }
}

}  // namespace pfb

using namespace pfb;

extern "C" {

size_t pfb_comps_work_bytes(size_t npix) {
    if (npix < 1 || npix > CP_MAX_PIX) return 0;
    return 8 * (comps_nwords(npix) + comps_nblocks(npix) + 1);
}

int pfb_comps_mask(int dtype, const void* image, int nplane, size_t npix, void* work, void* stream) {
    return pixmask_run("comps_mask", AnyNonzero{}, INT_MAX, dtype, image, nullptr, nplane, npix, work, stream);
}

int pfb_comps_compact(size_t npix, int ny, const void* work, long long* Ix, long long* Iy, void* stream) {
    PFB_REQUIRE(work && Ix && Iy, PFB_ERR_INVALID, "comps_compact: null argument");
    PFB_REQUIRE(npix >= 1 && npix <= CP_MAX_PIX && ny >= 1 && npix % (size_t)ny == 0, PFB_ERR_INVALID,
                "comps_compact: npix %zu is not a multiple of ny %d", npix, ny);
    const u64* mask = (const u64*)work;
    const i64* offs = (const i64*)work + comps_nwords(npix);
    hipLaunchKernelGGL(k_comps_compact, dim3((unsigned)comps_nblocks(npix)), dim3(CP_BLOCK), 0, as_stream(stream), mask,
                       offs, comps_nwords(npix), (i64)ny, Ix, Iy);
    PFB_HIP_CHECK(hipGetLastError());
    return PFB_OK;
}

int pfb_comps_fit(int dtype, const void* image, int nrow, size_t npix, int ny, const long long* Ix, const long long* Iy,
                  long long ncomps, const double* sys, int nparam, double* coeffs, void* stream) {
    PFB_REQUIRE(dtype == PFB_F32 || dtype == PFB_F64, PFB_ERR_INVALID, "comps_fit: bad dtype %d", dtype);
    PFB_REQUIRE(nrow >= 1 && nparam >= 1 && ncomps >= 0 && ny >= 1 && npix >= 1, PFB_ERR_INVALID,
                "comps_fit: nrow %d / nparam %d / ncomps %lld / npix %zu out of range", nrow, nparam, ncomps, npix);
    PFB_REQUIRE(nrow <= CP_MAX_ROWS && nparam <= CP_MAX_PARAMS, PFB_ERR_UNSUPPORTED,
                "comps_fit: nrow %d / nparam %d beyond the supported %d / %d", nrow, nparam, CP_MAX_ROWS, CP_MAX_PARAMS);
    if (ncomps == 0) return PFB_OK;
    PFB_REQUIRE(image && Ix && Iy && sys && coeffs, PFB_ERR_INVALID, "comps_fit: null argument");
    PFB_REQUIRE(ncomps <= (long long)npix, PFB_ERR_INVALID, "comps_fit: %lld components in %zu pixels", ncomps, npix);
    const size_t lds = sizeof(double) * ((size_t)nparam * nrow + (size_t)nparam * nparam + nparam +
                                         (size_t)nparam * CP_FIT_BLOCK);
    const dim3 grid((unsigned)((ncomps + CP_FIT_BLOCK - 1) / CP_FIT_BLOCK));
    hipStream_t st = as_stream(stream);
    if (dtype == PFB_F32)
        hipLaunchKernelGGL(k_comps_fit<float>, grid, dim3(CP_FIT_BLOCK), lds, st, (const float*)image, nrow, npix,
                           (i64)ny, Ix, Iy, ncomps, sys, nparam, coeffs);
    else
        hipLaunchKernelGGL(k_comps_fit<double>, grid, dim3(CP_FIT_BLOCK), lds, st, (const double*)image, nrow, npix,
                           (i64)ny, Ix, Iy, ncomps, sys, nparam, coeffs);
    PFB_HIP_CHECK(hipGetLastError());
    return PFB_OK;
}

int pfb_comps_eval(int dtype, const double* E, int nplane, int nparam, const double* coeffs, const long long* Ix,
                   const long long* Iy, long long ncomps, int nx, int ny, void* out, void* stream) {
    PFB_REQUIRE(out && E, PFB_ERR_INVALID, "comps_eval: null argument");
    PFB_REQUIRE(dtype == PFB_F32 || dtype == PFB_F64, PFB_ERR_INVALID, "comps_eval: bad dtype %d", dtype);
    PFB_REQUIRE(nplane >= 1 && nplane <= 65535 && nparam >= 1 && nx >= 1 && ny >= 1 && ncomps >= 0, PFB_ERR_INVALID,
                "comps_eval: nplane %d / nparam %d / shape (%d,%d) / ncomps %lld out of range", nplane, nparam, nx, ny,
                ncomps);
    hipStream_t st = as_stream(stream);
    const size_t n = (size_t)nplane * nx * ny;
    PFB_HIP_CHECK(hipMemsetAsync(out, 0, n * (dtype == PFB_F32 ? 4 : 8), st));
    if (ncomps == 0) return PFB_OK;
    PFB_REQUIRE(coeffs && Ix && Iy, PFB_ERR_INVALID, "comps_eval: null argument");
    const dim3 grid((unsigned)((ncomps + CP_BLOCK - 1) / CP_BLOCK), nplane);
    if (dtype == PFB_F32)
        hipLaunchKernelGGL(k_comps_eval<float>, grid, dim3(CP_BLOCK), 0, st, E, coeffs, Ix, Iy, ncomps, nparam, (i64)nx,
                           (i64)ny, (float*)out);
    else
        hipLaunchKernelGGL(k_comps_eval<double>, grid, dim3(CP_BLOCK), 0, st, E, coeffs, Ix, Iy, ncomps, nparam, (i64)nx,
                           (i64)ny, (double*)out);
    PFB_HIP_CHECK(hipGetLastError());
    return PFB_OK;
}

int pfb_comps_interp(int dtype, const double* image, int nxi, int nyi, int npad_xl, int npad_yl, const double* xin,
                     int nx_pad, const double* yin, int ny_pad, const double* xo, int nxo, const double* yo, int nyo,
                     void* out, void* stream) {
    PFB_REQUIRE(image && xin && yin && xo && yo && out, PFB_ERR_INVALID, "comps_interp: null argument");
    PFB_REQUIRE(dtype == PFB_F32 || dtype == PFB_F64, PFB_ERR_INVALID, "comps_interp: bad dtype %d", dtype);
    PFB_REQUIRE(nxi >= 1 && nyi >= 1 && npad_xl >= 0 && npad_yl >= 0 && nx_pad >= npad_xl + nxi &&
                ny_pad >= npad_yl + nyi, PFB_ERR_INVALID,
                "comps_interp: padding (%d,%d) puts the (%d,%d) plane outside the (%d,%d) grid", npad_xl, npad_yl, nxi,
                nyi, nx_pad, ny_pad);
    PFB_REQUIRE(nx_pad >= 2 && ny_pad >= 2 && nxo >= 1 && nyo >= 1, PFB_ERR_INVALID,
                "comps_interp: grid (%d,%d) / output (%d,%d) out of range", nx_pad, ny_pad, nxo, nyo);
    const InterpGeom g{nxi, nyi, npad_xl, npad_yl, nx_pad, ny_pad, nxo, nyo};
    const dim3 grid((nyo + CP_BLOCK - 1) / CP_BLOCK, nxo < 65535 ? nxo : 65535);
    hipStream_t st = as_stream(stream);
    if (dtype == PFB_F32)
        hipLaunchKernelGGL(k_comps_interp<float>, grid, dim3(CP_BLOCK), 0, st, image, g, xin, yin, xo, yo, (float*)out);
    else
        hipLaunchKernelGGL(k_comps_interp<double>, grid, dim3(CP_BLOCK), 0, st, image, g, xin, yin, xo, yo,
                           (double*)out);
    PFB_HIP_CHECK(hipGetLastError());
    return PFB_OK;
}

}  // extern "C"
