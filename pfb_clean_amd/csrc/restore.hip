// restore.hip -- Gaussian restoring-beam kernels: what pfb/utils/misc.py:109-138 (Gaussian2D) and :186-238
// (convolve2gaussres) compute before and between their FFTs.  The convolution itself is the library's own
// (PsfConvPlan.from_psf / pfb_psfconv_apply); these kernels only PRODUCE its kernel, once per beam (plan time):
//   k_gauss2d        Gaussian2D on caller coordinates, batched over parameter sets, with a deterministic fp64 sum
//   k_kernel_gather  the (P, Q)-periodic padded kernel gathered onto the grid the convolution plan wants -- from the
//                    analytic Gaussian (the padded kernel never exists in memory) or from an array
//   k_kernhat_ratio  where(|den| > 0, num / den, 0): the ratio of kernel spectra of the `gausspari` branch
// Everything is fp64 whatever the image dtype, like the reference (Gaussian2D returns float64, the kernel spectra are
// complex128); only the gathered kernel is written in the plan's dtype.
//
// No FMA contraction in this file: `x*x + y*y <= extent` must take numpy's decision pixel by pixel (the zero pattern
// of the truncated kernel is part of the result), and the quadratic form / complex division round like numpy's.
#pragma clang fp contract(off)
#include "common.hpp"

namespace pfb {

constexpr int RS_BLOCK = 256;
constexpr int RS_MAX_GRID = 1024;
// 2 sqrt(2 ln 2), misc.py:130 (GaussPar holds FWHMs)
constexpr double FWHM_CONV = 2.3548200450309493;

// one parameter set: the entries of R^T A R (misc.py:114-120) and the truncation radius squared (misc.py:123)
struct GaussSet { double a00, a01, a11, extent; };

__device__ __forceinline__ double gauss_value(double x, double y, const GaussSet g) {
    if (!(x * x + y * y <= g.extent)) return 0.0;
    const double q = g.a00 * x * x + 2.0 * g.a01 * x * y + g.a11 * y * y;
    return exp(-FWHM_CONV * q);
}

// grid (G, nset): out[s, i] = gauss(xx[i], yy[i]; pars[s]) (out may be null: sums only); ws[s * G + block] = block sum
__global__ void __launch_bounds__(RS_BLOCK)
k_gauss2d(const double* __restrict__ xx, const double* __restrict__ yy, size_t npix,
          const GaussSet* __restrict__ pars, double* __restrict__ out, double* __restrict__ ws) {
    __shared__ double red[RS_BLOCK / 64];
    const int s = blockIdx.y;
    const GaussSet g = pars[s];
    double acc[1] = {0.0};
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (size_t)gridDim.x * blockDim.x) {
        const double v = gauss_value(xx[i], yy[i], g);
        if (out) out[(size_t)s * npix + i] = v;
        acc[0] += v;
    }
    block_sum<1>(acc, red);
    if (threadIdx.x == 0) ws[(size_t)s * gridDim.x + blockIdx.x] = acc[0];
}

// grid (nset): sums[s] = sum_g ws[s * G + g] in a fixed order
__global__ void __launch_bounds__(RS_BLOCK)
k_gauss_sum(const double* __restrict__ ws, int G, double* __restrict__ sums) {
    __shared__ double red[RS_BLOCK / 64];
    const int s = blockIdx.x;
    double acc[1] = {0.0};
    for (int g = threadIdx.x; g < G; g += blockDim.x) acc[0] += ws[(size_t)s * G + g];
    block_sum<1>(acc, red);
    if (threadIdx.x == 0) sums[s] = acc[0];
}

// grid (G, nset): out[s, i] /= sums[s]   (misc.py:135-136, a division like the reference's)
__global__ void __launch_bounds__(RS_BLOCK)
k_gauss_scale(double* __restrict__ out, size_t npix, const double* __restrict__ sums) {
    const int s = blockIdx.y;
    const double d = sums[s];
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (size_t)gridDim.x * blockDim.x)
        out[(size_t)s * npix + i] /= d;
}

// floor modulo for |a| that may exceed n
__device__ __forceinline__ int pmod(int a, int n) {
    const int r = a % n;
    return r < 0 ? r + n : r;
}

struct GatherGeom {
    int nx, ny;          // image (and coordinate array) shape
    int P, Q;            // the periodic source grid
    int cx, cy;          // source index of the kernel's centre
    int P2, Q2;          // output grid, centre at (P2/2, Q2/2)
    int clip;            // keep only the offsets |dx| < nx, |dy| < ny
};

// One thread per output element, grid (ceil(Q2 / block), P2, nset); out[s, i, j] with offsets dx = i - P2/2,
// dy = j - Q2/2 takes the source at ((cx + dx) mod P, (cy + dy) mod Q).
//   ANALYTIC: the source is pad(Gaussian2D(xx, yy, pars[s])) with (padx, pady) zeros in front (misc.py:211):
//             padded index (u, v) is pixel (u - padx, v - pady) of the coordinate arrays, zero in the padding;
//             norm (nullable): the sums the values are divided by (normalise=True)
//   else:     src is (nset, P, Q) fp64
template <typename T, bool ANALYTIC>
__global__ void __launch_bounds__(RS_BLOCK)
k_kernel_gather(GatherGeom g, int padx, int pady, const double* __restrict__ xx, const double* __restrict__ yy,
                const GaussSet* __restrict__ pars, const double* __restrict__ norm,
                const double* __restrict__ src, T* __restrict__ out) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= g.Q2) return;
    const int i = blockIdx.y, s = blockIdx.z;
    const int dx = i - g.P2 / 2, dy = j - g.Q2 / 2;
    double v = 0.0;
    const bool keep = !g.clip || (dx > -g.nx && dx < g.nx && dy > -g.ny && dy < g.ny);
    if (keep) {
        const int u = pmod(g.cx + dx, g.P), w = pmod(g.cy + dy, g.Q);
        if constexpr (ANALYTIC) {
            const int px = u - padx, py = w - pady;
            if (px >= 0 && px < g.nx && py >= 0 && py < g.ny) {
                const size_t k = (size_t)px * g.ny + py;
                v = gauss_value(xx[k], yy[k], pars[s]);
                if (norm) v /= norm[s];
            }
        } else {
            v = src[((size_t)s * g.P + u) * g.Q + w];
        }
    }
    out[((size_t)s * g.P2 + i) * g.Q2 + j] = (T)v;
}

// out[b, i] = |den[b, i]| > 0 ? num[i] / den[b, i] : 0   (misc.py:229-231).  |z| > 0 exactly as numpy decides it:
// hypot(re, im) >= max(|re|, |im|), so it is zero only when both parts are.  The quotient is numpy's (Smith's
// algorithm, scaled by the larger part of the denominator).
__global__ void __launch_bounds__(RS_BLOCK)
k_kernhat_ratio(const double2* __restrict__ num, const double2* __restrict__ den, size_t n, double2* __restrict__ out) {
    const int b = blockIdx.y;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const double2 a = num[i], d = den[(size_t)b * n + i];
        double2 r = {0.0, 0.0};
        if (d.x != 0.0 || d.y != 0.0) {
            if (fabs(d.x) >= fabs(d.y)) {
                const double rat = d.y / d.x, scl = 1.0 / (d.x + d.y * rat);
                r.x = (a.x + a.y * rat) * scl;
                r.y = (a.y - a.x * rat) * scl;
            } else {
                const double rat = d.x / d.y, scl = 1.0 / (d.y + d.x * rat);
                r.x = (a.x * rat + a.y) * scl;
                r.y = (a.y * rat - a.x) * scl;
            }
        }
        out[(size_t)b * n + i] = r;
    }
}

static inline int stream_grid(size_t n, int cap) {
    size_t g = (n + RS_BLOCK - 1) / RS_BLOCK;
    if (g < 1) g = 1;
    if (g > (size_t)cap) g = cap;
    return (int)g;
}

static int check_geom(const char* who, const GatherGeom& g, int nset) {
    PFB_REQUIRE(nset >= 1 && nset <= 65535, PFB_ERR_INVALID, "%s: nset %d outside 1..65535", who, nset);
    PFB_REQUIRE(g.nx >= 1 && g.ny >= 1 && g.P >= g.nx && g.Q >= g.ny, PFB_ERR_INVALID,
                "%s: source grid (%d,%d) smaller than the image (%d,%d)", who, g.P, g.Q, g.nx, g.ny);
    PFB_REQUIRE(g.P2 >= 1 && g.P2 <= 65535 && g.Q2 >= 1, PFB_ERR_INVALID, "%s: output grid (%d,%d) out of range", who,
                g.P2, g.Q2);
    if (g.clip)
        PFB_REQUIRE(g.P2 >= 2 * g.nx - 1 && g.Q2 >= 2 * g.ny - 1, PFB_ERR_INVALID,
                    "%s: output grid (%d,%d) does not hold the offsets of a (%d,%d) image", who, g.P2, g.Q2, g.nx, g.ny);
    else
        PFB_REQUIRE(g.P2 == g.P && g.Q2 == g.Q, PFB_ERR_INVALID,
                    "%s: without clipping the output grid must be the source grid", who);
    return PFB_OK;
}

template <typename T, bool ANALYTIC>
static int gather_launch(const GatherGeom& g, int padx, int pady, const double* xx, const double* yy,
                         const GaussSet* pars, const double* norm, const double* src, int nset, void* out,
                         hipStream_t st) {
    const dim3 grid((g.Q2 + RS_BLOCK - 1) / RS_BLOCK, g.P2, nset);
    hipLaunchKernelGGL((k_kernel_gather<T, ANALYTIC>), grid, dim3(RS_BLOCK), 0, st, g, padx, pady, xx, yy, pars, norm,
                       src, (T*)out);
    PFB_HIP_CHECK(hipGetLastError());
    return PFB_OK;
}

}  // namespace pfb

using namespace pfb;

extern "C" {

int pfb_gauss2d(const double* xx, const double* yy, size_t npix, const double* pars, int nset, int normalise,
                double* out, double* sums, double* ws, void* stream) {
    PFB_REQUIRE(xx && yy && pars && ws && (out || sums), PFB_ERR_INVALID, "gauss2d: null argument");
    PFB_REQUIRE(!normalise || (out && sums), PFB_ERR_INVALID, "gauss2d: normalise needs out and sums");
    PFB_REQUIRE(npix >= 1 && nset >= 1 && nset <= PFB_REDUCE_WS_DOUBLES, PFB_ERR_INVALID,
                "gauss2d: npix %zu / nset %d out of range", npix, nset);
    hipStream_t st = as_stream(stream);
    int cap = PFB_REDUCE_WS_DOUBLES / nset;              // nset * G partial sums fit the scratch
    if (cap > RS_MAX_GRID) cap = RS_MAX_GRID;
    const int G = stream_grid((npix + 3) / 4, cap);
    hipLaunchKernelGGL(k_gauss2d, dim3(G, nset), dim3(RS_BLOCK), 0, st, xx, yy, npix, (const GaussSet*)pars, out, ws);
    if (sums) hipLaunchKernelGGL(k_gauss_sum, dim3(nset), dim3(RS_BLOCK), 0, st, ws, G, sums);
    if (normalise) hipLaunchKernelGGL(k_gauss_scale, dim3(G, nset), dim3(RS_BLOCK), 0, st, out, npix, sums);
    PFB_HIP_CHECK(hipGetLastError());
    return PFB_OK;
}

int pfb_gauss_kernel_grid(int dtype, const double* xx, const double* yy, int nx, int ny, int npad_xl, int npad_yl,
                          int nx_pad, int ny_pad, const double* pars, const double* norm, int nset, int clip,
                          int nx_out, int ny_out, void* out, void* stream) {
    PFB_REQUIRE(xx && yy && pars && out, PFB_ERR_INVALID, "gauss_kernel_grid: null argument");
    PFB_REQUIRE(dtype == PFB_F32 || dtype == PFB_F64, PFB_ERR_INVALID, "gauss_kernel_grid: bad dtype %d", dtype);
    const GatherGeom g{nx, ny, nx_pad, ny_pad, nx_pad / 2, ny_pad / 2, nx_out, ny_out, clip ? 1 : 0};
    if (int rc = check_geom("gauss_kernel_grid", g, nset)) return rc;
    PFB_REQUIRE(npad_xl >= 0 && npad_yl >= 0 && npad_xl + nx <= nx_pad && npad_yl + ny <= ny_pad, PFB_ERR_INVALID,
                "gauss_kernel_grid: padding (%d,%d) puts the (%d,%d) image outside the (%d,%d) grid", npad_xl, npad_yl,
                nx, ny, nx_pad, ny_pad);
    const GaussSet* ps = (const GaussSet*)pars;
    return dtype == PFB_F32
        ? gather_launch<float, true>(g, npad_xl, npad_yl, xx, yy, ps, norm, nullptr, nset, out, as_stream(stream))
        : gather_launch<double, true>(g, npad_xl, npad_yl, xx, yy, ps, norm, nullptr, nset, out, as_stream(stream));
}

int pfb_kernel_gather(int dtype, const double* kern, int nband, int nx, int ny, int nx_pad, int ny_pad, int cx, int cy,
                      int nx_out, int ny_out, void* out, void* stream) {
    PFB_REQUIRE(kern && out, PFB_ERR_INVALID, "kernel_gather: null argument");
    PFB_REQUIRE(dtype == PFB_F32 || dtype == PFB_F64, PFB_ERR_INVALID, "kernel_gather: bad dtype %d", dtype);
    const GatherGeom g{nx, ny, nx_pad, ny_pad, cx, cy, nx_out, ny_out, 1};
    if (int rc = check_geom("kernel_gather", g, nband)) return rc;
    PFB_REQUIRE(cx >= 0 && cx < nx_pad && cy >= 0 && cy < ny_pad, PFB_ERR_INVALID,
                "kernel_gather: centre (%d,%d) outside the (%d,%d) grid", cx, cy, nx_pad, ny_pad);
    return dtype == PFB_F32
        ? gather_launch<float, false>(g, 0, 0, nullptr, nullptr, nullptr, nullptr, kern, nband, out, as_stream(stream))
        : gather_launch<double, false>(g, 0, 0, nullptr, nullptr, nullptr, nullptr, kern, nband, out, as_stream(stream));
}

int pfb_kernhat_ratio(const void* num, const void* den, int nband, size_t n, void* out, void* stream) {
    PFB_REQUIRE(num && den && out, PFB_ERR_INVALID, "kernhat_ratio: null argument");
    PFB_REQUIRE(nband >= 1 && nband <= 65535 && n >= 1, PFB_ERR_INVALID, "kernhat_ratio: nband %d / n %zu out of range",
                nband, n);
    hipLaunchKernelGGL(k_kernhat_ratio, dim3(stream_grid((n + 3) / 4, 4096), nband), dim3(RS_BLOCK), 0, as_stream(stream),
                       (const double2*)num, (const double2*)den, n, (double2*)out);
    PFB_HIP_CHECK(hipGetLastError());
    return PFB_OK;
}

}  // extern "C"
