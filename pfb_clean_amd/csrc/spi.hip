// spi.hip -- spectral index and reference-flux maps: what pfb/utils/spi.py (fit_spi) does on image-sized arrays, with
// the per-component Gauss-Newton fit of m_b = I0 B_b x_b^alpha it hands to fit_spi_components.  The host keeps ln x_b,
// w_b and the reference band (utils/spi.py); these kernels do the rest:
//   k_pixmask    (pixmask.hpp, with the rule CutAbove) one pass over image and beam, (nband, npix) each: the beam cut,
//                amin over the bands > threshold as a bit mask, the set bits per workgroup and the workgroup's
//                NaN-propagating maximum of the cut image
//   k_count_scan (pixmask.hpp) exclusive scan of the workgroup counts with the total behind them, and the maximum of
//                the partial maxima (one workgroup)
//   k_spi_fit    one component per lane: Gauss-Newton on (alpha, I0), then the errors at the returned parameters, all
//                fp64; CUBE: gather by (Ix, Iy) with the cut applied on load, scatter into the four maps; else a dense
//                (ncomps, nband) list in, (4, ncomps) out
// Ix, Iy come from pfb_comps_compact (comps.hip), which reads the same work layout.
#include "pixmask.hpp"

namespace pfb {

constexpr int SPI_FIT_BLOCK = 256;
constexpr int SPI_MAX_BANDS = 64;
constexpr unsigned SPI_FIT_MAX_GRID = 1u << 20;             // workgroups; beyond it a lane takes several components

// The mask rule of fit_spi.  Per pixel and band the cut value is c = beam > pb_min ? image : 0 (a NaN beam fails),
// compared in fp64; the pixel is set iff every band's c > threshold (a NaN c fails: np.amin propagates it), and the
// maximum of c is kept for the empty-mask message.  Both loops stay rolled: the planes unrolled by 4 measured slower
// (DESIGN 4.9).
struct CutAbove {
    double pb_min, threshold;
    static constexpr int NCUBE = 2, PLANE_UNROLL = 1;
    static constexpr bool START = true, HAS_MAX = true, UNROLL_ITS = false;
    template <typename T> __device__ __forceinline__ double value(T image, T beam) const {
        return (double)beam > pb_min ? (double)image : 0.0;
    }
    __device__ __forceinline__ bool update(bool flag, double cut) const { return flag && (cut > threshold); }
};

struct SpiFitArgs {
    // CUBE: image / beam (nband, npix) of T, Ix / Iy, maps (4, npix) of T
    // list: data (ncomps, nband) doubles, beam the same shape or null (= 1), alphai / I0i (ncomps) or null,
    //       out (4, ncomps) doubles
    const void* data;
    const void* beam;
    const i64* Ix;
    const i64* Iy;
    const double* alphai;
    const double* I0i;
    void* out;
    u64* notconv;
    i64 ncomps;
    i64 npix, ny;
    double pb_min, tol;
    int nband, ref, maxiter;
};

// ln x_b and w_b travel in the kernel arguments: b is wave-uniform, so they are read with wave-uniform loads from the
// argument segment and nothing is uploaded for them
struct SpiBands { double lnx[SPI_MAX_BANDS], w[SPI_MAX_BANDS]; };

// The normal equations of one component at (alpha, I0), bands in ascending order.  `at(b, d, B)` fetches the datum
// and the beam value of band b: the 2 nband inputs are re-read on every call (through L2), nothing
// per-lane is indexed at run time.
struct SpiNormal { double h00, h01, h11, g0, g1, chi2; };

template <typename At>
__device__ __forceinline__ SpiNormal spi_normal(const SpiBands& bands, int nband, double alpha, double I0,
                                                At at) {
    SpiNormal s{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < nband; ++b) {
        const double lnx = bands.lnx[b], w = bands.w[b];
        double d, B;
        at(b, d, B);
        const double j1 = B * exp(alpha * lnx);
        const double j0 = I0 * j1 * lnx;
        const double r = d - I0 * j1;
        s.h00 += w * j0 * j0;
        s.h01 += w * j0 * j1;
        s.h11 += w * j1 * j1;
        s.g0 += w * j0 * r;
        s.g1 += w * j1 * r;
        s.chi2 += w * r * r;
    }
    return s;
}

template <typename T, bool CUBE>
__global__ void __launch_bounds__(SPI_FIT_BLOCK)
k_spi_fit(const SpiFitArgs a, const SpiBands bands) {
    const int nband = a.nband;
    const T* __restrict__ data = (const T*)a.data;
    const T* __restrict__ beam = (const T*)a.beam;
    const double dof = nband > 2 ? (double)(nband - 2) : 1.0;
    int late = 0;
    for (i64 c = (i64)blockIdx.x * SPI_FIT_BLOCK + threadIdx.x; c < a.ncomps; c += (i64)gridDim.x * SPI_FIT_BLOCK) {
        i64 base, stride;
        if constexpr (CUBE) {
            base = a.Ix[c] * a.ny + a.Iy[c];
            stride = a.npix;
        } else {
            base = c * (i64)nband;
            stride = 1;
        }
        auto at = [&](int b, double& d, double& B) {
            const i64 i = base + (i64)b * stride;
            if constexpr (CUBE) {
                B = (double)beam[i];
                d = B > a.pb_min ? (double)data[i] : 0.0;
            } else {
                B = beam ? (double)beam[i] : 1.0;
                d = (double)data[i];
            }
        };
        double alpha = -0.7, I0, B0;
        at(a.ref, I0, B0);
        if constexpr (!CUBE) {
            if (a.alphai) alpha = a.alphai[c];
            if (a.I0i) I0 = a.I0i[c];
        }
        double eps = 1.0;
        int k = 0;
        bool dead = false;
        while (eps > a.tol && k < a.maxiter) {
            const SpiNormal s = spi_normal(bands, nband, alpha, I0, at);
            const double det = s.h00 * s.h11 - s.h01 * s.h01;
            if (!__builtin_isfinite(det) || det == 0.0) {
                dead = true;
                break;
            }
            const double da = (s.h11 * s.g0 - s.h01 * s.g1) / det;
            const double di = (-s.h01 * s.g0 + s.h00 * s.g1) / det;
            alpha += da;
            I0 += di;
            eps = fmax(fabs(da), fabs(di));
            if (da != da || di != di) eps = NAN;                 // fmax drops a NaN; the loop must end on one
            ++k;
        }
        double r0 = NAN, r1 = NAN, r2 = NAN, r3 = NAN;
        if (!dead) {
            const SpiNormal s = spi_normal(bands, nband, alpha, I0, at);
            const double det = s.h00 * s.h11 - s.h01 * s.h01;
            if (__builtin_isfinite(det) && det != 0.0) {
                r0 = alpha;
                r1 = sqrt(s.h11 / det * s.chi2 / dof);
                r2 = I0;
                r3 = sqrt(s.h00 / det * s.chi2 / dof);
            }
            late += (k >= a.maxiter);
        }
        T* __restrict__ out = (T*)a.out;
        const i64 o = CUBE ? base : c, os = CUBE ? a.npix : a.ncomps;
        out[o] = (T)r0;
        out[o + os] = (T)r1;
        out[o + 2 * os] = (T)r2;
        out[o + 3 * os] = (T)r3;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) late += __shfl_down(late, off, 64);
    if ((threadIdx.x & 63) == 0 && late) atomicAdd(a.notconv, (u64)late);
}

static inline unsigned spi_fit_grid(long long ncomps) {
    const long long g = (ncomps + SPI_FIT_BLOCK - 1) / SPI_FIT_BLOCK;
    return (unsigned)(g < (long long)SPI_FIT_MAX_GRID ? g : (long long)SPI_FIT_MAX_GRID);
}

}  // namespace pfb

using namespace pfb;

extern "C" {

size_t pfb_spi_work_bytes(size_t npix) {
    if (npix < 1 || npix > CP_MAX_PIX) return 0;
    return 8 * (comps_nwords(npix) + 2 * comps_nblocks(npix) + 2);
}

int pfb_spi_mask(int dtype, const void* image, const void* beam, int nband, size_t npix, double pb_min, double threshold,
                 void* work, void* stream) {
    return pixmask_run("spi_mask", CutAbove{pb_min, threshold}, SPI_MAX_BANDS, dtype, image, beam, nband, npix, work,
                       stream);
}

static int spi_fit_check(const char* who, int nband, int ref, long long ncomps, double tol, int maxiter,
                         const double* lnx, const double* w, SpiBands& bands) {
    PFB_REQUIRE(nband >= 1 && ref >= 0 && ref < nband && ncomps >= 0 && maxiter >= 0 && tol == tol, PFB_ERR_INVALID,
                "%s: nband %d / ref %d / ncomps %lld / maxiter %d / tol %g out of range", who, nband, ref, ncomps,
                maxiter, tol);
    PFB_REQUIRE(nband <= SPI_MAX_BANDS, PFB_ERR_UNSUPPORTED, "%s: %d bands beyond the supported %d", who, nband,
                SPI_MAX_BANDS);
    PFB_REQUIRE(lnx && w, PFB_ERR_INVALID, "%s: null argument", who);
    memset(&bands, 0, sizeof(bands));
    memcpy(bands.lnx, lnx, sizeof(double) * nband);
    memcpy(bands.w, w, sizeof(double) * nband);
    return PFB_OK;
}

int pfb_spi_fit(int dtype, const void* image, const void* beam, int nband, size_t npix, int ny, const long long* Ix,
                const long long* Iy, long long ncomps, const double* lnx, const double* w, int ref, double pb_min, double tol,
                int maxiter, void* maps, long long* notconv, void* stream) {
    PFB_REQUIRE(dtype == PFB_F32 || dtype == PFB_F64, PFB_ERR_INVALID, "spi_fit: bad dtype %d", dtype);
    SpiBands bands;
    if (int rc = spi_fit_check("spi_fit", nband, ref, ncomps, tol, maxiter, lnx, w, bands)) return rc;
    PFB_REQUIRE(npix >= 1 && npix <= CP_MAX_PIX && ny >= 1 && npix % (size_t)ny == 0, PFB_ERR_INVALID,
                "spi_fit: npix %zu is not a multiple of ny %d", npix, ny);
    PFB_REQUIRE(ncomps <= (long long)npix, PFB_ERR_INVALID, "spi_fit: %lld components in %zu pixels", ncomps, npix);
    PFB_REQUIRE(notconv, PFB_ERR_INVALID, "spi_fit: null argument");
    hipStream_t st = as_stream(stream);
    PFB_HIP_CHECK(hipMemsetAsync(notconv, 0, 8, st));
    if (ncomps == 0) return PFB_OK;
    PFB_REQUIRE(image && beam && Ix && Iy && maps, PFB_ERR_INVALID, "spi_fit: null argument");
    const SpiFitArgs a{image, beam, Ix, Iy, nullptr, nullptr, maps, (u64*)notconv, ncomps, (i64)npix, (i64)ny,
                       pb_min, tol, nband, ref, maxiter};
    const dim3 grid(spi_fit_grid(ncomps));
    if (dtype == PFB_F32) hipLaunchKernelGGL((k_spi_fit<float, true>), grid, dim3(SPI_FIT_BLOCK), 0, st, a, bands);
    else                  hipLaunchKernelGGL((k_spi_fit<double, true>), grid, dim3(SPI_FIT_BLOCK), 0, st, a, bands);
    PFB_HIP_CHECK(hipGetLastError());
    return PFB_OK;
}

int pfb_spi_fit_components(const double* data, const double* beam, int nband, long long ncomps, const double* lnx,
                           const double* w, int ref, const double* alphai, const double* I0i, double tol, int maxiter, double* out,
                           long long* notconv, void* stream) {
    SpiBands bands;
    if (int rc = spi_fit_check("spi_fit_components", nband, ref, ncomps, tol, maxiter, lnx, w, bands)) return rc;
    PFB_REQUIRE(notconv, PFB_ERR_INVALID, "spi_fit_components: null argument");
    hipStream_t st = as_stream(stream);
    PFB_HIP_CHECK(hipMemsetAsync(notconv, 0, 8, st));
    if (ncomps == 0) return PFB_OK;
    PFB_REQUIRE(data && out, PFB_ERR_INVALID, "spi_fit_components: null argument");
    const SpiFitArgs a{data, beam, nullptr, nullptr, alphai, I0i, out, (u64*)notconv, ncomps, 0, 0,
                       0.0, tol, nband, ref, maxiter};
    hipLaunchKernelGGL((k_spi_fit<double, false>), dim3(spi_fit_grid(ncomps)), dim3(SPI_FIT_BLOCK), 0, st, a, bands);
    PFB_HIP_CHECK(hipGetLastError());
    return PFB_OK;
}

}  // extern "C"
