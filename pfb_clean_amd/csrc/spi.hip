// spi.hip -- spectral index and reference-flux maps: what pfb/utils/spi.py (fit_spi) does on image-sized arrays, with
// the per-component Gauss-Newton fit of m_b = I0 B_b x_b^alpha it hands to fit_spi_components.  The host keeps ln x_b,
// w_b and the reference band (utils/spi.py); these kernels do the rest:
//   k_spi_mask   one pass over image and beam, (nband, npix) each: the beam cut, amin over the bands > threshold as a
//                bit mask in the work layout of comps.hip, the set bits per workgroup and the workgroup's
//                NaN-propagating maximum of the cut image (PEEL: planes off 16 bytes)
//   k_spi_scan   exclusive scan of the workgroup counts with the total behind them, and the maximum of the partial
//                maxima (one workgroup)
//   k_spi_fit    one component per lane: Gauss-Newton on (alpha, I0), then the errors at the returned parameters, all
//                fp64; CUBE: gather by (Ix, Iy) with the cut applied on load, scatter into the four maps; else a dense
//                (ncomps, nband) list in, (4, ncomps) out
// Ix, Iy come from pfb_comps_compact (comps.hip), which reads the same work layout.
#include "comps_layout.hpp"

namespace pfb {

constexpr int SPI_SCAN_BLOCK = 256;
constexpr int SPI_FIT_BLOCK = 256;
constexpr int SPI_MAX_BANDS = 64;
constexpr unsigned SPI_FIT_MAX_GRID = 1u << 20;             // workgroups; beyond it a lane takes several components

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

// Workgroup g owns mask words [64 g, 64 g + 64), wave w of it the 16 words from 64 g + 16 w, as in k_comps_mask.  A lane
// holds V consecutive pixels.  Per pixel and band the cut value is c = beam > pb_min ? image : 0 (a NaN beam fails),
// compared in fp64; the pixel is set iff every c > threshold (a NaN c fails: np.amin propagates it).  counts[g] = set
// bits of the workgroup's words, maxpart[g] = max of c over the workgroup's pixels and all bands, NaN if any c is.
template <typename T, int V, bool PEEL>
__global__ void __launch_bounds__(CP_BLOCK)
k_spi_mask(const T* __restrict__ img, const T* __restrict__ beam, int nband, size_t npix, size_t nwords, double pb_min,
           double threshold, u64* __restrict__ mask, i64* __restrict__ counts, double* __restrict__ maxpart) {
    __shared__ int cnt[CP_WAVES];
    __shared__ double wmax[CP_WAVES];
    __shared__ int wnan[CP_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t w0 = (size_t)blockIdx.x * CP_WORDS + (size_t)wave * CP_WAVE_WORDS;
    const unsigned ai = (unsigned)((reinterpret_cast<uintptr_t>(img) / sizeof(T)) % V);
    const unsigned ab = (unsigned)((reinterpret_cast<uintptr_t>(beam) / sizeof(T)) % V);
    const unsigned step = (unsigned)(npix % V);
    int c = 0;
    double mx = -INFINITY;
    bool nan = false;
#pragma unroll 1
    for (int it = 0; it < CP_WAVE_WORDS / V; ++it) {
        const size_t wbase = w0 + (size_t)it * V;
        const size_t pix = wbase * 64 + (size_t)lane * V;
        bool ok[V];
#pragma unroll
        for (int k = 0; k < V; ++k) ok[k] = pix + k < npix;
        if (wbase * 64 < npix) {                                             // wave-uniform
            for (int p = 0; p < nband; ++p) {
                const int hi = PEEL ? (int)((V - (ai + p * step) % V) % V) : 0;
                const int hb = PEEL ? (int)((V - (ab + p * step) % V) % V) : 0;
                const Pack<T, V> vi = load_own<T, V, PEEL>(img + (size_t)p * npix, pix, npix, hi, lane);
                const Pack<T, V> vb = load_own<T, V, PEEL>(beam + (size_t)p * npix, pix, npix, hb, lane);
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const double cut = (double)vb.e[k] > pb_min ? (double)vi.e[k] : 0.0;
                    const bool in = pix + k < npix;
                    ok[k] = ok[k] && (cut > threshold);
                    nan = nan || (in && cut != cut);
                    mx = (in && cut > mx) ? cut : mx;
                }
            }
        }
        u64 b[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            b[k] = __ballot(ok[k]);
            c += __popcll(b[k]);
        }
        if (lane < V && wbase + lane < nwords) mask[wbase + lane] = mask_word<V>(b, lane);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_down(mx, off, 64);
        mx = o > mx ? o : mx;
    }
    const bool anynan = __ballot(nan) != 0;
    if (lane == 0) {
        cnt[wave] = c;
        wmax[wave] = mx;
        wnan[wave] = anynan;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0, n = 0;
        double m = -INFINITY;
#pragma unroll
        for (int w = 0; w < CP_WAVES; ++w) {
            s += cnt[w];
            n |= wnan[w];
            m = wmax[w] > m ? wmax[w] : m;
        }
        counts[blockIdx.x] = s;
        maxpart[blockIdx.x] = n ? (double)NAN : m;
    }
}

// one workgroup: offs[g] <- sum_{h < g} offs[h] in place, offs[n] <- the total; *mxout <- max of maxpart[0 .. n), NaN
// if any of them is
__global__ void __launch_bounds__(SPI_SCAN_BLOCK)
k_spi_scan(i64* __restrict__ offs, const double* __restrict__ maxpart, int n, double* __restrict__ mxout) {
    __shared__ i64 wsum[SPI_SCAN_BLOCK / 64];
    __shared__ double wmax[SPI_SCAN_BLOCK / 64];
    __shared__ int wnan[SPI_SCAN_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    i64 carry = 0;
    double mx = -INFINITY;
    bool nan = false;
    for (int base = 0; base < n; base += SPI_SCAN_BLOCK) {
        const int i = base + threadIdx.x;
        const i64 c = i < n ? offs[i] : 0;
        if (i < n) {
            const double m = maxpart[i];
            nan = nan || (m != m);
            mx = m > mx ? m : mx;
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
        for (int w = 0; w < SPI_SCAN_BLOCK / 64; ++w) {
            const i64 s = wsum[w];
            if (w < wave) before += s;
            total += s;
        }
        if (i < n) offs[i] = carry + before + inc - c;
        carry += total;
        __syncthreads();
    }
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
        offs[n] = carry;
        int nn = 0;
        double m = -INFINITY;
#pragma unroll
        for (int w = 0; w < SPI_SCAN_BLOCK / 64; ++w) {
            nn |= wnan[w];
            m = wmax[w] > m ? wmax[w] : m;
        }
        *mxout = nn ? (double)NAN : m;
    }
}

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

template <typename T, bool PEEL>
static void spi_mask_launch(const void* img, const void* beam, int nband, size_t npix, double pb_min, double threshold,
                            u64* mask, i64* counts, double* maxpart, hipStream_t st) {
    constexpr int V = V16<T>::N;
    hipLaunchKernelGGL((k_spi_mask<T, V, PEEL>), dim3((unsigned)comps_nblocks(npix)), dim3(CP_BLOCK), 0, st,
                       (const T*)img, (const T*)beam, nband, npix, comps_nwords(npix), pb_min, threshold, mask, counts,
                       maxpart);
}

template <typename T>
static void spi_mask_dispatch(const void* img, const void* beam, int nband, size_t npix, double pb_min,
                              double threshold, u64* mask, i64* counts, double* maxpart, hipStream_t st) {
    // every plane of both cubes starts on a 16-byte boundary
    if (aligned16(img) && aligned16(beam) && (npix * sizeof(T)) % 16 == 0)
        spi_mask_launch<T, false>(img, beam, nband, npix, pb_min, threshold, mask, counts, maxpart, st);
    else
        spi_mask_launch<T, true>(img, beam, nband, npix, pb_min, threshold, mask, counts, maxpart, st);
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
    PFB_REQUIRE(image && beam && work, PFB_ERR_INVALID, "spi_mask: null argument");
    PFB_REQUIRE(dtype == PFB_F32 || dtype == PFB_F64, PFB_ERR_INVALID, "spi_mask: bad dtype %d", dtype);
    PFB_REQUIRE(nband >= 1 && npix >= 1 && npix <= CP_MAX_PIX, PFB_ERR_INVALID,
                "spi_mask: nband %d / npix %zu out of range", nband, npix);
    PFB_REQUIRE(nband <= SPI_MAX_BANDS, PFB_ERR_UNSUPPORTED, "spi_mask: %d bands beyond the supported %d", nband,
                SPI_MAX_BANDS);
    PFB_REQUIRE(((uintptr_t)work & 7u) == 0, PFB_ERR_INVALID, "spi_mask: work must be 8-byte aligned");
    const unsigned el = dtype == PFB_F32 ? 4 : 8;
    PFB_REQUIRE((uintptr_t)image % el == 0 && (uintptr_t)beam % el == 0, PFB_ERR_INVALID,
                "spi_mask: image / beam is not aligned to its element size");
    hipStream_t st = as_stream(stream);
    const size_t nblocks = comps_nblocks(npix);
    u64* mask = (u64*)work;
    i64* offs = (i64*)work + comps_nwords(npix);
    double* maxpart = (double*)(offs + nblocks + 1);
    if (dtype == PFB_F32) spi_mask_dispatch<float>(image, beam, nband, npix, pb_min, threshold, mask, offs, maxpart, st);
    else                  spi_mask_dispatch<double>(image, beam, nband, npix, pb_min, threshold, mask, offs, maxpart, st);
    hipLaunchKernelGGL(k_spi_scan, dim3(1), dim3(SPI_SCAN_BLOCK), 0, st, offs, maxpart, (int)nblocks,
                       maxpart + nblocks);
    PFB_HIP_CHECK(hipGetLastError());
    return PFB_OK;
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
