// beamfit.hip -- the clean beam: what pfb/utils/misc.py:506-584 (psf_errorsq, fitcleanbeam) do on image-sized arrays.
// The optimiser (scipy's L-BFGS-B) stays on the host (utils/beamfit.py); these kernels do the rest:
//   k_beamfit_max        one streaming pass over the (nband, npix) cube: per band and workgroup the NaN-propagating
//                        maximum and np.any; it also clears the band's visited mask.  The only pass over the cube
//   k_beamfit_max_final  the workgroups' partials of a band in a fixed order -> record
//   k_beamfit_lobe       one workgroup per band: the 8-connected set of pixels with psf / max > level grown from
//                        (nx // 2, ny // 2) by sweeps over its bounding box + 1 until a sweep adds nothing, then the
//                        extents of misc.py:561-567 and the number of pixels of the fit region
//   k_beamfit_objective  one workgroup: psf_errorsq and its three derivatives over the fit region of one band
//
// work = [record (nband, 16) doubles | partials (nband, G, 2) doubles | visited (nband, nwords) 64-bit words].
//
// No FMA contraction in this file: the membership test x^2 + y^2 < extent * rsq is exact in fp64 for the half-integer
// coordinates as it is written, and the sums round like numpy's multiply-then-add.
#pragma clang fp contract(off)
#include "common.hpp"
#include <limits>

namespace pfb {

typedef unsigned long long u64;

constexpr int BF_BLOCK = 256;
constexpr int BF_WAVES = BF_BLOCK / 64;
constexpr int BF_REC = PFB_BEAMFIT_RECORD;
constexpr int BF_MAX_GRID = 1024;                          // workgroups per band of the max pass
constexpr size_t BF_PIX_PER_BLOCK = 8192;                  // ... each of at least this many pixels
constexpr size_t BF_MAX_PIX = (size_t)1 << 40;
enum { R_MAX = 0, R_ANY, R_ABOVE, R_XMIN, R_XMAX, R_YMIN, R_YMAX, R_AX, R_AY, R_NLOBE, R_NFIT, R_RSQ };

__host__ __device__ static inline size_t bf_nwords(size_t npix) { return (npix + 63) / 64; }
static inline int bf_grid(size_t npix) {
    size_t g = (npix + BF_PIX_PER_BLOCK - 1) / BF_PIX_PER_BLOCK;
    return (int)(g < 1 ? 1 : (g > (size_t)BF_MAX_GRID ? BF_MAX_GRID : g));
}

// ndarray.max's combination: a NaN on either side wins
template <typename T>
__device__ __forceinline__ T nanmax(T a, T b) { return (b > a || b != b) ? b : a; }

template <typename T>
__device__ __forceinline__ T neg_inf() { return -std::numeric_limits<T>::infinity(); }

// grid (G, nband).  A plane that starts a elements past a 16-byte boundary is read as `head` = (V - a) mod V single
// elements, 16-byte vectors from there, and the rest of the plane (fewer than V elements) singly: the peel of
// load_own (pixmask.hpp), which here needs no shifting because a maximum does not care where an element sits.
template <typename T>
__global__ void __launch_bounds__(BF_BLOCK)
k_beamfit_max(const T* __restrict__ img, size_t npix, size_t nwords, double* __restrict__ part,
              u64* __restrict__ visited) {
    constexpr int V = V16<T>::N;
    __shared__ T wmax[BF_WAVES];
    __shared__ int wany[BF_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int band = blockIdx.y;
    const T* plane = img + (size_t)band * npix;
    const size_t a = (reinterpret_cast<uintptr_t>(plane) / sizeof(T)) % V;
    size_t head = (V - a) % V;
    if (head > npix) head = npix;
    const size_t nvec = (npix - head) / V;
    const size_t tail0 = head + nvec * V;
    const T* vecs = plane + head;
    const size_t stride = (size_t)gridDim.x * BF_BLOCK;
    T m = neg_inf<T>();
    bool any = false;
    auto take = [&](const Pack<T, V>& p) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
            m = nanmax(m, p.e[k]);
            any |= (p.e[k] != (T)0);
        }
    };
    size_t i = (size_t)blockIdx.x * BF_BLOCK + threadIdx.x;
    for (; i + 3 * stride < nvec; i += 4 * stride) {            // four loads in flight
        const Pack<T, V> p0 = ld_nt<T, V>(vecs, i), p1 = ld_nt<T, V>(vecs, i + stride),
                         p2 = ld_nt<T, V>(vecs, i + 2 * stride), p3 = ld_nt<T, V>(vecs, i + 3 * stride);
        take(p0); take(p1); take(p2); take(p3);
    }
    for (; i < nvec; i += stride) take(ld_nt<T, V>(vecs, i));
    if (blockIdx.x == 0) {
        const size_t nloose = head + (npix - tail0);            // < 2 V
        if (threadIdx.x < nloose) {
            const T v = plane[threadIdx.x < head ? threadIdx.x : tail0 + (threadIdx.x - head)];
            m = nanmax(m, v);
            any |= (v != (T)0);
        }
    }
    u64* vis = visited + (size_t)band * nwords;
    for (size_t w = (size_t)blockIdx.x * BF_BLOCK + threadIdx.x; w < nwords; w += stride) vis[w] = 0;

#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = nanmax(m, __shfl_down(m, off, 64));
    const u64 anyb = __ballot(any);
    if (lane == 0) {
        wmax[wave] = m;
        wany[wave] = anyb != 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        T r = wmax[0];
        int n = wany[0];
#pragma unroll
        for (int w = 1; w < BF_WAVES; ++w) {
            r = nanmax(r, wmax[w]);
            n |= wany[w];
        }
        double* p = part + 2 * ((size_t)band * gridDim.x + blockIdx.x);
        p[0] = (double)r;
        p[1] = (double)n;
    }
}

// grid (nband), one wave: the G partials of the band, lane l takes g = l, l + 64, ... in order, then the shuffle tree
__global__ void __launch_bounds__(64)
k_beamfit_max_final(const double* __restrict__ part, int G, double* __restrict__ rec) {
    const int band = blockIdx.x;
    const double* p = part + 2 * (size_t)band * G;
    double m = -INFINITY, any = 0.0;
    for (int g = threadIdx.x; g < G; g += 64) {
        m = nanmax(m, p[2 * g]);
        any = any != 0.0 || p[2 * g + 1] != 0.0 ? 1.0 : 0.0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        m = nanmax(m, __shfl_down(m, off, 64));
        const double other = __shfl_down(any, off, 64);         // every lane takes part: no shuffle behind a ||
        any = (any != 0.0 || other != 0.0) ? 1.0 : 0.0;
    }
    if (threadIdx.x == 0) {
        double* r = rec + (size_t)band * BF_REC;
        r[R_MAX] = m;
        r[R_ANY] = any;
        for (int k = R_ABOVE; k < BF_REC; ++k) r[k] = 0.0;
    }
}

// misc.py:542-543: x = np.arange(-n / 2, n / 2), half-integers for odd n
__device__ __forceinline__ double coord(int n, int i) { return -(double)n / 2.0 + (double)i; }

// index range [lo, hi] of an axis of n pixels that holds every |coordinate| < half (a superset; empty: lo > hi)
__device__ __forceinline__ void axis_range(int n, double half, int& lo, int& hi) {
    const double c = (double)n / 2.0;
    const double l = floor(c - half) - 1.0, h = ceil(c + half) + 1.0;
    lo = !(l > 0.0) ? 0 : (l > (double)n ? n : (int)l);
    hi = !(h < (double)(n - 1)) ? n - 1 : (h < -1.0 ? -1 : (int)h);
}

// misc.py:552-554 for one pixel: the quotient in the array's dtype, compared in that dtype (NumPy 2: the Python float
// `level` takes the array's dtype)
template <typename T>
__device__ __forceinline__ bool above(const T* __restrict__ plane, size_t q, T mx, T lv) { return plane[q] / mx > lv; }

__device__ __forceinline__ bool seen(const u64* vis, size_t q) {
    return (__hip_atomic_load(vis + (q >> 6), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> (q & 63)) & 1ull;
}

// grid (nband).  The visited mask of the band is all zero on entry (k_beamfit_max cleared it).  A sweep looks at every
// pixel of the lobe's bounding box grown by one pixel: one that is not in the lobe yet, is above the level and has one
// of its 8 neighbours in the lobe joins it.  Bits set during a sweep may or may not be seen by that sweep; a sweep
// that adds nothing has read a mask that no longer changes, so the lobe is complete.  The mask words are read and
// written with device-scope atomics: they never sit stale in a cache between sweeps.
template <typename T>
__global__ void __launch_bounds__(BF_BLOCK)
k_beamfit_lobe(const T* __restrict__ img, int nx, int ny, double level, double extent, double* __restrict__ recs,
               u64* __restrict__ visited) {
    __shared__ int box[4], grown[4], changed;                   // imin, imax, jmin, jmax
    __shared__ u64 count, nfit;
    const int band = blockIdx.x;
    const size_t npix = (size_t)nx * ny;
    const T* plane = img + (size_t)band * npix;
    u64* vis = visited + (size_t)band * bf_nwords(npix);
    double* rec = recs + (size_t)band * BF_REC;
    if (rec[R_ANY] == 0.0) return;                              // the record is already zero behind R_ANY
    const T mx = (T)rec[R_MAX], lv = (T)level;
    const int ci = nx / 2, cj = ny / 2;
    const size_t qc = (size_t)ci * ny + cj;
    if (!above(plane, qc, mx, lv)) return;                      // a NaN maximum ends here as well
    if (threadIdx.x == 0) {
        atomicOr(vis + (qc >> 6), 1ull << (qc & 63));
        box[0] = box[1] = ci;
        box[2] = box[3] = cj;
        count = 1;
    }
    __threadfence();
    __syncthreads();
    for (;;) {
        const int i0 = max(box[0] - 1, 0), i1 = min(box[1] + 1, nx - 1);
        const int j0 = max(box[2] - 1, 0), j1 = min(box[3] + 1, ny - 1);
        if (threadIdx.x == 0) {
            changed = 0;
            for (int k = 0; k < 4; ++k) grown[k] = box[k];
        }
        __syncthreads();
        const long long wj = j1 - j0 + 1, total = (long long)(i1 - i0 + 1) * wj;
        for (long long idx = threadIdx.x; idx < total; idx += BF_BLOCK) {
            const int i = i0 + (int)(idx / wj), j = j0 + (int)(idx % wj);
            const size_t q = (size_t)i * ny + j;
            if (seen(vis, q) || !above(plane, q, mx, lv)) continue;
            bool touch = false;
            for (int di = -1; di <= 1 && !touch; ++di) {
                const int ii = i + di;
                if (ii < 0 || ii >= nx) continue;
                for (int dj = -1; dj <= 1; ++dj) {
                    const int jj = j + dj;
                    if ((di == 0 && dj == 0) || jj < 0 || jj >= ny) continue;
                    if (seen(vis, (size_t)ii * ny + jj)) { touch = true; break; }
                }
            }
            if (!touch) continue;
            atomicOr(vis + (q >> 6), 1ull << (q & 63));
            atomicMin(&grown[0], i); atomicMax(&grown[1], i);
            atomicMin(&grown[2], j); atomicMax(&grown[3], j);
            atomicAdd(&count, 1ull);
            changed = 1;
        }
        __threadfence();
        __syncthreads();
        if (!changed) break;
        if (threadIdx.x == 0)
            for (int k = 0; k < 4; ++k) box[k] = grown[k];
        __syncthreads();
    }
    // misc.py:561-567
    const double xmin = coord(nx, box[0]), xmax = coord(nx, box[1]);
    const double ymin = coord(ny, box[2]), ymax = coord(ny, box[3]);
    const double ax = fmax(fabs(xmin), fabs(xmax)), ay = fmax(fabs(ymin), fabs(ymax));
    const double rsq = ax * ax + ay * ay;
    const double r2 = extent * rsq;
    int fi0, fi1, fj0, fj1;
    const double half = ceil(sqrt(r2));
    axis_range(nx, half, fi0, fi1);
    axis_range(ny, half, fj0, fj1);
    if (threadIdx.x == 0) nfit = 0;
    __syncthreads();
    u64 mine = 0;
    if (fi1 >= fi0 && fj1 >= fj0) {
        const long long wj = fj1 - fj0 + 1, total = (long long)(fi1 - fi0 + 1) * wj;
        for (long long idx = threadIdx.x; idx < total; idx += BF_BLOCK) {
            const double x = coord(nx, fi0 + (int)(idx / wj)), y = coord(ny, fj0 + (int)(idx % wj));
            mine += (x * x + y * y < r2) ? 1 : 0;
        }
    }
    atomicAdd(&nfit, mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        rec[R_ABOVE] = 1.0;
        rec[R_XMIN] = xmin; rec[R_XMAX] = xmax;
        rec[R_YMIN] = ymin; rec[R_YMAX] = ymax;
        rec[R_AX] = ax; rec[R_AY] = ay;
        rec[R_NLOBE] = (double)count;
        rec[R_NFIT] = (double)nfit;
        rec[R_RSQ] = r2;
    }
}

struct BeamPoint {
    double c, s;            // cos / sin of deg2rad(-pa)
    double amin, amaj;      // 1 / Smin^2, 1 / Smaj^2
    double k;               // 2 sqrt(2 ln 2)
    double gmin, gmaj, gpa; // what the three sums are multiplied by
    int order;              // emaj < emin: -1, emaj == emin: 0, emaj > emin: 1
};

// One workgroup.  With (u, v) = R (x, y), Q = u^2 / Smin^2 + v^2 / Smaj^2, m = exp(-k Q), r = d - m:
//   f = sum r^2,  df/dSmin = -4 k / Smin^3 sum r m u^2,  df/dSmaj = -4 k / Smaj^3 sum r m v^2,
//   df/dt = 4 k (1 / Smaj^2 - 1 / Smin^2) sum r m u v,  t = deg2rad(-pa).
// Thread t takes the pixels t, t + 256, ... of the fit region's box in row-major order, then block_sum's fixed tree.
template <typename T>
__global__ void __launch_bounds__(BF_BLOCK)
k_beamfit_objective(const T* __restrict__ plane, int nx, int ny, const double* __restrict__ rec, BeamPoint p,
                    double* __restrict__ out) {
    __shared__ double red[4 * BF_WAVES];
    const T mx = (T)rec[R_MAX];
    const double r2 = rec[R_RSQ];
    int fi0, fi1, fj0, fj1;
    const double half = ceil(sqrt(r2));
    axis_range(nx, half, fi0, fi1);
    axis_range(ny, half, fj0, fj1);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (fi1 >= fi0 && fj1 >= fj0) {
        const long long wj = fj1 - fj0 + 1, total = (long long)(fi1 - fi0 + 1) * wj;
        for (long long idx = threadIdx.x; idx < total; idx += BF_BLOCK) {
            const int i = fi0 + (int)(idx / wj), j = fj0 + (int)(idx % wj);
            const double x = coord(nx, i), y = coord(ny, j);
            if (!(x * x + y * y < r2)) continue;
            const double d = (double)(T)(plane[(size_t)i * ny + j] / mx);
            const double u = p.c * x - p.s * y, v = p.s * x + p.c * y;
            const double Q = p.amin * (u * u) + p.amaj * (v * v);
            const double m = exp(-p.k * Q);
            const double r = d - m, rm = r * m;
            acc[0] += r * r;
            acc[1] += rm * (u * u);
            acc[2] += rm * (v * v);
            acc[3] += rm * (u * v);
        }
    }
    block_sum<4>(acc, red);
    if (threadIdx.x == 0) {
        const double gmin = p.gmin * acc[1], gmaj = p.gmaj * acc[2];
        out[0] = acc[0];
        out[1] = p.order < 0 ? gmin : (p.order > 0 ? gmaj : 0.5 * (gmin + gmaj));
        out[2] = p.order < 0 ? gmaj : (p.order > 0 ? gmin : 0.5 * (gmin + gmaj));
        out[3] = p.gpa * acc[3];
    }
}

static bool bf_shape_ok(int nband, size_t npix) { return nband >= 1 && nband <= 65535 && npix >= 1 && npix <= BF_MAX_PIX; }

struct BfWork {
    double* rec;
    double* part;
    u64* visited;
};
static BfWork bf_work(void* work, int nband, size_t npix) {
    double* rec = (double*)work;
    double* part = rec + (size_t)nband * BF_REC;
    return {rec, part, (u64*)(part + 2 * (size_t)nband * bf_grid(npix))};
}

}  // namespace pfb

using namespace pfb;

extern "C" {

size_t pfb_beamfit_work_bytes(int nband, size_t npix) {
    if (!bf_shape_ok(nband, npix)) return 0;
    return 8 * (size_t)nband * (BF_REC + 2 * (size_t)bf_grid(npix) + bf_nwords(npix));
}

int pfb_beamfit_max(int dtype, const void* psf, int nband, size_t npix, void* work, void* stream) {
    PFB_REQUIRE(psf && work, PFB_ERR_INVALID, "beamfit_max: null argument");
    PFB_REQUIRE(dtype == PFB_F32 || dtype == PFB_F64, PFB_ERR_INVALID, "beamfit_max: bad dtype %d", dtype);
    PFB_REQUIRE(bf_shape_ok(nband, npix), PFB_ERR_INVALID, "beamfit_max: nband %d / npix %zu out of range", nband, npix);
    PFB_REQUIRE(((uintptr_t)work & 7u) == 0, PFB_ERR_INVALID, "beamfit_max: work must be 8-byte aligned");
    PFB_REQUIRE((uintptr_t)psf % (dtype == PFB_F32 ? 4 : 8) == 0, PFB_ERR_INVALID,
                "beamfit_max: psf is not aligned to its element size");
    hipStream_t st = as_stream(stream);
    const BfWork w = bf_work(work, nband, npix);
    const int G = bf_grid(npix);
    const dim3 grid(G, nband);
    if (dtype == PFB_F32)
        hipLaunchKernelGGL(k_beamfit_max<float>, grid, dim3(BF_BLOCK), 0, st, (const float*)psf, npix, bf_nwords(npix),
                           w.part, w.visited);
    else
        hipLaunchKernelGGL(k_beamfit_max<double>, grid, dim3(BF_BLOCK), 0, st, (const double*)psf, npix,
                           bf_nwords(npix), w.part, w.visited);
    hipLaunchKernelGGL(k_beamfit_max_final, dim3(nband), dim3(64), 0, st, w.part, G, w.rec);
    PFB_HIP_CHECK(hipGetLastError());
    return PFB_OK;
}

int pfb_beamfit_lobe(int dtype, const void* psf, int nband, int nx, int ny, double level, double extent, void* work,
                     void* stream) {
    PFB_REQUIRE(psf && work, PFB_ERR_INVALID, "beamfit_lobe: null argument");
    PFB_REQUIRE(dtype == PFB_F32 || dtype == PFB_F64, PFB_ERR_INVALID, "beamfit_lobe: bad dtype %d", dtype);
    PFB_REQUIRE(nx >= 1 && ny >= 1 && bf_shape_ok(nband, (size_t)nx * ny), PFB_ERR_INVALID,
                "beamfit_lobe: nband %d / shape (%d,%d) out of range", nband, nx, ny);
    PFB_REQUIRE(((uintptr_t)work & 7u) == 0, PFB_ERR_INVALID, "beamfit_lobe: work must be 8-byte aligned");
    hipStream_t st = as_stream(stream);
    const BfWork w = bf_work(work, nband, (size_t)nx * ny);
    if (dtype == PFB_F32)
        hipLaunchKernelGGL(k_beamfit_lobe<float>, dim3(nband), dim3(BF_BLOCK), 0, st, (const float*)psf, nx, ny, level,
                           extent, w.rec, w.visited);
    else
        hipLaunchKernelGGL(k_beamfit_lobe<double>, dim3(nband), dim3(BF_BLOCK), 0, st, (const double*)psf, nx, ny,
                           level, extent, w.rec, w.visited);
    PFB_HIP_CHECK(hipGetLastError());
    return PFB_OK;
}

int pfb_beamfit_objective(int dtype, const void* psf, int band, int nx, int ny, double emaj, double emin, double pa,
                          const void* work, double* out, void* stream) {
    PFB_REQUIRE(psf && work && out, PFB_ERR_INVALID, "beamfit_objective: null argument");
    PFB_REQUIRE(dtype == PFB_F32 || dtype == PFB_F64, PFB_ERR_INVALID, "beamfit_objective: bad dtype %d", dtype);
    PFB_REQUIRE(nx >= 1 && ny >= 1 && band >= 0 && bf_shape_ok(band + 1, (size_t)nx * ny), PFB_ERR_INVALID,
                "beamfit_objective: band %d / shape (%d,%d) out of range", band, nx, ny);
    const double smin = emaj < emin ? emaj : emin, smaj = emaj < emin ? emin : emaj;
    const double t = -pa * (M_PI / 180.0);                      // np.deg2rad(-pa)
    BeamPoint p;
    p.c = std::cos(t);
    p.s = std::sin(t);
    p.amin = 1.0 / (smin * smin);
    p.amaj = 1.0 / (smaj * smaj);
    p.k = 2.0 * std::sqrt(2.0 * std::log(2.0));
    p.gmin = -4.0 * p.k / (smin * smin * smin);
    p.gmaj = -4.0 * p.k / (smaj * smaj * smaj);
    p.gpa = -(M_PI / 180.0) * 4.0 * p.k * (p.amaj - p.amin);
    p.order = emaj < emin ? -1 : (emaj > emin ? 1 : 0);
    const size_t npix = (size_t)nx * ny;
    const double* rec = (const double*)work + (size_t)band * BF_REC;
    hipStream_t st = as_stream(stream);
    if (dtype == PFB_F32)
        hipLaunchKernelGGL(k_beamfit_objective<float>, dim3(1), dim3(BF_BLOCK), 0, st,
                           (const float*)psf + (size_t)band * npix, nx, ny, rec, p, out);
    else
        hipLaunchKernelGGL(k_beamfit_objective<double>, dim3(1), dim3(BF_BLOCK), 0, st,
                           (const double*)psf + (size_t)band * npix, nx, ny, rec, p, out);
    PFB_HIP_CHECK(hipGetLastError());
    return PFB_OK;
}

}  // extern "C"
