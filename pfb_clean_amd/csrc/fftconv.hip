// fftconv.hip -- PSF convolution plan + the coverage ("generic") paths + C-ABI.
//
// out = [beam*] crop(irfft2(rfft2(pad([beam*] x)) * psfhat)) [/wsum] + sigmainv * x
// (pfb/operators/psf.py:11-56, pfb/operators/hessian.py:129-158, 254-281)
//
// Three stages per apply, never materialising the zero-padded image:
//   1. rows_r2c : one image row -> packed real FFT of length Q -> M+1 bins into T
//   2. columns  : one frequency column of T -> FFT_P -> * psfhat -> IFFT_P -> first nx
//                 samples back into T (in place)
//   3. rows_c2r : M+1 bins of one output row -> c2r of length Q -> crop, scale, beam,
//                 Tikhonov term, fused <dot_with, out> partial sums
// The same row stages, over other views (fft_generic.hpp), and the plain column transform `cols`
// also make psfhat = r2c(ifftshift(psf)) and re-grid a psfhat (pfb_psfhat_regrid).  Every stage
// entry runs either one line per 256-thread workgroup with a runtime mixed-radix Stockham FFT in
// LDS (the kernels here) or, for lines beyond the LDS, as global-memory passes (fft_long.hpp);
// the caller says which and brings the scratch.  fftconv_pow2.hip supplies the fast versions of
// the three stages on the same layouts.
#include "conv_plan.hpp"
#include "fft_long.hpp"
#include <algorithm>
#include <vector>
#include <cstring>
#include <cstdlib>

namespace pfb {

thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// the coverage layouts (VB = 1): T[band][v][i], psf_l[band][v][u]
struct ConvDims {
    int nx, ny, P, Q, M;
    size_t T_band, psf_band;
};

__device__ __forceinline__ size_t t_index(const ConvDims& d, int band, int i, int v) {
    return (size_t)band * d.T_band + (size_t)v * d.nx + i;
}
__device__ __forceinline__ size_t psf_index(const ConvDims& d, int band, int u, int v) {
    return (size_t)band * d.psf_band + (size_t)v * d.P + u;
}

// ---------------------------------------------------------------- psfhat re-layout
template <typename T>
__global__ void k_relayout_psfhat(const cplx<T>* __restrict__ psfhat, cplx<T>* __restrict__ psf_l,
                                  ConvDims d) {
    // grid: (ceil((M+1) / 64), P, nband); thread -> v
    const int band = blockIdx.z;
    const int u = blockIdx.y;
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v > d.M) return;
    psf_l[psf_index(d, band, u, v)] = psfhat[((size_t)band * d.P + u) * (d.M + 1) + v];
}

// ------------------------------------------------------------------- rows, r2c
// grid (P, nb): row r of band b of the real view -> its M+1 bins in the spectrum view
template <typename T>
__global__ void __launch_bounds__(256)
k_rows_r2c(RealView<const T> in, const T* __restrict__ beam, SpecView<T> out, const cplx<T>* __restrict__ twQ,
           FftFactors f) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int M = in.Q / 2;
    cplx<T>* bufA = reinterpret_cast<cplx<T>*>(smem);
    cplx<T>* bufB = bufA + M;
    const int r = blockIdx.x, b = blockIdx.y;
    const size_t off = in.row(b, r);
    const T* xr = in.base + off;
    const T* br = beam ? beam + off : nullptr;
    for (int n = threadIdx.x; n < M; n += blockDim.x) bufA[n] = packed_pair(in, xr, br, n);
    cplx<T>* Z = fft_lds_generic<T, false>(bufA, bufB, f, twQ, 2);
    cplx<T>* orow = out.line(b, r);
    for (int v = threadIdx.x; v <= M; v += blockDim.x) orow[(size_t)v * out.bin] = r2c_bin(Z, M, v, twQ);
}

// ------------------------------------------------------------------------ column
template <typename T>
__global__ void __launch_bounds__(256)
k_col_generic(cplx<T>* __restrict__ Tw, const cplx<T>* __restrict__ psf_l,
              const cplx<T>* __restrict__ twP, ConvDims d, FftFactors f, int band0) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cplx<T>* bufA = reinterpret_cast<cplx<T>*>(smem);
    cplx<T>* bufB = bufA + d.P;
    const int v = blockIdx.x;
    const int band = band0 + blockIdx.y;
    for (int n = threadIdx.x; n < d.P; n += blockDim.x)
        bufA[n] = n < d.nx ? Tw[t_index(d, band, n, v)] : cplx<T>(0, 0);
    cplx<T>* X = fft_lds_generic<T, false>(bufA, bufB, f, twP, 1);
    for (int u = threadIdx.x; u < d.P; u += blockDim.x)
        X[u] = X[u] * psf_l[psf_index(d, band, u, v)];
    cplx<T>* other = (X == bufA) ? bufB : bufA;
    cplx<T>* Y = fft_lds_generic<T, true>(X, other, f, twP, 1);
    for (int n = threadIdx.x; n < d.nx; n += blockDim.x)
        Tw[t_index(d, band, n, v)] = Y[n];
}

// plain FFT of length P down every column of a spectrum view, in place: grid (bins, nb)
template <typename T, bool INV>
__global__ void __launch_bounds__(256)
k_psfhat_cols(SpecView<T> a, const cplx<T>* __restrict__ twP, FftFactors f) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int P = f.n;
    cplx<T>* bufA = reinterpret_cast<cplx<T>*>(smem);
    cplx<T>* bufB = bufA + P;
    cplx<T>* col = a.line(blockIdx.y, 0) + (size_t)blockIdx.x * a.bin;
    for (int n = threadIdx.x; n < P; n += blockDim.x) bufA[n] = col[(size_t)n * a.row];
    cplx<T>* X = fft_lds_generic<T, INV>(bufA, bufB, f, twP, 1);
    for (int n = threadIdx.x; n < P; n += blockDim.x) col[(size_t)n * a.row] = X[n];
}

// ------------------------------------------------------------------- rows, c2r
// grid (P, nb): the M+1 bins of row r of band b -> c2r of length Q -> the row's first `valid` samples through the
// epilogue.  LDS: the two line buffers, then (only with e.dot_with) 128 B for the block sums -- all in the one dynamic
// array (a static __shared__ beside it would eat into the 160 KB limit)
template <typename T>
__global__ void __launch_bounds__(256)
k_rows_c2r(SpecView<T> in, RealView<T> out, const cplx<T>* __restrict__ twQ, FftFactors f, Epilogue<T> e) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int M = out.Q / 2;
    cplx<T>* bufA = reinterpret_cast<cplx<T>*>(smem);
    cplx<T>* bufB = bufA + M;
    double* red = reinterpret_cast<double*>(bufB + M);          // 3 sums x 4 waves = 96 B
    const int r = blockIdx.x, b = blockIdx.y;
    const cplx<T>* srow = in.line(b, r);
    for (int v = threadIdx.x; v < M; v += blockDim.x)
        bufA[v] = c2r_bin(srow[(size_t)v * in.bin], srow[(size_t)(M - v) * in.bin], v, twQ[v]);
    cplx<T>* z = fft_lds_generic<T, true>(bufA, bufB, f, twQ, 2);
    double acc[3] = {0.0, 0.0, 0.0};
    finish_row(z, out.base, out.row(b, r), out.valid, (int)threadIdx.x, (int)blockDim.x, e, acc);
    if (e.dot_with) store_row_partials(acc, red, e.partials, (size_t)b * out.P + r, (size_t)gridDim.x * gridDim.y);
}

// psf2[u2][v2] = scale * psf[(du mod P)][(dv mod Q)] for the offsets |du| < nx, |dv| < ny a
// convolution of an (nx, ny) image can touch (origin at index 0, periodic in the OLD grid --
// which reproduces the wrap-around of grids with nx_psf < 2 nx exactly), zero elsewhere
template <typename T>
__global__ void __launch_bounds__(256)
k_psf_embed(const T* __restrict__ psf, T* __restrict__ psf2, int nx, int ny, int P, int Q, int P2, int Q2,
            T scale) {
    const int v2 = blockIdx.x * blockDim.x + threadIdx.x, u2 = blockIdx.y, band = blockIdx.z;
    if (v2 >= Q2) return;
    const int du = u2 < nx ? u2 : u2 - P2, dv = v2 < ny ? v2 : v2 - Q2;
    T val = 0;
    if (du > -nx && dv > -ny) {
        const int u = ((du % P) + P) % P, v = ((dv % Q) + Q) % Q;
        val = scale * psf[((size_t)band * P + u) * Q + v];
    }
    psf2[((size_t)band * P2 + u2) * Q2 + v2] = val;
}

// out[q] = sum of the n partials of quantity q (q < nq), fixed order => deterministic
__global__ void __launch_bounds__(256)
k_sum_partials(const double* __restrict__ partials, int n, int nq, double* __restrict__ out) {
    __shared__ double red[4];
    for (int q = 0; q < nq; ++q) {
        double acc[1] = {0.0};
        for (int k = threadIdx.x; k < n; k += blockDim.x) acc[0] += partials[(size_t)q * n + k];
        block_sum<1>(acc, red);
        if (threadIdx.x == 0) out[q] = acc[0];
    }
}

// per band: out[bl * 3 + q] = sum of band bl's `bs` partials of quantity q (at q * qs + bl * bst), one workgroup per
// band, fixed order => deterministic
__global__ void __launch_bounds__(256)
k_sum_partials_bands(const double* __restrict__ partials, int bs, int qs, int bst, double* __restrict__ out) {
    __shared__ double red[4];
    const int bl = blockIdx.x;
    for (int q = 0; q < 3; ++q) {
        const double* src = partials + (size_t)q * qs + (size_t)bl * bst;
        double acc[1] = {0.0};
        for (int k = threadIdx.x; k < bs; k += blockDim.x) acc[0] += src[k];
        block_sum<1>(acc, red);
        if (threadIdx.x == 0) out[(size_t)bl * 3 + q] = acc[0];
    }
}

static ConvDims dims_of(const pfb_conv_plan* p) {
    ConvDims d;
    d.nx = p->nx; d.ny = p->ny; d.P = p->P; d.Q = p->Q; d.M = p->M;
    d.T_band = p->T_elems_per_band; d.psf_band = p->psf_elems_per_band;
    return d;
}

template <typename T>
static int upload_twiddles(int n, void** dev) {
    std::vector<cplx<T>> h(n);
    const long double two_pi = 6.283185307179586476925286766559005768L;
    for (int k = 0; k < n; ++k) {
        // octant-exact: reduce the angle so that sin/cos see |a| <= pi/4 where possible
        long double a = two_pi * (long double)k / (long double)n;
        h[k].x = (T)cosl(a);
        h[k].y = (T)(-sinl(a));
    }
    PFB_HIP_CHECK(hipMalloc(dev, sizeof(cplx<T>) * (size_t)n));
    PFB_HIP_CHECK(hipMemcpy(*dev, h.data(), sizeof(cplx<T>) * (size_t)n, hipMemcpyHostToDevice));
    return PFB_OK;
}

// device memory owned by a scope: freed on every way out (hipFree waits for work that still uses it)
struct DevBuf {
    void* p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    bool alloc(size_t bytes) { return bytes == 0 || hipMalloc(&p, bytes) == hipSuccess; }
};

template <typename T>
static int set_lds_limits() {
    // the attribute is per function, not per launch: always raise it to the whole
    // 160 KB of a gfx950 CU so plans of different sizes can coexist
    const int lds_max = 160 * 1024;
    for (const void* k : {(const void*)k_rows_r2c<T>, (const void*)k_rows_c2r<T>, (const void*)k_col_generic<T>,
                          (const void*)(k_psfhat_cols<T, false>), (const void*)(k_psfhat_cols<T, true>)})
        PFB_HIP_CHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
    return PFB_OK;
}

// a line of n complex values fits the LDS ping-pong buffers of the one-workgroup-per-line kernels
template <typename T> static inline bool line_fits_lds(int n) { return 2 * sizeof(cplx<T>) * (size_t)n <= (size_t)160 * 1024; }

// ---------------------------------------------------------------------------------------------- stage entries
// One host entry per stage.  lds: one line per workgroup in LDS (no scratch); otherwise global-memory passes in the
// caller's scratch `ws` (rows_ws_elems / cols_ws_elems complex values).  Launches only: the caller checks
// hipGetLastError and synchronises where it has to.
static inline size_t rows_ws_elems(bool lds, int nb, int P, int M) { return lds ? 0 : 2 * (size_t)nb * P * M; }
static inline size_t cols_ws_elems(bool lds, int P, int nbins) { return lds ? 0 : (size_t)P * nbins; }

// r2c of every row of nb bands of a real view (f: length Q/2, twQ: exp(-2 pi i n / Q))
template <typename T>
static int rows_r2c(const RealView<const T>& in, const T* beam, const SpecView<T>& out, int nb, const FftFactors& f,
                    const cplx<T>* twQ, bool lds, cplx<T>* ws, hipStream_t st) {
    const int M = in.Q / 2;
    if (lds) {
        hipLaunchKernelGGL((k_rows_r2c<T>), dim3(in.P, nb), dim3(256), 2 * sizeof(cplx<T>) * (size_t)M, st, in, beam, out, twQ, f);
        return PFB_OK;
    }
    const size_t n = (size_t)nb * in.P * M;
    hipLaunchKernelGGL((k_long_pack<T>), long_grid(M, in.P, nb), dim3(256), 0, st, in, beam, ws);
    if (int rc = long_fft<T, false>(ws, ws + n, n, f, twQ, 2, (size_t)nb * in.P, 1, (size_t)M, st); rc != PFB_OK) return rc;
    hipLaunchKernelGGL((k_long_post<T>), long_grid(M + 1, in.P, nb), dim3(256), 0, st, (const cplx<T>*)ws, out, twQ, in.P, M);
    return PFB_OK;
}

// unnormalised c2r of every row of nb bands of a spectrum view, through the epilogue, into a real view
template <typename T>
static int rows_c2r(const SpecView<T>& in, const RealView<T>& out, const Epilogue<T>& e, int nb, const FftFactors& f,
                    const cplx<T>* twQ, bool lds, cplx<T>* ws, hipStream_t st) {
    const int M = out.Q / 2;
    if (lds) {
        hipLaunchKernelGGL((k_rows_c2r<T>), dim3(out.P, nb), dim3(256), 2 * sizeof(cplx<T>) * (size_t)M + (e.dot_with ? 128 : 0),
                           st, in, out, twQ, f, e);
        return PFB_OK;
    }
    const size_t n = (size_t)nb * out.P * M;
    hipLaunchKernelGGL((k_long_pre<T>), long_grid(M, out.P, nb), dim3(256), 0, st, in, ws, twQ, out.P, M);
    if (int rc = long_fft<T, true>(ws, ws + n, n, f, twQ, 2, (size_t)nb * out.P, 1, (size_t)M, st); rc != PFB_OK) return rc;
    hipLaunchKernelGGL((k_long_finish<T>), e.dot_with ? dim3(1, out.P, nb) : long_grid(out.valid, out.P, nb), dim3(256), 0, st,
                       (const cplx<T>*)ws, out, e);
    return PFB_OK;
}

// FFT of length f.n down the `nbins` columns of nb bands of a spectrum view, in place (a band is contiguous)
template <typename T, bool INV>
static int cols(const SpecView<T>& a, int nb, int nbins, const FftFactors& f, const cplx<T>* twP, bool lds, cplx<T>* ws,
                hipStream_t st) {
    if (lds) {
        hipLaunchKernelGGL((k_psfhat_cols<T, INV>), dim3(nbins, nb), dim3(256), 2 * sizeof(cplx<T>) * (size_t)f.n, st, a, twP, f);
        return PFB_OK;
    }
    for (int b = 0; b < nb; ++b)
        if (int rc = long_fft<T, INV>(a.line(b, 0), ws, (size_t)f.n * nbins, f, twP, 1, (size_t)nbins, a.row, a.bin, st);
            rc != PFB_OK)
            return rc;
    return PFB_OK;
}

// the column stage of the convolution, in place in T: zero-pad to P, forward, multiply by psf_l, inverse, keep nx
template <typename T>
static int conv_cols(pfb_conv_plan* p, int band0, int nb, bool lds, cplx<T>* ws, hipStream_t st) {
    if (lds) {
        hipLaunchKernelGGL((k_col_generic<T>), dim3(p->M + 1, nb), dim3(256), 2 * sizeof(cplx<T>) * (size_t)p->P, st,
                           (cplx<T>*)p->T, (const cplx<T>*)p->psf_l, (const cplx<T>*)p->twP, dims_of(p), p->fcol, band0);
        return PFB_OK;
    }
    // band by band through one contiguous zero-padded column per line: C[v][u]
    const int nbins = p->M + 1;
    const size_t ncol = (size_t)nbins * p->P;
    const SpecView<T> C{ws, ncol, 1, (size_t)p->P};
    for (int bl = 0; bl < nb; ++bl) {
        cplx<T>* Tb = (cplx<T>*)p->T + (size_t)(band0 + bl) * p->T_elems_per_band;
        const cplx<T>* psf_b = (const cplx<T>*)p->psf_l + (size_t)(band0 + bl) * p->psf_elems_per_band;
        hipLaunchKernelGGL((k_long_col_load<T>), long_grid(p->P, nbins, 1), dim3(256), 0, st, (const cplx<T>*)Tb, ws, p->nx, p->P);
        if (int rc = cols<T, false>(C, 1, nbins, p->fcol, (const cplx<T>*)p->twP, false, ws + ncol, st); rc != PFB_OK) return rc;
        hipLaunchKernelGGL((k_long_col_mul<T>), dim3(4096), dim3(256), 0, st, ws, psf_b, ncol);
        if (int rc = cols<T, true>(C, 1, nbins, p->fcol, (const cplx<T>*)p->twP, false, ws + ncol, st); rc != PFB_OK) return rc;
        hipLaunchKernelGGL((k_long_col_store<T>), long_grid(p->nx, nbins, 1), dim3(256), 0, st, (const cplx<T>*)ws, Tb, p->nx, p->P);
    }
    return PFB_OK;
}

// scratch of apply_coverage on a long_lines plan for nb bands: the larger of the row stages' and the column stage's
template <typename T>
static size_t long_apply_ws_bytes(int nb, int nx, int M, int P) {
    const size_t rows = rows_ws_elems(false, nb, nx, M), cols = 2 * (size_t)(M + 1) * P;
    return sizeof(cplx<T>) * (rows > cols ? rows : cols);
}

// the convolution off the fast path: three stage calls, all in LDS or (long_lines plan) all as global passes
template <typename T>
static int apply_coverage(pfb_conv_plan* p, const ApplyArgs& a) {
    const bool lds = !p->long_lines;
    cplx<T>* ws = (cplx<T>*)p->long_ws;
    const size_t img = (size_t)p->nx * p->ny;
    const hipStream_t st = a.st;
    const RealView<const T> xin{(const T*)a.x, img, p->ny, p->nx, p->Q, p->ny, 0, 0};
    const RealView<T> xout{(T*)a.out, img, p->ny, p->nx, p->Q, p->ny, 0, 0};
    const SpecView<T> Tv{(cplx<T>*)p->T + (size_t)a.band0 * p->T_elems_per_band, p->T_elems_per_band, 1, (size_t)p->nx};
    const Epilogue<T> e{(const T*)a.x, (const T*)a.beam, (const T*)a.dot_with, (const T*)a.dot_with2, p->partials,
                        (T)a.scale, (T)a.sigmainv};
    prof_mark(p, st, 0);
    int rc = rows_r2c<T>(xin, (const T*)a.beam, Tv, a.nb, p->frow, (const cplx<T>*)p->twQ, lds, ws, st);
    prof_mark(p, st, 1);
    if (rc == PFB_OK) rc = conv_cols<T>(p, a.band0, a.nb, lds, ws, st);
    prof_mark(p, st, 2);
    if (rc == PFB_OK) rc = rows_c2r<T>(Tv, xout, e, a.nb, p->frow, (const cplx<T>*)p->twQ, lds, ws, st);
    prof_mark(p, st, 3);
    if (rc != PFB_OK) return rc;
    PFB_HIP_CHECK(hipGetLastError());
    return PFB_OK;
}

// psfhat_out (nband, P, M+1) = r2c(ifftshift(psf)) for ANY 13-smooth grid: rows, then columns in place; each of the two
// transforms runs in LDS when its line fits, else as global passes.  twP / twQ: exp(-2 pi i n / P), exp(-2 pi i n / Q).
// Synchronous.
template <typename T>
static int psfhat_from_psf_t(const void* psf, void* psfhat_out, int nband, int P, int Q, const FftFactors& frow,
                             const FftFactors& fcol, const void* twP, const void* twQ, hipStream_t st) {
    const int M = Q / 2;
    const bool rl = line_fits_lds<T>(M), cl = line_fits_lds<T>(P);
    const size_t need = sizeof(cplx<T>) * std::max(rows_ws_elems(rl, nband, P, M), cols_ws_elems(cl, P, M + 1));
    DevBuf ws;
    PFB_REQUIRE(ws.alloc(need), PFB_ERR_ALLOC, "psfhat_from_psf: device allocation failed (%zu B)", need);
    const RealView<const T> in{(const T*)psf, (size_t)P * Q, Q, P, Q, Q, P / 2, M};
    const SpecView<T> out{(cplx<T>*)psfhat_out, (size_t)P * (M + 1), (size_t)(M + 1), 1};
    int rc = rows_r2c<T>(in, nullptr, out, nband, frow, (const cplx<T>*)twQ, rl, (cplx<T>*)ws.p, st);
    if (rc == PFB_OK) rc = cols<T, false>(out, nband, M + 1, fcol, (const cplx<T>*)twP, cl, (cplx<T>*)ws.p, st);
    if (rc != PFB_OK) return rc;
    PFB_HIP_CHECK(hipGetLastError());
    PFB_HIP_CHECK(hipStreamSynchronize(st));
    return PFB_OK;
}

// plan-less form (pfb_psfhat_from_psf): builds its own factor lists and twiddle tables
template <typename T>
static int psfhat_from_psf_grid(const void* psf, void* psfhat_out, int nband, int P, int Q, hipStream_t st) {
    FftFactors fr, fc;
    PFB_REQUIRE(plan_factors(Q / 2, &fr) && plan_factors(P, &fc), PFB_ERR_UNSUPPORTED,
                "psfhat_from_psf: (%d,%d) has a prime factor > 13", P, Q);
    DevBuf twP, twQ;
    int rc = upload_twiddles<T>(P, &twP.p);
    if (rc == PFB_OK) rc = upload_twiddles<T>(Q, &twQ.p);
    if (rc == PFB_OK) rc = set_lds_limits<T>();
    if (rc == PFB_OK) rc = psfhat_from_psf_t<T>(psf, psfhat_out, nband, P, Q, fr, fc, twP.p, twQ.p, st);
    return rc;
}

// psfhat on the (P, Q) grid -> psfhat of the SAME image-space PSF on a (P2, Q2) grid, for images
// of (nx, ny) pixels: inverse transform, embed (k_psf_embed), forward transform.  Lets a plan for
// an arbitrary size run on the power-of-two fast path (P2 = 2 nx2 >= 2 nx) with identical results.
template <typename T>
static int psfhat_regrid_t(const void* psfhat, int nband, int nx, int ny, int P, int Q, int P2, int Q2,
                           void* psfhat2, hipStream_t st) {
    const int M = Q / 2, M2 = Q2 / 2;
    FftFactors fr, fc, fr2, fc2;
    PFB_REQUIRE(plan_factors(M, &fr) && plan_factors(P, &fc) && plan_factors(M2, &fr2) && plan_factors(P2, &fc2),
                PFB_ERR_UNSUPPORTED, "psfhat_regrid: a grid length has a prime factor > 13");
    DevBuf twP, twQ, twP2, twQ2, spec, psf, psf2, ws;
    int rc = upload_twiddles<T>(P, &twP.p);
    if (rc == PFB_OK) rc = upload_twiddles<T>(Q, &twQ.p);
    if (rc == PFB_OK) rc = upload_twiddles<T>(P2, &twP2.p);
    if (rc == PFB_OK) rc = upload_twiddles<T>(Q2, &twQ2.p);
    if (rc != PFB_OK) return rc;
    // every transform picks the one-workgroup-per-line LDS kernel when its line fits, else the global-memory passes
    const bool rl = line_fits_lds<T>(M), cl = line_fits_lds<T>(P), rl2 = line_fits_lds<T>(M2), cl2 = line_fits_lds<T>(P2);
    const size_t nspec = (size_t)nband * P * (M + 1), npsf = (size_t)nband * P * Q, npsf2 = (size_t)nband * P2 * Q2;
    const size_t nws = std::max(std::max(rows_ws_elems(rl, nband, P, M), cols_ws_elems(cl, P, M + 1)),
                                std::max(rows_ws_elems(rl2, nband, P2, M2), cols_ws_elems(cl2, P2, M2 + 1)));
    PFB_REQUIRE(spec.alloc(nspec * sizeof(cplx<T>)) && psf.alloc(npsf * sizeof(T)) && psf2.alloc(npsf2 * sizeof(T)) &&
                    ws.alloc(nws * sizeof(cplx<T>)),
                PFB_ERR_ALLOC, "psfhat_regrid: device allocation failed");
    set_lds_limits<T>();
    const SpecView<T> sv{(cplx<T>*)spec.p, (size_t)P * (M + 1), (size_t)(M + 1), 1};
    const SpecView<T> sv2{(cplx<T>*)psfhat2, (size_t)P2 * (M2 + 1), (size_t)(M2 + 1), 1};
    const RealView<T> pv{(T*)psf.p, (size_t)P * Q, Q, P, Q, Q, 0, 0};
    const RealView<const T> pv2{(const T*)psf2.p, (size_t)P2 * Q2, Q2, P2, Q2, Q2, 0, 0};
    const Epilogue<T> plain{nullptr, nullptr, nullptr, nullptr, nullptr, T(1), T(0)};
    cplx<T>* w = (cplx<T>*)ws.p;
    (void)hipMemcpyAsync(spec.p, psfhat, nspec * sizeof(cplx<T>), hipMemcpyDeviceToDevice, st);
    rc = cols<T, true>(sv, nband, M + 1, fc, (const cplx<T>*)twP.p, cl, w, st);
    if (rc == PFB_OK) rc = rows_c2r<T>(sv, pv, plain, nband, fr, (const cplx<T>*)twQ.p, rl, w, st);
    if (rc == PFB_OK) {
        hipLaunchKernelGGL((k_psf_embed<T>), dim3((Q2 + 255) / 256, P2, nband), dim3(256), 0, st, (const T*)psf.p,
                           (T*)psf2.p, nx, ny, P, Q, P2, Q2, (T)(1.0 / ((double)P * (double)Q)));
        rc = rows_r2c<T>(pv2, nullptr, sv2, nband, fr2, (const cplx<T>*)twQ2.p, rl2, w, st);
    }
    if (rc == PFB_OK) rc = cols<T, false>(sv2, nband, M2 + 1, fc2, (const cplx<T>*)twP2.p, cl2, w, st);
    if (rc == PFB_OK && (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess)) {
        set_error("psfhat_regrid: kernel launch failed");
        rc = PFB_ERR_HIP;
    }
    return rc;
}

}  // namespace pfb

using namespace pfb;

extern "C" {

int pfb_abi_version(void) { return PFB_ABI_VERSION; }
const char* pfb_last_error(void) { return pfb::g_err; }

int pfb_psfconv_plan_create(int nx, int ny, int nx_psf, int ny_psf, int nband, int dtype,
                            pfb_conv_plan** plan) {
    PFB_REQUIRE(plan != nullptr, PFB_ERR_INVALID, "plan_create: null plan pointer");
    *plan = nullptr;
    PFB_REQUIRE(dtype == PFB_F32 || dtype == PFB_F64, PFB_ERR_INVALID, "plan_create: bad dtype %d", dtype);
    PFB_REQUIRE(nx > 0 && ny > 0 && nband > 0, PFB_ERR_INVALID, "plan_create: non-positive size");
    PFB_REQUIRE(nx <= nx_psf && ny <= ny_psf, PFB_ERR_INVALID,
                "plan_create: image (%d,%d) larger than psf grid (%d,%d)", nx, ny, nx_psf, ny_psf);
    PFB_REQUIRE(ny_psf % 2 == 0, PFB_ERR_UNSUPPORTED,
                "plan_create: ny_psf=%d must be even (pfb's grid worker makes it so)", ny_psf);
    PFB_REQUIRE(factorable(nx_psf) && factorable(ny_psf / 2), PFB_ERR_UNSUPPORTED,
                "plan_create: (%d,%d) has a prime factor > 13", nx_psf, ny_psf);
    pfb_conv_plan* p = (pfb_conv_plan*)calloc(1, sizeof(pfb_conv_plan));
    PFB_REQUIRE(p != nullptr, PFB_ERR_ALLOC, "plan_create: host alloc failed");
    p->nx = nx; p->ny = ny; p->P = nx_psf; p->Q = ny_psf; p->M = ny_psf / 2;
    p->nband = nband; p->dtype = dtype;
    const size_t csz = dtype == PFB_F32 ? 8 : 16;
    p->fast = pow2_supported(p) ? 1 : 0;
    if (const char* e = getenv("PFB_FORCE_GENERIC")) { if (atoi(e)) p->fast = 0; }
    int vb = 1;                 // the pow2 kernels are written for VB = 1 (pure transposed T)
    p->partials_per_band = p->fast ? nx / pow2_rows_per_wg(p) : nx;
    if (p->fast) {              // 16-byte column blocks per parity class (fftconv_pow2.hip)
        vb = pow2_nvb(p);
        p->nvb = pow2_nblocks(p);
    } else {
        p->nvb = (p->M + 1 + vb - 1) / vb;
    }
    p->VB = vb;
    p->T_elems_per_band = (size_t)p->nvb * nx * vb;
    p->psf_elems_per_band = (size_t)p->nvb * p->P * vb;
    if (!plan_factors(p->M, &p->frow) || !plan_factors(p->P, &p->fcol)) {
        free(p);
        set_error("plan_create: cannot factor (%d,%d)", nx_psf, ny_psf / 2);
        return PFB_ERR_UNSUPPORTED;
    }
    if (!p->fast) {
        // a line that does not fit the two LDS buffers of the line-per-workgroup kernels: every transform of this plan
        // runs as global-memory passes instead (fft_long.hpp) -- slow, but no grid is refused for its size
        const size_t lds_need = 128 + 2 * csz * (size_t)(p->P > p->M ? p->P : p->M);
        if (lds_need > 160 * 1024) p->long_lines = 1;
    }
    int rc = (dtype == PFB_F32) ? upload_twiddles<float>(p->P, &p->twP) : upload_twiddles<double>(p->P, &p->twP);
    if (rc == PFB_OK)
        rc = (dtype == PFB_F32) ? upload_twiddles<float>(p->Q, &p->twQ) : upload_twiddles<double>(p->Q, &p->twQ);
    const size_t tbytes = csz * p->T_elems_per_band * nband;
    const size_t pbytes = csz * p->psf_elems_per_band * nband;
    if (rc == PFB_OK && hipMalloc(&p->T, tbytes) != hipSuccess) rc = PFB_ERR_ALLOC;
    if (rc == PFB_OK && hipMalloc(&p->psf_l, pbytes) != hipSuccess) rc = PFB_ERR_ALLOC;
    if (rc == PFB_OK && hipMalloc((void**)&p->partials, sizeof(double) * 3 * (size_t)nx * nband) != hipSuccess)
        rc = PFB_ERR_ALLOC;
    if (rc == PFB_OK) {
        p->workspace_bytes = tbytes + pbytes;
        rc = (dtype == PFB_F32) ? set_lds_limits<float>() : set_lds_limits<double>();
        if (p->fast && rc == PFB_OK) rc = pow2_prepare(p);
    }
    if (rc != PFB_OK) {
        if (rc == PFB_ERR_ALLOC) set_error("plan_create: device allocation failed (%zu B)", tbytes + pbytes);
        pfb_psfconv_plan_destroy(p);
        return rc;
    }
    *plan = p;
    return PFB_OK;
}

int pfb_psfconv_plan_destroy(pfb_conv_plan* p) {
    if (!p) return PFB_OK;
    if (p->twP) (void)hipFree(p->twP);
    if (p->twQ) (void)hipFree(p->twQ);
    if (p->psf_l) (void)hipFree(p->psf_l);
    if (p->T) (void)hipFree(p->T);
    if (p->partials) (void)hipFree(p->partials);
    if (p->long_ws) (void)hipFree(p->long_ws);
    pow2_release(p);
    if (p->prof_ev) {
        for (int k = 0; k < 4 * PROF_MAX; ++k) (void)hipEventDestroy(p->prof_ev[k]);
        free(p->prof_ev);
    }
    if (p->pcg_pin) (void)hipHostFree(p->pcg_pin);
    for (int e = 0; e < 2; ++e) if (p->pcg_ev[e]) (void)hipEventDestroy(p->pcg_ev[e]);
    free(p);
    return PFB_OK;
}

int pfb_psfconv_plan_info(const pfb_conv_plan* p, int* fast_path, int* vb, size_t* workspace_bytes) {
    PFB_REQUIRE(p != nullptr, PFB_ERR_INVALID, "plan_info: null plan");
    if (fast_path) *fast_path = p->fast;
    if (vb) *vb = p->VB;
    if (workspace_bytes) *workspace_bytes = p->workspace_bytes;
    return PFB_OK;
}

int pfb_psfconv_set_profiling(pfb_conv_plan* p, int on) {
    PFB_REQUIRE(p != nullptr, PFB_ERR_INVALID, "set_profiling: null plan");
    if (on && !p->prof_ev) {
        p->prof_ev = (hipEvent_t*)calloc(4 * PROF_MAX, sizeof(hipEvent_t));
        PFB_REQUIRE(p->prof_ev != nullptr, PFB_ERR_ALLOC, "set_profiling: host alloc failed");
        for (int k = 0; k < 4 * PROF_MAX; ++k) PFB_HIP_CHECK(hipEventCreate(&p->prof_ev[k]));
    }
    p->prof_on = on > 0 ? on : 0;
    p->prof_n = 0;
    p->prof_tick = 0;
    return PFB_OK;
}

int pfb_psfconv_get_profile(pfb_conv_plan* p, double* stage_ms, int* napply) {
    PFB_REQUIRE(p && stage_ms && napply, PFB_ERR_INVALID, "get_profile: null argument");
    stage_ms[0] = stage_ms[1] = stage_ms[2] = 0.0;
    *napply = p->prof_n;
    for (int a = 0; a < p->prof_n; ++a) {
        PFB_HIP_CHECK(hipEventSynchronize(p->prof_ev[a * 4 + 3]));
        for (int k = 0; k < 3; ++k) {
            float ms = 0.f;
            PFB_HIP_CHECK(hipEventElapsedTime(&ms, p->prof_ev[a * 4 + k], p->prof_ev[a * 4 + k + 1]));
            stage_ms[k] += ms;
        }
    }
    p->prof_n = 0;
    return PFB_OK;
}

int pfb_psfconv_set_psfhat(pfb_conv_plan* p, const void* psfhat, void* stream) {
    PFB_REQUIRE(p && psfhat, PFB_ERR_INVALID, "set_psfhat: null argument");
    if (p->fast) {
        int rc = pow2_set_psfhat(p, psfhat, as_stream(stream));
        if (rc == PFB_OK) p->have_psf = 1;
        return rc;
    }
    const ConvDims d = dims_of(p);
    dim3 grid((p->M + 1 + 63) / 64, p->P, p->nband);
    if (p->dtype == PFB_F32)
        hipLaunchKernelGGL((k_relayout_psfhat<float>), grid, dim3(64), 0, as_stream(stream),
                           (const cplx<float>*)psfhat, (cplx<float>*)p->psf_l, d);
    else
        hipLaunchKernelGGL((k_relayout_psfhat<double>), grid, dim3(64), 0, as_stream(stream),
                           (const cplx<double>*)psfhat, (cplx<double>*)p->psf_l, d);
    PFB_HIP_CHECK(hipGetLastError());
    p->have_psf = 1;
    return PFB_OK;
}

int pfb_psfconv_set_psf(pfb_conv_plan* p, const void* psf, void* psfhat_out, void* stream) {
    PFB_REQUIRE(p && psf, PFB_ERR_INVALID, "set_psf: null argument");
    if (p->fast) {             // power-of-two plan: the fast path's own row / column kernels (fftconv_pow2.hip)
        int rc = pow2_set_psf(p, psf, psfhat_out, as_stream(stream));
        if (rc == PFB_OK) p->have_psf = 1;
        return rc;
    }
    const size_t csz = p->dtype == PFB_F32 ? 8 : 16;
    hipStream_t st = as_stream(stream);
    DevBuf tmp;
    void* dst = psfhat_out;
    if (!dst) {
        PFB_HIP_CHECK(hipMalloc(&tmp.p, csz * (size_t)p->nband * p->P * (p->M + 1)));
        dst = tmp.p;
    }
    int rc = p->dtype == PFB_F32
        ? psfhat_from_psf_t<float>(psf, dst, p->nband, p->P, p->Q, p->frow, p->fcol, p->twP, p->twQ, st)
        : psfhat_from_psf_t<double>(psf, dst, p->nband, p->P, p->Q, p->frow, p->fcol, p->twP, p->twQ, st);
    if (rc == PFB_OK) rc = pfb_psfconv_set_psfhat(p, dst, stream);
    if (tmp.p) (void)hipStreamSynchronize(st);
    return rc;
}

int pfb_psfhat_from_psf(int dtype, const void* psf, int nband, int nx_psf, int ny_psf, void* psfhat, void* stream) {
    PFB_REQUIRE(psf && psfhat && nband > 0 && nx_psf > 0 && ny_psf > 0, PFB_ERR_INVALID, "psfhat_from_psf: bad argument");
    PFB_REQUIRE(dtype == PFB_F32 || dtype == PFB_F64, PFB_ERR_INVALID, "psfhat_from_psf: bad dtype");
    PFB_REQUIRE(ny_psf % 2 == 0, PFB_ERR_UNSUPPORTED, "psfhat_from_psf: ny_psf=%d must be even", ny_psf);
    return dtype == PFB_F32 ? psfhat_from_psf_grid<float>(psf, psfhat, nband, nx_psf, ny_psf, as_stream(stream))
                            : psfhat_from_psf_grid<double>(psf, psfhat, nband, nx_psf, ny_psf, as_stream(stream));
}

int pfb_psfhat_regrid(int dtype, const void* psfhat, int nband, int nx, int ny, int nx_psf, int ny_psf,
                      int nx_psf2, int ny_psf2, void* psfhat2, void* stream) {
    PFB_REQUIRE(psfhat && psfhat2 && nband > 0 && nx > 0 && ny > 0, PFB_ERR_INVALID, "psfhat_regrid: bad argument");
    PFB_REQUIRE(dtype == PFB_F32 || dtype == PFB_F64, PFB_ERR_INVALID, "psfhat_regrid: bad dtype");
    PFB_REQUIRE(ny_psf % 2 == 0 && ny_psf2 % 2 == 0, PFB_ERR_UNSUPPORTED, "psfhat_regrid: odd last axis");
    PFB_REQUIRE(nx_psf2 >= 2 * nx - 1 && ny_psf2 >= 2 * ny - 1, PFB_ERR_INVALID,
                "psfhat_regrid: the new grid (%d,%d) must hold every offset of a (%d,%d) image", nx_psf2, ny_psf2, nx, ny);
    return dtype == PFB_F32
        ? psfhat_regrid_t<float>(psfhat, nband, nx, ny, nx_psf, ny_psf, nx_psf2, ny_psf2, psfhat2, as_stream(stream))
        : psfhat_regrid_t<double>(psfhat, nband, nx, ny, nx_psf, ny_psf, nx_psf2, ny_psf2, psfhat2, as_stream(stream));
}

static int apply_common(pfb_conv_plan* p, int band0, int nb, const void* x, const void* beam,
                        double wsum, double sigmainv, void* out, const void* dot_with,
                        const void* dot_with2, double* dots_out, int ndots, void* stream, bool per_band = false) {
    PFB_REQUIRE(p && x && out, PFB_ERR_INVALID, "apply: null argument");
    PFB_REQUIRE(p->have_psf, PFB_ERR_INVALID, "apply: pfb_psfconv_set_psfhat was never called");
    PFB_REQUIRE(band0 >= 0 && nb > 0 && band0 + nb <= p->nband, PFB_ERR_INVALID,
                "apply: band range [%d,%d) outside plan (nband=%d)", band0, band0 + nb, p->nband);
    PFB_REQUIRE(x != out, PFB_ERR_INVALID, "apply: out must not alias x");
    PFB_REQUIRE(!dot_with || dots_out || ndots == 0, PFB_ERR_INVALID, "apply: dot_with given without an output");
    PFB_REQUIRE(!dot_with2 || dot_with, PFB_ERR_INVALID, "apply: dot_with2 needs dot_with");
    hipStream_t st = as_stream(stream);
    double scale = 1.0 / ((double)p->P * (double)p->Q);
    if (wsum > 0) scale /= wsum;
    const ApplyArgs a{band0, nb, x, beam, scale, sigmainv, out, dot_with, dot_with2, per_band, st};
    int rc;
    // slot k of the plain / coverage kernels is band k / ppb's; the persistent row-inverse kernel writes fewer
    p->last = {p->partials_per_band * nb, p->partials_per_band, p->partials_per_band * nb, p->partials_per_band};
    if (p->fast)
        rc = pow2_apply(p, a);
    else {
        if (p->long_lines) {                                  // the global passes' scratch: grown on demand, freed with the plan
            const size_t need = p->dtype == PFB_F32 ? long_apply_ws_bytes<float>(nb, p->nx, p->M, p->P)
                                                    : long_apply_ws_bytes<double>(nb, p->nx, p->M, p->P);
            if (need > p->long_ws_bytes) {
                PFB_HIP_CHECK(hipStreamSynchronize(st));
                if (p->long_ws) (void)hipFree(p->long_ws);
                p->long_ws = nullptr; p->long_ws_bytes = 0;
                if (hipMalloc(&p->long_ws, need) != hipSuccess) {
                    set_error("apply: workspace allocation of %zu B for the long-line path failed", need);
                    return PFB_ERR_ALLOC;
                }
                p->long_ws_bytes = need;
            }
        }
        rc = p->dtype == PFB_F32 ? apply_coverage<float>(p, a) : apply_coverage<double>(p, a);
    }
    if (rc != PFB_OK) return rc;
    if (dot_with && ndots > 0 && per_band) {
        hipLaunchKernelGGL(k_sum_partials_bands, dim3(nb), dim3(256), 0, st, p->partials, p->last.band_slots,
                           p->last.q_stride, p->last.band_stride, dots_out);
        PFB_HIP_CHECK(hipGetLastError());
    } else if (dot_with && ndots > 0) {    // ndots == 0: the caller sums p->partials itself (PCG driver)
        hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, st, p->partials,
                           p->last.slots, ndots, dots_out);
        PFB_HIP_CHECK(hipGetLastError());
    }
    return PFB_OK;
}

int pfb_psfconv_apply(pfb_conv_plan* p, int band0, int nb, const void* x, const void* beam,
                      double wsum, double sigmainv, void* out, const void* dot_with,
                      double* dot_out, void* stream) {
    return apply_common(p, band0, nb, x, beam, wsum, sigmainv, out, dot_with, nullptr, dot_out, 1, stream);
}

int pfb_psfconv_apply_dots(pfb_conv_plan* p, int band0, int nb, const void* x, const void* beam,
                           double wsum, double sigmainv, void* out, const void* dot_with,
                           const void* dot_with2, double* dots_out, void* stream) {
    PFB_REQUIRE(dot_with && dots_out, PFB_ERR_INVALID, "apply_dots: dot_with and dots_out are required");
    return apply_common(p, band0, nb, x, beam, wsum, sigmainv, out, dot_with, dot_with2, dots_out, 3, stream);
}

int pfb_psfconv_apply_dots_bands(pfb_conv_plan* p, int band0, int nb, const void* x, const void* beam,
                                 double wsum, double sigmainv, void* out, const void* dot_with,
                                 const void* dot_with2, double* dots_out, void* stream) {
    PFB_REQUIRE(dot_with && dots_out, PFB_ERR_INVALID, "apply_dots_bands: dot_with and dots_out are required");
    return apply_common(p, band0, nb, x, beam, wsum, sigmainv, out, dot_with, dot_with2, dots_out, 3, stream, true);
}

}  // extern "C"

// internal (cgvec.hip): the convolution with its three fused dots left as per-workgroup partials in
// plan->partials -- the PCG driver sums them in the same launch that does its per-iteration scalar
// bookkeeping.  per_band: every partial belongs to ONE band (a system per band); otherwise the range is one system and
// all plan->last.slots slots of a quantity are its partials
int pfb::psfconv_apply_partials(pfb_conv_plan* p, int band0, int nb, const void* x, const void* beam,
                                double wsum, double sigmainv, void* out, const void* dot_with,
                                const void* dot_with2, bool per_band, int* bs, int* qs, int* bst, void* stream) {
    PFB_REQUIRE(dot_with, PFB_ERR_INVALID, "apply_partials: dot_with is required");
    const int rc = apply_common(p, band0, nb, x, beam, wsum, sigmainv, out, dot_with, dot_with2, nullptr, 0, stream,
                                per_band);
    if (rc != PFB_OK) return rc;
    *bs = per_band ? p->last.band_slots : p->last.slots;
    *qs = per_band ? p->last.q_stride : p->last.slots;
    *bst = per_band ? p->last.band_stride : 0;
    return PFB_OK;
}
