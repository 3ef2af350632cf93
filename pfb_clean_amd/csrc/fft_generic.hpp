// fft_generic.hpp -- runtime-length mixed-radix Stockham FFT executed by one workgroup
// in LDS (ping-pong buffers).  Any N = 2^a 3^b 5^c 7^d 11^e 13^f whose two complex
// buffers fit in the 160 KB LDS of a gfx950 CU.  This is the coverage path (odd
// good_size lengths, PSF grids that are not exactly 2x the image); power-of-two
// grids with 2x oversampling take the register-resident path in fft_pow2.hpp.
//
// Stockham autosort pass of radix R (p = product of the radices already done):
//   for i < N/R:  k = i mod p
//     u[r] = src[i + r N/R] * w_{pR}^{r k}          r < R
//     v    = DFT_R(u)
//     dst[(i-k) R + k + s p] = v[s]                 s < R
// natural order in, natural order out, no bit reversal.
//
// Below the FFT: the line-transform layer of the coverage paths -- the two views (RealView, SpecView) and the inline
// helpers that hold, once, the arithmetic of real rows as packed complex transforms (packed_pair, r2c_bin, c2r_bin,
// finish_row).  The LDS kernels of fftconv.hip and the global-memory kernels of fft_long.hpp are thin loops over them.
#pragma once
#include "common.hpp"

namespace pfb {

struct FftFactors {
    int n;          // transform length
    int npass;
    int radix[24];
};

inline bool plan_factors(int n, FftFactors* f) {
    f->n = n;
    f->npass = 0;
    int m = n;
    // radix 4 first (fewest LDS round trips for the power-of-two part), then the rest
    while (m % 4 == 0) { f->radix[f->npass++] = 4; m /= 4; }
    const int pr[] = {2, 3, 5, 7, 11, 13};
    for (int p : pr) while (m % p == 0) { f->radix[f->npass++] = p; m /= p; }
    return m == 1 && f->npass <= 24;
}

// tw[n * tws] = exp(-2 pi i n / N) for the transform length N of this call
// (tables are built for the full axis length; half-length transforms use tws = 2).
template <typename T, bool INV>
__device__ __forceinline__ cplx<T> twiddle(const cplx<T>* __restrict__ tw, int idx) {
    cplx<T> w = tw[idx];
    if (INV) w.y = -w.y;
    return w;
}

template <typename T, int R, bool INV>
__device__ void stockham_pass(const cplx<T>* __restrict__ src, cplx<T>* __restrict__ dst,
                              int N, int p, const cplx<T>* __restrict__ tw, int tws) {
    const int S = N / R;
    const int tstep = (N / (p * R)) * tws;      // index step of w_{pR}
    cplx<T> root[R];                             // R-th roots of unity
    if (R != 2 && R != 4) {
#pragma unroll
        for (int m = 0; m < R; ++m) root[m] = twiddle<T, INV>(tw, m * S * tws);
    }
    for (int i = threadIdx.x; i < S; i += blockDim.x) {
        const int k = i % p;
        cplx<T> u[R];
#pragma unroll
        for (int r = 0; r < R; ++r) u[r] = src[i + r * S];
        if (p > 1) {
#pragma unroll
            for (int r = 1; r < R; ++r) u[r] = u[r] * twiddle<T, INV>(tw, r * k * tstep);
        }
        cplx<T> v[R];
        if (R == 2) {
            v[0] = u[0] + u[1];
            v[1] = u[0] - u[1];
        } else if (R == 4) {
            cplx<T> a = u[0] + u[2], b = u[0] - u[2];
            cplx<T> c = u[1] + u[3], d = u[1] - u[3];
            // forward: w_4 = -i ; inverse: +i
            cplx<T> di = INV ? mul_i(d) : mul_mi(d);
            v[0] = a + c;
            v[1] = b + di;
            v[2] = a - c;
            v[3] = b - di;
        } else {
#pragma unroll
            for (int s = 0; s < R; ++s) {
                cplx<T> acc = u[0];
#pragma unroll
                for (int r = 1; r < R; ++r) acc = acc + u[r] * root[(r * s) % R];
                v[s] = acc;
            }
        }
        const int j = (i - k) * R + k;
#pragma unroll
        for (int s = 0; s < R; ++s) dst[j + s * p] = v[s];
    }
}

// Whole FFT by one workgroup.  Data starts in bufA; returns the buffer holding the
// result (bufA or bufB).  Ends with a barrier.  All threads of the block must call.
template <typename T, bool INV>
__device__ cplx<T>* fft_lds_generic(cplx<T>* bufA, cplx<T>* bufB, const FftFactors& f,
                                    const cplx<T>* __restrict__ tw, int tws) {
    cplx<T>* src = bufA;
    cplx<T>* dst = bufB;
    int p = 1;
    __syncthreads();
    for (int s = 0; s < f.npass; ++s) {
        const int R = f.radix[s];
        switch (R) {
            case 2:  stockham_pass<T, 2, INV>(src, dst, f.n, p, tw, tws); break;
            case 3:  stockham_pass<T, 3, INV>(src, dst, f.n, p, tw, tws); break;
            case 4:  stockham_pass<T, 4, INV>(src, dst, f.n, p, tw, tws); break;
            case 5:  stockham_pass<T, 5, INV>(src, dst, f.n, p, tw, tws); break;
            case 7:  stockham_pass<T, 7, INV>(src, dst, f.n, p, tw, tws); break;
            case 11: stockham_pass<T, 11, INV>(src, dst, f.n, p, tw, tws); break;
            default: stockham_pass<T, 13, INV>(src, dst, f.n, p, tw, tws); break;
        }
        p *= R;
        cplx<T>* t = src; src = dst; dst = t;
        __syncthreads();
    }
    return src;
}

// ------------------------------------------------------------------------------------------------
// Real rows as packed complex transforms: the arithmetic of the row stages, written once for the LDS kernels
// (fftconv.hip) and the global-memory kernels (fft_long.hpp).  Two views say where the data is.

// Real array (nband, P, columns): sample (b, r, c) at base[b * band + r * pitch + c].  A row is one period of length Q
// of which the first `valid` columns exist (the rest read as zero); su / sv: rows and samples read through ifftshift
// (row r is stored row (r + su) % P, sample c is stored sample (c + sv) % Q).  The image x is {.., nx, Q, ny, 0, 0},
// a PSF {.., P, Q, Q, P/2, Q/2}.
template <typename T>
struct RealView {
    T* base;
    size_t band;
    int pitch, P, Q, valid, su, sv;
    __host__ __device__ size_t row(int b, int r) const {
        int rr = r + su;
        if (rr >= P) rr -= P;
        return (size_t)b * band + (size_t)rr * pitch;
    }
};

// Half spectrum (nband, P, M+1): bin v of row r of band b at base[b * band + r * row + v * bin].  The plan's T
// (T[band][v][i]) is {T, T_band, 1, nx}; the caller's row-major (P, M+1) psfhat is {psfhat, P (M+1), M+1, 1}.
template <typename T>
struct SpecView {
    cplx<T>* base;
    size_t band, row, bin;
    __host__ __device__ cplx<T>* line(int b, int r) const { return base + (size_t)b * band + (size_t)r * row; }
};

// pair n of a row: z[n] = (x[2n], x[2n+1]) [* beam]; xr / br: the row of the view and of the beam (or null)
template <typename T>
__device__ __forceinline__ cplx<T> packed_pair(const RealView<const T>& a, const T* __restrict__ xr,
                                               const T* __restrict__ br, int n) {
    int j0 = 2 * n + a.sv, j1 = 2 * n + 1 + a.sv;
    if (j0 >= a.Q) j0 -= a.Q;
    if (j1 >= a.Q) j1 -= a.Q;
    T p = 0, q = 0;
    if (j0 < a.valid) p = br ? xr[j0] * br[j0] : xr[j0];
    if (j1 < a.valid) q = br ? xr[j1] * br[j1] : xr[j1];
    return cplx<T>(p, q);
}

// r2c: X[v] = 1/2 [ (Z[v] + conj Z[M-v]) - i w_Q^v (Z[v] - conj Z[M-v]) ],  v = 0..M, Z the length-M packed transform.
// The twiddle is read AFTER Z (and in c2r_bin's callers after Y): the compiler orders the operands of the commutative
// adds and multiplies by where their loads stand, and with them which product of the fp64 complex multiply it rounds
// before the fused multiply-add -- another load order gives results that differ in the last bit.
template <typename T>
__device__ __forceinline__ cplx<T> r2c_bin(const cplx<T>* Z, int M, int v, const cplx<T>* __restrict__ twQ) {
    const cplx<T> zv = Z[v == M ? 0 : v];
    const cplx<T> zm = conj(Z[v == 0 ? 0 : M - v]);
    const cplx<T> w = twQ[v];
    const cplx<T> s = zv + zm;
    const cplx<T> t = mul_mi(w * (zv - zm));
    return T(0.5) * (s + t);
}

// c2r: Z[v] = (Y[v] + conj Y[M-v]) + i conj(w_Q^v) (Y[v] - conj Y[M-v]),  v < M, from yv = Y[v], ym = Y[M-v];
// imaginary parts of the DC and Nyquist bins are ignored (ducc0/pocketfft c2r)
template <typename T>
__device__ __forceinline__ cplx<T> c2r_bin(cplx<T> yv, cplx<T> ym, int v, cplx<T> w) {
    if (v == 0) { yv.y = 0; ym.y = 0; }
    ym = conj(ym);
    return (yv + ym) + mul_i(mulc(yv - ym, w));
}

// What the c2r rows do with their samples: out = z * scale [* beam] [+ sigmainv x], and with dot_with the fp64
// sums <dot_with, out>, [<dot_with2, out>,] <out, out> of the row.  x, beam, dot_with* are laid out like out.
// {nullptr, nullptr, nullptr, nullptr, nullptr, 1, 0} is the plain unnormalised c2r.
template <typename T>
struct Epilogue {
    const T *x, *beam, *dot_with, *dot_with2;
    double* partials;           // [3][rows of the launch]
    T scale, sigmainv;
};

// samples j = j0, j0 + step, ... < ncol of one output row (at offset rowoff) from its packed c2r result z
template <typename T>
__device__ __forceinline__ void finish_row(const cplx<T>* z, T* __restrict__ out, size_t rowoff, int ncol, int j0, int step,
                                           const Epilogue<T>& e, double (&acc)[3]) {
    for (int j = j0; j < ncol; j += step) {
        const cplx<T> zz = z[j >> 1];
        T val = ((j & 1) ? zz.y : zz.x) * e.scale;
        if (e.beam) val *= e.beam[rowoff + j];
        if (e.x) val += e.sigmainv * e.x[rowoff + j];
        out[rowoff + j] = val;
        if (e.dot_with) {
            acc[0] += (double)e.dot_with[rowoff + j] * (double)val;
            if (e.dot_with2) acc[1] += (double)e.dot_with2[rowoff + j] * (double)val;
            acc[2] += (double)val * (double)val;
        }
    }
}

// the row's three sums -> partials[q * nrows + row]; red: 12 doubles of LDS.  All threads of the block must call.
__device__ __forceinline__ void store_row_partials(double (&acc)[3], double* red, double* __restrict__ partials, size_t row,
                                                   size_t nrows) {
    block_sum<3>(acc, red);
    if (threadIdx.x == 0) {
        partials[row] = acc[0]; partials[nrows + row] = acc[1]; partials[2 * nrows + row] = acc[2];
    }
}

}  // namespace pfb
