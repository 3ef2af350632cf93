// fft_long.hpp -- line FFTs of ANY 13-smooth length in global memory: the passes behind the stage entries of fftconv.hip
// (rows_r2c / rows_c2r / cols) when a line does not fit the LDS.
//
// The line-per-workgroup kernels keep one line in two LDS buffers, which caps a line at 10240 complex64 / 5120
// complex128 values.  Longer lines (PSF grids with nx_psf up to 16384 and more, fp64 rows of more than 10240 pixels)
// take the kernels here instead: every Stockham pass (same recurrence as fft_generic.hpp) is its
// own launch over all lines of a batch, ping-ponging between two global buffers: N log N work, radix-sized passes, no
// length limit.  Around the passes, the rows of a real array are packed (k_long_pack), Hermitian-unpacked
// (k_long_post), pre-combined for the c2r (k_long_pre) and finished (k_long_finish) with the helpers of
// fft_generic.hpp, through the same two views as the LDS kernels.  Nothing here allocates: the caller owns the scratch.
#pragma once
#include "common.hpp"
#include "fft_generic.hpp"

namespace pfb {

// one Stockham pass of radix R over `nlines` lines of length N.
//   element e of line l lives at base + l * ls + e * es  (same strides in src and dst)
//   tw[n * tws] = exp(-2 pi i n / N)
// line_fast: consecutive threads take consecutive LINES (column transforms of a row-major array: ls = 1)
template <typename T, int R, bool INV>
__global__ void __launch_bounds__(256)
k_long_pass(const cplx<T>* __restrict__ src, cplx<T>* __restrict__ dst, int N, int p,
            const cplx<T>* __restrict__ tw, int tws, size_t nlines, size_t es, size_t ls, int line_fast) {
    const int S = N / R;
    const size_t total = nlines * (size_t)S;
    const int tstep = (N / (p * R)) * tws;
    cplx<T> root[R];
    if (R != 2 && R != 4) {
#pragma unroll
        for (int m = 0; m < R; ++m) root[m] = twiddle<T, INV>(tw, m * S * tws);
    }
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        size_t l;
        int i;
        if (line_fast) { l = idx % nlines; i = (int)(idx / nlines); }
        else           { i = (int)(idx % S); l = idx / S; }
        const int k = i % p;
        const cplx<T>* sp = src + l * ls;
        cplx<T> u[R];
#pragma unroll
        for (int r = 0; r < R; ++r) u[r] = sp[(size_t)(i + r * S) * es];
        if (p > 1) {
#pragma unroll
            for (int r = 1; r < R; ++r) u[r] = u[r] * twiddle<T, INV>(tw, r * k * tstep);
        }
        cplx<T> v[R];
        if (R == 2) {
            v[0] = u[0] + u[1];
            v[1] = u[0] - u[1];
        } else if (R == 4) {
            const cplx<T> a = u[0] + u[2], b = u[0] - u[2], c = u[1] + u[3], d = u[1] - u[3];
            const cplx<T> di = INV ? mul_i(d) : mul_mi(d);
            v[0] = a + c; v[1] = b + di; v[2] = a - c; v[3] = b - di;
        } else {
#pragma unroll
            for (int s = 0; s < R; ++s) {
                cplx<T> acc = u[0];
#pragma unroll
                for (int r = 1; r < R; ++r) acc = acc + u[r] * root[(r * s) % R];
                v[s] = acc;
            }
        }
        cplx<T>* dp = dst + l * ls;
        const int j = (i - k) * R + k;
#pragma unroll
        for (int s = 0; s < R; ++s) dp[(size_t)(j + s * p) * es] = v[s];
    }
}

// All passes of a batch; the result is left in `data` (`work`: same size / layout).
template <typename T, bool INV>
static int long_fft(cplx<T>* data, cplx<T>* work, size_t total_elems, const FftFactors& f, const cplx<T>* tw, int tws,
                    size_t nlines, size_t es, size_t ls, hipStream_t st) {
    cplx<T>* src = data;
    cplx<T>* dst = work;
    int p = 1;
    const int line_fast = ls < es ? 1 : 0;
    for (int s = 0; s < f.npass; ++s) {
        const int R = f.radix[s];
        const size_t items = nlines * (size_t)(f.n / R);
        size_t g = (items + 255) / 256;
        if (g > 65536) g = 65536;
        if (g < 1) g = 1;
#define PFB_LP(RR) hipLaunchKernelGGL((k_long_pass<T, RR, INV>), dim3((unsigned)g), dim3(256), 0, st, \
                                      (const cplx<T>*)src, dst, f.n, p, tw, tws, nlines, es, ls, line_fast)
        switch (R) {
            case 2:  PFB_LP(2); break;
            case 3:  PFB_LP(3); break;
            case 4:  PFB_LP(4); break;
            case 5:  PFB_LP(5); break;
            case 7:  PFB_LP(7); break;
            case 11: PFB_LP(11); break;
            default: PFB_LP(13); break;
        }
#undef PFB_LP
        p *= R;
        cplx<T>* t = src; src = dst; dst = t;
    }
    if (src != data)
        PFB_HIP_CHECK(hipMemcpyAsync(data, src, sizeof(cplx<T>) * total_elems, hipMemcpyDeviceToDevice, st));
    PFB_HIP_CHECK(hipGetLastError());
    return PFB_OK;
}

static inline dim3 long_grid(int n, int y, int zdim) {
    int gx = (n + 255) / 256;
    if (gx > 64) gx = 64;
    if (gx < 1) gx = 1;
    return dim3((unsigned)gx, (unsigned)y, (unsigned)zdim);
}

// ---- rows of a real array as packed complex transforms: z holds (nb, P, M) packed lines, contiguous.
// grid (chunks of the line, P, nb)
template <typename T>
__global__ void __launch_bounds__(256)
k_long_pack(RealView<const T> in, const T* __restrict__ beam, cplx<T>* __restrict__ z) {
    const int M = in.Q / 2, r = blockIdx.y, b = blockIdx.z;
    const size_t off = in.row(b, r);
    const T* xr = in.base + off;
    const T* br = beam ? beam + off : nullptr;
    cplx<T>* zr = z + ((size_t)b * in.P + r) * M;
    for (int n = blockIdx.x * blockDim.x + threadIdx.x; n < M; n += gridDim.x * blockDim.x) zr[n] = packed_pair(in, xr, br, n);
}

template <typename T>
__global__ void __launch_bounds__(256)
k_long_post(const cplx<T>* __restrict__ z, SpecView<T> out, const cplx<T>* __restrict__ twQ, int P, int M) {
    const int r = blockIdx.y, b = blockIdx.z;
    const cplx<T>* zr = z + ((size_t)b * P + r) * M;
    cplx<T>* orow = out.line(b, r);
    for (int v = blockIdx.x * blockDim.x + threadIdx.x; v <= M; v += gridDim.x * blockDim.x)
        orow[(size_t)v * out.bin] = r2c_bin(zr, M, v, twQ);
}

template <typename T>
__global__ void __launch_bounds__(256)
k_long_pre(SpecView<T> in, cplx<T>* __restrict__ z, const cplx<T>* __restrict__ twQ, int P, int M) {
    const int r = blockIdx.y, b = blockIdx.z;
    const cplx<T>* srow = in.line(b, r);
    cplx<T>* zr = z + ((size_t)b * P + r) * M;
    for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < M; v += gridDim.x * blockDim.x)
        zr[v] = c2r_bin(srow[(size_t)v * in.bin], srow[(size_t)(M - v) * in.bin], v, twQ[v]);
}

// with e.dot_with the grid is (1, P, nb): one workgroup per row, so that a row's sums are one partial
template <typename T>
__global__ void __launch_bounds__(256)
k_long_finish(const cplx<T>* __restrict__ z, RealView<T> out, Epilogue<T> e) {
    __shared__ double red[3 * 4];
    const int r = blockIdx.y, b = blockIdx.z;
    const size_t row = (size_t)b * out.P + r;
    double acc[3] = {0.0, 0.0, 0.0};
    finish_row(z + row * (out.Q / 2), out.base, out.row(b, r), out.valid, blockIdx.x * blockDim.x + threadIdx.x,
               gridDim.x * blockDim.x, e, acc);
    if (e.dot_with) store_row_partials(acc, red, e.partials, row, (size_t)gridDim.y * gridDim.z);
}

// ---- the column stage of the convolution on long lines, one band at a time (T[v][i], psf_l[v][u]: see conv_plan.hpp)
// C[v][u] = u < nx ? T[band][v][u] : 0     (one zero-padded column per line, contiguous)
template <typename T>
__global__ void __launch_bounds__(256)
k_long_col_load(const cplx<T>* __restrict__ Tb, cplx<T>* __restrict__ Cw, int nx, int P) {
    const size_t v = blockIdx.y;
    for (int u = blockIdx.x * blockDim.x + threadIdx.x; u < P; u += gridDim.x * blockDim.x)
        Cw[v * P + u] = u < nx ? Tb[v * nx + u] : cplx<T>(0, 0);
}
template <typename T>
__global__ void __launch_bounds__(256)
k_long_col_mul(cplx<T>* __restrict__ Cw, const cplx<T>* __restrict__ psf_b, size_t n) {
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x)
        Cw[k] = Cw[k] * psf_b[k];
}
template <typename T>
__global__ void __launch_bounds__(256)
k_long_col_store(const cplx<T>* __restrict__ Cw, cplx<T>* __restrict__ Tb, int nx, int P) {
    const size_t v = blockIdx.y;
    for (int u = blockIdx.x * blockDim.x + threadIdx.x; u < nx; u += gridDim.x * blockDim.x)
        Tb[v * nx + u] = Cw[v * P + u];
}

}  // namespace pfb
