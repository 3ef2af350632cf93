// wgrid.hip -- the visibility-space operators of the major cycle (pfb/operators/hessian.py:62-106: ducc0's dirty2vis and
// vis2dirty) by w-stacking on a twice oversampled grid with the kernel phi(x) = exp(2.3 W (sqrt(1 - x^2) - 1)), |x| < 1,
// of W cells.  The plane transform itself is the caller's (torch.fft, operators/gridder.py); this file is
// everything around it:
//   k_order_count / k_order_fill   counting sort of the unmasked visibilities by (first w plane, uv tile): histogram, the
//                                  caller's scan, placement.  Plane p's visibilities are then one contiguous range
//   k_prep / k_finish / k_weight   visibility <-> sorted slot: weight, centre phase, the zero of masked samples
//   k_finish_block / k_restore_corrs   the predict step: a block's slots into a strided (row, chan, corr) model column
//   k_grid                         one plane: 2 W lanes per visibility, a lane owns one real of a footprint row and adds
//                                  down the W rows with float atomics (2 W contiguous reals per slot and instruction)
//   k_order_keys64 / k_order_coords   the order of the reproducible mode: a 64-bit key per visibility on FINE tiles of
//                                  16 x 16 cells for the caller's stable sort, and the coordinates of a given order
//   k_grid_tile                    one plane without atomics: a workgroup owns a fine tile, a lane one cell, and sums the
//                                  slots of the tile's pair list in list order ("The tile-owned gridder")
//   k_degrid                       one plane: a lane per visibility gathers its W x W footprint; no atomics, each slot's
//                                  sum has a fixed order
//   k_image_forward / _adjoint / _correct   the image side: window <-> grid with the plane's w phase, the kernel
//                                  correction with 1/n and the beam fused in
// The slot, footprint and image kernels carry a product axis NP = 1 .. 4 (the Stokes products of one chunk under ONE
// order; pfb_wgrid_*_multi): what does not depend on the values is formed once and applied to every plane.
// Coordinates (u, v, w -> cells and planes) and every phase are fp64 whatever the data type: a phase of some tens of
// turns leaves 1e-6 of a turn in fp32.  Kernel values, grids and sums are in the data's type.
//
// Every index is reduced modulo the grid before it is used, so no coordinate, however wild, addresses outside it.
#include "entry.hpp"
#include <mutex>
#include <new>

namespace pfb {

constexpr int WG_BLOCK = ENTRY_BLOCK;
constexpr int WG_MIN_W = 4, WG_MAX_W = 12;
constexpr int WG_MAX_TILES = 4096;        // uv tiles of the sort key; the tile edge doubles from 16 until they fit
constexpr int WG_FINE = 16;               // the tile edge of the reproducible mode, whatever the grid: a workgroup's cells
constexpr int WG_BATCH = 64;              // slots that k_grid_tile stages per round
static_assert(WG_FINE * WG_FINE == WG_BLOCK, "a lane per cell of a fine tile");

// the target map of pfb_wgrid_grid_tile as it was last checked (wg_tile_map)
struct WgTileMap {
    const void *tile = nullptr, *ptr = nullptr, *start = nullptr, *count = nullptr, *p0 = nullptr;
    size_t ntgt = 0, npair = 0, nsorted = 0;
    bool operator==(const WgTileMap& o) const {
        return tile == o.tile && ptr == o.ptr && start == o.start && count == o.count && p0 == o.p0 && ntgt == o.ntgt &&
               npair == o.npair && nsorted == o.nsorted;
    }
};

struct WgridPlan {
    int dtype, nx, ny, Nu, Nv, W, nplanes, np0, tile, ntu, ntv;
    double px, py, cx, cy, w0, dw;
    bool wkernel() const { return nplanes > 1; }
    int nkeys() const { return np0 * ntu * ntv; }
    // what the entry points derive from the record, each written once
    size_t esize() const { return dtype == PFB_F32 ? 4 : 8; }
    size_t npix() const { return (size_t)nx * ny; }
    size_t grid_bytes() const { return 2 * esize() * (size_t)Nu * Nv; }
    double wp(int plane) const { return w0 + plane * (wkernel() ? dw : 0.0); }
    double cxs() const { return cx / (px * Nu); }          // turns of the centre phase per cell of u, of v
    double cys() const { return cy / (py * Nv); }
    int centre() const { return cx != 0.0 || cy != 0.0; }
    int nfu() const { return (Nu + WG_FINE - 1) / WG_FINE; }        // fine tiles per axis
    int nfv() const { return (Nv + WG_FINE - 1) / WG_FINE; }
    // the one thing a plan remembers: the map that passed wg_tile_map last (the geometry above never changes)
    mutable std::mutex map_lock;
    mutable WgTileMap map_ok;
};

template <typename T>
__device__ __forceinline__ T wg_phi(T x, T beta) {
    const T q = T(1) - x * x;
    return q > T(0) ? exp(beta * (sqrt(q) - T(1))) : T(0);
}

// first cell of a footprint around g, and the same reduced to [0, N)
__device__ __forceinline__ double wg_first(double g, double h) { return ceil(g - h); }
__device__ __forceinline__ int wg_wrap(double a0, int N) {
    const double m = a0 - N * floor(a0 / N);
    const int i = (int)m;
    return i < 0 ? 0 : (i >= N ? N - 1 : i);
}

struct WgGeom {
    int Nu, Nv, W, np0, tile, ntv, wk;
    double su, sv, w0, dw, h;          // su = pixsize_x Nu: u -> cells
};

// ---------------------------------------------------------------------------------------------------- the order
__device__ __forceinline__ void wg_coords(const double* __restrict__ uvw, const double* __restrict__ freq, size_t t,
                                          int nchan, const WgGeom& g, double& ug, double& vg, double& pg) {
    const size_t r = t / nchan;
    const double f = freq[t - r * nchan];
    ug = uvw[3 * r] * f / C_LIGHT * g.su;
    vg = uvw[3 * r + 1] * f / C_LIGHT * g.sv;
    pg = g.wk ? (uvw[3 * r + 2] * f / C_LIGHT - g.w0) / g.dw : 0.0;
}

__global__ void __launch_bounds__(WG_BLOCK)
k_order_count(const double* __restrict__ uvw, const double* __restrict__ freq, const u8* __restrict__ mask, size_t nvis,
              int nchan, WgGeom g, int* __restrict__ keys, int* __restrict__ counts) {
    const size_t t = (size_t)blockIdx.x * WG_BLOCK + threadIdx.x;
    if (t >= nvis) return;
    if (mask && !mask[t]) { keys[t] = -1; return; }
    double ug, vg, pg;
    wg_coords(uvw, freq, t, nchan, g, ug, vg, pg);
    const int a = wg_wrap(wg_first(ug, g.h), g.Nu), b = wg_wrap(wg_first(vg, g.h), g.Nv);
    int p0 = 0;
    if (g.wk) {
        const double p = wg_first(pg, g.h);
        p0 = p > 0.0 ? (p < g.np0 - 1 ? (int)p : g.np0 - 1) : 0;
    }
    const int ntiles = ((g.Nu + g.tile - 1) / g.tile) * g.ntv;
    const int key = p0 * ntiles + (a / g.tile) * g.ntv + b / g.tile;
    keys[t] = key;
    atomicAdd(&counts[key], 1);
}

__global__ void __launch_bounds__(WG_BLOCK)
k_order_fill(const double* __restrict__ uvw, const double* __restrict__ freq, size_t nvis, int nchan, WgGeom g,
             const int* __restrict__ keys, const long long* __restrict__ offsets, int* __restrict__ cursor,
             size_t nsorted, int* __restrict__ idx, double* __restrict__ coord) {
    const size_t t = (size_t)blockIdx.x * WG_BLOCK + threadIdx.x;
    if (t >= nvis) return;
    const int key = keys[t];
    if (key < 0) return;
    const size_t s = (size_t)offsets[key] + (size_t)atomicAdd(&cursor[key], 1);
    if (s >= nsorted) return;          // cannot happen with the counts of k_order_count; never write past the arrays
    double ug, vg, pg;
    wg_coords(uvw, freq, t, nchan, g, ug, vg, pg);
    idx[s] = (int)t;
    coord[s] = ug;
    coord[nsorted + s] = vg;
    coord[2 * nsorted + s] = pg;
}

// The order of the reproducible mode.  key = (p0 nfu + a / 16) nfv + b / 16 with a, b, p0 as k_order_count forms them, and
// a sentinel above every key where masked: the caller's STABLE sort then puts the slots of a key in ascending t
constexpr long long WG_KEY_MASKED = 0x7fffffffffffffffLL;

__global__ void __launch_bounds__(WG_BLOCK)
k_order_keys64(const double* __restrict__ uvw, const double* __restrict__ freq, const u8* __restrict__ mask, size_t nvis,
               int nchan, WgGeom g, long long* __restrict__ keys) {
    const size_t t = (size_t)blockIdx.x * WG_BLOCK + threadIdx.x;
    if (t >= nvis) return;
    if (mask && !mask[t]) { keys[t] = WG_KEY_MASKED; return; }
    double ug, vg, pg;
    wg_coords(uvw, freq, t, nchan, g, ug, vg, pg);
    const int a = wg_wrap(wg_first(ug, g.h), g.Nu), b = wg_wrap(wg_first(vg, g.h), g.Nv);
    int p0 = 0;
    if (g.wk) {
        const double p = wg_first(pg, g.h);
        p0 = p > 0.0 ? (p < g.np0 - 1 ? (int)p : g.np0 - 1) : 0;
    }
    const long long nfu = (g.Nu + WG_FINE - 1) / WG_FINE, nfv = (g.Nv + WG_FINE - 1) / WG_FINE;
    keys[t] = (p0 * nfu + a / WG_FINE) * nfv + b / WG_FINE;
}

// coord[.][s] of visibility idx[s]: what k_order_fill writes for it, bit for bit
__global__ void __launch_bounds__(WG_BLOCK)
k_order_coords(const double* __restrict__ uvw, const double* __restrict__ freq, size_t nvis, int nchan, WgGeom g,
               const int* __restrict__ idx, size_t nsorted, double* __restrict__ coord) {
    const size_t s = (size_t)blockIdx.x * WG_BLOCK + threadIdx.x;
    if (s >= nsorted) return;
    const int t = idx[s];
    if (t < 0 || (size_t)t >= nvis) return;          // an order never holds one; never address outside the arrays
    double ug, vg, pg;
    wg_coords(uvw, freq, (size_t)t, nchan, g, ug, vg, pg);
    coord[s] = ug;
    coord[nsorted + s] = vg;
    coord[2 * nsorted + s] = pg;
}

// ------------------------------------------------------------------------------------- visibility <-> sorted slot
// turns of the centre phase of slot s: u center_x + v center_y
__device__ __forceinline__ double wg_centre_turns(const double* __restrict__ coord, size_t ns, size_t s, double cxs,
                                                  double cys) {
    return coord[s] * cxs + coord[ns + s] * cys;
}
template <typename T>
__device__ __forceinline__ cplx<T> wg_cis(double turns) {
    double sn, cs;
    sincospi(2.0 * turns, &sn, &cs);
    return cplx<T>((T)cs, (T)sn);
}

// The kernels below carry a product axis: NP planes (Stokes products) of slot values, grids and images, product-major,
// under ONE order.  What does not depend on the values -- the slot's index and centre phase, the footprint's cells and
// kernel values, a pixel's w phase, correction and beam -- is formed once and applied to every plane.  NP = 1 is the
// single operator.  Plane k of the visibilities and weights starts at k nvis, of the slot values at k ns; with
// `wshared` every plane takes the weights' plane 0.
constexpr int WG_MAX_PROD = 4;

// val[k][s] = wgt vis exp(+2 pi i (u cx + v cy))
template <typename T, int NP>
__global__ void __launch_bounds__(WG_BLOCK)
k_prep(const cplx<T>* __restrict__ vis, const T* __restrict__ wgt, int wshared, const int* __restrict__ idx,
       const double* __restrict__ coord, size_t ns, size_t nvis, double cxs, double cys, int centre,
       cplx<T>* __restrict__ val) {
    const size_t s = (size_t)blockIdx.x * WG_BLOCK + threadIdx.x;
    if (s >= ns) return;
    const int t = idx[s];
    cplx<T> ph;                        // formed with the first product, under the same uniform branch as its use
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        cplx<T> v = vis[k * nvis + t];
        if (wgt) v = wgt[(wshared ? 0 : k * nvis) + t] * v;
        if (centre) {
            if (k == 0) ph = wg_cis<T>(wg_centre_turns(coord, ns, s, cxs, cys));
            v = v * ph;
        }
        val[k * ns + s] = v;
    }
}

// vis[k][idx[s]] = wgt acc[k][s] exp(-2 pi i (u cx + v cy)); vis was zeroed by the launcher
template <typename T, int NP>
__global__ void __launch_bounds__(WG_BLOCK)
k_finish(const cplx<T>* __restrict__ acc, const T* __restrict__ wgt, int wshared, const int* __restrict__ idx,
         const double* __restrict__ coord, size_t ns, size_t nvis, double cxs, double cys, int centre,
         cplx<T>* __restrict__ vis) {
    const size_t s = (size_t)blockIdx.x * WG_BLOCK + threadIdx.x;
    if (s >= ns) return;
    const int t = idx[s];
    cplx<T> ph;                        // as in k_prep
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        cplx<T> v = acc[k * ns + s];
        if (centre) {
            if (k == 0) ph = wg_cis<T>(-wg_centre_turns(coord, ns, s, cxs, cys));
            v = v * ph;
        }
        if (wgt) v = wgt[(wshared ? 0 : k * nvis) + t] * v;
        vis[k * nvis + t] = v;
    }
}

// the block form of k_finish: slot s is visibility (r, c) = (t / nchan_blk, t % nchan_blk) of a block of rows and
// channels, landed at row0 + r, chan0 + c of a (.., nchan_out, ncorr) array in correlations 0 and ncorr - 1, cast to the
// output's type O and then stored, or added in O.  No other cell is touched
template <typename T, typename O>
__global__ void __launch_bounds__(WG_BLOCK)
k_finish_block(const cplx<T>* __restrict__ acc, const int* __restrict__ idx, const double* __restrict__ coord, size_t ns,
               double cxs, double cys, int centre, int nchan_blk, cplx<O>* __restrict__ out, size_t row0,
               size_t nchan_out, size_t chan0, int ncorr, int accumulate) {
    const size_t s = (size_t)blockIdx.x * WG_BLOCK + threadIdx.x;
    if (s >= ns) return;
    const int t = idx[s];
    if (t < 0) return;                 // an order never holds one; never address below the array
    cplx<T> v = acc[s];
    if (centre) v = v * wg_cis<T>(-wg_centre_turns(coord, ns, s, cxs, cys));
    const cplx<O> o((O)v.x, (O)v.y);
    const size_t r = (size_t)t / (size_t)nchan_blk, c = (size_t)t - r * (size_t)nchan_blk;
    cplx<O>* cell = out + ((row0 + r) * nchan_out + chan0 + c) * (size_t)ncorr;
    cell[0] = accumulate ? cell[0] + o : o;
    if (ncorr > 1) cell[ncorr - 1] = accumulate ? cell[ncorr - 1] + o : o;
}

// out (nvis, ncorr): vis in correlations 0 and ncorr - 1, zero between; a lane per OUTPUT element, so a wave's stores
// are consecutive
template <typename T>
__global__ void __launch_bounds__(WG_BLOCK)
k_restore_corrs(const cplx<T>* __restrict__ vis, size_t n, int ncorr, cplx<T>* __restrict__ out) {
    const size_t e = (size_t)blockIdx.x * WG_BLOCK + threadIdx.x;
    if (e >= n) return;
    const size_t v = e / (size_t)ncorr;
    const int k = (int)(e - v * (size_t)ncorr);
    out[e] = (k == 0 || k == ncorr - 1) ? vis[v] : cplx<T>(T(0), T(0));
}

// val[s] = wgt acc[s]: the Hessian's hand-over from degridding to gridding (the two centre phases cancel)
template <typename T>
__global__ void __launch_bounds__(WG_BLOCK)
k_weight(const cplx<T>* __restrict__ acc, const T* __restrict__ wgt, const int* __restrict__ idx, size_t ns,
         cplx<T>* __restrict__ val) {
    const size_t s = (size_t)blockIdx.x * WG_BLOCK + threadIdx.x;
    if (s >= ns) return;
    cplx<T> v = acc[s];
    if (wgt) v = wgt[idx[s]] * v;
    val[s] = v;
}

// ------------------------------------------------------------------------------------------- gridding, one plane
// 2 W consecutive lanes per slot: lane (b, c) owns the real (c = 0) or imaginary part of column b of the footprint and
// walks down its W rows.  One atomic wave-instruction then lands 2 W contiguous reals per slot (but for the wrap) in
// about 64 / (2 W) rows; with a lane per ROW instead, its 64 adds went to 64 different rows, the slowest shape there is
// (5.5e2 us per plane for either data type).  Every lane re-evaluates the W row values: arithmetic is
// cheap next to the adds, and a slot's lanes may straddle two waves, so they cannot be shuffled
// With NP products a lane forms its coordinates, w weight, column value and each row's value once and issues NP adds
// per row, one into each product's grid
template <typename T, int W, int NP>
__global__ void __launch_bounds__(WG_BLOCK)
k_grid(const cplx<T>* __restrict__ val, const double* __restrict__ coord, size_t ns, size_t s0, size_t s1, int plane,
       WgGeom g, T* __restrict__ grid) {
    constexpr int L = 2 * W;
    const size_t tid = (size_t)blockIdx.x * WG_BLOCK + threadIdx.x;
    const size_t s = s0 + tid / L;
    const int j = (int)(tid % L), b = j >> 1, c = j & 1;
    if (s >= s1) return;
    const T beta = T(2.3) * W;
    const double h = 0.5 * W;
    T ww = T(1);
    if (g.wk) {
        ww = wg_phi<T>((T)((plane - coord[2 * ns + s]) / h), beta);
        if (ww == T(0)) return;
    }
    const double ug = coord[s], vg = coord[ns + s];
    const double a0 = wg_first(ug, h), b0 = wg_first(vg, h);
    const T fv = wg_phi<T>((T)((b0 + b - vg) / h), beta);
    T part[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const cplx<T> v = val[k * ns + s];
        part[k] = (c ? v.y : v.x) * ww * fv;
    }
    int col = wg_wrap(b0, g.Nv) + b;
    if (col >= g.Nv) col -= g.Nv;
    int row = wg_wrap(a0, g.Nu);
    const size_t gplane = 2 * (size_t)g.Nu * g.Nv;
    T* __restrict__ cell = grid + 2 * (size_t)col + c;
#pragma unroll
    for (int a = 0; a < W; ++a) {
        const T fu = wg_phi<T>((T)((a0 + a - ug) / h), beta);
#pragma unroll
        for (int k = 0; k < NP; ++k) atomic_add(cell + k * gplane + 2 * (size_t)row * g.Nv, fu * part[k]);
        if (++row == g.Nu) row = 0;
    }
}

// ------------------------------------------------------------------------- gridding without atomics, one plane
// A workgroup owns one fine tile of 16 x 16 cells -- target blockIdx.x of the map -- and lane (i, j) its cell
// (r0 + i, c0 + j) for every product: NP complex sums in registers, stored once with plain stores.  The map lists per
// target the pairs (start, count, p0): the slot segments whose footprints can reach the tile, sorted by (p0, source
// tile).  The pairs of first planes plane - W + 1 .. plane are contiguous there; their slots are walked in list order,
// WG_BATCH at a time (a batch runs across pair boundaries).  Per batch a lane stages a quarter of one slot's 2 W kernel
// values -- the expressions and the type of k_grid -- next to the wrapped first cell and ww val[k] in LDS; after the
// barrier every lane runs over the batch in order and adds fu[da] (val.c ww fv[db]) where its cell lies in the
// footprint: k_grid's product order, each product rounded on its own (no fma), so a cell sums the contributions k_grid
// would add -- in the slot order and nothing else.  No atomic, no shuffle.  A workgroup without a pair in range stores
// nothing: the launcher has zeroed the grid
template <typename T>
__device__ __forceinline__ T wg_add_product(T acc, T a, T b) {
#pragma clang fp contract(off)
    const T p = a * b;
    return acc + p;
}

template <typename T, int W, int NP>
__global__ void __launch_bounds__(WG_BLOCK)
k_grid_tile(const cplx<T>* __restrict__ val, const double* __restrict__ coord, size_t ns, int plane, WgGeom g,
            const int* __restrict__ tgt_tile, const long long* __restrict__ tgt_ptr,
            const long long* __restrict__ pair_start, const int* __restrict__ pair_count,
            const int* __restrict__ pair_p0, cplx<T>* __restrict__ grid) {
    __shared__ int s_a0[WG_BATCH], s_b0[WG_BATCH];
    __shared__ T s_fu[WG_BATCH][W], s_fv[WG_BATCH][W];
    __shared__ T s_vx[NP][WG_BATCH], s_vy[NP][WG_BATCH];
    const int tid = threadIdx.x;
    const int tile = tgt_tile[blockIdx.x], nfv = (g.Nv + WG_FINE - 1) / WG_FINE;
    if (tile < 0) return;
    const int row = (tile / nfv) * WG_FINE + (tid >> 4), col = (tile % nfv) * WG_FINE + (tid & 15);
    const bool live = row < g.Nu && col < g.Nv;          // a partial last tile
    // the pairs ascend by first plane: those below the plane's range and those up to its end are counted by all lanes
    // at once, a chunk of WG_BLOCK pairs per round
    const long long lo = tgt_ptr[blockIdx.x], hi = tgt_ptr[blockIdx.x + 1];
    long long pbeg = lo, pend = lo;
    for (long long base = lo; base < hi; base += WG_BLOCK) {
        const int p0 = base + tid < hi ? pair_p0[base + tid] : 0x7fffffff;
        pbeg += __syncthreads_count(p0 < plane - W + 1);
        const int upto = __syncthreads_count(p0 <= plane);
        pend += upto;
        if (upto < WG_BLOCK) break;          // the same in every lane
    }
    if (pbeg >= pend) return;
    const T beta = T(2.3) * W;
    const double h = 0.5 * W;
    const int sl = tid & (WG_BATCH - 1), part = tid / WG_BATCH;          // staging: slot of the batch, quarter of its work
    T ax[NP], ay[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) ax[k] = ay[k] = T(0);
    long long pi = pbeg, off = 0;          // the cursor, the same in every lane: pair, and slots of it already taken
    while (pi < pend) {
        // ---- stage: the slot sl places past the cursor
        long long q = pi, o = off + sl;
        for (; q < pend; ++q) {
            const long long c = pair_count[q];
            if (o < c) break;
            o -= c;
        }
        bool on = q < pend;
        size_t s = 0;
        if (on) {
            s = (size_t)(pair_start[q] + o);
            on = s < ns;          // what the entry point has checked; never read past the slots
        }
        // the slot's loads leave together; the w weight decides afterwards whether it is staged
        double ug = 0.0, vg = 0.0, pg = 0.0;
        cplx<T> v(T(0), T(0));
        if (on) {
            ug = coord[s];
            vg = coord[ns + s];
            if (g.wk) pg = coord[2 * ns + s];
            if (part < NP) v = val[part * ns + s];
        }
        T ww = T(1);
        if (on && g.wk) {
            ww = wg_phi<T>((T)((plane - pg) / h), beta);
            on = ww != T(0);
        }
        if (on) {
            const double a0 = wg_first(ug, h), b0 = wg_first(vg, h);
#pragma unroll
            for (int e = 0; e < 2 * W; ++e) {
                if ((e & 3) != part) continue;
                if (e < W) s_fu[sl][e] = wg_phi<T>((T)((a0 + e - ug) / h), beta);
                else s_fv[sl][e - W] = wg_phi<T>((T)((b0 + (e - W) - vg) / h), beta);
            }
            if (part == 0) {
                s_a0[sl] = wg_wrap(a0, g.Nu);
                s_b0[sl] = wg_wrap(b0, g.Nv);
            }
            if (part < NP) {
                s_vx[part][sl] = v.x * ww;
                s_vy[part][sl] = v.y * ww;
            }
        } else if (part == 0) {
            s_a0[sl] = -1;          // no slot here, or one that does not reach the plane
        }
        // ---- the batch's size and the next cursor: WG_BATCH places on
        long long q2 = pi, o2 = off + WG_BATCH;
        for (; q2 < pend; ++q2) {
            const long long c = pair_count[q2];
            if (o2 < c) break;
            o2 -= c;
        }
        const int nb = q2 < pend ? WG_BATCH : (int)(WG_BATCH - (o2 < WG_BATCH ? o2 : WG_BATCH));
        pi = q2;
        off = o2;
        __syncthreads();
        // ---- accumulate, in slot order
        if (live) {
            for (int b = 0; b < nb; ++b) {
                const int a0 = s_a0[b];
                if (a0 < 0) continue;
                int da = row - a0, db = col - s_b0[b];
                if (da < 0) da += g.Nu;
                if (db < 0) db += g.Nv;
                if (da < W && db < W) {
                    const T fu = s_fu[b][da], fv = s_fv[b][db];
#pragma unroll
                    for (int k = 0; k < NP; ++k) {
                        ax[k] = wg_add_product(ax[k], fu, s_vx[k][b] * fv);
                        ay[k] = wg_add_product(ay[k], fu, s_vy[k][b] * fv);
                    }
                }
            }
        }
        __syncthreads();
    }
    if (!live) return;
    const size_t gplane = (size_t)g.Nu * g.Nv, cell = (size_t)row * g.Nv + col;
#pragma unroll
    for (int k = 0; k < NP; ++k) grid[k * gplane + cell] = cplx<T>(ax[k], ay[k]);
}

// what pfb_wgrid_grid_tile requires of a map, a lane per pair and per target: bad[0] the targets (tile in range, ptr
// from 0 to npair, never descending), bad[1] a pair outside the slots or the first planes, bad[2] first planes that
// descend inside a target
__global__ void __launch_bounds__(WG_BLOCK)
k_tile_map_check(const int* __restrict__ tgt_tile, const long long* __restrict__ tgt_ptr,
                 const long long* __restrict__ pair_start, const int* __restrict__ pair_count,
                 const int* __restrict__ pair_p0, size_t ntgt, size_t npair, size_t nsorted, int ntiles, int np0,
                 int* __restrict__ bad) {
    const size_t i = (size_t)blockIdx.x * WG_BLOCK + threadIdx.x;
    if (i < ntgt) {
        const long long lo = tgt_ptr[i], hi = tgt_ptr[i + 1];
        if (tgt_tile[i] < 0 || tgt_tile[i] >= ntiles || lo < 0 || hi < lo || hi > (long long)npair ||
            (i == 0 && lo != 0) || (i == ntgt - 1 && hi != (long long)npair))
            bad[0] = 1;
    }
    if (i < npair) {
        const long long s = pair_start[i], c = pair_count[i];
        if (s < 0 || c < 1 || (size_t)s > nsorted || (size_t)c > nsorted - (size_t)s || pair_p0[i] < 0 || pair_p0[i] >= np0)
            bad[1] = 1;
        if (i > 0 && pair_p0[i - 1] > pair_p0[i]) {
            // a descent is right only where pair i opens a target: the last target whose ptr is <= i
            size_t lo = 0, hi = ntgt;
            while (lo < hi) {
                const size_t mid = lo + (hi - lo) / 2;
                if (tgt_ptr[mid] <= (long long)i) lo = mid + 1; else hi = mid;
            }
            if (lo == 0 || tgt_ptr[lo - 1] != (long long)i) bad[2] = 1;
        }
    }
}

// ----------------------------------------------------------------------------------------- degridding, one plane
// With NP products the W column values and each row's value are formed once; NP running sums
template <typename T, int W, int NP>
__global__ void __launch_bounds__(WG_BLOCK)
k_degrid(const cplx<T>* __restrict__ grid, const double* __restrict__ coord, size_t ns, size_t s0, size_t s1, int plane,
         WgGeom g, cplx<T>* __restrict__ acc) {
    const size_t s = s0 + (size_t)blockIdx.x * WG_BLOCK + threadIdx.x;
    if (s >= s1) return;
    const T beta = T(2.3) * W;
    const double h = 0.5 * W;
    T ww = T(1);
    if (g.wk) {
        ww = wg_phi<T>((T)((plane - coord[2 * ns + s]) / h), beta);
        if (ww == T(0)) return;
    }
    const double ug = coord[s], vg = coord[ns + s];
    const double a0 = wg_first(ug, h), b0 = wg_first(vg, h);
    T fv[W];
#pragma unroll
    for (int b = 0; b < W; ++b) fv[b] = wg_phi<T>((T)((b0 + b - vg) / h), beta);
    int row = wg_wrap(a0, g.Nu);
    const int col0 = wg_wrap(b0, g.Nv);
    const size_t gplane = (size_t)g.Nu * g.Nv;
    T sx[NP], sy[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) sx[k] = sy[k] = T(0);
#pragma unroll 1          // one row of loads in flight: unrolled, the fp64 kernels of W = 11, 12 spill
    for (int a = 0; a < W; ++a) {
        const T fu = wg_phi<T>((T)((a0 + a - ug) / h), beta);
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const cplx<T>* __restrict__ line = grid + k * gplane + (size_t)row * g.Nv;
            int col = col0;
            T rx = T(0), ry = T(0);
#pragma unroll
            for (int b = 0; b < W; ++b) {
                const cplx<T> c = line[col];
                rx += fv[b] * c.x;
                ry += fv[b] * c.y;
                if (++col == g.Nv) col = 0;
            }
            sx[k] += fu * rx;
            sy[k] += fu * ry;
        }
        if (++row == g.Nu) row = 0;
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        cplx<T> r = acc[k * ns + s];
        r.x += ww * sx[k];
        r.y += ww * sy[k];
        acc[k * ns + s] = r;
    }
}

// ------------------------------------------------------------------------------------------------ the image side
// pixel (i, j) of the image <-> cell ((i - nx/2) mod Nu, (j - ny/2) mod Nv) of the grid
__device__ __forceinline__ size_t wg_cell(int i, int j, int nx, int ny, int Nu, int Nv) {
    const int gi = i < nx / 2 ? i - nx / 2 + Nu : i - nx / 2;
    const int gj = j < ny / 2 ? j - ny / 2 + Nv : j - ny / 2;
    return (size_t)gi * Nv + gj;
}

// grid (zeroed by the launcher) <- dirty corr [beam] exp(+2 pi i w_p nm1)
// NP images and grids, product-major; corr, beam and the w phase of a pixel are the same for every product
template <typename T, int NP>
__global__ void __launch_bounds__(WG_BLOCK)
k_image_forward(const T* __restrict__ dirty, const T* __restrict__ beam, const double* __restrict__ corr,
                const double* __restrict__ nm1, double wp, int nx, int ny, int Nu, int Nv, cplx<T>* __restrict__ grid) {
    const size_t npix = (size_t)nx * ny, q = (size_t)blockIdx.x * WG_BLOCK + threadIdx.x;
    if (q >= npix) return;
    const int i = (int)(q / ny), j = (int)(q - (size_t)i * ny);
    const double cq = corr[q], bq = beam ? (double)beam[q] : 1.0;
    double sn = 0.0, cs = 1.0;
    if (nm1) sincospi(2.0 * wp * nm1[q], &sn, &cs);
    const size_t cell = wg_cell(i, j, nx, ny, Nu, Nv), gplane = (size_t)Nu * Nv;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        double d = (double)dirty[k * npix + q] * cq;
        if (beam) d *= bq;
        grid[k * gplane + cell] = nm1 ? cplx<T>((T)(d * cs), (T)(d * sn)) : cplx<T>((T)d, T(0));
    }
}

// img += window(grid) exp(-2 pi i w_p nm1)
template <typename T, int NP>
__global__ void __launch_bounds__(WG_BLOCK)
k_image_adjoint(const cplx<T>* __restrict__ grid, const double* __restrict__ nm1, double wp, int nx, int ny, int Nu,
                int Nv, cplx<T>* __restrict__ img) {
    const size_t npix = (size_t)nx * ny, q = (size_t)blockIdx.x * WG_BLOCK + threadIdx.x;
    if (q >= npix) return;
    const int i = (int)(q / ny), j = (int)(q - (size_t)i * ny);
    const size_t cell = wg_cell(i, j, nx, ny, Nu, Nv), gplane = (size_t)Nu * Nv;
    T cx, sx;                          // the pixel's w phase: formed with the first product, under the branch of its use
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const cplx<T> c = grid[k * gplane + cell];
        cplx<T> r = img[k * npix + q];
        if (nm1) {
            if (k == 0) {
                double sn, cs;
                sincospi(-2.0 * wp * nm1[q], &sn, &cs);
                cx = (T)cs;
                sx = (T)sn;
            }
            r.x += c.x * cx - c.y * sx;
            r.y += c.x * sx + c.y * cx;
        } else {
            r.x += c.x;
            r.y += c.y;
        }
        img[k * npix + q] = r;
    }
}

// dirty = Re(img) corr [beam]
template <typename T, int NP>
__global__ void __launch_bounds__(WG_BLOCK)
k_image_correct(const cplx<T>* __restrict__ img, const double* __restrict__ corr, const T* __restrict__ beam, size_t npix,
                T* __restrict__ dirty) {
    const size_t q = (size_t)blockIdx.x * WG_BLOCK + threadIdx.x;
    if (q >= npix) return;
    const double cq = corr[q], bq = beam ? (double)beam[q] : 1.0;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        double d = (double)img[k * npix + q].x * cq;
        if (beam) d *= bq;
        dirty[k * npix + q] = (T)d;
    }
}

// ------------------------------------------------------------------------------------------------------ launchers
// The entry layer is entry.hpp; what follows is the w-gridder's own: the geometry record of the kernels, the plan in
// front of check(), and the size checks that speak of planes and slots.
constexpr size_t WG_MAX_THREADS = (size_t)0x7fffffff * WG_BLOCK;        // one launch's grid limit

static WgGeom wg_geom(const WgridPlan& p) {
    WgGeom g;
    g.Nu = p.Nu; g.Nv = p.Nv; g.W = p.W; g.np0 = p.np0; g.tile = p.tile; g.ntv = p.ntv; g.wk = p.wkernel();
    g.su = p.px * p.Nu; g.sv = p.py * p.Nv; g.w0 = p.w0; g.dw = p.dw; g.h = 0.5 * p.W;
    return g;
}

static const WgridPlan& wg_plan(const void* plan) { return *static_cast<const WgridPlan*>(plan); }
// the plan and the pointers of entry point `name` (REAL, CPLX: of the plan's type)
static int wg_check(const void* plan, const char* name, std::initializer_list<Array> arrays) {
    PFB_REQUIRE(plan, PFB_ERR_INVALID, "%s: null plan", name);
    return check(wg_plan(plan).dtype, name, arrays);
}

// a plane; slots [s0, s1) of a plane, few enough for one launch of k_grid (2 W lanes a slot)
static int wg_plane(const WgridPlan& p, const char* name, int plane) {
    PFB_REQUIRE(plane >= 0 && plane < p.nplanes, PFB_ERR_INVALID, "%s: plane %d of %d", name, plane, p.nplanes);
    return PFB_OK;
}
static int wg_range(const WgridPlan& p, const char* name, int plane, size_t s0, size_t s1, size_t nsorted) {
    if (int rc = wg_plane(p, name, plane); rc != PFB_OK) return rc;
    PFB_REQUIRE(s0 <= s1 && s1 <= nsorted, PFB_ERR_INVALID, "%s: range [%zu, %zu) of %zu slots", name, s0, s1, nsorted);
    PFB_REQUIRE((s1 - s0) * 2 * (size_t)p.W <= WG_MAX_THREADS, PFB_ERR_UNSUPPORTED, "%s: %zu slots in one launch", name,
                s1 - s0);
    return PFB_OK;
}
static int wg_nprod(const char* name, int nprod) {
    PFB_REQUIRE(nprod >= 1 && nprod <= WG_MAX_PROD, PFB_ERR_INVALID, "%s: %d products outside 1 .. %d", name, nprod,
                WG_MAX_PROD);
    return PFB_OK;
}

// The entry points with a product axis, under both of their names: pfb_wgrid_X is X with one product,
// pfb_wgrid_X_multi with nprod (checked there).  One body each, so the two cannot drift apart.
static int wg_prep(const char* name, void* plan, int nprod, const void* vis, const void* wgt, int wshared, const int* idx,
                   const double* coord, size_t nsorted, size_t nvis, void* val, void* stream) {
    if (int rc = wg_check(plan, name, {{vis, CPLX}, {wgt, REAL, true}, {idx, I32}, {coord, F64}, {val, CPLX}});
        rc != PFB_OK) return rc;
    if (int rc = check_count(name, nsorted, PFB_ERR_INVALID); rc != PFB_OK) return rc;
    const WgridPlan& p = wg_plan(plan);
    return by_type(p.dtype, [&](auto t) {
        return by_int<1, WG_MAX_PROD>(nprod, [&](auto np) {
            return launch(k_prep<decltype(t), np()>, nsorted, stream, vis, wgt, wshared, idx, coord, nsorted, nvis,
                          p.cxs(), p.cys(), p.centre(), val);
        });
    });
}

static int wg_finish(const char* name, void* plan, int nprod, const void* acc, const void* wgt, int wshared,
                     const int* idx, const double* coord, size_t nsorted, void* vis, size_t nvis, void* stream) {
    if (int rc = wg_check(plan, name, {{acc, CPLX}, {wgt, REAL, true}, {idx, I32}, {coord, F64}, {vis, CPLX}});
        rc != PFB_OK) return rc;
    if (int rc = check_count(name, nsorted, PFB_ERR_INVALID); rc != PFB_OK) return rc;
    PFB_REQUIRE(nsorted <= nvis && nvis <= (size_t)0x7fffffff, PFB_ERR_INVALID, "%s: %zu slots for %zu visibilities",
                name, nsorted, nvis);
    const WgridPlan& p = wg_plan(plan);
    PFB_HIP_CHECK(hipMemsetAsync(vis, 0, 2 * p.esize() * nvis * (size_t)nprod, as_stream(stream)));
    return by_type(p.dtype, [&](auto t) {
        return by_int<1, WG_MAX_PROD>(nprod, [&](auto np) {
            return launch(k_finish<decltype(t), np()>, nsorted, stream, acc, wgt, wshared, idx, coord, nsorted, nvis,
                          p.cxs(), p.cys(), p.centre(), vis);
        });
    });
}

static int wg_grid(const char* name, void* plan, int nprod, int plane, const void* val, const double* coord,
                   size_t nsorted, size_t s0, size_t s1, void* grid, void* stream) {
    if (int rc = wg_check(plan, name, {{val, CPLX}, {coord, F64}, {grid, CPLX}}); rc != PFB_OK) return rc;
    const WgridPlan& p = wg_plan(plan);
    if (int rc = wg_range(p, name, plane, s0, s1, nsorted); rc != PFB_OK) return rc;
    PFB_HIP_CHECK(hipMemsetAsync(grid, 0, p.grid_bytes() * (size_t)nprod, as_stream(stream)));
    if (s1 == s0) return PFB_OK;
    return by_type(p.dtype, [&](auto t) {
        return by_int<WG_MIN_W, WG_MAX_W>(p.W, [&](auto w) {
            return by_int<1, WG_MAX_PROD>(nprod, [&](auto np) {
                return launch(k_grid<decltype(t), w(), np()>, (s1 - s0) * 2 * w(), stream, val, coord, nsorted, s0, s1,
                              plane, wg_geom(p), grid);
            });
        });
    });
}

// The map of a reproducible plan, checked where it is first presented to the plan: one small launch and ONE host read
// (the only entry point that waits for the device).  A plan remembers the map that passed -- its arrays and counts -- and
// takes it as read from then on: the arrays of a map do not change while a plan uses them, like idx and coord
static int wg_tile_map(const WgridPlan& p, const char* name, const WgTileMap& m, void* stream) {
    std::lock_guard<std::mutex> guard(p.map_lock);
    if (p.map_ok == m) return PFB_OK;
    int* bad = nullptr;
    PFB_HIP_CHECK(hipMalloc(&bad, 3 * sizeof(int)));
    int host[3] = {0, 0, 0};
    hipError_t e = hipMemsetAsync(bad, 0, sizeof(host), as_stream(stream));
    if (e == hipSuccess) {
        const size_t n = m.ntgt > m.npair ? m.ntgt : m.npair;
        hipLaunchKernelGGL(k_tile_map_check, dim3(blocks(n)), dim3(WG_BLOCK), 0, as_stream(stream), (const int*)m.tile,
                           (const long long*)m.ptr, (const long long*)m.start, (const int*)m.count, (const int*)m.p0,
                           m.ntgt, m.npair, m.nsorted, p.nfu() * p.nfv(), p.np0, bad);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(host, bad, sizeof(host), hipMemcpyDeviceToHost, as_stream(stream));
    if (e == hipSuccess) e = hipStreamSynchronize(as_stream(stream));
    (void)hipFree(bad);
    PFB_HIP_CHECK(e);
    PFB_REQUIRE(!host[0], PFB_ERR_INVALID, "%s: a target outside the %d fine tiles, or pointers that do not run from 0 "
                "to %zu pairs", name, p.nfu() * p.nfv(), m.npair);
    PFB_REQUIRE(!host[1], PFB_ERR_INVALID, "%s: a pair outside the %zu slots or the %d first planes", name, m.nsorted,
                p.np0);
    PFB_REQUIRE(!host[2], PFB_ERR_INVALID, "%s: the pairs of a target do not ascend by first plane", name);
    p.map_ok = m;
    return PFB_OK;
}

static int wg_grid_tile(const char* name, void* plan, int nprod, int plane, const void* val, const double* coord,
                        size_t nsorted, const int* tgt_tile, const long long* tgt_ptr, const long long* pair_start,
                        const int* pair_count, const int* pair_p0, size_t ntgt, size_t npair, void* grid, void* stream) {
    if (int rc = wg_check(plan, name, {{val, CPLX}, {coord, F64}, {tgt_tile, I32}, {tgt_ptr, I64}, {pair_start, I64},
                                       {pair_count, I32}, {pair_p0, I32}, {grid, CPLX}});
        rc != PFB_OK) return rc;
    const WgridPlan& p = wg_plan(plan);
    if (int rc = wg_plane(p, name, plane); rc != PFB_OK) return rc;
    if (int rc = check_count(name, nsorted, PFB_ERR_INVALID); rc != PFB_OK) return rc;
    PFB_REQUIRE(ntgt >= 1 && ntgt <= (size_t)p.nfu() * p.nfv() && npair >= ntgt && npair <= (size_t)0x7fffffff,
                PFB_ERR_INVALID, "%s: %zu targets and %zu pairs for %d fine tiles", name, ntgt, npair, p.nfu() * p.nfv());
    if (int rc = wg_tile_map(p, name, {tgt_tile, tgt_ptr, pair_start, pair_count, pair_p0, ntgt, npair, nsorted}, stream);
        rc != PFB_OK) return rc;
    PFB_HIP_CHECK(hipMemsetAsync(grid, 0, p.grid_bytes() * (size_t)nprod, as_stream(stream)));
    return by_type(p.dtype, [&](auto t) {
        return by_int<WG_MIN_W, WG_MAX_W>(p.W, [&](auto w) {
            return by_int<1, WG_MAX_PROD>(nprod, [&](auto np) {
                return launch_groups(k_grid_tile<decltype(t), w(), np()>, ntgt, stream, val, coord, nsorted, plane,
                                     wg_geom(p), tgt_tile, tgt_ptr, pair_start, pair_count, pair_p0, grid);
            });
        });
    });
}

static int wg_degrid(const char* name, void* plan, int nprod, int plane, const void* grid, const double* coord,
                     size_t nsorted, size_t s0, size_t s1, void* acc, void* stream) {
    if (int rc = wg_check(plan, name, {{grid, CPLX}, {coord, F64}, {acc, CPLX}}); rc != PFB_OK) return rc;
    const WgridPlan& p = wg_plan(plan);
    if (int rc = wg_range(p, name, plane, s0, s1, nsorted); rc != PFB_OK) return rc;
    if (s1 == s0) return PFB_OK;
    return by_type(p.dtype, [&](auto t) {
        return by_int<WG_MIN_W, WG_MAX_W>(p.W, [&](auto w) {
            return by_int<1, WG_MAX_PROD>(nprod, [&](auto np) {
                return launch(k_degrid<decltype(t), w(), np()>, s1 - s0, stream, grid, coord, nsorted, s0, s1, plane,
                              wg_geom(p), acc);
            });
        });
    });
}

static int wg_image_forward(const char* name, void* plan, int nprod, int plane, const void* dirty, const void* beam,
                            const double* corr, const double* nm1, void* grid, void* stream) {
    if (int rc = wg_check(plan, name, {{dirty, REAL}, {beam, REAL, true}, {corr, F64}, {nm1, F64, true}, {grid, CPLX}});
        rc != PFB_OK) return rc;
    const WgridPlan& p = wg_plan(plan);
    if (int rc = wg_plane(p, name, plane); rc != PFB_OK) return rc;
    PFB_HIP_CHECK(hipMemsetAsync(grid, 0, p.grid_bytes() * (size_t)nprod, as_stream(stream)));
    return by_type(p.dtype, [&](auto t) {
        return by_int<1, WG_MAX_PROD>(nprod, [&](auto np) {
            return launch(k_image_forward<decltype(t), np()>, p.npix(), stream, dirty, beam, corr, nm1, p.wp(plane), p.nx,
                          p.ny, p.Nu, p.Nv, grid);
        });
    });
}

static int wg_image_adjoint(const char* name, void* plan, int nprod, int plane, const void* grid, const double* nm1,
                            void* img, void* stream) {
    if (int rc = wg_check(plan, name, {{grid, CPLX}, {nm1, F64, true}, {img, CPLX}}); rc != PFB_OK) return rc;
    const WgridPlan& p = wg_plan(plan);
    if (int rc = wg_plane(p, name, plane); rc != PFB_OK) return rc;
    return by_type(p.dtype, [&](auto t) {
        return by_int<1, WG_MAX_PROD>(nprod, [&](auto np) {
            return launch(k_image_adjoint<decltype(t), np()>, p.npix(), stream, grid, nm1, p.wp(plane), p.nx, p.ny, p.Nu,
                          p.Nv, img);
        });
    });
}

static int wg_image_correct(const char* name, void* plan, int nprod, const void* img, const double* corr,
                            const void* beam, void* dirty, void* stream) {
    if (int rc = wg_check(plan, name, {{img, CPLX}, {corr, F64}, {beam, REAL, true}, {dirty, REAL}}); rc != PFB_OK)
        return rc;
    const WgridPlan& p = wg_plan(plan);
    return by_type(p.dtype, [&](auto t) {
        return by_int<1, WG_MAX_PROD>(nprod, [&](auto np) {
            return launch(k_image_correct<decltype(t), np()>, p.npix(), stream, img, corr, beam, p.npix(), dirty);
        });
    });
}

}  // namespace pfb

using namespace pfb;

extern "C" {

int pfb_wgrid_plan_create(int dtype, int nx, int ny, double pixsize_x, double pixsize_y, double center_x,
                          double center_y, int support, int nplanes, double w0, double dw, void** plan) {
    PFB_REQUIRE(plan, PFB_ERR_INVALID, "wgrid_plan_create: null plan pointer");
    *plan = nullptr;
    PFB_REQUIRE(dtype == PFB_F32 || dtype == PFB_F64, PFB_ERR_INVALID, "wgrid_plan_create: bad dtype %d", dtype);
    PFB_REQUIRE(nx >= 2 && ny >= 2 && nx % 2 == 0 && ny % 2 == 0, PFB_ERR_INVALID,
                "wgrid_plan_create: nx %d, ny %d must be even and >= 2", nx, ny);
    PFB_REQUIRE(nx <= (1 << 29) && ny <= (1 << 29), PFB_ERR_UNSUPPORTED, "wgrid_plan_create: image %d x %d too large", nx, ny);
    PFB_REQUIRE(support >= WG_MIN_W && support <= WG_MAX_W, PFB_ERR_UNSUPPORTED,
                "wgrid_plan_create: support %d outside [%d, %d]", support, WG_MIN_W, WG_MAX_W);
    PFB_REQUIRE(2 * nx >= support && 2 * ny >= support, PFB_ERR_UNSUPPORTED,
                "wgrid_plan_create: grid %d x %d narrower than the support %d", 2 * nx, 2 * ny, support);
    PFB_REQUIRE(std::isfinite(pixsize_x) && std::isfinite(pixsize_y) && pixsize_x > 0 && pixsize_y > 0 &&
                std::isfinite(center_x) && std::isfinite(center_y), PFB_ERR_INVALID,
                "wgrid_plan_create: pixel sizes must be positive and finite, the centre finite");
    PFB_REQUIRE(nplanes == 1 || (nplanes > support && std::isfinite(w0) && std::isfinite(dw) && dw > 0), PFB_ERR_INVALID,
                "wgrid_plan_create: %d planes need a finite w0, dw > 0 and more planes than the support %d", nplanes, support);
    PFB_REQUIRE(nplanes >= 1 && nplanes <= (1 << 20), PFB_ERR_UNSUPPORTED, "wgrid_plan_create: %d planes", nplanes);
    int tile = 16;
    while ((size_t)((2 * nx + tile - 1) / tile) * ((2 * ny + tile - 1) / tile) > (size_t)WG_MAX_TILES) tile *= 2;
    const int ntu = (2 * nx + tile - 1) / tile, ntv = (2 * ny + tile - 1) / tile;
    const int np0 = nplanes > 1 ? nplanes - support + 1 : 1;
    PFB_REQUIRE((size_t)np0 * ntu * ntv <= (size_t)0x3fffffff, PFB_ERR_UNSUPPORTED,
                "wgrid_plan_create: %d planes x %d tiles exceed the key range", nplanes, ntu * ntv);
    WgridPlan* q = new (std::nothrow) WgridPlan();
    PFB_REQUIRE(q, PFB_ERR_ALLOC, "wgrid_plan_create: out of host memory");
    q->dtype = dtype; q->nx = nx; q->ny = ny; q->Nu = 2 * nx; q->Nv = 2 * ny; q->W = support; q->nplanes = nplanes;
    q->np0 = np0;
    q->px = pixsize_x; q->py = pixsize_y; q->cx = center_x; q->cy = center_y;
    q->w0 = std::isfinite(w0) ? w0 : 0.0; q->dw = nplanes > 1 ? dw : 1.0;
    q->tile = tile; q->ntu = ntu; q->ntv = ntv;
    *plan = q;
    return PFB_OK;
}

int pfb_wgrid_plan_destroy(void* plan) {
    delete static_cast<WgridPlan*>(plan);
    return PFB_OK;
}

int pfb_wgrid_plan_info(void* plan, int* nkeys, int* np0, int* tile) {
    if (int rc = wg_check(plan, "wgrid_plan_info", {}); rc != PFB_OK) return rc;
    const WgridPlan& p = wg_plan(plan);
    if (nkeys) *nkeys = p.nkeys();
    if (np0) *np0 = p.np0;
    if (tile) *tile = p.tile;
    return PFB_OK;
}

size_t pfb_wgrid_work_bytes(void* plan) { return plan ? 2 * sizeof(int) * (size_t)wg_plan(plan).nkeys() : 0; }

int pfb_wgrid_order_count(void* plan, const double* uvw, const double* freq, const unsigned char* mask, size_t nrow,
                          int nchan, int* keys, void* work, void* stream) {
    if (int rc = wg_check(plan, "wgrid_order_count", {{uvw, F64}, {freq, F64}, {keys, I32}, {work, I32}});
        rc != PFB_OK) return rc;
    if (int rc = check_nvis("wgrid_order_count", nrow, nchan); rc != PFB_OK) return rc;
    const size_t nvis = nrow * (size_t)nchan;
    PFB_HIP_CHECK(hipMemsetAsync(work, 0, pfb_wgrid_work_bytes(plan), as_stream(stream)));
    return launch(k_order_count, nvis, stream, uvw, freq, mask, nvis, nchan, wg_geom(wg_plan(plan)), keys, work);
}

int pfb_wgrid_order_fill(void* plan, const double* uvw, const double* freq, size_t nrow, int nchan, const int* keys,
                         const long long* offsets, void* work, size_t nsorted, int* idx, double* coord, void* stream) {
    if (int rc = wg_check(plan, "wgrid_order_fill", {{uvw, F64}, {freq, F64}, {keys, I32}, {offsets, I64},
                                                     {work, I32}, {idx, I32}, {coord, F64}});
        rc != PFB_OK) return rc;
    if (int rc = check_nvis("wgrid_order_fill", nrow, nchan); rc != PFB_OK) return rc;
    const WgridPlan& p = wg_plan(plan);
    const size_t nvis = nrow * (size_t)nchan;
    PFB_REQUIRE(nsorted >= 1 && nsorted <= nvis, PFB_ERR_INVALID, "wgrid_order_fill: %zu slots for %zu visibilities",
                nsorted, nvis);
    return launch(k_order_fill, nvis, stream, uvw, freq, nvis, nchan, wg_geom(p), keys, offsets, (int*)work + p.nkeys(),
                  nsorted, idx, coord);
}

int pfb_wgrid_order_keys64(void* plan, const double* uvw, const double* freq, const unsigned char* mask, size_t nrow,
                           int nchan, long long* keys, void* stream) {
    if (int rc = wg_check(plan, "wgrid_order_keys64", {{uvw, F64}, {freq, F64}, {keys, I64}}); rc != PFB_OK) return rc;
    if (int rc = check_nvis("wgrid_order_keys64", nrow, nchan); rc != PFB_OK) return rc;
    const size_t nvis = nrow * (size_t)nchan;
    return launch(k_order_keys64, nvis, stream, uvw, freq, mask, nvis, nchan, wg_geom(wg_plan(plan)), keys);
}

int pfb_wgrid_order_coords(void* plan, const double* uvw, const double* freq, size_t nrow, int nchan, const int* idx,
                           size_t nsorted, double* coord, void* stream) {
    if (int rc = wg_check(plan, "wgrid_order_coords", {{uvw, F64}, {freq, F64}, {idx, I32}, {coord, F64}});
        rc != PFB_OK) return rc;
    if (int rc = check_nvis("wgrid_order_coords", nrow, nchan); rc != PFB_OK) return rc;
    const size_t nvis = nrow * (size_t)nchan;
    PFB_REQUIRE(nsorted >= 1 && nsorted <= nvis, PFB_ERR_INVALID, "wgrid_order_coords: %zu slots for %zu visibilities",
                nsorted, nvis);
    return launch(k_order_coords, nsorted, stream, uvw, freq, nvis, nchan, wg_geom(wg_plan(plan)), idx, nsorted, coord);
}

int pfb_wgrid_prep(void* plan, const void* vis, const void* wgt, const int* idx, const double* coord, size_t nsorted,
                   void* val, void* stream) {
    return wg_prep("wgrid_prep", plan, 1, vis, wgt, 0, idx, coord, nsorted, 0, val, stream);
}

int pfb_wgrid_prep_multi(void* plan, int nprod, const void* vis, const void* wgt, int wgt_shared, const int* idx,
                         const double* coord, size_t nsorted, size_t nvis, void* val, void* stream) {
    if (int rc = wg_nprod("wgrid_prep_multi", nprod); rc != PFB_OK) return rc;
    PFB_REQUIRE(nsorted <= nvis && nvis <= (size_t)0x7fffffff, PFB_ERR_INVALID,
                "wgrid_prep_multi: %zu slots for %zu visibilities", nsorted, nvis);
    return wg_prep("wgrid_prep_multi", plan, nprod, vis, wgt, wgt_shared != 0, idx, coord, nsorted, nvis, val, stream);
}

int pfb_wgrid_finish(void* plan, const void* acc, const void* wgt, const int* idx, const double* coord, size_t nsorted,
                     void* vis, size_t nvis, void* stream) {
    return wg_finish("wgrid_finish", plan, 1, acc, wgt, 0, idx, coord, nsorted, vis, nvis, stream);
}

int pfb_wgrid_finish_multi(void* plan, int nprod, const void* acc, const void* wgt, int wgt_shared, const int* idx,
                           const double* coord, size_t nsorted, void* vis, size_t nvis, void* stream) {
    if (int rc = wg_nprod("wgrid_finish_multi", nprod); rc != PFB_OK) return rc;
    return wg_finish("wgrid_finish_multi", plan, nprod, acc, wgt, wgt_shared != 0, idx, coord, nsorted, vis, nvis, stream);
}

int pfb_wgrid_finish_block(void* plan, const void* acc, const int* idx, const double* coord, size_t nsorted,
                           int nchan_blk, void* out, int out_dtype, size_t row0, int nchan_out, int chan0, int ncorr,
                           int accumulate, void* stream) {
    PFB_REQUIRE(out_dtype == PFB_F32 || out_dtype == PFB_F64, PFB_ERR_INVALID, "wgrid_finish_block: bad out_dtype %d",
                out_dtype);
    if (int rc = wg_check(plan, "wgrid_finish_block", {{acc, CPLX}, {idx, I32}, {coord, F64},
                                                       {out, bytes(2 * esize(out_dtype))}});
        rc != PFB_OK) return rc;
    if (int rc = check_count("wgrid_finish_block", nsorted, PFB_ERR_INVALID); rc != PFB_OK) return rc;
    const WgridPlan& p = wg_plan(plan);
    PFB_REQUIRE(out_dtype == p.dtype || out_dtype == PFB_F32, PFB_ERR_INVALID,
                "wgrid_finish_block: a complex128 output under a single-precision plan");
    PFB_REQUIRE(ncorr >= 1 && ncorr <= 4, PFB_ERR_INVALID, "wgrid_finish_block: %d correlations outside 1 .. 4", ncorr);
    PFB_REQUIRE(nchan_blk >= 1 && chan0 >= 0 && nchan_out >= 1 &&
                (size_t)chan0 + (size_t)nchan_blk <= (size_t)nchan_out, PFB_ERR_INVALID,
                "wgrid_finish_block: channels %d .. + %d of %d", chan0, nchan_blk, nchan_out);
    return by_type(p.dtype, [&](auto t) {
        using T = decltype(t);
        if constexpr (std::is_same_v<T, double>) {
            if (out_dtype == PFB_F32)
                return launch(k_finish_block<T, float>, nsorted, stream, acc, idx, coord, nsorted, p.cxs(), p.cys(),
                              p.centre(), nchan_blk, out, row0, (size_t)nchan_out, (size_t)chan0, ncorr, accumulate);
        }
        return launch(k_finish_block<T, T>, nsorted, stream, acc, idx, coord, nsorted, p.cxs(), p.cys(), p.centre(),
                      nchan_blk, out, row0, (size_t)nchan_out, (size_t)chan0, ncorr, accumulate);
    });
}

int pfb_vis_restore_corrs(int dtype, const void* vis, size_t nvis, int ncorr, void* out, void* stream) {
    if (int rc = check(dtype, "vis_restore_corrs", {{vis, CPLX}, {out, CPLX}}); rc != PFB_OK) return rc;
    if (int rc = check_count("vis_restore_corrs", nvis, PFB_ERR_INVALID); rc != PFB_OK) return rc;
    PFB_REQUIRE(ncorr >= 1 && ncorr <= 4, PFB_ERR_INVALID, "vis_restore_corrs: %d correlations outside 1 .. 4", ncorr);
    const size_t n = nvis * (size_t)ncorr;
    return by_type(dtype, [&](auto t) {
        return launch(k_restore_corrs<decltype(t)>, n, stream, vis, n, ncorr, out);
    });
}

int pfb_wgrid_weight(void* plan, const void* acc, const void* wgt, const int* idx, size_t nsorted, void* val,
                     void* stream) {
    if (int rc = wg_check(plan, "wgrid_weight", {{acc, CPLX}, {wgt, REAL, true}, {idx, I32}, {val, CPLX}});
        rc != PFB_OK) return rc;
    if (int rc = check_count("wgrid_weight", nsorted, PFB_ERR_INVALID); rc != PFB_OK) return rc;
    return by_type(wg_plan(plan).dtype, [&](auto t) {
        return launch(k_weight<decltype(t)>, nsorted, stream, acc, wgt, idx, nsorted, val);
    });
}

int pfb_wgrid_grid(void* plan, int plane, const void* val, const double* coord, size_t nsorted, size_t s0, size_t s1,
                   void* grid, void* stream) {
    return wg_grid("wgrid_grid", plan, 1, plane, val, coord, nsorted, s0, s1, grid, stream);
}

int pfb_wgrid_grid_multi(void* plan, int nprod, int plane, const void* val, const double* coord, size_t nsorted,
                         size_t s0, size_t s1, void* grid, void* stream) {
    if (int rc = wg_nprod("wgrid_grid_multi", nprod); rc != PFB_OK) return rc;
    return wg_grid("wgrid_grid_multi", plan, nprod, plane, val, coord, nsorted, s0, s1, grid, stream);
}

int pfb_wgrid_grid_tile(void* plan, int plane, const void* val, const double* coord, size_t nsorted, const int* tgt_tile,
                        const long long* tgt_ptr, const long long* pair_start, const int* pair_count, const int* pair_p0,
                        size_t ntgt, size_t npair, void* grid, void* stream) {
    return wg_grid_tile("wgrid_grid_tile", plan, 1, plane, val, coord, nsorted, tgt_tile, tgt_ptr, pair_start, pair_count,
                        pair_p0, ntgt, npair, grid, stream);
}

int pfb_wgrid_grid_tile_multi(void* plan, int nprod, int plane, const void* val, const double* coord, size_t nsorted,
                              const int* tgt_tile, const long long* tgt_ptr, const long long* pair_start,
                              const int* pair_count, const int* pair_p0, size_t ntgt, size_t npair, void* grid,
                              void* stream) {
    if (int rc = wg_nprod("wgrid_grid_tile_multi", nprod); rc != PFB_OK) return rc;
    return wg_grid_tile("wgrid_grid_tile_multi", plan, nprod, plane, val, coord, nsorted, tgt_tile, tgt_ptr, pair_start,
                        pair_count, pair_p0, ntgt, npair, grid, stream);
}

int pfb_wgrid_degrid(void* plan, int plane, const void* grid, const double* coord, size_t nsorted, size_t s0, size_t s1,
                     void* acc, void* stream) {
    return wg_degrid("wgrid_degrid", plan, 1, plane, grid, coord, nsorted, s0, s1, acc, stream);
}

int pfb_wgrid_degrid_multi(void* plan, int nprod, int plane, const void* grid, const double* coord, size_t nsorted,
                           size_t s0, size_t s1, void* acc, void* stream) {
    if (int rc = wg_nprod("wgrid_degrid_multi", nprod); rc != PFB_OK) return rc;
    return wg_degrid("wgrid_degrid_multi", plan, nprod, plane, grid, coord, nsorted, s0, s1, acc, stream);
}

int pfb_wgrid_image_forward(void* plan, int plane, const void* dirty, const void* beam, const double* corr,
                            const double* nm1, void* grid, void* stream) {
    return wg_image_forward("wgrid_image_forward", plan, 1, plane, dirty, beam, corr, nm1, grid, stream);
}

int pfb_wgrid_image_forward_multi(void* plan, int nprod, int plane, const void* dirty, const void* beam,
                                  const double* corr, const double* nm1, void* grid, void* stream) {
    if (int rc = wg_nprod("wgrid_image_forward_multi", nprod); rc != PFB_OK) return rc;
    return wg_image_forward("wgrid_image_forward_multi", plan, nprod, plane, dirty, beam, corr, nm1, grid, stream);
}

int pfb_wgrid_image_adjoint(void* plan, int plane, const void* grid, const double* nm1, void* img, void* stream) {
    return wg_image_adjoint("wgrid_image_adjoint", plan, 1, plane, grid, nm1, img, stream);
}

int pfb_wgrid_image_adjoint_multi(void* plan, int nprod, int plane, const void* grid, const double* nm1, void* img,
                                  void* stream) {
    if (int rc = wg_nprod("wgrid_image_adjoint_multi", nprod); rc != PFB_OK) return rc;
    return wg_image_adjoint("wgrid_image_adjoint_multi", plan, nprod, plane, grid, nm1, img, stream);
}

int pfb_wgrid_image_correct(void* plan, const void* img, const double* corr, const void* beam, void* dirty, void* stream) {
    return wg_image_correct("wgrid_image_correct", plan, 1, img, corr, beam, dirty, stream);
}

int pfb_wgrid_image_correct_multi(void* plan, int nprod, const void* img, const double* corr, const void* beam,
                                  void* dirty, void* stream) {
    if (int rc = wg_nprod("wgrid_image_correct_multi", nprod); rc != PFB_OK) return rc;
    return wg_image_correct("wgrid_image_correct_multi", plan, nprod, img, corr, beam, dirty, stream);
}

}  // extern "C"
