// visconcat.hip -- the grid worker's merge of the datasets that `init` wrote, before anything is gridded
// (pfb/workers/grid.py:150-214, 404-412), DESIGN 4.14:
//   k_sum_overlap    sum_overlap (pfb/utils/misc.py:1030-1067): the weighted mean of the visibilities of the source
//                    datasets that share an output channel.  A lane per output (row, channel), the channel fastest: a
//                    source whose channels land on consecutive output channels is read coalesced.  Per source and
//                    element 1 map entry, and where it is not -1 one visibility, weight and mask byte; 1 visibility,
//                    weight and mask byte written
//   k_weight_sum     _sum_beam's wgt_i.sum() (misc.py:1017) over ALL elements, no mask, fp64: a partial per workgroup,
//                    then the one-workgroup sum of common.hpp into the device record (the two-stage form of imweight.hip)
//   k_beam_combine   _sum_beam's beam = sum_i wsum_i beam_i [/ sum_i wsum_i] with the sums read from the device record
//   k_beam_eval      _eval_beam (pfb/utils/beam.py:120-140): scipy's RegularGridInterpolator(method='linear',
//                    bounds_error=False, fill_value=None) -- bilinear inside, linearly extrapolated from the edge cell
//                    outside.  A lane per output pixel, j fastest; 2 binary searches, 4 beam values read, 1 written
// The sources of a call go to the kernel BY VALUE, PFB_VIS_BATCH at a time (no device table of pointers to fill and
// keep alive): a batch after the first reads the partial sums back from the outputs, the last one closes.  Partial sums
// are of the data's type, so the round trip through memory is exact: any number of sources gives the bits of one
// ordered sum.  No atomics anywhere: the same bits from run to run.
#include "entry.hpp"

namespace pfb {

constexpr int VIS_BATCH = PFB_VIS_BATCH;

template <typename T>
struct VisSrc {
    const cplx<T>* vis;
    const T* wgt;
    const u8* mask;
    int nchan;
};
template <typename T>
struct VisBatch { VisSrc<T> s[VIS_BATCH]; };

template <typename T>
struct BeamBatch { const T* beam[VIS_BATCH]; };

// ------------------------------------------------------------------------------------------------- sum_overlap
// map (n, nchan_out): the channel of source i that lands in output channel c, or -1; an entry outside [0, nchan_i) is
// read as -1, so that no map addresses outside a source.  Every product and sum is rounded on its own, in the order
// numpy forms them: (vis * wgt) * mask added to the sum, wgt * mask added to the sum.
template <typename T>
__global__ void __launch_bounds__(ENTRY_BLOCK)
k_sum_overlap(VisBatch<T> b, int n, const int* __restrict__ map, size_t nvis, int nchan_out, int first, int last,
              cplx<T>* __restrict__ viso, T* __restrict__ wgto, u8* __restrict__ masko) {
#pragma clang fp contract(off)
    const size_t t = (size_t)blockIdx.x * ENTRY_BLOCK + threadIdx.x;
    if (t >= nvis) return;
    const size_t r = t / nchan_out;
    const int c = (int)(t - r * nchan_out);
    T re = T(0), im = T(0), w = T(0);
    u8 any = 0;
    if (!first) {
        const cplx<T> v = viso[t];
        re = v.x; im = v.y; w = wgto[t]; any = masko[t];
    }
#pragma unroll
    for (int i = 0; i < VIS_BATCH; ++i) {
        if (i < n) {
            const int sc = map[(size_t)i * nchan_out + c];
            if ((unsigned)sc < (unsigned)b.s[i].nchan) {
                const size_t at = r * (size_t)b.s[i].nchan + sc;
                const cplx<T> v = b.s[i].vis[at];
                const T wi = b.s[i].wgt[at];
                const u8 m = b.s[i].mask[at];
                const T f = (T)m;
                re += (v.x * wi) * f;
                im += (v.y * wi) * f;
                w += wi * f;
                any |= m ? 1 : 0;
            }
        }
    }
    if (last) {
        if (any) { re = re / w; im = im / w; }
        else { re = T(0); im = T(0); w = T(0); }
    }
    viso[t] = cplx<T>(re, im);
    wgto[t] = w;
    masko[t] = any;
}

// ---------------------------------------------------------------------------------------------------- sum_beam
template <typename T>
__global__ void __launch_bounds__(ENTRY_BLOCK)
k_weight_sum(const T* __restrict__ wgt, size_t n, double* __restrict__ ws) {
    double acc[1] = {0.0};
    for (size_t i = (size_t)blockIdx.x * ENTRY_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * ENTRY_BLOCK)
        acc[0] += (double)wgt[i];
    emit_partials<1>(acc, ws);
}

// wsum (nds) fp64, the record; this launch adds the beams of sources [i0, i0 + n).  The last launch divides by the sum
// of the whole record, added in dataset order, where that is not zero
template <typename T>
__global__ void __launch_bounds__(ENTRY_BLOCK)
k_beam_combine(BeamBatch<T> b, int n, int i0, int nds, const double* __restrict__ wsum, size_t npix, int last,
               T* __restrict__ out) {
#pragma clang fp contract(off)
    const size_t p = (size_t)blockIdx.x * ENTRY_BLOCK + threadIdx.x;
    if (p >= npix) return;
    T acc = i0 ? out[p] : T(0);
#pragma unroll
    for (int i = 0; i < VIS_BATCH; ++i)
        if (i < n) acc += (T)wsum[i0 + i] * b.beam[i][p];
    if (last) {
        double tot = 0.0;
        for (int i = 0; i < nds; ++i) tot += wsum[i];
        if (tot != 0.0) acc = acc / (T)tot;
    }
    out[p] = acc;
}

// --------------------------------------------------------------------------------------------------- eval_beam
// the cell of x on the ascending axis g (n >= 2): the i of g[i] <= x < g[i + 1] clipped to [0, n - 2], x == g[n - 1] in
// the last cell; a NaN lands in cell 0 and stays a NaN in the distance
__device__ __forceinline__ int beam_cell(const double* __restrict__ g, int n, double x) {
    int lo = 0, hi = n - 1;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (g[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

template <typename T, typename O>
__global__ void __launch_bounds__(ENTRY_BLOCK)
k_beam_eval(const T* __restrict__ beam, int nl, int nm, const double* __restrict__ l_in, const double* __restrict__ m_in,
            const double* __restrict__ l_out, const double* __restrict__ m_out, int coord2d, size_t npix, int nyo,
            O* __restrict__ out) {
#pragma clang fp contract(off)
    const size_t p = (size_t)blockIdx.x * ENTRY_BLOCK + threadIdx.x;
    if (p >= npix) return;
    const size_t io = p / nyo;
    const double x = coord2d ? l_out[p] : l_out[io];
    const double y = coord2d ? m_out[p] : m_out[p - io * nyo];
    const int i = beam_cell(l_in, nl, x), j = beam_cell(m_in, nm, y);
    const double tx = (x - l_in[i]) / (l_in[i + 1] - l_in[i]);
    const double ty = (y - m_in[j]) / (m_in[j + 1] - m_in[j]);
    const T* __restrict__ v = beam + (size_t)i * nm + j;
    const double v00 = (double)v[0], v01 = (double)v[1], v10 = (double)v[nm], v11 = (double)v[nm + 1];
    const double r = v00 * ((1.0 - tx) * (1.0 - ty)) + v01 * ((1.0 - tx) * ty) + v10 * (tx * (1.0 - ty)) + v11 * (tx * ty);
    out[p] = (O)r;
}

static inline size_t vis_stream_threads(size_t n) {
    const size_t cap = (size_t)(PFB_IMW_WORK_DOUBLES / PFB_IMW_RECORD) * ENTRY_BLOCK;
    return n < cap ? n : cap;
}

}  // namespace pfb

using namespace pfb;

extern "C" {

int pfb_vis_sum_overlap(int dtype, int nds, const void* const* vis, const void* const* wgt,
                        const unsigned char* const* mask, const size_t* nrows, const int* nchans, const int* chan_map,
                        size_t nrow, int nchan_out, void* viso, void* wgto, unsigned char* masko, void* stream) {
    if (int rc = check(dtype, "vis_sum_overlap", {{vis, bytes(8)}, {wgt, bytes(8)}, {mask, bytes(8)}, {nrows, bytes(8)},
                                                  {nchans, I32}, {chan_map, I32}, {viso, CPLX}, {wgto, REAL}, {masko, U8}});
        rc != PFB_OK) return rc;
    PFB_REQUIRE(nds >= 1, PFB_ERR_INVALID, "vis_sum_overlap: %d sources", nds);
    if (int rc = check_nvis("vis_sum_overlap", nrow, nchan_out); rc != PFB_OK) return rc;
    for (int i = 0; i < nds; ++i) {
        if (int rc = check(dtype, "vis_sum_overlap", {{vis[i], CPLX}, {wgt[i], REAL}, {mask[i], U8}}); rc != PFB_OK)
            return rc;
        PFB_REQUIRE(nrows[i] == nrow, PFB_ERR_INVALID, "vis_sum_overlap: source %d has %zu rows, the output %zu", i,
                    nrows[i], nrow);
        if (int rc = check_nvis("vis_sum_overlap", nrow, nchans[i]); rc != PFB_OK) return rc;
    }
    const size_t nvis = nrow * (size_t)nchan_out;
    return by_type(dtype, [&](auto t) {
        using T = decltype(t);
        for (int i0 = 0; i0 < nds; i0 += VIS_BATCH) {
            const int n = nds - i0 < VIS_BATCH ? nds - i0 : VIS_BATCH;
            VisBatch<T> b{};
            for (int i = 0; i < n; ++i)
                b.s[i] = {static_cast<const cplx<T>*>(vis[i0 + i]), static_cast<const T*>(wgt[i0 + i]), mask[i0 + i],
                          nchans[i0 + i]};
            if (int rc = launch(k_sum_overlap<T>, nvis, stream, b, n, chan_map + (size_t)i0 * nchan_out, nvis, nchan_out,
                                (int)(i0 == 0), (int)(i0 + n == nds), viso, wgto, masko);
                rc != PFB_OK) return rc;
        }
        return (int)PFB_OK;
    });
}

int pfb_vis_weight_sums(int dtype, const void* wgt, size_t n, double* rec, double* work, void* stream) {
    if (int rc = check(dtype, "vis_weight_sums", {{wgt, REAL}, {rec, F64}, {work, F64}}); rc != PFB_OK) return rc;
    if (int rc = check_count("vis_weight_sums", n, PFB_ERR_UNSUPPORTED); rc != PFB_OK) return rc;
    const unsigned groups = blocks(vis_stream_threads(n));
    const int rc = by_type(dtype, [&](auto t) {
        return launch_groups(k_weight_sum<decltype(t)>, groups, stream, wgt, n, work);
    });
    return rc != PFB_OK ? rc : final_sum(work, groups, 1, rec, stream);
}

int pfb_beam_combine(int dtype, int nds, const void* const* beams, const double* wsum, size_t npix, void* out,
                     void* stream) {
    if (int rc = check(dtype, "beam_combine", {{beams, bytes(8)}, {wsum, F64}, {out, REAL}}); rc != PFB_OK) return rc;
    PFB_REQUIRE(nds >= 1, PFB_ERR_INVALID, "beam_combine: %d sources", nds);
    if (int rc = check_count("beam_combine", npix, PFB_ERR_UNSUPPORTED); rc != PFB_OK) return rc;
    for (int i = 0; i < nds; ++i)
        if (int rc = check(dtype, "beam_combine", {{beams[i], REAL}}); rc != PFB_OK) return rc;
    return by_type(dtype, [&](auto t) {
        using T = decltype(t);
        for (int i0 = 0; i0 < nds; i0 += VIS_BATCH) {
            const int n = nds - i0 < VIS_BATCH ? nds - i0 : VIS_BATCH;
            BeamBatch<T> b{};
            for (int i = 0; i < n; ++i) b.beam[i] = static_cast<const T*>(beams[i0 + i]);
            if (int rc = launch(k_beam_combine<T>, npix, stream, b, n, i0, nds, wsum, npix, (int)(i0 + n == nds), out);
                rc != PFB_OK) return rc;
        }
        return (int)PFB_OK;
    });
}

int pfb_beam_eval(int dtype, const void* beam, int nl, int nm, const double* l_in, const double* m_in,
                  const double* l_out, const double* m_out, int coord2d, int nxo, int nyo, int out_dtype, void* out,
                  void* stream) {
    if (int rc = check(dtype, "beam_eval", {{beam, REAL}, {l_in, F64}, {m_in, F64}, {l_out, F64}, {m_out, F64}});
        rc != PFB_OK) return rc;
    if (int rc = check(out_dtype, "beam_eval", {{out, REAL}}); rc != PFB_OK) return rc;
    PFB_REQUIRE(nl >= 2 && nm >= 2 && (size_t)nl <= (size_t)0x7fffffff / (size_t)nm, PFB_ERR_INVALID,
                "beam_eval: a %d x %d beam; both axes need 2 nodes, the beam fewer than 2^31 pixels", nl, nm);
    PFB_REQUIRE(nxo >= 1 && nyo >= 1 && (size_t)nxo <= (size_t)0x7fffffff / (size_t)nyo, PFB_ERR_UNSUPPORTED,
                "beam_eval: %d x %d output pixels outside [1, 2^31)", nxo, nyo);
    const size_t npix = (size_t)nxo * nyo;
    return by_type(dtype, [&](auto t) {
        return by_type(out_dtype, [&](auto o) {
            return launch(k_beam_eval<decltype(t), decltype(o)>, npix, stream, beam, nl, nm, l_in, m_in, l_out, m_out,
                          coord2d ? 1 : 0, npix, nyo, out);
        });
    });
}

}  // extern "C"
