// stokes.hip -- Stokes visibilities and weights from correlations and Jones terms (pfb/utils/weighting.py:281-350 over
// the functions that pfb/utils/stokes.py generates, and the preparation of pfb/utils/stokes2im.py:98-195), DESIGN 4.12:
//   k_stokes   one streaming pass: a (row, channel) visibility per thread, channels fastest.  With Gp, Gq the 2 x 2 Jones
//              matrices of the row's two antennas at its time bin and channel, V the 2 x 2 matrix of its correlations,
//              w their weights and B the Stokes basis matrix,
//                  vis = 1/2 tr(B^H Gp^-1 V Gq^-H)            wgt = sum_ab w_ab |(Gp B Gq^H)_ab|^2
//              the closed form of the reference's generated expressions (the weights cancel out of its C).  Fused into
//              the pass: data +- data2, the weight forms (ones, 1 / sigma^2, a spectrum, a row weight), the flag
//              any(flag[row, chan, :]) | frow[row] | ant1[row] == ant2[row], mask = !flag as bytes, and the fp64 sum of
//              the unflagged wgt (a partial per workgroup, then k_final_sum of common.hpp: the same bits every run).
//   k_stokes_multi   the same pass for up to four products at once: every input of a visibility is read once, product k
//              lands in plane k of vis and wgt (nprod, nrow, nchan); what the bases share is formed once
//   k_chan_average, k_chan_average_lane   the weighted mean of vis, wgt, mask over bins of chan_average channels, a pass
//              of its own behind the ones above
// The Stokes kernels are templated on the type, the Jones mode (diagonal with 4 or 2 correlations, full 2 x 2 with 4,
// none with 4 or 2) and the basis; the weight form, the flags and the second column are uniform branches.
//
// A workgroup takes STK_BLOCK / nchan whole rows at a time (one row when nchan > STK_BLOCK): its first lanes find their
// row's time bin by a binary search over tbin_idx and leave (bin, ant1, ant2) in LDS, then every lane takes visibilities
// of those rows, consecutive lanes consecutive (row, channel) pairs: the correlations, weights and flags of a wave are
// one contiguous stretch read in 16-byte pieces, the Jones terms of a row contiguous along its channels, the three stores
// coalesced.  Flagged or uncovered visibilities are SELECTED to zero: whatever their data and weights hold (NaN, Inf)
// never reaches an output.  A row whose antenna is outside [0, nant) counts as uncovered: nothing addresses outside
// the arrays, whatever the input.  Every index is a size_t.
#include "entry.hpp"

namespace pfb {

constexpr int STK_BLOCK = ENTRY_BLOCK;
// at most this many workgroups stride over the row groups: one partial each in the reduction scratch
constexpr int STK_MAX_GROUPS = 4096;
static_assert(STK_MAX_GROUPS <= PFB_REDUCE_WS_DOUBLES, "one fp64 partial per workgroup");

struct StkArgs {
    const void* data; const void* data2; const void* weight; const void* jones;
    const u8* flag; const u8* frow;
    const int* ant1; const int* ant2;
    const long long* tbin_idx; const long long* tbin_counts;
    long long tbin_off;
    size_t nrow, ngroups;
    int nchan, rows_per_group, ntime, nant, ndir, wform, nflagcorr, autocorr, subtract;
    void* vis; void* wgt; u8* mask;
    double* ws;
};

constexpr bool stk_has_jones(int mode) { return mode <= PFB_STOKES_FULL4; }
constexpr int stk_ncorr(int mode) { return mode == PFB_STOKES_DIAG2 || mode == PFB_STOKES_NOJ2 ? 2 : 4; }
constexpr int stk_njones(int mode) { return mode == PFB_STOKES_FULL4 ? 4 : 2; }

// BYTES contiguous bytes at p (aligned to min(BYTES, 16)) in the widest loads; NT: read once, keep out of the caches' way
template <int BYTES, bool NT>
__device__ __forceinline__ void stk_load(const void* __restrict__ p, void* __restrict__ dst) {
    if constexpr (BYTES >= 16) {
        typedef float v4f __attribute__((ext_vector_type(4)));
#pragma unroll
        for (int i = 0; i < BYTES / 16; ++i) {
            const v4f v = NT ? __builtin_nontemporal_load(static_cast<const v4f*>(p) + i) : static_cast<const v4f*>(p)[i];
            memcpy(static_cast<char*>(dst) + 16 * i, &v, 16);
        }
    } else if constexpr (BYTES == 8) {
        const v2f v = NT ? __builtin_nontemporal_load(static_cast<const v2f*>(p)) : *static_cast<const v2f*>(p);
        memcpy(dst, &v, 8);
    } else if constexpr (BYTES == 4) {
        const unsigned v = NT ? __builtin_nontemporal_load(static_cast<const unsigned*>(p)) : *static_cast<const unsigned*>(p);
        memcpy(dst, &v, 4);
    } else {
        static_assert(BYTES == 2, "2, 4, 8 or a multiple of 16 bytes");
        const unsigned short v = NT ? __builtin_nontemporal_load(static_cast<const unsigned short*>(p))
                                    : *static_cast<const unsigned short*>(p);
        memcpy(dst, &v, 2);
    }
}

template <typename T> __device__ __forceinline__ T stk_abs2(cplx<T> a) { return a.x * a.x + a.y * a.y; }
// a / d
template <typename T> __device__ __forceinline__ cplx<T> stk_div(cplx<T> a, cplx<T> d) {
    const cplx<T> n = mulc(a, d);
    const T s = stk_abs2(d);
    return {n.x / s, n.y / s};
}
// 1/2 tr(B^H X) from the two entries of X that the basis reads: (x00, x11) for B = 1, diag(1, -1); (x01, x10) for
// [[0, 1], [1, 0]], [[0, i], [-i, 0]]
template <int BASIS, typename T> __device__ __forceinline__ cplx<T> stk_trace(cplx<T> a, cplx<T> b) {
    if constexpr (BASIS == 0 || BASIS == 2) return T(0.5) * (a + b);
    else if constexpr (BASIS == 1) return T(0.5) * (a - b);
    else return T(0.5) * mul_i(b - a);
}

// v: the correlations (v00, v01, v10, v11), or (v00, v11) of two; w: their weights; gp, gq: the Jones terms (g00, g11)
// or (g00, g01, g10, g11)
template <typename T, int MODE, int BASIS>
__device__ __forceinline__ void stk_eval(const cplx<T>* v, const T* w, const cplx<T>* gp, const cplx<T>* gq, cplx<T>& vis,
                                         T& wgt) {
    constexpr bool offdiag = BASIS >= 2;
    constexpr int NC = stk_ncorr(MODE);
    // the two correlations and weights that a diagonal Jones term pairs with this basis; with two correlations the
    // reference takes v01 = v10 = 0 and w01 = w10 = 1
    cplx<T> va, vb;
    T wa, wb;
    if constexpr (NC == 4) {
        va = v[offdiag ? 1 : 0]; vb = v[offdiag ? 2 : 3];
        wa = w[offdiag ? 1 : 0]; wb = w[offdiag ? 2 : 3];
    } else if constexpr (offdiag) {
        va = vb = cplx<T>(T(0), T(0));
        wa = wb = T(1);
    } else {
        va = v[0]; vb = v[1];
        wa = w[0]; wb = w[1];
    }
    if constexpr (!stk_has_jones(MODE)) {
        vis = stk_trace<BASIS>(va, vb);
        wgt = wa + wb;
    } else if constexpr (MODE != PFB_STOKES_FULL4) {
        // x_ab = v_ab / (gp_aa conj(gq_bb)), (Gp B Gq^H)_ab = +- gp_aa conj(gq_bb) on the basis' two entries
        const cplx<T> da = mulc(gp[0], gq[offdiag ? 1 : 0]), db = mulc(gp[1], gq[offdiag ? 0 : 1]);
        vis = stk_trace<BASIS>(stk_div(va, da), stk_div(vb, db));
        wgt = wa * stk_abs2(da) + wb * stk_abs2(db);
    } else {
        // X = adj(Gp) V adj(Gq)^H / (det Gp conj(det Gq)), adj G = [[g11, -g01], [-g10, g00]]
        const cplx<T> m00 = gp[3] * v[0] - gp[1] * v[2], m01 = gp[3] * v[1] - gp[1] * v[3];
        const cplx<T> m10 = gp[0] * v[2] - gp[2] * v[0], m11 = gp[0] * v[3] - gp[2] * v[1];
        cplx<T> xa, xb;
        if constexpr (!offdiag) {
            xa = mulc(m00, gq[3]) - mulc(m01, gq[1]);           // x00 = m00 conj(c00) + m01 conj(c01)
            xb = mulc(m11, gq[0]) - mulc(m10, gq[2]);           // x11 = m10 conj(c10) + m11 conj(c11)
        } else {
            xa = mulc(m01, gq[0]) - mulc(m00, gq[2]);           // x01 = m00 conj(c10) + m01 conj(c11)
            xb = mulc(m10, gq[3]) - mulc(m11, gq[1]);           // x10 = m10 conj(c00) + m11 conj(c01)
        }
        const cplx<T> dp = gp[0] * gp[3] - gp[1] * gp[2], dq = gq[0] * gq[3] - gq[1] * gq[2];
        vis = stk_div(stk_trace<BASIS>(xa, xb), mulc(dp, dq));
        // E_ab = gp_a0 conj(gq_b{0|1}) +- gp_a1 conj(gq_b{1|0})
        wgt = T(0);
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const cplx<T> e0 = mulc(gp[2 * a], gq[2 * b + (offdiag ? 1 : 0)]);
                const cplx<T> e1 = mulc(gp[2 * a + 1], gq[2 * b + (offdiag ? 0 : 1)]);
                wgt += w[2 * a + b] * stk_abs2((BASIS == 0 || BASIS == 2) ? e0 + e1 : e0 - e1);
            }
        }
    }
}

template <typename T, int MODE, int BASIS>
__global__ void __launch_bounds__(STK_BLOCK)
k_stokes(StkArgs a) {
    constexpr int NC = stk_ncorr(MODE), NJ = stk_njones(MODE);
    __shared__ int s_bin[STK_BLOCK], s_p[STK_BLOCK], s_q[STK_BLOCK];
    const cplx<T>* __restrict__ data = static_cast<const cplx<T>*>(a.data);
    const cplx<T>* __restrict__ data2 = static_cast<const cplx<T>*>(a.data2);
    const T* __restrict__ weight = static_cast<const T*>(a.weight);
    const cplx<T>* __restrict__ jones = static_cast<const cplx<T>*>(a.jones);
    cplx<T>* __restrict__ vis = static_cast<cplx<T>*>(a.vis);
    T* __restrict__ wgt = static_cast<T*>(a.wgt);
    const unsigned nchan = (unsigned)a.nchan;
    double acc[1] = {0.0};
    for (size_t g = blockIdx.x; g < a.ngroups; g += gridDim.x) {
        const size_t r0 = g * (size_t)a.rows_per_group;
        const unsigned nr = (unsigned)(a.nrow - r0 < (size_t)a.rows_per_group ? a.nrow - r0 : (size_t)a.rows_per_group);
        __syncthreads();                                        // the readers of the group before
        if (threadIdx.x < nr) {
            // the last bin that starts at or before the row (bins ascend; empty ones share their start with the next)
            const size_t r = r0 + threadIdx.x;
            const long long row = (long long)r;
            int lo = 0, hi = a.ntime;                           // tbin_idx[lo] - off <= row (lo = 0: off is the minimum)
            while (hi - lo > 1) {
                const int mid = lo + (hi - lo) / 2;
                if (a.tbin_idx[mid] - a.tbin_off <= row) lo = mid; else hi = mid;
            }
            const int p = a.ant1[r], q = a.ant2[r];
            const bool covered = row - (a.tbin_idx[lo] - a.tbin_off) < a.tbin_counts[lo] &&
                                 p >= 0 && p < a.nant && q >= 0 && q < a.nant;
            bool frow = a.autocorr && p == q;
            if (a.frow) frow = frow || a.frow[r] != 0;
            s_bin[threadIdx.x] = frow ? -2 : covered ? lo : -1;
            s_p[threadIdx.x] = p;
            s_q[threadIdx.x] = q;
        }
        __syncthreads();
        const unsigned n = nr * nchan;                          // <= STK_BLOCK, or one row
        for (unsigned i = threadIdx.x; i < n; i += STK_BLOCK) {
            const unsigned lr = a.rows_per_group == 1 ? 0u : i / nchan;
            const unsigned chan = i - lr * nchan;
            const size_t r = r0 + lr;
            const size_t t = r * nchan + chan;
            const int bin = s_bin[lr];
            bool flagged = bin == -2;
            if (a.nflagcorr == 1) {
                flagged = flagged || __builtin_nontemporal_load(a.flag + t) != 0;
            } else if (a.nflagcorr) {
                unsigned f = 0;
                stk_load<NC, true>(a.flag + t * NC, &f);
                flagged = flagged || f != 0;
            }
            const bool live = !flagged && bin >= 0;
            cplx<T> v[NC];
            stk_load<NC * (int)sizeof(cplx<T>), true>(data + t * NC, v);
            if (data2) {
                cplx<T> d[NC];
                stk_load<NC * (int)sizeof(cplx<T>), true>(data2 + t * NC, d);
#pragma unroll
                for (int c = 0; c < NC; ++c) v[c] = a.subtract ? v[c] - d[c] : v[c] + d[c];
            }
            T w[NC];
            if (a.wform == PFB_STOKES_W_NONE) {
#pragma unroll
                for (int c = 0; c < NC; ++c) w[c] = T(1);
            } else if (a.wform == PFB_STOKES_W_ROW) {
                stk_load<NC * (int)sizeof(T), false>(weight + r * NC, w);
            } else {
                stk_load<NC * (int)sizeof(T), true>(weight + t * NC, w);
                if (a.wform == PFB_STOKES_W_SIGMA) {
#pragma unroll
                    for (int c = 0; c < NC; ++c) w[c] = T(1) / (w[c] * w[c]);
                }
            }
            cplx<T> gp[NJ], gq[NJ];
            if constexpr (stk_has_jones(MODE)) {
                // an uncovered row reads the first entry and drops the result
                const size_t tb = live ? (size_t)bin : 0, p = live ? (size_t)s_p[lr] : 0, q = live ? (size_t)s_q[lr] : 0;
                const size_t step = (size_t)a.ndir * NJ;
                stk_load<NJ * (int)sizeof(cplx<T>), false>(jones + ((tb * a.nant + p) * nchan + chan) * step, gp);
                stk_load<NJ * (int)sizeof(cplx<T>), false>(jones + ((tb * a.nant + q) * nchan + chan) * step, gq);
            }
            cplx<T> ov;
            T ow;
            stk_eval<T, MODE, BASIS>(v, w, gp, gq, ov, ow);
            vis[t] = live ? ov : cplx<T>(T(0), T(0));
            wgt[t] = live ? ow : T(0);
            a.mask[t] = flagged ? 0 : 1;
            acc[0] += live ? (double)ow : 0.0;
        }
    }
    emit_partials<1>(acc, a.ws);
}

// --------------------------------------------------------------------------------- several products in one pass
// Up to four products of one chunk: the correlations, weights, flags and Jones terms of a visibility are read once, and
// product k lands in plane k of vis and wgt, (nprod, nrow, nchan); the mask does not depend on the product.
constexpr int STK_MAX_PROD = 4;
// four partials per workgroup in the reduction scratch
constexpr int STK_MULTI_MAX_GROUPS = 2048;
static_assert(STK_MAX_PROD * STK_MULTI_MAX_GROUPS <= PFB_REDUCE_WS_DOUBLES, "four fp64 partials per workgroup");

struct StkMultiArgs {
    StkArgs s;                         // vis, wgt: plane 0
    int nprod;
    int basis[STK_MAX_PROD];           // of plane k < nprod
    int plane[4];                      // of basis b, or -1
};

// what stk_eval<T, MODE, B> gives for the two bases of a family -- (0, 1), or (2, 3) with OFFDIAG -- with everything
// they share formed once: the two entries of X, the divisors, the products of the Jones terms.  m, dpq: the FULL mode's
// adj(Gp) V and det Gp conj(det Gq), the same for both families
template <typename T, int MODE, bool OFFDIAG>
__device__ __forceinline__ void stk_eval_family(const cplx<T>* v, const T* w, const cplx<T>* gp, const cplx<T>* gq,
                                                const cplx<T>* m, cplx<T> dpq, cplx<T>& vis_sum, cplx<T>& vis_dif,
                                                T& wgt_sum, T& wgt_dif) {
    constexpr int NC = stk_ncorr(MODE);
    constexpr int BS = OFFDIAG ? 2 : 0, BD = OFFDIAG ? 3 : 1;
    cplx<T> va, vb;
    T wa, wb;
    if constexpr (NC == 4) {
        va = v[OFFDIAG ? 1 : 0]; vb = v[OFFDIAG ? 2 : 3];
        wa = w[OFFDIAG ? 1 : 0]; wb = w[OFFDIAG ? 2 : 3];
    } else if constexpr (OFFDIAG) {
        va = vb = cplx<T>(T(0), T(0));
        wa = wb = T(1);
    } else {
        va = v[0]; vb = v[1];
        wa = w[0]; wb = w[1];
    }
    if constexpr (!stk_has_jones(MODE)) {
        vis_sum = stk_trace<BS>(va, vb);
        vis_dif = stk_trace<BD>(va, vb);
        wgt_sum = wgt_dif = wa + wb;
    } else if constexpr (MODE != PFB_STOKES_FULL4) {
        const cplx<T> da = mulc(gp[0], gq[OFFDIAG ? 1 : 0]), db = mulc(gp[1], gq[OFFDIAG ? 0 : 1]);
        const cplx<T> xa = stk_div(va, da), xb = stk_div(vb, db);
        vis_sum = stk_trace<BS>(xa, xb);
        vis_dif = stk_trace<BD>(xa, xb);
        wgt_sum = wgt_dif = wa * stk_abs2(da) + wb * stk_abs2(db);
    } else {
        cplx<T> xa, xb;
        if constexpr (!OFFDIAG) {
            xa = mulc(m[0], gq[3]) - mulc(m[1], gq[1]);
            xb = mulc(m[3], gq[0]) - mulc(m[2], gq[2]);
        } else {
            xa = mulc(m[1], gq[0]) - mulc(m[0], gq[2]);
            xb = mulc(m[2], gq[3]) - mulc(m[3], gq[1]);
        }
        vis_sum = stk_div(stk_trace<BS>(xa, xb), dpq);
        vis_dif = stk_div(stk_trace<BD>(xa, xb), dpq);
        wgt_sum = wgt_dif = T(0);
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const cplx<T> e0 = mulc(gp[2 * a], gq[2 * b + (OFFDIAG ? 1 : 0)]);
                const cplx<T> e1 = mulc(gp[2 * a + 1], gq[2 * b + (OFFDIAG ? 0 : 1)]);
                wgt_sum += w[2 * a + b] * stk_abs2(e0 + e1);
                wgt_dif += w[2 * a + b] * stk_abs2(e0 - e1);
            }
        }
    }
}

template <typename T, int MODE>
__global__ void __launch_bounds__(STK_BLOCK)
k_stokes_multi(StkMultiArgs ma) {
    constexpr int NC = stk_ncorr(MODE), NJ = stk_njones(MODE);
    __shared__ int s_bin[STK_BLOCK], s_p[STK_BLOCK], s_q[STK_BLOCK];
    const StkArgs& a = ma.s;
    const cplx<T>* __restrict__ data = static_cast<const cplx<T>*>(a.data);
    const cplx<T>* __restrict__ data2 = static_cast<const cplx<T>*>(a.data2);
    const T* __restrict__ weight = static_cast<const T*>(a.weight);
    const cplx<T>* __restrict__ jones = static_cast<const cplx<T>*>(a.jones);
    cplx<T>* __restrict__ vis = static_cast<cplx<T>*>(a.vis);
    T* __restrict__ wgt = static_cast<T*>(a.wgt);
    const unsigned nchan = (unsigned)a.nchan;
    const size_t nvis = a.nrow * (size_t)nchan;                 // a plane
    const bool fam0 = ma.plane[0] >= 0 || ma.plane[1] >= 0, fam1 = ma.plane[2] >= 0 || ma.plane[3] >= 0;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};                       // by basis
    for (size_t g = blockIdx.x; g < a.ngroups; g += gridDim.x) {
        const size_t r0 = g * (size_t)a.rows_per_group;
        const unsigned nr = (unsigned)(a.nrow - r0 < (size_t)a.rows_per_group ? a.nrow - r0 : (size_t)a.rows_per_group);
        __syncthreads();                                        // the readers of the group before
        if (threadIdx.x < nr) {
            const size_t r = r0 + threadIdx.x;
            const long long row = (long long)r;
            int lo = 0, hi = a.ntime;
            while (hi - lo > 1) {
                const int mid = lo + (hi - lo) / 2;
                if (a.tbin_idx[mid] - a.tbin_off <= row) lo = mid; else hi = mid;
            }
            const int p = a.ant1[r], q = a.ant2[r];
            const bool covered = row - (a.tbin_idx[lo] - a.tbin_off) < a.tbin_counts[lo] &&
                                 p >= 0 && p < a.nant && q >= 0 && q < a.nant;
            bool frow = a.autocorr && p == q;
            if (a.frow) frow = frow || a.frow[r] != 0;
            s_bin[threadIdx.x] = frow ? -2 : covered ? lo : -1;
            s_p[threadIdx.x] = p;
            s_q[threadIdx.x] = q;
        }
        __syncthreads();
        const unsigned n = nr * nchan;                          // <= STK_BLOCK, or one row
        for (unsigned i = threadIdx.x; i < n; i += STK_BLOCK) {
            const unsigned lr = a.rows_per_group == 1 ? 0u : i / nchan;
            const unsigned chan = i - lr * nchan;
            const size_t r = r0 + lr;
            const size_t t = r * nchan + chan;
            const int bin = s_bin[lr];
            bool flagged = bin == -2;
            if (a.nflagcorr == 1) {
                flagged = flagged || __builtin_nontemporal_load(a.flag + t) != 0;
            } else if (a.nflagcorr) {
                unsigned f = 0;
                stk_load<NC, true>(a.flag + t * NC, &f);
                flagged = flagged || f != 0;
            }
            const bool live = !flagged && bin >= 0;
            cplx<T> v[NC];
            stk_load<NC * (int)sizeof(cplx<T>), true>(data + t * NC, v);
            if (data2) {
                cplx<T> d[NC];
                stk_load<NC * (int)sizeof(cplx<T>), true>(data2 + t * NC, d);
#pragma unroll
                for (int c = 0; c < NC; ++c) v[c] = a.subtract ? v[c] - d[c] : v[c] + d[c];
            }
            T w[NC];
            if (a.wform == PFB_STOKES_W_NONE) {
#pragma unroll
                for (int c = 0; c < NC; ++c) w[c] = T(1);
            } else if (a.wform == PFB_STOKES_W_ROW) {
                stk_load<NC * (int)sizeof(T), false>(weight + r * NC, w);
            } else {
                stk_load<NC * (int)sizeof(T), true>(weight + t * NC, w);
                if (a.wform == PFB_STOKES_W_SIGMA) {
#pragma unroll
                    for (int c = 0; c < NC; ++c) w[c] = T(1) / (w[c] * w[c]);
                }
            }
            cplx<T> gp[NJ], gq[NJ];
            if constexpr (stk_has_jones(MODE)) {
                const size_t tb = live ? (size_t)bin : 0, p = live ? (size_t)s_p[lr] : 0, q = live ? (size_t)s_q[lr] : 0;
                const size_t step = (size_t)a.ndir * NJ;
                stk_load<NJ * (int)sizeof(cplx<T>), false>(jones + ((tb * a.nant + p) * nchan + chan) * step, gp);
                stk_load<NJ * (int)sizeof(cplx<T>), false>(jones + ((tb * a.nant + q) * nchan + chan) * step, gq);
            }
            cplx<T> m[4], dpq;
            if constexpr (MODE == PFB_STOKES_FULL4) {
                m[0] = gp[3] * v[0] - gp[1] * v[2]; m[1] = gp[3] * v[1] - gp[1] * v[3];
                m[2] = gp[0] * v[2] - gp[2] * v[0]; m[3] = gp[0] * v[3] - gp[2] * v[1];
                dpq = mulc(gp[0] * gp[3] - gp[1] * gp[2], gq[0] * gq[3] - gq[1] * gq[2]);
            }
            cplx<T> ov[4];
            T ow[4];
            if (fam0) stk_eval_family<T, MODE, false>(v, w, gp, gq, m, dpq, ov[0], ov[1], ow[0], ow[1]);
            if (fam1) stk_eval_family<T, MODE, true>(v, w, gp, gq, m, dpq, ov[2], ov[3], ow[2], ow[3]);
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int k = ma.plane[b];
                if (k < 0) continue;
                const size_t o = (size_t)k * nvis + t;
                vis[o] = live ? ov[b] : cplx<T>(T(0), T(0));
                wgt[o] = live ? ow[b] : T(0);
                acc[b] += live ? (double)ow[b] : 0.0;
            }
            a.mask[t] = flagged ? 0 : 1;
        }
    }
    // the partials in the order of the planes
    double part[STK_MAX_PROD];
#pragma unroll
    for (int k = 0; k < STK_MAX_PROD; ++k) {
        const int b = ma.basis[k];
        part[k] = k >= ma.nprod ? 0.0 : b == 0 ? acc[0] : b == 1 ? acc[1] : b == 2 ? acc[2] : acc[3];
    }
    emit_partials<STK_MAX_PROD>(part, a.ws);
}

// -------------------------------------------------------------------------------------------- channel averaging
// DESIGN 4.16.  With n = chan_average, bin j of a row covers its channels [j n, min((j + 1) n, nchan)), nout =
// ceil(nchan / n) bins; per row, bin and product plane, over the bin's LIVE samples (mask != 0) in channel order:
//     wgt_out = sum wgt_i     vis_out = sum wgt_i vis_i / wgt_out, exactly 0 where wgt_out == 0     mask_out = any(mask_i)
// The samples that are not live are selected out, never multiplied by zero: what a masked sample holds is not read into a
// sum (an unflagged sample that no time bin covers has mask 1 and vis = wgt = 0, and adds its zeros).  A product
// wgt_i vis_i is formed in T and rounded on its own (no fused multiply-add, so that both kernels give the same bits);
// the sums run in fp64 in channel order -- an order that depends on the shapes only: the same bits every run -- and are
// rounded to T once, in front of the division.
//   k_chan_average        STK_AVG_LANE_MAX < n <= STK_BLOCK: the lanes take consecutive (row, channel) samples, as in k_stokes, so the loads
//                         are coalesced; they leave wgt vis, wgt and the mask byte in LDS -- 3 T per lane and plane, 24 KB
//                         for four fp64 planes -- and after one barrier the first lanes sum a bin each, divide and store.
//                         nchan <= STK_BLOCK / 2: a workgroup holds whole rows, so a bin never leaves it.  Else it
//                         strides over its one row in stretches of floor(STK_BLOCK / n) n channels, so that no bin
//                         straddles a stretch
//   k_chan_average_lane   any n: a lane per (row, bin), which walks its n channels.  Launched for n <= STK_AVG_LANE_MAX,
//                         where a lane's n samples fill whole 32-byte sectors and the barriers of the other kernel cost
//                         more than its coalescing gains (DESIGN 4.16 has the figures), and for n > STK_BLOCK

// the largest chan_average of the lane-per-bin kernel below STK_BLOCK (measured at 4 and 16 only)
constexpr int STK_AVG_LANE_MAX = 4;

__device__ __forceinline__ float stk_mul_rn(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ double stk_mul_rn(double a, double b) { return __dmul_rn(a, b); }

// the sums of a bin and what its lane does with them: round, divide, store, and the fp64 sum of wgt_out over
// mask_out != 0
template <typename T>
struct StkBinSum {
    double vx = 0.0, vy = 0.0, w = 0.0;
    // a live sample: its wgt vis (formed in T) and its wgt
    __device__ __forceinline__ void add(T wvx, T wvy, T wgt) { vx += (double)wvx; vy += (double)wvy; w += (double)wgt; }
    __device__ __forceinline__ void store(bool any_mask, cplx<T>* __restrict__ vis, T* __restrict__ wgt, size_t o,
                                          double& acc) const {
        const T sw = (T)w, sx = (T)vx, sy = (T)vy;
        vis[o] = sw == T(0) ? cplx<T>(T(0), T(0)) : cplx<T>(sx / sw, sy / sw);
        wgt[o] = sw;
        acc += any_mask ? (double)sw : 0.0;
    }
};

struct AvgArgs {
    const void* vis; const void* wgt; const u8* mask;
    size_t nrow, nbins, ngroups;       // nbins = nrow nout
    int nprod, nchan, nout, n, rows_per_group;
    void* viso; void* wgto; u8* masko;
    double* ws;
};

template <typename T>
__global__ void __launch_bounds__(STK_BLOCK)
k_chan_average(AvgArgs a) {
    __shared__ T s_vx[STK_MAX_PROD][STK_BLOCK], s_vy[STK_MAX_PROD][STK_BLOCK], s_w[STK_MAX_PROD][STK_BLOCK];
    __shared__ u8 s_m[STK_BLOCK];
    const cplx<T>* __restrict__ vis = static_cast<const cplx<T>*>(a.vis);
    const T* __restrict__ wgt = static_cast<const T*>(a.wgt);
    cplx<T>* __restrict__ viso = static_cast<cplx<T>*>(a.viso);
    T* __restrict__ wgto = static_cast<T*>(a.wgto);
    const unsigned nchan = (unsigned)a.nchan, navg = (unsigned)a.n, nout = (unsigned)a.nout;
    const size_t plane_in = a.nrow * (size_t)nchan;
    const bool one_row = a.rows_per_group == 1;
    // the channels a pass of the workgroup takes: whole rows, or whole bins of its one row
    const unsigned width = one_row ? STK_BLOCK / navg * navg : nchan;
    double acc[STK_MAX_PROD] = {0.0, 0.0, 0.0, 0.0};
    for (size_t g = blockIdx.x; g < a.ngroups; g += gridDim.x) {
        const size_t r0 = g * (size_t)a.rows_per_group;
        const unsigned nr = (unsigned)(a.nrow - r0 < (size_t)a.rows_per_group ? a.nrow - r0 : (size_t)a.rows_per_group);
        for (unsigned c0 = 0; c0 < nchan; c0 += width) {        // one pass unless one_row; uniform over the workgroup
            __syncthreads();                                    // the bins' readers of the pass before
            // the samples of this pass: nr whole rows, or channels [c0, c0 + len) of the one row
            const unsigned len = nchan - c0 < width ? nchan - c0 : width;
            const unsigned nin = one_row ? len : nr * nchan;    // <= STK_BLOCK
            if (threadIdx.x < nin) {
                const unsigned i = threadIdx.x;
                const unsigned lr = one_row ? 0u : i / nchan;
                const unsigned chan = one_row ? c0 + i : i - lr * nchan;
                const size_t t = (r0 + lr) * nchan + chan;
                const u8 m = a.mask[t];
                s_m[i] = m;
                if (m) {
#pragma unroll
                    for (int k = 0; k < STK_MAX_PROD; ++k) {
                        if (k >= a.nprod) break;
                        const T w = wgt[(size_t)k * plane_in + t];
                        const cplx<T> v = vis[(size_t)k * plane_in + t];
                        s_vx[k][i] = stk_mul_rn(w, v.x);
                        s_vy[k][i] = stk_mul_rn(w, v.y);
                        s_w[k][i] = w;
                    }
                }
            }
            __syncthreads();
            // the bins of this pass, a lane each: of nr rows (nout each), or the ceil(len / n) of the stretch
            const unsigned per_row = one_row ? (len + navg - 1) / navg : nout;
            const unsigned nb = one_row ? per_row : nr * nout;  // <= nin
            if (threadIdx.x < nb) {
                const unsigned lr = threadIdx.x / per_row, j = threadIdx.x - lr * per_row;
                const unsigned row_len = one_row ? len : nchan;
                const unsigned i0 = lr * row_len + j * navg;
                const unsigned i1 = lr * row_len + (row_len - j * navg < navg ? row_len : (j + 1) * navg);
                const size_t o = (r0 + lr) * nout + (one_row ? c0 / navg : 0u) + j;
                bool any_mask = false;
                for (unsigned i = i0; i < i1; ++i) any_mask = any_mask || s_m[i] != 0;
                a.masko[o] = any_mask ? 1 : 0;
#pragma unroll
                for (int k = 0; k < STK_MAX_PROD; ++k) {
                    if (k >= a.nprod) break;
                    StkBinSum<T> sum;
                    for (unsigned i = i0; i < i1; ++i) {
                        if (s_m[i]) sum.add(s_vx[k][i], s_vy[k][i], s_w[k][i]);
                    }
                    sum.store(any_mask, viso, wgto, (size_t)k * a.nbins + o, acc[k]);
                }
            }
        }
    }
    emit_partials<STK_MAX_PROD>(acc, a.ws);
}

template <typename T>
__global__ void __launch_bounds__(STK_BLOCK)
k_chan_average_lane(AvgArgs a) {
    const cplx<T>* __restrict__ vis = static_cast<const cplx<T>*>(a.vis);
    const T* __restrict__ wgt = static_cast<const T*>(a.wgt);
    cplx<T>* __restrict__ viso = static_cast<cplx<T>*>(a.viso);
    T* __restrict__ wgto = static_cast<T*>(a.wgto);
    const size_t nout = (size_t)a.nout, nchan = (size_t)a.nchan, n = (size_t)a.n;
    const size_t plane_in = a.nrow * nchan;
    double acc[STK_MAX_PROD] = {0.0, 0.0, 0.0, 0.0};
    for (size_t b = (size_t)blockIdx.x * STK_BLOCK + threadIdx.x; b < a.nbins; b += (size_t)gridDim.x * STK_BLOCK) {
        const size_t r = b / nout, j = b - r * nout;
        const size_t c0 = j * n, c1 = nchan - c0 < n ? nchan : c0 + n;
        const size_t t0 = r * nchan;
        bool any_mask = false;
        for (size_t c = c0; c < c1; ++c) any_mask = any_mask || a.mask[t0 + c] != 0;
        a.masko[b] = any_mask ? 1 : 0;
#pragma unroll
        for (int k = 0; k < STK_MAX_PROD; ++k) {
            if (k >= a.nprod) break;
            StkBinSum<T> sum;
            for (size_t c = c0; c < c1; ++c) {
                if (a.mask[t0 + c] == 0) continue;
                const size_t t = (size_t)k * plane_in + t0 + c;
                const T w = wgt[t];
                const cplx<T> v = vis[t];
                sum.add(stk_mul_rn(w, v.x), stk_mul_rn(w, v.y), w);
            }
            sum.store(any_mask, viso, wgto, (size_t)k * a.nbins + b, acc[k]);
        }
    }
    emit_partials<STK_MAX_PROD>(acc, a.ws);
}

// the checks and the kernel record that both entry points share; vis, wgt: plane 0 of the outputs
static int stk_setup(const char* name, int dtype, int mode, const void* data, const void* data2, int subtract,
                     const void* weight, int wform, const unsigned char* flag, int nflagcorr, const unsigned char* frow,
                     int autocorr, const void* jones, int ndir, int ntime, int nant, const long long* tbin_idx,
                     const long long* tbin_counts, long long tbin_off, const int* ant1, const int* ant2, size_t nrow,
                     int nchan, void* vis, void* wgt, unsigned char* mask, double* wsum, double* work, StkArgs& a) {
    PFB_REQUIRE(mode >= PFB_STOKES_DIAG4 && mode <= PFB_STOKES_NOJ2, PFB_ERR_INVALID, "%s: bad Jones mode %d", name, mode);
    PFB_REQUIRE(wform >= PFB_STOKES_W_NONE && wform <= PFB_STOKES_W_ROW, PFB_ERR_INVALID, "%s: bad weight form %d", name, wform);
    const size_t e = esize(dtype), nc = (size_t)stk_ncorr(mode), nj = (size_t)stk_njones(mode);
    // what one vector load reads: a visibility's correlations, its weights, an antenna's Jones terms; 16 bytes at most
    const auto vload = [](size_t n) { return bytes(n < 16 ? n : 16); };
    PFB_REQUIRE(nflagcorr == 0 || nflagcorr == 1 || nflagcorr == (int)nc, PFB_ERR_INVALID,
                "%s: %d flags per visibility of %zu correlations", name, nflagcorr, nc);
    if (int rc = check(dtype, name,
                       {{data, vload(2 * e * nc)}, {data2, vload(2 * e * nc), true},
                        {weight, vload(e * nc), wform == PFB_STOKES_W_NONE},
                        {flag, bytes(nflagcorr > 1 ? nc : 1), nflagcorr == 0}, {frow, U8, true},
                        {jones, vload(2 * e * nj), !stk_has_jones(mode)}, {tbin_idx, I64}, {tbin_counts, I64},
                        {ant1, I32}, {ant2, I32}, {vis, CPLX}, {wgt, REAL}, {mask, U8}, {wsum, F64}, {work, F64}});
        rc != PFB_OK) return rc;
    PFB_REQUIRE(nrow >= 1 && nchan >= 1 && nrow <= (size_t)0x7fffffff, PFB_ERR_UNSUPPORTED,
                "%s: %zu rows x %d channels outside [1, 2^31) each", name, nrow, nchan);
    PFB_REQUIRE(ntime >= 1 && nant >= 1 && ndir >= 1, PFB_ERR_INVALID, "%s: ntime %d, nant %d, ndir %d must be positive",
                name, ntime, nant, ndir);
    a.data = data; a.data2 = data2; a.weight = weight; a.jones = jones; a.flag = flag; a.frow = frow;
    a.ant1 = ant1; a.ant2 = ant2; a.tbin_idx = tbin_idx; a.tbin_counts = tbin_counts; a.tbin_off = tbin_off;
    a.nrow = nrow; a.nchan = nchan;
    a.rows_per_group = nchan >= STK_BLOCK ? 1 : STK_BLOCK / nchan;
    a.ngroups = (nrow + (size_t)a.rows_per_group - 1) / (size_t)a.rows_per_group;
    a.ntime = ntime; a.nant = nant; a.ndir = ndir; a.wform = wform; a.nflagcorr = nflagcorr; a.autocorr = autocorr != 0;
    a.subtract = subtract != 0;
    a.vis = vis; a.wgt = wgt; a.mask = mask; a.ws = work;
    return PFB_OK;
}

}  // namespace pfb

using namespace pfb;

extern "C" {

int pfb_stokes_vis(int dtype, int mode, int basis, const void* data, const void* data2, int subtract, const void* weight,
                   int wform, const unsigned char* flag, int nflagcorr, const unsigned char* frow, int autocorr,
                   const void* jones, int ndir, int ntime, int nant, const long long* tbin_idx,
                   const long long* tbin_counts, long long tbin_off, const int* ant1, const int* ant2, size_t nrow,
                   int nchan, void* vis, void* wgt, unsigned char* mask, double* wsum, double* work, void* stream) {
    PFB_REQUIRE(mode >= PFB_STOKES_DIAG4 && mode <= PFB_STOKES_NOJ2, PFB_ERR_INVALID, "stokes_vis: bad Jones mode %d", mode);
    PFB_REQUIRE(basis >= 0 && basis <= 3, PFB_ERR_INVALID, "stokes_vis: bad basis %d", basis);
    StkArgs a;
    if (int rc = stk_setup("stokes_vis", dtype, mode, data, data2, subtract, weight, wform, flag, nflagcorr, frow, autocorr,
                           jones, ndir, ntime, nant, tbin_idx, tbin_counts, tbin_off, ant1, ant2, nrow, nchan, vis, wgt,
                           mask, wsum, work, a);
        rc != PFB_OK) return rc;
    const size_t groups = a.ngroups < (size_t)STK_MAX_GROUPS ? a.ngroups : (size_t)STK_MAX_GROUPS;
    const int rc = by_type(dtype, [&](auto t) {
        return by_int<0, PFB_STOKES_NOJ2>(mode, [&](auto m) {
            return by_int<0, 3>(basis, [&](auto b) {
                return launch_groups(k_stokes<decltype(t), m(), b()>, groups, stream, a);
            });
        });
    });
    return rc != PFB_OK ? rc : final_sum(work, (int)groups, 1, wsum, stream);
}

int pfb_stokes_vis_multi(int dtype, int mode, int nprod, const int* basis, const void* data, const void* data2,
                         int subtract, const void* weight, int wform, const unsigned char* flag, int nflagcorr,
                         const unsigned char* frow, int autocorr, const void* jones, int ndir, int ntime, int nant,
                         const long long* tbin_idx, const long long* tbin_counts, long long tbin_off, const int* ant1,
                         const int* ant2, size_t nrow, int nchan, void* vis, void* wgt, unsigned char* mask, double* wsum,
                         double* work, void* stream) {
    PFB_REQUIRE(nprod >= 1 && nprod <= STK_MAX_PROD, PFB_ERR_INVALID, "stokes_vis_multi: %d products outside 1 .. %d",
                nprod, STK_MAX_PROD);
    PFB_REQUIRE(basis, PFB_ERR_INVALID, "stokes_vis_multi: null basis list");
    StkMultiArgs ma;
    for (int b = 0; b < 4; ++b) ma.plane[b] = -1;
    for (int k = 0; k < STK_MAX_PROD; ++k) ma.basis[k] = 0;
    for (int k = 0; k < nprod; ++k) {
        const int b = basis[k];                                 // a host array
        PFB_REQUIRE(b >= 0 && b <= 3, PFB_ERR_INVALID, "stokes_vis_multi: bad basis %d", b);
        PFB_REQUIRE(ma.plane[b] < 0, PFB_ERR_INVALID, "stokes_vis_multi: basis %d asked for twice", b);
        ma.plane[b] = k;
        ma.basis[k] = b;
    }
    ma.nprod = nprod;
    if (int rc = stk_setup("stokes_vis_multi", dtype, mode, data, data2, subtract, weight, wform, flag, nflagcorr, frow,
                           autocorr, jones, ndir, ntime, nant, tbin_idx, tbin_counts, tbin_off, ant1, ant2, nrow, nchan,
                           vis, wgt, mask, wsum, work, ma.s);
        rc != PFB_OK) return rc;
    const size_t groups = ma.s.ngroups < (size_t)STK_MULTI_MAX_GROUPS ? ma.s.ngroups : (size_t)STK_MULTI_MAX_GROUPS;
    const int rc = by_type(dtype, [&](auto t) {
        return by_int<0, PFB_STOKES_NOJ2>(mode, [&](auto m) {
            return launch_groups(k_stokes_multi<decltype(t), m()>, groups, stream, ma);
        });
    });
    return rc != PFB_OK ? rc : final_sum(work, (int)groups, nprod, wsum, stream);
}

int pfb_chan_average(int dtype, int nprod, const void* vis, const void* wgt, const unsigned char* mask, size_t nrow,
                     int nchan, int chan_average, void* viso, void* wgto, unsigned char* masko, double* wsum,
                     double* work, void* stream) {
    PFB_REQUIRE(nprod >= 1 && nprod <= STK_MAX_PROD, PFB_ERR_INVALID, "chan_average: %d products outside 1 .. %d", nprod,
                STK_MAX_PROD);
    PFB_REQUIRE(chan_average >= 1, PFB_ERR_INVALID, "chan_average: chan_average %d < 1", chan_average);
    if (int rc = check(dtype, "chan_average", {{vis, CPLX}, {wgt, REAL}, {mask, U8}, {viso, CPLX}, {wgto, REAL},
                                               {masko, U8}, {wsum, F64}, {work, F64}});
        rc != PFB_OK) return rc;
    PFB_REQUIRE(nrow >= 1 && nchan >= 1 && nrow <= (size_t)0x7fffffff, PFB_ERR_UNSUPPORTED,
                "chan_average: %zu rows x %d channels outside [1, 2^31) each", nrow, nchan);
    AvgArgs a;
    a.vis = vis; a.wgt = wgt; a.mask = mask; a.nrow = nrow; a.nprod = nprod; a.nchan = nchan; a.n = chan_average;
    a.nout = (int)(((long long)nchan + chan_average - 1) / chan_average);
    a.nbins = nrow * (size_t)a.nout;
    a.rows_per_group = nchan >= STK_BLOCK ? 1 : STK_BLOCK / nchan;
    a.ngroups = (nrow + (size_t)a.rows_per_group - 1) / (size_t)a.rows_per_group;
    a.viso = viso; a.wgto = wgto; a.masko = masko; a.ws = work;
    const bool lane = chan_average <= STK_AVG_LANE_MAX || chan_average > STK_BLOCK;
    const size_t need = lane ? (a.nbins + STK_BLOCK - 1) / STK_BLOCK : a.ngroups;
    const size_t groups = need < (size_t)STK_MULTI_MAX_GROUPS ? need : (size_t)STK_MULTI_MAX_GROUPS;
    const int rc = by_type(dtype, [&](auto t) {
        return lane ? launch_groups(k_chan_average_lane<decltype(t)>, groups, stream, a)
                    : launch_groups(k_chan_average<decltype(t)>, groups, stream, a);
    });
    return rc != PFB_OK ? rc : final_sum(work, (int)groups, nprod, wsum, stream);
}

}  // extern "C"
