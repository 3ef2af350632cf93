// imweight.hip -- the imaging weights of the grid worker (pfb/utils/weighting.py:43-171 and the l2reweight_dof block of
// pfb/operators/gridder.py:604-615), DESIGN 4.11:
//   k_counts        _compute_counts: the uv-cell counts.  k == 0: one add per unmasked visibility; k = 2 .. 16: a k x k
//                   footprint of phi(x / (k/2)) phi(y / (k/2)), phi(t) = exp(2.3 k (sqrt((1 - t)(1 + t)) - 1)).  k
//                   consecutive lanes per visibility: a lane owns one column of the footprint and adds down its k rows
//                   with float atomics, so that one atomic wave-instruction lands k contiguous reals per visibility
//                   (the shape of k_grid in wgrid.hip)
//   k_moments       sum c, sum c^2 and the number of non-zero cells of the counts, fp64, one pass: a partial per
//                   workgroup, then the one-workgroup sum of common.hpp into a 3-double device record (the two-stage
//                   form of cycle.hip: a fixed order, the same bits from run to run)
//   k_weights       _counts_to_weights: the lookup at (floor ug, floor vg) and uniform / Briggs weights, ssq formed on the
//                   device from the record
//   k_l2_residual   residual_vis = (vis - model_vis) * mask with sum |residual_vis|^2 and sum mask
//   k_l2_weights    the Student-t weights (dof + 1) / (dof + |r|^2 / ovar) / ovar [* imwgt] with their masked sum
//   k_wsum          sum wgt[mask != 0]
//   k_residual_weigh  the fastim chunk's three passes between its stages in one (stokes2im.py:268, 279-295, DESIGN
//                   4.15): vis = (vis - model_vis) * mask on the planes that have a model, wgt *= imwgt, sum wgt[mask != 0]
// The grid coordinate of a visibility is formed as the reference forms it -- freq / c, u * that, (. + umax) / u_cell, in
// fp64, every operation rounded on its own (no contraction) -- so that cell indices are the reference's bit for bit.
// u_cell and umax come from the host, which evaluates the reference's expressions in Python floats.
//
// A visibility whose cell (floor ug, floor vg) is outside [0, nx) x [0, ny), or whose coordinate is not finite, is
// dropped, and so is every footprint cell outside the grid: nothing addresses outside the arrays, whatever the input.
#include "entry.hpp"

namespace pfb {

constexpr int IMW_BLOCK = ENTRY_BLOCK;
constexpr int IMW_MAX_K = 16;

struct ImwGeom {
    int nx, ny;
    double u_cell, umax, v_cell, vmax;
};

// row r -> partial grid: bins of nrow / ngrid rows, the first nrow % ngrid of them one longer (weighting.py:64-67)
struct ImwBins {
    size_t base, rem;
    __device__ __forceinline__ size_t of(size_t r) const {
        const size_t cut = rem * (base + 1);
        return r < cut ? r / (base + 1) : rem + (r - cut) / base;        // base == 0: cut == nrow > r
    }
};

// (ug, vg) of visibility t = r * nchan + c; true iff its cell is inside the grid
__device__ __forceinline__ bool imw_coords(const double* __restrict__ uvw, const double* __restrict__ freq, size_t t,
                                           int nchan, const ImwGeom& g, double& ug, double& vg) {
#pragma clang fp contract(off)
    const size_t r = t / nchan;
    const double nf = freq[t - r * nchan] / C_LIGHT;
    const double ut = uvw[3 * r] * nf, vt = uvw[3 * r + 1] * nf;
    ug = (ut + g.umax) / g.u_cell;
    vg = (vt + g.vmax) / g.v_cell;
    return ug >= 0.0 && ug < (double)g.nx && vg >= 0.0 && vg < (double)g.ny;          // false for a NaN
}

// _es_kernel(t, 2.3, k), betak = 2.3 * k
__device__ __forceinline__ double imw_phi(double t, double betak) {
#pragma clang fp contract(off)
    const double q = (1.0 - t) * (1.0 + t);
    return exp(betak * ((q > 0.0 ? sqrt(q) : 0.0) - 1.0));
}

// --------------------------------------------------------------------------------------------------- the counts
template <typename T, int K>
__global__ void __launch_bounds__(IMW_BLOCK)
k_counts(const double* __restrict__ uvw, const double* __restrict__ freq, const u8* __restrict__ mask, size_t nvis,
         int nchan, ImwGeom g, ImwBins bins, T* __restrict__ counts) {
#pragma clang fp contract(off)
    constexpr int L = K ? K : 1;
    const size_t tid = (size_t)blockIdx.x * IMW_BLOCK + threadIdx.x;
    const size_t t = tid / L;
    if (t >= nvis || !mask[t]) return;
    double ug, vg;
    if (!imw_coords(uvw, freq, t, nchan, g, ug, vg)) return;
    T* __restrict__ grid = counts + bins.of(t / nchan) * ((size_t)g.nx * g.ny);
    if constexpr (K == 0) {
        atomic_add(grid + (size_t)floor(ug) * g.ny + (size_t)floor(vg), T(1));
    } else {
        constexpr int ko2 = K / 2;
        const double betak = 2.3 * K;
        const int u_idx = (int)rint(ug), v_idx = (int)rint(vg);        // round half to even, in [0, nx] x [0, ny]
        const int y_idx = v_idx + (int)(tid % L) - ko2;
        if (y_idx < 0 || y_idx >= g.ny) return;
        const double y = y_idx - vg + 0.5;
        const double fy = imw_phi(y / ko2, betak);
        T* __restrict__ cell = grid + y_idx;
#pragma unroll
        for (int i = -ko2; i < ko2; ++i) {
            const int x_idx = u_idx + i;
            if (x_idx < 0 || x_idx >= g.nx) continue;
            const double x = x_idx - ug + 0.5;
            atomic_add(cell + (size_t)x_idx * g.ny, (T)(imw_phi(x / ko2, betak) * fy));
        }
    }
}

// ------------------------------------------------------------------------------------- sums into a device record
// Every sum is two launches: the streaming kernel leaves one fp64 partial per workgroup and quantity in `ws`
// (emit_partials), k_final_sum adds them in a fixed order into the record.
// [sum c, sum c^2, number of c != 0]
template <typename T>
__global__ void __launch_bounds__(IMW_BLOCK)
k_moments(const T* __restrict__ counts, size_t n, double* __restrict__ ws) {
    double acc[3] = {0.0, 0.0, 0.0};
    for (size_t i = (size_t)blockIdx.x * IMW_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * IMW_BLOCK) {
        const double c = (double)counts[i];
        acc[0] += c;
        acc[1] += c * c;
        acc[2] += c != 0.0 ? 1.0 : 0.0;
    }
    emit_partials<3>(acc, ws);
}

// ---------------------------------------------------------------------------------------------------- the weights
// uniform (briggs == 0): 1 / c where c != 0, else 0.  Briggs: counts := 1 + counts * ssq BEFORE the lookup, as the
// reference has it, so an empty cell gives 1 / (1 + 0) = 1.  All-zero counts: zeros.  Outside the grid: 0
template <typename T>
__global__ void __launch_bounds__(IMW_BLOCK)
k_weights(const T* __restrict__ counts, const double* __restrict__ rec, const double* __restrict__ uvw,
          const double* __restrict__ freq, size_t nvis, int nchan, ImwGeom g, int briggs, double numsq,
          T* __restrict__ weights) {
#pragma clang fp contract(off)
    const size_t t = (size_t)blockIdx.x * IMW_BLOCK + threadIdx.x;
    if (t >= nvis) return;
    T out = T(0);
    double ug, vg;
    if (rec[2] != 0.0 && imw_coords(uvw, freq, t, nchan, g, ug, vg)) {
        const T c = counts[(size_t)floor(ug) * g.ny + (size_t)floor(vg)];
        if (briggs) {
            const T ssq = (T)(numsq / (rec[1] / rec[0]));
            const T d = T(1) + c * ssq;
            out = T(1) / d;
        } else if (c != T(0)) {
            out = T(1) / c;
        }
    }
    weights[t] = out;
}

// ------------------------------------------------------------------------------------------------- the l2 reweight
// [sum |residual_vis|^2, sum mask]
template <typename T>
__global__ void __launch_bounds__(IMW_BLOCK)
k_l2_residual(const cplx<T>* __restrict__ vis, const cplx<T>* __restrict__ model_vis, const u8* __restrict__ mask,
              size_t n, cplx<T>* __restrict__ res, double* __restrict__ ws) {
#pragma clang fp contract(off)
    double acc[2] = {0.0, 0.0};
    for (size_t i = (size_t)blockIdx.x * IMW_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * IMW_BLOCK) {
        const cplx<T> v = vis[i], m = model_vis[i];
        const T f = (T)mask[i];
        const T re = (v.x - m.x) * f, im = (v.y - m.y) * f;
        res[i] = cplx<T>(re, im);
        acc[0] += (double)re * (double)re + (double)im * (double)im;
        acc[1] += (double)mask[i];
    }
    emit_partials<2>(acc, ws);
}

// wgt = (dof + 1) / (dof + |r|^2 / ovar) / ovar [* imwgt], ovar = rec[0] / rec[1]; [sum wgt[mask != 0]]
template <typename T>
__global__ void __launch_bounds__(IMW_BLOCK)
k_l2_weights(const cplx<T>* __restrict__ res, const u8* __restrict__ mask, const T* __restrict__ imwgt, size_t n,
             double dof, const double* __restrict__ rec, T* __restrict__ wgt, double* __restrict__ ws) {
#pragma clang fp contract(off)
    const T ovar = (T)(rec[0] / rec[1]);
    const T d = (T)dof, d1 = (T)(dof + 1.0);
    double acc[1] = {0.0};
    for (size_t i = (size_t)blockIdx.x * IMW_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * IMW_BLOCK) {
        const cplx<T> r = res[i];
        const T rs = r.x * r.x + r.y * r.y;
        T w = d1 / (d + rs / ovar) / ovar;
        if (imwgt) w = w * imwgt[i];
        wgt[i] = w;
        if (mask[i]) acc[0] += (double)w;
    }
    emit_partials<1>(acc, ws);
}

template <typename T>
__global__ void __launch_bounds__(IMW_BLOCK)
k_wsum(const T* __restrict__ wgt, const u8* __restrict__ mask, size_t n, double* __restrict__ ws) {
    double acc[1] = {0.0};
    for (size_t i = (size_t)blockIdx.x * IMW_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * IMW_BLOCK)
        if (mask[i]) acc[0] += (double)wgt[i];
    emit_partials<1>(acc, ws);
}

// ------------------------------------------------------------------------------------------- the fastim chunk
// plane p of vis has model plane m[p], or none (m[p] < 0)
constexpr int IMW_RW_MAX_PROD = 4;
struct RwMap { int m[IMW_RW_MAX_PROD]; };

// NP planes of n visibilities, in place: vis[p] = (vis[p] - model_vis[m[p]]) * mask where m[p] >= 0, wgt[p] = (T)((double)
// wgt[p] * imwgt) where imwgt is given -- the product in fp64, rounded once --, and [sum wgt[p][mask != 0]], p < NP, of the
// weights as stored.  A lane loads one complex (8 or 16 bytes) per plane and element: a wave reads whole cache lines.
// mask and imwgt are read once for all planes.  m[] and the imwgt test are uniform: no lane diverges but on mask
template <typename T, int NP>
__global__ void __launch_bounds__(IMW_BLOCK)
k_residual_weigh(cplx<T>* __restrict__ vis, const cplx<T>* __restrict__ model_vis, RwMap map,
                 const u8* __restrict__ mask, const double* __restrict__ imwgt, size_t n, T* __restrict__ wgt,
                 double* __restrict__ ws) {
#pragma clang fp contract(off)
    double acc[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[p] = 0.0;
    for (size_t i = (size_t)blockIdx.x * IMW_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * IMW_BLOCK) {
        const u8 mk = mask[i];
        const T f = (T)mk;
        const double g = imwgt ? imwgt[i] : 1.0;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const size_t e = (size_t)p * n + i;
            if (map.m[p] >= 0) {
                const cplx<T> v = vis[e], m = model_vis[(size_t)map.m[p] * n + i];
                vis[e] = cplx<T>((v.x - m.x) * f, (v.y - m.y) * f);
            }
            T w = wgt[e];
            if (imwgt) {
                w = (T)((double)w * g);
                wgt[e] = w;
            }
            if (mk) acc[p] += (double)w;
        }
    }
    emit_partials<NP>(acc, ws);
}

// ------------------------------------------------------------------------------------------------------ launchers
// the streaming sums: at most IMW_MAX_GROUPS workgroups stride over the array
constexpr int IMW_MAX_GROUPS = PFB_IMW_WORK_DOUBLES / PFB_IMW_RECORD;
static inline size_t imw_stream_threads(size_t n) {
    const size_t cap = (size_t)IMW_MAX_GROUPS * IMW_BLOCK;
    return n < cap ? n : cap;
}
// k_residual_weigh leaves up to IMW_RW_MAX_PROD partials per workgroup in the same scratch
constexpr int IMW_RW_MAX_GROUPS = PFB_IMW_WORK_DOUBLES / IMW_RW_MAX_PROD;
static_assert(IMW_RW_MAX_PROD == PFB_IMW_MAX_PROD, "the header states the planes of pfb_imw_residual_weigh");
static int imw_geom(const char* name, int nx, int ny, double u_cell, double umax, double v_cell, double vmax, ImwGeom& g) {
    PFB_REQUIRE(nx >= 1 && ny >= 1 && (size_t)nx * (size_t)ny <= (size_t)0x7fffffff, PFB_ERR_UNSUPPORTED,
                "%s: grid %d x %d outside [1, 2^31) cells", name, nx, ny);
    PFB_REQUIRE(std::isfinite(u_cell) && std::isfinite(v_cell) && u_cell > 0 && v_cell > 0 && std::isfinite(umax) &&
                std::isfinite(vmax), PFB_ERR_INVALID, "%s: u_cell, v_cell must be positive and finite, umax, vmax finite", name);
    g.nx = nx; g.ny = ny; g.u_cell = u_cell; g.umax = umax; g.v_cell = v_cell; g.vmax = vmax;
    return PFB_OK;
}

}  // namespace pfb

using namespace pfb;

extern "C" {

int pfb_imw_counts(int dtype, const double* uvw, const double* freq, const unsigned char* mask, size_t nrow, int nchan,
                   int nx, int ny, double u_cell, double umax, double v_cell, double vmax, int k, int ngrid, void* counts,
                   void* stream) {
    if (int rc = check(dtype, "imw_counts", {{uvw, F64}, {freq, F64}, {mask, U8}, {counts, REAL}});
        rc != PFB_OK) return rc;
    if (int rc = check_nvis("imw_counts", nrow, nchan); rc != PFB_OK) return rc;
    ImwGeom g;
    if (int rc = imw_geom("imw_counts", nx, ny, u_cell, umax, v_cell, vmax, g); rc != PFB_OK) return rc;
    PFB_REQUIRE(k >= 0 && k <= IMW_MAX_K && k % 2 == 0, PFB_ERR_INVALID, "imw_counts: support %d not in {0, 2, .., %d}", k, IMW_MAX_K);
    PFB_REQUIRE(ngrid >= 1, PFB_ERR_INVALID, "imw_counts: %d grids", ngrid);
    PFB_REQUIRE((size_t)ngrid <= (size_t)0x7fffffff / ((size_t)nx * ny), PFB_ERR_UNSUPPORTED,
                "imw_counts: %d grids of %d x %d exceed 2^31 cells", ngrid, nx, ny);
    const size_t nvis = nrow * (size_t)nchan;
    PFB_HIP_CHECK(hipMemsetAsync(counts, 0, esize(dtype) * (size_t)ngrid * nx * ny, as_stream(stream)));
    const ImwBins bins{nrow / (size_t)ngrid, nrow % (size_t)ngrid};
    return by_type(dtype, [&](auto t) {
        return by_int<0, IMW_MAX_K, 2>(k, [&](auto kk) {
            return launch(k_counts<decltype(t), kk()>, nvis * (kk() ? kk() : 1), stream, uvw, freq, mask, nvis, nchan,
                          g, bins, counts);
        });
    });
}

int pfb_imw_moments(int dtype, const void* counts, size_t n, double* rec, double* work, void* stream) {
    if (int rc = check(dtype, "imw_moments", {{counts, REAL}, {rec, F64}, {work, F64}}); rc != PFB_OK)
        return rc;
    if (int rc = check_count("imw_moments", n, PFB_ERR_UNSUPPORTED); rc != PFB_OK) return rc;
    const unsigned groups = blocks(imw_stream_threads(n));
    const int rc = by_type(dtype, [&](auto t) {
        return launch_groups(k_moments<decltype(t)>, groups, stream, counts, n, work);
    });
    return rc != PFB_OK ? rc : final_sum(work, groups, 3, rec, stream);
}

int pfb_imw_weights(int dtype, const void* counts, const double* rec, const double* uvw, const double* freq, size_t nrow,
                    int nchan, int nx, int ny, double u_cell, double umax, double v_cell, double vmax, int briggs,
                    double numsqrt, void* weights, void* stream) {
    if (int rc = check(dtype, "imw_weights", {{counts, REAL}, {rec, F64}, {uvw, F64}, {freq, F64}, {weights, REAL}});
        rc != PFB_OK) return rc;
    if (int rc = check_nvis("imw_weights", nrow, nchan); rc != PFB_OK) return rc;
    ImwGeom g;
    if (int rc = imw_geom("imw_weights", nx, ny, u_cell, umax, v_cell, vmax, g); rc != PFB_OK) return rc;
    PFB_REQUIRE(!briggs || (std::isfinite(numsqrt) && numsqrt > 0), PFB_ERR_INVALID, "imw_weights: numsqrt must be positive and finite");
    const size_t nvis = nrow * (size_t)nchan;
    return by_type(dtype, [&](auto t) {
        return launch(k_weights<decltype(t)>, nvis, stream, counts, rec, uvw, freq, nvis, nchan, g, briggs,
                      numsqrt * numsqrt, weights);
    });
}

int pfb_imw_l2_residual(int dtype, const void* vis, const void* model_vis, const unsigned char* mask, size_t nvis,
                        void* residual_vis, double* rec, double* work, void* stream) {
    if (int rc = check(dtype, "imw_l2_residual", {{vis, CPLX}, {model_vis, CPLX}, {mask, U8},
                                                  {residual_vis, CPLX}, {rec, F64}, {work, F64}});
        rc != PFB_OK) return rc;
    if (int rc = check_count("imw_l2_residual", nvis, PFB_ERR_UNSUPPORTED); rc != PFB_OK) return rc;
    PFB_HIP_CHECK(hipMemsetAsync(rec, 0, PFB_IMW_RECORD * sizeof(double), as_stream(stream)));
    const unsigned groups = blocks(imw_stream_threads(nvis));
    const int rc = by_type(dtype, [&](auto t) {
        return launch_groups(k_l2_residual<decltype(t)>, groups, stream, vis, model_vis, mask, nvis,
                             residual_vis, work);
    });
    return rc != PFB_OK ? rc : final_sum(work, groups, 2, rec, stream);
}

int pfb_imw_l2_weights(int dtype, const void* residual_vis, const unsigned char* mask, const void* imwgt, size_t nvis,
                       double dof, double* rec, void* wgt, double* work, void* stream) {
    if (int rc = check(dtype, "imw_l2_weights", {{residual_vis, CPLX}, {mask, U8}, {imwgt, REAL, true},
                                                 {rec, F64}, {wgt, REAL}, {work, F64}});
        rc != PFB_OK) return rc;
    if (int rc = check_count("imw_l2_weights", nvis, PFB_ERR_UNSUPPORTED); rc != PFB_OK) return rc;
    PFB_REQUIRE(std::isfinite(dof), PFB_ERR_INVALID, "imw_l2_weights: dof must be finite");
    const unsigned groups = blocks(imw_stream_threads(nvis));
    const int rc = by_type(dtype, [&](auto t) {
        return launch_groups(k_l2_weights<decltype(t)>, groups, stream, residual_vis, mask, imwgt, nvis,
                             dof, rec, wgt, work);
    });
    return rc != PFB_OK ? rc : final_sum(work, groups, 1, rec + 2, stream);
}

int pfb_imw_wsum(int dtype, const void* wgt, const unsigned char* mask, size_t nvis, double* rec, double* work,
                 void* stream) {
    if (int rc = check(dtype, "imw_wsum", {{wgt, REAL}, {mask, U8}, {rec, F64}, {work, F64}});
        rc != PFB_OK) return rc;
    if (int rc = check_count("imw_wsum", nvis, PFB_ERR_UNSUPPORTED); rc != PFB_OK) return rc;
    const unsigned groups = blocks(imw_stream_threads(nvis));
    const int rc = by_type(dtype, [&](auto t) {
        return launch_groups(k_wsum<decltype(t)>, groups, stream, wgt, mask, nvis, work);
    });
    return rc != PFB_OK ? rc : final_sum(work, groups, 1, rec, stream);
}

int pfb_imw_residual_weigh(int dtype, int nprod, void* vis, const void* model_vis, int nmodel, const int* model_of,
                           const unsigned char* mask, const double* imwgt, size_t nvis, void* wgt, double* rec,
                           double* work, void* stream) {
    if (int rc = check(dtype, "imw_residual_weigh", {{vis, CPLX}, {model_vis, CPLX, true}, {mask, U8}, {imwgt, F64, true},
                                                     {wgt, REAL}, {rec, F64}, {work, F64}});
        rc != PFB_OK) return rc;
    PFB_REQUIRE(nprod >= 1 && nprod <= IMW_RW_MAX_PROD, PFB_ERR_INVALID, "imw_residual_weigh: %d planes outside 1 .. %d",
                nprod, IMW_RW_MAX_PROD);
    PFB_REQUIRE(model_of && nmodel >= 0 && nmodel <= IMW_RW_MAX_PROD && (nmodel == 0 || model_vis), PFB_ERR_INVALID,
                "imw_residual_weigh: %d model planes need a table and, above 0, model_vis; at most %d", nmodel,
                IMW_RW_MAX_PROD);
    RwMap map;
    for (int p = 0; p < IMW_RW_MAX_PROD; ++p) {
        map.m[p] = p < nprod && model_of[p] >= 0 ? model_of[p] : -1;
        PFB_REQUIRE(map.m[p] < nmodel, PFB_ERR_INVALID, "imw_residual_weigh: plane %d reads model plane %d of %d", p,
                    map.m[p], nmodel);
    }
    PFB_REQUIRE(nvis <= (size_t)0x7fffffff, PFB_ERR_UNSUPPORTED, "imw_residual_weigh: %zu elements outside [0, 2^31)", nvis);
    if (nvis == 0) {            // nothing to launch: the sums of no weights
        PFB_HIP_CHECK(hipMemsetAsync(rec, 0, (size_t)nprod * sizeof(double), as_stream(stream)));
        return PFB_OK;
    }
    const size_t cap = (size_t)IMW_RW_MAX_GROUPS * IMW_BLOCK;
    const unsigned groups = blocks(nvis < cap ? nvis : cap);
    const int rc = by_type(dtype, [&](auto t) {
        return by_int<1, IMW_RW_MAX_PROD>(nprod, [&](auto np) {
            return launch_groups(k_residual_weigh<decltype(t), np()>, groups, stream, vis, model_vis, map, mask, imwgt,
                                 nvis, wgt, work);
        });
    });
    return rc != PFB_OK ? rc : final_sum(work, groups, nprod, rec, stream);
}

}  // extern "C"
