// cgvec.hip -- fused CG vector kernels, deterministic fp64 reductions and the PCG driver.
//
// Replaces the ~12 numpy passes per iteration of pfb/opt/pcg.py:86-122 and the
// serial numba norm_diff (pfb/utils/misc.py:1316-1351) by three HBM-bound kernels:
//   k_pcg_init        r = A x0 - b ; y = M r ; p = -y           + <r,y>, any(y)
//   k_pcg_update      x' = x + a p ; r' = r + a Ap ; y' = M r'   + <r',y'>, |x'-x|^2, |x'|^2
//   k_pcg_dir         p = beta p - M r'                          + any(p)
//   k_pcg_update_dir  the last two in one pass (the sync-free driver; the two above: the exact backtracking loop)
// All inner products accumulate in fp64 (wave64 __shfl_down -> LDS -> one partial per
// workgroup -> single-workgroup final sum in a fixed order), scalars stay in device
// memory (alpha, beta are read by the kernels from there), the p.Ap product comes
// fused out of the convolution epilogue (fftconv*.hip) -- or, in the parametrised solve (pfb_pcg_solve_param), out of the
// second band mix of hessparam.hip: the two forms of the operator step PcgOp, the driver's whole view of A.
// The 16-byte packs (V16, Pack, ld / st and their non-temporal forms), can_vec, emit_partials and k_final_sum live in
// common.hpp, shared with the prox / primal-dual kernels of wavelet.hip; final_sum, k_final_sum's launch with its status,
// in entry.hpp.
#include "conv_plan.hpp"
#include "pcg_state.hpp"
#include "entry.hpp"
#include <chrono>
#include <unistd.h>
#include <cstring>
#include <cstdlib>
#include <utility>
#include <vector>

namespace pfb {

constexpr int RED_MAX_GRID = 1024;

static inline int red_grid(size_t nvec) {
    size_t g = (nvec + RED_BLOCK - 1) / RED_BLOCK;
    g = (g + 3) / 4;                      // >= 4 vectors per thread when large
    if (g < 1) g = 1;
    if (g > (size_t)RED_MAX_GRID) g = RED_MAX_GRID;   // 4 sums x grid <= PFB_REDUCE_WS_DOUBLES
    return (int)g;
}

template <typename T, int V>
__global__ void __launch_bounds__(RED_BLOCK)
k_dot(const T* __restrict__ a, const T* __restrict__ b, size_t nvec, double* __restrict__ ws) {
    double acc[1] = {0.0};
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
         i += (size_t)gridDim.x * blockDim.x) {
        Pack<T, V> pa = ld<T, V>(a, i), pb = ld<T, V>(b, i);
#pragma unroll
        for (int e = 0; e < V; ++e) acc[0] += (double)pa.e[e] * (double)pb.e[e];
    }
    emit_partials<1>(acc, ws);
}

template <typename T, int V>
__global__ void __launch_bounds__(RED_BLOCK)
k_norm_diff(const T* __restrict__ x, const T* __restrict__ xp, size_t nvec,
            double* __restrict__ ws) {
    double acc[2] = {0.0, 0.0};
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
         i += (size_t)gridDim.x * blockDim.x) {
        Pack<T, V> a = ld<T, V>(x, i), b = ld<T, V>(xp, i);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const double d = (double)a.e[e] - (double)b.e[e];
            acc[0] += d * d;
            acc[1] += (double)a.e[e] * (double)a.e[e];
        }
    }
    emit_partials<2>(acc, ws);
}

template <typename T, int V>
__global__ void __launch_bounds__(RED_BLOCK)
k_any(const T* __restrict__ a, size_t nvec, double* __restrict__ ws) {
    double acc[1] = {0.0};
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
         i += (size_t)gridDim.x * blockDim.x) {
        Pack<T, V> pa = ld<T, V>(a, i);
#pragma unroll
        for (int e = 0; e < V; ++e) acc[0] += (pa.e[e] != T(0)) ? 1.0 : 0.0;   // NaN counts, like np.any
    }
    emit_partials<1>(acc, ws);
}

template <typename T, int V>
__global__ void __launch_bounds__(RED_BLOCK)
k_axpby(T a, const T* __restrict__ x, T b, T* __restrict__ y, size_t nvec) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
         i += (size_t)gridDim.x * blockDim.x) {
        Pack<T, V> px = ld<T, V>(x, i), py = ld<T, V>(y, i);
#pragma unroll
        for (int e = 0; e < V; ++e) py.e[e] = a * px.e[e] + b * py.e[e];
        st<T, V>(y, i, py);
    }
}

// ------------------------------------------------------------------ the fused solver's kernels, by SYSTEM
// A system (pcg_state.hpp) is a contiguous run of bands solved as one PCG: the whole cube (pfb_pcg_solve, one system) or
// one band (pfb_pcg_solve_bands, a system per band).  System s has `nvs` vectors at offset s * nvs, its state block
// S + s * SB and `gps` workgroups of its own in the vector kernels (workgroup w works on system w / gps only), so every
// partial sum belongs to one system: ws[q * (nsys gps) + s * gps + g].  The bookkeeping kernels run one workgroup per
// system and sum that system's partials in a fixed order.

// M(r) = r / mdiv when mdiv > 0 (pcg.py:264-267: M = x / sigmainv), identity otherwise.
// r holds A(x0) on entry.  r = r - b ; y = M r ; p = -y ; sums per system: <r,y>, count(y != 0)
template <typename T, int V>
__global__ void __launch_bounds__(RED_BLOCK)
k_pcg_init(T* __restrict__ r, const T* __restrict__ b, T* __restrict__ p, T mdiv, size_t nvs, int gps,
           double* __restrict__ ws) {
    const int s = blockIdx.x / gps, g = blockIdx.x - s * gps;
    const size_t off = (size_t)s * nvs;
    double acc[2] = {0.0, 0.0};
    for (size_t i = (size_t)g * blockDim.x + threadIdx.x; i < nvs; i += (size_t)gps * blockDim.x) {
        Pack<T, V> pr = ld<T, V>(r, off + i), pb = ld<T, V>(b, off + i), pp;
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const T rr = pr.e[e] - pb.e[e];
            const T y = mdiv > T(0) ? rr / mdiv : rr;
            pr.e[e] = rr;
            pp.e[e] = -y;
            acc[0] += (double)rr * (double)y;
            acc[1] += (y != T(0)) ? 1.0 : 0.0;
        }
        st<T, V>(r, off + i, pr);
        st<T, V>(p, off + i, pp);
    }
    emit_partials<2>(acc, ws);
}

// one workgroup per system.  `sum`: S_RHON = <r,y>, S_NUM = count(y != 0) from k_pcg_init's partials (k_final_sum's
// order).  `place` (after the all-reduce of those two, when there is one): the rule's parameters and the start values;
// a system with a zero initial residual is marked S_ZERO + S_STOP, so that no later kernel touches it
__global__ void __launch_bounds__(RED_BLOCK)
k_init_state(const double* __restrict__ ws, int gps, double* __restrict__ S, double tol, double minit, double maxit,
             int sum, int place) {
    __shared__ double red[RED_BLOCK / 64];
    double* Sb = S + (size_t)blockIdx.x * SB;
    for (int q = 0; sum && q < 2; ++q) {
        const double* src = ws + ((size_t)q * gridDim.x + blockIdx.x) * gps;
        double acc[1] = {0.0};
        for (int g = threadIdx.x; g < gps; g += blockDim.x) acc[0] += src[g];
        block_sum<1>(acc, red);
        if (threadIdx.x == 0) Sb[S_RHON + q] = acc[0];
    }
    if (place && threadIdx.x == 0) {
        Sb[S_TOL] = tol; Sb[S_MINIT] = minit; Sb[S_MAXIT] = maxit;
        Sb[S_RHO] = Sb[S_RHON];
        Sb[S_ANY] = Sb[S_NUM];                 // count(y != 0) = count(p != 0) for p = -y
        Sb[S_EPS] = 1.0; Sb[S_EPSP] = 1.0;
        if (Sb[S_NUM] == 0.0) { Sb[S_ZERO] = 1.0; Sb[S_STOP] = 1.0; }
    }
}

// x' = x + a p ; r' = r + a Ap ; y' = M r' ; sums: <r',y'>, |x'-x|^2, |x'|^2
// alpha is read from device memory (fp64), rounded to T like the reference's scalar.
template <typename T, int V>
__global__ void __launch_bounds__(RED_BLOCK)
k_pcg_update(const T* __restrict__ x, const T* __restrict__ r, const T* __restrict__ p,
             const T* __restrict__ Ap, T* __restrict__ xn, T* __restrict__ rn,
             const double* __restrict__ alpha_dev, T mdiv, size_t nvec,
             double* __restrict__ ws) {
    // alpha_dev points at S[S_ALPHA]; once the solve is "dead" (all-zero direction,
    // pcg.py:106-107 detected one iteration late) the step is forced to 0: x' = x, r' = r
    const bool dead = alpha_dev[S_DEAD - S_ALPHA] != 0.0;
    const T alpha = dead ? T(0) : (T)alpha_dev[0];
    double acc[3] = {0.0, 0.0, 0.0};
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
         i += (size_t)gridDim.x * blockDim.x) {
        Pack<T, V> px = ld<T, V>(x, i), pr = ld<T, V>(r, i), pp = ld<T, V>(p, i),
                   pa = ld<T, V>(Ap, i), ox, orr;
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const T xnew = px.e[e] + alpha * pp.e[e];
            const T rnew = pr.e[e] + alpha * pa.e[e];
            const T y = mdiv > T(0) ? rnew / mdiv : rnew;
            ox.e[e] = xnew;
            orr.e[e] = rnew;
            const double d = (double)xnew - (double)px.e[e];
            acc[0] += (double)rnew * (double)y;
            acc[1] += d * d;
            acc[2] += (double)xnew * (double)xnew;
        }
        st<T, V>(xn, i, ox);
        st<T, V>(rn, i, orr);
    }
    emit_partials<3>(acc, ws);
}

// p = beta p - M r ; sums: count(p != 0)
template <typename T, int V>
__global__ void __launch_bounds__(RED_BLOCK)
k_pcg_dir(T* __restrict__ p, const T* __restrict__ r, const double* __restrict__ beta_dev,
          T mdiv, size_t nvec, double* __restrict__ ws) {
    double acc[1] = {0.0};
    if (beta_dev[S_DEAD - S_BETA] != 0.0) {        // dead: leave p (all zero) alone
        emit_partials<1>(acc, ws);
        return;
    }
    const T beta = (T)beta_dev[0];
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
         i += (size_t)gridDim.x * blockDim.x) {
        Pack<T, V> pp = ld<T, V>(p, i), pr = ld<T, V>(r, i);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const T y = mdiv > T(0) ? pr.e[e] / mdiv : pr.e[e];
            const T v = beta * pp.e[e] - y;
            pp.e[e] = v;
            acc[0] += (v != T(0)) ? 1.0 : 0.0;
        }
        st<T, V>(p, i, pp);
    }
    emit_partials<1>(acc, ws);
}

// update + direction in ONE pass (7 vector streams instead of 6 + 3): possible because the
// predictive line search already knows rnorm_next = rho(alpha) before the vectors are touched,
// so beta = rho(alpha)/rho is available up front (the reference forms beta from the recomputed
// <r',y'>; the two differ by rounding only -- the recomputed value is still what the NEXT
// iteration uses as rnorm).  x' = x + a p, r' = r + a Ap, p' = beta p - M r' with the system's own alpha / beta;
// sums per system: <r',y'>, |x'-x|^2, |x'|^2, count(p' != 0).  x' and r' go to xn and rn, which may be x and r
// themselves (hence no __restrict__ on the four): in place costs nothing where the vectors stream from HBM, but on
// vectors that live in the caches writing a line just read measured 10.1 instead of 8.9 us at 1024^2 fp32, so a solve
// whose work buffer has the room alternates between two copies.  A system that is not live changes nothing: in place it
// is skipped, with separate destinations its x and r are carried over.
// XNT: x is read and x' written non-temporally (x is not touched again until the next update, ~20 N bytes later)
// REV: walk each system from its END.  The inverse row kernel before this one finishes on the last band (its Ap, p, r
// rows are the freshest lines of the Infinity Cache) and the forward row kernel after it starts on the first band,
// whose p' this kernel then has written last: one band's worth of each stream is served from that cache at both
// boundaries instead of none.
template <typename T, int V, int U, bool XNT, bool REV>
__global__ void __launch_bounds__(RED_BLOCK)
k_pcg_update_dir(const T* x, const T* r, T* __restrict__ p, const T* __restrict__ Ap, T* xn, T* rn,
                 const double* __restrict__ S, T mdiv, size_t nvs, int gps, double* __restrict__ ws) {
    const int s = blockIdx.x / gps, g = blockIdx.x - s * gps;
    const double* Sb = S + (size_t)s * SB;
    { const size_t off = (size_t)s * nvs * V; x += off; r += off; p += off; Ap += off; xn += off; rn += off; }
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (sys_live(Sb)) {
        const T alpha = (T)Sb[S_ALPHA];
        const T beta = (T)Sb[S_BETA];
        const size_t stride = (size_t)gps * blockDim.x;
        for (size_t i0 = (size_t)g * blockDim.x + threadIdx.x; i0 < nvs; i0 += U * stride) {
            Pack<T, V> px[U], pr[U], pp[U], pa[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {          // all loads of the U strips in flight together
                const size_t ii = i0 + u * stride;
                const size_t i = REV ? nvs - 1 - ii : ii;
                if (ii < nvs) {
                    px[u] = XNT ? ld_nt<T, V>(x, i) : ld<T, V>(x, i);
                    pr[u] = ld<T, V>(r, i); pp[u] = ld<T, V>(p, i); pa[u] = ld<T, V>(Ap, i);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const size_t ii = i0 + u * stride;
                const size_t i = REV ? nvs - 1 - ii : ii;
                if (ii >= nvs) break;
                Pack<T, V> ox, orr;
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const T xnew = px[u].e[e] + alpha * pp[u].e[e];
                    const T rnew = pr[u].e[e] + alpha * pa[u].e[e];
                    const T y = mdiv > T(0) ? rnew / mdiv : rnew;
                    ox.e[e] = xnew;
                    orr.e[e] = rnew;
                    const double d = (double)xnew - (double)px[u].e[e];
                    acc[0] += (double)rnew * (double)y;
                    acc[1] += d * d;
                    acc[2] += (double)xnew * (double)xnew;
                    const T pn = beta * pp[u].e[e] - y;
                    pp[u].e[e] = pn;
                    acc[3] += (pn != T(0)) ? 1.0 : 0.0;
                }
                if constexpr (XNT) st_nt<T, V>(xn, i, ox); else st<T, V>(xn, i, ox);
                st<T, V>(rn, i, orr);
                st<T, V>(p, i, pp[u]);
            }
        }
    } else if (xn != x) {
        for (size_t i = (size_t)g * blockDim.x + threadIdx.x; i < nvs; i += (size_t)gps * blockDim.x) {
            st<T, V>(xn, i, ld<T, V>(x, i));
            st<T, V>(rn, i, ld<T, V>(r, i));
        }
    }
    emit_partials<4>(acc, ws);
}

// tiny scalar kernels of the exact backtracking loop
__global__ void k_set_alpha(double* S) { S[S_ALPHA] = S[S_RHO] / S[S_PAP]; S[S_NBT] = 0.0; }
__global__ void k_scale_alpha(double* S) { S[S_ALPHA] *= 0.75; }
__global__ void k_set_beta(double* S) { S[S_BETA] = S[S_RHON] / S[S_RHO]; }
__global__ void k_accept_rho(double* S) { S[S_RHO] = S[S_RHON]; }

// One launch per iteration, one workgroup per system, for every scalar the sync-free driver needs: the three fused
// dots of the convolution (`cp`: the system's `bs` per-workgroup partials of quantity q at q * qs + s * bst; null: none
// to sum), the four sums the previous iteration's fused update left in `ws` (when `have_upd`), then -- unless an
// all-reduce has to come first (`logic` == 0) -- the end of that iteration and the begin of this one.
// Seven independent sums, each by ONE wave in a fixed lane-strided order (deterministic): wave w takes conv quantity w
// (w < 3) and update quantity w (w < 4).
// Predictive backtracking (iter_begin_dev).  With M(r) = r/d linear, <r',M r'> along r' = r + a Ap is the
// quadratic  rho(a) = rho + (2 a <r,Ap> + a^2 <Ap,Ap>) / d,  so the reference's loop
// "while rnorm_next > rnorm: alpha *= 0.75" (pcg.py:96-101) is evaluated on three scalars
// instead of three more passes over the vectors; the accepted step is then applied ONCE and
// rnorm_next is recomputed from the actual r' exactly as the reference does.
__global__ void __launch_bounds__(256)
k_iter_sums(const double* __restrict__ cp, int bs, int qs, int bst, const double* __restrict__ ws, int gps,
            int have_upd, double* __restrict__ S, double mdiv, int predict, int logic) {
    __shared__ double vals[8];
    const int s = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (cp && w < 3) {
        const double* src = cp + (size_t)w * qs + (size_t)s * bst;
        double acc = 0.0;
        for (int k = lane; k < bs; k += 64) acc += src[k];
        acc = wave_sum(acc);
        if (lane == 0) vals[w] = acc;
    }
    if (have_upd && w < 4) {
        const double* src = ws + ((size_t)w * gridDim.x + s) * gps;
        double acc = 0.0;
        for (int g = lane; g < gps; g += 64) acc += src[g];
        acc = wave_sum(acc);
        if (lane == 0) vals[3 + w] = acc;
    }
    __syncthreads();
    double* Sb = S + (size_t)s * SB;
    if (threadIdx.x == 0 && sys_live(Sb)) {
        if (cp) { Sb[S_PAP] = vals[0]; Sb[S_RAP] = vals[1]; Sb[S_APAP] = vals[2]; }
        if (have_upd) { Sb[S_RHON] = vals[3]; Sb[S_NUM] = vals[4]; Sb[S_DEN] = vals[5]; Sb[S_ANY] = vals[6]; }
        if (logic) {
            if (have_upd) iter_end_dev(Sb);
            iter_begin_dev(Sb, mdiv, predict);
        }
    }
}
// the update's four sums (unless an all-reduce stood between: `ws` null) and the end of the iteration, past minit,
// where the host may look
__global__ void __launch_bounds__(256)
k_iter_end(const double* __restrict__ ws, int gps, double* __restrict__ S) {
    __shared__ double vals[4];
    const int s = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (ws) {
        const double* src = ws + ((size_t)w * gridDim.x + s) * gps;
        double acc = 0.0;
        for (int g = lane; g < gps; g += 64) acc += src[g];
        acc = wave_sum(acc);
        if (lane == 0) vals[w] = acc;
        __syncthreads();
    }
    double* Sb = S + (size_t)s * SB;
    if (threadIdx.x == 0 && sys_live(Sb)) {
        if (ws) { Sb[S_RHON] = vals[0]; Sb[S_NUM] = vals[1]; Sb[S_DEN] = vals[2]; Sb[S_ANY] = vals[3]; }
        iter_end_dev(Sb);
    }
}
// the all-reduce path (one system): what k_iter_sums left out, after the exchange
__global__ void k_iter_begin(double* S, double mdiv, int predict) { iter_begin_dev(S, mdiv, predict); }
__global__ void k_iter_end_begin(double* S, double mdiv, int predict) {
    iter_end_dev(S);
    iter_begin_dev(S, mdiv, predict);
}
// the direction a system's last iteration built has not been looked at yet
__global__ void k_final_check(double* S, int nsys) {
    for (int s = threadIdx.x; s < nsys; s += blockDim.x) {
        double* Sb = S + (size_t)s * SB;
        if (Sb[S_ZERO] == 0.0 && Sb[S_DEAD] == 0.0 && Sb[S_ANY] == 0.0) {
            Sb[S_DEAD] = 1.0; Sb[S_K] -= 1.0; Sb[S_EPS] = Sb[S_EPSP];
        }
    }
}

// ------------------------------------------------------------------ launch helpers
#define PFB_LAUNCH_VEC(T, kern, n, ptrs, ...)                                              \
    do {                                                                                   \
        if (can_vec<T>(n, ptrs)) {                                                         \
            const size_t nvec = (n) / V16<T>::N;                                           \
            const int G = red_grid(nvec);                                                  \
            G_used = G;                                                                    \
            hipLaunchKernelGGL((kern<T, V16<T>::N>), dim3(G), dim3(RED_BLOCK), 0, st,      \
                               __VA_ARGS__, nvec, ws);                                     \
        } else {                                                                           \
            const int G = red_grid(n);                                                     \
            G_used = G;                                                                    \
            hipLaunchKernelGGL((kern<T, 1>), dim3(G), dim3(RED_BLOCK), 0, st, __VA_ARGS__, \
                               (size_t)(n), ws);                                           \
        }                                                                                  \
    } while (0)

template <typename T>
static int dot_impl(const void* a, const void* b, size_t n, double* out, double* ws, hipStream_t st) {
    int G_used = 0;
    using PL = std::initializer_list<const void*>;
    PFB_LAUNCH_VEC(T, k_dot, n, (PL{a, b}), (const T*)a, (const T*)b);
    return final_sum(ws, G_used, 1, out, st);
}
template <typename T>
static int nd_impl(const void* x, const void* xp, size_t n, double* out, double* ws, hipStream_t st) {
    int G_used = 0;
    using PL = std::initializer_list<const void*>;
    PFB_LAUNCH_VEC(T, k_norm_diff, n, (PL{x, xp}), (const T*)x, (const T*)xp);
    return final_sum(ws, G_used, 2, out, st);
}
template <typename T>
static int any_impl(const void* a, size_t n, double* out, double* ws, hipStream_t st) {
    int G_used = 0;
    using PL = std::initializer_list<const void*>;
    PFB_LAUNCH_VEC(T, k_any, n, (PL{a}), (const T*)a);
    return final_sum(ws, G_used, 1, out, st);
}
template <typename T>
static int axpby_impl(double a, const void* x, double b, void* y, size_t n, hipStream_t st) {
    using PL = std::initializer_list<const void*>;
    if (can_vec<T>(n, PL{x, y})) {
        const size_t nvec = n / V16<T>::N;
        hipLaunchKernelGGL((k_axpby<T, V16<T>::N>), dim3(red_grid(nvec)), dim3(RED_BLOCK), 0, st,
                           (T)a, (const T*)x, (T)b, (T*)y, nvec);
    } else {
        hipLaunchKernelGGL((k_axpby<T, 1>), dim3(red_grid(n)), dim3(RED_BLOCK), 0, st,
                           (T)a, (const T*)x, (T)b, (T*)y, n);
    }
    PFB_HIP_CHECK(hipGetLastError());
    return PFB_OK;
}

// ------------------------------------------------------------------------ PCG driver
// The fused update streams 4 reads + 3 writes; measured on MI355X (tools/micro/hbm_stream.hip and
// the bench) that mix runs fastest with ONE 256-thread workgroup per CU -- few concurrent streams
// per HBM channel -- not with the chip oversubscribed: 256 workgroups 0.60 ms, 1024 0.78 ms at
// 8 x 4096^2 fp32.  Returns the grid (= number of partial sums per quantity).
static int stream_grid(size_t nvec) {
    const int ncu = device_cu_count();
    size_t g = (nvec + RED_BLOCK - 1) / RED_BLOCK;
    g = (g + 3) / 4;
    if (g < 1) g = 1;
    if (g > (size_t)ncu) g = ncu;
    return (int)g;
}
// workgroups per system of the fused update: the whole grid stays near one workgroup per CU, split evenly over the
// systems; of k_pcg_init: red_grid's rule.  nsys * gps <= max(nsys, RED_MAX_GRID) bounds the partials of both.
static int update_grid(size_t nvs, int nsys) {
    int g = stream_grid(nvs);
    const int share = stream_grid((size_t)1 << 40) / nsys;
    if (g > share) g = share;
    if (g > RED_MAX_GRID / nsys) g = RED_MAX_GRID / nsys;
    return g < 1 ? 1 : g;
}
static int init_grid(size_t nvs, int nsys) {
    int g = red_grid(nvs);
    if (g > RED_MAX_GRID / nsys) g = RED_MAX_GRID / nsys;
    return g < 1 ? 1 : g;
}

// The work buffer of a solve, stated once: the byte offset of every region (each starts on a 256-byte boundary) and the
// total, which is what the three pfb_pcg_*_work_bytes return.  NONE: the solve has no such region.
//   r, p, Ap    nb bands each
//   S           one state block per system
//   ws          4 sums x max(nsys, RED_MAX_GRID) partials of the vector kernels
//   xalt, ralt  `alternates` (the cube and the parametrised solve): second copies of x and r, nb bands each
//   tmp, mixp   `param`: the operator step's own scratch (MixWork: one cube, the second mix's partials)
struct PcgLayout {
    static constexpr size_t NONE = ~(size_t)0;
    size_t r, p, Ap, S, ws, xalt = NONE, ralt = NONE, tmp = NONE, mixp = NONE, total = 0;
    PcgLayout(const pfb_conv_plan* plan, int nb, int nsys, bool alternates, bool param) {
        auto take = [&](size_t bytes) { const size_t at = total; total += bytes; return at; };
        const size_t vb = vec_bytes(plan, nb);
        r = take(vb); p = take(vb); Ap = take(vb);
        S = take(((size_t)nsys * SB * sizeof(double) + 255) & ~(size_t)255);
        ws = take(sizeof(double) * 4 * (size_t)(nsys > RED_MAX_GRID ? nsys : RED_MAX_GRID));
        if (alternates) { xalt = take(vb); ralt = take(vb); }
        if (param) { const MixWork mw(plan); tmp = take(mw.total); mixp = tmp + mw.partials; }
    }
    template <typename U> U* at(void* work, size_t off) const { return off == NONE ? nullptr : (U*)((char*)work + off); }
};

// The exchange can lose a participant (include/pfb_hip.h, "Failure protocol"): with a hook the solver never waits for
// the device unboundedly -- it polls an event, probes the exchange (count = 0) and gives up after PFB_COMM_TIMEOUT_S
// seconds, aborting the exchange (count < 0) so that no rank stays blocked in a collective.  Without a hook every wait
// is a plain synchronise.
struct PcgSync {
    pfb_allreduce_fn allreduce;
    void* actx;
    hipStream_t st;
    hipEvent_t ev = nullptr;
    double comm_timeout = 600.0;
    ~PcgSync() { if (ev) (void)hipEventDestroy(ev); }
    int open() {
        if (!allreduce) return PFB_OK;
        set_error("%s", "");                   // comm_fail() quotes the hook's message: no stale text from an earlier call
        if (const char* e = getenv("PFB_COMM_TIMEOUT_S")) { const double v = atof(e); if (v > 0) comm_timeout = v; }
        PFB_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        return PFB_OK;
    }
    int comm_fail(const char* what) {
        char msg[384];
        snprintf(msg, sizeof(msg), "%s", pfb_last_error());      // the hook's own message, if it left one
        (void)allreduce(actx, nullptr, -1, (void*)st);            // abort: peers blocked in the collective are released
        set_error("pcg: %s%s%s -- exchange aborted, this rank's result is void", what, msg[0] ? ": " : "", msg);
        return PFB_ERR_COMM;
    }
    int reduce(double* buf, int count) {
        if (allreduce && allreduce(actx, buf, count, (void*)st) != 0) return comm_fail("the all-reduce hook failed");
        return PFB_OK;
    }
    int wait_event(hipEvent_t e) {
        if (!allreduce) { PFB_HIP_CHECK(hipEventSynchronize(e)); return PFB_OK; }
        const auto t0 = std::chrono::steady_clock::now();
        for (long spins = 0;; ++spins) {
            const hipError_t q = hipEventQuery(e);
            if (q == hipSuccess) return PFB_OK;
            if (q != hipErrorNotReady) { set_error("pcg: hipEventQuery -> %s", hipGetErrorString(q)); return PFB_ERR_HIP; }
            if (spins < 4096) continue;                           // a look normally returns within tens of microseconds
            if (allreduce(actx, nullptr, 0, (void*)st) != 0) return comm_fail("the exchange reported a failure");
            const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (el > comm_timeout) {
                char what[128];
                snprintf(what, sizeof(what), "no progress on the solver's stream for %.0f s (PFB_COMM_TIMEOUT_S)", el);
                set_error("%s", "");
                return comm_fail(what);
            }
            usleep(el < 0.01 ? 20 : 500);
        }
    }
    int wait_stream() {
        if (!allreduce) { PFB_HIP_CHECK(hipStreamSynchronize(st)); return PFB_OK; }
        PFB_HIP_CHECK(hipEventRecord(ev, st));
        return wait_event(ev);
    }
    int fetch(double* h, const double* S, size_t count) {
        PFB_HIP_CHECK(hipMemcpyAsync(h, S, sizeof(double) * count, hipMemcpyDeviceToHost, st));
        return wait_stream();
    }
};

// What an entry point asks for: bands [band0, band0 + nb) as one system (the cube: inner products over all bands) or,
// `per_band`, every band its own; L, LH non-null: the parametrised solve (`beam` is then e).
struct PcgSolve {
    pfb_conv_plan* plan;
    int band0, nb;
    bool per_band;
    const void* b; void* x; void* r_out; const void* beam;
    double wsum, sigmainv, mdiv, tol;
    int maxit, minit, backtrack;
    size_t lookahead_max;      // elements up to which the host looks one iteration late
    void* work;
    pfb_allreduce_fn allreduce; void* actx;
    const void *L, *LH;
    pfb_pcg_result* res;
    hipStream_t st;
};

// The operator step: the driver's whole view of A, one operation per place it applies A.  Two forms: the convolution
// of the solve's bands (Lm null), or mix -> convolution -> mix over all the plan's bands as one system (hessparam.hip),
// whose three dots come out of the second mix into mixp.
template <typename T>
struct PcgOp {
    pfb_conv_plan* plan;
    int band0, nb, bps;        // the solve's bands [band0, band0 + nb); bands per system
    size_t ns;                 // elements per system
    bool per_band;
    const T* beam;
    double wsum, sigmainv;
    const T *Lm, *LHm;
    T* tmp;
    double* mixp;
    hipStream_t st;
    // where apply_partials left system s's partials: k_iter_sums' (cp, bs, qs, bst)
    struct Partials { const double* cp; int bs, qs, bst; };

    int mix(const T* v, T* out, const T* rr, double* partials, int* G) const {
        return hessparam_apply_partials(plan, Lm, LHm, beam, sigmainv, v, out, rr, tmp, partials, G, st);
    }
    // r = A x0 over all systems, no sums
    int apply(const T* x0, T* r) const {
        return Lm ? mix(x0, r, nullptr, nullptr, nullptr)
                  : pfb_psfconv_apply(plan, band0, nb, x0, beam, wsum, sigmainv, r, nullptr, nullptr, (void*)st);
    }
    // Ap = A p on the systems [lo, lo + nl), with <p,Ap>, <rc,Ap>, <Ap,Ap> left as per-workgroup partials at *w
    int apply_partials(const T* p, T* Ap, const T* rc, int lo, int nl, Partials* w) const {
        if (Lm) {
            int G = 0;
            const int err = mix(p, Ap, rc, mixp, &G);
            *w = {mixp, G, G, 0};
            return err;
        }
        const size_t off = (size_t)lo * ns;
        w->cp = plan->partials;
        return psfconv_apply_partials(plan, band0 + lo * bps, nl * bps, p + off, beam ? beam + off : nullptr, wsum,
                                      sigmainv, Ap + off, p + off, rc + off, per_band, &w->bs, &w->qs, &w->bst, (void*)st);
    }
    // Ap = A p over all systems, <p,Ap> summed into *pap (device)
    int apply_dot(const T* p, T* Ap, double* pap) const {
        if (!Lm) return pfb_psfconv_apply(plan, band0, nb, p, beam, wsum, sigmainv, Ap, p, pap, (void*)st);
        int G = 0;
        const int err = mix(p, Ap, nullptr, mixp, &G);
        if (err == PFB_OK)
            hipLaunchKernelGGL(k_final_sum<RED_BLOCK>, dim3(1), dim3(RED_BLOCK), 0, st, (const double*)mixp, G, 1, pap);
        return err;
    }
};

// One solve.  init(), then run() or run_exact(), then report().
template <typename T>
struct Pcg {
    pfb_conv_plan* plan;
    int nb;
    const T* b; T* x; T* r_out;
    double mdiv_d, tol;
    int maxit, minit;
    PcgSync sync;
    hipStream_t st;
    int nsys;
    size_t n, ns, nvs;         // elements of the solve and of a system; vectors of a system
    bool vec;                  // every system starts on a 16-byte boundary and is a whole number of them
    T *r, *p, *Ap, *xalt, *ralt;
    double *S, *ws;
    T mdiv;
    std::vector<double> h;     // the host's copy of the state blocks
    PcgOp<T> A;

    explicit Pcg(const PcgSolve& q)
        : plan(q.plan), nb(q.nb), b((const T*)q.b), x((T*)q.x), r_out((T*)q.r_out), mdiv_d(q.mdiv), tol(q.tol),
          maxit(q.maxit), minit(q.minit), sync{q.allreduce, q.actx, q.st}, st(q.st), nsys(q.per_band ? q.nb : 1),
          mdiv((T)q.mdiv), h((size_t)nsys * SB) {
        n = (size_t)nb * plan->nx * plan->ny;
        ns = n / nsys;
        // alternates of x and r: not in the per-band solve's work buffer, where x and r are updated in place
        const PcgLayout lay(plan, nb, nsys, !q.per_band, q.L != nullptr);
        r = lay.at<T>(q.work, lay.r); p = lay.at<T>(q.work, lay.p); Ap = lay.at<T>(q.work, lay.Ap);
        S = lay.at<double>(q.work, lay.S); ws = lay.at<double>(q.work, lay.ws);
        xalt = lay.at<T>(q.work, lay.xalt); ralt = lay.at<T>(q.work, lay.ralt);
        A = {plan, q.band0, nb, nb / nsys, ns, q.per_band, (const T*)q.beam, q.wsum, q.sigmainv, (const T*)q.L,
             (const T*)q.LH, lay.at<T>(q.work, lay.tmp), lay.at<double>(q.work, lay.mixp), st};
        using PL = std::initializer_list<const void*>;
        // decided once for every vector kernel of the solve (r, p, Ap and the alternates are 256-byte aligned parts of
        // `work`).  A caller whose x or b is not 16-byte aligned gets the scalar kernels throughout, init included
        vec = can_vec<T>(ns, PL{x, b, r, p, Ap});
        nvs = vec ? ns / V16<T>::N : ns;
    }

    // r = A(x0) - b ; y = M r ; p = -y ; the state blocks, on the device and in h          pcg.py:71-76
    int init() {
        int err;
        if ((err = sync.open()) != PFB_OK) return err;
        PFB_HIP_CHECK(hipMemsetAsync(S, 0, sizeof(double) * h.size(), st));
        if ((err = A.apply(x, r)) != PFB_OK) return err;
        const int gps = init_grid(nvs, nsys);
        if (vec)
            hipLaunchKernelGGL((k_pcg_init<T, V16<T>::N>), dim3(nsys * gps), dim3(RED_BLOCK), 0, st, r, b, p, mdiv, nvs,
                               gps, ws);
        else
            hipLaunchKernelGGL((k_pcg_init<T, 1>), dim3(nsys * gps), dim3(RED_BLOCK), 0, st, r, b, p, mdiv, nvs, gps, ws);
        // S_RHON = <r,y>, S_NUM = count(y != 0): moved into place after the hook
        const int hook = sync.allreduce ? 1 : 0;
        hipLaunchKernelGGL(k_init_state, dim3(nsys), dim3(RED_BLOCK), 0, st, (const double*)ws, gps, S, tol,
                           (double)minit, (double)maxit, 1, 1 - hook);
        if (hook) {
            if ((err = sync.reduce(S + S_RHON, 2)) != PFB_OK) return err;
            hipLaunchKernelGGL(k_init_state, dim3(nsys), dim3(RED_BLOCK), 0, st, (const double*)ws, gps, S, tol,
                               (double)minit, (double)maxit, 0, 1);
        }
        PFB_HIP_CHECK(hipGetLastError());
        return sync.fetch(h.data(), S, h.size());
    }

    // Sync-free driver (backtrack off or predictive).  Everything an iteration needs to decide lives in the state
    // blocks on the device; the host only has to look when the stopping rule `(eps > tol or k < minit) and k < maxit`
    // can actually fire, i.e. never while k < minit, and then only at whether any system is still live.  Two reduction
    // points per iteration:  [p.Ap, r.Ap, Ap.Ap, any(p)]  and  [r'.y', |x'-x|^2, |x'|^2]
    // -- with sharded bands one all-reduce each, merged into ONE per iteration while k < minit.
    int run(int predict, size_t lookahead_max) {
        const size_t nS = h.size();
        const bool hook = sync.allreduce != nullptr;
        auto any_live = [&](const double* hs) {
            for (int s = 0; s < nsys; ++s) if (sys_live(hs + (size_t)s * SB)) return true;
            return false;
        };
        int err;
        // Past minit the stopping rule needs eps after every iteration.  Looking costs a copy + stream sync
        // (13-24 us, tools/exp_sync_cost.py): a third of an iteration at 1024^2, 1 % at 8 x 4096^2.  Small
        // problems therefore run ONE iteration ahead: iteration j is enqueued, then the pinned snapshot taken
        // after iteration j-1 is read; every system evaluates the rule itself (S_STOP) so that the speculative
        // iteration is a no-op once it fired.  Price: one wasted iteration per solve -- large problems keep
        // the synchronous look.  PFB_PCG_LOOKAHEAD=0/1 overrides the size rule.
        bool lookahead = n <= lookahead_max;
        if (const char* la = getenv("PFB_PCG_LOOKAHEAD")) lookahead = atoi(la) != 0;
        if (lookahead && plan->pcg_pin_n < nsys) {     // two snapshots of the state blocks, grown on demand
            if (plan->pcg_pin) { PFB_HIP_CHECK(hipStreamSynchronize(st)); (void)hipHostFree(plan->pcg_pin); }
            plan->pcg_pin = nullptr;
            plan->pcg_pin_n = 0;
            PFB_HIP_CHECK(hipHostMalloc((void**)&plan->pcg_pin, sizeof(double) * 2 * nS, hipHostMallocDefault));
            plan->pcg_pin_n = nsys;
            for (int e = 0; e < 2; ++e)
                if (!plan->pcg_ev[e]) PFB_HIP_CHECK(hipEventCreateWithFlags(&plan->pcg_ev[e], hipEventDisableTiming));
        }
        // x non-temporal (and the walk from the end) only when the vectors are far beyond the caches anyway (>= 32 MB
        // each): small problems live in L2 / the Infinity Cache between iterations and nt would send x to HBM
        // (1024^2: 0.060 -> 0.066 ms per iteration)
        const bool xnt = vec && n * sizeof(T) >= ((size_t)32 << 20);
        const double* seen = h.data();             // the newest state the host has looked at
        bool go = (1.0 > tol || 0 < minit) && 0 < maxit && any_live(seen);
        int khost = 0, slot = 0;
        bool pending_end = false, have_prev = false;
        // the span [lo, lo + nl) of systems that may still be live: narrowed at every host look, so that bands which
        // have stopped at either end are no longer convolved (a stopped band between two live ones still is)
        int lo = 0, nl = nsys, gpl = update_grid(nvs, nsys);
        // the iterate, and where the next update writes it (k_pcg_update_dir): the alternates, or in place
        T *xc = x, *rc = r, *xn = xalt ? xalt : x, *rn = ralt ? ralt : r;
        auto narrow = [&](const double* hs) {
            int a = 0, z = nsys;
            while (a < z && !sys_live(hs + (size_t)a * SB)) ++a;
            while (z > a && !sys_live(hs + (size_t)(z - 1) * SB)) --z;
            if (z > a && (a != lo || z - a != nl)) { lo = a; nl = z - a; gpl = update_grid(nvs, nl); }
        };
        while (go) {
            const size_t off = (size_t)lo * ns;
            double* Sl = S + (size_t)lo * SB;
            typename PcgOp<T>::Partials c;
            if ((err = A.apply_partials(p, Ap, rc, lo, nl, &c)) != PFB_OK) return err;
            // ONE scalar launch per iteration: the convolution's dots, the previous update's sums
            // (left pending while nobody can look at k / eps, i.e. while k < minit) and the
            // bookkeeping; with sharded bands the all-reduce of those 7 (or 4) scalars sits between
            // the sums and the bookkeeping -- one RCCL call per iteration instead of two.
            hipLaunchKernelGGL(k_iter_sums, dim3(nl), dim3(256), 0, st, c.cp, c.bs, c.qs, c.bst,
                               (const double*)ws, gpl, pending_end ? 1 : 0, Sl, mdiv_d, predict, hook ? 0 : 1);
            // Behind a stop (the look-ahead's one speculative iteration) k_iter_sums writes nothing, so these exchanges
            // sum S_PAP .. S_ANY over the ranks a second time.  Every rank stops on the same reduced scalars, so all
            // still take part; nothing reads S_PAP .. S_DEN of a stopped system again, and S_ANY, which k_final_check
            // compares with zero, is a sum of counts >= 0: zero stays zero, non-zero stays non-zero.
            if (hook) {
                if ((err = sync.reduce(Sl + S_PAP, pending_end ? 7 : 4)) != PFB_OK) return err;
                if (pending_end) hipLaunchKernelGGL(k_iter_end_begin, dim3(1), dim3(1), 0, st, Sl, mdiv_d, predict);
                else hipLaunchKernelGGL(k_iter_begin, dim3(1), dim3(1), 0, st, Sl, mdiv_d, predict);
            }
            pending_end = false;
            // two strips per trip (all eight loads in flight before the first use): fp64 0.79 -> 0.71 ms at
            // 4 x 4096^2, fp32 0.64 -> 0.62 ms at 8 x 4096^2 (rocprofv3)
#define PFB_UPDATE(VV, XN)                                                                                     \
            hipLaunchKernelGGL((k_pcg_update_dir<T, VV, 2, XN, XN>), dim3(nl * gpl), dim3(RED_BLOCK), 0, st,   \
                               (const T*)xc + off, (const T*)rc + off, p + off, (const T*)Ap + off, xn + off,    \
                               rn + off, (const double*)Sl, mdiv, nvs, gpl, ws)
            if (xnt) PFB_UPDATE(V16<T>::N, true);
            else if (vec) PFB_UPDATE(V16<T>::N, false);
            else PFB_UPDATE(1, false);
#undef PFB_UPDATE
            std::swap(xc, xn);
            std::swap(rc, rn);
            if (khost + 1 < minit && khost + 1 < maxit) {
                pending_end = true;        // summed by the next iteration's k_iter_sums (no look, so no narrowing, between)
            } else {
                if (hook) {
                    hipLaunchKernelGGL(k_iter_sums, dim3(nl), dim3(256), 0, st, (const double*)nullptr, 0, 0, 0,
                                       (const double*)ws, gpl, 1, Sl, mdiv_d, predict, 0);
                    if ((err = sync.reduce(Sl + S_RHON, 3)) != PFB_OK) return err;
                }
                hipLaunchKernelGGL(k_iter_end, dim3(nl), dim3(256), 0, st, hook ? nullptr : (const double*)ws, gpl, Sl);
            }
            PFB_HIP_CHECK(hipGetLastError());
            ++khost;
            if (khost < minit && khost < maxit) continue;          // no system can stop yet: no need to look
            if (lookahead && khost < maxit) {
                double* snap = plan->pcg_pin + (size_t)slot * nS;
                PFB_HIP_CHECK(hipMemcpyAsync(snap, S, sizeof(double) * nS, hipMemcpyDeviceToHost, st));
                PFB_HIP_CHECK(hipEventRecord(plan->pcg_ev[slot], st));
                if (have_prev) {
                    if ((err = sync.wait_event(plan->pcg_ev[slot ^ 1])) != PFB_OK) return err;
                    seen = plan->pcg_pin + (size_t)(slot ^ 1) * nS;
                    go = any_live(seen);       // if not, the iteration just enqueued changes nothing
                    if (go) narrow(seen);      // an older snapshot: a system stopped there is stopped now as well
                }
                have_prev = true;
                slot ^= 1;
                continue;
            }
            if ((err = sync.fetch(h.data(), S, nS)) != PFB_OK) return err;
            seen = h.data();
            go = khost < maxit && any_live(seen);
            if (go) narrow(seen);
        }
        // the direction a system's last iteration built has not been looked at yet (a system seen dead has none)
        bool check = false;
        for (int s = 0; s < nsys; ++s) check |= seen[(size_t)s * SB + S_DEAD] == 0.0 && seen[(size_t)s * SB + S_ZERO] == 0.0;
        if (check) {
            if ((err = sync.reduce(S + S_ANY, 1)) != PFB_OK) return err;
            hipLaunchKernelGGL(k_final_check, dim3(1), dim3(64), 0, st, S, nsys);
            PFB_HIP_CHECK(hipGetLastError());
        }
        if (xc != x) PFB_HIP_CHECK(hipMemcpyAsync(x, xc, n * sizeof(T), hipMemcpyDeviceToDevice, st));
        if (r_out) PFB_HIP_CHECK(hipMemcpyAsync(r_out, rc, n * sizeof(T), hipMemcpyDeviceToDevice, st));
        return sync.fetch(h.data(), S, nS);
    }

    // Exact backtracking: the reference's loop verbatim, driven from the host (one system; it needs the old x and r:
    // the iterate lives alternately in x / xalt, r / ralt).  Leaves its outcome in h for report().
    int run_exact() {
        using PL = std::initializer_list<const void*>;
        T *xcur = x, *rcur = r, *xnew = xalt, *rnew = ralt;
        int err, G_used = 0, k = 0, nbt = 0;
        double eps = 1.0, rho = h[S_RHO];
        bool broke = false;
        while (h[S_ZERO] == 0.0 && (eps > tol || k < minit) && k < maxit) {
            // Ap = A(p); S_PAP = <p,Ap>                                                     pcg.py:89-91
            if ((err = A.apply_dot(p, Ap, S + S_PAP)) != PFB_OK) return err;
            if ((err = sync.reduce(S + S_PAP, 1)) != PFB_OK) return err;
            hipLaunchKernelGGL(k_set_alpha, dim3(1), dim3(1), 0, st, S);
            for (;;) {
                PFB_LAUNCH_VEC(T, k_pcg_update, n, (PL{xcur, rcur, p, Ap, xnew, rnew}), (const T*)xcur,
                               (const T*)rcur, (const T*)p, (const T*)Ap, xnew, rnew,
                               (const double*)(S + S_ALPHA), mdiv);
                hipLaunchKernelGGL(k_final_sum<RED_BLOCK>, dim3(1), dim3(RED_BLOCK), 0, st, ws, G_used, 3, S + S_RHON);
                if ((err = sync.reduce(S + S_RHON, 3)) != PFB_OK) return err;
                if ((err = sync.fetch(h.data(), S, S_NSCALAR)) != PFB_OK) return err;
                if (!(h[S_RHON] > rho)) break;          // pcg.py:96-101
                hipLaunchKernelGGL(k_scale_alpha, dim3(1), dim3(1), 0, st, S);
                ++nbt;
            }
            // accept x', r'
            { T* t = xcur; xcur = xnew; xnew = t; t = rcur; rcur = rnew; rnew = t; }
            // beta = rnorm_next / rnorm ; p = beta p - y      pcg.py:103-107
            hipLaunchKernelGGL(k_set_beta, dim3(1), dim3(1), 0, st, S);
            PFB_LAUNCH_VEC(T, k_pcg_dir, n, (PL{p, rcur}), p, (const T*)rcur, (const double*)(S + S_BETA), mdiv);
            hipLaunchKernelGGL(k_final_sum<RED_BLOCK>, dim3(1), dim3(RED_BLOCK), 0, st, ws, G_used, 1, S + S_ANY);
            if ((err = sync.reduce(S + S_ANY, 1)) != PFB_OK) return err;
            hipLaunchKernelGGL(k_accept_rho, dim3(1), dim3(1), 0, st, S);
            rho = h[S_RHON];
            const double num = h[S_NUM], den = h[S_DEN];
            if ((err = sync.fetch(h.data(), S, S_NSCALAR)) != PFB_OK) return err;
            if (h[S_ANY] == 0.0) { broke = true; break; }    // break BEFORE k += 1
            k += 1;
            eps = sqrt(num / (1e-12 + den));                 // norm_diff, misc.py:1326-1351
        }
        h[S_K] = k; h[S_EPS] = eps; h[S_RHO] = rho; h[S_NBTSUM] = nbt; h[S_DEAD] = broke ? 1.0 : 0.0;
        if (xcur != x) PFB_HIP_CHECK(hipMemcpyAsync(x, xcur, n * sizeof(T), hipMemcpyDeviceToDevice, st));
        if (r_out) PFB_HIP_CHECK(hipMemcpyAsync(r_out, rcur, n * sizeof(T), hipMemcpyDeviceToDevice, st));
        if ((err = sync.wait_stream()) != PFB_OK) return err;
        PFB_HIP_CHECK(hipGetLastError());
        return PFB_OK;
    }

    void report(pfb_pcg_result* res) const {
        for (int s = 0; s < nsys; ++s) {
            const double* Sb = h.data() + (size_t)s * SB;
            pfb_pcg_result& o = res[s];
            o.rnorm = Sb[S_RHO];
            if (Sb[S_ZERO] != 0.0) {           // "Initial residual is zero": x untouched
                o.status = PFB_PCG_ZERO_RESIDUAL;
                o.matvecs = 1;
                o.eps = 1.0;
                continue;
            }
            const int k = (int)Sb[S_K];
            const bool dead = Sb[S_DEAD] != 0.0;
            o.status = dead ? PFB_PCG_BREAKDOWN : (k >= maxit ? PFB_PCG_MAXIT : PFB_PCG_CONVERGED);
            o.iters = k;
            o.eps = Sb[S_EPS];
            o.backtracks = (int)Sb[S_NBTSUM];
            o.matvecs = 1 + k + (dead ? 1 : 0);
        }
    }
};

template <typename T>
static int pcg_solve(const PcgSolve& q) {
    Pcg<T> s(q);
    PFB_REQUIRE(!q.allreduce || s.nsys == 1, PFB_ERR_INVALID, "pcg: an all-reduce hook needs the bands to be one system");
    memset(q.res, 0, sizeof(*q.res) * s.nsys);
    int err = s.init();
    // beta always comes from rho(alpha) in the sync-free driver: predict 2 with, 3 without the line search
    if (err == PFB_OK) err = q.backtrack == 1 ? s.run_exact() : s.run(q.backtrack == 2 ? 2 : 3, q.lookahead_max);
    if (err == PFB_OK) s.report(q.res);
    return err;
}

// what the three entry points (`who`) check alike, and the one fork by dtype
static int pcg_checked(const char* who, const PcgSolve& q) {
    PFB_REQUIRE(q.plan && q.b && q.x && q.work && q.res, PFB_ERR_INVALID, "%s: null argument", who);
    PFB_REQUIRE(q.band0 >= 0 && q.nb > 0 && q.band0 + q.nb <= q.plan->nband, PFB_ERR_INVALID,
                "%s: band range [%d,%d) outside plan", who, q.band0, q.band0 + q.nb);
    PFB_REQUIRE((reinterpret_cast<uintptr_t>(q.work) & 255u) == 0, PFB_ERR_INVALID,
                "%s: work must be 256-byte aligned", who);
    return q.plan->dtype == PFB_F32 ? pcg_solve<float>(q) : pcg_solve<double>(q);
}

}  // namespace pfb

using namespace pfb;

extern "C" {

int pfb_dot(int dtype, const void* a, const void* b, size_t n, double* out, double* ws, void* stream) {
    PFB_REQUIRE(a && b && out && ws, PFB_ERR_INVALID, "dot: null argument");
    return dtype == PFB_F32 ? dot_impl<float>(a, b, n, out, ws, as_stream(stream))
                            : dot_impl<double>(a, b, n, out, ws, as_stream(stream));
}

int pfb_norm_diff_sums(int dtype, const void* x, const void* xp, size_t n, double* out, double* ws,
                       void* stream) {
    PFB_REQUIRE(x && xp && out && ws, PFB_ERR_INVALID, "norm_diff_sums: null argument");
    return dtype == PFB_F32 ? nd_impl<float>(x, xp, n, out, ws, as_stream(stream))
                            : nd_impl<double>(x, xp, n, out, ws, as_stream(stream));
}

int pfb_any_nonzero(int dtype, const void* a, size_t n, double* out, double* ws, void* stream) {
    PFB_REQUIRE(a && out && ws, PFB_ERR_INVALID, "any_nonzero: null argument");
    return dtype == PFB_F32 ? any_impl<float>(a, n, out, ws, as_stream(stream))
                            : any_impl<double>(a, n, out, ws, as_stream(stream));
}

int pfb_axpby(int dtype, double a, const void* x, double b, void* y, size_t n, void* stream) {
    PFB_REQUIRE(x && y, PFB_ERR_INVALID, "axpby: null argument");
    return dtype == PFB_F32 ? axpby_impl<float>(a, x, b, y, n, as_stream(stream))
                            : axpby_impl<double>(a, x, b, y, n, as_stream(stream));
}
size_t pfb_pcg_work_bytes(const pfb_conv_plan* plan, int nb) {
    if (!plan || nb <= 0) return 0;
    return PcgLayout(plan, nb, 1, true, false).total;
}

int pfb_pcg_solve(pfb_conv_plan* plan, int band0, int nb, const void* b, void* x, void* r_out,
                  const void* beam, double wsum, double sigmainv, double mdiv, double tol,
                  int maxit, int minit, int backtrack, void* work, pfb_allreduce_fn allreduce,
                  void* allreduce_ctx, pfb_pcg_result* result, void* stream) {
    return pcg_checked("pcg_solve", {plan, band0, nb, false, b, x, r_out, beam, wsum, sigmainv, mdiv, tol, maxit, minit,
                                     backtrack, (size_t)4 << 20, work, allreduce, allreduce_ctx, nullptr, nullptr, result,
                                     as_stream(stream)});
}

size_t pfb_pcg_param_work_bytes(const pfb_conv_plan* plan, int nb) {
    if (!plan || nb != plan->nband) return 0;
    return PcgLayout(plan, nb, 1, true, true).total;
}

int pfb_pcg_solve_param(pfb_conv_plan* plan, int nb, const void* L, const void* LH, const void* e, const void* b,
                        void* x, void* r_out, double sigmainv, double mdiv, double tol, int maxit, int minit,
                        int backtrack, void* work, pfb_pcg_result* result, void* stream) {
    PFB_REQUIRE(plan && L && LH, PFB_ERR_INVALID, "pcg_solve_param: null argument");
    PFB_REQUIRE(nb == plan->nband, PFB_ERR_INVALID,
                "pcg_solve_param: the band mix couples all %d bands of the plan, nb = %d", plan->nband, nb);
    PFB_REQUIRE(nb <= 16, PFB_ERR_UNSUPPORTED, "pcg_solve_param: nband %d > 16", nb);
    PFB_REQUIRE(backtrack >= 0 && backtrack <= 2, PFB_ERR_INVALID, "pcg_solve_param: backtrack must be 0, 1 or 2");
    return pcg_checked("pcg_solve_param", {plan, 0, nb, false, b, x, r_out, e, 0.5, sigmainv, mdiv, tol, maxit, minit,
                                           backtrack, (size_t)4 << 20, work, nullptr, nullptr, L, LH, result,
                                           as_stream(stream)});
}

size_t pfb_pcg_bands_work_bytes(const pfb_conv_plan* plan, int nb) {
    if (!plan || nb <= 0) return 0;
    return PcgLayout(plan, nb, nb, false, false).total;
}

int pfb_pcg_solve_bands(pfb_conv_plan* plan, int band0, int nb, const void* b, void* x, void* r_out,
                        const void* beam, double wsum, double sigmainv, double mdiv, double tol,
                        int maxit, int minit, int backtrack, void* work, pfb_pcg_result* results, void* stream) {
    PFB_REQUIRE(backtrack != 1, PFB_ERR_UNSUPPORTED,
                "pcg_solve_bands: backtrack=1 (the exact loop) is not batched; solve band by band with pfb_pcg_solve");
    PFB_REQUIRE(backtrack == 0 || backtrack == 2, PFB_ERR_INVALID, "pcg_solve_bands: backtrack must be 0 or 2");
    return pcg_checked("pcg_solve_bands", {plan, band0, nb, true, b, x, r_out, beam, wsum, sigmainv, mdiv, tol, maxit,
                                           minit, backtrack, (size_t)16 << 20, work, nullptr, nullptr, nullptr, nullptr,
                                           results, as_stream(stream)});
}

}  // extern "C"
