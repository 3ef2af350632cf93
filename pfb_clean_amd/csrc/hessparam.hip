// hessparam.hip -- the band-coupled Hessian of the parametrised forward step (fwdbwd.py:246-252, misc.py:1366-1423):
//
//   hesspsf(v) = 2 dhf(psf_convolve(df(v))) + sigmainv v,   df(v) = e * (L v),  dhf(w) = L^T (e * w),  e = exp(L x0) | 1
//              = L^T [ e * conv(e * (L v)) / wsum ] + sigmainv v        with wsum = 0.5 (the factor 2, exact)
//
// The bracket is the beam sandwich the convolution's row kernels already fuse (pfb_psfconv_apply with beam = e).  New
// here are the two band mixes around it:
//   k_bandmix<T, NB, V, DOTS>   out[k] = sum_l A[k, l] c[l]  [+ sigmainv p[k]]  [+ fp64 partials of <p,out>, <r,out>,
//                               <out,out>]
// NB is a compile-time band count (1 .. 16): a thread holds the NB values (16-byte packs where the planes allow it) of
// its pixels in registers, nothing is indexed at run time (pfb_freqmul's xv[FM_MAXBAND] lives in scratch memory), the
// matrix sits in LDS and is read at wave-uniform addresses.  The sum runs in T with l ascending from zero: pfb_freqmul's
// order, which is the reference loop's.  A thread reads all NB inputs of a pixel before it writes any output, and a
// pixel belongs to one thread: `out` may be `c` itself.
// The partials are quantity-major, one per workgroup (emit_partials): k_iter_sums of the PCG driver (cgvec.hip) reads
// them with bs = qs = grid, bst = 0.
#include "conv_plan.hpp"
#include "pcg_state.hpp"
#include "entry.hpp"

namespace pfb {

constexpr int MIX_MAXBAND = 16;         // MIX_MAX_GRID (pcg_state.hpp): 3 sums x grid doubles of partials

__device__ __forceinline__ float fma_t(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_t(double a, double b, double c) { return __builtin_fma(a, b, c); }

// nvp: 16-byte vectors (V > 1) or elements (V = 1) per band plane.  p null: no Tikhonov term (and no sums); r null:
// the second sum stays zero.  c, p, r, out carry no __restrict__: out may alias c.
template <typename T, int NB, int V, bool DOTS>
__global__ void __launch_bounds__(RED_BLOCK)
k_bandmix(const T* __restrict__ A, const T* c, size_t nvp, T sigmainv, const T* p, const T* r, T* out,
          double* __restrict__ ws) {
    __shared__ T As[NB * NB];
    for (int k = threadIdx.x; k < NB * NB; k += blockDim.x) As[k] = A[k];
    __syncthreads();
    const size_t plane = nvp * V;
    double acc[3] = {0.0, 0.0, 0.0};
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvp; i += (size_t)gridDim.x * blockDim.x) {
        Pack<T, V> xv[NB];
#pragma unroll
        for (int l = 0; l < NB; ++l) xv[l] = ld<T, V>(c + (size_t)l * plane, i);
        // a real loop over the output bands: unrolled, the NB * NB matrix reads are hoisted out of the pixel loop into
        // registers (NB = 16: all 512 of them and 764 B of scratch); the inputs xv[l] keep compile-time indices
#pragma unroll 1
        for (int k = 0; k < NB; ++k) {
            Pack<T, V> o;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                T s = 0;
#pragma unroll
                for (int l = 0; l < NB; ++l) s += As[k * NB + l] * xv[l].e[e];
                o.e[e] = s;
            }
            if (p) {
                const Pack<T, V> pp = ld<T, V>(p + (size_t)k * plane, i);
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    o.e[e] = fma_t(sigmainv, pp.e[e], o.e[e]);      // one rounding for the Tikhonov term
                    if constexpr (DOTS) acc[0] += (double)pp.e[e] * (double)o.e[e];
                }
            }
            if constexpr (DOTS) {
                if (r) {
                    const Pack<T, V> pr = ld<T, V>(r + (size_t)k * plane, i);
#pragma unroll
                    for (int e = 0; e < V; ++e) acc[1] += (double)pr.e[e] * (double)o.e[e];
                }
#pragma unroll
                for (int e = 0; e < V; ++e) acc[2] += (double)o.e[e] * (double)o.e[e];
            }
            st<T, V>(out + (size_t)k * plane, i, o);
        }
    }
    if constexpr (DOTS) emit_partials<3>(acc, ws);
}

template <typename T, int NB>
static void bandmix_nb(bool vec, int G, size_t nvp, const void* A, const void* c, double sigmainv, const void* p,
                       const void* r, void* out, double* partials, hipStream_t st) {
#define PFB_MIX(VV, DD)                                                                                         \
    hipLaunchKernelGGL((k_bandmix<T, NB, VV, DD>), dim3(G), dim3(RED_BLOCK), 0, st, (const T*)A, (const T*)c, nvp, \
                       (T)sigmainv, (const T*)p, (const T*)r, (T*)out, partials)
    if (vec) { if (partials) PFB_MIX(V16<T>::N, true); else PFB_MIX(V16<T>::N, false); }
    else     { if (partials) PFB_MIX(1, true); else PFB_MIX(1, false); }
#undef PFB_MIX
}

template <typename T>
static int bandmix_t(const void* A, const void* c, int nband, size_t npix, double sigmainv, const void* p,
                     const void* r, void* out, double* partials, int* grid, hipStream_t st) {
    using PL = std::initializer_list<const void*>;
    // every plane base is 16-byte aligned when the cube's base is and a plane is a whole number of vectors
    const bool vec = can_vec<T>(npix, PL{c, p, r, out});
    const size_t nvp = vec ? npix / V16<T>::N : npix;
    size_t g = (nvp + RED_BLOCK - 1) / RED_BLOCK;
    if (g > (size_t)MIX_MAX_GRID) g = MIX_MAX_GRID;
    const int G = (int)g;
    switch (nband) {
#define PFB_CASE(N) case N: bandmix_nb<T, N>(vec, G, nvp, A, c, sigmainv, p, r, out, partials, st); break;
        PFB_CASE(1) PFB_CASE(2) PFB_CASE(3) PFB_CASE(4) PFB_CASE(5) PFB_CASE(6) PFB_CASE(7) PFB_CASE(8)
        PFB_CASE(9) PFB_CASE(10) PFB_CASE(11) PFB_CASE(12) PFB_CASE(13) PFB_CASE(14) PFB_CASE(15) PFB_CASE(16)
#undef PFB_CASE
        default: set_error("bandmix: nband %d outside 1..%d", nband, MIX_MAXBAND); return PFB_ERR_UNSUPPORTED;
    }
    PFB_HIP_CHECK(hipGetLastError());
    if (grid) *grid = G;
    return PFB_OK;
}

static int bandmix_partials(int dtype, const void* A, const void* c, int nband, size_t npix, double sigmainv, const void* p,
                     const void* r, void* out, double* partials, int* grid, hipStream_t st) {
    PFB_REQUIRE(A && c && out, PFB_ERR_INVALID, "bandmix: null argument");
    PFB_REQUIRE(dtype == PFB_F32 || dtype == PFB_F64, PFB_ERR_INVALID, "bandmix: bad dtype");
    PFB_REQUIRE(nband >= 1 && nband <= MIX_MAXBAND, PFB_ERR_UNSUPPORTED, "bandmix: nband %d outside 1..%d", nband,
                MIX_MAXBAND);
    PFB_REQUIRE(npix >= 1, PFB_ERR_INVALID, "bandmix: empty plane");
    PFB_REQUIRE(p || (!r && !partials), PFB_ERR_INVALID, "bandmix: the sums need p");
    PFB_REQUIRE(p != out && r != out, PFB_ERR_INVALID, "bandmix: out may alias c only");
    return dtype == PFB_F32 ? bandmix_t<float>(A, c, nband, npix, sigmainv, p, r, out, partials, grid, st)
                            : bandmix_t<double>(A, c, nband, npix, sigmainv, p, r, out, partials, grid, st);
}

// mix (L) -> convolution with the e sandwich and wsum = 0.5 -> mix (L^T) + sigmainv x [+ partials].  `out` holds L x
// between the first two steps, `tmp` the convolution's output (which may not alias its input).
int hessparam_apply_partials(pfb_conv_plan* plan, const void* L, const void* LH, const void* e, double sigmainv,
                             const void* x, void* out, const void* r, void* tmp, double* partials, int* grid,
                             hipStream_t st) {
    const size_t npix = (size_t)plan->nx * plan->ny;
    int rc = bandmix_partials(plan->dtype, L, x, plan->nband, npix, 0.0, nullptr, nullptr, out, nullptr, nullptr, st);
    if (rc != PFB_OK) return rc;
    rc = pfb_psfconv_apply(plan, 0, plan->nband, out, e, 0.5, 0.0, tmp, nullptr, nullptr, (void*)st);
    if (rc != PFB_OK) return rc;
    return bandmix_partials(plan->dtype, LH, tmp, plan->nband, npix, sigmainv, x, r, out, partials, grid, st);
}

}  // namespace pfb

using namespace pfb;

extern "C" {

int pfb_bandmix_dots(int dtype, const void* A, const void* c, int nband, size_t npix, double sigmainv, const void* p,
                     const void* r, void* out, double* dots3, double* ws, void* stream) {
    PFB_REQUIRE(!dots3 || ws, PFB_ERR_INVALID, "bandmix_dots: dots3 needs the reduction scratch ws");
    PFB_REQUIRE(dots3 || !r, PFB_ERR_INVALID, "bandmix_dots: r given without dots3");
    hipStream_t st = as_stream(stream);
    int G = 0;
    const int rc = bandmix_partials(dtype, A, c, nband, npix, sigmainv, p, r, out, dots3 ? ws : nullptr, &G, st);
    if (rc != PFB_OK || !dots3) return rc;
    return final_sum(ws, G, 3, dots3, st);
}

size_t pfb_hessparam_work_bytes(const pfb_conv_plan* plan) {
    if (!plan) return 0;
    return MixWork(plan).total;
}

static int hessparam_checked(pfb_conv_plan* plan, const void* L, const void* LH, const void* e, double sigmainv,
                             const void* x, void* out, const void* dot_with, const void* dot_with2, double* dots_out,
                             void* work, void* stream) {
    PFB_REQUIRE(plan && L && LH && x && out && work, PFB_ERR_INVALID, "hessparam_apply: null argument");
    PFB_REQUIRE(plan->nband <= MIX_MAXBAND, PFB_ERR_UNSUPPORTED, "hessparam_apply: nband %d > %d", plan->nband,
                MIX_MAXBAND);
    PFB_REQUIRE(x != out && work != x && work != out, PFB_ERR_INVALID, "hessparam_apply: x, out and work must differ");
    PFB_REQUIRE((reinterpret_cast<uintptr_t>(work) & 255u) == 0, PFB_ERR_INVALID,
                "hessparam_apply: work must be 256-byte aligned");
    PFB_REQUIRE(!dots_out || dot_with == x, PFB_ERR_UNSUPPORTED,
                "hessparam_apply_dots: dot_with must be x itself (the products the PCG and the power method form)");
    hipStream_t st = as_stream(stream);
    double* partials = dots_out ? (double*)((char*)work + MixWork(plan).partials) : nullptr;
    int G = 0;
    const int rc = hessparam_apply_partials(plan, L, LH, e, sigmainv, x, out, dot_with2, work, partials, &G, st);
    if (rc != PFB_OK || !dots_out) return rc;
    return final_sum(partials, G, 3, dots_out, st);
}

int pfb_hessparam_apply(pfb_conv_plan* plan, const void* L, const void* LH, const void* e, double sigmainv,
                        const void* x, void* out, void* work, void* stream) {
    return hessparam_checked(plan, L, LH, e, sigmainv, x, out, nullptr, nullptr, nullptr, work, stream);
}

int pfb_hessparam_apply_dots(pfb_conv_plan* plan, const void* L, const void* LH, const void* e, double sigmainv,
                             const void* x, void* out, const void* dot_with, const void* dot_with2, double* dots_out,
                             void* work, void* stream) {
    PFB_REQUIRE(dot_with && dots_out, PFB_ERR_INVALID, "hessparam_apply_dots: dot_with and dots_out are required");
    return hessparam_checked(plan, L, LH, e, sigmainv, x, out, dot_with, dot_with2, dots_out, work, stream);
}

}  // extern "C"
