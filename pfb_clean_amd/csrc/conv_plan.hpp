// conv_plan.hpp -- the PSF-convolution plan shared by the generic and the pow2 kernels.
//
// Data layout in HBM (per band b; P = nx_psf, Q = ny_psf, M = Q/2):
//   x, out     (nx, ny) real, row-major (caller-owned)
//   T          half-spectrum after the row (y) transform, BLOCKED-TRANSPOSED:
//                T[b][v / VB][i][v % VB]   v in [0, M], i in [0, nx)
//              so a group of VB adjacent frequency columns is ONE contiguous region
//              of nx*VB complex: the column (x) transform streams it with unit stride
//              and the row passes write VB-wide pieces.  The column pass works in
//              place (reads column v of T, writes column v of T).
//   psf_l      the caller's psfhat (P, M+1) re-laid out once into the same blocking:
//                psf_l[b][v / VB][u][v % VB]  u in [0, P)
//              Only the fast path blocks (VB > 1); the coverage paths keep VB = 1, T[b][v][i] and psf_l[b][v][u].
//   twP, twQ   exp(-2 pi i n / P), exp(-2 pi i n / Q), computed in long double.
#pragma once
#include "common.hpp"
#include "fft_generic.hpp"

// Where a row-inverse launch left its fused-dot partials in plan->partials: `slots` per quantity; band bl's `band_slots`
// partials of quantity q start at q * q_stride + bl * band_stride (band_slots 0: the launch summed across bands -- the
// whole-cube persistent kernel).  Read by k_sum_partials* and psfconv_apply_partials.
struct pfb_partial_layout {
    int slots, band_slots, q_stride, band_stride;
};

struct pfb_conv_plan {
    int nx, ny, P, Q, M;       // M = Q/2
    int nband, dtype;
    int VB, nvb;               // column blocking, number of column blocks
    int fast;                  // 1: pow2 register-resident kernels are used
    int long_lines;            // 1: a line does not fit the LDS and the fast path cannot hold the grid: every transform
                               //    runs as multi-launch global-memory passes (fft_long.hpp) -- coverage, not speed
    void* long_ws;             // the scratch of its stages (grown on demand, freed with the plan)
    size_t long_ws_bytes;
    pfb::FftFactors frow;      // length M  (row transform on packed reals)
    pfb::FftFactors fcol;      // length P
    void* twP;
    void* twQ;
    void* psf_l;
    void* T;
    double* partials;          // nx * nband doubles (fused dot)
    size_t T_elems_per_band;   // nvb * nx * VB
    size_t psf_elems_per_band; // nvb * P * VB
    size_t workspace_bytes;
    int have_psf;
    int partials_per_band;     // fused-dot partial sums emitted per band by row_inv
    pfb_partial_layout last;   // of the LAST row-inverse launch (apply_common sets the default, the pow2 launcher its own)
    void* fast_tables;         // pow2 path: per-pass twiddle tables (fftconv_pow2.hip)
    // optional per-stage timing (bench.py roofline): 4 events per apply, up to PROF_MAX applies
    int prof_on, prof_n, prof_tick;   // prof_on = sampling period (every prof_on-th apply is timed)
    hipEvent_t* prof_ev;
    // PCG driver (cgvec.hip): two pinned snapshots of the solver's `pcg_pin_n` state blocks + their events, for looking
    // at iteration j-1 while iteration j is already enqueued (created on first use, grown on demand)
    double* pcg_pin;
    int pcg_pin_n;
    hipEvent_t pcg_ev[2];
};

namespace pfb {
// bytes of `nb` bands of the plan's images, rounded up to the 256 bytes every region of a work buffer starts on
inline size_t vec_bytes(const pfb_conv_plan* plan, int nb) {
    const size_t b = (size_t)nb * plan->nx * plan->ny * (plan->dtype == PFB_F32 ? 4 : 8);
    return (b + 255) & ~(size_t)255;
}
constexpr int PROF_MAX = 512;
// record stage boundary `k` (0..3) of the current apply on `st` when profiling is on
inline void prof_mark(pfb_conv_plan* p, hipStream_t st, int k) {
    if (!p->prof_on) return;
    const bool sampled = (p->prof_tick % p->prof_on) == 0 && p->prof_n < PROF_MAX;
    if (sampled) (void)hipEventRecord(p->prof_ev[p->prof_n * 4 + k], st);
    if (k == 3) {
        if (sampled) p->prof_n++;
        p->prof_tick++;
    }
}
// fftconv.hip: convolution + fused dots left un-summed in plan->partials (see there).  The PCG's systems are the bands
// (`per_band`) or the whole range is one; system s's `bs` partials of quantity q start at q * qs + s * bst
int psfconv_apply_partials(pfb_conv_plan* p, int band0, int nb, const void* x, const void* beam,
                           double wsum, double sigmainv, void* out, const void* dot_with,
                           const void* dot_with2, bool per_band, int* bs, int* qs, int* bst, void* stream);
// One apply: bands [band0, band0 + nb) of x (times beam, if given) convolved into out on `st`; the epilogue's scale
// (1 / (P Q wsum)) and sigmainv, and the operands of the fused dots (per band, or over the whole range).  Built once by
// apply_common (fftconv.hip) and handed down by reference to the coverage path and to the fast path's launchers.
struct ApplyArgs {
    int band0, nb;
    const void *x, *beam;
    double scale, sigmainv;
    void* out;
    const void *dot_with, *dot_with2;
    bool per_band;
    hipStream_t st;
};
// fftconv_pow2.hip: the fast path's entry points
bool pow2_supported(const pfb_conv_plan* p);
int pow2_apply(pfb_conv_plan* p, const ApplyArgs& a);
int pow2_prepare(pfb_conv_plan* p);
void pow2_release(pfb_conv_plan* p);
int pow2_rows_per_wg(const pfb_conv_plan* p);
int pow2_nblocks(const pfb_conv_plan* p);
int pow2_nvb(const pfb_conv_plan* p);
int pow2_set_psfhat(pfb_conv_plan* p, const void* psfhat, hipStream_t st);
int pow2_set_psf(pfb_conv_plan* p, const void* psf, void* psfhat_out, hipStream_t st);
}  // namespace pfb
