// pcg_state.hpp -- the device-resident scalar state of the PCG driver (cgvec.hip) and the per-iteration bookkeeping on
// it.  A SYSTEM is a contiguous run of bands that is solved as one PCG -- the whole cube (pfb_pcg_solve) or one band
// (pfb_pcg_solve_bands) -- and owns one state block of SB doubles, S + s * SB.
#pragma once
#include "conv_plan.hpp"

namespace pfb {

// scalar slots in the device state array
enum { S_PAP = 0, S_RAP = 1, S_APAP = 2,          // <p,Ap>, <r,Ap>, <Ap,Ap>   (conv epilogue)
       S_ANY = 3,                                 // count(p != 0) of the direction in use
       S_RHON = 4, S_NUM = 5, S_DEN = 6,          // <r',y'>, |x'-x|^2, |x'|^2 (update kernel)
       S_RHO = 7, S_ALPHA = 8, S_BETA = 9, S_NBT = 10,
       S_DEAD = 11,                               // p became all-zero: later work is a no-op
       S_K = 12, S_EPS = 13, S_EPSP = 14, S_NBTSUM = 15,
       S_STOP = 16,                               // the stopping rule fired on the device: later work is a no-op
       S_TOL = 17, S_MINIT = 18, S_MAXIT = 19,    // the rule's parameters (set once per solve)
       S_ZERO = 20,                               // the initial residual was zero: the system never iterates
       S_NSCALAR = 21 };
constexpr int SB = 32;                            // doubles per state block
static_assert(S_NSCALAR <= SB, "state block too small");

// a system that has stopped (S_STOP) or broken down (S_DEAD) is neither read nor written, and its state is left as the
// iteration that stopped it left it
__device__ __host__ __forceinline__ bool sys_live(const double* Sb) { return Sb[S_DEAD] == 0.0 && Sb[S_STOP] == 0.0; }

// ---- device-side loop bookkeeping of the sync-free driver
__device__ __forceinline__ void iter_begin_dev(double* S, double mdiv, int predict) {
    if (S[S_DEAD] != 0.0 || S[S_STOP] != 0.0) return;
    if (S[S_ANY] == 0.0) {                 // the direction built last iteration is all zero:
        S[S_DEAD] = 1.0;                   // the reference broke BEFORE k += 1 (pcg.py:106-108)
        S[S_K] -= 1.0;
        S[S_EPS] = S[S_EPSP];
        return;
    }
    const double rho = S[S_RHO];
    double alpha = rho / S[S_PAP];
    int nbt = 0;
    if (predict == 1 || predict == 2) {
        const double d = mdiv > 0.0 ? mdiv : 1.0;
        const double s1 = S[S_RAP] / d, s2 = S[S_APAP] / d;
        while (rho + (2.0 * alpha * s1 + alpha * alpha * s2) > rho && nbt < 200) { alpha *= 0.75; ++nbt; }
    }
    S[S_ALPHA] = alpha;
    S[S_NBT] = (double)nbt;
    if (predict >= 2) {                    // fused update+direction: beta from rho(alpha)
        const double d = mdiv > 0.0 ? mdiv : 1.0;
        S[S_BETA] = (rho + (2.0 * alpha * S[S_RAP] + alpha * alpha * S[S_APAP]) / d) / rho;
    }
}
__device__ __forceinline__ void iter_end_dev(double* S) {
    if (S[S_DEAD] != 0.0 || S[S_STOP] != 0.0) return;
    S[S_RHO] = S[S_RHON];
    const double k = S[S_K] + 1.0;
    const double eps = sqrt(S[S_NUM] / (1e-12 + S[S_DEN]));
    S[S_K] = k;
    S[S_EPSP] = S[S_EPS];
    S[S_EPS] = eps;
    S[S_NBTSUM] += S[S_NBT];
    // the reference's loop condition (pcg.py:86), evaluated where the numbers are: an iteration the host
    // enqueued speculatively behind this one finds S_STOP set and changes nothing
    if (!((eps > S[S_TOL] || k < S[S_MINIT]) && k < S[S_MAXIT])) S[S_STOP] = 1.0;
}

// ---- the operator step of the parametrised solve (pfb_pcg_solve_param), hessparam.hip:
// out = L^T [e conv(e (L x)) / 0.5] + sigmainv x over all the plan's bands (L, LH: device nband x nband; e: null or a
// cube; tmp: one cube of scratch; x, out, tmp distinct).  partials non-null: the per-workgroup fp64 partials of <x,out>,
// <r,out> (r may be null), <out,out>, quantity-major with *grid (<= MIX_MAX_GRID) per quantity -- what k_iter_sums
// reads through (cp, bs = qs = *grid, bst = 0)
constexpr int MIX_MAX_GRID = 1024;
int hessparam_apply_partials(pfb_conv_plan* plan, const void* L, const void* LH, const void* e, double sigmainv,
                             const void* x, void* out, const void* r, void* tmp, double* partials, int* grid,
                             hipStream_t st);
// its scratch, stated once: `tmp` at the start, the partials behind it (pfb_hessparam_work_bytes; the tail of the
// parametrised solve's work buffer, cgvec.hip)
struct MixWork {
    size_t partials, total;
    explicit MixWork(const pfb_conv_plan* plan)
        : partials(vec_bytes(plan, plan->nband)), total(partials + sizeof(double) * 3 * MIX_MAX_GRID) {}
};

}  // namespace pfb
