/*
 * pfb_hip.h -- C-ABI of libpfb_hip.so: the MI355X (gfx950) implementation of the
 * pfb-imaging PCG / PSF-convolution / wavelet hot path.
 *
 * The reference (ratt-ru/pfb-imaging 0.0.4) is pure Python and has no FFI of its own;
 * its boundary is the set of Python callables the workers import.  Each
 * entry point below names the reference function (file:line under /root/reference)
 * whose arithmetic it replaces; pfb_clean_amd/{operators,opt,prox,wavelets,utils}
 * re-export the reference's Python names on top of these and INTEGRATION.md shows
 * the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - every function returns an int status (PFB_OK = 0, negative = error) and never
 *     throws; pfb_last_error() gives a thread-local message for the last failure;
 *   - all array arguments are DEVICE pointers (hipMalloc / torch-ROCm storage),
 *     C-contiguous, in the dtype named by `dtype` (real arrays) or its complex pair
 *     (interleaved re,im);
 *   - `stream` is a hipStream_t passed as void*; nothing synchronises the device
 *     except functions documented to (the *_solve drivers read scalars back);
 *   - the library never allocates caller-visible memory: plans own their twiddles /
 *     re-laid-out PSF / workspaces, callers own every vector;
 *   - one plan may be used by one stream AND one host thread at a time (its spectrum
 *     workspace, fused-dot partials and profiling slots are per plan); distinct plans
 *     are independent and there is no global mutable state (re-entrant like the
 *     reference, which dask may call from several threads with one band each,
 *     pcg.py:346-356 -- one plan per band there).
 */
#ifndef PFB_HIP_H
#define PFB_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PFB_ABI_VERSION 1

/* dtype of the real arrays; complex arrays use the matching complex type */
#define PFB_F32 0
#define PFB_F64 1

/* status codes */
#define PFB_OK               0
#define PFB_ERR_INVALID     -1   /* bad argument (null pointer, shape mismatch ...)      */
#define PFB_ERR_UNSUPPORTED -2   /* size / radix / dtype outside the supported set       */
#define PFB_ERR_HIP         -3   /* a HIP runtime call failed                            */
#define PFB_ERR_NONFINITE   -4   /* NaN/Inf met where the reference drops into pdb       */
#define PFB_ERR_ALLOC       -5   /* device allocation for a plan failed                  */
#define PFB_ERR_COMM        -6   /* the band-shard exchange failed, was aborted or timed out */

/* pcg exit status (written to pfb_pcg_result.status) */
#define PFB_PCG_CONVERGED     0  /* "Success, converged after k iterations" pcg.py:131-132 */
#define PFB_PCG_MAXIT         1  /* "Max iters reached"                    pcg.py:124-126 */
#define PFB_PCG_ZERO_RESIDUAL 2  /* "Initial residual is zero": x0 returned pcg.py:73-75  */
#define PFB_PCG_BREAKDOWN     3  /* search direction became all-zero       pcg.py:106-107 */

int         pfb_abi_version(void);
const char* pfb_last_error(void);

/* ------------------------------------------------------------------ PSF convolution
 * Replaces pfb/operators/psf.py:11-29 (psf_convolve_slice), :32-56 (psf_convolve_cube)
 * and the Tikhonov-regularised wrappers pfb/operators/hessian.py:129-158
 * (_hessian_psf_slice) and :254-281 (hessian_psf_cube):
 *
 *   out = [beam *] crop( irfft2( rfft2( pad([beam *] x) ) * psfhat ) ) [/ wsum]
 *         + sigmainv * x
 *
 * rfft2 unnormalised (ducc0 r2c inorm=0), irfft2 scaled by 1/(nx_psf*ny_psf) (c2r
 * inorm=2, lastsize=ny_psf), imaginary parts of the DC / Nyquist bins of the last
 * axis ignored like ducc0/pocketfft do.
 */
typedef struct pfb_conv_plan pfb_conv_plan;

/* nx,ny: image; nx_psf,ny_psf(=lastsize): padded PSF grid, ny_psf even,
 * nx <= nx_psf, ny <= ny_psf; every 1-D length must factor into {2,3,5,7,11,13}.
 * nband: leading (imaging band) axis of the cubes this plan serves.
 * Three kernel families behind one plan, chosen here: power-of-two images with nx_psf = 2 nx, ny_psf = 2 ny
 * (64 <= nx <= 8192, 128 <= ny <= 16384 fp32 / 8192 fp64) take the register-FFT fast path; other grids the
 * line-in-LDS coverage kernels while a line fits (<= 10240 complex64 / 5120 complex128), and multi-launch
 * global-memory passes beyond that -- no grid is refused for its size (the host layer embeds arbitrary sizes in the
 * fast path through pfb_psfhat_regrid whenever that is possible: see pfb_clean_amd/operators/psf.py). */
int pfb_psfconv_plan_create(int nx, int ny, int nx_psf, int ny_psf, int nband,
                            int dtype, pfb_conv_plan** plan);
int pfb_psfconv_plan_destroy(pfb_conv_plan* plan);

/* psfhat: (nband, nx_psf, ny_psf/2+1) complex, as produced by
 * pfb/operators/gridder.py:712-714 (r2c(ifftshift(psf))) and divided by wsum in
 * pfb/utils/misc.py:721-723.  Copied into the plan's own layout (once). */
int pfb_psfconv_set_psfhat(pfb_conv_plan* plan, const void* psfhat, void* stream);

/* Produce psfhat ON THE DEVICE from the real PSF and install it:
 *   psfhat = r2c(ifftshift(psf), axes=(0,1), forward, unnormalised)
 * (pfb/operators/gridder.py:712-714 and pfb/utils/fft.py:7-9).  psf: (nband, nx_psf, ny_psf)
 * real, row-major.  psfhat_out: NULL, or (nband, nx_psf, ny_psf/2+1) complex that also
 * receives the transform in the reference's layout (e.g. for the DDS PSFHAT variable).
 * Power-of-two plans (nx_psf = 2 nx, ny_psf = 2 ny: every BASELINE size up to 16384 x 16384 fp64) run it on
 * the fast path's own register-FFT row / column kernels; other plans on the line-in-LDS kernels.  Synchronous. */
int pfb_psfconv_set_psf(pfb_conv_plan* plan, const void* psf, void* psfhat_out, void* stream);

/* The same transform without a plan, for ANY grid whose lengths are 13-smooth and whose ny_psf is even:
 * psfhat (nband, nx_psf, ny_psf/2+1) = r2c(ifftshift(psf)).  Lines that fit the LDS take the
 * one-workgroup-per-line kernels, longer ones (nx_psf > 10240 fp32 / 5120 fp64) multi-launch Stockham passes
 * in global memory -- no length limit.  Plan time (gridder.py:712-714 runs once per gridding run).  Synchronous. */
int pfb_psfhat_from_psf(int dtype, const void* psf, int nband, int nx_psf, int ny_psf, void* psfhat, void* stream);

/* Re-grid a PSF transform: psfhat on the (nx_psf, ny_psf) grid -> psfhat2 of the SAME image-space
 * PSF on an (nx_psf2, ny_psf2) grid (both (nband, n, m/2+1) complex, row-major), for images of
 * (nx, ny) pixels: only the offsets |du| < nx, |dv| < ny a convolution of such an image touches
 * are carried over (periodically in the old grid, so the wrap-around of grids with
 * nx_psf < 2 nx is reproduced), which needs nx_psf2 >= 2 nx - 1, ny_psf2 >= 2 ny - 1.
 * The convolution psf.py:11-56 on the old grid and on the new grid (image zero-padded to
 * nx_psf2/2 x ny_psf2/2, result cropped) then agree to rounding; the host layer uses this to run
 * arbitrary image sizes on the power-of-two fast path.  Plan-time, synchronous.  Lengths 13-smooth, last axes
 * even; lines of any length (beyond the LDS: multi-launch global-memory passes). */
int pfb_psfhat_regrid(int dtype, const void* psfhat, int nband, int nx, int ny, int nx_psf, int ny_psf,
                      int nx_psf2, int ny_psf2, void* psfhat2, void* stream);

/* Apply to bands [band0, band0+nb) of the plan.  x, out: (nb, nx, ny) real; out may
 * not alias x.  beam: (nb, nx, ny) or NULL.  wsum <= 0 means "no division"
 * (reference wsum=None).  sigmainv may be 0.
 * If dot_with != NULL (same shape as x) the fp64 sum over all nb bands of
 * dot_with*out is written to *dot_out (device double) -- the fused p.Ap of
 * pcg.py:91.  Asynchronous on `stream`. */
int pfb_psfconv_apply(pfb_conv_plan* plan, int band0, int nb,
                      const void* x, const void* beam, double wsum, double sigmainv,
                      void* out, const void* dot_with, double* dot_out, void* stream);

/* Same, with the three fused fp64 sums the predictive line search of pfb_pcg_solve needs:
 * dots_out[0] = <dot_with, out>, dots_out[1] = <dot_with2, out> (0 if dot_with2 is NULL),
 * dots_out[2] = <out, out>  -- all over the nb bands (pcg.py:91,95 and the backtracking
 * loop :96-101 evaluated without further passes over the vectors). */
int pfb_psfconv_apply_dots(pfb_conv_plan* plan, int band0, int nb,
                           const void* x, const void* beam, double wsum, double sigmainv,
                           void* out, const void* dot_with, const void* dot_with2,
                           double* dots_out, void* stream);

/* Same apply, with the three sums PER BAND: dots_out is [nb][3] device doubles, dots_out[3 bl + 0] =
 * <dot_with, out>, [3 bl + 1] = <dot_with2, out> (0 if dot_with2 is NULL), [3 bl + 2] = <out, out> over band
 * band0 + bl alone, each summed in fp64 in a fixed order (the per-band products pfb_pcg_solve_bands needs). */
int pfb_psfconv_apply_dots_bands(pfb_conv_plan* plan, int band0, int nb,
                                 const void* x, const void* beam, double wsum, double sigmainv,
                                 void* out, const void* dot_with, const void* dot_with2,
                                 double* dots_out, void* stream);

/* Introspection for benchmarks / tests */
int    pfb_psfconv_plan_info(const pfb_conv_plan* plan, int* fast_path, int* vb,
                             size_t* workspace_bytes);

/* Per-stage timing for benchmarks: while on > 0, every on-th apply (on = 1: every apply)
 * records HIP events on its stream around the three kernels (row-forward, column,
 * row-inverse) -- an event record costs ~6 us of stream time, hence the sampling period;
 * get_profile waits for them, returns the summed milliseconds per stage and the number of
 * applies covered (at most 512 between calls), and resets the counters. */
int pfb_psfconv_set_profiling(pfb_conv_plan* plan, int on);
int pfb_psfconv_get_profile(pfb_conv_plan* plan, double stage_ms[3], int* napply);

/* ------------------------------------------------------------- CG vector kernels
 * Fused replacements for the numpy passes of pfb/opt/pcg.py:77-111 and
 * pfb/utils/misc.py:1316-1351 (norm_diff).  `ws` is a caller-provided device
 * scratch of at least PFB_REDUCE_WS_DOUBLES doubles; results are device doubles,
 * accumulated in fp64 in a fixed (deterministic) order. */
#define PFB_REDUCE_WS_DOUBLES 8192

/* out[0] = sum a*b                                   (np.vdot on real arrays) */
int pfb_dot(int dtype, const void* a, const void* b, size_t n,
            double* out, double* ws, void* stream);
/* out[0] = sum (x-xp)^2, out[1] = sum x^2            (norm_diff partial sums) */
int pfb_norm_diff_sums(int dtype, const void* x, const void* xp, size_t n,
                       double* out, double* ws, void* stream);
/* out[0] = 1.0 if any element of a is non-zero else 0.0   (np.any) */
int pfb_any_nonzero(int dtype, const void* a, size_t n, double* out, double* ws,
                    void* stream);
/* y = a*x + b*y elementwise (a, b host scalars) */
int pfb_axpby(int dtype, double a, const void* x, double b, void* y, size_t n,
              void* stream);

/* -------------------------------------------------------------------- fused PCG
 * Replaces pfb/opt/pcg.py:53-136 (pcg) for the operator
 *   A(x) = hessian_psf(plan, beam, wsum, sigmainv)           (hessian.py:129-158/254-281)
 * and the preconditioner M(r) = r / mdiv (mdiv = sigmainv as pcg.py:264-267;
 * mdiv <= 0 means M = identity).  NaN/Inf propagate silently exactly as in the reference.
 * Works on bands [band0, band0+nb) as ONE system (np.vdot over the whole cube, the
 * fluxmop semantics fluxmop.py:193-199); for pcg_psf semantics call it once per band, or solve all
 * bands at once with pfb_pcg_solve_bands below.
 *
 * backtrack: 0 = off; 1 = the reference's loop verbatim (every rejected step re-runs the
 * vector update); 2 = predictive: the same decisions from the quadratic
 * rnorm(alpha) = rnorm + (2 alpha <r,Ap> + alpha^2 <Ap,Ap>)/mdiv (three scalars fused into the
 * convolution epilogue), then ONE vector update with the accepted alpha.  1 and 2 differ only
 * by rounding in the comparison rnorm_next > rnorm.
 *
 * allreduce: optional hook for band-sharded multi-GPU solves -- called on `stream`
 * order with a device buffer of `count` doubles that must be summed in place over
 * all ranks (RCCL); NULL for single-GPU.
 * Failure protocol (the reference's sums run over all bands in one process, pfb/opt/pcg.py:90-107, and cannot
 * lose a participant; a sharded solve can).  The same function doubles as the health interface of the exchange:
 *   count  > 0   the exchange itself; non-zero return = it could not be issued
 *   count == 0   PROBE (dev_buf NULL): non-zero = the exchange has failed asynchronously (a peer died, the
 *                communicator was aborted); called by the solver while it waits for the device
 *   count  < 0   ABORT (dev_buf NULL): tear the exchange down so that neither this rank nor its peers stay blocked
 *                in a collective; called once before the solver gives up
 * A solver with a hook never waits for the device unboundedly: it polls, probes, and after PFB_COMM_TIMEOUT_S
 * seconds (environment, default 600) without progress aborts the exchange.  In all three cases pfb_pcg_solve
 * returns PFB_ERR_COMM; the caller's buffers then hold no result and the process should exit non-zero.
 */
typedef int (*pfb_allreduce_fn)(void* ctx, double* dev_buf, int count, void* stream);

typedef struct {
    int    status;       /* PFB_PCG_* */
    int    iters;        /* k at exit */
    int    matvecs;      /* number of A applications the REFERENCE loop makes (k + 1 unless early exit); small
                          * problems run one iteration ahead of the host's look at eps past minit, so one
                          * further, discarded application may have been executed (PFB_PCG_LOOKAHEAD=0: never) */
    int    backtracks;   /* total backtracking steps taken */
    double eps;          /* last norm_diff(x, xp) */
    double rnorm;        /* last r.y */
} pfb_pcg_result;

/* b, x: (nb, nx, ny).  x holds x0 on entry and the solution on exit (for
 * PFB_PCG_ZERO_RESIDUAL it is left untouched = x0, as the reference returns x0).
 * r_out: optional (nb,nx,ny) residual A x - b on exit (return_resid=True).
 * work: device scratch of pfb_pcg_work_bytes() bytes.
 * pfb_pcg_solve and pfb_pcg_solve_bands below are ONE driver and one set of kernels: a solve works on systems --
 * contiguous runs of bands that share a block of device-resident scalars -- and this entry point is the solve with a
 * single system that spans all nb bands (and, alone, the all-reduce hook and backtrack = 1).  backtrack 0 and 2 read
 * scalars back only once the stopping rule can fire (k >= minit); backtrack = 1 keeps the host-driven loop (scalars
 * read back every iteration).  x and r alternate between the caller's arrays and two copies in `work`.
 * Synchronises `stream` before it returns. */
size_t pfb_pcg_work_bytes(const pfb_conv_plan* plan, int nb);
int pfb_pcg_solve(pfb_conv_plan* plan, int band0, int nb,
                  const void* b, void* x, void* r_out,
                  const void* beam, double wsum, double sigmainv, double mdiv,
                  double tol, int maxit, int minit, int backtrack,
                  void* work, pfb_allreduce_fn allreduce, void* allreduce_ctx,
                  pfb_pcg_result* result, void* stream);

/* ------------------------------------------------------------ batched per-band PCG
 * pcg_psf (pfb/opt/pcg.py:243-360): every band of [band0, band0+nb) is its OWN system, solved as in
 * pfb_pcg_solve with nb = 1 -- its own step lengths, backtracking, stopping rule and exit status -- but all
 * bands in one solve (pfb_pcg_solve's driver with nb systems instead of one): one convolution launch group per
 * iteration over the bands still active, per-band scalars on the device, and the host looks only once some band
 * can stop (k >= minit), and then only at whether any band is still active.  Band bl's result equals
 * pfb_pcg_solve's on that band alone up to the order of the fp64 reductions (every band's convolution output is
 * bit-identical to that solve's, except on the plain-kernel paths, which both share).
 *   - a band whose initial residual is zero keeps x = x0 and gets PFB_PCG_ZERO_RESIDUAL; the others solve;
 *   - breakdown (all-zero direction) ends that band before k += 1, as pcg.py:106-107;
 *   - once a band has stopped, its x and r are never written again (iterations the host enqueued ahead of
 *     its look change nothing there).
 * backtrack: 0 or 2 (predictive); 1 (the exact loop) returns PFB_ERR_UNSUPPORTED -- solve band by band with
 * pfb_pcg_solve for it.  No all-reduce hook: the bands are independent; shard them over GPUs and run one
 * batched solve per rank.
 * Convolution: at every host look the convolved range narrows to the span of bands still live; a stopped band
 * between two live ones is still convolved (its result is discarded), so bands that need very different
 * iteration counts can cost more convolution work than a band-by-band loop.
 * Memory: work holds r, p and Ap of ALL nb bands at once (3 nb nx ny elements + per-band state), where a
 * band-by-band loop of pfb_pcg_solve holds 5 vectors of one band; here x and r are updated in place.
 * results: nb entries.  Synchronises `stream`. */
size_t pfb_pcg_bands_work_bytes(const pfb_conv_plan* plan, int nb);
int pfb_pcg_solve_bands(pfb_conv_plan* plan, int band0, int nb,
                        const void* b, void* x, void* r_out,
                        const void* beam, double wsum, double sigmainv, double mdiv,
                        double tol, int maxit, int minit, int backtrack,
                        void* work, pfb_pcg_result* results, void* stream);

/* ------------------------------------- band-coupled Hessian of the parametrised forward step
 * pfb/workers/fwdbwd.py:246-252 with the parametrisations of pfb/utils/misc.py:1366-1423:
 *
 *   hesspsf(v) = 2 dhf(psf_convolve(df(v))) + sigmainv v,  df(v) = e * (L v),  dhf(w) = L^T (e * w),
 *   e = exp(L x0) (mode 'exp') or 1 (mode 'id': e = NULL)
 *              = L^T [ e * conv(e * (L v)) / wsum ] + sigmainv v      with wsum = 0.5 (the factor 2 is exact)
 *
 * i.e. a band mix, pfb_psfconv_apply(beam = e, wsum = 0.5, sigmainv = 0), and a second band mix that adds the
 * Tikhonov term and, on request, emits the three fp64 sums of the PCG.
 *
 * pfb_bandmix_dots (fwdbwd.py:246-252, misc.py:1366-1423): out[k] = sum_l A[k, l] c[l] + sigmainv p[k] on (nband, npix)
 * arrays, A a device nband x nband matrix, the sum in the arrays' dtype with l ascending (misc.py:1366-1375's order).
 * dots3 (device, 3 doubles; needs p and the scratch ws of PFB_REDUCE_WS_DOUBLES): <p, out>, <r, out> (0 if r is
 * NULL), <out, out>, fp64 in a fixed order.  With p, r and dots3 NULL and sigmainv = 0 it is the plain mix.  out may
 * alias c (not p or r).  nband > 16: PFB_ERR_UNSUPPORTED (pfb_freqmul serves up to 64 bands). */
int pfb_bandmix_dots(int dtype, const void* A, const void* c, int nband, size_t npix, double sigmainv,
                     const void* p, const void* r, void* out, double* dots3, double* ws, void* stream);

/* pfb_hessparam_apply (fwdbwd.py:246-252, misc.py:1366-1423): out = hesspsf(x) over ALL bands of the plan.  L, LH:
 * device nband x nband arrays of the plan's real dtype (LH = L^T); e: NULL or an (nband, nx, ny) cube; x, out:
 * (nband, nx, ny), distinct.  work: pfb_hessparam_work_bytes() bytes of device scratch, 256-byte aligned.
 * nband > 16: PFB_ERR_UNSUPPORTED.  Asynchronous on `stream`.
 * pfb_hessparam_apply_dots: the same with dots_out[0] = <dot_with, out>, [1] = <dot_with2, out> (0 if NULL),
 * [2] = <out, out>; dot_with must be x itself (what the PCG and the power method form), else PFB_ERR_UNSUPPORTED. */
size_t pfb_hessparam_work_bytes(const pfb_conv_plan* plan);
int pfb_hessparam_apply(pfb_conv_plan* plan, const void* L, const void* LH, const void* e, double sigmainv,
                        const void* x, void* out, void* work, void* stream);
int pfb_hessparam_apply_dots(pfb_conv_plan* plan, const void* L, const void* LH, const void* e, double sigmainv,
                             const void* x, void* out, const void* dot_with, const void* dot_with2,
                             double* dots_out, void* work, void* stream);

/* pfb_pcg_solve_param (fwdbwd.py:246-252 and :327-334, misc.py:1366-1423): pfb_pcg_solve's driver and kernels with
 * A = hesspsf as the operator step: ONE system over all nb = plan nband bands (the mix couples every band, so there is
 * no band range and no all-reduce hook: a band shard cannot apply it).  Per iteration: mix, the three convolution
 * kernels, mix with the three sums, one scalar launch, the fused vector update.  b, x, r_out, mdiv, tol, maxit,
 * minit, backtrack (0, 1, 2), result: as pfb_pcg_solve.  work: pfb_pcg_param_work_bytes() bytes (pfb_pcg_work_bytes
 * plus one cube and the mix's partial sums).  Synchronises `stream`. */
size_t pfb_pcg_param_work_bytes(const pfb_conv_plan* plan, int nb);
int pfb_pcg_solve_param(pfb_conv_plan* plan, int nb, const void* L, const void* LH, const void* e,
                        const void* b, void* x, void* r_out, double sigmainv, double mdiv,
                        double tol, int maxit, int minit, int backtrack,
                        void* work, pfb_pcg_result* result, void* stream);

/* ------------------------------------------------ band-shard exchange (RCCL, called from C)
 * The reference sums the CG inner products over ALL bands inside one process
 * (pfb/opt/pcg.py:92-107 on (nband, nx, ny) arrays); with one process per GPU and the bands sharded
 * (pfb/opt/pcg.py:320-356 is the reference's per-band parallelism) those sums need one all-reduce
 * of 3..7 doubles per iteration.  pfb_comm_allreduce is a ready-made pfb_allreduce_fn (ctx = the
 * communicator): an RCCL all-reduce enqueued on the solver's own stream, nothing on the host per
 * iteration.  RCCL is bound at run time (the copy already loaded in the process -- PyTorch's --
 * else librccl.so.1; pfb_comm_bind names one explicitly); single-GPU callers never load it.
 *
 *   rank 0: pfb_comm_unique_id(id)  -> ship the 128 bytes to every rank (any channel)
 *   all   : pfb_comm_init(rank, nranks, id, &comm)   collective, binds to the CURRENT device
 *           pfb_pcg_solve(..., pfb_comm_allreduce, comm, ...)
 *           pfb_comm_destroy(comm)
 */
#define PFB_COMM_ID_BYTES 128
typedef struct pfb_comm pfb_comm;
int pfb_comm_bind(const char* librccl_path);            /* optional; NULL = default search */
int pfb_comm_unique_id(void* id128);
int pfb_comm_init(int rank, int nranks, const void* id128, pfb_comm** out);
int pfb_comm_destroy(pfb_comm* comm);
int pfb_comm_info(const pfb_comm* comm, int* rank, int* nranks, int* device, int* rccl_version);
int pfb_comm_allreduce(void* comm, double* dev_buf, int count, void* stream);   /* incl. the probe / abort protocol */
/* asynchronous state of the communicator (ncclCommGetAsyncError): PFB_OK, or PFB_ERR_COMM once a collective on it
 * has failed or it was aborted */
int pfb_comm_check(pfb_comm* comm);
/* ncclCommAbort: frees the communicator's resources and makes every collective still queued on it, here AND on the
 * peers, complete with an error instead of blocking; the handle stays valid for pfb_comm_destroy only */
int pfb_comm_abort(pfb_comm* comm);

/* ----------------------------------------------------------- wavelets / prox / PD
 * Replaces pfb/wavelets/wavelets.py:175-213 (dwt2d), :261-315 (idwt2d) and
 * pfb/operators/psi.py:187-256 (psi_band.dot / hdot) over all (band, basis) pairs.
 * Coefficient cube layout identical to the reference: (nband, nbasis, Nymax, Nxmax),
 * each basis block transposed (y-major) in [0:Ntoty, 0:Ntotx]; cells outside the
 * union of level blocks are neither written by dot nor read by hdot.
 */
typedef struct pfb_psi_plan pfb_psi_plan;

/* basis_k[i] = 0 for 'self', K for 'dbK' (1..9).  filters: nbasis*4*18 doubles,
 * [basis][dec_lo,dec_hi,rec_lo,rec_hi][tap] (unused taps 0), the table PyWavelets
 * would supply (psi.py:37-43). */
int pfb_psi_plan_create(int nband, int nx, int ny, int nbasis, const int* basis_k,
                        const double* filters, int nlevel, int dtype,
                        pfb_psi_plan** plan);
int pfb_psi_plan_destroy(pfb_psi_plan* plan);
int pfb_psi_plan_dims(const pfb_psi_plan* plan, int* nymax, int* nxmax);
/* analysis  psi.py:187-218 : x (nband,nx,ny) -> alpha (nband,nbasis,Nymax,Nxmax) */
int pfb_psi_dot(pfb_psi_plan* plan, const void* x, void* alpha, void* stream);
/* synthesis psi.py:221-256 : alpha -> xo (nband,nx,ny), summed over bases */
int pfb_psi_hdot(pfb_psi_plan* plan, const void* alpha, void* xo, void* stream);

/* pfb/prox/prox_21m.py:76-103 dual_update_numba, in place on v.
 * vp, v: (nband, nbasis, nymax, nxmax); weight: (nbasis, nymax, nxmax).
 * If vp_out != NULL it additionally receives 2*v_new - vp (primal_dual.py:137); vp_out may alias vp (here and in
 * pfb_dual_apply[_chunk]).  No other two arrays may overlap.  Pointers of any element alignment and any nper are
 * accepted; 16-byte aligned arrays with nper a multiple of 16 / sizeof(T) and nband <= 8 take the 16-byte kernels. */
int pfb_dual_update(int dtype, const void* vp, void* v, const void* weight,
                    double lam, double sigma, int nband, size_t nper,
                    void* vp_out, void* stream);
/* The same update with the bands sharded over GPUs: pfb_dual_bandsum writes the
 * LOCAL band sum of vtilde = vp + sigma v into sum_out (nper values); the caller all-reduces
 * that plane (RCCL, bandwidth bound) and pfb_dual_apply finishes with the GLOBAL sum. */
int pfb_dual_bandsum(int dtype, const void* vp, const void* v, double sigma, int nband,
                     size_t nper, void* sum_out, void* stream);
int pfb_dual_apply(int dtype, const void* vp, void* v, const void* weight, const void* sum_in,
                   double lam, double sigma, int nband, size_t nper, void* vp_out, void* stream);
/* The same two steps on a CHUNK of the coefficient plane, so that the exchange of one chunk (reduce-scatter +
 * all-gather over xGMI) overlaps the band sums / threshold of its neighbours: every pointer is pre-offset to the
 * chunk's first coefficient, `count` coefficients are processed, bands of vp / v / vp_out are `band_stride`
 * elements apart (the full plane's nper), weight / sum are the chunk's slices. */
int pfb_dual_bandsum_chunk(int dtype, const void* vp, const void* v, double sigma, int nband, size_t count,
                           size_t band_stride, void* sum_out, void* stream);
int pfb_dual_apply_chunk(int dtype, const void* vp, void* v, const void* weight, const void* sum_in,
                         double lam, double sigma, int nband, size_t count, size_t band_stride,
                         void* vp_out, void* stream);

/* The band-l2-NORM variants (pfb/prox/prox_21.py; the "m" functions threshold |sum over bands|, these the Euclidean norm
 * over bands).  pfb_prox_21: prox_21_numba (prox_21.py:23-48) -- and, with sigma = 1, the array form prox_21 (:5-20);
 * pfb_dual_update_l2: dual_update_numba of the same file (:62-88), in place on v.  Shapes as for the "m" forms. */
int pfb_prox_21(int dtype, const void* v, void* result, const void* weight,
                double lam, double sigma, int nband, size_t nper, void* stream);
int pfb_dual_update_l2(int dtype, const void* vp, void* v, const void* weight,
                       double lam, double sigma, int nband, size_t nper, void* stream);
/* pfb/prox/prox_21m.py:31-61 prox_21m_numba */
int pfb_prox_21m(int dtype, const void* v, void* result, const void* weight,
                 double lam, double sigma, int nband, size_t nper, void* stream);
/* primal_dual.py:140-146: x = xp - tau*(xout + g); positivity 0|1|2 over nband; g may be NULL (no gradient term).
 * sums[0..1] receive the norm_diff partial sums of (x, xp); sums[2] is zero if and only if x is identically zero (it
 * counts the non-zero elements, a NaN included: test it against 0, like np.any).  ws: PFB_REDUCE_WS_DOUBLES doubles.
 * x must not alias xp, xout, xout_prev, g or gsub (the kernel reads them as non-overlapping with what it writes). */
int pfb_pd_primal_update(int dtype, const void* xp, const void* xout, const void* g,
                         double tau, int positivity, int nband, size_t npix,
                         void* x, double* sums, double* ws, void* stream);
/* The same statement with two fusions (either pointer may be NULL):
 *   xout_prev: the synthesis term is 2*xout - xout_prev.  psi^H is linear, so psi^H(2 v - vp) of
 *              primal_dual.py:137-138 equals 2 psi^H(v) - psi^H(vp), and psi^H(vp) is the previous iteration's
 *              psi^H(v): the caller synthesises v itself and the cube 2 v - vp is never written nor read;
 *   gsub:      the gradient is g - gsub (grad(x) = conv(x) - dirty, workers/spotless.py:259-260: the data term is
 *              subtracted here instead of in a pass of its own). */
int pfb_pd_primal_update2(int dtype, const void* xp, const void* xout, const void* xout_prev, const void* g,
                          const void* gsub, double tau, int positivity, int nband, size_t npix,
                          void* x, double* sums, double* ws, void* stream);

/* ------------------------------------------------------------ Clark CLEAN sub-minor loop
 * pfb/deconv/clark.py:29-84 (subminor + subtract).  A: (nband, nact) active-set values, updated
 * in place; Ip, Iq: (nact) int32 pixel indices of the active set; psf: (nband, nx_psf, ny_psf);
 * model: (nband, nx, ny), receives gamma * component / wsums[band] at the chosen pixel for bands
 * with wsums > 0; loop `while |sum_b A[b, pq]| > th and k < maxit` with pq the FIRST arg-max of
 * (sum_b A)^2 like numpy.  The whole loop runs in one resident workgroup (no per-iteration
 * launch); *iters_out (device int, may be NULL) receives the number of components taken.
 * Needs nx_psf/2 >= nx - 1 and ny_psf/2 >= ny - 1 (the reference's overlap mask is then all
 * true; for smaller PSFs the reference mis-indexes its shrunken active set), nband <= 64. */
int pfb_clark_subminor(int dtype, void* A, size_t nact, int nband, const void* psf, int nx_psf,
                       int ny_psf, const int* Ip, const int* Iq, void* model, int nx, int ny,
                       const void* wsums, double gamma, double th, int maxit, int* iters_out,
                       void* stream);

/* Hogbom CLEAN, pfb/deconv/hogbom.py:8-74.  IR (nband, nx, ny): on entry the dirty cube, on exit the
 * residual; model (nband, nx, ny): zero on entry, receives the components; wsums (nband) = per-band PSF
 * peak (hogbom.py:27), all > 0.  Loop `while IRmax > max(pf * IRmax0, threshold) and k < maxit`, peak =
 * FIRST arg-max of (sum_b IR)^2.  work: device scratch of at least 17 KiB (loop state, arg-max partials).
 * Synchronous (the host looks at the loop state every 64 iterations); *k_out / *irmax_out are HOST
 * outputs.  The PSF must cover every shift: nx_psf/2 >= nx - 1, ny_psf/2 >= ny - 1. */
int pfb_hogbom(int dtype, void* IR, const void* psf, void* model, const void* wsums, int nband, int nx,
               int ny, int nx_psf, int ny_psf, double gamma, double pf, double threshold, int maxit,
               void* work, size_t work_bytes, int* k_out, double* irmax_out, void* stream);

/* Band coupling of the fwdbwd parametrisations, pfb/utils/misc.py:1366-1375 (freqmul):
 * out[k, :] = [post[k, :] *] sum_l A[k, l] * ([pre[l, :] *] x[l, :]) over npix pixels; A: (nband, nband)
 * row-major on the device; pre / post (nband, npix) or NULL fuse the elementwise factors of the 'exp'
 * parametrisation (misc.py:1412-1416).  out must not alias x; nband <= 64. */
int pfb_freqmul(int dtype, const void* A, const void* x, void* out, int nband, size_t npix,
                const void* pre, const void* post, void* stream);

/* ------------------------------------------------------- Gaussian restoring beam
 * What pfb/utils/misc.py:186-238 (convolve2gaussres) and pfb/utils/restoration.py:6-57 (restore_image) need besides
 * the PSF convolution above: the convolution kernel.  Plan-time work, all of it in fp64 whatever the image dtype
 * (Gaussian2D returns float64, the kernel spectra are complex128); the truncation test and the quadratic form are
 * evaluated without FMA contraction, so the zero pattern is numpy's.  Asynchronous on `stream`.
 *
 * A parameter set is 4 doubles [a00, a01, a11, extent]: the entries of R^T A R (misc.py:114-120) and
 * (nsigma * Smaj)^2 (misc.py:123); `pars` is a DEVICE array of nset of them.  The value at (x, y) is
 * exp(-2 sqrt(2 ln 2) (a00 x^2 + 2 a01 x y + a11 y^2)) where x^2 + y^2 <= extent, else 0. */

/* Gaussian2D, misc.py:109-138, for nset parameter sets on the same npix coordinates xx, yy in one launch group.
 * out: (nset, npix) doubles, or NULL when only the sums are wanted; sums: nset device doubles (or NULL) that receive
 * the sum of the UNnormalised values, accumulated in a fixed order; normalise != 0 divides out[s] by sums[s]
 * (misc.py:135-136; needs out and sums).  ws: PFB_REDUCE_WS_DOUBLES doubles of scratch. */
int pfb_gauss2d(const double* xx, const double* yy, size_t npix, const double* pars, int nset, int normalise,
                double* out, double* sums, double* ws, void* stream);

/* The zero-padded kernel of misc.py:210-211, np.pad(Gaussian2D(xx, yy, .), ((npad_xl, .), (npad_yl, .))) on the
 * (nx_pad, ny_pad) grid, evaluated straight onto the grid a convolution plan wants, without ever being stored:
 *   out[s, nx_out/2 + dx, ny_out/2 + dy] = kpad_s[(nx_pad/2 + dx) mod nx_pad, (ny_pad/2 + dy) mod ny_pad]
 * xx, yy: (nx, ny) coordinates.  norm: NULL, or nset doubles the values are divided by (the sums of pfb_gauss2d).
 *   clip != 0: only |dx| < nx, |dy| < ny are kept, the offsets a convolution of an (nx, ny) image touches, zero
 *              elsewhere; needs nx_out >= 2 nx - 1, ny_out >= 2 ny - 1.  The circular convolution of misc.py:212-236
 *              on (nx_pad, ny_pad), wrap-around included, then equals the top-left convolution psf.py:11-56 with
 *              this kernel on (nx_out, ny_out) -- the image-space twin of pfb_psfhat_regrid;
 *   clip == 0: (nx_out, ny_out) = (nx_pad, ny_pad): the padded kernel itself.
 * out: (nset, nx_out, ny_out) reals of `dtype`, peak at (nx_out/2, ny_out/2) as pfb_psfconv_set_psf expects. */
int pfb_gauss_kernel_grid(int dtype, const double* xx, const double* yy, int nx, int ny, int npad_xl, int npad_yl,
                          int nx_pad, int ny_pad, const double* pars, const double* norm, int nset, int clip,
                          int nx_out, int ny_out, void* out, void* stream);

/* The same gather (clipped) from an array: kern is (nband, nx_pad, ny_pad) doubles, periodic, its centre at index
 * (cx, cy) -- (0, 0) for the c2r of a kernel spectrum, (nx_pad/2, ny_pad/2) for a padded kernel. */
int pfb_kernel_gather(int dtype, const double* kern, int nband, int nx, int ny, int nx_pad, int ny_pad, int cx, int cy,
                      int nx_out, int ny_out, void* out, void* stream);

/* misc.py:229-231: out[b, i] = |den[b, i]| > 0 ? num[i] / den[b, i] : 0 over n complex128 values per band, num
 * shared by the bands.  The test is exactly |den| > 0, not a threshold: where the initial kernel's spectrum has
 * decayed to rounding noise the quotient is noise over noise, in the reference as here. */
int pfb_kernhat_ratio(const void* num, const void* den, int nband, size_t n, void* out, void* stream);

/* ----------------------------------------------------------------- component model
 * What pfb/utils/misc.py:1084-1313 (fit_image_cube, eval_coeffs_to_cube, eval_coeffs_to_slice) do on image-sized
 * arrays.  The host keeps what is tiny: the design matrix Xfit and its strings (misc.py:1146-1202), the LU factors of
 * Xfit^T diag(w) Xfit (misc.py:1206-1211), the basis values of the parsed expression (misc.py:1223-1233) and the 1-D
 * coordinate arrays of the regrid (misc.py:1254-1294).  All arithmetic is fp64 whatever the image dtype; nothing is
 * allocated, there is no plan and no global state; asynchronous on `stream`.
 *
 * The fit is three calls.  `work` is device scratch of pfb_comps_work_bytes(npix) bytes, 8-byte aligned: the bit mask
 * (one 64-bit word per 64 pixels), the scanned per-workgroup counts and, in its LAST 8 bytes, the number of
 * components as an int64.  The caller reads that one number between pfb_comps_mask and pfb_comps_compact to size
 * Ix / Iy / coeffs -- the only synchronisation of the fit (the output shape depends on the data). */

/* Bytes of `work` for a cube of npix pixels per plane; 0 when npix is out of range. */
size_t pfb_comps_work_bytes(size_t npix);

/* misc.py:1131: np.any(image, axis=(0, 1)) of an (nplane, npix) cube of `dtype` as a bit mask -- a pixel is set iff
 * any plane value != 0, so a NaN counts and -0.0 does not -- then the scan of the counts.  One pass over the cube,
 * 16-byte loads; planes that do not start on a 16-byte boundary (odd npix in fp32) are read from their first aligned
 * vector on, with a peel of up to 3 pixels. */
int pfb_comps_mask(int dtype, const void* image, int nplane, size_t npix, void* work, void* stream);

/* misc.py:1132: Ix, Iy = np.where(mask) for the (npix / ny, ny) mask in `work`, in np.where's row-major order.
 * Ix, Iy: device int64 arrays of (at least) the component count. */
int pfb_comps_compact(size_t npix, int ny, const void* work, long long* Ix, long long* Iy, void* stream);

/* misc.py:1136, 1206-1211: coeffs[:, c] = solve(H, (Xfit^T diag(w)) image[:, Ix[c], Iy[c]]), one component per lane.
 * sys: device doubles [A (nparam, nrow) | LU (nparam, nparam) | piv (nparam)], A = Xfit^T diag(w), LU / piv the getrf
 * factors of H (scipy.linalg.lu_factor; piv stored as doubles).  image: (nrow, npix) of `dtype`; coeffs:
 * (nparam, ncomps) doubles.  A NaN in a component's pixel gives NaN coefficients for that component only.
 * nrow <= 64 and nparam <= 32, else PFB_ERR_UNSUPPORTED. */
int pfb_comps_fit(int dtype, const void* image, int nrow, size_t npix, int ny, const long long* Ix, const long long* Iy,
                  long long ncomps, const double* sys, int nparam, double* coeffs, void* stream);

/* misc.py:1222-1233 / :1243-1252: out (nplane, nx, ny) of `dtype` is zero-filled, then
 * out[plane, Ix[c], Iy[c]] = sum_p E[plane, p] coeffs[p, c], accumulated in fp64.  E: (nplane, nparam) device doubles,
 * the value of expr's factor of parameter p at plane's (t, f).  The (Ix, Iy) pairs must be UNIQUE (numpy's
 * last-one-wins for duplicates is not reproduced); a pair outside the plane is skipped.  nplane <= 65535. */
int pfb_comps_eval(int dtype, const double* E, int nplane, int nparam, const double* coeffs, const long long* Ix,
                   const long long* Iy, long long ncomps, int nx, int ny, void* out, void* stream);

/* misc.py:1302-1306: RegularGridInterpolator((xin, yin), np.pad(image, ...), method='linear') at meshgrid(xo, yo).
 * image: (nxi, nyi) device doubles; the padded plane is virtual: padded index (a, b) is image[a - npad_xl, b - npad_yl]
 * and 0 outside it.  xin (nx_pad), yin (ny_pad), xo (nxo), yo (nyo): device doubles, computed by the caller with the
 * reference's expressions and used as they are (the kernel never recomputes index * cell + x0); xin, yin ascending.
 * Interval np.searchsorted(grid, x) - 1 clipped to [0, n - 2], distance (x - grid[i]) / (grid[i+1] - grid[i]), sum of
 * the four corner products; no bounds check (the caller's, misc.py:1304).  out: (nxo, nyo) of `dtype`. */
int pfb_comps_interp(int dtype, const double* image, int nxi, int nyi, int npad_xl, int npad_yl, const double* xin,
                     int nx_pad, const double* yin, int ny_pad, const double* xo, int nxo, const double* yo, int nyo,
                     void* out, void* stream);

/* ------------------------------------------------------------------ spectral index
 * What pfb/utils/spi.py:18-70 (fit_spi) does on image-sized arrays, and the per-component fit it hands to
 * fit_spi_components: the model m_b = I0 B_b x_b^alpha, x_b = freqs_b / ref_freq, fitted to the data d_b with band
 * weights w_b by Gauss-Newton from alpha = -0.7, I0 = d[ref]:
 *   j1_b = B_b exp(alpha ln x_b), j0_b = I0 j1_b ln x_b, r_b = d_b - I0 j1_b,
 *   h00 = sum w j0^2, h01 = sum w j0 j1, h11 = sum w j1^2, g0 = sum w j0 r, g1 = sum w j1 r, det = h00 h11 - h01^2,
 *   alpha += (h11 g0 - h01 g1) / det, I0 += (-h01 g0 + h00 g1) / det, eps = max(|d alpha|, |d I0|),
 * while eps > tol and fewer than maxiter steps were taken (eps starts at 1).  The errors are taken at the returned
 * parameters: alpha_err = sqrt(h11 / det chi2 / dof), I0_err = sqrt(h00 / det chi2 / dof), chi2 = sum w r^2,
 * dof = max(nband - 2, 1).  A det that is 0 or not finite, in a step or at the end, gives NaN in all four outputs of
 * that component only.  A component that takes maxiter steps returns its last iterate and is counted in *notconv.
 * All arithmetic is fp64 whatever the image dtype, the band sums run in ascending order.
 *
 * The host keeps what is tiny: ln x_b and w_b (HOST arrays of nband doubles, copied into the kernel arguments at the
 * call) and ref = argmin |freqs - ref_freq|.  Two numbers cross to the host: the component count between pfb_spi_mask
 * and pfb_comps_compact (it sizes Ix / Iy and decides fit_spi's ValueError), and *notconv after the fit (it decides the
 * warning).  Nothing is allocated, there is no plan and no global state; asynchronous on `stream`.  nband <= 64, else
 * PFB_ERR_UNSUPPORTED.
 *
 * `work` is device scratch of pfb_spi_work_bytes(npix) bytes, 8-byte aligned.  It BEGINS with the layout of
 * pfb_comps_mask -- pfb_comps_work_bytes(npix) bytes: the bit mask, the scanned per-workgroup counts and, in the last 8
 * of them, the component count as an int64 -- so that pfb_comps_compact(npix, ny, work, Ix, Iy) yields the components
 * in np.argwhere's order.  Behind it: the partial maxima of the pass and, in the LAST 8 bytes of `work`, image.max()
 * after the beam cut as a double, NaN-propagating (spi.py:39; read only to word the ValueError). */

/* Bytes of `work` for cubes of npix pixels per plane; 0 when npix is out of range. */
size_t pfb_spi_work_bytes(size_t npix);

/* spi.py:29-35: one pass over image and beam, both (nband, npix) of `dtype`.  Per value c = beam > pb_min ? image : 0 (a
 * NaN beam fails the comparison); a pixel is set iff every band's c > threshold (a NaN c fails, as np.amin propagates
 * it).  The comparisons are made on the exact fp64 values of the inputs.  16-byte loads; planes that do not start on a
 * 16-byte boundary (odd npix in fp32) are read from their first aligned vector on, with a peel of up to 3 pixels. */
int pfb_spi_mask(int dtype, const void* image, const void* beam, int nband, size_t npix, double pb_min, double threshold,
                 void* work, void* stream);

/* spi.py:40-68: the fit of component c at pixel q = Ix[c] * ny + Iy[c], one component per lane.  Its data are the cut
 * values c_b of pfb_spi_mask, its beam values the raw beam[b, q].  maps: (4, npix) of `dtype` -- alpha, alpha_err, I0,
 * I0_err -- written at the components only (the caller fills it with NaN first).  The 2 nband inputs of a component
 * are re-read on every step.  ncomps <= npix; notconv: one device int64, cleared and then counted into. */
int pfb_spi_fit(int dtype, const void* image, const void* beam, int nband, size_t npix, int ny, const long long* Ix,
                const long long* Iy, long long ncomps, const double* lnx, const double* w, int ref, double pb_min,
                double tol, int maxiter, void* maps, long long* notconv, void* stream);

/* The same fit of a dense component list.  data: (ncomps, nband) device doubles; beam: the same shape, or NULL for 1;
 * alphai, I0i: (ncomps) device doubles that replace the starting values, or NULL; out: (4, ncomps) device doubles. */
int pfb_spi_fit_components(const double* data, const double* beam, int nband, long long ncomps, const double* lnx,
                           const double* w, int ref, const double* alphai, const double* I0i, double tol, int maxiter,
                           double* out, long long* notconv, void* stream);

/* ----------------------------------------------------------------------- clean beam
 * What pfb/utils/misc.py:506-584 (psf_errorsq, fitcleanbeam) do on image-sized arrays.  The host keeps the optimiser
 * (scipy's fmin_l_bfgs_b, misc.py:577-581) and calls pfb_beamfit_objective from its callback.  All fit arithmetic is
 * fp64 whatever the PSF dtype; nothing is allocated, there is no plan and no global state; asynchronous on `stream`.
 *
 * `work` is device scratch of pfb_beamfit_work_bytes(nband, npix) bytes, 8-byte aligned.  It BEGINS with one record of
 * PFB_BEAMFIT_RECORD doubles per band, the only thing the host reads:
 *   [0] max          psf[v].max(), NaN-propagating (misc.py:552)
 *   [1] any          1.0 iff psf[v].any() (misc.py:549); everything behind it is 0 when it is 0
 *   [2] centre_above 1.0 iff psf[v, nx//2, ny//2] / max > level; everything behind it is 0 when it is 0
 *   [3..6]           x.min(), x.max(), y.min(), y.max() over the centre island (misc.py:561-564)
 *   [7], [8]         np.abs(x).max(), np.abs(y).max() (misc.py:565)
 *   [9]              pixels of the centre island
 *   [10]             pixels of the fit region rrsq < extent * rsq (misc.py:566-567)
 *   [11]             extent * rsq
 * Behind the records: the partial maxima of the streaming pass and per band a visited bit mask, one 64-bit word per
 * 64 pixels. */
#define PFB_BEAMFIT_RECORD 16

/* Bytes of `work`; 0 when nband (1 .. 65535) or npix (1 .. 2^40) is out of range. */
size_t pfb_beamfit_work_bytes(int nband, size_t npix);

/* misc.py:549, 552: per band of the (nband, npix) cube of `dtype` the maximum (a NaN anywhere gives NaN, like
 * ndarray.max) and np.any (a NaN counts, -0.0 does not) into record [0], [1]; the rest of the record and the band's
 * visited mask are cleared.  One pass over the cube, the only one of the fit; 16-byte loads, a plane that does not
 * start on a 16-byte boundary (odd npix in fp32) is read from its first aligned vector on with a peel of up to 3
 * elements at either end.  The partials are combined in a fixed order. */
int pfb_beamfit_max(int dtype, const void* psf, int nband, size_t npix, void* work, void* stream);

/* misc.py:552-567, all bands in one launch: the island of `psf[v] / max > level` that holds (nx // 2, ny // 2) under
 * 8-connectivity (skimage.morphology.label's default in 2-D), grown from that pixel until a sweep adds nothing, and
 * from it record [2..11].  The quotient is formed in `dtype` and compared in `dtype` with `level` rounded to it
 * (NumPy 2), strictly.  Coordinates are x_i = -nx / 2 + i, y_j = -ny / 2 + j (misc.py:542-543).  The fit region is
 * counted inside the square of half-side ceil(sqrt(extent * rsq)) around the centre, never over the plane.
 * To follow pfb_beamfit_max on the same `work` (it needs the cleared mask), once. */
int pfb_beamfit_lobe(int dtype, const void* psf, int nband, int nx, int ny, double level, double extent, void* work,
                     void* stream);

/* misc.py:506-526 and its gradient for band `band` of the cube at x = (emaj, emin, pa): out[0] = f =
 * sum_i (d_i - exp(-2 sqrt(2 ln 2) Q_i))^2 over the fit region of the band's record, out[1..3] = df/d(emaj, emin, pa);
 * out: 4 device doubles.  d_i = psf / max in `dtype`, then fp64; Q = xy^T R^T diag(1/Smin^2, 1/Smaj^2) R xy with
 * Smin = min(emaj, emin), Smaj = max(emaj, emin) and R the rotation by deg2rad(-pa), whose cosine and sine are taken on
 * the host.  The derivatives are analytic, through Smin and Smaj; at emaj == emin each of the two gets the mean of
 * the Smin and the Smaj derivative, which is what jax's documentation states for minimum / maximum at a tie (taken
 * from the documentation, not verified against jax).  emin = 0 gives non-finite values as in the reference.  Sums in a
 * fixed order. */
int pfb_beamfit_objective(int dtype, const void* psf, int band, int nx, int ny, double emaj, double emin, double pa,
                          const void* work, double* out, void* stream);

/* ------------------------------------------------------------------ major-cycle statistics
 * What the workers' major-cycle loops do inline between the solver calls (workers/klean.py:190-339, spotless.py:155-363,
 * fluxmop.py:129-199, fwdbwd.py:233, 423): the band sum of a cube with its statistics, the mop mask and the masked
 * system of the flux mop.  fp32 and fp64; nothing is allocated, there is no plan and no global state; asynchronous on
 * `stream`.  16-byte loads when every plane starts on a 16-byte boundary (npix a multiple of 4 resp. 2 elements and
 * aligned bases); otherwise (odd npix in fp32, a base offset by 1-3 elements) the same kernels run one element per
 * lane.  Masks are unsigned char planes, 0 = out, anything else = in; the ones written here hold 0 or 1.  No output may
 * overlap an input or another output (sum_out a band of x, b the residual, x0 the seed, ...): the kernels are not
 * written for in-place use and nothing checks it beyond `out != mask` in pfb_mask_close. */

/* Doubles per set of the record pfb_bandsum_stats writes: [count, mean, M2, absmax]. */
#define PFB_CYCLE_RECORD 4

/* Bytes of the `work` buffer of pfb_bandsum_stats (the workgroups' partial records) for nset sets; host only; 0 when
 * nset (1 .. 65535) is out of range. */
size_t pfb_cycle_work_bytes(int nset);

/* np.sum(x, axis=0) with np.std and np.abs().max() of the result, in one pass.
 * x: (nband, nset, npix) of `dtype` -- a residual cube has nset = 1, a coefficient cube nset = nbasis and npix =
 *   Nymax * Nxmax.  Per pixel s = x[0] + x[1] + ... in `dtype`, in band order (numpy's order: the bits of np.sum).
 * model: NULL, or (nband_m, npix) of `dtype`, allowed with nset == 1 only.  A pixel is quiet iff every model band is
 *   == 0 there (a NaN makes it not quiet, -0.0 does not: ~np.any(model, axis=0)); without a model every pixel is quiet.
 * sum_out: NULL, or (nset, npix) of `dtype`, receives s.
 * work: device scratch of pfb_cycle_work_bytes(nset) bytes, 8-byte aligned.
 * out: nset records of PFB_CYCLE_RECORD device doubles:
 *   [0] count   quiet pixels of the set
 *   [1] mean    of s over them, fp64 (0 when count == 0)
 *   [2] M2      sum (s - mean)^2 over them, fp64: np.std = sqrt(M2 / count), nan for count == 0 as in numpy
 *   [3] absmax  max |s| over ALL pixels of the set, a NaN anywhere gives NaN (ndarray.max)
 * The moments are accumulated about a pivot from the data and merged pairwise (M2 = M2a + M2b + d^2 na nb / (na + nb)),
 * never as sum x, sum x^2: |mean| >> std does not cancel.  Fixed combination order: identical bits from run to run.  No
 * floating-point atomics; the merge of the workgroups' partials is a second, one-wave-per-set launch. */
int pfb_bandsum_stats(int dtype, const void* x, int nband, int nset, size_t npix, const void* model, int nband_m,
                      void* sum_out, void* work, double* out, void* stream);

/* klean.py:301-305 / fluxmop.py:129: a support and its binary closing.
 * Exactly one of `cube` and `mask` is non-NULL:
 *   cube: (nband, nx, ny) of `dtype`; the support is any(v != 0) over the bands (a NaN counts, -0.0 does not), or
 *         any(v > min_value) when has_min != 0, min_value rounded to `dtype` (NumPy 2 for a Python-float bound; a NaN
 *         does not count);
 *   mask: (nx, ny) unsigned char, the support is mask != 0 (`dtype`, nband, has_min, min_value are ignored).
 * connectivity selects the structure of scipy.ndimage.generate_binary_structure(2, c): c <= 0: no closing, out is the
 * support itself (the worker's `if opts.dirosion`); c == 1: the 5-point cross; c >= 2: the full 3 x 3.
 * out: (nx, ny) unsigned char, 0 or 1, not the input mask: one binary_dilation followed by one binary_erosion, outside
 * the image counting as 0 in BOTH (scipy's border_value=0).  A pixel whose structure reaches outside the image is
 * therefore never set, whatever the support: the reference's mop mask loses its border pixels the same way. */
int pfb_mask_close(int dtype, const void* cube, int nband, const unsigned char* mask, int nx, int ny, int has_min,
                   double min_value, int connectivity, unsigned char* out, void* stream);

/* klean.py:306-317 / fluxmop.py:166-199: the masked system in one pass.
 * residual: (nband, npix) of `dtype` (may be NULL when b is); mask: (npix) unsigned char.
 * beam: NULL, or (nband_beam, npix) of `dtype` with nband_beam == nband or 1; seed: NULL, or one (npix) plane.
 * Outputs, each may be NULL:
 *   beam_eff (nband_beam, npix), or (1, npix) without a beam: beam * mask resp. the mask as 0 / 1 of `dtype`;
 *   b (nband, npix) = beam_eff * residual, the product formed in `dtype` in this order: a NaN residual outside the mask
 *     stays NaN, as in numpy;
 *   x0 (nband, npix) = mask ? seed : 0, zeros without a seed. */
int pfb_masked_problem(int dtype, const void* residual, const unsigned char* mask, const void* beam, int nband_beam,
                       const void* seed, int nband, size_t npix, void* b, void* x0, void* beam_eff, void* stream);

/* ------------------------------------------------------------------------- w-gridder
 * pfb/operators/hessian.py:62-106 (_hessian_impl): ducc0's dirty2vis and vis2dirty, defined by the direct Fourier sums
 *   (u, v, w) = uvw[r] * freq[k] / 299792458,  l_i = (i - nx/2) pixsize_x + center_x,  m_j likewise,
 *   nm1 = -(l^2 + m^2) / (1 + sqrt(1 - l^2 - m^2))   (0 without w-gridding),   phase = u l + v m - w nm1,
 *   vis2dirty: dirty[i,j] = f_ij sum_{mask != 0} Re(wgt vis exp(+2 pi i phase)),
 *   dirty2vis: vis[r,k]   = wgt sum_ij f_ij dirty[i,j] exp(-2 pi i phase), 0 where mask == 0,
 * evaluated by w-stacking on a (2 nx, 2 ny) grid with the kernel exp(2.3 W (sqrt(1 - x^2) - 1)) of `support` = W cells
 * (DESIGN 4.10).  The additive family leaves PFB_ABI_VERSION at 1, like every family added since the first.
 *
 * A plan is a host record of the geometry: it owns no device memory, launches nothing on creation and is immutable, so
 * one plan may serve any number of streams; the single-owner rule applies to the caller's arrays (grid, acc, val, img).
 * The caller owns, as device arrays:
 *   keys   (nrow * nchan) int: the sort key of a visibility, -1 where masked;
 *   work   pfb_wgrid_work_bytes(plan) bytes, 4-byte aligned: the key histogram (nkeys ints, which the caller scans
 *          into `offsets`, nkeys exclusive prefix sums as int64) and the placement cursors behind it;
 *   idx    (nsorted) int: visibility r * nchan + k of a slot;  coord (3, nsorted) double: its position in grid cells
 *          (u pixsize_x 2 nx, v pixsize_y 2 ny) and in planes ((w - w0) / dw);
 *   val / acc (nsorted) complex: what is gridded / what degridding sums, per slot;
 *   grid   (2 nx, 2 ny) complex, one w plane;  img (nx, ny) complex: the sum of the planes' images;
 *   corr   (nx, ny) double: 1 / (c_u(i) c_v(j) c_w(i,j)) [/ n_ij], the kernel correction with divide_by_n folded in;
 *   nm1    (nx, ny) double, or NULL without w-gridding.
 * Plane p lies at w0 + p dw and takes the slots whose first plane is in [p - W + 1, p]: one contiguous range [s0, s1)
 * of the order, which the caller reads off `offsets`.  A slot of the range that does not reach the plane is skipped.
 * Between pfb_wgrid_grid and pfb_wgrid_image_adjoint (pfb_wgrid_image_forward and pfb_wgrid_degrid) the caller
 * transforms the grid: unnormalised c2c, sign + (sign -).  Every function is asynchronous on `stream`.
 *
 * pfb_wgrid_grid accumulates with floating-point atomic adds: its sums depend on arrival order and vis2dirty differs
 * in the last bits from run to run.  dirty2vis uses none and is reproducible bit for bit; pfb_wgrid_grid_tile (below) is
 * the gridding step without atomics. */

/* support: 4 .. 12.  nplanes == 1: one plane at w0 and no w kernel (dw ignored); else nplanes > support, dw > 0.
 * nx, ny even.  PFB_ERR_UNSUPPORTED: a support outside the range, a grid narrower than the support, too many keys. */
int pfb_wgrid_plan_create(int dtype, int nx, int ny, double pixsize_x, double pixsize_y, double center_x,
                          double center_y, int support, int nplanes, double w0, double dw, void** plan);
int pfb_wgrid_plan_destroy(void* plan);
/* nkeys = np0 * (uv tiles); np0 = number of first planes (nplanes - support + 1, or 1); tile: the tile edge in cells.
 * Slots with first plane q occupy [offsets[q * nkeys / np0], offsets[(q + 1) * nkeys / np0]). */
int pfb_wgrid_plan_info(void* plan, int* nkeys, int* np0, int* tile);
/* Bytes of `work`; host only; 0 for a NULL plan. */
size_t pfb_wgrid_work_bytes(void* plan);

/* The order, step 1: keys and their histogram (work is cleared first).  uvw (nrow, 3), freq (nchan) double;
 * mask (nrow, nchan) unsigned char or NULL.  nrow * nchan < 2^31. */
int pfb_wgrid_order_count(void* plan, const double* uvw, const double* freq, const unsigned char* mask, size_t nrow,
                          int nchan, int* keys, void* work, void* stream);
/* Step 2, after the caller's scan: place every unmasked visibility.  nsorted = the histogram's total (>= 1).  The order
 * within one key is the arrival order of the lanes. */
int pfb_wgrid_order_fill(void* plan, const double* uvw, const double* freq, size_t nrow, int nchan, const int* keys,
                         const long long* offsets, void* work, size_t nsorted, int* idx, double* coord, void* stream);

/* val[s] = wgt vis exp(+2 pi i (u center_x + v center_y)); wgt (nrow, nchan) of `dtype`, or NULL for 1. */
int pfb_wgrid_prep(void* plan, const void* vis, const void* wgt, const int* idx, const double* coord, size_t nsorted,
                   void* val, void* stream);
/* vis = 0, then vis[idx[s]] = wgt acc[s] exp(-2 pi i (u center_x + v center_y)); vis holds nvis = nrow * nchan. */
int pfb_wgrid_finish(void* plan, const void* acc, const void* wgt, const int* idx, const double* coord, size_t nsorted,
                     void* vis, size_t nvis, void* stream);
/* The block form of pfb_wgrid_finish, for the predict step (pfb/operators/gridder.py:492-548): `plan` is a plan on a
 * block of rows and channels, (.., nchan_blk) visibilities without a mask, and `out` a (nrow_out, nchan_out, ncorr)
 * complex array of `out_dtype` -- the plan's type, or PFB_F32 under a double-precision plan (the worker's
 * astype(complex64), one rounding).  For slot s, t = idx[s], r = t / nchan_blk, c = t % nchan_blk and
 * v = acc[s] exp(-2 pi i (u center_x + v center_y)) formed as pfb_wgrid_finish forms it:
 *   out[row0 + r, chan0 + c, k] = (out type) v            for k = 0 and k = ncorr - 1,
 *   out[row0 + r, chan0 + c, k] += (out type) v           with accumulate != 0: cast first, then add in the out type.
 * No weight (the reference applies none in this direction), no memset and no other cell written: zeroing is the
 * caller's.  ncorr in 1 .. 4, chan0 + nchan_blk <= nchan_out, every row0 + r inside out (the caller's check: out's
 * extent is not passed).  PFB_ERR_INVALID: a complex128 output under a single-precision plan. */
int pfb_wgrid_finish_block(void* plan, const void* acc, const int* idx, const double* coord, size_t nsorted,
                           int nchan_blk, void* out, int out_dtype, size_t row0, int nchan_out, int chan0, int ncorr,
                           int accumulate, void* stream);
/* pfb/utils/misc.py:498-503 (_restore_corrs): out (nvis, ncorr) complex `dtype`, out[v, 0] = out[v, ncorr - 1] = vis[v]
 * and zero between, every element written by one launch (no memset).  ncorr in 1 .. 4, nvis < 2^31. */
int pfb_vis_restore_corrs(int dtype, const void* vis, size_t nvis, int ncorr, void* out, void* stream);
/* val[s] = wgt acc[s]: degridding handed straight to gridding (the Hessian; the centre phases cancel). */
int pfb_wgrid_weight(void* plan, const void* acc, const void* wgt, const int* idx, size_t nsorted, void* val,
                     void* stream);

/* grid = 0, then the slots [s0, s1) are added to plane `plane`. */
int pfb_wgrid_grid(void* plan, int plane, const void* val, const double* coord, size_t nsorted, size_t s0, size_t s1,
                   void* grid, void* stream);
/* The reproducible mode ("The tile-owned gridder"): pfb_wgrid_grid without atomics.  Every grid cell is
 * summed by one lane in one fixed order, so the grid is identical bit for bit from run to run; each contribution is the
 * value pfb_wgrid_grid adds.  It needs an order of its own and a map of it, both built once by the caller:
 *
 * The order.  pfb_wgrid_order_keys64 writes keys (nrow * nchan) long long: (p0 nfu + a / 16) nfv + b / 16 of a
 * visibility with first plane p0 and first footprint cell (a, b), on FINE tiles of 16 x 16 cells whatever the grid
 * (nfu = ceil(2 nx / 16), nfv = ceil(2 ny / 16)), and 2^63 - 1 where masked.  The caller sorts them STABLY: idx is the
 * permutation's head of nsorted live entries (ascending visibility inside a key), and slots with first plane q occupy
 * [lower_bound(q nfu nfv), lower_bound((q + 1) nfu nfv)) of the sorted keys.  pfb_wgrid_order_coords fills
 * coord (3, nsorted) for that idx, bit for bit what pfb_wgrid_order_fill writes for the same visibility.  Every other
 * function works on this order unchanged.
 *
 * The map, a CSR over the fine tiles that receive anything (device arrays):
 *   tgt_tile (ntgt) int: tile fu nfv + fv, rows 16 fu .., columns 16 fv ..;  tgt_ptr (ntgt + 1) long long, from 0 to npair;
 *   per pair p in [tgt_ptr[t], tgt_ptr[t + 1]): pair_start, pair_count (npair) long long, int -- a run of slots of one
 *   key -- and pair_p0 (npair) int, its first plane.  Inside a target the pairs ascend by (first plane, source tile).
 * A target must list every key whose footprints can reach it: first rows a with (r - a) mod 2 nx < W for a row r of the
 * tile, likewise columns; each key once.  A cell's sum runs over its target's pairs with first plane in
 * [plane - W + 1, plane], in list order, and over each pair's slots ascending.
 *
 * grid = 0, then the plane is summed; one workgroup per target.  The map is checked where it is first presented to a
 * plan -- one small launch and one host read, the only wait in this family -- and remembered by its arrays and counts:
 * the arrays of a map must not change while a plan uses them (the kernel never addresses outside the slots or the grid
 * whatever they hold).  PFB_ERR_INVALID: ntgt or npair of 0 or beyond the tiles, a target outside the tiles, pointers
 * that do not run from 0 to npair, a pair with count < 1, start + count > nsorted or a first plane outside the plan's,
 * first planes that descend inside a target. */
int pfb_wgrid_order_keys64(void* plan, const double* uvw, const double* freq, const unsigned char* mask, size_t nrow,
                           int nchan, long long* keys, void* stream);
int pfb_wgrid_order_coords(void* plan, const double* uvw, const double* freq, size_t nrow, int nchan, const int* idx,
                           size_t nsorted, double* coord, void* stream);
int pfb_wgrid_grid_tile(void* plan, int plane, const void* val, const double* coord, size_t nsorted, const int* tgt_tile,
                        const long long* tgt_ptr, const long long* pair_start, const int* pair_count, const int* pair_p0,
                        size_t ntgt, size_t npair, void* grid, void* stream);
/* acc[s] += the footprint sum of slot s on plane `plane`, s in [s0, s1). */
int pfb_wgrid_degrid(void* plan, int plane, const void* grid, const double* coord, size_t nsorted, size_t s0, size_t s1,
                     void* acc, void* stream);

/* grid = 0, then its centred window = dirty corr [beam] exp(+2 pi i w_p nm1).  beam (nx, ny) of `dtype`, or NULL. */
int pfb_wgrid_image_forward(void* plan, int plane, const void* dirty, const void* beam, const double* corr,
                            const double* nm1, void* grid, void* stream);
/* img += window(grid) exp(-2 pi i w_p nm1). */
int pfb_wgrid_image_adjoint(void* plan, int plane, const void* grid, const double* nm1, void* img, void* stream);
/* dirty = Re(img) corr [beam]. */
int pfb_wgrid_image_correct(void* plan, const void* img, const double* corr, const void* beam, void* dirty, void* stream);

/* The same operators with a product axis ("Several products under one order"): nprod = 1 .. 4 planes --
 * the Stokes products of one chunk -- share the plan and its order, and every array that holds values gains a leading
 * axis, product-major and contiguous:
 *   vis, wgt (nprod, nvis);  val / acc (nprod, nsorted);  grid (nprod, 2 nx, 2 ny);  img, dirty (nprod, nx, ny).
 * idx, coord, corr, nm1 and beam stay single: they do not depend on the product.  wgt is NULL for 1, one (nvis) plane
 * for every product with wgt_shared != 0, else (nprod, nvis).  Per plane each function computes what its single form
 * computes; what does not depend on the values -- a slot's centre phase, a footprint's cells and kernel values, a
 * pixel's w phase, correction and beam -- is formed once and applied to all planes.  The caller transforms the grids
 * between the calls as before (torch.fft batches over the leading axis).  nprod == 1 is the single form.
 * PFB_ERR_INVALID: nprod outside 1 .. 4 (before anything else; nothing is written), and what the single forms refuse.
 * pfb_wgrid_prep_multi takes nvis, the plane stride of vis and wgt: nsorted <= nvis < 2^31. */
int pfb_wgrid_prep_multi(void* plan, int nprod, const void* vis, const void* wgt, int wgt_shared, const int* idx,
                         const double* coord, size_t nsorted, size_t nvis, void* val, void* stream);
int pfb_wgrid_finish_multi(void* plan, int nprod, const void* acc, const void* wgt, int wgt_shared, const int* idx,
                           const double* coord, size_t nsorted, void* vis, size_t nvis, void* stream);
/* every grid = 0, then the slots [s0, s1) of every plane of val are added to `plane` of its grid. */
int pfb_wgrid_grid_multi(void* plan, int nprod, int plane, const void* val, const double* coord, size_t nsorted,
                         size_t s0, size_t s1, void* grid, void* stream);
/* pfb_wgrid_grid_tile on every plane of val: a lane holds the nprod sums of its cell. */
int pfb_wgrid_grid_tile_multi(void* plan, int nprod, int plane, const void* val, const double* coord, size_t nsorted,
                              const int* tgt_tile, const long long* tgt_ptr, const long long* pair_start,
                              const int* pair_count, const int* pair_p0, size_t ntgt, size_t npair, void* grid,
                              void* stream);
int pfb_wgrid_degrid_multi(void* plan, int nprod, int plane, const void* grid, const double* coord, size_t nsorted,
                           size_t s0, size_t s1, void* acc, void* stream);
int pfb_wgrid_image_forward_multi(void* plan, int nprod, int plane, const void* dirty, const void* beam,
                                  const double* corr, const double* nm1, void* grid, void* stream);
int pfb_wgrid_image_adjoint_multi(void* plan, int nprod, int plane, const void* grid, const double* nm1, void* img,
                                  void* stream);
int pfb_wgrid_image_correct_multi(void* plan, int nprod, const void* img, const double* corr, const void* beam,
                                  void* dirty, void* stream);

/* --------------------------------------------------------------------- imaging weights
 * pfb/utils/weighting.py:43-171 (_compute_counts, _counts_to_weights) and the l2reweight_dof block of
 * pfb/operators/gridder.py:604-615.  No plan: every function is one asynchronous launch (behind a clear
 * of what it accumulates into) on `stream`.  `dtype` is the type T of counts and weights; visibilities are complex T.
 * uvw (nrow, 3) and freq (nchan) are double, mask (nrow, nchan) is unsigned char and required; nrow * nchan < 2^31.
 *
 * The grid coordinate of a visibility, in fp64 and with every operation rounded on its own, as the reference writes it:
 *   ug = (uvw[r][0] * (freq[c] / 299792458) + umax) / u_cell,   vg likewise,
 * with u_cell = 1 / (nx cell_size_x) and umax = |-1 / cell_size_x / 2 - u_cell / 2| evaluated by the caller, in this
 * order, in double.  A visibility whose cell (floor ug, floor vg) lies outside [0, nx) x [0, ny), or whose coordinate is
 * not finite, contributes nothing and gets weight 0, and a footprint cell outside the grid is skipped (the reference
 * wraps a negative index and writes past the array at the top): no input addresses outside the arrays.
 *
 * The sums go to device records of PFB_IMW_RECORD doubles and never to the host; no floating-point atomics but in the
 * counts. */
#define PFB_IMW_RECORD 3
/* Doubles of the `work` scratch of the functions that sum (8-byte aligned device memory, the caller's, one per stream in
 * use): one partial per workgroup and quantity, added by a second, one-workgroup launch in a fixed order -- the sums
 * are the same bits from run to run. */
#define PFB_IMW_WORK_DOUBLES 6144

/* counts (ngrid, nx, ny) of `dtype`, cleared first.  Row r adds to grid g of the partition in bins of nrow / ngrid rows,
 * the first nrow % ngrid bins one longer.  k == 0: 1 to cell (floor ug, floor vg) of every visibility with mask != 0.
 * k = 2, 4, .. 16, h = k / 2: phi(x / h) phi(y / h) to the cells (rint ug + i, rint vg + j), i, j in [-h, h), rint
 * rounding halves to even, x = cell - ug + 0.5, phi(t) = exp(2.3 k (sqrt((1 - t)(1 + t)) - 1)); phi and the product in
 * fp64, rounded once to `dtype`.  Floating-point atomic adds: for k > 0 the sums depend on arrival order in the last
 * bits; for k == 0 they are integers and exact (below 2^24 per cell in float). */
int pfb_imw_counts(int dtype, const double* uvw, const double* freq, const unsigned char* mask, size_t nrow, int nchan,
                   int nx, int ny, double u_cell, double umax, double v_cell, double vmax, int k, int ngrid, void* counts,
                   void* stream);
/* rec = [sum c, sum c^2, number of cells with c != 0] over the n cells of counts, accumulated in fp64. */
int pfb_imw_moments(int dtype, const void* counts, size_t n, double* rec, double* work, void* stream);
/* weights (nrow, nchan) of `dtype` for EVERY visibility (no mask, as in the reference) from counts (nx, ny) and their
 * record `rec`, c = counts[floor ug, floor vg]:
 *   briggs == 0 (robust <= -2): 1 / c where c != 0, else 0;
 *   briggs != 0: 1 / (1 + c ssq), ssq = numsqrt^2 / (rec[1] / rec[0]) formed in fp64 and rounded to `dtype`, the rest in
 *     `dtype` (the reference replaces counts by 1 + counts ssq BEFORE the lookup: an empty cell gives 1);
 *   all-zero counts (rec[2] == 0): zeros. */
int pfb_imw_weights(int dtype, const void* counts, const double* rec, const double* uvw, const double* freq, size_t nrow,
                    int nchan, int nx, int ny, double u_cell, double umax, double v_cell, double vmax, int briggs,
                    double numsqrt, void* weights, void* stream);
/* residual_vis = (vis - model_vis) * mask, all complex `dtype` of nvis elements; rec = [sum |residual_vis|^2, sum mask,
 * 0], accumulated in fp64. */
int pfb_imw_l2_residual(int dtype, const void* vis, const void* model_vis, const unsigned char* mask, size_t nvis,
                        void* residual_vis, double* rec, double* work, void* stream);
/* After pfb_imw_l2_residual on the same rec, and only when rec[1] != 0 (the caller's one look at the record):
 * wgt = (dof + 1) / (dof + |residual_vis|^2 / ovar) / ovar, ovar = rec[0] / rec[1] rounded to `dtype`, times imwgt where
 * imwgt (nvis of `dtype`) is not NULL; rec[2] = sum of wgt where mask != 0, in fp64. */
int pfb_imw_l2_weights(int dtype, const void* residual_vis, const unsigned char* mask, const void* imwgt, size_t nvis,
                       double dof, double* rec, void* wgt, double* work, void* stream);
/* rec[0] = sum of wgt where mask != 0, in fp64. */
int pfb_imw_wsum(int dtype, const void* wgt, const unsigned char* mask, size_t nvis, double* rec, double* work,
                 void* stream);
/* Planes (Stokes products) of one pfb_imw_residual_weigh call. */
#define PFB_IMW_MAX_PROD 4
/* The three passes between the stages of a fastim chunk in one (stokes2im.py:268, 279-295), IN PLACE on
 * nprod (1 .. PFB_IMW_MAX_PROD) planes of nvis visibilities each, vis (nprod, nvis) complex and wgt (nprod, nvis) real of
 * `dtype`:
 *   vis[p, i] = (vis[p, i] - model_vis[model_of[p], i]) * mask[i]   for the planes with model_of[p] >= 0; a plane with
 *     model_of[p] < 0 is not touched.  model_of: nprod ints on the HOST, read before the call returns; model_vis
 *     (nmodel, nvis) complex of `dtype`, NULL with nmodel == 0; every model_of[p] < nmodel;
 *   wgt[p, i] = wgt[p, i] * imwgt[i]   the product formed in fp64 and rounded once to `dtype` (numpy's in-place multiply
 *     of a float32 array by a float64 one); imwgt: nvis DOUBLES whatever `dtype`, one plane for all products; NULL
 *     leaves wgt as it is;
 *   rec[p] = sum of wgt[p, i] over mask[i] != 0, of the weights as stored, accumulated in fp64: nprod device doubles.
 * work: PFB_IMW_WORK_DOUBLES doubles of scratch; a fixed order, no atomics: the same bits from run to run.  nvis == 0
 * launches nothing and clears rec.  vis, wgt, model_vis, imwgt and mask must not overlap. */
int pfb_imw_residual_weigh(int dtype, int nprod, void* vis, const void* model_vis, int nmodel, const int* model_of,
                           const unsigned char* mask, const double* imwgt, size_t nvis, void* wgt, double* rec,
                           double* work, void* stream);

/* ---------------------------------------------------------------- Stokes visibilities and weights
 * pfb/utils/weighting.py:281-350 (_weight_data over the functions pfb/utils/stokes.py generates) with the preparation
 * of pfb/utils/stokes2im.py:98-195 fused in, one pass.  Per (row, channel), with Gp, Gq the 2 x 2 Jones matrices of
 * ant1[row], ant2[row] at the row's time bin and the channel, direction 0, V the correlations, w their weights and B the
 * basis matrix:
 *     vis = 1/2 tr(B^H Gp^-1 V Gq^-H)          wgt = sum_ab w_ab |(Gp B Gq^H)_ab|^2
 * basis 0: [[1,0],[0,1]]   1: [[1,0],[0,-1]]   2: [[0,1],[1,0]]   3: [[0,i],[-i,0]].
 * Jones modes: `jones` is (ntime, nant, nchan, ndir, 2) with the diagonal (DIAG4, DIAG2), (ntime, nant, nchan, ndir, 2, 2)
 * (FULL4) or not read (NOJ4, NOJ2: unit Jones terms); the last digit is the number of correlations of data, data2,
 * weight and flag.  With two correlations v01 = v10 = 0 and w01 = w10 = 1, as in the reference. */
#define PFB_STOKES_DIAG4 0
#define PFB_STOKES_DIAG2 1
#define PFB_STOKES_FULL4 2
#define PFB_STOKES_NOJ4  3
#define PFB_STOKES_NOJ2  4
/* weight forms: ones (weight not read); weight holds sigma (nrow, nchan, ncorr), w = 1 / (sigma sigma); a weight
 * spectrum (nrow, nchan, ncorr); a row weight (nrow, ncorr) */
#define PFB_STOKES_W_NONE     0
#define PFB_STOKES_W_SIGMA    1
#define PFB_STOKES_W_SPECTRUM 2
#define PFB_STOKES_W_ROW      3
/* data, data2 (or NULL; data - data2 when subtract, else data + data2): complex `dtype` (nrow, nchan, ncorr).
 * flag: nflagcorr bytes per visibility, nflagcorr = ncorr (any of them flags), 1, or 0 (flag not read); frow (nrow) or
 * NULL; autocorr != 0 flags rows with ant1 == ant2.  Row r belongs to time bin t when
 * tbin_idx[t] - tbin_off <= r < tbin_idx[t] - tbin_off + tbin_counts[t]; the bins ascend and do not overlap (the
 * caller's check), tbin_off is their minimum; found per row by a binary search on the device.
 * Out: vis complex (nrow, nchan), wgt real (nrow, nchan), mask bytes (nrow, nchan) = !flagged, wsum[0] = the fp64 sum of
 * wgt over unflagged visibilities (work: PFB_REDUCE_WS_DOUBLES doubles of scratch; a fixed order, the same bits from run
 * to run).  A flagged visibility, a row no bin covers and a row with an antenna outside [0, nant) get vis = wgt = 0 by
 * selection: NaN or Inf in their data or weights do not reach an output.  A singular Jones matrix on a live visibility
 * gives IEEE inf / nan, as in the reference.  data, data2, weight, jones must be aligned to their vector loads
 * (min(16, bytes per visibility)), else PFB_ERR_INVALID. */
int pfb_stokes_vis(int dtype, int mode, int basis, const void* data, const void* data2, int subtract, const void* weight,
                   int wform, const unsigned char* flag, int nflagcorr, const unsigned char* frow, int autocorr,
                   const void* jones, int ndir, int ntime, int nant, const long long* tbin_idx,
                   const long long* tbin_counts, long long tbin_off, const int* ant1, const int* ant2, size_t nrow,
                   int nchan, void* vis, void* wgt, unsigned char* mask, double* wsum, double* work, void* stream);
/* pfb_stokes_vis for nprod = 1 .. 4 products in ONE pass: `basis` is a HOST array of nprod distinct basis indices (0 .. 3,
 * read before the call returns), in the order of the output planes.  The correlations, weights, flags and Jones terms of
 * a visibility are read once.  Out: vis complex and wgt real (nprod, nrow, nchan), product-major; mask (nrow, nchan), the
 * same for every product; wsum[k], k < nprod, the fp64 sum of plane k's wgt over unflagged visibilities.  Everything
 * else as pfb_stokes_vis, per plane.  PFB_ERR_INVALID: nprod outside 1 .. 4, a NULL basis list, a basis outside 0 .. 3
 * or asked for twice, and what pfb_stokes_vis refuses; nothing is written. */
int pfb_stokes_vis_multi(int dtype, int mode, int nprod, const int* basis, const void* data, const void* data2,
                         int subtract, const void* weight, int wform, const unsigned char* flag, int nflagcorr,
                         const unsigned char* frow, int autocorr, const void* jones, int ndir, int ntime, int nant,
                         const long long* tbin_idx, const long long* tbin_counts, long long tbin_off, const int* ant1,
                         const int* ant2, size_t nrow, int nchan, void* vis, void* wgt, unsigned char* mask, double* wsum,
                         double* work, void* stream);
/* Channel averaging (what africanus.averaging.time_and_channel does for pfb/utils/stokes2vis.py:174-203 with
 * time_bin_secs -> 0) of vis complex and wgt real (nprod, nrow, nchan), nprod = 1 .. 4, with their one mask (nrow, nchan),
 * as the two entry points above leave them.  With n = chan_average >= 1, nchan_out = ceil(nchan / n); bin j of a row
 * covers its channels [j n, min((j + 1) n, nchan)).  Per row, bin and plane, over the bin's LIVE samples (mask != 0) in
 * channel order:
 *     wgt_out = sum wgt_i    vis_out = sum wgt_i vis_i / wgt_out, exactly 0 where wgt_out == 0    mask_out = any(mask_i)
 * Samples that are not live are selected out, never multiplied by zero: what a masked sample holds reaches no output.  A
 * product wgt_i vis_i is formed in `dtype`, the sums in fp64 and rounded to `dtype` once, in front of the division.
 * Out: viso, wgto (nprod, nrow, nchan_out), masko (nrow, nchan_out), wsum[k], k < nprod, the fp64 sum of plane k's wgt_out
 * over mask_out != 0 (work: PFB_REDUCE_WS_DOUBLES doubles of scratch).  A fixed order, no atomics: the same bits from
 * run to run.  The outputs must not overlap the inputs.  PFB_ERR_INVALID: nprod outside 1 .. 4, chan_average < 1, a null
 * or misaligned array; PFB_ERR_UNSUPPORTED: nrow or nchan outside [1, 2^31); nothing is written. */
int pfb_chan_average(int dtype, int nprod, const void* vis, const void* wgt, const unsigned char* mask, size_t nrow,
                     int nchan, int chan_average, void* viso, void* wgto, unsigned char* masko, double* wsum,
                     double* work, void* stream);

/* ------------------------------------------------ band / time concatenation and beam resampling
 * The grid worker's merge of its input datasets (pfb/workers/grid.py:150-214, 404-412): sum_overlap and _sum_beam of
 * pfb/utils/misc.py:1009-1067 and _eval_beam of pfb/utils/beam.py:120-140.  Asynchronous on `stream`, no atomics: the
 * same bits from run to run.  Arrays of pointers (vis, wgt, mask, beams) and nrows, nchans are HOST arrays of nds
 * entries, read before the call returns; what they point to is device memory. */
/* Sources travel to a kernel by value, this many per launch; a later launch accumulates onto the first one's partial
 * sums (of the data's type: the round trip is exact), the last one closes. */
#define PFB_VIS_BATCH 8
/* Source i: vis complex, wgt real, mask bytes, each (nrows[i], nchans[i]).  chan_map: DEVICE int (nds, nchan_out), the
 * channel of source i that lands in output channel c or -1 (an entry outside [0, nchans[i]) is read as -1).
 *   viso = sum_i vis wgt mask, wgto = sum_i wgt mask, masko = 1 where any source mask != 0 else 0, summed in source
 *   order in `dtype`, every operation rounded on its own; viso /= wgto where masko (a plain IEEE division: weights that
 *   sum to zero on an unflagged sample give inf / nan, as in the reference); where masko == 0 all three are exactly 0.
 * All (nrow, nchan_out).  PFB_ERR_INVALID: a null array, a source whose nrows[i] != nrow. */
int pfb_vis_sum_overlap(int dtype, int nds, const void* const* vis, const void* const* wgt,
                        const unsigned char* const* mask, const size_t* nrows, const int* nchans, const int* chan_map,
                        size_t nrow, int nchan_out, void* viso, void* wgto, unsigned char* masko, void* stream);
/* rec[0] = the sum of ALL n elements of wgt (no mask, as _sum_beam has it), in fp64 (work: PFB_IMW_WORK_DOUBLES doubles
 * of scratch; a fixed order). */
int pfb_vis_weight_sums(int dtype, const void* wgt, size_t n, double* rec, double* work, void* stream);
/* out = sum_i wsum[i] beams[i], divided by sum_i wsum[i] where that is not zero; wsum: the DEVICE record of nds doubles
 * that pfb_vis_weight_sums filled, each rounded to `dtype`; summed in source order in `dtype`.  npix pixels each. */
int pfb_beam_combine(int dtype, int nds, const void* const* beams, const double* wsum, size_t npix, void* out,
                     void* stream);
/* Bilinear interpolation of beam (nl, nm) of `dtype`, given on the ascending axes l_in (nl), m_in (nm), at (nxo, nyo)
 * points: coord2d == 0: (l_out[i], m_out[j]) of l_out (nxo), m_out (nyo); else l_out, m_out are (nxo, nyo).  The cell
 * of x is the i of g[i] <= x < g[i + 1] clipped to [0, n - 2] (binary search: any spacing), the distance
 * (x - g[i]) / (g[i + 1] - g[i]): points outside are linearly extrapolated from the edge cell, a NaN gives NaN.
 * Coordinates and weights are fp64; out is of `out_dtype`, rounded at the store.  nl, nm >= 2. */
int pfb_beam_eval(int dtype, const void* beam, int nl, int nm, const double* l_in, const double* m_in,
                  const double* l_out, const double* m_out, int coord2d, int nxo, int nyo, int out_dtype, void* out,
                  void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PFB_HIP_H */
