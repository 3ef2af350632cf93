"""
Preconditioned conjugate gradients on MI355X -- drop-in for pfb/opt/pcg.py.

    pcg(A, b, x0=None, M=None, tol=1e-5, maxit=500, minit=100, verbosity=1,
        report_freq=10, backtrack=True, return_resid=False)          pcg.py:53-136
    pcg_psf(psfhat, b, x0, beam, lastsize, nthreads, sigmainv, cgopts, compute=True)
                                                                      pcg.py:243-360
    pcg_fused_bands(A, b, x0, mdiv, tol, maxit, minit, backtrack, return_resid)
                                                       every band its own PCG, one batched solve

Two execution paths with identical semantics (residual r = A x - b, stopping rule
`(eps > tol or k < minit) and k < maxit`, backtracking without extra matvecs,
break-before-increment on an all-zero direction, "Initial residual is zero" returns x0):

 * FUSED: when `A` is a HessianPsf (or a functools.partial of this package's
   hessian_psf_cube / _hessian_psf_slice, which is exactly what the reference workers
   build -- fluxmop.py:160-174, pcg.py:276-284) and `M` is None or a DivPrecond, the
   whole solve runs inside libpfb_hip.so (pfb_pcg_solve): 3 convolution kernels + 3
   fused vector kernels per iteration, device-resident scalars.
 * FUSED, band-coupled: when `A` is a ParamHessian of at most 16 bands (or the fwdbwd worker's
   `partial(hessian_psf, psf_convolve, xp, sigmainv, df, dhf)` built from this package's pieces,
   fwdbwd.py:318) the same driver runs with the mix -> convolution -> mix operator step
   (pfb_pcg_solve_param): one system over all bands.
 * GENERIC: any Python callables A, M.  Vector arithmetic and reductions still run in
   the HIP kernels (pfb_dot, pfb_axpby, pfb_norm_diff_sums, pfb_any_nonzero); A and M
   are called with the same array kind (numpy / tensor) the caller passed for `b`.
"""
import ctypes as C
import functools
import math
import os
import sys

import torch

from .. import _lib, _dev
from ..operators import hessian as _hess
from ..operators.hessian import HessianPsf, ParamHessian


class DivPrecond:
    """M(x) = x / div -- the diagonal preconditioner of pcg.py:264-267."""

    def __init__(self, div):
        self.div = float(div)

    def __call__(self, x):
        return x / self.div


def _detect_div_precond(M, b):
    """The workers write the preconditioner as a closure, `lambda x: x / sigmainv` (pcg.py:264-267,
    fluxmop.py).  A closure cannot be inspected, but it can be ASKED: M is applied once to b itself and
    to -2 b; if both answers are b / c and -2 b / c for one scalar c (elementwise, to rounding), M is the
    scalar division and the solve stays on the fused path.  Anything else (a diagonal with varying
    entries, an operator, something non-linear) fails the elementwise test and keeps the generic path."""
    try:
        bd = _dev.to_dev(b)
        y1 = _dev.to_dev(M(_dev.host_like(bd, b)), bd.dtype)
        if y1.shape != bd.shape:
            return None
        flat_b, flat_y = bd.reshape(-1), y1.reshape(-1)
        k = int(torch.argmax(flat_b.abs()).item())
        if flat_b[k].item() == 0.0 or flat_y[k].item() == 0.0:
            return None
        c = flat_b[k].item() / flat_y[k].item()
        eps = 16 * torch.finfo(bd.dtype).eps
        scale = flat_b.abs().max().item() / abs(c)
        if (flat_y - flat_b / c).abs().max().item() > eps * scale:
            return None
        y2 = _dev.to_dev(M(_dev.host_like(-2.0 * bd, b)), bd.dtype).reshape(-1)
        if (y2 + 2.0 * flat_b / c).abs().max().item() > 2 * eps * scale:
            return None
        return DivPrecond(c)
    except Exception:
        return None


def _log(msg, verbosity, level=1):
    if verbosity >= level:
        print(msg, file=sys.stderr)


def _as_hessian(A, b):
    """Recognise the operator objects / partials the fused driver can run."""
    if isinstance(A, HessianPsf):
        return A
    if isinstance(A, ParamHessian):
        return A if A.fused and tuple(b.shape) == (A.nb, A.nx, A.ny) else None
    if isinstance(A, functools.partial) and A.func is _hess.hessian_psf:
        H = _hess.as_param_hessian(A, b)        # None as well with _nofuse=True among the partial's keywords
        return H if H is not None and H.fused else None
    if isinstance(A, functools.partial) and not A.keywords.get('_nofuse', False):
        kw = dict(A.keywords)
        args = A.args
        nx, ny = b.shape[-2:]
        try:
            if A.func is _hess.hessian_psf_cube and len(args) == 6:
                _, _, _, beam, psfhat, lastsize = args
            elif A.func is _hess._hessian_psf_slice and len(args) == 6:
                _, _, _, psfhat, beam, lastsize = args
            else:
                return None
        except ValueError:
            return None
        return HessianPsf(psfhat, nx, ny, lastsize, beam=beam,
                          sigmainv=kw.get('sigmainv', 1), wsum=kw.get('wsum', None))
    return None


def _backtrack_mode(backtrack):
    """False -> 0; True -> 2 (predictive line search, same decisions as pcg.py:96-101 from
    three fused scalars) unless PFB_PCG_EXACT_BACKTRACK=1 or backtrack == 'exact' -> 1 (the
    reference loop verbatim, one extra vector pass per rejected step)."""
    if not backtrack:
        return 0
    if backtrack == 'exact' or os.environ.get('PFB_PCG_EXACT_BACKTRACK', '0') == '1':
        return 1
    return 2


class _Staged:
    """What pcg_fused and pcg_fused_bands share around the native call: the checks on b, the contiguous copies on the
    plan's grid (an embedded plan solves in its padded domain, operators/psf.py: zero-padded b and x0, a beam that is
    zero outside the image; a ParamHessian's e is one already), the work buffer (kept on the plan,
    PsfConvPlan._solve_work), the call itself and the way back.  `kind`: the work buffer's layout for a HessianPsf, ''
    (the cube solve's) or 'bands_'."""

    def __init__(self, A, b3, x0, return_resid, kind=''):
        self.plan = plan = A.plan
        b3 = b3.contiguous()
        if kind == 'bands_' and b3.ndim != 3:
            raise ValueError("pcg_fused_bands expects (nb, nx, ny) arrays")
        self.nb = nb = b3.shape[0]
        if nb != A.nb:
            raise ValueError(f"b has {nb} bands, operator has {A.nb}")
        if b3.dtype != plan.rdtype:
            raise TypeError(f"b is {b3.dtype}, operator is {plan.rdtype}")
        x = torch.zeros_like(b3) if x0 is None else x0.contiguous().clone()
        param = isinstance(A, ParamHessian)
        b3, x = plan.to_grid(b3, nb), plan.to_grid(x, nb)
        beam = A.e if param else plan.grid_beam(A.beam, nb)
        self.b, self.x, self.beam = b3, x, beam
        self.r = torch.empty_like(b3) if return_resid else None
        self.work = plan._solve_work('param_' if param else kind, nb)
        # what the entry point's arguments start with, up to sigmainv
        ptr = _dev.ptr
        if param:
            self.args = (nb, ptr(A.L), ptr(A.LH), ptr(beam), ptr(b3), ptr(x), ptr(self.r), A.sigmainv)
        else:
            self.args = (A.band0, nb, ptr(b3), ptr(x), ptr(self.r), ptr(beam),
                         A.wsum if A.wsum is not None else 0.0, A.sigmainv)

    def solve(self, fn_name, mdiv, tol, maxit, minit, backtrack, *tail):
        """fn_name(plan, *args, mdiv .. backtrack, work, *tail, stream), one solve at a time per plan (a plan is
        single-owner, include/pfb_hip.h).  Returns (x, r|None) in the caller's domain."""
        self.plan.run(fn_name, *self.args, float(mdiv), float(tol), int(maxit), int(minit), _backtrack_mode(backtrack),
                      _dev.ptr(self.work), *tail)
        return self.plan.from_grid(self.x), None if self.r is None else self.plan.from_grid(self.r)


def pcg_fused(A, b, x0=None, mdiv=0.0, tol=1e-5, maxit=500, minit=100, backtrack=True,
              return_resid=False, group=None, distributed=False):
    """Run pfb_pcg_solve (A a ParamHessian: pfb_pcg_solve_param).  b, x0: GPU tensors (nb, nx, ny) | (nx, ny).  Returns
    (x, r|None, PcgResult).  distributed=True: the bands of this call are one rank's
    shard of a cube solve; every inner product is all-reduced over `group`
    (pfb_clean_amd.dist.AllReduceHook, RCCL)."""
    param = isinstance(A, ParamHessian)
    if param and distributed:
        raise ValueError("a ParamHessian couples every band: it cannot be solved on a band shard")
    squeeze = b.ndim == 2 and not param
    s = _Staged(A, b[None] if squeeze else b, x0[None] if squeeze and x0 is not None else x0, return_resid)
    res = _lib.PcgResult()
    cb_ctx = None
    native = None
    if distributed:
        from ..dist import AllReduceHook, native_comm
        native = native_comm(group, s.b.device) if s.b.is_cuda else None
    if not distributed:
        cb = _lib.ALLREDUCE_FN(0)
    elif native is not None:             # RCCL from C on the solver's stream: nothing on the host per iteration
        cb, cb_ctx = native.fn, native.ctx
    else:
        allreduce = AllReduceHook(s.work, group)

        def _hook(ctx, buf, count, stream):
            try:
                allreduce(buf or 0, count)      # count == 0: probe, count < 0: abort (include/pfb_hip.h)
                return 0
            except Exception as e:   # never let an exception cross the C boundary
                if count > 0:
                    print(f"pfb_clean_amd: allreduce hook failed: {e!r}", file=sys.stderr)
                return 1
        cb = _lib.ALLREDUCE_FN(_hook)
    if param:                        # no hook argument: a band shard cannot apply the mix
        x, r = s.solve('pfb_pcg_solve_param', mdiv, tol, maxit, minit, backtrack, C.byref(res))
    else:
        x, r = s.solve('pfb_pcg_solve', mdiv, tol, maxit, minit, backtrack, cb, cb_ctx, C.byref(res))
    if distributed:                  # bench.py reports which exchange ran and what the hook costs the host
        res.exchange = 'rccl-native' if native is not None else 'torch-hook'
        res.hook_calls, res.hook_host_s = (0, 0.0) if native is not None else (allreduce.calls, allreduce.host_s)
    if squeeze:
        x = x[0]
        r = None if r is None else r[0]
    return x, r, res


def pcg_fused_bands(A, b, x0=None, mdiv=0.0, tol=1e-5, maxit=500, minit=100, backtrack=True,
                    return_resid=False):
    """Run pfb_pcg_solve_bands: every band of A (a HessianPsf over nb bands) is its own PCG, all bands in one
    batched device solve -- pcg_psf's semantics (pcg.py:243-360).  b, x0: GPU tensors (nb, nx, ny).  Returns
    (x, r|None, [PcgResult] * nb); a band with PFB_PCG_ZERO_RESIDUAL keeps x = x0.  backtrack='exact' (or
    PFB_PCG_EXACT_BACKTRACK=1) has no batched form: the library raises PfbHipError (unsupported)."""
    s = _Staged(A, b, x0, return_resid, kind='bands_')
    res = (_lib.PcgResult * s.nb)()
    x, r = s.solve('pfb_pcg_solve_bands', mdiv, tol, maxit, minit, backtrack, res)
    return x, r, list(res)


def _bands_batched(plan):
    """Whether pcg_psf runs its bands as one batched solve on this plan.  Not on the 4096-point fp32 rows (plan ny = 8192:
    8192-pixel images and, embedded, fp32 images of 6145-8192 pixels): that row tile has no per-band persistent
    inverse kernel, the batched solve launches the whole-cube one once per band there, and measured 2-3 % slower than
    the band loop (2 x 8192^2: 153.2 vs 148.8 ms, 2 x 6000^2: 162.5 vs 159.2 ms for 50 iterations).  fp32 images with rows of
    4097-6144 pixels, which that plan held before the 5 2^k / 3 2^k rows (plan ny = 5120, 6144) took them, keep the band
    loop they had: on the plain inverse-row kernel of those rows the two are 1.3 % apart the other way (2 x 6000^2 on
    6144^2, 50 iterations, three alternating runs: loop 142.1 / 141.1 / 141.0 ms, batched 139.4 / 139.7 / 139.3 ms), which
    was not taken as reason enough to change what pcg_psf does for these images."""
    ny = plan.embed[1] if plan.embed is not None else plan.ny
    return not (plan.fast_path and plan.rdtype == torch.float32 and 4096 < ny <= 8192)


def _report(res_status, k, eps, verbosity):
    if res_status == 'maxit':
        _log(f"Max iters reached. eps = {eps:.3e}", verbosity)
    elif res_status in ('converged', 'breakdown'):
        _log(f"Success, converged after {k} iterations", verbosity)


def pcg(A, b, x0=None, M=None, tol=1e-5, maxit=500, minit=100, verbosity=1,
        report_freq=10, backtrack=True, return_resid=False):
    """pfb/opt/pcg.py:53-136."""
    H = _as_hessian(A, b)
    if H is not None and M is not None and not isinstance(M, DivPrecond):
        M = _detect_div_precond(M, b) or M
    fusable_M = M is None or isinstance(M, DivPrecond)
    if H is not None and fusable_M:
        bd = _dev.to_dev(b)
        x0d = None if x0 is None else _dev.to_dev(x0, bd.dtype)
        x, r, res = pcg_fused(H, bd, x0d, mdiv=M.div if M is not None else 0.0, tol=tol,
                              maxit=maxit, minit=minit, backtrack=backtrack,
                              return_resid=return_resid)
        status = _lib.PCG_STATUS[res.status]
        if status == 'zero-residual':
            _log("Initial residual is zero", verbosity)
            # the reference returns x0 itself, and ONLY x0, even with return_resid
            return x0 if x0 is not None else _dev.host_like(x, b)
        _report(status, res.iters, res.eps, verbosity)
        return (_dev.host_like(x, b), _dev.host_like(r, b)) if return_resid else _dev.host_like(x, b)
    return _pcg_generic(A, b, x0, M, tol, maxit, minit, verbosity, report_freq, backtrack,
                        return_resid)


def _pcg_generic(A, b, x0, M, tol, maxit, minit, verbosity, report_freq, backtrack,
                 return_resid):
    as_numpy = _dev.is_numpy(b)
    bd = _dev.to_dev(b)
    dt = bd.dtype

    def host(t):
        return _dev.host_like(t, b)

    def dev(a):
        return _dev.to_dev(a, dt)

    def callA(v):
        return dev(A(host(v))).clone() if not as_numpy else dev(A(host(v)))

    def callM(v):
        return v if M is None else dev(M(host(v)))

    dot, axpby = _dev.dot, _dev.axpby
    x0_in = x0
    x = torch.zeros_like(bd) if x0 is None else dev(x0).clone()
    r = callA(x)
    axpby(-1.0, bd, 1.0, r)                          # r = A(x0) - b
    y = callM(r)
    if not _dev.any_nonzero(y):
        _log("Initial residual is zero", verbosity)
        return x0_in if x0_in is not None else host(x)
    p = y.clone()
    axpby(0.0, y, -1.0, p)                           # p = -y
    k = 0
    eps = 1.0
    xp = torch.empty_like(x)
    rp = torch.empty_like(r)
    broke = False
    while (eps > tol or k < minit) and k < maxit:
        xp.copy_(x)
        rp.copy_(r)
        Ap = callA(p)
        rnorm = dot(r, y)
        alpha = rnorm / dot(p, Ap)
        x.copy_(xp); axpby(alpha, p, 1.0, x)
        r.copy_(rp); axpby(alpha, Ap, 1.0, r)
        y = callM(r)
        rnorm_next = dot(r, y)
        while rnorm_next > rnorm and backtrack:
            alpha *= 0.75
            x.copy_(xp); axpby(alpha, p, 1.0, x)
            r.copy_(rp); axpby(alpha, Ap, 1.0, r)
            y = callM(r)
            rnorm_next = dot(r, y)
        beta = rnorm_next / rnorm
        axpby(-1.0, y, beta, p)                      # p = beta*p - y
        if not _dev.any_nonzero(p):
            broke = True
            break
        k += 1
        num, den = _dev.norm_diff_sums(x, xp).tolist()
        eps = math.sqrt(num / (1e-12 + den))
        if not k % report_freq and verbosity > 1:
            _log(f"At iteration {k} epsx = {eps:.3e}", verbosity, 2)
    _report('maxit' if (k >= maxit and not broke) else 'converged', k, eps, verbosity)
    if not return_resid:
        return host(x)
    return host(x), host(r)


def cg_dct(A, b, x, tol=1e-5, maxit=500, verbosity=1, report_freq=10):
    """pfb/opt/pcg.py:139-239 -- plain CG whose unknown is a nested dict
    {field: {'t..b..': image}} (distinct fields, no preconditioner, no backtracking; unused by
    the live workers).  r = A x - b, eps = <r, r> over all leaves, rule
    `eps > tol and k < maxit`.  Leaves live on the GPU for the whole solve; `A` is called with a
    dict of GPU tensors when the caller's leaves are tensors, of numpy arrays otherwise, and like
    the reference the caller's `x` leaves are updated in place.  Returns (x, r)."""
    leaf = next(iter(next(iter(b.values())).values()))

    def todev(d):
        return {f: {i: _dev.to_dev(d[f][i]) for i in d[f]} for f in d}

    def callA(d):
        if not _dev.is_numpy(leaf):
            return todev(A(d))
        return todev(A({f: {i: _dev.host_like(d[f][i], leaf) for i in d[f]} for f in d}))

    def vdot(u, v):
        return sum(_dev.dot(u[f][i], v[f][i]) for f in u for i in u[f])

    def axpby(a, u, bb, v):       # v = a*u + bb*v, leaf by leaf
        for f in v:
            for i in v[f]:
                _dev.axpby(a, u[f][i], bb, v[f][i])

    xd = todev(x)                    # a caller's contiguous device tensors are the leaves themselves: updated in place
    bd = todev(b)
    r = callA(xd)
    r = {f: {i: r[f][i].clone() for i in r[f]} for f in r}
    axpby(-1.0, bd, 1.0, r)                                   # r = A x - b
    p = {f: {i: -r[f][i] for i in r[f]} for f in r}
    rnorm = vdot(r, r)
    eps, k = rnorm, 0
    while eps > tol and k < maxit:
        Ap = callA(p)
        alpha = rnorm / vdot(p, Ap)
        axpby(alpha, p, 1.0, xd)                              # x += alpha p
        axpby(alpha, Ap, 1.0, r)                              # r += alpha Ap
        rnorm_next = vdot(r, r)
        beta = rnorm_next / rnorm
        axpby(-1.0, r, beta, p)                               # p = beta p - r
        rnorm = rnorm_next
        eps = rnorm
        k += 1
        if not k % report_freq and verbosity > 1:
            _log(f"At iteration {k} eps = {eps:.3e}", verbosity, 2)
    if verbosity:
        _log(f"Max iters reached. eps = {eps:.3e}" if k >= maxit
             else f"Success, converged after {k} iterations", verbosity)
    for f in x:                                               # in-place semantics of the reference
        for i in x[f]:
            _dev.deliver(xd[f][i], x[f][i])
    return x, {f: {i: _dev.host_like(r[f][i], leaf) for i in r[f]} for f in r}


def pcg_dist(A, maxit, minit, tol, sigmainv):
    """pfb/opt/pcg.py:363-420 -- the per-band PCG variant of the (commented-out) distributed
    spotless: b = A.residual/A.wsum (A.dirty without a residual), x0 = 0, M = x/sigmainv,
    eps = rnorm/eps0 with eps0 the INITIAL <r, y>, stall counter in the stopping rule.  A is a
    hessian_psf_slice (or anything with those attributes, callable on GPU tensors).  All vectors
    stay on the GPU; the matvec is the fused convolution, the recurrences are pfb_axpby /
    pfb_dot / pfb_any_nonzero; the scalars the while-conditions need come back per iteration
    (this path keeps the reference's exact backtracking loop)."""
    src = A.residual if hasattr(A, 'residual') else A.dirty
    b = _dev.to_dev(src) / float(A.wsum)
    dt = b.dtype
    dot, axpby = _dev.dot, _dev.axpby

    def callA(v):
        return _dev.to_dev(A(v), dt).clone()

    x = torch.zeros_like(b)
    r = callA(x)
    axpby(-1.0, b, 1.0, r)                           # r = A(x) - b
    y = r / sigmainv
    p = -y
    rnorm = dot(r, y)
    eps0 = 1.0 if (math.isnan(rnorm) or rnorm == 0.0) else rnorm
    k, eps, stall = 0, 1.0, 0
    xp, rp = torch.empty_like(x), torch.empty_like(r)
    while (eps > tol or k < minit) and k < maxit and stall < 5:
        xp.copy_(x)
        rp.copy_(r)
        epsp = eps
        Ap = callA(p)
        rnorm = dot(r, y)
        alpha = rnorm / dot(p, Ap)
        while True:
            x.copy_(xp); axpby(alpha, p, 1.0, x)
            r.copy_(rp); axpby(alpha, Ap, 1.0, r)
            y = r / sigmainv
            rnorm_next = dot(r, y)
            if not rnorm_next > rnorm:
                break
            alpha *= 0.75
        beta = rnorm_next / rnorm
        axpby(-1.0, y, beta, p)                      # p = beta*p - y
        if not _dev.any_nonzero(p):
            break
        rnorm = rnorm_next
        k += 1
        eps = rnorm / eps0
        if abs(eps - epsp) < 1e-3 * tol:
            stall += 1
    print(f'Band={getattr(A, "bandid", "?")}, iters{k}, eps={eps}', file=sys.stderr)
    return _dev.host_like(x, src)


def cg(A, b, x0=None, tol=1e-5, maxit=500, verbosity=1, report_freq=10):
    """pfb/opt/pcg.py:12-50 -- the plain CG variant (no preconditioner, no backtracking,
    stopping rule `eps = <r,r> > tol`, unused by the live workers).  Vector work and
    reductions in the HIP kernels; A is called with the array kind of `b`."""
    bd = _dev.to_dev(b)
    dt = bd.dtype
    dot, axpby = _dev.dot, _dev.axpby

    def host(t):
        return _dev.host_like(t, b)

    x = torch.zeros_like(bd) if x0 is None else _dev.to_dev(x0, dt).clone()
    r = _dev.to_dev(A(host(x)), dt).clone()
    axpby(-1.0, bd, 1.0, r)                          # r = A(x) - b
    p = r.clone()
    axpby(0.0, r, -1.0, p)                           # p = -r
    rnorm = dot(r, r)
    eps, k = rnorm, 0
    while eps > tol and k < maxit:
        Ap = _dev.to_dev(A(host(p)), dt)
        alpha = rnorm / dot(p, Ap)
        axpby(alpha, p, 1.0, x)
        axpby(alpha, Ap, 1.0, r)
        rnorm_next = dot(r, r)
        beta = rnorm_next / rnorm
        axpby(-1.0, r, beta, p)                      # p = beta*p - r
        rnorm = rnorm_next
        eps = rnorm
        k += 1
    if k >= maxit and verbosity:
        print(f"Max iters reached eps = {eps}", file=sys.stderr)
    return host(x)


def pcg_psf(psfhat, b, x0, beam, lastsize, nthreads, sigmainv, cgopts, compute=True):
    """pfb/opt/pcg.py:310-360 (+ _pcg_psf_impl :243-291): independent PCG per band with
    A = _hessian_psf_slice(psfhat[k], beam[k], sigmainv) and M = x/sigmainv when
    sigmainv > 0.  The reference's dask blockwise-over-bands becomes ONE batched device solve
    on one plan (pcg_fused_bands: every band keeps its own step lengths and stopping rule);
    backtrack='exact' (or PFB_PCG_EXACT_BACKTRACK=1) has no batched form, and fp32 plans of
    8192-pixel rows are faster band by band (_bands_batched): both run the bands one after
    another through pcg_fused.  Bands are independent: shard them over GPUs with
    pfb_clean_amd.dist.shard_bands for multi-GPU."""
    bd = _dev.to_dev(b)
    nband, nx, ny = bd.shape
    if psfhat.shape[0] != nband:
        raise ValueError("psfhat and b disagree on the number of bands")
    beamd = None
    if beam is not None:
        beamd = _dev.to_dev(beam, bd.dtype)
        if beamd.ndim == 2:
            beamd = beamd[None]
        if beamd.shape[0] == 1:
            beamd = beamd.expand(nband, -1, -1)
        elif beamd.shape[0] != nband:
            raise ValueError('Beam has incorrect shape')
    x0d = torch.zeros_like(bd) if x0 is None else _dev.to_dev(x0, bd.dtype)
    from ..operators.psf import plan_for
    plan = plan_for(psfhat, nx, ny, lastsize)
    model = torch.zeros_like(bd)
    opts = dict(cgopts)
    verbosity = opts.pop('verbosity', 1)
    opts.pop('report_freq', None)
    mdiv = sigmainv if sigmainv > 0 else 0.0

    def deliver(k, res, xk):
        status = _lib.PCG_STATUS[res.status]
        if status == 'zero-residual':
            _log("Initial residual is zero", verbosity)
            model[k] = x0d[k]
        else:
            _report(status, res.iters, res.eps, verbosity)
            model[k] = xk

    if _backtrack_mode(opts.get('backtrack', True)) != 1 and _bands_batched(plan):
        A = HessianPsf(plan, nx, ny, lastsize, beam=beamd, sigmainv=sigmainv, band0=0, nb=nband)
        x, _, results = pcg_fused_bands(A, bd, x0d, mdiv=mdiv, **opts)
        for k, res in enumerate(results):
            deliver(k, res, x[k])
        return _dev.host_like(model, b)
    for k in range(nband):
        A = HessianPsf(plan, nx, ny, lastsize, beam=None if beamd is None else beamd[k:k + 1],
                       sigmainv=sigmainv, band0=k, nb=1)
        x, _, res = pcg_fused(A, bd[k:k + 1], x0d[k:k + 1], mdiv=mdiv, **opts)
        deliver(k, res, x[0])
    return _dev.host_like(model, b)
