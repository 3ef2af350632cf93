"""
PSF-approximated, Tikhonov-regularised Hessians on MI355X -- drop-in for
pfb/operators/hessian.py:129-158 (_hessian_psf_slice) and :254-281 (hessian_psf_cube).

    out = [beam*] psf_convolve([beam*] x) [/ wsum] + sigmainv * x

beam multiply, 1/wsum, the Tikhonov term and (optionally) <p, A p> are fused into the
row kernels of the convolution; the reference's 3-4 extra numpy passes disappear.
Argument orders are the reference's (they differ between the two functions!).
Unlike psf_convolve_* these return a NEW array (hessian.py:158,281: `xout + x*sigmainv`),
and so do we; `xout` additionally receives the result (the reference leaves the
un-regularised convolution there, which no caller reads).

HessianPsf is the object form used by the fused PCG (opt/pcg.py): it carries the plan
and the operator parameters so that `pcg(A, b, ...)` can run the whole solve inside
libpfb_hip.so when A is one of these.

_hessian_impl / hessian / hessian_xds are the VISIBILITY-space Hessian (hessian.py:11-126): dirty2vis then vis2dirty
through operators/gridder.py, the visibilities never leaving their sorted slots in between.
hessian_psf_slice.compute_residual uses it when the dataset carries UVW / WEIGHT / VIS_MASK / FREQ.

ParamHessian / hessian_psf are the band-coupled Hessian of the parametrised forward step
(workers/fwdbwd.py:246-252):  2 dhf(psf_convolve(df(v))) + sigmainv v  with the closures of
utils/misc.py::setup_parametrisation, as band mix -> convolution with the e sandwich -> band mix
(csrc/hessparam.hip).
"""
import functools

import numpy as np
import torch

from .. import _dev, _lib
from . import gridder
from .psf import plan_for, PsfConvPlan, psf_convolve_cube, _run


# ------------------------------------------------------------------ the visibility-space Hessian (hessian.py:11-126)
def _hessian_impl(x, uvw, weight, vis_mask, freq, beam, x0=0.0, y0=0.0, cell=None, do_wgridding=None, epsilon=None,
                  double_accum=None, nthreads=None, reproducible=False):
    """pfb/operators/hessian.py:62-106: beam * vis2dirty(weight * dirty2vis(beam * x)), divide_by_n=False both ways,
    image centre (x0, y0), square pixels of `cell`.  An all-zero x answers zeros without a launch of the gridder.
    beam and weight may be None.  double_accum with a float32 x runs the fp64 kernels on the data cast up.  `nthreads`
    is accepted and ignored.  reproducible (hessopts['reproducible']) grids without atomics: identical bits from run to
    run.  numpy in gives numpy out."""
    if cell is None or do_wgridding is None or epsilon is None:
        raise TypeError("cell, do_wgridding and epsilon are required")
    xd = _dev.to_dev(x)
    if xd.ndim != 2 or xd.dtype not in _dev.CPLX_OF:
        raise TypeError(f"x must be a 2-D float32 or float64 image, got {xd.dtype} {tuple(xd.shape)}")
    if not _dev.any_nonzero(xd):
        return _dev.host_like(torch.zeros_like(xd), x)
    rdt = torch.float64 if double_accum else xd.dtype
    nx, ny = xd.shape
    plan = gridder.plan_for(uvw, freq, vis_mask, nx, ny, cell, cell, x0, y0, epsilon, do_wgridding, rdt, reproducible)
    out = plan.hessian(xd.to(rdt), _dev.to_dev(weight, rdt), _dev.to_dev(beam, rdt))
    return _dev.host_like(out.to(xd.dtype), x)


def hessian(x, uvw, weight, vis_mask, freq, beam, hessopts):
    """hessian.py:113-126 without dask: _hessian_impl on one band's arrays with the options of `hessopts`."""
    return _hessian_impl(x, uvw, weight, vis_mask, freq, beam, **hessopts)


def hessian_xds(x, xds, hessopts, wsum, sigmainv, mask, compute=True, use_beam=True):
    """hessian.py:11-59 over a list of in-memory datasets (variables with `.values`: UVW, FREQ, WEIGHT, MASK [, BEAM],
    and `bandid`): per dataset the Hessian of x[bandid] with beam = BEAM * mask (the mask alone with use_beam=False),
    summed per band, divided by wsum, plus x * sigmainv**2.  x (nband, nx, ny); mask (nx, ny).  `compute` is accepted
    and ignored.  numpy in gives numpy out."""
    xd = _dev.to_dev(x)
    if xd.ndim != 3:
        raise ValueError("hessian_xds expects a (nband, nx, ny) cube")
    md = _dev.to_dev(mask, xd.dtype)
    if md.ndim != 2:
        raise ValueError("mask must be 2-D")
    convim = torch.zeros_like(xd)
    for ds in xds:
        b = ds.bandid
        beam = _dev.to_dev(ds.BEAM.values, xd.dtype) * md if use_beam else md
        convim[b] += _hessian_impl(xd[b], ds.UVW.values, ds.WEIGHT.values, ds.MASK.values, ds.FREQ.values, beam,
                                   **hessopts)
    convim /= wsum
    if sigmainv:
        convim += xd * sigmainv ** 2
    return _dev.host_like(convim, x)


class HessianPsf:
    """A(x) = [beam*]conv([beam*]x)[/wsum] + sigmainv*x on bands [band0, band0+nb).

    psfhat: (nband, nx_psf, nyo2) | (nx_psf, nyo2) complex (numpy or tensor) or an
    existing PsfConvPlan.  beam: None | (nb, nx, ny) | (nx, ny).  Callable on GPU
    tensors or numpy arrays of shape (nb, nx, ny) or (nx, ny)."""

    def __init__(self, psfhat, nx, ny, lastsize, beam=None, sigmainv=0.0, wsum=None,
                 band0=0, nb=None):
        self.plan = psfhat if isinstance(psfhat, PsfConvPlan) else plan_for(psfhat, nx, ny, lastsize)
        self.nx, self.ny = int(nx), int(ny)
        self.band0 = int(band0)
        self.nb = int(nb) if nb is not None else self.plan.nband - self.band0
        self.sigmainv = float(sigmainv)
        self.wsum = None if wsum is None else float(wsum)
        self.beam = None
        if beam is not None:
            b = _dev.to_dev(beam, self.plan.rdtype)
            if b.ndim == 2:
                b = b[None].expand(self.nb, -1, -1)
            if tuple(b.shape) != (self.nb, self.nx, self.ny):
                raise ValueError('Beam has incorrect shape')
            self.beam = b.contiguous()

    @property
    def dtype(self):
        return self.plan.rdtype

    def __call__(self, x, out=None):
        xd = _dev.to_dev(x)
        squeeze = xd.ndim == 2
        if squeeze and self.nb != 1:
            raise ValueError("2-D input to a multi-band HessianPsf")
        res = self.plan.apply(xd, out=out, beam=self.beam, wsum=self.wsum,
                              sigmainv=self.sigmainv, band0=self.band0)
        return _dev.host_like(res, x)

    def apply_dots(self, x, out, dots_out):
        """out = A(x) for contiguous device cubes of the plan's own grid, with <x, A x> left in dots_out[0] and
        <A x, A x> in dots_out[2] (device fp64) out of the convolution's epilogue."""
        self.plan.run('pfb_psfconv_apply_dots', self.band0, self.nb, _dev.ptr(x), _dev.ptr(self.beam),
                      self.wsum if self.wsum is not None else 0.0, self.sigmainv, _dev.ptr(out), _dev.ptr(x), None,
                      _dev.ptr(dots_out))


class hessian_psf_slice:
    """pfb/operators/hessian.py:161-251 -- the per-band stateful operator (only referenced
    from the commented-out distributed spotless, workers/spotless.py:439-520).
    Same constructor signature and attributes; the image-space members live on the GPU
    (torch tensors), `__call__` is _hessian_psf_slice through the band's own plan with the
    wsum given to set_wsum.  `ds` is the reference's per-band dataset or anything exposing the
    same variables with `.values` (DIRTY, PSFHAT, PSF, BEAM, WSUM [, MODEL, DUAL, RESIDUAL])
    and `bandid`.  With UVW, WEIGHT, VIS_MASK and FREQ in the dataset compute_residual is the reference's
    dirty - _hessian_impl(beam * x, ...); without them it raises NotImplementedError."""

    def __init__(self, ds, nbasis, nmax, nthreads, sigmainv, cell=None, do_wgridding=None,
                 epsilon=None, double_accum=None, reproducible=False):
        self.nthreads = nthreads
        self.reproducible = bool(reproducible)          # compute_residual grids without atomics
        self.sigmainv = sigmainv
        self.cell, self.do_wgridding, self.epsilon, self.double_accum = cell, do_wgridding, epsilon, double_accum
        self.lastsize = ds.PSF.shape[-1]
        self.bandid = ds.bandid
        self.dirty = _dev.to_dev(ds.DIRTY.values)
        rdt = self.dirty.dtype
        self.psfhat = _dev.to_dev(ds.PSFHAT.values)
        self.psf = _dev.to_dev(ds.PSF.values, rdt)
        self.beam = _dev.to_dev(ds.BEAM.values, rdt)
        self.wsumb = ds.WSUM.values[0]
        self.model = (_dev.to_dev(ds.MODEL.values, rdt) if 'MODEL' in ds
                      else torch.zeros_like(self.dirty))
        if 'DUAL' in ds:
            self.dual = _dev.to_dev(ds.DUAL.values, rdt)
            assert tuple(self.dual.shape) == (nbasis, nmax)
        else:
            self.dual = torch.zeros((nbasis, nmax), dtype=rdt, device=self.dirty.device)
        self.residual = (_dev.to_dev(ds.RESIDUAL.values, rdt) if 'RESIDUAL' in ds
                         else self.dirty.clone())
        self.uvw = self.wgt = self.vmask = self.freq = None
        if all(k in ds for k in ('UVW', 'WEIGHT', 'VIS_MASK', 'FREQ')):
            self.uvw, self.freq = _dev.to_dev(ds.UVW.values), _dev.to_dev(ds.FREQ.values)
            self.wgt, self.vmask = _dev.to_dev(ds.WEIGHT.values), _dev.to_dev(ds.VIS_MASK.values)
        nx, ny = self.dirty.shape
        self._op = HessianPsf(self.psfhat, nx, ny, self.lastsize, beam=self.beam, sigmainv=sigmainv)

    def __call__(self, x):
        self._op.wsum = None if self.wsum is None else float(self.wsum)
        self._op.sigmainv = float(self.sigmainv)
        return self._op(x)

    def compute_residual(self, x):
        """hessian.py:236-247: dirty - _hessian_impl(beam * x, uvw, wgt, vmask, freq, None, ...)."""
        if self.uvw is not None:
            xd = _dev.to_dev(x, self.dirty.dtype)
            hx = _hessian_impl(self.beam * xd, self.uvw, self.wgt, self.vmask, self.freq, None, cell=self.cell,
                               do_wgridding=self.do_wgridding, epsilon=self.epsilon, double_accum=self.double_accum,
                               nthreads=self.nthreads, reproducible=self.reproducible)
            return _dev.host_like(self.dirty - hx, x)
        raise NotImplementedError("visibility-space residual (wgridder) is outside the PSF-convolution "
                                  "hot path; use the reference's _hessian_impl")

    def set_wsum(self, wsum):
        self.wsum = wsum


def _hessian_psf_slice(xpad, xhat, xout, psfhat, beam, lastsize, x,
                       nthreads=1, sigmainv=1, wsum=None):
    """pfb/operators/hessian.py:129-158 -- note (psfhat, beam) order."""
    if x.ndim != 2:
        raise ValueError("_hessian_psf_slice expects a 2-D image")
    return _run(psfhat, lastsize, x, xout, beam, wsum, sigmainv, fresh=True)


def hessian_psf_cube(xpad, xhat, xout, beam, psfhat, lastsize, x,
                     nthreads=1, sigmainv=1, wsum=None):
    """pfb/operators/hessian.py:254-281 -- note (beam, psfhat) order."""
    if x.ndim != 3:
        raise ValueError("hessian_psf_cube expects a (nband, nx, ny) cube")
    return _run(psfhat, lastsize, x, xout, beam, wsum, sigmainv, fresh=True)


# --------------------------------------------------- the parametrised forward step (workers/fwdbwd.py:246-252)
MIX_MAXBAND = 16          # csrc/hessparam.hip: band counts the fused mix kernels are built for


def _param_tags(dfunc, dhfunc):
    """(mode, L) when dfunc / dhfunc are the tagged closures of ONE setup_parametrisation call, else None."""
    try:
        if dfunc.adjoint or not dhfunc.adjoint or dfunc.mode != dhfunc.mode or dfunc.L is not dhfunc.L:
            return None
        return dfunc.mode, dfunc.L
    except AttributeError:
        return None


class ParamHessian:
    """A(v) = 2 dhfunc(x0, psf_convolve_cube(dfunc(x0, v))) + sigmainv v over all bands of the plan
    (workers/fwdbwd.py:246-252; dfunc, dhfunc from utils/misc.py::setup_parametrisation), evaluated as
        L^T [ e * conv(e * (L v)) / 0.5 ] + sigmainv v,      e = exp(L x0) (mode 'exp') | 1 (mode 'id')
    by pfb_hessparam_apply: two band mixes around the convolution, whose row kernels apply e and the exact factor 2.
    e is built ONCE per x0 (the closures rebuild it on every call): the operator is bound to the value of x0 at
    construction (x0 is copied); a new x0 needs a new ParamHessian, which is what pcg / power_method build per call from
    the worker's partial.  psfhat: as HessianPsf, or a PsfConvPlan.
    Callable on GPU tensors or numpy arrays of shape (nband, nx, ny); recognised by opt/pcg.py (pfb_pcg_solve_param),
    opt/power_method.py and opt/primal_dual.py::ParamGradient.  On an embedded plan e lives on the plan's grid, zero
    outside the image (the padded domain, operators/psf.py), and a call stages v like PsfConvPlan.apply.  More than 16 bands: `fused` is False and a call
    evaluates the closure composition as it stands."""

    def __init__(self, psfhat, nx, ny, lastsize, x0, sigmainv, dfunc, dhfunc):
        tags = _param_tags(dfunc, dhfunc)
        if tags is None:
            raise TypeError("dfunc / dhfunc must be the pair one setup_parametrisation call returned")
        self.mode, Lh = tags
        self.plan = plan = psfhat if isinstance(psfhat, PsfConvPlan) else plan_for(psfhat, nx, ny, lastsize)
        self.nx, self.ny = int(nx), int(ny)
        self.nb = nb = plan.nband
        self.sigmainv = float(sigmainv)
        self.dfunc, self.dhfunc = dfunc, dhfunc
        if Lh.shape != (nb, nb):
            raise ValueError(f"the parametrisation has {Lh.shape[0]} bands, the plan {nb}")
        # a private copy: e is formed from x0 once, so the operator is bound to the VALUE x0 has now, on the fused route
        # and in the fallback alike, whatever the caller does to its array afterwards (the worker's xp lives on)
        self.x0 = _dev.to_dev(x0, plan.rdtype).clone()
        if tuple(self.x0.shape) != (nb, self.nx, self.ny):
            raise ValueError(f"x0 has shape {tuple(self.x0.shape)}, operator is ({nb},{self.nx},{self.ny})")
        self.fused = nb <= MIX_MAXBAND
        self.e = None
        if not self.fused:
            return
        self.L = _dev.to_dev(Lh, plan.rdtype)
        self.LH = _dev.to_dev(np.ascontiguousarray(Lh.T), plan.rdtype)
        if self.mode == 'exp':
            from ..utils.misc import _freqmul
            self.e = torch.exp(_freqmul(Lh, self.x0))           # the closures' own statement, once
        self.e = plan.grid_beam(self.e, nb)      # embedded plan: e takes the beam's place in the padded domain (psf.py)
        nbytes = _lib.load().pfb_hessparam_work_bytes(plan.handle)
        self._work = torch.empty(nbytes, dtype=torch.uint8, device=self.x0.device)

    @property
    def dtype(self):
        return self.plan.rdtype

    def __call__(self, x, out=None):
        plan = self.plan
        xd = _dev.to_dev(x, plan.rdtype if _dev.is_numpy(x) else None)
        if xd.dtype != plan.rdtype:
            raise TypeError(f"x is {xd.dtype}, operator is {plan.rdtype}")
        if tuple(xd.shape) != (self.nb, self.nx, self.ny):
            raise ValueError(f"x has shape {tuple(xd.shape)}, operator is ({self.nb},{self.nx},{self.ny})")
        if not self.fused:           # the closure composition on the same plan: pfb_freqmul serves up to 64 bands
            res = 2 * self.dhfunc(self.x0, plan.apply(self.dfunc(self.x0, xd))) + self.sigmainv * xd
            if out is not None:
                out.copy_(res)
                res = out
            return _dev.host_like(res, x)
        buf = _dev.out_buffer(out, xd, alias=False)
        plan._on_grid('pfb_hessparam_apply', xd, buf, lambda xs, os_: (
            _dev.ptr(self.L), _dev.ptr(self.LH), _dev.ptr(self.e), self.sigmainv, _dev.ptr(xs), _dev.ptr(os_),
            _dev.ptr(self._work)))
        return _dev.host_like(_dev.deliver(buf, out), x)

    def apply_dots(self, x, out, dots_out):
        """As HessianPsf.apply_dots, the sums out of the second band mix."""
        self.plan.run('pfb_hessparam_apply_dots', _dev.ptr(self.L), _dev.ptr(self.LH), _dev.ptr(self.e), self.sigmainv,
                      _dev.ptr(x), _dev.ptr(out), _dev.ptr(x), None, _dev.ptr(dots_out), _dev.ptr(self._work))


def hessian_psf(psfo, x0, sigmainv, df, dhf, v, _nofuse=False):
    """workers/fwdbwd.py:246-252 with the worker's signature (its unused `dx0 = df(x0)` is not evaluated):
        2 * dhf(psfo(df(v))) + v * sigmainv
    so that the worker's `partial(hessian_psf, psf_convolve, xp, sigmainv, df, dhf)` can import it unchanged.  Called
    directly it evaluates exactly that composition with whatever callables it is given; pcg and power_method look at
    the partial and, when psfo is a partial of this package's psf_convolve_cube and df / dhf are partials of the
    tagged closures of setup_parametrisation over the same x0, run the fused ParamHessian instead (as_param_hessian).
    _nofuse=True (keyword of the partial) keeps the generic path."""
    # _nofuse is deliberately unused here: only as_param_hessian reads it, from the partial's keywords
    return 2 * dhf(psfo(df(v))) + v * sigmainv


def as_param_hessian(A, b):
    """The ParamHessian a `partial(hessian_psf, psfo, x0, sigmainv, df, dhf)` stands for, or None: psfo must be a
    partial of this package's psf_convolve_cube binding (xpad, xhat, xout, psfhat, lastsize), df / dhf partials of the
    two tagged closures of one setup_parametrisation call, both over the very x0 the partial carries, and x0 shaped
    like b.  Anything else -- a foreign convolution, a wrapped closure, another x0 -- is not recognised."""
    if not (isinstance(A, functools.partial) and A.func is hessian_psf and len(A.args) == 5):
        return None
    if any(A.keywords.values()) or set(A.keywords) - {'_nofuse'}:
        return None
    psfo, x0, sigmainv, df, dhf = A.args
    if not (isinstance(psfo, functools.partial) and psfo.func is psf_convolve_cube and len(psfo.args) == 5
            and not psfo.keywords):
        return None
    for f in (df, dhf):
        if not (isinstance(f, functools.partial) and len(f.args) == 1 and not f.keywords and f.args[0] is x0):
            return None
    if _param_tags(df.func, dhf.func) is None:
        return None
    psfhat, lastsize = psfo.args[3], psfo.args[4]
    if getattr(psfhat, 'ndim', 0) != 3 or tuple(getattr(x0, 'shape', ())) != tuple(b.shape) or b.ndim != 3:
        return None
    if psfhat.shape[0] != b.shape[0] or df.func.L.shape[0] != b.shape[0]:
        return None
    nx, ny = b.shape[-2:]
    return ParamHessian(psfhat, nx, ny, lastsize, x0, float(sigmainv), df.func, dhf.func)
