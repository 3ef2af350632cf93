"""
The three pfb/utils/misc.py helpers that sit on the hot path.

    norm_diff(x, xp)                      misc.py:1316-1351
    l1reweight_func(psiH, outvar, ...)    misc.py:1070-1080
    dds2cubes(dds, nband, ...)            misc.py:664-739   (cube assembly, device resident)
    freqmul(A, x), setup_parametrisation  misc.py:1366-1423 (band coupling of the fwdbwd parametrisations)
    Gaussian2D, get_padding_info, convolve2gaussres   misc.py:109-238 (restoring-beam convolution)
    fit_image_cube, eval_coeffs_to_cube, eval_coeffs_to_slice   misc.py:1084-1313 (component model, utils/comps.py)
    fitcleanbeam                          misc.py:506-584   (clean beam, utils/beamfit.py)
    restore_corrs                         misc.py:490-503   (a Stokes model column back into the correlations)
    concat_row, concat_chan, sum_overlap, sum_beam, _sum_beam   misc.py:776-1067 (the grid worker's merge, utils/concat.py)
"""
import math

import numpy as np
import torch

from .. import _lib, _dev
from .._dev import norm_diff_sums
from .._plan import PlanCache, array_key
from ..operators.psf import PsfConvPlan
from .comps import fit_image_cube, eval_coeffs_to_cube, eval_coeffs_to_slice  # noqa: F401
from .beamfit import fitcleanbeam  # noqa: F401
from .concat import VisDataset, concat_row, concat_chan, sum_overlap, sum_beam, _sum_beam  # noqa: F401


def norm_diff(x, xp):
    """sqrt(sum((x-xp)^2) / (1e-12 + sum(x^2))) with fp64 accumulation
    (misc.py:1326-1351); 2-D or 3-D input only, like the reference."""
    if x.ndim not in (2, 3):
        raise ValueError("norm_diff is only implemented for 2D or 3D arrays")
    xd, xpd = _dev.to_dev(x), _dev.to_dev(xp)
    if xd.dtype != xpd.dtype or xd.shape != xpd.shape:
        raise ValueError("norm_diff: x and xp must have the same shape and dtype")
    num, den = norm_diff_sums(xd, xpd).tolist()
    return math.sqrt(num / (1e-12 + den))


def _restore_corrs(vis, ncorr):
    """misc.py:498-503: (nrow, nchan, ncorr) of the type of vis with vis in correlations 0 and -1 and zeros between, every
    element written by one launch."""
    vd = _dev.to_dev(vis)
    if vd.dtype not in _dev.REAL_OF or vd.ndim != 2:
        raise TypeError(f"vis must be a (nrow, nchan) complex64 or complex128 array, got {vd.dtype} {tuple(vd.shape)}")
    ncorr = int(ncorr)
    if not 1 <= ncorr <= 4:
        raise ValueError(f"ncorr must be 1 .. 4, got {ncorr}")
    out = torch.empty(tuple(vd.shape) + (ncorr,), dtype=vd.dtype, device=vd.device)
    if vd.numel():
        _lib.check(_lib.load().pfb_vis_restore_corrs(_dev.code(_dev.REAL_OF[vd.dtype]), _dev.ptr(vd), vd.numel(), ncorr,
                                                     _dev.ptr(out), _dev.stream()))
    return _dev.host_like(out, vis)


restore_corrs = _restore_corrs          # the reference's name is the dask wrapper of the same function


def l1reweight_func(psiH, outvar, rmsfactor, rms_comps, model, alpha=4, group=None):
    """misc.py:1070-1080: weights (1+rmsfactor)/(1+(|sum_band psiH(model)|/rms_comps)^alpha).
    `psiH` is the analysis operator (Psi.dot) at the call site (spotless.py:243-245).
    The band-sum / power / divide run as torch device ops on the (nbasis, Nymax, Nxmax)
    plane -- executed once per reweighting, not per iteration.  group (extension): bands
    sharded over a torch.distributed group -> the band sum is all-reduced (GPU tensors)."""
    psiH(model, outvar)
    if group is not None:
        import torch.distributed as dist
        plane = torch.sum(outvar, dim=0)
        dist.all_reduce(plane, op=dist.ReduceOp.SUM, group=None if group is True else group)
        rc = rms_comps if not _dev.is_numpy(rms_comps) else torch.as_tensor(rms_comps, device=outvar.device)
        return (1 + rmsfactor) / (1 + torch.abs(plane) ** alpha / rc ** alpha)
    if _dev.is_numpy(outvar):
        mcomps = np.abs(np.sum(outvar, axis=0))
        return (1 + rmsfactor) / (1 + mcomps ** alpha / rms_comps ** alpha)
    mcomps = torch.abs(torch.sum(outvar, dim=0))
    rc = rms_comps if not _dev.is_numpy(rms_comps) else torch.as_tensor(rms_comps, device=outvar.device)
    return (1 + rmsfactor) / (1 + mcomps ** alpha / rc ** alpha)


def dds2cubes(dds, nband, apparent=False, dual=True, modelname='MODEL'):
    """pfb/utils/misc.py:664-739 -- assembles the image cubes the solvers work on, here as
    DEVICE-RESIDENT tensors (no dask graph): returns
    `(dirty, model, residual, psf, psfhat, mean_beam, wsums, dual)` with the reference's
    normalisation (dirty/residual beam-weighted unless `apparent` and, like psf/psfhat, divided by
    the TOTAL wsum; mean_beam = sum(beam*wsum)/wsums[band]; datasets sharing a band are summed,
    model/dual come from the band's last dataset; absent variables give None).  `dds` is a list of
    the reference's per-band datasets or of anything exposing DIRTY, BEAM, WSUM [, RESIDUAL, PSF,
    PSFHAT, DUAL, <modelname>] with `.values` (numpy or tensors), `bandid`, `name in ds` and
    `ds[name]`.  Reading the `.dds` zarr store itself stays with xarray/zarr (not in this image)."""
    dev = _dev.require_device()
    d0 = dds[0]
    first = _dev.to_dev(d0.DIRTY.values)
    rt = first.dtype
    ct = torch.complex64 if rt == torch.float32 else torch.complex128
    nx, ny = first.shape

    def get(ds, name, dt=rt):
        return _dev.to_dev(ds[name].values, dt)

    dirty = torch.zeros((nband, nx, ny), dtype=rt, device=dev)
    model = torch.zeros_like(dirty)
    residual = torch.zeros_like(dirty) if 'RESIDUAL' in d0 else None
    wsums = torch.zeros(nband, dtype=rt, device=dev)
    psf = psfhat = None
    if 'PSF' in d0:
        psf = torch.zeros((nband,) + tuple(d0['PSF'].values.shape), dtype=rt, device=dev)
        psfhat = torch.zeros((nband,) + tuple(d0['PSFHAT'].values.shape), dtype=ct, device=dev)
    mean_beam = torch.zeros_like(dirty)
    dualc = (torch.zeros((nband,) + tuple(d0['DUAL'].values.shape), dtype=rt, device=dev)
             if (dual and 'DUAL' in d0) else None)
    for ds in dds:
        b = ds.bandid
        beam = get(ds, 'BEAM')
        w = float(ds['WSUM'].values[0])
        dirty[b] += get(ds, 'DIRTY') if apparent else get(ds, 'DIRTY') * beam
        if 'RESIDUAL' in ds:
            residual[b] += get(ds, 'RESIDUAL') if apparent else get(ds, 'RESIDUAL') * beam
        if 'PSF' in ds:
            psf[b] += get(ds, 'PSF')
            psfhat[b] += get(ds, 'PSFHAT', ct)
        if modelname in ds:
            model[b] = get(ds, modelname)
        if dual and 'DUAL' in ds:
            dualc[b] = get(ds, 'DUAL')
        mean_beam[b] += beam * w
        wsums[b] += w
    wsum = wsums.sum()
    dirty /= wsum
    if residual is not None:
        residual /= wsum
    if psf is not None:
        psf /= wsum
        psfhat /= wsum
    nz = wsums != 0
    mean_beam[nz] /= wsums[nz][:, None, None]
    return dirty, model, residual, psf, psfhat, mean_beam, wsums, dualc


def _freqmul(A, x, pre=None, post=None):
    lib = _lib.load()
    xd = _dev.to_dev(x)
    Ad = _dev.to_dev(A, xd.dtype)
    out = torch.empty_like(xd)
    nband = xd.shape[0]
    if tuple(Ad.shape) != (nband, nband):
        raise ValueError(f"A must be ({nband},{nband})")
    _lib.check(lib.pfb_freqmul(_dev.code(xd.dtype), _dev.ptr(Ad), _dev.ptr(xd), _dev.ptr(out), nband,
                               xd[0].numel(), _dev.ptr(pre), _dev.ptr(post), _dev.stream()))
    return out


def freqmul(A, x):
    """misc.py:1366-1375: out[k] = sum_l A[k, l] x[l] for an (nband, nx, ny) cube, on the GPU."""
    return _dev.host_like(_freqmul(A, x), x)


def setup_parametrisation(mode='id', minval=1e-5, sigma=1.0, freq=None, lscale=1.0):
    """misc.py:1378-1423: x = f(s) with a squared-exponential band covariance K = L L^T.  Returns
    (func, finv, dfunc, dhfunc) working on GPU tensors or numpy cubes; the nband x nband factor is
    built on the host (numpy Cholesky), every cube-sized operation is one pfb_freqmul launch (the
    exp / product factors of mode='exp' fused into it).  finv applies L^-1 through the same kernel
    (the reference's scipy.solve_triangular on the cube).  dfunc and dhfunc carry `mode`, the host factor `L` and
    `adjoint` (False / True) as attributes."""
    nu = np.asarray(freq, dtype=np.float64) / np.mean(freq)
    nband = nu.size
    K = sigma ** 2 * np.exp(-(nu[:, None] - nu[None, :]) ** 2 / (2 * lscale ** 2))
    L = np.linalg.cholesky(K + 1e-10 * np.eye(nband))
    LH = np.ascontiguousarray(L.T)
    Linv = np.linalg.solve(L, np.eye(nband))

    if mode == 'id':
        def func(x):
            return _dev.host_like(_freqmul(L, x), x)

        def finv(x):
            return _dev.host_like(_freqmul(Linv, x), x)

        def dfunc(x0, v):
            return _dev.host_like(_freqmul(L, v), v)

        def dhfunc(x0, v):
            return _dev.host_like(_freqmul(LH, v), v)
    elif mode == 'exp':
        def func(x):
            return _dev.host_like(torch.exp(_freqmul(L, x)), x)

        def finv(x):
            t = _freqmul(Linv, x)
            return _dev.host_like(torch.log(torch.clamp(torch.abs(t), min=minval)), x)

        def dfunc(x0, v):
            e = torch.exp(_freqmul(L, x0))
            return _dev.host_like(_freqmul(L, v, post=e), v)         # exp(L x0) * (L v)

        def dhfunc(x0, v):
            e = torch.exp(_freqmul(L, x0))
            return _dev.host_like(_freqmul(LH, v, pre=e), v)         # L^T (v * exp(L x0))
    else:
        raise ValueError(f"Unknown mode - {mode}")
    # what operators/hessian.py::ParamHessian (and through it the fused PCG) needs to know about the two closures
    dfunc.mode, dfunc.L, dfunc.adjoint = mode, L, False
    dhfunc.mode, dhfunc.L, dhfunc.adjoint = mode, L, True
    return func, finv, dfunc, dhfunc


# ------------------------------------------------------------------ Gaussian restoring beam
# pfb/utils/misc.py:109-238.  The kernels (csrc/restore.hip) synthesise the Gaussian in fp64 and gather it straight
# onto the grid of a PsfConvPlan; the convolution is that plan's (DESIGN "Restoring beam").
def _gauss_sets(gausspars, nsigma=5):
    """(nset, 4) float64 rows [a00, a01, a11, extent] -- R^T A R and the truncation radius squared, computed on the
    host exactly as misc.py:110-123 does."""
    rows = []
    for S0, S1, PA in gausspars:
        Smaj, Smin = S0, S1
        A = np.array([[1. / Smin ** 2, 0],
                      [0, 1. / Smaj ** 2]])
        c, s, t = np.cos, np.sin, np.deg2rad(-PA)
        R = np.array([[c(t), -s(t)],
                      [s(t), c(t)]])
        A = np.dot(np.dot(R.T, A), R)
        rows.append((A[0, 0], A[0, 1], A[1, 1], (nsigma * Smaj) ** 2))
    return np.array(rows, dtype=np.float64)


def _pars_dev(gausspars, nsigma=5):
    return torch.from_numpy(_gauss_sets(gausspars, nsigma)).to(_dev.require_device())


def _gauss_sums(xd, yd, pars):
    """Device fp64 vector: the sum of the unnormalised Gaussian2D of every parameter set."""
    sums = torch.empty(pars.shape[0], dtype=torch.float64, device=xd.device)
    _lib.check(_lib.load().pfb_gauss2d(_dev.ptr(xd), _dev.ptr(yd), xd.numel(), _dev.ptr(pars), pars.shape[0], 0,
                                       None, _dev.ptr(sums), _dev.ptr(_dev.scratch()[0]), _dev.stream()))
    return sums


def Gaussian2D(xin, yin, GaussPar=(1., 1., 0.), normalise=True, nsigma=5):
    """misc.py:109-138: elliptical Gaussian with FWHMs / position angle GaussPar = (emaj, emin, pa) on the caller's
    coordinates, zero beyond the radius nsigma * emaj; float64 in the shape of xin.  numpy in -> numpy out, device
    tensors stay on the device."""
    xd, yd = _dev.to_dev(xin, torch.float64), _dev.to_dev(yin, torch.float64)
    if xd.shape != yd.shape:
        raise ValueError(f"xin {tuple(xd.shape)} and yin {tuple(yd.shape)} differ in shape")
    pars = _pars_dev([GaussPar], nsigma)
    out = torch.empty((1,) + tuple(xd.shape), dtype=torch.float64, device=xd.device)
    sums = torch.empty(1, dtype=torch.float64, device=xd.device)
    _lib.check(_lib.load().pfb_gauss2d(_dev.ptr(xd), _dev.ptr(yd), xd.numel(), _dev.ptr(pars), 1, int(bool(normalise)),
                                       _dev.ptr(out), _dev.ptr(sums), _dev.ptr(_dev.scratch()[0]), _dev.stream()))
    return _dev.host_like(out[0], xin)


def good_size(n, real=True):
    """The smallest 5-smooth integer >= n: what ducc0.fft.good_size(n, True) returns (misc.py:172,177)."""
    n = max(int(n), 1)
    best = None
    p5 = 1
    while best is None or p5 < best:
        p35 = p5
        while best is None or p35 < best:
            m = p35
            while m < n:
                m *= 2
            if best is None or m < best:
                best = m
            p35 *= 3
        p5 *= 5
    return best


def get_padding_info(nx, ny, pfrac):
    """misc.py:170-183."""
    npad_x = int(pfrac * nx)
    nfft = good_size(nx + npad_x, True)
    npad_xl = (nfft - nx) // 2
    npad_xr = nfft - nx - npad_xl

    npad_y = int(pfrac * ny)
    nfft = good_size(ny + npad_y, True)
    npad_yl = (nfft - ny) // 2
    npad_yr = nfft - ny - npad_yl
    padding = ((0, 0), (npad_xl, npad_xr), (npad_yl, npad_yr))
    unpad_x = slice(npad_xl, -npad_xr)
    unpad_y = slice(npad_yl, -npad_yr)
    return padding, unpad_x, unpad_y


def _even_smooth(n):
    """Smallest even 13-smooth integer >= n (the lengths pfb_psfconv_plan_create takes)."""
    m = n + (n & 1)
    while True:
        r = m
        for p in (2, 3, 5, 7, 11, 13):
            while r % p == 0:
                r //= p
        if r == 1:
            return m
        m += 2


def _engine_grid(nx, ny, rdtype):
    """(plan image shape, kernel grid) a restoring-beam kernel for (nx, ny) images is gathered onto: the power-of-two
    fast path of the convolution with its 2x grid whenever the image fits it, else the image itself on the smallest
    even 13-smooth grid that holds every offset (>= 2 n - 1).  Only this module's plans use it."""
    from ..operators.psf import _pow2ceil, NX_FAST_MAX, NY_FAST_MAX
    nx2, ny2 = max(64, _pow2ceil(nx)), max(128, _pow2ceil(ny))
    if nx2 <= NX_FAST_MAX and ny2 <= NY_FAST_MAX[rdtype]:
        return (nx2, ny2), (2 * nx2, 2 * ny2)
    return (nx, ny), (_even_smooth(2 * nx - 1), _even_smooth(2 * ny - 1))


class _BeamPlan:
    """A PsfConvPlan holding restoring-beam kernels for (nx, ny) images -- an embedded one where the engine grid is
    larger than the image.  `shared` (model branch of convolve2gaussres): the plan has one band that serves every band
    of the cube; otherwise band b of the cube meets kernel b."""

    def __init__(self, plan, shared):
        self.plan, self.shared = plan, shared

    def apply(self, x):
        """x: (nb, nx, ny) contiguous device tensor of the plan's dtype -> new tensor, x untouched."""
        out = torch.empty_like(x)
        if self.shared:
            for b in range(x.shape[0]):
                self.plan.apply(x[b:b + 1], out=out[b:b + 1])
        else:
            self.plan.apply(x, out=out)
        return out


_beam_cache = PlanCache(4)


def clear_beam_cache():
    _beam_cache.clear()


def _coord_key(a):
    """Content fingerprint of a coordinate array (the caller may rebuild xx, yy for every call): shape, dtype and a
    strided sample for numpy; identity + version (array_key) for a device tensor, which the cache entry keeps alive."""
    if isinstance(a, np.ndarray):
        # no address in this key, on purpose: the rebuilt xx, yy of the next call are the same coordinates elsewhere
        flat = a.reshape(-1)
        samp = flat[::max(1, flat.size // 257)][:257]
        return ('np', a.shape, str(a.dtype), float(flat[0]), float(flat[-1]), float(samp.sum()))
    return array_key(a)


def _model_plan(xd, yd, gausspars, nx, ny, rdtype, pfrac, norm_kernel):
    """Plan with one band per entry of gausspars: kernel b is Gaussian2D(xx, yy, gausspars[b], norm_kernel) padded as
    misc.py:206-211 pads it, gathered onto the engine grid."""
    padding, _, _ = get_padding_info(nx, ny, pfrac)
    P, Q = nx + sum(padding[1]), ny + sum(padding[2])
    (pnx, pny), (P2, Q2) = _engine_grid(nx, ny, rdtype)
    pars = _pars_dev(gausspars)
    norm = _gauss_sums(xd, yd, pars) if norm_kernel else None
    k2 = torch.empty((len(gausspars), P2, Q2), dtype=rdtype, device=xd.device)
    _lib.check(_lib.load().pfb_gauss_kernel_grid(_dev.code(rdtype), _dev.ptr(xd), _dev.ptr(yd), nx, ny, padding[1][0],
                                                 padding[2][0], P, Q, _dev.ptr(pars), _dev.ptr(norm), len(gausspars),
                                                 1, P2, Q2, _dev.ptr(k2), _dev.stream()))
    return PsfConvPlan.from_psf(k2, pnx, pny, image=(nx, ny))


def _ratio_plan(xd, yd, gaussparf, gausspari, nx, ny, rdtype, pfrac, norm_kernel):
    """Plan whose band b multiplies by gausskernhat / thiskernhat_b (misc.py:223-233) on the reference's own
    (P, Q) grid -- the ratio is defined per frequency of THAT grid."""
    from ..operators.fft import psfhat_from_psf
    lib = _lib.load()
    nband = len(gausspari)
    padding, _, _ = get_padding_info(nx, ny, pfrac)
    P, Q = nx + sum(padding[1]), ny + sum(padding[2])
    pars = _pars_dev([gaussparf] + list(gausspari))
    norm = _gauss_sums(xd, yd, pars) if norm_kernel else None
    kpad = torch.empty((nband + 1, P, Q), dtype=torch.float64, device=xd.device)
    _lib.check(lib.pfb_gauss_kernel_grid(_lib.PFB_F64, _dev.ptr(xd), _dev.ptr(yd), nx, ny, padding[1][0], padding[2][0],
                                         P, Q, _dev.ptr(pars), _dev.ptr(norm), nband + 1, 0, P, Q, _dev.ptr(kpad),
                                         _dev.stream()))
    khat = psfhat_from_psf(kpad)
    del kpad
    ratio = torch.empty((nband, P, Q // 2 + 1), dtype=torch.complex128, device=xd.device)
    _lib.check(lib.pfb_kernhat_ratio(_dev.ptr(khat[0]), _dev.ptr(khat[1:]), nband, P * (Q // 2 + 1), _dev.ptr(ratio),
                                     _dev.stream()))
    del khat
    if Q % 2 == 0:
        return PsfConvPlan(ratio.to(_dev.CPLX_OF[rdtype]), nx, ny, Q)
    # odd Q: no plan takes the spectrum; back to image space (plan time, as operators/fft.py does for odd grids) and
    # onto the engine grid like the model branch
    kern = torch.fft.irfft2(ratio, s=(P, Q), dim=(-2, -1)).contiguous()
    del ratio
    (pnx, pny), (P2, Q2) = _engine_grid(nx, ny, rdtype)
    k2 = torch.empty((nband, P2, Q2), dtype=rdtype, device=xd.device)
    _lib.check(lib.pfb_kernel_gather(_dev.code(rdtype), _dev.ptr(kern), nband, nx, ny, P, Q, 0, 0, P2, Q2,
                                     _dev.ptr(k2), _dev.stream()))
    return PsfConvPlan.from_psf(k2, pnx, pny, image=(nx, ny))


def _beam_plan(xx, yy, coord_key, gaussparf, gausspari, nx, ny, rdtype, pfrac, norm_kernel, per_band=False):
    """Cached _BeamPlan.  gaussparf: one parameter triple -- or, with per_band, one per band
    (restore_image's model step); gausspari: None (model branch) or one triple per band (ratio branch).  xx, yy may be
    callables that build the coordinates: they are only needed on a miss."""
    tup = lambda g: tuple(float(v) for v in g)
    gpf = tuple(tup(g) for g in gaussparf) if per_band else tup(gaussparf)
    gpi = None if gausspari is None else tuple(tup(g) for g in gausspari)
    key = (gpf, gpi, coord_key, (nx, ny), str(rdtype), float(pfrac), bool(norm_kernel), per_band)

    def make():
        xs, ys = (xx(), yy()) if callable(xx) else (xx, yy)
        xd, yd = _dev.to_dev(xs, torch.float64), _dev.to_dev(ys, torch.float64)
        if tuple(xd.shape) != (nx, ny) or tuple(yd.shape) != (nx, ny):
            raise ValueError(f"xx {tuple(xd.shape)} / yy {tuple(yd.shape)} must have the image's shape ({nx}, {ny})")
        if gpi is not None:
            plan = _ratio_plan(xd, yd, gpf, gpi, nx, ny, rdtype, pfrac, norm_kernel)
        else:
            plan = _model_plan(xd, yd, gpf if per_band else [gpf], nx, ny, rdtype, pfrac, norm_kernel)
        # device coordinate tensors are kept so that their address cannot be re-used by others while the entry lives
        keep = [a for a in (xs, ys) if isinstance(a, torch.Tensor)]
        return _BeamPlan(plan, shared=gpi is None and not per_band), keep
    return _beam_cache.get(key, make)[0]


def _convolve_dev(img, bp):
    if img.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"image must be float32 or float64, got {img.dtype}")
    return bp.apply(img.contiguous())


def convolve2gaussres(image, xx, yy, gaussparf, nthreads, gausspari=None, pfrac=0.5, norm_kernel=False):
    """misc.py:186-238: convolve an (nband, nx, ny) cube to the resolution gaussparf = (emaj, emin, pa); with
    gausspari (one triple per band: the resolution the bands already have) by the RATIO of the kernel spectra instead.
    xx, yy: (nx, ny) coordinates in the unit of the Gaussian parameters.  Returns a new array of the image's dtype
    (numpy in -> numpy out, device tensors stay on the device); `image` is not modified; nthreads is ignored.
    The kernel is built once per (beam, coordinates, shape, dtype, pfrac, norm_kernel) and cached.
    Like the reference's, the ratio is noise over noise wherever the initial kernel's spectrum has decayed to rounding
    level (initial FWHM above ~3 pixels): see DESIGN "Restoring beam"."""
    if image.ndim != 3:
        raise ValueError("convolve2gaussres expects an (nband, nx, ny) image")
    img = _dev.to_dev(image)
    nband, nx, ny = (int(v) for v in img.shape)
    if gausspari is not None and len(gausspari) != nband:
        raise ValueError(f"gausspari has {len(gausspari)} entries for {nband} bands")
    bp = _beam_plan(xx, yy, (_coord_key(xx), _coord_key(yy)), gaussparf, gausspari, nx, ny, img.dtype, pfrac,
                    norm_kernel)
    return _dev.host_like(_convolve_dev(img, bp), image)
