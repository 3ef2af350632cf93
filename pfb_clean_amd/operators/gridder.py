"""
The w-gridder on MI355X -- ducc0.wgridder.experimental.vis2dirty / dirty2vis as pfb/operators/hessian.py:62-106 calls
them, with ducc0's names and defaults.  The operators are the direct Fourier sums stated in include/pfb_hip.h
("w-gridder"); they are evaluated by w-stacking on a twice oversampled grid with the kernel
exp(2.3 W (sqrt(1 - x^2) - 1)) of W = ceil(log10(1/epsilon)) + 2 cells:

    vis2dirty   per w plane: grid (pfb_wgrid_grid), unnormalised inverse c2c, window and w phase
                (pfb_wgrid_image_adjoint); at the end the kernel correction with 1/n (pfb_wgrid_image_correct)
    dirty2vis   the adjoint, step by step: pfb_wgrid_image_forward, forward c2c, pfb_wgrid_degrid

The c2c transform of a plane is torch.fft (the precedent of operators/fft.py); everything else is csrc/wgrid.hip.

A WgridPlan holds what one (uvw, freq, mask) set and one image geometry share between calls: support, planes, the
correction tables and the visibilities' sorted order.  Plans live in a PlanCache: a major cycle that presents the same
arrays again builds nothing.  numpy in gives numpy out, tensors in give tensors out; there is no CPU path.

image_data_products (pfb/operators/gridder.py:551-740) composes these with utils/weighting.py into the grid worker's
products: WEIGHT, WSUM, DIRTY, PSF, PSFHAT and RESIDUAL of one band.
"""
import ctypes as C
import math

import numpy as np
import torch

from .. import _dev, _lib
from .._plan import NativePlan, PlanCache, array_key
from ..utils import weighting
from .fft import psfhat_from_psf

C_LIGHT = 299792458.0
EPS_MAX = 1e-2
# lower bounds of epsilon: fp64 by the support range of the kernels (W <= 12); fp32 measured: the lowest decade tried
# (1e-3, 1e-4, 1e-5) at which every case of tests/wgrid_cases.py stays under epsilon / 3 on the MI355X
EPS_MIN = {torch.float64: 1e-10, torch.float32: 1e-5}
_QUAD_NODES = 128


def support_for(epsilon):
    """W = ceil(log10(1 / epsilon)) + 2 (a whole decade is not pushed up by the rounding of the logarithm)."""
    return int(math.ceil(-math.log10(epsilon) - 1e-9)) + 2


def check_epsilon(epsilon, rdtype):
    eps = float(epsilon)
    lo = EPS_MIN[rdtype]
    if not (lo * (1 - 1e-12) <= eps <= EPS_MAX * (1 + 1e-12)):
        raise ValueError(f"epsilon {eps:g} outside the supported range [{lo:g}, {EPS_MAX:g}] for {rdtype}")
    return eps


def _quadrature(W):
    """(x, f) of the correction integral below: the Gauss-Legendre nodes in theta as x = sin(theta) -- a node's
    frequency in t is 2 pi h x -- and phi(x) cos(theta) times the node's weight."""
    th, wq = np.polynomial.legendre.leggauss(_QUAD_NODES)
    th, wq = th * (np.pi / 2), wq * (np.pi / 2)
    return np.sin(th), np.exp(2.3 * W * (np.cos(th) - 1.0)) * np.cos(th) * wq


def kernel_correction(W, t):
    """c(t) = h int_-1^1 phi(x) cos(2 pi h t x) dx, h = W / 2, phi(x) = exp(2.3 W (sqrt(1 - x^2) - 1)): Gauss-Legendre
    in theta, x = sin(theta), where the integrand is smooth up to the ends.  fp64 on the host."""
    t = np.asarray(t, dtype=np.float64)
    h = 0.5 * W
    x, f = _quadrature(W)
    return h * (np.cos(2 * np.pi * h * t[..., None] * x) * f).sum(-1)


def _kernel_correction_dev(W, t):
    """kernel_correction on a device fp64 tensor, node by node: the (nx, ny) table of the w axis is summed where it
    will live instead of as an (nx, ny, nodes) array on the host."""
    h = 0.5 * W
    x, f = _quadrature(W)
    acc = torch.zeros_like(t)
    for a, fq in zip(2 * np.pi * h * x, f):
        acc.add_(torch.cos(t * float(a)), alpha=float(fq))
    return acc.mul_(h)


def image_lmn(nx, ny, pixsize_x, pixsize_y, center_x, center_y):
    """(l, m, nm1) of the pixel grid: l (nx, 1), m (1, ny), nm1 (nx, ny)."""
    l = ((np.arange(nx) - nx // 2) * pixsize_x + center_x)[:, None]
    m = ((np.arange(ny) - ny // 2) * pixsize_y + center_y)[None, :]
    r2 = l * l + m * m
    if r2.max() >= 1.0:
        raise ValueError("the image reaches beyond the horizon (l^2 + m^2 >= 1)")
    return l, m, -r2 / (1.0 + np.sqrt(1.0 - r2))


def plane_layout(wmin, wmax, max_nm1, W, epsilon, do_wgridding):
    """(nplanes, w0, dw): planes at w0 + p dw.  One plane -- no w kernel -- without w-gridding (at w = 0) and where the
    w term cannot matter: the phase it leaves, pi max|nm1| (wmax - wmin), is below epsilon / 100 (at the mid w)."""
    if not do_wgridding:
        return 1, 0.0, 1.0
    if math.pi * max_nm1 * (wmax - wmin) <= 0.01 * epsilon:
        return 1, 0.5 * (wmin + wmax), 1.0
    dw = 1.0 / (4.0 * max_nm1)
    # a visibility at plane coordinate g = (w - w0) / dw touches planes ceil(g - h) .. + W - 1, g in [h, h + range / dw];
    # one plane to spare for the rounding of g at wmax
    return int(math.ceil((wmax - wmin) / dw)) + W + 1, wmin - 0.5 * W * dw, dw


class WgridPlan(NativePlan):
    """One (uvw, freq, mask) set on one image geometry: the native geometry record, the sorted order (idx, coord, the
    planes' slot ranges), nm1 and the correction tables, and the per-call buffers (one grid, val / acc, the complex
    image).  Use through vis2dirty / dirty2vis / hessian, which hold `lock`."""
    _destroy = 'pfb_wgrid_plan_destroy'

    def __init__(self, uvw, freq, mask, nx, ny, pixsize_x, pixsize_y, center_x, center_y, epsilon, do_wgridding, rdtype):
        super().__init__()
        dev = _dev.require_device()
        nx, ny = int(nx), int(ny)
        if nx < 2 or ny < 2 or nx % 2 or ny % 2:
            raise ValueError(f"npix_x, npix_y must be even (got {nx}, {ny})")
        self.rdtype, self.cdtype = rdtype, _dev.CPLX_OF[rdtype]
        self.epsilon = check_epsilon(epsilon, rdtype)
        self.W = W = support_for(self.epsilon)
        self.nx, self.ny = nx, ny
        self.do_wgridding = bool(do_wgridding)
        self.uvw, self.freq = _dev.uvw_freq(uvw, freq)
        self.nrow, self.nchan = int(self.uvw.shape[0]), int(self.freq.shape[0])
        self.nvis = self.nrow * self.nchan
        self.mask = None if mask is None else _dev.byte_mask(mask, (self.nrow, self.nchan))
        if self.do_wgridding:
            nm1 = image_lmn(nx, ny, pixsize_x, pixsize_y, center_x, center_y)[2]
        else:
            nm1 = np.zeros((nx, ny))            # without w-gridding nm1 := 0 and n := 1
        # ---- the w range of the unmasked visibilities -> planes
        self.nsorted = 0
        w = self.uvw[:, 2:3] * self.freq[None, :] / C_LIGHT
        if self.mask is not None:
            w = w[self.mask != 0]
        if self.nvis == 0 or w.numel() == 0:
            return                      # nothing to grid: every call answers zeros without a launch
        wmin, wmax = w.min().item(), w.max().item()
        del w
        if not (math.isfinite(wmin) and math.isfinite(wmax)):
            raise ValueError("uvw / freq hold a non-finite value")
        self.nplanes, self.w0, self.dw = plane_layout(wmin, wmax, float(np.abs(nm1).max()), W, self.epsilon,
                                                      self.do_wgridding)
        tu = (np.arange(nx) - nx // 2) / (2.0 * nx)
        tv = (np.arange(ny) - ny // 2) / (2.0 * ny)
        cuv = kernel_correction(W, tu)[:, None] * kernel_correction(W, tv)[None, :]
        self.nm1 = torch.from_numpy(np.ascontiguousarray(nm1)).to(dev) if self.do_wgridding else None
        self._corr1 = 1.0 / torch.from_numpy(cuv).to(dev)
        if self.nplanes > 1:
            self._corr1 /= _kernel_correction_dev(W, self.dw * self.nm1)
        self._corr = {}
        _lib.check(self._lib.pfb_wgrid_plan_create(_dev.code(rdtype), nx, ny, float(pixsize_x), float(pixsize_y),
                                                   float(center_x), float(center_y), W, self.nplanes, self.w0, self.dw,
                                                   C.byref(self._h)))
        nkeys, np0, tile = C.c_int(), C.c_int(), C.c_int()
        _lib.check(self._lib.pfb_wgrid_plan_info(self._h, C.byref(nkeys), C.byref(np0), C.byref(tile)))
        self.nkeys, self.np0, self.tile = nkeys.value, np0.value, tile.value
        self._build_order(dev)
        self._grid = torch.empty((2 * nx, 2 * ny), dtype=self.cdtype, device=dev)
        self._slots = torch.empty((2, self.nsorted), dtype=self.cdtype, device=dev)
        self._img = torch.empty((nx, ny), dtype=self.cdtype, device=dev)

    def _build_order(self, dev):
        """Counting sort by (first plane, uv tile): histogram kernel, torch.cumsum, placement kernel.  One number -- the
        count of unmasked visibilities -- and the planes' offsets cross to the host."""
        work = torch.empty(self._lib.pfb_wgrid_work_bytes(self._h), dtype=torch.uint8, device=dev)
        keys = torch.empty(self.nvis, dtype=torch.int32, device=dev)
        self.run('pfb_wgrid_order_count', _dev.ptr(self.uvw), _dev.ptr(self.freq), _dev.ptr(self.mask), self.nrow,
                 self.nchan, _dev.ptr(keys), _dev.ptr(work))
        counts = work[:4 * self.nkeys].view(torch.int32)
        offsets = torch.zeros(self.nkeys + 1, dtype=torch.int64, device=dev)
        offsets[1:] = torch.cumsum(counts, 0, dtype=torch.int64)
        self.plane_off = offsets[::self.nkeys // self.np0].cpu().tolist()        # np0 + 1 entries
        self.nsorted = self.plane_off[-1]
        self.idx = torch.empty(self.nsorted, dtype=torch.int32, device=dev)
        self.coord = torch.empty((3, self.nsorted), dtype=torch.float64, device=dev)
        self.run('pfb_wgrid_order_fill', _dev.ptr(self.uvw), _dev.ptr(self.freq), self.nrow, self.nchan, _dev.ptr(keys),
                 _dev.ptr(offsets), _dev.ptr(work), self.nsorted, _dev.ptr(self.idx), _dev.ptr(self.coord))

    # ------------------------------------------------------------------------------------------------ pieces
    def corr(self, divide_by_n):
        """1 / (c_u c_v c_w) [/ n] as a device fp64 table."""
        key = bool(divide_by_n) and self.do_wgridding            # without w-gridding n := 1
        if key not in self._corr:
            self._corr[key] = (self._corr1 / (1.0 + self.nm1)).contiguous() if key else self._corr1.contiguous()
        return self._corr[key]

    def plane_ranges(self):
        """(plane, s0, s1) of every plane that has slots: first planes p - W + 1 .. p."""
        off = self.plane_off
        for p in range(self.nplanes):
            s0, s1 = off[max(0, p - self.W + 1)], off[min(p, self.np0 - 1) + 1]
            if s1 > s0:
                yield p, s0, s1

    def _check(self, name, t, dtype, shape):
        if t is None:
            return
        if t.dtype != dtype or tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} must be {dtype} of shape {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")

    def _degrid_all(self, x, beam, divide_by_n):
        """acc (the first slot vector) = the footprint sums of every slot over all planes, from image x."""
        g = self._grid
        acc = self._slots[0]
        acc.zero_()
        corr = self.corr(divide_by_n)
        for p, s0, s1 in self.plane_ranges():
            self.run('pfb_wgrid_image_forward', p, _dev.ptr(x), _dev.ptr(beam), _dev.ptr(corr), _dev.ptr(self.nm1),
                     _dev.ptr(g))
            gh = torch.fft.fft2(g).contiguous()       # a fresh tensor: `out=` costs a copy of the grid per transform
            self.run('pfb_wgrid_degrid', p, _dev.ptr(gh), _dev.ptr(self.coord), self.nsorted, s0, s1, _dev.ptr(acc))
        return acc

    def _grid_all(self, val, beam, divide_by_n):
        """The (nx, ny) real image of the slot values `val`, corrected."""
        g = self._grid
        self._img.zero_()
        for p, s0, s1 in self.plane_ranges():
            self.run('pfb_wgrid_grid', p, _dev.ptr(val), _dev.ptr(self.coord), self.nsorted, s0, s1, _dev.ptr(g))
            gh = torch.fft.ifft2(g, norm='forward').contiguous()
            self.run('pfb_wgrid_image_adjoint', p, _dev.ptr(gh), _dev.ptr(self.nm1), _dev.ptr(self._img))
        out = torch.empty((self.nx, self.ny), dtype=self.rdtype, device=val.device)
        self.run('pfb_wgrid_image_correct', _dev.ptr(self._img), _dev.ptr(self.corr(divide_by_n)), _dev.ptr(beam),
                 _dev.ptr(out))
        return out

    # ---------------------------------------------------------------------------------------------- operators
    def vis2dirty(self, vis, wgt=None, divide_by_n=True):
        self._check('vis', vis, self.cdtype, (self.nrow, self.nchan))
        self._check('wgt', wgt, self.rdtype, (self.nrow, self.nchan))
        if self.nsorted == 0:
            return torch.zeros((self.nx, self.ny), dtype=self.rdtype, device=vis.device)
        with self.lock:
            val = self._slots[1]
            self.run('pfb_wgrid_prep', _dev.ptr(vis), _dev.ptr(wgt), _dev.ptr(self.idx), _dev.ptr(self.coord),
                     self.nsorted, _dev.ptr(val))
            return self._grid_all(val, None, divide_by_n)

    def dirty2vis(self, dirty, wgt=None, divide_by_n=True):
        self._check('dirty', dirty, self.rdtype, (self.nx, self.ny))
        self._check('wgt', wgt, self.rdtype, (self.nrow, self.nchan))
        if self.nsorted == 0:
            return torch.zeros((self.nrow, self.nchan), dtype=self.cdtype, device=dirty.device)
        vis = torch.empty((self.nrow, self.nchan), dtype=self.cdtype, device=dirty.device)
        with self.lock:
            acc = self._degrid_all(dirty, None, divide_by_n)
            self.run('pfb_wgrid_finish', _dev.ptr(acc), _dev.ptr(wgt), _dev.ptr(self.idx), _dev.ptr(self.coord),
                     self.nsorted, _dev.ptr(vis), self.nvis)
        return vis

    def hessian(self, x, wgt=None, beam=None):
        """beam * vis2dirty(wgt * dirty2vis(beam * x)), divide_by_n=False both ways (hessian.py:62-106): the
        visibilities stay in sorted slots between the two halves and the beam rides in the image-side kernels."""
        self._check('x', x, self.rdtype, (self.nx, self.ny))
        self._check('weight', wgt, self.rdtype, (self.nrow, self.nchan))
        self._check('beam', beam, self.rdtype, (self.nx, self.ny))
        if self.nsorted == 0:
            return torch.zeros_like(x)
        with self.lock:
            acc = self._degrid_all(x, beam, False)
            val = self._slots[1]
            self.run('pfb_wgrid_weight', _dev.ptr(acc), _dev.ptr(wgt), _dev.ptr(self.idx), self.nsorted, _dev.ptr(val))
            return self._grid_all(val, beam, False)


# ------------------------------------------------------------------------------------------------------ plan cache
_cache = PlanCache(8)
cache_stats = {'miss': 0}           # plans built (each builds one order): the tests count these


def plan_for(uvw, freq, mask, nx, ny, pixsize_x, pixsize_y, center_x, center_y, epsilon, do_wgridding, rdtype):
    """The cached plan of these arrays on this geometry.  The arrays are keyed by _plan.array_key (numpy: address, layout
    and a strided content sample; tensors: data_ptr and version counter); the entry keeps the arrays alive, so that
    their memory cannot come back as DIFFERENT data under the same key (clear_plan_cache() releases plans and
    references)."""
    key = (array_key(uvw), array_key(freq), array_key(mask), int(nx), int(ny), float(pixsize_x), float(pixsize_y),
           float(center_x), float(center_y), float(epsilon), bool(do_wgridding), str(rdtype))

    def make():
        cache_stats['miss'] += 1
        return (WgridPlan(uvw, freq, mask, nx, ny, pixsize_x, pixsize_y, center_x, center_y, epsilon, do_wgridding,
                          rdtype), (uvw, freq, mask))
    return _cache.get(key, make)[0]


def clear_plan_cache():
    _cache.clear()


# ---------------------------------------------------------------------------------------------------- ducc0's API
def _check_flags(do_wgridding, epsilon, pixsize_x, pixsize_y):
    if do_wgridding is None or epsilon is None or pixsize_x is None or pixsize_y is None:
        raise TypeError("pixsize_x, pixsize_y, epsilon and do_wgridding are required")


def vis2dirty(uvw, freq, vis, wgt=None, mask=None, npix_x=None, npix_y=None, pixsize_x=None, pixsize_y=None,
              center_x=0.0, center_y=0.0, epsilon=None, do_wgridding=None, divide_by_n=True,
              double_precision_accumulation=False, nthreads=1):
    """ducc0.wgridder.experimental.vis2dirty: dirty (npix_x, npix_y) in the real type of vis.  `nthreads` is accepted
    and ignored.  double_precision_accumulation with complex64 input runs the fp64 kernels on the data cast up."""
    _check_flags(do_wgridding, epsilon, pixsize_x, pixsize_y)
    if npix_x is None or npix_y is None:
        raise TypeError("npix_x and npix_y are required")
    vd = _dev.to_dev(vis)
    if vd.dtype not in _dev.REAL_OF:
        raise TypeError(f"vis must be complex64 or complex128, got {vd.dtype}")
    rdt_in = _dev.REAL_OF[vd.dtype]
    wd = _dev.to_dev(wgt)
    if wd is not None and wd.dtype != rdt_in:
        raise TypeError(f"wgt must be {rdt_in} for {vd.dtype} visibilities, got {wd.dtype}")
    rdt = torch.float64 if double_precision_accumulation else rdt_in
    if rdt != rdt_in:
        vd, wd = vd.to(torch.complex128), (None if wd is None else wd.to(torch.float64))
    plan = plan_for(uvw, freq, mask, npix_x, npix_y, pixsize_x, pixsize_y, center_x, center_y, epsilon, do_wgridding,
                    rdt)
    out = plan.vis2dirty(vd, wd, divide_by_n)
    return _dev.host_like(out.to(rdt_in), vis)


def dirty2vis(uvw, freq, dirty, wgt=None, mask=None, pixsize_x=None, pixsize_y=None, center_x=0.0, center_y=0.0,
              epsilon=None, do_wgridding=None, divide_by_n=True, nthreads=1):
    """ducc0.wgridder.experimental.dirty2vis: vis (nrow, nchan) in the complex type of dirty, 0 where mask == 0."""
    _check_flags(do_wgridding, epsilon, pixsize_x, pixsize_y)
    dd = _dev.to_dev(dirty)
    if dd.dtype not in _dev.CPLX_OF or dd.ndim != 2:
        raise TypeError(f"dirty must be a 2-D float32 or float64 image, got {dd.dtype} {tuple(dd.shape)}")
    wd = _dev.to_dev(wgt)
    if wd is not None and wd.dtype != dd.dtype:
        raise TypeError(f"wgt must be {dd.dtype} like dirty, got {wd.dtype}")
    nx, ny = dd.shape
    plan = plan_for(uvw, freq, mask, nx, ny, pixsize_x, pixsize_y, center_x, center_y, epsilon, do_wgridding, dd.dtype)
    return _dev.host_like(plan.dirty2vis(dd, wd, divide_by_n), dirty)


# --------------------------------------------------------------------------- the grid worker's products, in one go
def image_data_products(uvw, freq, vis, wgt, mask, counts, nx, ny, nx_psf, ny_psf, cellx, celly, model=None,
                        robustness=None, x0=0.0, y0=0.0, nthreads=1, epsilon=1e-7, do_wgridding=True, double_accum=True,
                        l2reweight_dof=None, do_dirty=True, do_psf=True, do_weight=True):
    """pfb/operators/gridder.py:551-740: the image-space data products of one band in one go, with the reference's
    keys -- WEIGHT (if do_weight), WSUM (1,), DIRTY, PSF and PSFHAT (if do_psf), RESIDUAL (if a model is given) -- and its
    statements in its order: model visibilities, the l2 reweight, the imaging weights of `robustness` from `counts`
    multiplied into wgt, the dirty image, the PSF on (nx_psf, ny_psf) (from unit visibilities, or for a centre
    (x0, y0) != 0 from the degridded 128 x 128 delta), its transform, the residual image.  divide_by_n=False throughout.

    One plan of the cache per geometry: the (nx, ny) plan serves model, dirty and residual, the (nx_psf, ny_psf) plan the
    PSF (and a 128 x 128 one the delta).  They work in float64 when double_accum is set and in the type of vis otherwise.
    The model is degridded WITH the mask -- which the plan carries -- since residual_vis is multiplied by it anyway.

    Differences from the reference: the caller's wgt is never written (the reference's `wgt *= imwgt` writes into it);
    no weights at all (wgt None, no robustness, no l2 reweight, or an l2 reweight with an all-zero mask and no
    robustness) is a ValueError here and a TypeError on `None[...]` there.  `nthreads` and `do_dirty` are accepted and
    ignored (the reference ignores do_dirty too).  numpy in gives numpy out; with tensors in, the l2 reweight's
    sum of the mask is the one number that is read on the host."""
    if model is None and l2reweight_dof:
        raise ValueError('Requested l2 reweight but no model passed in. '
                         'Perhaps transfer model from somewhere?')
    if robustness is not None and counts is None:
        raise ValueError('counts are None but robustness specified. '
                         'This is probably a bug!')
    vd = _dev.to_dev(vis)
    if vd.dtype not in _dev.REAL_OF or vd.ndim != 2:
        raise TypeError(f"vis must be a (nrow, nchan) complex64 or complex128 array, got {vd.dtype} {tuple(vd.shape)}")
    cdt_in, rdt_in = vd.dtype, _dev.REAL_OF[vd.dtype]
    rdt = torch.float64 if double_accum else rdt_in
    cdt = _dev.CPLX_OF[rdt]
    md = _dev.byte_mask(mask, vd.shape)
    wd = _dev.to_dev(wgt)
    if wd is not None and (wd.dtype != rdt_in or wd.shape != vd.shape):
        raise TypeError(f"wgt must be {rdt_in} of the shape of vis, got {wd.dtype} {tuple(wd.shape)}")
    nx, ny = int(nx), int(ny)

    def plan(npx, npy):
        return plan_for(uvw, freq, mask, npx, npy, cellx, celly, x0, y0, epsilon, do_wgridding, rdt)

    def image(p, v, w):
        return p.vis2dirty(v.to(cdt), None if w is None else w.to(rdt), False).to(rdt_in)

    def degrid(p, img):
        return p.dirty2vis(img.to(rdt), None, False).to(cdt_in)

    out = {}
    imwgt = None
    if robustness is not None:
        imwgt = weighting._counts_to_weights(_dev.to_dev(counts, rdt_in), _dev.to_dev(uvw), _dev.to_dev(freq), nx, ny,
                                             cellx, celly, robustness)
    residual_vis = wsum = None
    if model is not None:
        xd = _dev.to_dev(model)
        if xd.dtype not in _dev.CPLX_OF or tuple(xd.shape) != (nx, ny):
            raise TypeError(f"model must be a float32 or float64 image of shape {(nx, ny)}")
        model_vis = degrid(plan(nx, ny), xd)            # no weights in this direction
        residual_vis, wl2, wsum = weighting._l2_reweight_dev(vd, model_vis, md, l2reweight_dof, imwgt)
        if l2reweight_dof:
            wd, imwgt = wl2, (None if wl2 is not None else imwgt)         # the product was formed in the kernel
    if imwgt is not None:
        wd = imwgt if wd is None else wd * imwgt
    if wd is None:
        raise ValueError('no weights: wgt is None and neither robustness nor an l2 reweight gives any')
    if do_weight:
        out['WEIGHT'] = wd
    out['WSUM'] = wsum if wsum is not None else weighting.masked_sum(wd, md)
    out['DIRTY'] = image(plan(nx, ny), vd, wd)
    if do_psf:
        if x0 or y0:
            delta = torch.zeros((128, 128), dtype=rdt, device=vd.device)
            delta[64, 64] = 1.0
            psf_vis = degrid(plan(128, 128), delta)
        else:
            psf_vis = torch.ones(vd.shape, dtype=cdt_in, device=vd.device)
        out['PSF'] = image(plan(int(nx_psf), int(ny_psf)), psf_vis, wd)
        out['PSFHAT'] = psfhat_from_psf(out['PSF'])
    if model is not None:
        out['RESIDUAL'] = image(plan(nx, ny), residual_vis, wd)
    return {key: _dev.host_like(t, vis) for key, t in out.items()}
