"""
The component model on the MI355X -- pfb/utils/misc.py:1084-1313:

    fit_image_cube(time, freq, image, wgt, nbasist, nbasisf, method, sigmasq)      misc.py:1084-1214
    eval_coeffs_to_cube(time, freq, nx, ny, coeffs, Ix, Iy, expr, paramf, texpr, fexpr)   misc.py:1217-1235
    eval_coeffs_to_slice(time, freq, coeffs, Ix, Iy, expr, paramf, texpr, fexpr, nxi, ...)   misc.py:1238-1313

The host keeps what is tiny and fp64 (numpy + sympy + one LAPACK getrf): the design matrix and the strings that
describe it, the LU factors of the normal equations, the basis values of a parsed expression and the 1-D coordinate
arrays of the regrid.  Everything image-sized runs in csrc/comps.hip.  numpy in -> numpy out; with device tensors
nothing crosses to the host except the component count, which sizes the outputs (DESIGN "Component model").
"""
import functools

import numpy as np
import scipy.linalg
import sympy as sm
import torch
from sympy.parsing.sympy_parser import parse_expr

from .. import _lib, _dev

_T, _F = sm.Symbol('t'), sm.Symbol('f')


# ------------------------------------------------------------------------------------------------ host: the fit
def _unit_interval(v, sym):
    """misc.py:1165-1171 / :1190-1195: v shifted to its mid-range and divided by the largest shifted value, with the
    same map as a sympy expression of `sym`."""
    mid = (v.max() + v.min()) / 2
    w = v - mid
    top = w.max()
    w /= top
    return w, (sym - mid) / top


def _legendre_columns(w, orders):
    X = np.zeros((w.size, len(orders)))
    for k, i in enumerate(orders):
        X[:, k] = np.polynomial.Legendre.basis(i)(w)
    return X


def fit_design(time, freq, nbasist=None, nbasisf=None, method='poly'):
    """(Xfit, expr, params, texpr, fexpr) of _design, kept for the last few (time, freq, basis) sets: a worker fits the
    same axes after every major iteration and sympy takes milliseconds to build and print the expression."""
    time, freq = np.ascontiguousarray(time).ravel(), np.ascontiguousarray(freq).ravel()
    Xfit, expr, params, texpr, fexpr = _design_cached(time.tobytes(), time.dtype.str, freq.tobytes(), freq.dtype.str,
                                                      nbasist, nbasisf, method)
    return Xfit, expr, list(params), texpr, fexpr


@functools.lru_cache(maxsize=16)
def _design_cached(tbytes, tdtype, fbytes, fdtype, nbasist, nbasisf, method):
    Xfit, expr, params, texpr, fexpr = _design(np.frombuffer(tbytes, dtype=tdtype), np.frombuffer(fbytes, dtype=fdtype),
                                               nbasist, nbasisf, method)
    Xfit.setflags(write=False)
    return Xfit, expr, tuple(params), texpr, fexpr


def _design(time, freq, nbasist, nbasisf, method):
    """The design matrix of misc.py:1146-1202 and the strings that describe it:
    (Xfit (ntime * nband, nparam), expr, params, texpr, fexpr).

    Column j of Xfit is basis function j at the row's (t, f).  The reference tiles its time columns time-fastest and
    its frequency columns band-fastest, while the rows of its right-hand side run band-fastest; for ntime > 1 the time
    columns therefore do not line up with the data.  That is reproduced as it is (every live caller has ntime == 1).
    """
    ntime, nband = time.size, freq.size
    if nbasist is None:
        nbasist = ntime
    else:
        assert nbasist <= ntime
    if nbasisf is None:
        nbasisf = nband
    else:
        assert nbasisf <= nband
    if nband == 1:
        raise ValueError("fit_image_cube needs more than one band (the reference's frequency map is unbound for one)")
    if method not in ('poly', 'Legendre'):
        raise ValueError(f"unknown method {method!r}: 'poly' or 'Legendre'")

    tpar = [sm.Symbol(f't{i}') for i in range(nbasist)]
    fpar = [sm.Symbol(f'f{i}') for i in range(1, nbasisf)]
    if method == 'poly':
        # monomials of t / t[0] and f / f[0]; the constant belongs to the time block
        wt, tmap = time / time[0], _T / time[0]
        wf, fmap = freq / freq[0], _F / freq[0]
        Xt = wt[:, None] ** np.arange(nbasist)
        Xf = wf[:, None] ** np.arange(1, nbasisf)
        tbasis = [_T ** i for i in range(nbasist)]
        fbasis = [_F ** i for i in range(1, nbasisf)]
    else:
        # Legendre polynomials on [-1, 1]; a single time is used as it is
        wt, tmap = _unit_interval(time, _T) if ntime > 1 else (time, _T)
        wf, fmap = _unit_interval(freq, _F)
        Xt = _legendre_columns(wt, range(nbasist)) if nbasist > 1 else np.ones((ntime, 1))
        Xf = _legendre_columns(wf, range(1, nbasisf))
        tbasis = [sm.legendre_poly(i, _T) for i in range(nbasist)]
        fbasis = [sm.legendre_poly(i, _F) for i in range(1, nbasisf)]
    Xfit = np.hstack((np.tile(Xt, (nband, 1)), np.tile(Xf, (ntime, 1))))
    expr = sum(b * p for b, p in zip(tbasis + fbasis, tpar + fpar))
    return Xfit, str(expr), [str(p) for p in tpar + fpar], str(tmap), str(fmap)


def _fit_system(Xfit, wgt, sigmasq):
    """[A | LU | piv] as one float64 vector: A = Xfit^T diag(w), LU / piv the getrf factors of A Xfit (+ sigmasq I),
    misc.py:1206-1211 (np.linalg.solve is the same getrf followed by getrs)."""
    nrow, nparam = Xfit.shape
    w = np.ones((nrow, 1)) if wgt is None else np.asarray(wgt, dtype=np.float64).reshape(nrow, 1)
    A = np.ascontiguousarray((w * Xfit).T)
    H = Xfit.T.dot(w * Xfit)
    if sigmasq:
        H += sigmasq * np.eye(nparam)
    lu, piv = scipy.linalg.lu_factor(H, check_finite=False)
    if not np.all(np.diag(lu) != 0):
        raise np.linalg.LinAlgError("Singular matrix")
    return np.concatenate((A.ravel(), lu.ravel(), piv.astype(np.float64)))


def _components(img, nx, ny):
    """Device: the mask pass, the one read of the count, the compaction.  img: (nplane, nx * ny) view of the cube."""
    lib = _lib.load()
    npix = nx * ny
    work = torch.empty(lib.pfb_comps_work_bytes(npix) // 8, dtype=torch.int64, device=img.device)
    _lib.check(lib.pfb_comps_mask(_dev.code(img.dtype), _dev.ptr(img), img.shape[0], npix, _dev.ptr(work),
                                  _dev.stream()))
    ncomps = int(work[-1].item())
    Ix = torch.empty(ncomps, dtype=torch.int64, device=img.device)
    Iy = torch.empty(ncomps, dtype=torch.int64, device=img.device)
    if ncomps:
        _lib.check(lib.pfb_comps_compact(npix, ny, _dev.ptr(work), _dev.ptr(Ix), _dev.ptr(Iy), _dev.stream()))
    return Ix, Iy


def fit_image_cube(time, freq, image, wgt=None, nbasist=None, nbasisf=None, method='poly', sigmasq=0):
    """misc.py:1084-1214: least-squares fit of the time and frequency axes of every non-zero pixel of an
    (ntime, nband, nx, ny) cube.  Returns (coeffs (nparam, ncomps) float64, Ix, Iy int64, expr, params, texpr, fexpr);
    the arrays are numpy for a numpy image and device tensors for a device tensor."""
    time, freq = np.asarray(time), np.asarray(freq)
    Xfit, expr, params, texpr, fexpr = fit_design(time, freq, nbasist, nbasisf, method)
    if image.ndim != 4 or tuple(image.shape[:2]) != (time.size, freq.size):
        raise ValueError(f"image {tuple(image.shape)} is not (ntime={time.size}, nband={freq.size}, nx, ny)")
    if isinstance(wgt, torch.Tensor):
        wgt = wgt.cpu().numpy()
    sys_ = _fit_system(Xfit, wgt, sigmasq)
    nrow, nparam = Xfit.shape

    img = _dev.to_dev(image)
    _dev.code(img.dtype)
    nx, ny = int(img.shape[2]), int(img.shape[3])
    img = img.view(nrow, nx * ny)
    Ix, Iy = _components(img, nx, ny)
    ncomps = Ix.numel()
    coeffs = torch.empty((nparam, ncomps), dtype=torch.float64, device=img.device)
    sysd = torch.from_numpy(sys_).to(img.device)
    _lib.check(_lib.load().pfb_comps_fit(_dev.code(img.dtype), _dev.ptr(img), nrow, nx * ny, ny, _dev.ptr(Ix),
                                         _dev.ptr(Iy), ncomps, _dev.ptr(sysd), nparam, _dev.ptr(coeffs),
                                         _dev.stream()))
    h = lambda t: _dev.host_like(t, image)
    return h(coeffs), h(Ix), h(Iy), expr, params, texpr, fexpr


# ------------------------------------------------------------------------------------------- host: the evaluation
def basis_values(time, freq, expr, paramf, texpr, fexpr):
    """E (ntime * nfreq, nparam): the factor of parameter p in `expr` at (tfunc(time[i]), ffunc(freq[j])), plane
    i * nfreq + j -- what misc.py:1223-1233 evaluates with image-sized arguments, reduced to its scalars.  `expr`
    must be linear in its parameters (every expression fit_image_cube returns is)."""
    time = np.atleast_1d(np.asarray(time, dtype=np.float64))
    freq = np.atleast_1d(np.asarray(freq, dtype=np.float64))
    tfunc, ffunc, basis = _parsed(expr, tuple(paramf), texpr, fexpr)
    tv = np.asarray(tfunc(time), dtype=np.float64)
    fv = np.asarray(ffunc(freq), dtype=np.float64)
    E = np.empty((time.size, freq.size, len(basis)))
    for k, b in enumerate(basis):
        E[:, :, k] = b(tv[:, None], fv[None, :])
    return E.reshape(time.size * freq.size, len(basis))


@functools.lru_cache(maxsize=16)
def _parsed(expr, paramf, texpr, fexpr):
    """numpy callables (tfunc(t), ffunc(f), [basis_p(t, f)]) of the strings a fit returned."""
    pars = [sm.Symbol(p) for p in paramf]
    model = parse_expr(expr)
    basis = [sm.diff(model, p) for p in pars]
    if any(b.free_symbols & set(pars) for b in basis) or sm.expand(model - sum(b * p for b, p in zip(basis, pars))) != 0:
        raise ValueError(f"expression {expr!r} is not linear in its parameters {list(paramf)}")
    return (sm.lambdify(_T, parse_expr(texpr)), sm.lambdify(_F, parse_expr(fexpr)),
            [sm.lambdify((_T, _F), b) for b in basis])


def _render(E, nx, ny, coeffs, Ix, Iy, dtype):
    """Device (nplane, nx, ny) tensor of `dtype` from host E and coeffs / Ix / Iy of either kind."""
    cd = _dev.to_dev(coeffs, torch.float64)
    if cd.ndim != 2 or cd.shape[0] != E.shape[1]:
        raise ValueError(f"coeffs {tuple(cd.shape)} do not hold one row for each of the {E.shape[1]} parameters")
    ixd, iyd = _dev.to_dev(Ix, torch.int64), _dev.to_dev(Iy, torch.int64)
    ncomps = cd.shape[1]
    if ixd.numel() != ncomps or iyd.numel() != ncomps:
        raise ValueError(f"Ix ({ixd.numel()}) / Iy ({iyd.numel()}) do not match the {ncomps} components")
    out = torch.empty((E.shape[0], nx, ny), dtype=dtype, device=cd.device)
    Ed = torch.from_numpy(np.ascontiguousarray(E)).to(cd.device)
    _lib.check(_lib.load().pfb_comps_eval(_dev.code(dtype), _dev.ptr(Ed), E.shape[0], E.shape[1], _dev.ptr(cd),
                                          _dev.ptr(ixd), _dev.ptr(iyd), ncomps, nx, ny, _dev.ptr(out), _dev.stream()))
    return out


def _out_dtype(dtype):
    if dtype is None:
        return torch.float64
    if isinstance(dtype, torch.dtype):
        _dev.code(dtype)
        return dtype
    return _dev._NP2T[np.dtype(dtype)]


def eval_coeffs_to_cube(time, freq, nx, ny, coeffs, Ix, Iy, expr, paramf, texpr, fexpr, *, dtype=None):
    """misc.py:1217-1235: the (ntime, nfreq, nx, ny) cube of the fitted model at the given times and frequencies, zero
    off the components.  float64 like the reference's unless `dtype` (np.float32 renders straight into an fp32 model).
    The (Ix, Iy) pairs must be unique."""
    time, freq = np.asarray(time), np.asarray(freq)
    E = basis_values(time, freq, expr, paramf, texpr, fexpr)
    out = _render(E, int(nx), int(ny), coeffs, Ix, Iy, _out_dtype(dtype))
    return _dev.host_like(out.view(time.size, freq.size, int(nx), int(ny)), coeffs)


def slice_geometry(nxi, nyi, cellxi, cellyi, x0i, y0i, nxo, nyo, cellxo, cellyo, x0o, y0o):
    """The 1-D side of misc.py:1254-1301: (xin, yin, xo, yo, (npadxl, npadxu, npadyl, npadyu), do_interp), xin / yin in
    their padded form when the output reaches beyond the input.  Raises ValueError where RegularGridInterpolator's
    bounds_error=True would."""
    def axis(n, cell, x0, lo=0, hi=0):
        return (-(n // 2 + lo) + np.arange(n + lo + hi)) * cell + x0

    def pads(vin, vo, cell):
        lo, hi = vin.min() - vo.min(), vo.max() - vin.max()
        return (int(np.ceil(lo / cell)) if lo > 0.0 else 0), (int(np.ceil(hi / cell)) if hi > 0.0 else 0)

    xin, yin = axis(nxi, cellxi, x0i), axis(nyi, cellyi, y0i)
    xo, yo = axis(nxo, cellxo, x0o), axis(nyo, cellyo, y0o)
    npadxl, npadxu = pads(xin, xo, cellxi)
    npadyl, npadyu = pads(yin, yo, cellyi)
    if npadxl > 0 or npadxu > 0 or npadyl > 0 or npadyu > 0:
        xin, yin = axis(nxi, cellxi, x0i, npadxl, npadxu), axis(nyi, cellyi, y0i, npadyl, npadyu)
    do_interp = (cellxi != cellxo or cellyi != cellyo or x0i != x0o or y0i != y0o
                 or xin.size != nxo or yin.size != nyo)
    if do_interp:
        for d, (grid, pts) in enumerate(((xin, xo), (yin, yo))):
            if grid.size < 2 or not np.all(np.diff(grid) > 0):
                raise ValueError(f"The points in dimension {d} must be strictly ascending")
            if not (np.all(grid[0] <= pts) and np.all(pts <= grid[-1])):
                raise ValueError(f"One of the requested xi is out of bounds in dimension {d}")
    return xin, yin, xo, yo, (npadxl, npadxu, npadyl, npadyu), bool(do_interp)


def eval_coeffs_to_slice(time, freq, coeffs, Ix, Iy, expr, paramf, texpr, fexpr, nxi, nyi, cellxi, cellyi, x0i, y0i,
                         nxo, nyo, cellxo, cellyo, x0o, y0o, *, dtype=None):
    """misc.py:1238-1313: the model at one time and frequency, rendered on its own (nxi, nyi) grid and brought onto
    the (nxo, nyo) grid: zero padding where the output reaches beyond the input, bilinear interpolation when the grids
    differ.  float64 unless `dtype`."""
    nxi, nyi, nxo, nyo = int(nxi), int(nyi), int(nxo), int(nyo)
    E = basis_values(time, freq, expr, paramf, texpr, fexpr)
    xin, yin, xo, yo, (pxl, pxu, pyl, pyu), do_interp = slice_geometry(nxi, nyi, cellxi, cellyi, x0i, y0i, nxo, nyo,
                                                                       cellxo, cellyo, x0o, y0o)
    odt = _out_dtype(dtype)
    if not do_interp:
        out = _render(E, nxi, nyi, coeffs, Ix, Iy, odt)[0]
        if pxl or pxu or pyl or pyu:
            out = torch.nn.functional.pad(out, (pyl, pyu, pxl, pxu))
        return _dev.host_like(out, coeffs)
    plane = _render(E, nxi, nyi, coeffs, Ix, Iy, torch.float64)
    dev = plane.device
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    xind, yind, xod, yod = up(xin), up(yin), up(xo), up(yo)
    out = torch.empty((nxo, nyo), dtype=odt, device=dev)
    _lib.check(_lib.load().pfb_comps_interp(_dev.code(odt), _dev.ptr(plane), nxi, nyi, pxl, pyl, _dev.ptr(xind),
                                            xin.size, _dev.ptr(yind), yin.size, _dev.ptr(xod), nxo, _dev.ptr(yod), nyo,
                                            _dev.ptr(out), _dev.stream()))
    return _dev.host_like(out, coeffs)
