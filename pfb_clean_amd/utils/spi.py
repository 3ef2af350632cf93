"""
Spectral index and reference-flux maps on the MI355X -- pfb/utils/spi.py:

    fit_spi(image, beam, freqs, weights, threshold, nthreads, pb_min, padding_frac, ref_freq, dest)      spi.py:7-70
    fit_spi_components(data, weights, freqs, freq0, alphai, I0i, beam, tol, maxiter)    the fit fit_spi hands over

The model of a component is m_b = I0 B_b (freqs_b / ref_freq)^alpha, fitted by Gauss-Newton with the band weights
(include/pfb_hip.h, "spectral index", states every step).  The host keeps what is tiny and fp64: ln(freqs / ref_freq),
the weights and the reference band.  Everything image-sized runs in csrc/spi.hip.  numpy in -> numpy out; with device
tensors two numbers cross to the host: the component count, which sizes Ix / Iy and decides the ValueError, and the
number of components that used up maxiter, which decides the warning (DESIGN "Spectral index").
"""
import sys
import warnings

import numpy as np
import torch

from .. import _lib, _dev


# spi.py:37-39, verbatim (no space before "Max"); % image.max() after the beam cut
EMPTY_MASK = ("No components found above threshold. "
              "Try lowering your threshold."
              "Max of convolved model is %3.2e")


def _host64(a):
    """A small host float64 vector from a numpy array, a tensor of either kind or a sequence."""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a), dtype=np.float64).ravel()


def _bands(freqs, weights, ref_freq):
    """(ln x, w, ref): the per-band constants of the fit as ctypes-ready float64 arrays and the reference band."""
    lnx = np.log(freqs / ref_freq)
    return np.ascontiguousarray(lnx), np.ascontiguousarray(weights), int(np.argmin(np.abs(freqs - ref_freq)))


def _warn_late(notconv, maxiter):
    n = int(notconv.item())
    if n:
        warnings.warn(f"{n} components took maxiter = {maxiter} steps; their last iterate is returned")


def fit_spi_components(data, weights, freqs, freq0, alphai=None, I0i=None, beam=None, tol=1e-5, maxiter=100):
    """The per-component fit: data (ncomps, nband), weights and freqs (nband), beam (ncomps, nband) or None for 1,
    alphai / I0i (ncomps) starting values or None for -0.7 / data[:, ref].  Returns (4, ncomps) float64 -- alpha,
    alpha_err, I0, I0_err -- numpy for numpy data, a device tensor for a device tensor.  All-NaN for a component whose
    normal equations are singular; one warning with the number of components that took maxiter steps."""
    freqs, weights = _host64(freqs), _host64(weights)
    d = _dev.to_dev(data, torch.float64)
    if d.ndim != 2 or d.shape[1] != freqs.size or weights.size != freqs.size:
        raise ValueError(f"data {tuple(d.shape)} is not (ncomps, nband={freqs.size}) with {weights.size} weights")
    ncomps, nband = int(d.shape[0]), int(d.shape[1])

    def per_comp(a, shape, what):
        if a is None:
            return None
        t = _dev.to_dev(a, torch.float64)
        if tuple(t.shape) != shape:
            raise ValueError(f"{what} {tuple(t.shape)} is not {shape}")
        return t
    bm = per_comp(beam, (ncomps, nband), 'beam')
    a0, i0 = per_comp(alphai, (ncomps,), 'alphai'), per_comp(I0i, (ncomps,), 'I0i')
    lnx, w, ref = _bands(freqs, weights, float(freq0))
    out = torch.empty((4, ncomps), dtype=torch.float64, device=d.device)
    notconv = torch.empty(1, dtype=torch.int64, device=d.device)
    _lib.check(_lib.load().pfb_spi_fit_components(_dev.ptr(d), _dev.ptr(bm), nband, ncomps, lnx.ctypes.data,
                                                  w.ctypes.data, ref, _dev.ptr(a0), _dev.ptr(i0), float(tol),
                                                  int(maxiter), _dev.ptr(out), _dev.ptr(notconv), _dev.stream()))
    _warn_late(notconv, maxiter)
    return _dev.host_like(out, data)


def fit_spi(image, beam, freqs, weights, threshold, nthreads, pb_min, padding_frac, ref_freq, dest=sys.stdout, *,
            tol=1e-5, maxiter=100):
    """spi.py:7-70: alpha, alpha_err, I0 and I0_err maps of the pixels whose cube, after the beam cut
    where(beam > pb_min, image, 0), stays above `threshold` in every band.  image, beam: (nband, nx, ny) of one dtype,
    float32 or float64.  The maps have the image's dtype and are NaN off the fitted pixels; numpy in -> numpy out,
    device tensors in -> device tensors out.  nthreads and padding_frac are accepted and ignored."""
    freqs, weights = _host64(freqs), _host64(weights)
    assert image.ndim == 3
    assert beam.ndim == 3
    assert tuple(image.shape) == tuple(beam.shape)
    assert image.shape[0] > 1
    assert freqs.size == image.shape[0]
    assert weights.size == image.shape[0]

    img, bm = _dev.to_dev(image), _dev.to_dev(beam)
    if bm.dtype != img.dtype:
        raise TypeError(f"beam is {bm.dtype}, image {img.dtype}: one dtype for both")
    code = _dev.code(img.dtype)
    nband, nx, ny = (int(n) for n in img.shape)
    npix = nx * ny
    lib = _lib.load()
    lnx, w, ref = _bands(freqs, weights, float(ref_freq))

    # beam cut off, pixels above threshold
    work = torch.empty(lib.pfb_spi_work_bytes(npix) // 8, dtype=torch.int64, device=img.device)
    _lib.check(lib.pfb_spi_mask(code, _dev.ptr(img), _dev.ptr(bm), nband, npix, float(pb_min), float(threshold),
                                _dev.ptr(work), _dev.stream()))
    ncomps = int(work[lib.pfb_comps_work_bytes(npix) // 8 - 1].item())
    if not ncomps:
        raise ValueError(EMPTY_MASK % work[-1:].view(torch.float64).item())
    Ix = torch.empty(ncomps, dtype=torch.int64, device=img.device)
    Iy = torch.empty(ncomps, dtype=torch.int64, device=img.device)
    _lib.check(lib.pfb_comps_compact(npix, ny, _dev.ptr(work), _dev.ptr(Ix), _dev.ptr(Iy), _dev.stream()))

    print("Fitting %i components" % ncomps, file=dest)
    maps = torch.full((4, nx, ny), float('nan'), dtype=img.dtype, device=img.device)
    notconv = torch.empty(1, dtype=torch.int64, device=img.device)
    _lib.check(lib.pfb_spi_fit(code, _dev.ptr(img), _dev.ptr(bm), nband, npix, ny, _dev.ptr(Ix), _dev.ptr(Iy), ncomps,
                               lnx.ctypes.data, w.ctypes.data, ref, float(pb_min), float(tol), int(maxiter),
                               _dev.ptr(maps), _dev.ptr(notconv), _dev.stream()))
    _warn_late(notconv, maxiter)
    print("Done. Writing output. \n", file=dest)
    return tuple(_dev.host_like(maps[k], image) for k in range(4))
