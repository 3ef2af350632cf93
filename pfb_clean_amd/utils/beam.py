"""
Beam resampling on MI355X -- pfb/utils/beam.py with the reference's names (csrc/visconcat.hip).

    _eval_beam / eval_beam(beam_image, l_in, m_in, l_out, m_out)   the beam, given on the rectilinear grid l_in x m_in,
                                  at the output coordinates: bilinear inside, linearly extrapolated from the edge cell
                                  outside (what the reference falls back to once its bounds_error=True attempt fails)
    _interp_beam_impl(freq, nx, ny, cell_deg, btype=None)   ones: the only beam "model" built here

The beam MODELS of the reference (katbeam's JimBeam, the .npz holography cubes, africanus' beam_cube_dde) are out of
scope: those packages are not dependencies, and the reference's own function stops in a debugger behind them.
"""
import numpy as np
import torch

from .. import _dev, _lib


def _interp_beam_impl(freq, nx, ny, cell_deg, btype, utime=None, ant_pos=None, phase_dir=None):
    """beam.py:16-28 for btype=None: ones of (nx, ny), float64, on the device.  Any other btype: NotImplementedError."""
    if isinstance(freq, np.ndarray):
        assert freq.size == 1, "Only single frequency interpolation currently supported"
    if btype is not None:
        raise NotImplementedError(f"beam model {btype!r}: only btype=None (a unit beam) is built")
    return torch.ones((int(nx), int(ny)), dtype=torch.float64, device=_dev.require_device())


def _axis(a, name):
    """A beam axis on the host: float64, 1-D, at least 2 nodes, strictly monotonic; (ascending axis, was descending)."""
    g = np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    if g.ndim != 1 or g.size < 2:
        raise ValueError(f"{name} must be 1-D with at least 2 points")
    d = np.diff(g)
    if (d > 0).all():
        return g, False
    if (d < 0).all():
        return g[::-1].copy(), True
    raise ValueError(f"The points in dimension {name} must be strictly ascending or descending")


def _eval_beam(beam_image, l_in, m_in, l_out, m_out, *, dtype=None):
    """beam.py:120-140: beam_image (nl, nm), float32 or float64, given at l_in (nl) x m_in (nm), evaluated at l_out (nxo)
    x m_out (nyo) (their 'ij' mesh) or at the 2-D coordinates l_out, m_out (nxo, nyo).  The cell of a coordinate x on
    an axis g is the i of g[i] <= x < g[i + 1] clipped to [0, n - 2], its weight (x - g[i]) / (g[i + 1] - g[i]): scipy's
    RegularGridInterpolator(method='linear', bounds_error=False, fill_value=None).  A strictly descending axis is
    flipped (with the beam); the axes are metadata and are checked on the host.  Coordinates and weights are fp64.
    The result is float64, or `dtype` (float32 / float64), rounded at the store.  numpy in gives numpy out."""
    if l_out.ndim == 2:
        coord2d = True
    elif l_out.ndim == 1:
        coord2d = False
    else:
        raise ValueError('Only 1 or 2D coordinates supported for beam evaluation')
    from .weighting import _real_dtype
    odt = torch.float64 if dtype is None else _real_dtype(dtype)
    bd = _dev.to_dev(beam_image)
    if bd.dtype not in (torch.float32, torch.float64):
        bd = bd.to(torch.float64)
    gl, flip_l = _axis(l_in, 'l_in')
    gm, flip_m = _axis(m_in, 'm_in')
    if bd.ndim != 2 or tuple(bd.shape) != (gl.size, gm.size):
        raise ValueError(f"beam_image must be {(gl.size, gm.size)}, got {tuple(bd.shape)}")
    flips = [d for d, f in enumerate((flip_l, flip_m)) if f]
    if flips:
        bd = torch.flip(bd, flips).contiguous()
    lo, mo = _dev.to_dev(l_out, torch.float64), _dev.to_dev(m_out, torch.float64)
    if coord2d:
        if mo.shape != lo.shape:
            raise ValueError("2-D l_out and m_out must have one shape")
        nxo, nyo = (int(n) for n in lo.shape)
    else:
        if mo.ndim != 1:
            raise ValueError("m_out must be 1-D like l_out")
        nxo, nyo = int(lo.shape[0]), int(mo.shape[0])
    out = torch.empty((nxo, nyo), dtype=odt, device=bd.device)
    if nxo * nyo:
        gld, gmd = _dev.to_dev(gl), _dev.to_dev(gm)
        _lib.check(_lib.load().pfb_beam_eval(_dev.code(bd.dtype), _dev.ptr(bd), gl.size, gm.size, _dev.ptr(gld),
                                             _dev.ptr(gmd), _dev.ptr(lo), _dev.ptr(mo), int(coord2d), nxo, nyo,
                                             _dev.code(odt), _dev.ptr(out), _dev.stream()))
    return _dev.host_like(out, beam_image)


eval_beam = _eval_beam          # the reference's eval_beam is the dask wrapper of _eval_beam
