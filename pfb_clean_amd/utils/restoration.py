"""
The restored image on the MI355X -- pfb/utils/restoration.py:6-57:

    restore_image(model, residual, cell_size_x, cell_size_y, gaussparf, gausspari, convolve_residuals, nthreads,
                  padding_frac)

model (*) clean beam [+ residual brought to the same resolution], per band.  Same positional order and side effects as
the reference: `model` is overwritten band by band with its convolved self (restoration.py:45-49) and a NEW array is
returned.  numpy in -> numpy out; torch-ROCm tensors stay on the device.

Where the reference builds one single-band convolution per band, this builds ONE plan holding the nband kernels
gaussparf[b] and runs one cube apply; the residual step is convolve2gaussres' ratio branch; the sum is pfb_axpby.
"""
import numpy as np
import torch

from .. import _dev
from .misc import _beam_plan, _convolve_dev


def _coords(nx, ny, cell_size_x, cell_size_y, which):
    """restoration.py:41-43 on the device.  np.meshgrid(x, y) is 'xy'-indexed: xx[i, j] = x[j], yy[i, j] = y[i], i.e.
    for the (nx, ny) cube the coordinate called x runs along the LAST axis.  Kept as the reference has it."""
    dev = _dev.require_device()
    x = torch.arange(-(nx // 2), nx // 2 + nx % 2, dtype=torch.float64, device=dev) * cell_size_x
    y = torch.arange(-(ny // 2), ny // 2 + ny % 2, dtype=torch.float64, device=dev) * cell_size_y
    return torch.meshgrid(x, y, indexing='xy')[which].contiguous()


def restore_image(model, residual, cell_size_x, cell_size_y, gaussparf, gausspari, convolve_residuals, nthreads,
                  padding_frac):
    """Restored image at the resolutions gaussparf[b] (one (emaj, emin, pa) per band, in the unit of the cell sizes);
    gausspari[b]: the resolution of band b's residual, used when convolve_residuals brings the residuals to
    gaussparf[0].  The reference works for square images only (its coordinate grids are 'xy'-indexed and fail to
    broadcast otherwise); nx != ny is a ValueError here as there."""
    assert model.ndim == 3
    assert model.shape == residual.shape
    assert len(gaussparf) == model.shape[0]
    assert len(gausspari) == model.shape[0]

    nband, nx, ny = (int(v) for v in model.shape)
    if nx != ny:
        raise ValueError(f"restore_image needs square images (the reference's coordinate grids have shape "
                         f"({ny}, {nx}) for a cube of shape {tuple(model.shape)}: operands could not be broadcast)")
    md = _dev.to_dev(model)
    rd = _dev.to_dev(residual)
    ckey = ('cells', float(cell_size_x), float(cell_size_y))
    xx = lambda: _coords(nx, ny, cell_size_x, cell_size_y, 0)
    yy = lambda: _coords(nx, ny, cell_size_x, cell_size_y, 1)

    # peak of the kernels set to unity (restoration.py:48)
    bp = _beam_plan(xx, yy, ckey, gaussparf, None, nx, ny, md.dtype, padding_frac, False, per_band=True)
    mconv = _convolve_dev(md, bp)
    if isinstance(model, np.ndarray):
        model[...] = mconv.cpu().numpy()
    else:
        model.copy_(mconv)

    if convolve_residuals:
        # kernels of unit volume (restoration.py:54)
        bp = _beam_plan(xx, yy, ckey, gaussparf[0], gausspari, nx, ny, rd.dtype, padding_frac, True)
        out = _convolve_dev(rd, bp)
    else:
        out = rd.clone()
    if out.dtype != mconv.dtype:
        dt = torch.promote_types(out.dtype, mconv.dtype)
        out, mconv = out.to(dt), mconv.to(dt)
    _dev.axpby(1.0, mconv, 1.0, out)          # model + residual
    return _dev.host_like(out, model)
