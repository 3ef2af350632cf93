"""
Imaging weights on MI355X -- pfb/utils/weighting.py:43-215 with the reference's names and signatures, and the
l2reweight_dof block of pfb/operators/gridder.py:604-615 (csrc/imweight.hip).

    _compute_counts / compute_counts           the uv-cell counts: nearest cell (k = 0) or a k x k footprint
    _counts_to_weights / counts_to_weights     uniform (robust <= -2) or Briggs weights of EVERY visibility
    _filter_extreme_counts / filter_extreme_counts   positive counts raised to median / level
    l2_reweight                                residual visibilities, Student-t weights and their masked sum
    _weight_data / weight_data                 Stokes visibilities and weights from correlations and Jones terms
                                               (weighting.py:281-350; csrc/stokes.hip, DESIGN 4.12, utils/stokes.py)

The grid coordinate of a visibility is the reference's, operation by operation in fp64; u_cell and umax are evaluated
here in Python floats exactly as the reference writes them, so cell indices agree bit for bit.  numpy in gives numpy out,
tensors in give tensors out; there is no CPU path.  With tensors in nothing crosses to the host.

Where this differs from the reference, by definition:
  * a visibility whose cell is outside [0, nx) x [0, ny) contributes nothing and gets weight 0, and a footprint cell
    outside the grid is skipped (the reference wraps a negative index and writes past the array at the top);
  * _filter_extreme_counts returns a new array (the reference writes into its argument and returns it);
  * weight_data: see its docstring.
"""
import numpy as np
import torch

from .. import _dev, _lib
from . import stokes as _stokes

SUPPORTS = tuple(range(0, 17, 2))
RECORD = 3          # PFB_IMW_RECORD


def _real_dtype(dtype):
    """float32 / float64 given as a torch dtype or as anything numpy understands; everything else: ValueError."""
    if isinstance(dtype, torch.dtype):
        dt = dtype
    else:
        try:
            dt = {np.dtype('float32'): torch.float32, np.dtype('float64'): torch.float64}.get(np.dtype(dtype))
        except TypeError:
            dt = None
    if dt not in (torch.float32, torch.float64):
        raise ValueError(f"dtype must be float32 or float64, got {dtype!r}")
    return dt


def uv_cells(nx, ny, cell_size_x, cell_size_y):
    """(u_cell, umax, v_cell, vmax) as weighting.py:48-55 writes them."""
    u_cell = 1 / (nx * cell_size_x)
    umax = abs(-1 / cell_size_x / 2 - u_cell / 2)
    v_cell = 1 / (ny * cell_size_y)
    vmax = abs(-1 / cell_size_y / 2 - v_cell / 2)
    return float(u_cell), float(umax), float(v_cell), float(vmax)


def _record(dev):
    return torch.empty(RECORD, dtype=torch.float64, device=dev)


def _work():
    """The partial sums' scratch (PFB_IMW_WORK_DOUBLES fit): this thread's and stream's reduction workspace."""
    return _dev.ptr(_dev.scratch()[0])


# ------------------------------------------------------------------------------------------------------ counts
def _compute_counts(uvw, freq, mask, nx, ny, cell_size_x, cell_size_y, dtype, k=6, ngrid=1):
    """weighting.py:43-103: (ngrid, nx, ny) partial grids of `dtype`; row r goes to the grid of its bin (bins of
    nrow // ngrid rows, the first nrow % ngrid one longer)."""
    rdt = _real_dtype(dtype)
    if isinstance(k, bool) or int(k) != k or int(k) not in SUPPORTS:
        raise ValueError(f"k must be one of {SUPPORTS}, got {k!r}")
    nx, ny, ngrid = int(nx), int(ny), int(ngrid)
    if ngrid < 1:
        raise ValueError(f"ngrid must be >= 1, got {ngrid}")
    ud, fd = _dev.uvw_freq(uvw, freq)
    nrow, nchan = int(ud.shape[0]), int(fd.shape[0])
    md = _dev.byte_mask(mask, (nrow, nchan))
    counts = torch.empty((ngrid, nx, ny), dtype=rdt, device=ud.device)
    if nrow * nchan == 0:
        counts.zero_()
    else:
        _lib.check(_lib.load().pfb_imw_counts(_dev.code(rdt), _dev.ptr(ud), _dev.ptr(fd), _dev.ptr(md), nrow, nchan, nx,
                                              ny, *uv_cells(nx, ny, cell_size_x, cell_size_y), int(k), ngrid,
                                              _dev.ptr(counts), _dev.stream()))
    return _dev.host_like(counts, uvw)


def compute_counts(uvw, freq, mask, nx, ny, cell_size_x, cell_size_y, dtype, k=6, ngrid=1):
    """weighting.py:14-33 without dask: the (nx, ny) sum of the partial grids, formed on the device."""
    ud = _dev.to_dev(uvw)
    counts = _compute_counts(ud, _dev.to_dev(freq), _dev.to_dev(mask), nx, ny, cell_size_x, cell_size_y, dtype, k, ngrid)
    return _dev.host_like(counts.sum(dim=0), uvw)


# ----------------------------------------------------------------------------------------------------- weights
def _counts_to_weights(counts, uvw, freq, nx, ny, cell_size_x, cell_size_y, robust):
    """weighting.py:130-171: (nrow, nchan) weights in the type of counts, for every visibility (the reference applies
    no mask here).  The moments of the counts and the Briggs factor stay on the device."""
    cd = _dev.to_dev(counts)
    nx, ny = int(nx), int(ny)
    if cd.dtype not in (torch.float32, torch.float64) or tuple(cd.shape) != (nx, ny):
        raise ValueError(f"counts must be float32 or float64 of shape {(nx, ny)}, got {cd.dtype} {tuple(cd.shape)}")
    ud, fd = _dev.uvw_freq(uvw, freq)
    nrow, nchan = int(ud.shape[0]), int(fd.shape[0])
    weights = torch.zeros((nrow, nchan), dtype=cd.dtype, device=cd.device)
    if nrow * nchan:
        lib, code = _lib.load(), _dev.code(cd.dtype)
        rec = _record(cd.device)
        _lib.check(lib.pfb_imw_moments(code, _dev.ptr(cd), cd.numel(), _dev.ptr(rec), _work(), _dev.stream()))
        briggs = robust > -2
        numsqrt = float(5 * 10 ** (-robust)) if briggs else 0.0
        _lib.check(lib.pfb_imw_weights(code, _dev.ptr(cd), _dev.ptr(rec), _dev.ptr(ud), _dev.ptr(fd), nrow, nchan, nx, ny,
                                       *uv_cells(nx, ny, cell_size_x, cell_size_y), int(briggs), numsqrt,
                                       _dev.ptr(weights), _dev.stream()))
    return _dev.host_like(weights, counts)


def counts_to_weights(counts, uvw, freq, nx, ny, cell_size_x, cell_size_y, robust):
    """weighting.py:109-122 without dask."""
    return _counts_to_weights(counts, uvw, freq, nx, ny, cell_size_x, cell_size_y, robust)


# ------------------------------------------------------------------------------------------------------ filter
def _filter_extreme_counts(counts, nbox=16, level=10.0):
    """weighting.py:186-215: the positive counts raised to (their median) / level.  numpy's median: the mean of the two
    middle values of an even number of them.  A NEW array (the reference writes into `counts`); `nbox` is unused, as in
    the reference."""
    cd = _dev.to_dev(counts)
    pos = cd > 0
    cnts = torch.sort(cd[pos]).values
    n = cnts.numel()
    if n == 0:
        return _dev.host_like(cd.clone(), counts)
    med = (cnts[(n - 1) // 2] + cnts[n // 2]) / 2
    # a tensor divisor: torch divides by a Python scalar as a product with its reciprocal, which is not med / level
    lowval = med / torch.tensor(level, dtype=cd.dtype, device=cd.device)
    return _dev.host_like(torch.where(pos, torch.maximum(cd, lowval), cd), counts)


def filter_extreme_counts(counts, nbox=16, nlevel=10):
    """weighting.py:174-181 without dask."""
    return _filter_extreme_counts(counts, nbox, nlevel)


# -------------------------------------------------------------------------------------------------- l2 reweight
def masked_sum(wgt, mask):
    """wgt[mask != 0].sum() accumulated in fp64 and rounded to wgt's type, as a 1-element device tensor."""
    rec = _record(wgt.device)
    if wgt.numel() == 0:
        rec.zero_()
    else:
        _lib.check(_lib.load().pfb_imw_wsum(_dev.code(wgt.dtype), _dev.ptr(wgt), _dev.ptr(mask), wgt.numel(),
                                            _dev.ptr(rec), _work(), _dev.stream()))
    return rec[:1].to(wgt.dtype)


def _l2_reweight_dev(vis, model_vis, mask, dof, imwgt=None):
    """Device tensors in and out: (residual_vis, wgt, wsum).  residual_vis = (vis - model_vis) * mask always.  With a
    dof: wgt = (dof + 1) / (dof + |residual_vis|^2 / ovar) / ovar [* imwgt], ovar = sum |residual_vis|^2 / sum mask, and
    wsum = wgt[mask != 0].sum() as a 1-element tensor; (None, None) when sum mask == 0, the reference's `wgt = None`
    -- the one number that is read on the host.  Without a dof: (residual_vis, None, None) and nothing is read."""
    if vis.dtype not in _dev.REAL_OF or model_vis.dtype != vis.dtype or model_vis.shape != vis.shape:
        raise TypeError("vis and model_vis must be complex64 or complex128 arrays of one type and shape")
    rdt = _dev.REAL_OF[vis.dtype]
    lib, code, n = _lib.load(), _dev.code(rdt), vis.numel()
    res = torch.empty_like(vis)
    rec = _record(vis.device)
    if n == 0:
        rec.zero_()
    else:
        _lib.check(lib.pfb_imw_l2_residual(code, _dev.ptr(vis), _dev.ptr(model_vis), _dev.ptr(mask), n, _dev.ptr(res),
                                           _dev.ptr(rec), _work(), _dev.stream()))
    if not dof:
        return res, None, None
    if rec[1].item() == 0.0:
        return res, None, None
    if imwgt is not None and (imwgt.dtype != rdt or imwgt.shape != vis.shape):
        raise TypeError(f"imwgt must be {rdt} of the shape of vis")
    wgt = torch.empty(vis.shape, dtype=rdt, device=vis.device)
    _lib.check(lib.pfb_imw_l2_weights(code, _dev.ptr(res), _dev.ptr(mask), _dev.ptr(imwgt), n, float(dof), _dev.ptr(rec),
                                      _dev.ptr(wgt), _work(), _dev.stream()))
    return res, wgt, rec[2:3].to(rdt)


def l2_reweight(vis, model_vis, mask, dof, imwgt=None):
    """gridder.py:604-615 as a function: (residual_vis, wgt, wsum), see _l2_reweight_dev; numpy in gives numpy out."""
    vd = _dev.to_dev(vis)
    md = _dev.byte_mask(mask, vd.shape)
    out = _l2_reweight_dev(vd, _dev.to_dev(model_vis), md, dof, _dev.to_dev(imwgt))
    return tuple(None if t is None else _dev.host_like(t, vis) for t in out)


# --------------------------------------------------------------------------------------------------- weight_data
def _weight_data(data, weight, flag, jones, tbin_idx, tbin_counts, ant1, ant2, pol, product, nc):
    """weighting.py:298-350: (vis, wgt), each (nrow, nchan), of the Stokes `product` from data (nrow, nchan, ncorr)
    complex, weight (nrow, nchan, ncorr) of data's real type, flag (nrow, nchan) and jones of data's type:
    (ntime, nant, nchan, ndir, 2) is the DIAG mode, (ntime, nant, nchan, ndir, 2, 2) the FULL mode; direction 0 is
    read.  nc is '2' / '4' or the integers and must be data's number of correlations.  Row r takes the Jones terms of
    the time bin t with tbin_idx[t] <= r + min(tbin_idx) < tbin_idx[t] + tbin_counts[t], found on the device by a
    binary search per row.  A flagged visibility and a row that no bin covers get vis = wgt = 0 whatever their data and
    weights hold.  One kernel (utils/stokes.py states the closed form).

    Differences from the reference, by definition: tbin_idx is never modified (the reference subtracts its minimum in
    place; here on read); the time bins must be ascending and must not overlap, else ValueError (tbin_idx and tbin_counts
    are index metadata of ntime entries and are read on the host for that check); an unknown pol, product or nc, and
    FULL Jones terms with 2 correlations, are a ValueError (the reference: NameError / IndexError); a singular Jones
    matrix on an unflagged visibility gives IEEE inf / nan, as in the reference.

    A `product` of several letters ('IQUV', 'QU', a sequence of letters: utils/stokes.py) gives vis and wgt
    (nprod, nrow, nchan), the planes in the order asked, from one pass over the inputs."""
    basis = _stokes.basis_list(pol, product)
    n = _stokes.ncorr_of(nc)
    dd = _dev.to_dev(data)
    if dd.ndim != 3 or dd.shape[2] != n:
        raise ValueError(f"data must be (nrow, nchan, {n}) for nc={nc!r}, got {tuple(dd.shape)}")
    fd = _dev.byte_mask(flag, tuple(dd.shape[:2]), 'flag')
    vis, wgt, _, _ = _stokes.run(dd, _dev.to_dev(weight), _stokes.W_SPECTRUM, fd, None, False, _dev.to_dev(jones),
                                 tbin_idx, tbin_counts, ant1, ant2, basis)
    return _dev.host_like(vis, data), _dev.host_like(wgt, data)


def weight_data(data, weight, flag, jones, tbin_idx, tbin_counts, ant1, ant2, pol, product, nc):
    """weighting.py:281-295: {'vis', 'wgt'} of _weight_data."""
    vis, wgt = _weight_data(data, weight, flag, jones, tbin_idx, tbin_counts, ant1, ant2, pol, product, nc)
    return {'vis': vis, 'wgt': wgt}
