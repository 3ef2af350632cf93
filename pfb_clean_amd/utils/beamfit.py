"""
The clean beam on the MI355X -- pfb/utils/misc.py:506-584:

    fitcleanbeam(psf, level=0.5, pixsize=1.0, extent=15.0)      misc.py:529-584

The host keeps the optimiser (scipy.optimize.fmin_l_bfgs_b with the reference's arguments) and three numbers per
band; everything image-sized runs in csrc/beamfit.hip: one streaming pass for the maxima, the centre island and its
extents in one launch for all bands, and psf_errorsq with its analytic gradient per evaluation.  What crosses to the
host is the per-band record and 32 bytes per evaluation, never the cube (DESIGN "Clean beam").
"""
import numpy as np
import torch
from scipy.optimize import fmin_l_bfgs_b

from .. import _lib, _dev

RECORD = 16                     # PFB_BEAMFIT_RECORD doubles per band
FIELDS = ('max', 'any', 'centre_above', 'xmin', 'xmax', 'ymin', 'ymax', 'absx', 'absy', 'nlobe', 'nfit', 'rsq_extent')


def start_point(rec):
    """misc.py:563-564, 574-575, 578: (emaj0, emin0, 0.0) from one band's record."""
    r = dict(zip(FIELDS, rec))
    xdiff, ydiff = r['xmax'] - r['xmin'], r['ymax'] - r['ymin']
    return np.array((np.maximum(xdiff, ydiff), np.minimum(xdiff, ydiff), 0.0))


def lobe_records(psfd, level=0.5, extent=15.0):
    """Device: the max pass and the lobe pass on an (nband, nx, ny) device tensor.  Returns (records, work): the
    (nband, RECORD) float64 numpy records (columns FIELDS) and the device scratch that the objective reads."""
    lib = _lib.load()
    nband, nx, ny = (int(n) for n in psfd.shape)
    code = _dev.code(psfd.dtype)
    nbytes = lib.pfb_beamfit_work_bytes(nband, nx * ny)
    if nbytes == 0:
        raise ValueError(f"fitcleanbeam: psf of shape {tuple(psfd.shape)} is out of range")
    work = torch.empty(nbytes // 8, dtype=torch.float64, device=psfd.device)
    _lib.check(lib.pfb_beamfit_max(code, _dev.ptr(psfd), nband, nx * ny, _dev.ptr(work), _dev.stream()))
    _lib.check(lib.pfb_beamfit_lobe(code, _dev.ptr(psfd), nband, nx, ny, float(level), float(extent), _dev.ptr(work),
                                    _dev.stream()))
    return work[:nband * RECORD].cpu().numpy().reshape(nband, RECORD), work


def objective(psfd, work, band, out=None):
    """x -> (f, grad) of psf_errorsq (misc.py:506-526) over the fit region of `band`: one launch and one 32-byte read
    per call."""
    lib = _lib.load()
    _, nx, ny = (int(n) for n in psfd.shape)
    code = _dev.code(psfd.dtype)
    if out is None:
        out = torch.empty(4, dtype=torch.float64, device=psfd.device)

    def func(x):
        _lib.check(lib.pfb_beamfit_objective(code, _dev.ptr(psfd), band, nx, ny, float(x[0]), float(x[1]),
                                             float(x[2]), _dev.ptr(work), _dev.ptr(out), _dev.stream()))
        res = out.cpu().numpy()
        return res[0], res[1:].copy()
    return func


def fitcleanbeam(psf, level=0.5, pixsize=1.0, extent=15.0):
    """misc.py:529-584: the Gaussian that approximates the main lobe of every band of an (nband, nx, ny) PSF cube, as
    a list of [emaj * pixsize, emin * pixsize, pa] per band; [nan, nan, nan] for an all-zero band.  numpy array
    (staged) or device tensor (resident, not modified), float32 or float64.

    A band whose centre pixel is not above `level` (a NaN maximum included) raises ValueError: the reference labels
    the background as the 'centre island' there and fits that."""
    if psf.ndim != 3:
        raise ValueError(f"fitcleanbeam: psf {tuple(psf.shape)} is not (nband, nx, ny)")
    psfd = _dev.to_dev(psf)
    recs, work = lobe_records(psfd, level, extent)
    out = torch.empty(4, dtype=torch.float64, device=psfd.device)
    fields = dict(zip(FIELDS, recs.T))
    bad = np.flatnonzero((fields['any'] != 0) & (fields['centre_above'] == 0))
    if bad.size:
        v = int(bad[0])
        raise ValueError(f"fitcleanbeam: band {v}: the centre pixel is not above level {level} of the maximum "
                         f"({fields['max'][v]}); there is no main lobe to fit")
    gausspars = []
    for v, rec in enumerate(recs):
        if not fields['any'][v]:
            gausspars.append([np.nan, np.nan, np.nan])
            continue
        p, f, d = fmin_l_bfgs_b(objective(psfd, work, v, out), start_point(rec),
                                bounds=((0, None), (0, None), (None, None)), factr=1e11)
        gausspars.append([p[0] * pixsize, p[1] * pixsize, p[2]])
    return gausspars
