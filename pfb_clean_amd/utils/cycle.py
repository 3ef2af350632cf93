"""
The statements between the solver calls of the workers' major-cycle loops on the MI355X -- pfb/workers/klean.py:190-339,
spotless.py:155-363, fluxmop.py:129-199, fwdbwd.py:233, 423:

    residual_stats(residual, model=None)       residual_mfs = sum(residual, axis=0); rms = np.std(residual_mfs) or
                                               np.std(residual_mfs[~np.any(model, axis=0)]); rmax = np.abs(...).max()
    support(model, min_value=None)             np.any(model, axis=0) / np.any(model > min_value, axis=0)
    mop_mask(model, dirosion=1)                ... followed by binary_dilation and binary_erosion (klean.py:301-305)
    close_mask(mask, dirosion=1)               the same on a given mask
    masked_problem(residual, mask, beam, seed) b = beam * mask * residual, x0[:, mask] = seed[mask], beam * mask
    rms_comps(alpha)                           np.std(np.sum(alpha, axis=0), axis=(-1, -2))[:, None, None]
    model_change(model, modelp)                norm(model - modelp) / norm(model)

Everything image-sized runs in csrc/cycle.hip (DESIGN "Major-cycle statistics").  numpy in -> numpy out; device tensors
stay on the device, and the only host synchronisation is the 32-byte record that residual_stats turns into two floats.
"""
import numpy as np
import torch

from .. import _lib, _dev

RECORD = 4                      # PFB_CYCLE_RECORD doubles per set: count, mean, M2, absmax
ALL_OUTPUTS = ('b', 'x0', 'beam_eff')


def _cube(a, name, ndim, what):
    if not isinstance(a, (np.ndarray, torch.Tensor)):
        raise TypeError(f"{name}: a numpy array or a torch tensor, not {type(a).__name__}")
    if a.ndim != ndim:
        raise ValueError(f"{name} {tuple(a.shape)} is not {what}")
    if 0 in a.shape:
        raise ValueError(f"{name} {tuple(a.shape)} is empty")
    d = _dev.to_dev(a)
    _dev.code(d.dtype)
    return d


def _mask_dev(mask, shape=None):
    """(nx, ny) bool / uint8 mask of either kind as a contiguous uint8 device tensor (a view for bool: no pass)."""
    if not isinstance(mask, (np.ndarray, torch.Tensor)):
        raise TypeError(f"mask: a numpy array or a torch tensor, not {type(mask).__name__}")
    if mask.ndim != 2 or (shape is not None and tuple(mask.shape) != tuple(shape)):
        raise ValueError(f"mask {tuple(mask.shape)} is not (nx, ny)" + (f" = {tuple(shape)}" if shape else ""))
    if 0 in mask.shape:
        raise ValueError(f"mask {tuple(mask.shape)} is empty")
    md = _dev.to_dev(mask)
    if md.dtype == torch.bool:
        return md.view(torch.uint8)
    if md.dtype != torch.uint8:
        raise TypeError(f"mask of dtype {md.dtype}: bool or uint8 only")
    return md


def _stats(x, nband, nset, npix, model, sum_out):
    """Device: one pfb_bandsum_stats; returns the (nset, RECORD) float64 device records."""
    lib = _lib.load()
    nbytes = lib.pfb_cycle_work_bytes(nset)
    if nbytes == 0:
        raise ValueError(f"{nset} sets are out of range")
    work = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)
    out = torch.empty((nset, RECORD), dtype=torch.float64, device=x.device)
    _lib.check(lib.pfb_bandsum_stats(_dev.code(x.dtype), _dev.ptr(x), nband, nset, npix, _dev.ptr(model),
                                     0 if model is None else int(model.shape[0]), _dev.ptr(sum_out), _dev.ptr(work),
                                     _dev.ptr(out), _dev.stream()))
    return out


def residual_stats(residual, model=None):
    """(residual_mfs, rms, rmax) of an (nband, nx, ny) residual cube: residual_mfs = np.sum(residual, axis=0) bit for
    bit, rms = np.std(residual_mfs) -- over the pixels where no band of the (nband_m, nx, ny) `model` is non-zero when a
    model is given (klean.py:280-281), nan when there is no such pixel -- and rmax = np.abs(residual_mfs).max().  rms
    and rmax are Python floats; the moments are fp64 whatever the dtype."""
    rd = _cube(residual, 'residual', 3, '(nband, nx, ny)')
    nband, nx, ny = (int(n) for n in rd.shape)
    md = None
    if model is not None:
        md = _cube(model, 'model', 3, '(nband, nx, ny)')
        if tuple(md.shape[1:]) != (nx, ny):
            raise ValueError(f"model {tuple(md.shape)} and residual {tuple(rd.shape)} differ in (nx, ny)")
        if md.dtype != rd.dtype:
            raise TypeError(f"model is {md.dtype}, residual {rd.dtype}")
    mfs = torch.empty((nx, ny), dtype=rd.dtype, device=rd.device)
    count, _, m2, amax = _stats(rd, nband, 1, nx * ny, md, mfs)[0].tolist()
    rms = float(np.sqrt(m2 / count)) if count > 0 else float('nan')
    return _dev.host_like(mfs, residual), rms, amax


def rms_comps(alpha):
    """spotless.py:222-223, 362-363: np.std(np.sum(alpha, axis=0), axis=(-1, -2))[:, None, None] of an (nband, nbasis,
    Nymax, Nxmax) coefficient cube, margins of the packed plane included, as an (nbasis, 1, 1) array of alpha's dtype
    and kind -- what l1reweight_func takes.  No host synchronisation for a device tensor."""
    ad = _cube(alpha, 'alpha', 4, '(nband, nbasis, Nymax, Nxmax)')
    nband, nbasis, ny, nx = (int(n) for n in ad.shape)
    rec = _stats(ad, nband, nbasis, ny * nx, None, None)
    rms = torch.sqrt(rec[:, 2] / rec[:, 0]).to(ad.dtype).view(nbasis, 1, 1)
    return _dev.host_like(rms, alpha)


def model_change(model, modelp):
    """spotless.py:345: np.linalg.norm(model - modelp) / np.linalg.norm(model) as a float, the two sums in fp64 from one
    pass (pfb_norm_diff_sums); 0 / 0 gives nan and x / 0 inf, as in numpy."""
    for name, a in (('model', model), ('modelp', modelp)):
        if not isinstance(a, (np.ndarray, torch.Tensor)):
            raise TypeError(f"{name}: a numpy array or a torch tensor, not {type(a).__name__}")
    if tuple(model.shape) != tuple(modelp.shape):
        raise ValueError(f"model {tuple(model.shape)} and modelp {tuple(modelp.shape)} differ in shape")
    xd, xpd = _dev.to_dev(model), _dev.to_dev(modelp)
    _dev.code(xd.dtype)
    if xd.dtype != xpd.dtype:
        raise TypeError(f"model is {xd.dtype}, modelp {xpd.dtype}")
    num, den = _dev.norm_diff_sums(xd, xpd).tolist()
    with np.errstate(all='ignore'):
        return float(np.sqrt(np.float64(num)) / np.sqrt(np.float64(den)))


def _close(cube, mask, nx, ny, min_value, dirosion, like):
    out = torch.empty((nx, ny), dtype=torch.uint8, device=(cube if cube is not None else mask).device)
    _lib.check(_lib.load().pfb_mask_close(0 if cube is None else _dev.code(cube.dtype), _dev.ptr(cube),
                                          0 if cube is None else int(cube.shape[0]), _dev.ptr(mask), nx, ny,
                                          int(min_value is not None), 0.0 if min_value is None else float(min_value),
                                          int(dirosion), _dev.ptr(out), _dev.stream()))
    return _dev.host_like(out.view(torch.bool), like)


def support(model, min_value=None):
    """np.any(model, axis=0) of an (nband, nx, ny) cube (a NaN counts, -0.0 does not), or with `min_value`
    np.any(model > min_value, axis=0) (fluxmop.py:129; the bound rounded to the cube's dtype), as a bool (nx, ny)."""
    md = _cube(model, 'model', 3, '(nband, nx, ny)')
    return _close(md, None, int(md.shape[1]), int(md.shape[2]), min_value, 0, model)


def mop_mask(model, dirosion=1):
    """klean.py:301-305: np.any(model, axis=0), then for dirosion != 0 binary_dilation and binary_erosion with
    generate_binary_structure(2, dirosion) -- 1: the cross, >= 2: the full 3 x 3.  Both steps take the outside of the image
    as 0, so no pixel whose structure reaches outside the image is in the result (scipy's border_value=0)."""
    md = _cube(model, 'model', 3, '(nband, nx, ny)')
    return _close(md, None, int(md.shape[1]), int(md.shape[2]), None, dirosion, model)


def close_mask(mask, dirosion=1):
    """The closing of mop_mask on a given bool / uint8 (nx, ny) mask."""
    md = _mask_dev(mask)
    return _close(None, md, int(md.shape[0]), int(md.shape[1]), None, dirosion, mask)


def masked_problem(residual, mask, beam=None, seed=None, *, outputs=ALL_OUTPUTS):
    """(b, x0, beam_eff) in one pass over an (nband, nx, ny) residual and an (nx, ny) bool / uint8 mask:
        beam_eff = beam * mask[None]                  beam (nband, nx, ny) or (1, nx, ny); the mask itself as (1, nx, ny)
                                                      of the residual's dtype without a beam
        b        = beam_eff * residual                a NaN residual outside the mask stays NaN, as in numpy
        x0       = zeros, x0[:, mask] = seed[mask]    seed (nx, ny); zeros without a seed
    -- the (b, x0, beam) arguments of pcg_psf in klean's flux mop (klean.py:306-317, seed = residual_mfs) and the beam of
    hessian_psf_cube with the b of pcg in fluxmop.py:166-199.  An output not named in `outputs` is not computed and
    comes back as None."""
    unknown = set(outputs) - set(ALL_OUTPUTS)
    if unknown:
        raise ValueError(f"outputs {sorted(unknown)} are not among {ALL_OUTPUTS}")
    rd = _cube(residual, 'residual', 3, '(nband, nx, ny)')
    nband, nx, ny = (int(n) for n in rd.shape)
    md = _mask_dev(mask, (nx, ny))
    bd = sd = None
    if beam is not None:
        bd = _cube(beam, 'beam', 3, '(nband, nx, ny) or (1, nx, ny)')
        if tuple(bd.shape[1:]) != (nx, ny) or int(bd.shape[0]) not in (1, nband):
            raise ValueError(f"beam {tuple(bd.shape)} does not fit the residual {tuple(rd.shape)}")
        if bd.dtype != rd.dtype:
            raise TypeError(f"beam is {bd.dtype}, residual {rd.dtype}")
    if seed is not None:
        sd = _cube(seed, 'seed', 2, '(nx, ny)')
        if tuple(sd.shape) != (nx, ny):
            raise ValueError(f"seed {tuple(sd.shape)} does not fit the residual {tuple(rd.shape)}")
        if sd.dtype != rd.dtype:
            raise TypeError(f"seed is {sd.dtype}, residual {rd.dtype}")
    new = lambda n: torch.empty((n, nx, ny), dtype=rd.dtype, device=rd.device)
    b = new(nband) if 'b' in outputs else None
    x0 = new(nband) if 'x0' in outputs else None
    be = new(1 if bd is None else int(bd.shape[0])) if 'beam_eff' in outputs else None
    _lib.check(_lib.load().pfb_masked_problem(_dev.code(rd.dtype), _dev.ptr(rd), _dev.ptr(md), _dev.ptr(bd),
                                              0 if bd is None else int(bd.shape[0]), _dev.ptr(sd), nband, nx * ny,
                                              _dev.ptr(b), _dev.ptr(x0), _dev.ptr(be), _dev.stream()))
    h = lambda t: None if t is None else _dev.host_like(t, residual)
    return h(b), h(x0), h(be)
