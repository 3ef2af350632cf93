"""
Power method for the spectral norm of the (PSF-approximated) Hessian -- drop-in for
pfb/opt/power_method.py:11-49.  One matvec per iteration and ONE host look at the three inner products
<b,b>, <bp,b>, <bp,bp> (they are left in device scalars and read back together); when `A` is this package's
HessianPsf (or the functools.partial of hessian_psf_cube / _hessian_psf_slice the workers build) <bp,b> and
<b,b> come fused out of the convolution's epilogue (pfb_psfconv_apply_dots) instead of two more passes; for a
ParamHessian (or the fwdbwd worker's partial of hessian_psf, fwdbwd.py:318-324) out of its second band mix
(pfb_hessparam_apply_dots); on an embedded (non-power-of-two) plan the recognised ParamHessian is called as a whole --
its fused apply, pfb_hessparam_apply, in the padded domain -- and the three products are separate passes.
`A` may return an aliased buffer (it is normalised into `bp` straight away, power_method.py:29-36).  With b0=None the start vector is drawn with numpy's global
RNG exactly like the reference (np.random.randn, fp64); `dtype` (numpy or torch dtype,
an extension) casts it and, when a torch dtype, keeps the iteration on device tensors.
A is called with the same array kind (numpy / GPU tensor) as the start vector.

Extension `group` (the reference's power_method_dist, power_method.py:70-116, sums the same three numbers
over its dask workers): a torch.distributed process group over which the BAND axis is sharded.  `A`, `imsize` / `b0`
then describe this rank's bands; <bp,b>, <bp,bp>, <b,b> are all-reduced (three scalars per iteration, one collective)
and every rank returns the same beta together with its own bands of the eigenvector.
"""
import math
import sys

import numpy as np
import torch

from .. import _dev


def power_method(A, imsize, b0=None, tol=1e-5, maxit=250, verbosity=1, report_freq=25,
                 dtype=None, group=None):
    if group is not None:
        import torch.distributed as dist
        pg = None if group is True else group

    def allsum(vals):                   # sum of a short list of host scalars over the band shards
        if group is None:
            return vals
        t = torch.tensor(vals, dtype=torch.float64, device=bd.device if dist.get_backend(pg) != 'gloo' else 'cpu')
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=pg)
        return t.tolist()

    if b0 is None:
        b0 = np.random.randn(*imsize)
        if isinstance(dtype, torch.dtype):
            b0 = _dev.to_dev(b0, dtype)         # device tensors throughout
        elif dtype is not None:
            b0 = b0.astype(dtype)
    bd = _dev.to_dev(b0).clone()
    out = _dev.scratch()[1]

    # the fused path: A as the library's own operator on device tensors (HessianPsf or the band-coupled ParamHessian)
    H = None
    if not _dev.is_numpy(b0):
        from .pcg import _as_hessian
        from ..operators.hessian import ParamHessian
        H = _as_hessian(A, bd)
        if isinstance(H, ParamHessian):
            if H.plan.rdtype != bd.dtype:
                H = None
            elif H.plan.embed is not None:
                A, H = H, None    # embedded plan: the operator as a whole (its fused apply pads and crops), plain dots
        elif H is not None and (H.plan.rdtype != bd.dtype or H.plan.embed is not None or
                                tuple(bd.shape[-2:]) != (H.nx, H.ny) or (bd.ndim == 3 and bd.shape[0] != H.nb)
                                or (bd.ndim == 2 and H.nb != 1)):
            H = None
    bout = torch.empty_like(bd) if H is not None else None

    _dev.axpby(0.0, bd, 1.0 / math.sqrt(allsum([_dev.dot(bd, bd)])[0]), bd)
    bp = bd.clone()
    b = bd
    beta, eps, k = 1.0, 1.0, 0
    while eps > tol and k < maxit:
        if H is not None:
            H.apply_dots(bp, bout, out)                            # out[0] = <bp, b>, out[2] = <b, b>
            b = bout
            _dev.dot_into(bp, bp, out, 1)
            pb, pp, bb = allsum(out[:3].tolist())
        else:
            b = _dev.to_dev(A(_dev.host_like(bp, b0)), bp.dtype)
            _dev.dot_into(bp, b, out, 0)
            _dev.dot_into(bp, bp, out, 1)
            _dev.dot_into(b, b, out, 2)
            pb, pp, bb = allsum(out[:3].tolist())                  # ONE host look per iteration
        bnorm = math.sqrt(bb)
        betap = beta
        beta = pb / pp
        bp.copy_(b)
        _dev.axpby(0.0, bp, 1.0 / bnorm, bp)     # b /= bnorm ; bp[...] = b
        eps = abs(beta - betap) / betap
        k += 1
        if not k % report_freq and verbosity > 1:
            print(f"At iteration {k} eps = {eps:.3e}", file=sys.stderr)
    if verbosity:
        if k == maxit:
            print(f"Maximum iterations reached. eps = {eps:.3e}, beta = {beta:.3e}", file=sys.stderr)
        else:
            print(f"Success, converged after {k} iterations. beta = {beta:.3e}", file=sys.stderr)
    return beta, _dev.host_like(bp, b0)
