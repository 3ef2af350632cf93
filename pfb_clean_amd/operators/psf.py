"""
PSF convolution on MI355X -- drop-in for pfb/operators/psf.py:11-56.

    psf_convolve_slice(xpad, xhat, xout, psfhat, lastsize, x, nthreads=1)
    psf_convolve_cube (xpad, xhat, xout, psfhat, lastsize, x, nthreads=1)

Same positional order and aliasing contract as the reference: the result is written
into and returned as `xout` (psf.py:29,56) and `x` is not overwritten.  `xpad`/`xhat`
are the reference's host scratch buffers; the HIP path never materialises the padded
image or its spectrum, so they are accepted and ignored (None is fine).  numpy
arguments are staged through the GPU (PCIe both ways per call); torch-ROCm tensors
stay resident -- that is the fast way to drive it.

The psfhat re-layout happens once per distinct psfhat (plan cache keyed on the
buffer identity + a strided fingerprint), mirroring how the workers bind psfhat once
with functools.partial (workers/spotless.py:175-183).
"""
import ctypes as C
import threading

import torch

from .. import _lib, _dev
from .._plan import NativePlan, PlanCache, array_key


def _pow2ceil(n):
    p = 1
    while p < n:
        p *= 2
    return p


# what the kernels take (csrc): the fast path serves images whose axes are 2^k, 3 2^k or 5 2^k long -- 64 <= nx <= 8192
# (96 .. 6144, 160 .. 5120), 128 <= ny <= NY_FAST_MAX (160 .. 12288, fp64 6144) -- with nx_psf = 2 nx, ny_psf = 2 ny; the
# coverage ("generic") kernels hold one line in two LDS buffers
NX_FAST_MAX = 8192
NY_FAST_MAX = {torch.float32: 16384, torch.float64: 8192}
LINE_MAX = {torch.float32: 10240, torch.float64: 5120}
# Every 3 2^k / 5 2^k length the library takes (csrc/fftconv_pow2.hip): a plan created for such a size runs natively.
MIX_ALL = {
    'nx': {torch.float32: (96, 6144), torch.float64: (96, 6144)},
    'ny': {torch.float32: (160, 12288), torch.float64: (160, 6144)},
}
# The ones _embed_grid OFFERS, per axis: those that measured faster per plan.apply than the power-of-two grid the
# problem had before, by more than the run-to-run spread (profiles/mixed_conv_sweep.md).  The plain kernels these
# lengths run are about 2 x slower per pixel than the persistent power-of-two kernels.  The row kernels still win where
# the next power of two is 8192: fp32 rows of 5120 / 6144 pixels on power-of-two columns, 0.88-0.91 of the time.  The
# plain column kernel loses to the persistent ones (5120 x 8192 +8 % against 8192^2, 6144 x 4096 +15 %), 3072^2 fp32
# (+9 % against 4096^2) and 1536^2 fp64 (+2 % against 2048^2) lost, the shorter lengths and fp64 above 1536 were not
# timed: none of them is offered, and an image that IS such a size is embedded in the next power of two as before.
MIX_OFFERED = {
    'nx': {torch.float32: (), torch.float64: ()},
    'ny': {torch.float32: (5120, 6144), torch.float64: ()},
}


def _mix_lengths(lo, hi):
    """Ascending: the lengths 3 2^k and 5 2^k in [lo, hi]."""
    out, p = [], 1
    while p <= hi:
        out += [n for n in (3 * p, 5 * p) if lo <= n <= hi]
        p *= 2
    return sorted(out)


def _fast_lengths(lo, hi, mix):
    """Ascending: the powers of two in [lo, hi] and the lengths `mix`."""
    out, p = list(mix), 1
    while p <= hi:
        if p >= lo:
            out.append(p)
        p *= 2
    return sorted(out)


def is_fast_size(nx, ny, rdtype):
    """Whether an (nx, ny) image with a (2 nx, 2 ny) PSF is a size the fast kernels take natively."""
    xs = _fast_lengths(64, NX_FAST_MAX, _mix_lengths(*MIX_ALL['nx'][rdtype]))
    ys = _fast_lengths(128, NY_FAST_MAX[rdtype], _mix_lengths(*MIX_ALL['ny'][rdtype]))
    return nx in xs and ny in ys and nx % 32 == 0


def _fast_ceil(n, lengths):
    """The smallest of `lengths` that holds n, or None."""
    return next((m for m in lengths if m >= n), None)


def _embed_grid(nx, ny, nx_psf, ny_psf, rdtype):
    """(nx2, ny2) of the fast-path plan an (nx, ny | nx_psf, ny_psf) problem is embedded in -- per axis the smallest
    length among the powers of two and the offered 3 2^k / 5 2^k lengths (MIX_OFFERED) -- or None: already
    a fast-path size, switched off (PFB_NO_EMBED / PFB_FORCE_GENERIC), odd ny_psf, or beyond the fast kernels.
    Problems the coverage kernels can run (every line fits the LDS) are only embedded when the padded problem has
    at most 3x the pixels; problems they cannot run (nx_psf > 10240 fp32 / 5120 fp64: 6000^2, 7200^2 ... images
    with psf-oversize 2) are embedded whenever the fast path can hold them."""
    import os
    if os.environ.get('PFB_NO_EMBED', '0') not in ('', '0') or os.environ.get('PFB_FORCE_GENERIC', '0') not in ('', '0'):
        return None
    if ny_psf % 2:
        return None
    nx2 = _fast_ceil(nx, _fast_lengths(64, NX_FAST_MAX, MIX_OFFERED['nx'][rdtype]))
    ny2 = _fast_ceil(ny, _fast_lengths(128, NY_FAST_MAX[rdtype], MIX_OFFERED['ny'][rdtype]))
    if nx2 is None or ny2 is None:
        return None
    if (nx2, ny2) == (nx, ny) and (nx_psf, ny_psf) == (2 * nx, 2 * ny):
        return None
    generic_ok = max(nx_psf, ny_psf // 2) <= LINE_MAX[rdtype]
    if generic_ok and nx2 * ny2 > 3 * nx * ny:
        return None
    return nx2, ny2


class PsfConvPlan(NativePlan):
    """Owns the device plan (twiddles, re-laid-out psfhat, spectrum workspace) for one
    psfhat cube.  psfhat: (nband, nx_psf, nyo2) or (nx_psf, nyo2) complex.

    plan_for() hands the SAME plan to every host thread that presents the same psfhat (the reference's dask threads
    do, pcg.py:346-356), so `lock` is held for the enqueue of an apply and for a whole fused solve, and a caller on a
    different stream than the previous user first waits for that stream's work (NativePlan.run).

    `psf` (keyword, what from_psf passes instead of psfhat): the real PSF cube as a contiguous device tensor of a
    fast-path size; the library transforms it itself, into `psfhat_out` as well when that is given."""
    _destroy = 'pfb_psfconv_plan_destroy'

    def __init__(self, psfhat, nx, ny, lastsize, *, psf=None, psfhat_out=None):
        super().__init__()
        self.nx, self.ny, self.lastsize = int(nx), int(ny), int(lastsize)
        self.embed = None
        if psf is None:
            ph = _dev.to_dev(psfhat)
            if ph.dtype not in _dev.REAL_OF:
                raise TypeError(f"psfhat must be complex64/complex128, got {ph.dtype}")
            if ph.ndim == 2:
                ph = ph[None]
            if ph.ndim != 3:
                raise ValueError("psfhat must be (nx_psf, nyo2) or (nband, nx_psf, nyo2)")
            self.nband, self.nx_psf, self.nyo2 = ph.shape
            if self.nyo2 != self.lastsize // 2 + 1:
                raise ValueError(f"psfhat last axis {self.nyo2} != lastsize//2+1 "
                                 f"({self.lastsize // 2 + 1})")
            self.rdtype, self.device = _dev.REAL_OF[ph.dtype], ph.device
        else:
            self.nband, self.nx_psf = (int(v) for v in psf.shape[:2])
            self.nyo2 = self.lastsize // 2 + 1
            self.rdtype, self.device = psf.dtype, psf.device
        self.code = _dev.code(self.rdtype)
        cnx, cny, cpx, cpy = self.nx, self.ny, self.nx_psf, self.lastsize
        if psf is None:
            # Arbitrary sizes on the fast kernels: the same image-space PSF is re-gridded
            # (pfb_psfhat_regrid) onto nx_psf2 = 2 nx2, ny_psf2 = 2 ny2 with nx2, ny2 the next lengths
            # 2^k, 3 2^k or 5 2^k, images are zero-padded into (nx2, ny2) buffers and results cropped.  Identical
            # results to rounding, 3-6x faster than the line-per-workgroup coverage kernels
            # (measured: 3600^2 x 2 bands 3.2 ms generic vs 0.55 ms for two 4096^2 bands).
            grid2 = _embed_grid(self.nx, self.ny, self.nx_psf, self.lastsize, self.rdtype)
            if grid2 is not None:
                ph2 = self._regrid(ph.contiguous(), grid2)
                if ph2 is not None:
                    self.embed = grid2
                    ph = ph2
                    cnx, cny, cpx, cpy = grid2[0], grid2[1], 2 * grid2[0], 2 * grid2[1]
        _lib.check(self._lib.pfb_psfconv_plan_create(cnx, cny, cpx, cpy, self.nband, self.code, C.byref(self._h)))
        try:
            if psf is None:
                _lib.check(self._lib.pfb_psfconv_set_psfhat(self._h, _dev.ptr(ph.contiguous()), _dev.stream()))
            else:
                _lib.check(self._lib.pfb_psfconv_set_psf(self._h, _dev.ptr(psf), _dev.ptr(psfhat_out), _dev.stream()))
        except Exception:
            self.close()
            raise
        torch.cuda.current_stream().synchronize()      # psfhat / psf may be a temporary
        fast, vb, wsb = C.c_int(), C.c_int(), C.c_size_t()
        self._lib.pfb_psfconv_plan_info(self._h, C.byref(fast), C.byref(vb), C.byref(wsb))
        self.fast_path, self.vb, self.workspace_bytes = bool(fast.value), vb.value, wsb.value

    def _regrid(self, ph, grid2):
        """psfhat on the caller's grid -> psfhat on the (2 nx2, 2 ny2) grid, or None when the
        library cannot do it (prime factor > 13).  Done in fp64 (memory permitting: the detour holds
        the spectrum, the PSF and the embedded PSF of all bands at once), so that fp32 plans see no extra
        rounding from it."""
        nx2, ny2 = grid2
        cdt = ph.dtype
        # fp64 working set of pfb_psfhat_regrid: spec + psf + psf2 + psfhat2 (+ transform scratch)
        need64 = 16 * self.nband * (self.nx_psf * self.nyo2 * 2 + 2 * nx2 * (ny2 + 1) * 2) + 8 * self.nband * (
            self.nx_psf * self.lastsize + 4 * nx2 * ny2) * 2
        try:
            free = torch.cuda.mem_get_info(ph.device)[0]
        except Exception:
            free = 0
        works = ((torch.complex128, 1), (cdt, self.code)) if need64 < 0.6 * free else ((cdt, self.code),)
        for work in works:
            src = ph.to(work[0]) if ph.dtype != work[0] else ph
            dst = torch.empty((self.nband, 2 * nx2, ny2 + 1), dtype=work[0], device=ph.device)
            rc = self._lib.pfb_psfhat_regrid(work[1], _dev.ptr(src), self.nband, self.nx, self.ny,
                                             self.nx_psf, self.lastsize, 2 * nx2, 2 * ny2, _dev.ptr(dst),
                                             _dev.stream())
            if rc == _lib.PFB_OK:
                return dst.to(cdt)
            if rc != _lib.PFB_ERR_UNSUPPORTED:
                _lib.check(rc)
            if work[0] == cdt:
                break
        return None

    # ---- the padded domain.  An embedded plan computes on `embed`, a grid larger than the (nx, ny) image.  The image sits
    # in its corner and everything outside is ZERO: the input, and the beam (ones where the caller has none) of whoever
    # iterates there.  Outside the image a zero beam makes [beam*]conv([beam*]x) vanish, the operator reduces to sigmainv x
    # and maps zero to zero, so an iteration that starts from zero-padded arrays (a fused solve's b, x0 and with them
    # r, y, p; ParamHessian's e and both band mixes) stays exactly zero there and every inner product, step length and
    # stopping decision equals the un-padded one's.  A single apply needs no beam for that: its output is cropped.
    @property
    def grid(self):
        """The (nx, ny) the native plan computes on: `embed`, or the image's own."""
        return self.embed or (self.nx, self.ny)

    def to_grid(self, t, nb):
        """(nb, nx, ny) image cube -> a fresh zero-padded (nb,) + grid copy; t itself (None included) when not embedded."""
        if t is None or self.embed is None:
            return t
        z = torch.zeros((nb,) + self.embed, dtype=self.rdtype, device=t.device)
        z[:, :self.nx, :self.ny] = t
        return z

    def from_grid(self, t):
        """The image part of a (nb,) + grid cube, contiguous; t itself when not embedded."""
        return t if self.embed is None else t[:, :self.nx, :self.ny].contiguous()

    def grid_beam(self, beam, nb):
        """The beam an iteration on the grid multiplies by: `beam` -- ones where there is none -- zero outside the image;
        `beam` itself when not embedded."""
        if beam is None and self.embed is not None:
            beam = torch.ones((nb, self.nx, self.ny), dtype=self.rdtype, device=self.device)
        return self.to_grid(beam, nb)

    def _staging(self, nb, stream):
        """The cached (in, out) pair of (nb,) + grid buffers an embedded apply goes through, per stream (its handle) and
        host thread like _solve_work.  The margins of `in` are written once (zeros) and never again: a call costs one
        copy in and one out.  Only _on_grid touches them, inside the plan's critical section."""
        cache = self.__dict__.setdefault('_pad_cache', {})
        key = (nb, self.device, stream, threading.get_ident())
        if key not in cache:
            cache[key] = (torch.zeros((nb,) + self.embed, dtype=self.rdtype, device=self.device),
                          torch.empty((nb,) + self.embed, dtype=self.rdtype, device=self.device))
        return cache[key]

    def _on_grid(self, fn_name, x, out, args):
        """out = fn_name(x) for contiguous (nb, nx, ny) image cubes: run(fn_name, *args(xs, os)) with xs, os the cubes
        themselves or, embedded, the staging pair -- filled, used and copied out under `lock`, after the stream
        dependency, so that no earlier user of the pair can still be reading it."""
        if self.embed is None:
            return self.run(fn_name, *args(x, out))
        with self.lock:
            xs, os_ = self._staging(x.shape[0], self._enter_stream())
            xs[:, :self.nx, :self.ny] = x
            self.run(fn_name, *args(xs, os_))
            out.copy_(os_[:, :self.nx, :self.ny])

    def _solve_work(self, kind, nb):
        """Device scratch of a fused solve (opt/pcg.py) in the layout `kind` ('' the cube solve's, 'bands_', 'param_':
        pfb_pcg_<kind>work_bytes), kept on the plan like the padded buffers of apply() and freed with it.  Per stream and
        per host thread: the reference may drive per-band solves from several dask threads (pcg.py:346-356); solves on
        ONE plan are serialised by `lock`, but a thread's result must not be overwritten by the next thread's solve."""
        cache = self.__dict__.setdefault('_work_cache', {})
        key = (kind, nb, _dev.stream(), threading.get_ident())
        if key not in cache:
            nbytes = getattr(self._lib, f'pfb_pcg_{kind}work_bytes')(self._h, nb)
            cache[key] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return cache[key]

    @classmethod
    def from_psf(cls, psf, nx, ny, want_psfhat=False, *, image=None):
        """Build the plan straight from the real PSF cube (nband, nx_psf, ny_psf) | (nx_psf, ny_psf):
        psfhat = r2c(ifftshift(psf)) is produced by the library's own kernels
        (pfb_psfconv_set_psf; gridder.py:712-714) and never leaves the device.  With
        want_psfhat=True also returns it in the reference's layout.
        image: the shape of the images the plan is applied to when they are SMALLER than (nx, ny) -- a kernel that was
        laid out on a fast-path grid (nx, ny | 2 nx, 2 ny) for them; the plan is then embedded in that grid."""
        p = _dev.to_dev(psf)
        if p.ndim == 2:
            p = p[None]
        if p.ndim != 3 or p.dtype not in (torch.float32, torch.float64):
            raise ValueError("psf must be a real (nband, nx_psf, ny_psf) or (nx_psf, ny_psf) array")
        nband, nx_psf, ny_psf = (int(v) for v in p.shape)
        image = None if image is None or tuple(image) == (nx, ny) else tuple(int(v) for v in image)
        if _embed_grid(int(nx), int(ny), nx_psf, ny_psf, p.dtype) is not None:
            if image is not None:
                raise ValueError(f"image {image}: ({nx}, {ny} | {nx_psf}, {ny_psf}) is not a fast-path grid to embed it in")
            # not a fast-path size: transform on the PSF's own grid first, then let the constructor
            # re-grid it onto the fast-path plan (operators/fft.py picks the native producer)
            from .fft import psfhat_from_psf
            ph = psfhat_from_psf(p)
            plan = cls(ph, nx, ny, ny_psf)
            return (plan, ph) if want_psfhat else plan
        ph = torch.empty((nband, nx_psf, ny_psf // 2 + 1), dtype=_dev.CPLX_OF[p.dtype],
                         device=p.device) if want_psfhat else None
        plan = cls(None, nx, ny, ny_psf, psf=p, psfhat_out=ph)
        if image is not None:
            if image[0] > plan.nx or image[1] > plan.ny:
                raise ValueError(f"image {image} does not fit the ({plan.nx}, {plan.ny}) grid")
            plan.embed, (plan.nx, plan.ny) = (plan.nx, plan.ny), image
        return (plan, ph) if want_psfhat else plan

    def apply(self, x, out=None, beam=None, wsum=None, sigmainv=0.0, band0=0,
              dot_with=None, dot_out=None):
        """out = [beam*]conv([beam*]x)[/wsum] + sigmainv*x on bands
        [band0, band0+nb) where nb = x.shape[0] (x is (nb, nx, ny) or (nx, ny)).  Embedded plans take and return
        images all the same: the padded domain (above) is inside."""
        squeeze = x.ndim == 2
        x3 = x[None] if squeeze else x
        if x3.dtype != self.rdtype or not x3.is_cuda:
            raise TypeError(f"x must be a {self.rdtype} GPU tensor, got {x3.dtype}")
        nb = x3.shape[0]
        if tuple(x3.shape[1:]) != (self.nx, self.ny):
            raise ValueError(f"x has shape {tuple(x.shape)}, plan is for ({self.nx},{self.ny})")
        x3 = x3.contiguous()
        if out is None:
            out3 = torch.empty_like(x3)
        else:
            out3 = out[None] if out.ndim == 2 else out
            if not out3.is_contiguous() or out3.dtype != self.rdtype or out3.shape != x3.shape:
                raise ValueError("out must be a contiguous tensor shaped like x")
        if beam is not None:
            beam = beam[None] if beam.ndim == 2 else beam
            if beam.shape != x3.shape:
                raise ValueError('Beam has incorrect shape')
            beam = beam.contiguous()
        if dot_with is not None:
            dot_with = dot_with.contiguous()
        bs, ds = self.to_grid(beam, nb), self.to_grid(dot_with, nb)      # embedded: cropped afterwards (the padded domain)
        self._on_grid('pfb_psfconv_apply', x3, out3, lambda xs, os_: (
            int(band0), int(nb), _dev.ptr(xs), _dev.ptr(bs), float(wsum) if wsum is not None else 0.0, float(sigmainv),
            _dev.ptr(os_), _dev.ptr(ds), _dev.ptr(dot_out)))
        return out3[0] if squeeze else out3

    def set_profiling(self, on):
        """on: False/0 off, True/1 every apply, N > 1 every N-th apply (each timed apply puts
        four event records = ~20 us on the stream)."""
        _lib.check(self._lib.pfb_psfconv_set_profiling(self._h, int(on)))

    def get_profile(self):
        """(ms_row_fwd, ms_col, ms_row_inv) summed over `napply` applies, napply."""
        ms = (C.c_double * 3)()
        n = C.c_int()
        _lib.check(self._lib.pfb_psfconv_get_profile(self._h, ms, C.byref(n)))
        return tuple(ms), n.value


# ------------------------------------------------------------------- plan cache
_cache = PlanCache(8)


def plan_for(psfhat, nx, ny, lastsize):
    """Plan cache for the reference-shaped call sites (a functools.partial re-presents the same
    psfhat on every call).  The key is _plan.array_key: numpy arrays on address + layout + a strided
    content sample; tensors on data_ptr + shape + version counter, and the cache entry keeps a
    reference to the tensor so that its memory cannot be freed and re-used by a DIFFERENT psfhat at
    the same address while the entry lives (clear_plan_cache() releases plans and references)."""
    key = (array_key(psfhat), int(nx), int(ny), int(lastsize))
    return _cache.get(key, lambda: (PsfConvPlan(psfhat, nx, ny, lastsize),
                                    psfhat if isinstance(psfhat, torch.Tensor) else None))[0]


def clear_plan_cache():
    _cache.clear()


# ---------------------------------------------------------------- reference API
def _run(psfhat, lastsize, x, xout, beam=None, wsum=None, sigmainv=0.0, fresh=False):
    """Stage x (and the beam, which must have x's shape), apply the cached plan, deliver: into and as `xout` -- or,
    fresh=True (operators/hessian.py), as a NEW array that `xout` receives as well."""
    xd = _dev.to_dev(x)
    nx, ny = xd.shape[-2:]
    plan = plan_for(psfhat, nx, ny, lastsize)
    if xd.dtype != plan.rdtype:
        raise TypeError(f"x is {xd.dtype} but psfhat is {psfhat.dtype}")
    bd = _dev.to_dev(beam, plan.rdtype) if beam is not None else None
    if bd is not None and tuple(bd.shape) != tuple(xd.shape):
        raise ValueError('Beam has incorrect shape')
    # never overwrite x: stage when xout aliases it
    buf = torch.empty_like(xd) if fresh else _dev.out_buffer(xout, xd, alias=False)
    plan.apply(xd, out=buf, beam=bd, wsum=wsum, sigmainv=sigmainv)
    if not fresh:
        return _dev.deliver(buf, xout, like=x)
    if xout is not None:
        _dev.deliver(buf, xout)
    return _dev.host_like(buf, x)


def psf_convolve_slice(xpad, xhat, xout, psfhat, lastsize, x, nthreads=1):
    """pfb/operators/psf.py:11-29.  x (nx, ny), psfhat (nx_psf, nyo2)."""
    if x.ndim != 2 or psfhat.ndim != 2:
        raise ValueError("psf_convolve_slice expects 2-D x and psfhat")
    return _run(psfhat, lastsize, x, xout)


def psf_convolve_cube(xpad, xhat, xout, psfhat, lastsize, x, nthreads=1):
    """pfb/operators/psf.py:32-56.  x (nband, nx, ny), psfhat (nband, nx_psf, nyo2)."""
    if x.ndim != 3 or psfhat.ndim != 3:
        raise ValueError("psf_convolve_cube expects 3-D x and psfhat")
    if x.shape[0] != psfhat.shape[0]:
        raise ValueError("x and psfhat disagree on the number of bands")
    return _run(psfhat, lastsize, x, xout)
