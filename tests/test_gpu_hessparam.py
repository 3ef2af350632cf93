"""
The band-coupled Hessian of the parametrised forward step on the MI355X (csrc/hessparam.hip, operators/hessian.py::
ParamHessian, pfb_pcg_solve_param):

    hesspsf(v) = 2 dhf(psf_convolve(df(v))) + sigmainv v                      workers/fwdbwd.py:246-252

The oracle is that composition built from oracle/solvers.py::setup_parametrisation and oracle/fftconv.psf_convolve_cube
(both pinned to the reference by tests/test_oracle_golden.py), in float64.

Inputs: psfhat as _psd_psfhat of tests/test_gpu_dist_compose.py; truth a point of 1.0 plus a 3 x 3 patch of 0.3 in every
band; resid = conv(truth) + 1e-4 randn; freq = linspace(1e9, 2e9, nband), sigma 0.8, lscale 0.5; x0 = 0.1 randn;
j = 2 resid; sigmainv = max(std(j), 1e-3) and 0.5; default_rng(5).
Shapes: 64 x 64 with a 128 x 128 PSF (the fast-path kernels; their rows start at 128 pixels, so operators/psf.py embeds
it in a 64 x 128 plan: e padded with zeros, 'id' a mask of ones), 24 x 20 with 48 x 40 (too small to embed at 3 x the
pixels: the coverage kernels), 33 x 31 (an odd number of pixels: the scalar mix kernels inside the operator and the
solver) and 64 x 128 with 128 x 256 (the fast path as it is, nothing embedded: the path power_method fuses).  The PSF
grid of the 33 x 31 image is 66 x 64 and not 66 x 62: pfb_psfconv_plan_create takes 13-smooth lengths only
(62 / 2 = 31 is prime) and the convolution is not this file's subject; the image, whose odd pixel count is what the
case is for, is unchanged.

Bounds
  mix kernels   |got - ref| <= (nband + 3) eps sum_l |A_kl| |x_l|  (tests/clean_cases.py::freqmul_ref and the bound
                tests/test_gpu_clean.py uses with it) + eps |sigmainv p| for the Tikhonov term (one fused multiply-add);
                eps the unit roundoff.  The three sums against an fp64 host sum of the RETURNED Ap:
                n 2^-53 sum |a_i b_i|, the worst case of an fp64 accumulation of n terms.
  apply         err(route) = max|route - oracle64| / max|oracle64|;  err(fused) <= 2 err(unfused) + 16 eps, the unfused
                route being the closure composition on device tensors.  The factor 2: the fused route rounds e (L v) and
                scale e c inside the convolution instead of beside it.
  solves fp64   1e-9 max|x_ref| (test_fwdbwd_composition_config4_reduced's); fp32: the rule of
                tests/test_gpu_conv_pcg.py -- fp32 iterates are pinned only up to line-search ties, the relative residual
                of the normal equations, evaluated with the fp64 oracle operator, is at most 1.5 x the generic path's.
  power method  |beta - beta_ref| < 1e-10 beta_ref;  composition: 1e-8 relative for x and v (the existing tests' bounds).
"""
from functools import partial

import numpy as np
import pytest
import torch

import clean_cases as cc
from oracle import fftconv as ofc, solvers as osv, wavelets as owv

pytestmark = pytest.mark.gpu
pmp = pytest.mark.parametrize

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
EPS = {F32: 2.0 ** -24, F64: 2.0 ** -53}
CPLX = {F32: np.complex64, F64: np.complex128}
SHAPES = {'embedded': (64, 64, 128, 128), 'small': (24, 20, 48, 40), 'odd': (33, 31, 66, 64), 'fast': (64, 128, 128, 256)}
MODES = ['id', 'exp']
SENTINEL = -777.25
GUARD = 64
MIX_GRID_CAP = 1024 * 256          # threads of the capped grid: one 16-byte vector (or one element) each per trip


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def relerr(a, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(np.asarray(a, dtype=np.float64) - ref).max() / np.abs(ref).max())


# ------------------------------------------------------------------------------------------ 1. the mix kernels
def mix_call(dtype, A, c, sigmainv=0.0, p=None, r=None, dots=False, alias=False, offset=0, nband=None):
    """pfb_bandmix_dots with `out` pre-filled and a guard band behind it (alias: out IS c's buffer; offset: every array
    starts `offset` elements into its allocation).  Returns (rc, out, guard intact, dots | None)."""
    from pfb_clean_amd import _lib, _dev
    lib = _lib.load()
    nb, npix = c.shape
    tdt = torch.float32 if dtype == F32 else torch.float64

    def dev(a):
        if a is None:
            return None
        buf = torch.empty(a.size + offset, dtype=tdt, device='cuda')
        buf[offset:] = cuda(a.astype(dtype)).reshape(-1)
        return buf[offset:]
    Ad, pd, rd = cuda(A.astype(dtype)), dev(p), dev(r)
    buf = torch.full((offset + nb * npix + GUARD,), SENTINEL, dtype=tdt, device='cuda')
    if alias:
        buf[offset:offset + nb * npix] = cuda(c.astype(dtype)).reshape(-1)
        cd = buf[offset:]
    else:
        cd = dev(c)
    ws, d3 = _dev.scratch()
    d3.zero_()
    rc = lib.pfb_bandmix_dots(_dev.code(tdt), _dev.ptr(Ad), _dev.ptr(cd), nb if nband is None else nband, npix,
                              float(sigmainv), _dev.ptr(pd), _dev.ptr(rd), _dev.ptr(buf[offset:]),
                              _dev.ptr(d3) if dots else None, _dev.ptr(ws) if dots else None, _dev.stream())
    torch.cuda.synchronize()
    host = buf.cpu().numpy()[offset:]
    return (rc, host[:nb * npix].reshape(nb, npix), bool(np.all(host[nb * npix:] == SENTINEL)),
            d3[:3].cpu().numpy().copy() if dots else None)


def check_mix(dtype, nband, npix, offset=0):
    A, c, p, r = cc.freqmul_case(dtype, nband, npix)
    ref, mag = cc.freqmul_ref(A, c, None, None)
    eps, sig = EPS[dtype], 0.37
    worst = 0.0
    # the plain mix
    rc, out, guard, _ = mix_call(dtype, A, c, offset=offset)
    assert rc == 0 and guard and out.dtype == dtype
    ratio = float((np.abs(out.astype(np.float64) - ref) / (eps * mag)).max())
    assert ratio <= nband + 3, (nband, npix, ratio)
    worst = max(worst, ratio)
    # Tikhonov term and the three sums, with and without r
    # in extended precision: a float64 product and sum would carry the very roundings the bound is about
    LD = np.longdouble
    sp = LD(dtype.type(sig)) * p.astype(LD)
    for rr in (r, None):
        rc, ap, guard, dots = mix_call(dtype, A, c, sigmainv=sig, p=p, r=rr, dots=True, offset=offset)
        assert rc == 0 and guard
        err = np.abs(ap.astype(LD) - (ref.astype(LD) + sp))
        assert np.all(err <= (nband + 3) * eps * mag + eps * np.abs(sp)), (nband, npix, float(err.max()))
        a64 = ap.astype(np.float64)
        n = a64.size
        for q, other in enumerate((p, rr, ap)):
            if other is None:
                assert dots[q] == 0.0
                continue
            o64 = other.astype(np.float64)
            assert abs(dots[q] - float(np.sum(o64 * a64))) <= n * 2.0 ** -53 * float(np.sum(np.abs(o64 * a64))), (q, nband, npix)
        # Ap written over c: the same bits
        rc, ap2, guard, dots2 = mix_call(dtype, A, c, sigmainv=sig, p=p, r=rr, dots=True, alias=True, offset=offset)
        assert rc == 0 and guard and np.array_equal(ap, ap2) and np.array_equal(dots, dots2)
    # Tikhonov term without the sums
    rc, ap3, guard, _ = mix_call(dtype, A, c, sigmainv=sig, p=p, offset=offset)
    assert rc == 0 and guard and np.array_equal(ap3, ap)
    print(f'bandmix {dtype.name} nband {nband} npix {npix} offset {offset}: worst error {worst:.2f} eps sum|A||x| '
          f'(bound {nband + 3})')


@pmp('dtype', [F32, F64])
@pmp('nband', [1, 2, 3, 5, 8, 16])
def test_bandmix_edges(nband, dtype):
    """npix 1, 3, 4 (below, at the vector width), 255, 256, 257 (a workgroup less one, full, plus one: vector and scalar
    kernels); every compile-time band count family through 1, 2, 3, 5, 8, 16."""
    for npix in (1, 3, 4, 255, 256, 257):
        check_mix(dtype, nband, npix)


@pmp('dtype', [F32, F64])
def test_bandmix_capped_grid_and_offset_base(dtype):
    """Beyond the grid cap of 1024 workgroups on the vector kernel (a second trip for some threads of both dtypes) and,
    with an odd plane, on the scalar kernel; and a base pointer one element off 16-byte alignment (scalar kernel on a
    size the vector kernel would take)."""
    check_mix(dtype, 2, 4 * MIX_GRID_CAP + 20)
    check_mix(dtype, 2, MIX_GRID_CAP + 1)
    check_mix(dtype, 3, 256, offset=1)


def test_bandmix_rejects_more_than_16_bands():
    from pfb_clean_amd import _lib
    A, c, p, r = cc.freqmul_case(np.float64, 17, 5)
    rc, out, guard, _ = mix_call(F64, A, c, sigmainv=0.5, p=p, r=r, dots=True)
    assert rc == _lib.PFB_ERR_UNSUPPORTED and guard and np.all(out == SENTINEL)
    assert mix_call(F64, A, c, nband=0)[0] == _lib.PFB_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------ shared inputs
def _psd_psfhat(rng, nb, P, Q):
    u = np.fft.fftfreq(P)[:, None]
    v = np.fft.rfftfreq(Q)[None, :]
    W = rng.poisson(4 * np.exp(-(u ** 2 + v ** 2) / (2 * 0.12 ** 2)), size=(nb, P, Q // 2 + 1)).astype(np.float64)
    W /= nb * np.fft.irfft2(W, s=(P, Q)).max(axis=(1, 2))[:, None, None]
    return W.astype(np.complex128)


class Case:
    """One (shape, nband) problem in float64 on the host, with the oracle operator per (mode, sigmainv)."""

    def __init__(self, shape, nband):
        self.nx, self.ny, self.P, self.Q = nx, ny, P, Q = SHAPES[shape]
        self.nb = nband
        rng = np.random.default_rng(5)
        self.psfhat = _psd_psfhat(rng, nband, P, Q)
        truth = np.zeros((nband, nx, ny))
        truth[:, nx // 3, ny // 2] = 1.0
        truth[:, nx // 2:nx // 2 + 3, ny // 4:ny // 4 + 3] = 0.3
        self.scratch = ofc.make_scratch(self.psfhat, Q, truth.shape, np.float64)
        self.resid = self.oconv(truth).copy() + 1e-4 * rng.standard_normal(truth.shape)
        self.freq = np.linspace(1e9, 2e9, nband)
        self.x0 = 0.1 * rng.standard_normal(truth.shape)
        self.j = 2 * self.resid
        self.sigmainv = max(float(np.std(self.j)), 1e-3)
        self.v = rng.standard_normal(truth.shape)
        self.b0 = rng.standard_normal(truth.shape)
        self.xstart = 0.05 * rng.standard_normal(truth.shape)
        self._par = {}

    def oconv(self, x):
        return ofc.psf_convolve_cube(*self.scratch, self.psfhat, self.Q, x)

    def oracle(self, mode, sigmainv):
        if mode not in self._par:
            self._par[mode] = osv.setup_parametrisation(mode, sigma=0.8, freq=self.freq, lscale=0.5)
        _, _, odf, odhf = self._par[mode]
        return lambda v: 2 * odhf(self.x0, self.oconv(odf(self.x0, v))) + v * sigmainv

    def device(self, mode, dtype, sigmainv, **kw):
        """(hesspsf partial as the worker builds it, its pieces) on device tensors of `dtype`."""
        from pfb_clean_amd.operators.psf import psf_convolve_cube
        from pfb_clean_amd.operators.hessian import hessian_psf
        from pfb_clean_amd.utils.misc import setup_parametrisation
        _, _, dfunc, dhfunc = setup_parametrisation(mode, sigma=0.8, freq=self.freq, lscale=0.5)
        ph = cuda(self.psfhat.astype(CPLX[dtype]))
        x0 = cuda(self.x0.astype(dtype))
        conv = partial(psf_convolve_cube, None, None, None, ph, self.Q)
        df, dhf = partial(dfunc, x0), partial(dhfunc, x0)
        return partial(hessian_psf, conv, x0, sigmainv, df, dhf, **kw), (ph, x0, conv, dfunc, dhfunc)


_cases = {}


def case(shape, nband):
    if (shape, nband) not in _cases:
        _cases[shape, nband] = Case(shape, nband)
    return _cases[shape, nband]


@pytest.fixture(autouse=True)
def _fresh_plans():
    yield
    from pfb_clean_amd.operators.psf import clear_plan_cache
    clear_plan_cache()


# ------------------------------------------------------------------------------------------ 2. apply parity
@pmp('dtype', [F64, F32])
@pmp('mode', MODES)
@pmp('shape', list(SHAPES))
def test_apply_parity(shape, mode, dtype):
    from pfb_clean_amd.operators.hessian import ParamHessian
    for nband in (1, 2, 3, 5, 8, 16, 17):
        cs = case(shape, nband)
        for sigmainv in (cs.sigmainv, 0.5):
            ref = cs.oracle(mode, sigmainv)(cs.v)
            _, (ph, x0, conv, dfunc, dhfunc) = cs.device(mode, dtype, sigmainv)
            v = cuda(cs.v.astype(dtype))
            unfused = 2 * dhfunc(x0, conv(dfunc(x0, v))) + sigmainv * v
            H = ParamHessian(ph, cs.nx, cs.ny, cs.Q, x0, sigmainv, dfunc, dhfunc)
            assert H.fused == (nband <= 16) and (H.plan.embed is not None) == (shape == 'embedded')
            assert H.plan.fast_path == (shape in ('fast', 'embedded'))
            got = H(v)
            assert got.dtype == v.dtype and got.shape == v.shape
            eu, ef = relerr(unfused.cpu().numpy(), ref), relerr(got.cpu().numpy(), ref)
            print(f'apply {shape} {mode} {dtype.name} nband {nband} sigmainv {sigmainv:.3g}: fused {ef:.3e} unfused {eu:.3e}')
            assert ef <= 2 * eu + 16 * EPS[dtype], (nband, sigmainv, ef, eu)
            if nband == 3:                     # numpy in, numpy out; and into a caller's buffer
                gh = H(cs.v.astype(dtype))
                assert isinstance(gh, np.ndarray) and np.array_equal(gh, got.cpu().numpy())
                buf = torch.empty_like(v)
                assert H(v, out=buf) is buf and torch.equal(buf, got)


# ------------------------------------------------------------------------------------------ 3. solves, fp64
@pmp('mode', MODES)
@pmp('nband', [2, 4])
@pmp('shape', list(SHAPES))
def test_pcg_fp64(shape, nband, mode):
    from pfb_clean_amd.operators.hessian import ParamHessian
    from pfb_clean_amd.opt.pcg import pcg, _as_hessian
    cs = case(shape, nband)
    oH = cs.oracle(mode, cs.sigmainv)
    A, _ = cs.device(mode, F64, cs.sigmainv)
    jd = cuda(cs.j)
    H = _as_hessian(A, jd)
    assert isinstance(H, ParamHessian) and H.fused and H.mode == mode
    kw = dict(tol=0.0, maxit=15, minit=15)
    refs = {bt: osv.pcg(oH, cs.j, None, backtrack=bt, **kw) for bt in (False, True)}
    for bt in (False, True, 'exact'):
        x = pcg(A, jd, backtrack=bt, verbosity=0, **kw)
        ref = refs[bool(bt)]
        err = np.abs(x.cpu().numpy() - ref).max() / np.abs(ref).max()
        print(f'pcg {shape} nband {nband} {mode} backtrack {bt}: {err:.3e}')
        assert err < 1e-9, (bt, err)


@pmp('mode', MODES)
@pmp('shape', list(SHAPES))
def test_pcg_fp64_start_vector_residual_and_preconditioner(shape, mode):
    """A non-zero start, return_resid and M = x / sigmainv (as an object and as the closure the workers write), at
    sigmainv = 0.5; numpy arrays in and out as well."""
    from pfb_clean_amd.opt.pcg import pcg, DivPrecond
    cs = case(shape, 4)
    sig = 0.5
    oH = cs.oracle(mode, sig)
    A, _ = cs.device(mode, F64, sig)
    kw = dict(tol=0.0, maxit=15, minit=15)
    xo, ro = osv.pcg(oH, cs.j, cs.xstart.copy(), M=lambda w: w / sig, return_resid=True, **kw)
    for M in (DivPrecond(sig), lambda w: w / sig):
        x, r = pcg(A, cuda(cs.j), cuda(cs.xstart), M=M, return_resid=True, verbosity=0, **kw)
        assert np.abs(x.cpu().numpy() - xo).max() < 1e-9 * np.abs(xo).max()
        assert np.abs(r.cpu().numpy() - ro).max() < 1e-9 * np.abs(cs.j).max()
    xh = pcg(A, cs.j, cs.xstart.copy(), M=DivPrecond(sig), verbosity=0, **kw)
    assert isinstance(xh, np.ndarray) and np.abs(xh - xo).max() < 1e-9 * np.abs(xo).max()


# ------------------------------------------------------------------------------------------ 4. solves, fp32
@pmp('mode', MODES)
@pmp('nband', [2, 4])
@pmp('shape', list(SHAPES))
def test_pcg_fp32(shape, nband, mode):
    """Iterate parity at the project's fp32 PCG tolerance (tests/test_gpu_conv_pcg.py: 1e-3 between two fp32 solves,
    5e-3 against the fp64 oracle) -- always without the line search, which has no ties to lose; with it whenever the
    fused solve's backtracking history is the fp64 oracle's -- and in every case the residual rule."""
    from pfb_clean_amd.operators.hessian import ParamHessian
    from pfb_clean_amd.opt.pcg import pcg, pcg_fused, _as_hessian
    cs = case(shape, nband)
    oH = cs.oracle(mode, cs.sigmainv)
    A, _ = cs.device(mode, F32, cs.sigmainv)
    G, _ = cs.device(mode, F32, cs.sigmainv, _nofuse=True)
    jd = cuda(cs.j.astype(np.float32))
    H = _as_hessian(A, jd)
    assert isinstance(H, ParamHessian) and _as_hessian(G, jd) is None
    jn = np.linalg.norm(cs.j)
    kw = dict(tol=0.0, maxit=15, minit=15)
    for bt in (False, True):
        tr = osv.PCGTrace()
        xo = osv.pcg(oH, cs.j, None, backtrack=bt, trace=tr, **kw)
        nbt_ref = int(np.sum(tr.nbacktrack))
        xft, _, res = pcg_fused(H, jd, None, backtrack=bt, **kw)
        xf_t = pcg(A, jd, backtrack=bt, verbosity=0, **kw)
        assert res.iters == 15 and torch.equal(xf_t, xft)          # the drop-in call IS that solve
        xf = xft.cpu().numpy().astype(np.float64)
        xg = pcg(G, jd, backtrack=bt, verbosity=0, **kw).cpu().numpy().astype(np.float64)
        rf, rg = np.linalg.norm(oH(xf) - cs.j) / jn, np.linalg.norm(oH(xg) - cs.j) / jn
        eg, eo = relerr(xf, xg), relerr(xf, xo)
        print(f'pcg fp32 {shape} nband {nband} {mode} backtrack {bt}: fused - generic {eg:.3e}, fused - oracle64 '
              f'{eo:.3e}, backtracks {res.backtracks} (oracle {nbt_ref}), residual fused {rf:.4e} generic {rg:.4e} '
              f'ratio {rf / rg:.4f}')
        if not bt:
            assert res.backtracks == 0
        if not bt or res.backtracks == nbt_ref:
            assert eg < 1e-3 and eo < 5e-3, (bt, eg, eo)
        assert rf <= 1.5 * rg, (bt, rf, rg)


# ------------------------------------------------------------------------------------------ 5. power method
@pmp('mode', MODES)
@pmp('shape,nband', [('fast', 2), ('fast', 4), ('odd', 2), ('embedded', 2)])
def test_power_method(shape, nband, mode, monkeypatch):
    from pfb_clean_amd import _lib
    from pfb_clean_amd.opt.power_method import power_method
    cs = case(shape, nband)
    oH = cs.oracle(mode, cs.sigmainv)
    beta_ref, _ = osv.power_method(oH, cs.x0.shape, b0=cs.b0.copy(), tol=1e-6, maxit=60, verbosity=0)
    A, _ = cs.device(mode, F64, cs.sigmainv)
    lib, calls = _lib.load(), []
    native = lib.pfb_hessparam_apply_dots
    monkeypatch.setattr(lib, 'pfb_hessparam_apply_dots', lambda *a: calls.append(1) or native(*a), raising=False)
    whole, native_apply = [], lib.pfb_hessparam_apply
    monkeypatch.setattr(lib, 'pfb_hessparam_apply', lambda *a: whole.append(1) or native_apply(*a), raising=False)
    beta, bvec = power_method(A, cs.x0.shape, b0=cuda(cs.b0), tol=1e-6, maxit=60, verbosity=0)
    print(f'power_method {shape} nband {nband} {mode}: beta {beta:.12e} ref {beta_ref:.12e}, {len(calls)} fused applies')
    assert abs(beta - beta_ref) < 1e-10 * beta_ref
    # an embedded plan's operator is called as a whole: its fused apply, never the closures
    assert bool(calls) == (shape != 'embedded') and bool(whole) == (shape == 'embedded')


# ------------------------------------------------------------------------------------------ 6. fwdbwd composition
def test_fwdbwd_composition_parametrised():
    """power_method -> pcg -> primal_dual_optimised as workers/fwdbwd.py:310-375 composes them, with the parametrised
    Hessian ('exp') in all three: 2 bands x 64 x 128, bases self, db1, db2, 2 levels, 12 iterations, positivity 0.  The
    device gradient is ParamGradient(H, x0 + delx), i.e. H(v) - H(data); the oracle's is the worker's H(v - data)."""
    from pfb_clean_amd.operators.psi import Psi
    from pfb_clean_amd.opt.pcg import pcg, _as_hessian
    from pfb_clean_amd.opt.power_method import power_method
    from pfb_clean_amd.opt.primal_dual import primal_dual_optimised, ParamGradient, PsfGradient
    cs = case('fast', 2)
    nb, nx, ny = cs.x0.shape
    bases, nlevel, lam = ['self', 'db1', 'db2'], 2, 5e-4
    nbasis = len(bases)
    oH = cs.oracle('exp', cs.sigmainv)
    L_ref, _ = osv.power_method(oH, cs.x0.shape, b0=cs.b0.copy(), tol=1e-6, maxit=60, verbosity=0)
    delx_ref = osv.pcg(oH, cs.j, None, tol=0.0, maxit=15, minit=15)
    data_ref = cs.x0 + delx_ref
    opsi = owv.Psi(nb, nx, ny, bases, nlevel, 1)
    ov = np.zeros((nb, nbasis, opsi.Nymax, opsi.Nxmax))
    xb_ref, vb_ref = osv.primal_dual_optimised(cs.x0.copy(), ov, lam, opsi.hdot, opsi.dot, 1.05 * L_ref, None,
                                               np.ones(ov.shape[1:]), None, lambda w: oH(w - data_ref), nu=nbasis,
                                               tol=0.0, maxit=12, positivity=0)
    assert np.abs(vb_ref).max() > 0 and np.abs(xb_ref - cs.x0).max() > 0
    A, (ph, x0, conv, dfunc, dhfunc) = cs.device('exp', F64, cs.sigmainv)
    jd = cuda(cs.j)
    L, _ = power_method(A, cs.x0.shape, b0=cuda(cs.b0), tol=1e-6, maxit=60, verbosity=0)
    assert abs(L - L_ref) < 1e-10 * L_ref
    delx = pcg(A, jd, tol=0.0, maxit=15, minit=15, verbosity=0)
    assert np.abs(delx.cpu().numpy() - delx_ref).max() < 1e-9 * np.abs(delx_ref).max()
    grad = ParamGradient(_as_hessian(A, jd), x0 + delx)
    assert isinstance(grad, PsfGradient)
    w = cuda(cs.v)
    assert relerr(grad(w).cpu().numpy(), oH(cs.v - data_ref)) < 1e-11
    psi = Psi(nb, nx, ny, bases, nlevel, 1)
    v = torch.zeros((nb, nbasis, psi.Nymax, psi.Nxmax), dtype=torch.float64, device='cuda')
    xb, vb = primal_dual_optimised(x0.clone(), v, lam, psi.hdot, psi.dot, 1.05 * L, None, torch.ones_like(v[0]), None,
                                   grad, nu=nbasis, tol=0.0, maxit=12, positivity=0, verbosity=0)
    ex, ev = relerr(xb.cpu().numpy(), xb_ref), relerr(vb.cpu().numpy(), vb_ref)
    print(f'fwdbwd composition: x {ex:.3e} v {ev:.3e}')
    assert ex < 1e-8 and ev < 1e-8
