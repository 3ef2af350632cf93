"""
The 3 2^k and 5 2^k lengths of the fast convolution path (csrc/fftconv_pow2.hip: the plain column / row kernels on a
RegFft whose last pass has radix 3 or 5), natively and as the grid other sizes are embedded in, against the CPU oracle.

Tolerances are the project's own: conv 1e-12 fp64 / 1e-5 fp32, PCG iterate 1e-9 / 1e-3, relative to
max|reference|.  Every native case asserts `plan.fast_path and plan.embed is None`.

Offering.  `_embed_grid` offers only the lengths that measured faster than the power-of-two grid (fp32 rows of 5120 and
6144 pixels, profiles/mixed_conv_sweep.md); an image of any other 3 2^k / 5 2^k size is embedded in the next power of two as before.
The kernels of every class exist and are tested here all the same: the tests run with every class offered
(`all_classes_offered`), except the `test_default_*` ones, which pin what the shipped chooser does.

Classes.  Columns (nx): 96 .. 6144 and 160 .. 5120.  Rows (ny / 2): the same and 80 (ny = 160, the shortest 5 2^k row: 8
threads of 10 elements); fp64 rows up to 3072.
"""
from functools import partial

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from oracle import fftconv as ofc          # noqa: E402  (checker only)
from oracle import solvers as osv          # noqa: E402

pmp = pytest.mark.parametrize

TOL_CONV = {np.float64: 1e-12, np.float32: 1e-5}
TOL_PCG = {np.float64: 1e-9, np.float32: 1e-3}
EPS = {np.float64: 2.0 ** -53, np.float32: 2.0 ** -24}

MIX3 = [96, 192, 384, 768, 1536, 3072, 6144]
MIX5 = [160, 320, 640, 1280, 2560, 5120]
COL_CLASSES = MIX3 + MIX5
ROW_CLASSES = {np.float32: [80] + MIX3 + MIX5, np.float64: [n for n in [80] + MIX3 + MIX5 if n <= 3072]}


@pytest.fixture(scope='module')
def amd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from pfb_clean_amd import _lib, _dev
    from pfb_clean_amd.operators import psf, hessian
    from pfb_clean_amd.opt import pcg as pcgmod

    class NS:
        pass
    ns = NS()
    ns.lib, ns._lib, ns.dev, ns.psf, ns.hessian, ns.pcg = _lib.load(), _lib, _dev, psf, hessian, pcgmod
    return ns


@pytest.fixture(autouse=True)
def all_classes_offered(request, monkeypatch):
    """Every 3 2^k / 5 2^k class the library takes is offered by the chooser (not for the test_default_* tests)."""
    from pfb_clean_amd.operators import psf
    if not request.function.__name__.startswith('test_default_'):
        monkeypatch.setattr(psf, 'MIX_OFFERED', {ax: {dt: tuple(psf._mix_lengths(*rng)) for dt, rng in per.items()}
                                                 for ax, per in psf.MIX_ALL.items()})


@pytest.fixture(autouse=True)
def _fresh_plans():
    yield
    from pfb_clean_amd.operators.psf import clear_plan_cache
    clear_plan_cache()


def relerr(a, ref):
    a = np.asarray(a, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300)


def cdt(rdt):
    return np.complex64 if rdt == np.float32 else np.complex128


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ shared problems (float64 on the host, built once)
_problems = {}


def conv_problem(nb, nx, ny, P=None, Q=None):
    """Random PSF with a strong centre, random image, the oracle's convolution."""
    P, Q = P or 2 * nx, Q or 2 * ny
    key = ('conv', nb, nx, ny, P, Q)
    if key not in _problems:
        rng = np.random.default_rng(nx * 1000 + ny)
        psf = rng.standard_normal((nb, P, Q))
        psf[:, P // 2, Q // 2] += 5
        psfhat = ofc.psfhat_from_psf(psf)
        x = rng.standard_normal((nb, nx, ny))
        xpad, xhat, xout = ofc.make_scratch(psfhat, Q, x.shape, np.float64)
        ref = ofc.psf_convolve_cube(xpad, xhat, xout, psfhat, Q, x).copy()
        _problems[key] = (psf, psfhat, x, ref)
    return _problems[key]


def psd_psfhat(rng, nb, P, Q):
    """A positive spectrum (a PSF the PCG converges on), peak of the PSF 1 / nb."""
    u = np.fft.fftfreq(P)[:, None]
    v = np.fft.rfftfreq(Q)[None, :]
    W = rng.poisson(4 * np.exp(-(u ** 2 + v ** 2) / (2 * 0.12 ** 2)), size=(nb, P, Q // 2 + 1)).astype(np.float64)
    W /= nb * np.fft.irfft2(W, s=(P, Q)).max(axis=(1, 2))[:, None, None]
    return W.astype(np.complex128)


def check_native_conv(amd, nb, nx, ny, rdt):
    psf, psfhat, x, ref = conv_problem(nb, nx, ny)
    ph = psfhat.astype(cdt(rdt))
    plan = amd.psf.plan_for(ph, nx, ny, 2 * ny)
    assert plan.fast_path and plan.embed is None
    y = amd.psf.psf_convolve_cube(None, None, None, ph, 2 * ny, x.astype(rdt))
    err = relerr(y, ref)
    print(f'conv {nb} x {nx} x {ny} {np.dtype(rdt).name}: {err:.3e}')
    assert y.dtype == rdt and err < TOL_CONV[rdt]


# ----------------------------------------------------------------------------- 1. smallest classes and their mixes
@pmp('rdt', [np.float64, np.float32])
@pmp('shape', [(96, 192), (160, 320), (96, 128), (160, 128), (64, 192), (64, 320), (192, 320)])
def test_smallest_classes_and_mixes(amd, shape, rdt):
    """Inactive column groups in the last workgroup, 32-row tiles, both forms of row_fwd_post, and (ny = 192 / 320 / nx = 96
    / 160) transforms whose power-of-two passes are one butterfly per thread."""
    check_native_conv(amd, 2, shape[0], shape[1], rdt)


# ------------------------------------------------------------------------------- 2. every class, the other axis thin
@pmp('rdt', [np.float64, np.float32])
@pmp('nx', COL_CLASSES)
def test_every_column_class(amd, nx, rdt):
    check_native_conv(amd, 1, nx, 128, rdt)


@pmp('rdt,L', [(rdt, L) for rdt in (np.float64, np.float32) for L in ROW_CLASSES[rdt]])
def test_every_row_class(amd, L, rdt):
    """Up to the barrier-mode rows (more than 64 threads per row) and the longest row of each type."""
    check_native_conv(amd, 1, 64, 2 * L, rdt)


def test_row_classes_end_where_the_lds_does(amd):
    """fp64 rows beyond 3072 points are no class: the size is embedded (or left to the coverage kernels), not refused."""
    rng = np.random.default_rng(3)
    ph = cuda(ofc.psfhat_from_psf(rng.standard_normal((1, 128, 20480))))
    plan = amd.psf.PsfConvPlan(ph, 64, 10240, 20480)
    assert not plan.fast_path and plan.embed is None
    plan.close()


# ------------------------------------------------------------------ 3. a mixed axis against a persistent kernel
@pmp('shape,rdt', [((96, 4096), np.float32), ((2048, 192), np.float32),
                   ((96, 4096), np.float64),        # fp64 persistent inverse rows (2048 points) on 96 rows
                   ((160, 2048), np.float32),       # 1024-point persistent rows, 8-row tiles, on 160 rows
                   ((96, 8192), np.float32),        # 4096-point persistent rows (4-row tiles)
                   ((8192, 192), np.float32)])      # the two-level column kernel with 96-point rows
def test_mixed_axis_with_persistent_partner(amd, shape, rdt):
    check_native_conv(amd, 2, shape[0], shape[1], rdt)


# ----------------------------------------------------------------------------- 4. Hessian epilogue and fused sums
@pmp('rdt', [np.float64, np.float32])
@pmp('shape', [(96, 192), (160, 128)])
def test_hessian_epilogue_and_fused_sums(amd, shape, rdt):
    nx, ny = shape
    nb, Q = 2, 2 * ny
    psf, psfhat, x, _ = conv_problem(nb, nx, ny)
    rng = np.random.default_rng(11)
    beam = 0.5 + rng.random((nb, nx, ny))
    w = rng.standard_normal((nb, nx, ny))
    xpad, xhat, xout = ofc.make_scratch(psfhat, Q, x.shape, np.float64)
    ref = ofc.hessian_psf_cube(xpad, xhat, xout, beam, psfhat, Q, x, sigmainv=0.3, wsum=1.7)
    ph = psfhat.astype(cdt(rdt))
    got = amd.hessian.hessian_psf_cube(None, None, None, beam.astype(rdt), ph, Q, x.astype(rdt), sigmainv=0.3, wsum=1.7)
    assert relerr(got, ref) < TOL_CONV[rdt]
    plan = amd.psf.plan_for(ph, nx, ny, Q)
    assert plan.fast_path and plan.embed is None
    xt, wt, bt = cuda(x.astype(rdt)), cuda(w.astype(rdt)), cuda(beam.astype(rdt))
    _lib, _dev = amd._lib, amd.dev
    for two in (False, True):
        out = torch.empty_like(xt)
        dots = torch.zeros(3, dtype=torch.float64, device='cuda')
        _lib.check(amd.lib.pfb_psfconv_apply_dots(plan.handle, 0, nb, _dev.ptr(xt), _dev.ptr(bt), 1.7, 0.3, _dev.ptr(out),
                                                  _dev.ptr(wt), _dev.ptr(xt) if two else None, _dev.ptr(dots), _dev.stream()))
        o = out.cpu().numpy().astype(np.float64)
        d = dots.cpu().numpy()
        assert relerr(o, ref) < TOL_CONV[rdt]
        # fp64: against the oracle's numbers, 1e-9 relative (test_conv_tensor_path_and_fused_dot).  fp32: the sums are taken in
        # fp64 over the fp32 values the kernel wrote, so they are compared with those (test_persistent_row_kernels_multi_tile)
        w64, x64 = w.astype(rdt).astype(np.float64), x.astype(rdt).astype(np.float64)
        if rdt == np.float64:
            assert abs(d[0] - np.vdot(w64, ref)) < 1e-9 * abs(np.vdot(w64, ref))
            assert abs(d[2] - np.vdot(ref, ref)) < 1e-9 * np.vdot(ref, ref)
            if two:
                assert abs(d[1] - np.vdot(x64, ref)) < 1e-9 * abs(np.vdot(x64, ref))
        else:
            on = np.vdot(o, o) ** 0.5
            assert abs(d[0] - np.vdot(w64, o)) < 1e-9 * on * np.linalg.norm(w64)
            assert abs(d[2] - np.vdot(o, o)) < 1e-9 * np.vdot(o, o)
            if two:
                assert abs(d[1] - np.vdot(x64, o)) < 1e-9 * on * np.linalg.norm(x64)
        if not two:
            assert d[1] == 0.0


# ------------------------------------------------------------------------------------------------------ 5. solves
def pcg_problem(nb, nx, ny):
    key = ('pcg', nb, nx, ny)
    if key not in _problems:
        rng = np.random.default_rng(420 + nx)
        P, Q = 2 * nx, 2 * ny
        psfhat = psd_psfhat(rng, nb, P, Q)
        model = np.zeros((nb, nx, ny))
        model[:, nx // 3, ny // 2] = 1.0
        model[:, nx // 2, ny // 4] = 2.0
        scratch = ofc.make_scratch(psfhat, Q, model.shape, np.float64)
        b = ofc.psf_convolve_cube(*scratch, psfhat, Q, model).copy() + 1e-3 * rng.standard_normal(model.shape)
        sig = 1e-3 * np.abs(b).max()
        kw = dict(tol=0.0, maxit=8, minit=8)
        ref_cube = osv.pcg(lambda t: ofc.hessian_psf_cube(*scratch, None, psfhat, Q, t, sigmainv=sig), b, None,
                           M=lambda t: t / sig, **kw)
        ref_band = osv.pcg_psf(psfhat, b, np.zeros_like(b), None, Q, 1, sig, dict(verbosity=0, **kw))
        _problems[key] = (psfhat, b, sig, kw, ref_cube, ref_band)
    return _problems[key]


@pmp('rdt', [np.float64, np.float32])
@pmp('shape', [(96, 192), (160, 128)])
def test_fused_cube_pcg(amd, shape, rdt):
    nx, ny = shape
    psfhat, b, sig, kw, ref_cube, _ = pcg_problem(3, nx, ny)
    A = amd.hessian.HessianPsf(cuda(psfhat.astype(cdt(rdt))), nx, ny, 2 * ny, sigmainv=sig)
    assert A.plan.fast_path and A.plan.embed is None
    x = amd.pcg.pcg(A, cuda(b.astype(rdt)), None, M=amd.pcg.DivPrecond(sig), verbosity=0, **kw)
    err = relerr(x.cpu().numpy(), ref_cube)
    print(f'cube pcg {shape} {np.dtype(rdt).name}: {err:.3e}')
    assert err < TOL_PCG[rdt]


@pmp('rdt', [np.float64, np.float32])
def test_pcg_psf_per_band(amd, rdt):
    nx, ny = 96, 192
    psfhat, b, sig, kw, _, ref_band = pcg_problem(3, nx, ny)
    ph = psfhat.astype(cdt(rdt))
    assert amd.psf.plan_for(ph, nx, ny, 2 * ny).embed is None
    m = amd.pcg.pcg_psf(ph, b.astype(rdt), np.zeros_like(b, dtype=rdt), None, 2 * ny, 1, sig, dict(verbosity=0, **kw))
    err = relerr(m, ref_band)
    print(f'pcg_psf {np.dtype(rdt).name}: {err:.3e}')
    assert m.dtype == rdt and err < TOL_PCG[rdt]


@pmp('rdt', [np.float64, np.float32])
def test_param_hessian_apply(amd, rdt):
    """ParamHessian (mode exp, three bands) on a native 96 x 192 plan against the unfused composition of the same device
    pieces; bound as in test_gpu_hessparam.py::test_apply_parity: fused error <= 2 x unfused error + 16 eps."""
    from pfb_clean_amd.operators.hessian import ParamHessian
    from pfb_clean_amd.operators.psf import psf_convolve_cube
    from pfb_clean_amd.utils.misc import setup_parametrisation
    nb, nx, ny = 3, 96, 192
    Q = 2 * ny
    rng = np.random.default_rng(5)
    psfhat = psd_psfhat(rng, nb, 2 * nx, Q)
    freq = np.linspace(1e9, 2e9, nb)
    x0 = 0.1 * rng.standard_normal((nb, nx, ny))
    v = rng.standard_normal((nb, nx, ny))
    scratch = ofc.make_scratch(psfhat, Q, x0.shape, np.float64)
    _, _, odf, odhf = osv.setup_parametrisation('exp', sigma=0.8, freq=freq, lscale=0.5)
    _, _, dfunc, dhfunc = setup_parametrisation('exp', sigma=0.8, freq=freq, lscale=0.5)
    ph, x0d, vd = cuda(psfhat.astype(cdt(rdt))), cuda(x0.astype(rdt)), cuda(v.astype(rdt))
    conv = partial(psf_convolve_cube, None, None, None, ph, Q)
    for sigmainv in (0.02, 0.5):
        ref = 2 * odhf(x0, ofc.psf_convolve_cube(*scratch, psfhat, Q, odf(x0, v))) + v * sigmainv
        unfused = 2 * dhfunc(x0d, conv(dfunc(x0d, vd))) + sigmainv * vd
        H = ParamHessian(ph, nx, ny, Q, x0d, sigmainv, dfunc, dhfunc)
        assert H.fused and H.plan.fast_path and H.plan.embed is None
        got = H(vd)
        eu, ef = relerr(unfused.cpu().numpy(), ref), relerr(got.cpu().numpy(), ref)
        print(f'param hessian {np.dtype(rdt).name} sigmainv {sigmainv}: fused {ef:.3e} unfused {eu:.3e}')
        assert ef <= 2 * eu + 16 * EPS[rdt], (sigmainv, ef, eu)


# --------------------------------------------------------------------------------------------- 6. PSFHAT producer
@pmp('rdt', [np.float64, np.float32])
@pmp('shape', [(96, 192), (160, 320)])
def test_plan_from_psf(amd, shape, rdt):
    nx, ny = shape
    nb = 2
    psf, psfhat, x, ref = conv_problem(nb, nx, ny)
    plan, ph = amd.psf.PsfConvPlan.from_psf(cuda(psf.astype(rdt)), nx, ny, want_psfhat=True)
    assert plan.fast_path and plan.embed is None
    perr = np.abs(ph.cpu().numpy().astype(np.complex128) - psfhat).max() / np.abs(psfhat).max()
    assert perr < (1e-12 if rdt == np.float64 else TOL_CONV[rdt])
    y = plan.apply(cuda(x.astype(rdt)))
    assert relerr(y.cpu().numpy(), ref) < TOL_CONV[rdt]
    plan.close()
    # the plan-less entry point takes the same producer for such a grid
    from pfb_clean_amd.operators.fft import psfhat_from_psf
    ph2 = psfhat_from_psf(cuda(psf.astype(rdt)))
    assert torch.equal(ph2, ph)


# ----------------------------------------------------------------------------- 7. embedding into a new class, 8. refusal
@pmp('rdt', [np.float64, np.float32])
@pmp('grid,embed', [((100, 150, 200, 300), (128, 160)), ((250, 300, 400, 600), (256, 320))])
def test_embedded_in_a_mixed_class(amd, grid, embed, rdt, monkeypatch):
    """As test_embedded_plan_conv_and_pcg, on grids whose plan has a 5 2^k axis (the second one with wrap-around:
    nx_psf < 2 nx): convolution, Hessian and 8 PCG iterations against the oracle on the ORIGINAL grid, and the
    convolution against the coverage kernels (PFB_NO_EMBED)."""
    nx, ny, P, Q = grid
    rng = np.random.default_rng(nx + P)
    nb = 2
    W = psd_psfhat(rng, nb, P, Q)
    psfhat = (W * np.exp(2j * np.pi * rng.random(W.shape) * 0.05)).astype(np.complex128)   # not exactly symmetric
    psfhat[:, :, 0] = psfhat[:, :, 0].real
    psfhat[:, :, -1] = psfhat[:, :, -1].real
    psfhat = ofc.psfhat_from_psf(np.fft.fftshift(np.fft.irfft2(psfhat, s=(P, Q)), axes=(1, 2)))   # a valid real PSF
    x = rng.standard_normal((nb, nx, ny))
    beam = 0.5 + rng.random((nb, nx, ny))
    xpad, xhat, xout = ofc.make_scratch(psfhat, Q, x.shape, np.float64)
    ref_c = ofc.psf_convolve_cube(xpad, xhat, xout, psfhat, Q, x).copy()
    ref_h = ofc.hessian_psf_cube(xpad, xhat, xout, beam, psfhat, Q, x, sigmainv=0.3, wsum=1.7)
    cd, tol = cdt(rdt), TOL_CONV[rdt]
    plan = amd.psf.plan_for(psfhat.astype(cd), nx, ny, Q)
    assert plan.embed == embed and plan.fast_path
    got_c = amd.psf.psf_convolve_cube(None, None, None, psfhat.astype(cd), Q, x.astype(rdt))
    got_h = amd.hessian.hessian_psf_cube(None, None, None, beam.astype(rdt), psfhat.astype(cd), Q, x.astype(rdt),
                                         sigmainv=0.3, wsum=1.7)
    assert relerr(got_c, ref_c) < tol and relerr(got_h, ref_h) < tol
    sig = 0.05
    b = ref_c + 0.01 * rng.standard_normal(x.shape)
    xo = osv.pcg(lambda t: ofc.hessian_psf_cube(xpad, xhat, xout, beam, psfhat, Q, t, sigmainv=sig), b, None,
                 M=lambda t: t / sig, tol=0.0, maxit=8, minit=8)
    A = partial(amd.hessian.hessian_psf_cube, None, None, None, beam.astype(rdt), psfhat.astype(cd), Q, sigmainv=sig)
    xg = amd.pcg.pcg(A, b.astype(rdt), None, M=amd.pcg.DivPrecond(sig), tol=0.0, maxit=8, minit=8, verbosity=0)
    assert relerr(xg, xo) < TOL_PCG[rdt]
    monkeypatch.setenv('PFB_NO_EMBED', '1')
    amd.psf.clear_plan_cache()
    gen_c = amd.psf.psf_convolve_cube(None, None, None, psfhat.astype(cd), Q, x.astype(rdt))
    assert amd.psf.plan_for(psfhat.astype(cd), nx, ny, Q).embed is None
    monkeypatch.delenv('PFB_NO_EMBED')
    amd.psf.clear_plan_cache()
    assert relerr(gen_c, got_c) < tol


@pmp('rdt', [np.float64, np.float32])
def test_80_columns_are_embedded(amd, rdt, monkeypatch):
    """nx = 80 is no column class (the 32-row tiles of the shortest rows do not divide it): the library does not take it
    natively, the chooser embeds it in (96, 160), and the result is right."""
    nb, nx, ny = 2, 80, 160
    psf, psfhat, x, ref = conv_problem(nb, nx, ny)
    ph = psfhat.astype(cdt(rdt))
    plan = amd.psf.plan_for(ph, nx, ny, 2 * ny)
    assert plan.embed == (96, 160) and plan.fast_path
    y = amd.psf.psf_convolve_cube(None, None, None, ph, 2 * ny, x.astype(rdt))
    assert relerr(y, ref) < TOL_CONV[rdt]
    # the library itself: asked for (80, 160) directly it does not put it on the fast kernels
    monkeypatch.setenv('PFB_NO_EMBED', '1')
    direct = amd.psf.PsfConvPlan(cuda(ph), nx, ny, 2 * ny)
    assert direct.embed is None and not direct.fast_path
    assert relerr(direct.apply(cuda(x.astype(rdt))).cpu().numpy(), ref) < TOL_CONV[rdt]
    direct.close()


# ------------------------------------------------------------------------------------- 9. the chooser as shipped
@pmp('rdt', [np.float64, np.float32])
def test_default_unoffered_class_is_embedded_in_a_power_of_two(amd, rdt):
    """A 96 x 192 image is a class of its own, but not an offered one (not timed against the power-of-two grid): the
    shipped chooser embeds it in 128 x 256 as before; asked directly (PFB_NO_EMBED) the library runs it natively."""
    nb, nx, ny = 2, 96, 192
    psf, psfhat, x, ref = conv_problem(nb, nx, ny)
    ph = psfhat.astype(cdt(rdt))
    plan = amd.psf.plan_for(ph, nx, ny, 2 * ny)
    assert plan.embed == (128, 256) and plan.fast_path
    assert relerr(amd.psf.psf_convolve_cube(None, None, None, ph, 2 * ny, x.astype(rdt)), ref) < TOL_CONV[rdt]


def test_default_offered_class_runs_natively(amd):
    """fp32 rows of 5120 pixels are offered: a 64 x 5120 image has a plan of its own size, in fp64 (not timed) it is
    embedded; a 5120 x 128 image (no column length is offered) is embedded in 8192 x 128."""
    for rdt, embed in ((np.float32, None), (np.float64, (64, 8192))):
        psf, psfhat, x, ref = conv_problem(1, 64, 5120)
        ph = psfhat.astype(cdt(rdt))
        plan = amd.psf.plan_for(ph, 64, 5120, 10240)
        assert plan.embed == embed and plan.fast_path
        assert relerr(amd.psf.psf_convolve_cube(None, None, None, ph, 10240, x.astype(rdt)), ref) < TOL_CONV[rdt]
    psf, psfhat, x, ref = conv_problem(1, 5120, 128)
    assert amd.psf.plan_for(psfhat.astype(np.complex64), 5120, 128, 256).embed == (8192, 128)
