"""
GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the
C-ABI library via the reference-shaped Python entry points, against

  * the golden vectors the reference's own source produced (tests/golden/*.npz), and
  * the CPU oracle (oracle/) on seeded inputs.

Tolerances: fp64 conv 1e-12, fp64 PCG iterate 1e-9; fp32 conv 1e-5,
fp32 PCG iterate 1e-3 -- all relative to max|reference|.
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


@pytest.fixture(scope='module')
def amd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from pfb_clean_amd.operators import psf, hessian
    from pfb_clean_amd.opt import pcg as pcgmod, power_method as pmmod
    from pfb_clean_amd.utils import misc

    class NS:
        pass
    ns = NS()
    ns.psf, ns.hessian, ns.pcg, ns.pm, ns.misc = psf, hessian, pcgmod, pmmod, misc
    return ns


def relerr(a, ref):
    a = np.asarray(a, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300)


def cdt(rdt):
    return np.complex64 if rdt == np.float32 else np.complex128


# ----------------------------------------------------------------------- conv
@pmp('rdt', [np.float64, np.float32])
@pmp('c', range(6))
def test_conv_and_hessian_golden(amd, golden, c, rdt):
    g = golden('conv')
    nx, ny, P, Q = (int(v) for v in g['cases'][c])
    psfhat = g[f'c{c}_psfhat'].astype(cdt(rdt))
    x = g[f'c{c}_x'].astype(rdt)
    beam = g[f'c{c}_beam'].astype(rdt)
    tol = TOL_CONV[rdt]
    xout = np.empty((nx, ny), dtype=rdt)
    y = amd.psf.psf_convolve_slice(None, None, xout, psfhat[0], Q, x[0])
    assert y is xout                                   # psf.py:29 aliasing contract
    assert relerr(y, g[f'c{c}_slice']) < tol
    xoutc = np.empty(x.shape, dtype=rdt)
    yc = amd.psf.psf_convolve_cube(None, None, xoutc, psfhat, Q, x)
    assert yc is xoutc
    assert relerr(yc, g[f'c{c}_cube']) < tol
    h = amd.hessian._hessian_psf_slice(None, None, None, psfhat[1], beam[1], Q, x[1],
                                       sigmainv=0.37, wsum=2.5)
    assert relerr(h, g[f'c{c}_h_slice_full']) < tol
    h = amd.hessian._hessian_psf_slice(None, None, None, psfhat[1], None, Q, x[1], sigmainv=0.0)
    assert relerr(h, g[f'c{c}_h_slice_bare']) < tol
    h = amd.hessian.hessian_psf_cube(None, None, None, beam, psfhat, Q, x, sigmainv=1.25, wsum=3.0)
    assert relerr(h, g[f'c{c}_h_cube_full']) < tol
    h = amd.hessian.hessian_psf_cube(None, None, None, None, psfhat, Q, x, sigmainv=0.5)
    assert relerr(h, g[f'c{c}_h_cube_bare']) < tol
    assert h.dtype == rdt


SIZES = [  # nx, ny, nx_psf, ny_psf : pow2 2x (fast path), mixed radix, aliasing, ragged
    (64, 64, 128, 128), (128, 32, 256, 64), (256, 512, 512, 1024), (30, 50, 60, 100),
    (45, 33, 90, 66), (50, 21, 70, 44), (100, 128, 200, 256), (33, 17, 64, 32),
    (64, 64, 96, 80), (7, 5, 14, 10), (1, 1, 2, 2), (250, 78, 500, 156), (63, 64, 128, 128),
    # power-of-two with 2x oversampling: the register-resident fast path
    (64, 128, 128, 256), (128, 256, 256, 512), (512, 128, 1024, 256), (1024, 1024, 2048, 2048),
    (2048, 256, 4096, 512), (256, 4096, 512, 8192), (4096, 128, 8192, 256),
    # the largest instantiations (BASELINE config #5 is 8192 x 8192)
    (8192, 128, 16384, 256), (64, 8192, 128, 16384), (128, 2048, 256, 4096), (64, 16384, 128, 32768),
    # PSF lines beyond the LDS (nx_psf > 10240 fp32 / 5120 fp64; grid.py:276-285 good_size grids of 6000^2, 7200^2 ...
    # images): embedded in the power-of-two fast path, the re-gridding runs its long lines as global-memory passes
    (6000, 96, 12000, 192), (7200, 64, 14400, 128), (5040, 64, 10080, 128), (3000, 64, 6000, 128),
    (8000, 64, 16000, 128), (6000, 96, 9000, 144), (96, 7200, 192, 14400),
    # beyond the fast path as well (nx > 8192; fp64 rows of more than 8192 pixels): the long-line coverage path,
    # every transform as global-memory passes
    (9000, 32, 18000, 64), (10000, 48, 12000, 96), (64, 10000, 128, 20000),
]


@pmp('rdt', [np.float64, np.float32])
@pmp('size', SIZES)
def test_conv_vs_oracle_sizes(amd, size, rdt):
    nx, ny, P, Q = size
    rng = np.random.default_rng(nx * 1000 + ny)
    nb = 2
    psf = rng.standard_normal((nb, P, Q))
    psf[:, P // 2, Q // 2] += 5
    psfhat = ofc.psfhat_from_psf(psf)
    x = rng.standard_normal((nb, nx, ny))
    xpad, xhat, xout = ofc.make_scratch(psfhat, Q, x.shape, np.float64)
    ref = ofc.psf_convolve_cube(xpad, xhat, xout, psfhat, Q, x).copy()
    y = amd.psf.psf_convolve_cube(None, None, None, psfhat.astype(cdt(rdt)), Q, x.astype(rdt))
    assert relerr(y, ref) < TOL_CONV[rdt]


@pmp('shape', [(3, 64, 32), (3, 256, 512)])      # generic path, fast path
def test_conv_tensor_path_and_fused_dot(amd, shape):
    """GPU-resident call: xout written in place, x untouched, fused <dot_with, out>."""
    rng = np.random.default_rng(7)
    nb, nx, ny = shape
    P, Q = 2 * nx, 2 * ny
    psfhat = ofc.psfhat_from_psf(rng.standard_normal((nb, P, Q)))
    x = rng.standard_normal((nb, nx, ny))
    beam = 0.5 + rng.random((nb, nx, ny))
    xpad, xhat, xout = ofc.make_scratch(psfhat, Q, x.shape, np.float64)
    ref = ofc.hessian_psf_cube(xpad, xhat, xout, beam, psfhat, Q, x, sigmainv=0.3, wsum=1.7)
    dev = torch.device('cuda')
    xt = torch.from_numpy(x).to(dev)
    x_keep = xt.clone()
    plan = amd.psf.PsfConvPlan(torch.from_numpy(psfhat).to(dev), nx, ny, Q)
    out = torch.empty_like(xt)
    dot = torch.zeros(1, dtype=torch.float64, device=dev)
    w = torch.from_numpy(rng.standard_normal(x.shape)).to(dev)
    res = plan.apply(xt, out=out, beam=torch.from_numpy(beam).to(dev), wsum=1.7, sigmainv=0.3,
                     dot_with=w, dot_out=dot)
    assert res.data_ptr() == out.data_ptr()
    assert torch.equal(xt, x_keep)
    assert plan.fast_path == (nx >= 64 and ny >= 128) and plan.embed is None
    assert relerr(out.cpu().numpy(), ref) < 1e-12
    assert abs(dot.item() - np.vdot(w.cpu().numpy(), ref)) < 1e-9 * abs(np.vdot(w.cpu().numpy(), ref))
    # sub-range of bands on a multi-band plan
    out1 = plan.apply(xt[1:2], band0=1)
    xpad, xhat, xout = ofc.make_scratch(psfhat[1], Q, (nx, ny), np.float64)
    ref1 = ofc.psf_convolve_slice(xpad, xhat, xout, psfhat[1], Q, x[1])
    assert relerr(out1[0].cpu().numpy(), ref1) < 1e-12


@pmp('with_beam', [False, True])
@pmp('ny', [4096, 2048])
@pmp('mode', [0, 1, 2])
def test_persistent_row_kernels_multi_tile(amd, mode, ny, with_beam):
    """ny = 4096 / 2048 fp32 take the persistent pipelined row kernels (k_row_fwd_pow2q for ny = 4096,
    k_row_inv_pow2p for both; with and without a beam); with 3 bands every workgroup walks several row
    tiles and crosses band boundaries.  mode 0: no inner products, 1: <x, out>, <out, out>, 2: + <w, out>
    (pfb_psfconv_apply_dots, the call the fused PCG makes)."""
    from pfb_clean_amd import _lib, _dev
    rng = np.random.default_rng(21)
    nb, nx = 3, (1024 if ny == 4096 else 4096)      # 768 / 1536 row tiles on 256 workgroups
    P, Q = 2 * nx, 2 * ny
    psfhat = ofc.psfhat_from_psf(rng.standard_normal((nb, P, Q)))
    x = rng.standard_normal((nb, nx, ny)).astype(np.float32)
    w = rng.standard_normal((nb, nx, ny)).astype(np.float32)
    beam = (0.5 + rng.random((nb, nx, ny))).astype(np.float32) if with_beam else None
    xpad, xhat, xout = ofc.make_scratch(psfhat, Q, x.shape, np.float64)
    ref = ofc.hessian_psf_cube(xpad, xhat, xout, None if beam is None else beam.astype(np.float64), psfhat, Q,
                               x.astype(np.float64), sigmainv=0.3, wsum=1.7)
    dev = torch.device('cuda')
    plan = amd.psf.PsfConvPlan(torch.from_numpy(psfhat.astype(np.complex64)).to(dev), nx, ny, Q)
    xt, wt = torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev)
    bt = None if beam is None else torch.from_numpy(beam).to(dev)
    out = torch.empty_like(xt)
    dots = torch.zeros(3, dtype=torch.float64, device=dev)
    lib = _lib.load()
    if mode == 0:
        plan.apply(xt, out=out, beam=bt, wsum=1.7, sigmainv=0.3)
    else:
        _lib.check(lib.pfb_psfconv_apply_dots(plan._h, 0, nb, _dev.ptr(xt), _dev.ptr(bt), 1.7, 0.3, _dev.ptr(out),
                                              _dev.ptr(xt), _dev.ptr(wt) if mode == 2 else None,
                                              _dev.ptr(dots), _dev.stream()))
    o = out.cpu().numpy().astype(np.float64)
    assert relerr(o, ref) < TOL_CONV[np.float32]
    if mode:
        d = dots.cpu().numpy()
        assert abs(d[0] - np.vdot(x.astype(np.float64), o)) < 1e-9 * np.vdot(o, o) ** 0.5 * np.linalg.norm(x)
        assert abs(d[2] - np.vdot(o, o)) < 1e-9 * np.vdot(o, o)
        if mode == 2:
            assert abs(d[1] - np.vdot(w.astype(np.float64), o)) < 1e-9 * np.vdot(o, o) ** 0.5 * np.linalg.norm(w)


@pmp('with_beam', [False, True])
@pmp('rdt', [np.float32, np.float64])
@pmp('mode', [0, 2])
def test_persistent_row_kernels_8192_pixel_rows(amd, mode, rdt, with_beam):
    """ny = 8192 (4096-point rows, round 3): fp32 takes the 4-row small-table tiles of k_row_fwd_pow2q / k_row_inv_pow2p
    (16 elements per thread, operands read in place, two-loop epilogue -- also for the beam + two-dots call of the PCG on
    embedded plans), fp64 the plain forward kernel and the 2-row 512-thread inverse tile with its own pass table; 512
    rows x 2 bands = several tiles per workgroup across a band boundary.  Against the oracle."""
    from pfb_clean_amd import _lib, _dev
    rng = np.random.default_rng(33)
    nb, nx, ny = 2, 512, 8192
    P, Q = 2 * nx, 2 * ny
    psfhat = ofc.psfhat_from_psf(rng.standard_normal((nb, P, Q)))
    x = rng.standard_normal((nb, nx, ny)).astype(rdt)
    w = rng.standard_normal((nb, nx, ny)).astype(rdt)
    beam = (0.5 + rng.random((nb, nx, ny))).astype(rdt) if with_beam else None
    xpad, xhat, xout = ofc.make_scratch(psfhat, Q, x.shape, np.float64)
    ref = ofc.hessian_psf_cube(xpad, xhat, xout, None if beam is None else beam.astype(np.float64), psfhat, Q,
                               x.astype(np.float64), sigmainv=0.3, wsum=1.7)
    dev = torch.device('cuda')
    plan = amd.psf.PsfConvPlan(torch.from_numpy(psfhat.astype(cdt(rdt))).to(dev), nx, ny, Q)
    assert plan.fast_path
    xt, wt = torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev)
    bt = None if beam is None else torch.from_numpy(beam).to(dev)
    out = torch.empty_like(xt)
    dots = torch.zeros(3, dtype=torch.float64, device=dev)
    lib = _lib.load()
    if mode == 0:
        plan.apply(xt, out=out, beam=bt, wsum=1.7, sigmainv=0.3)
    else:
        _lib.check(lib.pfb_psfconv_apply_dots(plan._h, 0, nb, _dev.ptr(xt), _dev.ptr(bt), 1.7, 0.3, _dev.ptr(out),
                                              _dev.ptr(xt), _dev.ptr(wt), _dev.ptr(dots), _dev.stream()))
    o = out.cpu().numpy().astype(np.float64)
    assert relerr(o, ref) < TOL_CONV[rdt]
    if mode:
        d = dots.cpu().numpy()
        tol = 1e-9 if rdt == np.float32 else 1e-12
        assert abs(d[0] - np.vdot(x.astype(np.float64), o)) < tol * np.linalg.norm(o) * np.linalg.norm(x)
        assert abs(d[1] - np.vdot(w.astype(np.float64), o)) < tol * np.linalg.norm(o) * np.linalg.norm(w)
        assert abs(d[2] - np.vdot(o, o)) < tol * np.vdot(o, o)
    plan.close()


@pmp('with_beam', [False, True])
def test_persistent_row_inverse_fp64_multi_tile(amd, with_beam):
    """fp64 at ny = 4096: two-row tiles, 512-thread workgroups, even-bin result kept in registers,
    32-byte pieces XCD-grouped four to a line (k_row_inv_pow2p<double>); 8 tiles per workgroup, all
    three inner products."""
    from pfb_clean_amd import _lib, _dev
    rng = np.random.default_rng(5)
    nb, nx, ny = 2, 2048, 4096
    P, Q = 2 * nx, 2 * ny
    psfhat = ofc.psfhat_from_psf(rng.standard_normal((nb, P, Q)))
    x = rng.standard_normal((nb, nx, ny))
    w = rng.standard_normal((nb, nx, ny))
    beam = 0.5 + rng.random((nb, nx, ny)) if with_beam else None
    xpad, xhat, xout = ofc.make_scratch(psfhat, Q, x.shape, np.float64)
    ref = ofc.hessian_psf_cube(xpad, xhat, xout, beam, psfhat, Q, x, sigmainv=0.3, wsum=1.7)
    dev = torch.device('cuda')
    plan = amd.psf.PsfConvPlan(torch.from_numpy(psfhat).to(dev), nx, ny, Q)
    xt, wt = torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev)
    bt = None if beam is None else torch.from_numpy(beam).to(dev)
    out = torch.empty_like(xt)
    dots = torch.zeros(3, dtype=torch.float64, device=dev)
    lib = _lib.load()
    _lib.check(lib.pfb_psfconv_apply_dots(plan._h, 0, nb, _dev.ptr(xt), _dev.ptr(bt), 1.7, 0.3, _dev.ptr(out),
                                          _dev.ptr(xt), _dev.ptr(wt), _dev.ptr(dots), _dev.stream()))
    o = out.cpu().numpy()
    assert relerr(o, ref) < 1e-12
    d = dots.cpu().numpy()
    assert abs(d[0] - np.vdot(x, o)) < 1e-12 * np.linalg.norm(x) * np.linalg.norm(o)
    assert abs(d[1] - np.vdot(w, o)) < 1e-12 * np.linalg.norm(w) * np.linalg.norm(o)
    assert abs(d[2] - np.vdot(o, o)) < 1e-12 * np.vdot(o, o)


@pmp('rdt', [np.float64, np.float32])
def test_fast_path_equals_generic_path(amd, rdt, monkeypatch):
    """Same plan sizes through both kernel families (PFB_FORCE_GENERIC picks the coverage
    kernels): they must agree to rounding, band by band, with beam / wsum / sigmainv."""
    rng = np.random.default_rng(11)
    nb, nx, ny = 2, 512, 256
    P, Q = 2 * nx, 2 * ny
    psfhat = ofc.psfhat_from_psf(rng.standard_normal((nb, P, Q))).astype(cdt(rdt))
    x = rng.standard_normal((nb, nx, ny)).astype(rdt)
    beam = (0.5 + rng.random((nb, nx, ny))).astype(rdt)
    amd.psf.clear_plan_cache()
    fast = amd.hessian.hessian_psf_cube(None, None, None, beam, psfhat, Q, x, sigmainv=0.2, wsum=1.3)
    monkeypatch.setenv('PFB_FORCE_GENERIC', '1')
    amd.psf.clear_plan_cache()
    gen = amd.hessian.hessian_psf_cube(None, None, None, beam, psfhat, Q, x, sigmainv=0.2, wsum=1.3)
    monkeypatch.delenv('PFB_FORCE_GENERIC')
    amd.psf.clear_plan_cache()
    assert relerr(fast, gen) < (1e-13 if rdt == np.float64 else 2e-6)


def test_conv_errors(amd):
    from pfb_clean_amd._lib import PfbHipError
    rng = np.random.default_rng(0)
    with pytest.raises(PfbHipError):           # odd lastsize is outside the supported set
        amd.psf.PsfConvPlan(rng.standard_normal((1, 16, 6)).astype(np.complex128), 8, 4, 10 + 1)
    with pytest.raises(PfbHipError):           # prime factor 17
        amd.psf.PsfConvPlan(np.zeros((1, 34, 9), dtype=np.complex128), 17, 8, 16)
    with pytest.raises(ValueError):
        amd.psf.psf_convolve_cube(None, None, None, np.zeros((2, 16, 9), complex), 16,
                                  np.zeros((3, 8, 8)))
    psfhat = np.zeros((2, 16, 9), dtype=np.complex128)
    with pytest.raises(ValueError, match='Beam has incorrect shape'):
        amd.hessian.hessian_psf_cube(None, None, None, np.zeros((2, 8, 7)), psfhat, 16,
                                     np.zeros((2, 8, 8)))


# -------------------------------------------------------------- vector kernels
@pmp('rdt', [np.float64, np.float32])
@pmp('n', [1, 7, 64, 1000, 4099, 1 << 20, (1 << 20) + 3])
def test_vector_kernels(amd, n, rdt):
    from pfb_clean_amd import _lib, _dev
    lib = _lib.load()
    rng = np.random.default_rng(n)
    a = rng.standard_normal(n).astype(rdt)
    b = rng.standard_normal(n).astype(rdt)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    ws, out = _dev.scratch()
    code = _dev.code(ta.dtype)
    _lib.check(lib.pfb_dot(code, ta.data_ptr(), tb.data_ptr(), n, out.data_ptr(), ws.data_ptr(), _dev.stream()))
    ref = np.dot(a.astype(np.float64), b.astype(np.float64))
    assert abs(out[0].item() - ref) <= 1e-12 * max(1.0, np.abs(a.astype(np.float64) * b).sum())
    _lib.check(lib.pfb_norm_diff_sums(code, ta.data_ptr(), tb.data_ptr(), n, out.data_ptr(), ws.data_ptr(), _dev.stream()))
    num, den = out[:2].tolist()
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    assert abs(num - np.sum((a64 - b64) ** 2)) <= 1e-12 * np.sum((a64 - b64) ** 2) + 1e-300
    assert abs(den - np.sum(a64 ** 2)) <= 1e-12 * np.sum(a64 ** 2)
    _lib.check(lib.pfb_any_nonzero(code, ta.data_ptr(), n, out.data_ptr(), ws.data_ptr(), _dev.stream()))
    assert out[0].item() > 0
    z = torch.zeros_like(ta)
    _lib.check(lib.pfb_any_nonzero(code, z.data_ptr(), n, out.data_ptr(), ws.data_ptr(), _dev.stream()))
    assert out[0].item() == 0
    _lib.check(lib.pfb_axpby(code, 0.5, ta.data_ptr(), -2.0, tb.data_ptr(), n, _dev.stream()))
    np.testing.assert_allclose(tb.cpu().numpy(), rdt(0.5) * a + rdt(-2.0) * b, rtol=1e-6 if rdt == np.float32 else 1e-14)
    # deterministic: same input, bitwise same result
    _lib.check(lib.pfb_dot(code, ta.data_ptr(), ta.data_ptr(), n, out.data_ptr(), ws.data_ptr(), _dev.stream()))
    d1 = out[0].item()
    _lib.check(lib.pfb_dot(code, ta.data_ptr(), ta.data_ptr(), n, out.data_ptr(), ws.data_ptr(), _dev.stream()))
    assert out[0].item() == d1
    # each operand in turn one element off the 16-byte boundary (fp32 also two: 8-byte aligned): the V = 1 kernels,
    # the same tolerances; axpby's y lies between sentinels that must survive
    SENT, PAD = -1234.5, 64

    def off16(arr, k):
        full = torch.full((PAD + k + n + PAD,), SENT, dtype=ta.dtype, device='cuda')
        full[PAD + k:PAD + k + n] = torch.from_numpy(arr).cuda()
        view = full[PAD + k:PAD + k + n]
        assert (view.data_ptr() % 16 == 0) == (k * arr.itemsize % 16 == 0)
        return full, view
    for k in ((1, 2) if rdt == np.float32 else (1,)):
        for ka, kb in ((k, 0), (0, k), (k, k)):
            (fa, va), (fb, vb) = off16(a, ka), off16(b, kb)
            _lib.check(lib.pfb_dot(code, va.data_ptr(), vb.data_ptr(), n, out.data_ptr(), ws.data_ptr(), _dev.stream()))
            assert abs(out[0].item() - ref) <= 1e-12 * max(1.0, np.abs(a64 * b).sum())
            _lib.check(lib.pfb_norm_diff_sums(code, va.data_ptr(), vb.data_ptr(), n, out.data_ptr(), ws.data_ptr(),
                                              _dev.stream()))
            num, den = out[:2].tolist()
            assert abs(num - np.sum((a64 - b64) ** 2)) <= 1e-12 * np.sum((a64 - b64) ** 2) + 1e-300
            assert abs(den - np.sum(a64 ** 2)) <= 1e-12 * np.sum(a64 ** 2)
            _lib.check(lib.pfb_axpby(code, 0.5, va.data_ptr(), -2.0, vb.data_ptr(), n, _dev.stream()))
            np.testing.assert_allclose(vb.cpu().numpy(), rdt(0.5) * a + rdt(-2.0) * b,
                                       rtol=1e-6 if rdt == np.float32 else 1e-14)
            assert torch.equal(va, ta)
            for f, kk in ((fa, ka), (fb, kb)):
                assert bool((f[:PAD + kk] == SENT).all()) and bool((f[PAD + kk + n:] == SENT).all())
        fz, vz = off16(np.zeros(n, rdt), k)
        _lib.check(lib.pfb_any_nonzero(code, vz.data_ptr(), n, out.data_ptr(), ws.data_ptr(), _dev.stream()))
        assert out[0].item() == 0
        vz[n - 1] = 1e-30
        _lib.check(lib.pfb_any_nonzero(code, vz.data_ptr(), n, out.data_ptr(), ws.data_ptr(), _dev.stream()))
        assert out[0].item() > 0
    if n in (4099, (1 << 20) + 3):          # a single non-zero element, the last one, behind the last full pack
        z[n - 1] = -1e-30
        _lib.check(lib.pfb_any_nonzero(code, z.data_ptr(), n, out.data_ptr(), ws.data_ptr(), _dev.stream()))
        assert out[0].item() > 0


def test_norm_diff_api(amd):
    rng = np.random.default_rng(3)
    x, xp = rng.standard_normal((2, 40, 50)), rng.standard_normal((2, 40, 50))
    assert abs(amd.misc.norm_diff(x, xp) - osv.norm_diff(x, xp)) < 1e-14
    assert abs(amd.misc.norm_diff(torch.from_numpy(x[0]).cuda(), torch.from_numpy(xp[0]).cuda())
               - osv.norm_diff(x[0], xp[0])) < 1e-14
    with pytest.raises(ValueError):
        amd.misc.norm_diff(x[0, 0], xp[0, 0])


# ------------------------------------------------------------------------ pcg
@pmp('rdt', [np.float64, np.float32])
def test_pcg_psf_band_history_golden(amd, golden, rdt):
    g = golden('pcg')
    psfhat, b, beam = g['psfhat'].astype(cdt(rdt)), g['b'].astype(rdt), g['beam'].astype(rdt)
    sigmainv, Q = float(g['sigmainv']), int(g['Q'])
    tol = TOL_PCG[rdt]
    for tag, bm in (('nobeam', None), ('beam', beam)):
        for k in (1, 2, 5, 20):
            for bt in (True, False):
                m = amd.pcg.pcg_psf(psfhat, b, np.zeros_like(b), bm, Q, 1, sigmainv,
                                    dict(tol=0.0, maxit=k, minit=k, verbosity=0, backtrack=bt))
                assert m.dtype == rdt
                assert relerr(m, g[f'band_{tag}_k{k}_bt{int(bt)}']) < tol, (tag, k, bt)
    if rdt == np.float64:       # exit iteration is tolerance-controlled: fp64 only
        for key, minit in (('band_tol1e-2', 1), ('band_tol1e-2_minit15', 15)):
            m = amd.pcg.pcg_psf(psfhat, b, np.zeros_like(b), None, Q, 1, sigmainv,
                                dict(tol=1e-2, maxit=100, minit=minit, verbosity=0, backtrack=True))
            assert relerr(m, g[key]) < tol


@pmp('rdt', [np.float64, np.float32])
def test_pcg_cube_golden_via_reference_call_pattern(amd, golden, rdt):
    """The exact construction fluxmop.py:160-199 uses -- functools.partial of
    hessian_psf_cube with scratch buffers -- must take the fused path and match."""
    g = golden('pcg')
    psfhat, b, beam = g['psfhat'].astype(cdt(rdt)), g['b'].astype(rdt), g['beam'].astype(rdt)
    sigmainv, Q = float(g['sigmainv']), int(g['Q'])
    tol = TOL_PCG[rdt]
    A = partial(amd.hessian.hessian_psf_cube, None, None, None, beam, psfhat, Q,
                nthreads=1, sigmainv=sigmainv, wsum=1.0)
    assert amd.pcg._as_hessian(A, b) is not None
    for k in (1, 3, 10, 25):
        x, r = amd.pcg.pcg(A, beam * b, np.zeros_like(b), tol=0.0, maxit=k, minit=k,
                           verbosity=0, backtrack=True, return_resid=True)
        assert relerr(x, g[f'cube_k{k}_x']) < tol
        assert relerr(r, g[f'cube_k{k}_r']) < 10 * tol
    x0 = g['cube_x0'].astype(rdt)
    x = amd.pcg.pcg(A, beam * b, x0, M=amd.pcg.DivPrecond(sigmainv), tol=0.0, maxit=7, minit=7,
                    verbosity=0)
    assert relerr(x, g['cube_M_x0_k7']) < tol
    # generic path (opaque callables) agrees with the fused one
    xg = amd.pcg.pcg(lambda v: A(v), beam * b, x0, M=lambda v: v / rdt(sigmainv), tol=0.0,
                     maxit=7, minit=7, verbosity=0)
    assert relerr(xg, g['cube_M_x0_k7']) < tol
    # zero residual: x0 itself comes back (pcg.py:73-75)
    xz = amd.pcg.pcg(A, A(x0), x0, tol=1e-5, maxit=5, minit=1, verbosity=0)
    assert xz is x0


def test_pcg_backtracking_golden(amd, golden):
    g = golden('pcg')
    ph, bb = g['indef_psfhat'], g['indef_b']
    sigmainv, Q = float(g['sigmainv']), int(g['Q'])
    nx, ny = bb.shape
    A = amd.hessian.HessianPsf(ph, nx, ny, Q, sigmainv=sigmainv)
    # True = predictive line search (three fused scalars), 'exact' = the reference loop verbatim
    counts = {}
    for bt in (True, 'exact', False):
        for k in (3, 8):
            x, _, res = amd.pcg.pcg_fused(A, torch.from_numpy(bb).cuda(), None, tol=0.0, maxit=k,
                                          minit=k, backtrack=bt)
            assert relerr(x.cpu().numpy(), g[f'indef_k{k}_bt{int(bool(bt))}']) < 1e-8, (bt, k)
            assert res.iters == k and res.matvecs == k + 1
            counts[(bt, k)] = res.backtracks
    assert counts[(True, 8)] > 0 and counts[(True, 8)] == counts[('exact', 8)]
    assert counts[(False, 8)] == 0


@pmp('mode', [True, 'exact', False])
def test_pcg_breakdown_all_zero_direction(amd, mode):
    """pcg.py:106-107: `if not np.any(p): break` BEFORE k += 1.  A = identity (psfhat = 0,
    sigmainv = 1) converges exactly in one step: r' = 0, p = 0.  The sync-free driver notices
    one iteration late on the device and must still report k = 0 and x = b."""
    rng = np.random.default_rng(5)
    nx, ny = 64, 128
    b = rng.standard_normal((1, nx, ny))
    psfhat = np.zeros((1, 2 * nx, ny + 1), dtype=np.complex128)
    A = amd.hessian.HessianPsf(psfhat, nx, ny, 2 * ny, sigmainv=1.0)
    x, r, res = amd.pcg.pcg_fused(A, torch.from_numpy(b).cuda(), None, tol=1e-8, maxit=10, minit=5,
                                  backtrack=mode, return_resid=True)
    assert res.status == 3 and res.iters == 0 and res.matvecs == 2
    assert np.array_equal(x.cpu().numpy(), b)
    assert not r.cpu().numpy().any()
    ref = osv.pcg(lambda v: v.copy(), b, None, tol=1e-8, maxit=10, minit=5, backtrack=bool(mode))
    assert np.array_equal(ref, b)


def test_pcg_tensor_inputs_stay_on_device(amd, golden):
    g = golden('pcg')
    psfhat, b = torch.from_numpy(g['psfhat']).cuda(), torch.from_numpy(g['b']).cuda()
    sigmainv, Q = float(g['sigmainv']), int(g['Q'])
    nb, nx, ny = b.shape
    A = amd.hessian.HessianPsf(psfhat, nx, ny, Q, sigmainv=sigmainv, wsum=1.0)
    x = amd.pcg.pcg(A, b, None, tol=0.0, maxit=5, minit=5, verbosity=0)
    assert isinstance(x, torch.Tensor) and x.is_cuda
    xpad, xhat, xout = ofc.make_scratch(g['psfhat'], Q, g['b'].shape, np.float64)
    ref = osv.pcg(lambda v: ofc.hessian_psf_cube(xpad, xhat, xout, None, g['psfhat'], Q, v,
                                                 sigmainv=sigmainv, wsum=1.0),
                  g['b'], None, tol=0.0, maxit=5, minit=5)
    assert relerr(x.cpu().numpy(), ref) < 1e-9


def test_power_method_golden(amd, golden):
    g = golden('pcg')
    psfhat, Q, b0 = g['psfhat'], int(g['Q']), g['pm_b0']
    conv = partial(amd.psf.psf_convolve_cube, None, None, None, psfhat, Q)
    beta, bvec = amd.pm.power_method(conv, b0.shape, b0=b0.copy(), tol=1e-3, maxit=40, verbosity=0)
    assert abs(beta - float(g['pm_beta'])) < 1e-10 * abs(float(g['pm_beta']))
    assert relerr(bvec, g['pm_b']) < 1e-9
    # device-resident form
    convt = partial(amd.psf.psf_convolve_cube, None, None, None, torch.from_numpy(psfhat).cuda(), Q)
    beta2, b2 = amd.pm.power_method(convt, b0.shape, b0=torch.from_numpy(b0).cuda(), tol=1e-3,
                                    maxit=40, verbosity=0)
    assert abs(beta2 - beta) < 1e-12 * abs(beta) and b2.is_cuda


def test_plan_cache_survives_address_reuse(amd):
    """Two different psfhat TENSORS that end up at the same device address (the first one freed
    before the second is created) must not share a cached plan."""
    rng = np.random.default_rng(33)
    nx = ny = 64
    P = Q = 128
    dev = torch.device('cuda')
    x = rng.standard_normal((1, nx, ny))
    xt = torch.from_numpy(x).to(dev)
    amd.psf.clear_plan_cache()
    outs, refs, ptrs = [], [], []
    for k in range(3):
        psfhat = ofc.psfhat_from_psf(rng.standard_normal((1, P, Q)))
        t = torch.from_numpy(psfhat).to(dev)
        ptrs.append(t.data_ptr())
        outs.append(amd.psf.psf_convolve_cube(None, None, None, t, Q, xt).clone())
        del t
        xpad, xhat, xout = ofc.make_scratch(psfhat, Q, x.shape, np.float64)
        refs.append(ofc.psf_convolve_cube(xpad, xhat, xout, psfhat, Q, x).copy())
    for o, r in zip(outs, refs):
        assert relerr(o.cpu().numpy(), r) < 1e-12


@pmp('rdt', [np.float64, np.float32])
@pmp('grid', [(100, 120, 200, 240), (100, 120, 150, 180), (250, 78, 500, 156)])
def test_embedded_plan_conv_and_pcg(amd, grid, rdt, monkeypatch):
    """Arbitrary sizes ride the power-of-two kernels through a re-gridded PSF (pfb_psfhat_regrid)
    and zero-padded images, incl. PSF grids with wrap-around (nx_psf < 2 nx).  The convolution,
    the Hessian with a beam and the fused PCG must match the oracle on the ORIGINAL grid, and the
    coverage kernels (PFB_NO_EMBED) on the same inputs."""
    nx, ny, P, Q = grid
    rng = np.random.default_rng(nx + P)
    nb = 2
    u = np.fft.fftfreq(P)[:, None]
    v = np.fft.rfftfreq(Q)[None, :]
    W = rng.poisson(4 * np.exp(-(u ** 2 + v ** 2) / (2 * 0.12 ** 2)), size=(nb, P, Q // 2 + 1)).astype(np.float64)
    W /= nb * np.fft.irfft2(W, s=(P, Q)).max(axis=(1, 2))[:, None, None]
    psfhat = (W * np.exp(2j * np.pi * rng.random(W.shape) * 0.05)).astype(np.complex128)   # not exactly symmetric
    psfhat[:, :, 0] = psfhat[:, :, 0].real
    psfhat[:, :, -1] = psfhat[:, :, -1].real
    psfhat = ofc.psfhat_from_psf(np.fft.fftshift(np.fft.irfft2(psfhat, s=(P, Q)), axes=(1, 2)))   # a valid real PSF
    x = rng.standard_normal((nb, nx, ny))
    beam = 0.5 + rng.random((nb, nx, ny))
    xpad, xhat, xout = ofc.make_scratch(psfhat, Q, x.shape, np.float64)
    ref_c = ofc.psf_convolve_cube(xpad, xhat, xout, psfhat, Q, x).copy()
    ref_h = ofc.hessian_psf_cube(xpad, xhat, xout, beam, psfhat, Q, x, sigmainv=0.3, wsum=1.7)
    cd = cdt(rdt)
    tol = TOL_CONV[rdt]
    amd.psf.clear_plan_cache()
    plan = amd.psf.plan_for(psfhat.astype(cd), nx, ny, Q)
    assert plan.embed == (max(64, 1 << (nx - 1).bit_length()), max(128, 1 << (ny - 1).bit_length())) and plan.fast_path
    got_c = amd.psf.psf_convolve_cube(None, None, None, psfhat.astype(cd), Q, x.astype(rdt))
    got_h = amd.hessian.hessian_psf_cube(None, None, None, beam.astype(rdt), psfhat.astype(cd), Q, x.astype(rdt),
                                         sigmainv=0.3, wsum=1.7)
    assert relerr(got_c, ref_c) < tol and relerr(got_h, ref_h) < tol
    # fused PCG on the embedded plan == oracle PCG on the original grid
    sig = 0.05
    b = ref_c + 0.01 * rng.standard_normal(x.shape)

    def oA(t):
        return ofc.hessian_psf_cube(xpad, xhat, xout, beam, psfhat, Q, t, sigmainv=sig)
    xo = osv.pcg(oA, b, None, M=lambda t: t / sig, tol=0.0, maxit=8, minit=8)
    A = partial(amd.hessian.hessian_psf_cube, None, None, None, beam.astype(rdt), psfhat.astype(cd), Q, sigmainv=sig)
    xg = amd.pcg.pcg(A, b.astype(rdt), None, M=amd.pcg.DivPrecond(sig), tol=0.0, maxit=8, minit=8, verbosity=0)
    assert relerr(xg, xo) < (1e-9 if rdt == np.float64 else 2e-3)
    # and the coverage kernels agree
    monkeypatch.setenv('PFB_NO_EMBED', '1')
    amd.psf.clear_plan_cache()
    gen_c = amd.psf.psf_convolve_cube(None, None, None, psfhat.astype(cd), Q, x.astype(rdt))
    assert amd.psf.plan_for(psfhat.astype(cd), nx, ny, Q).embed is None
    monkeypatch.delenv('PFB_NO_EMBED')
    amd.psf.clear_plan_cache()
    assert relerr(gen_c, got_c) < tol


def test_per_band_solves_from_concurrent_host_threads(amd, golden):
    """The reference's dask `threads` scheduler runs _pcg_psf for different bands concurrently
    (pcg.py:346-356).  Here: one host thread per band, each with its own per-band plan (what
    functools.partial(_hessian_psf_slice, psfhat[k], ...) gives), all on the same stream -- the
    results must equal the sequential ones bitwise."""
    import threading
    g = golden('pcg')
    psfhat, b, beam = g['psfhat'], g['b'], g['beam']
    sigmainv, Q = float(g['sigmainv']), int(g['Q'])
    nband = b.shape[0]
    dev = torch.device('cuda')
    ops = [amd.hessian.HessianPsf(torch.from_numpy(psfhat[k]).to(dev), b.shape[1], b.shape[2], Q,
                                  beam=torch.from_numpy(beam[k]).to(dev), sigmainv=sigmainv) for k in range(nband)]
    rhs = [torch.from_numpy((beam * b)[k]).to(dev) for k in range(nband)]

    def solve(k):
        return amd.pcg.pcg_fused(ops[k], rhs[k], None, mdiv=sigmainv, tol=0.0, maxit=12, minit=12)[0]
    seq = [solve(k).clone() for k in range(nband)]
    for _ in range(3):
        out = [None] * nband

        def work(k):
            out[k] = solve(k)
        ts = [threading.Thread(target=work, args=(k,)) for k in range(nband)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        for k in range(nband):
            assert torch.equal(out[k], seq[k]), k


def test_closure_preconditioner_is_recognised(amd, golden):
    """fluxmop / _pcg_psf_impl pass `M = lambda x: x / sigmainv` (pcg.py:264-267): it is probed and kept on the
    fused path (same iterates as DivPrecond); a diagonal with varying entries and a nonlinear M are not."""
    from pfb_clean_amd.opt import pcg as P
    g = golden('pcg')
    psfhat, b, beam = g['psfhat'], g['b'], g['beam']
    sigmainv, Q = float(g['sigmainv']), int(g['Q'])
    A = partial(amd.hessian.hessian_psf_cube, None, None, None, beam, psfhat, Q, sigmainv=sigmainv, wsum=1.0)
    rhs = beam * b
    calls = []
    orig = P.pcg_fused

    def spy(*a, **k):
        calls.append(k.get('mdiv'))
        return orig(*a, **k)
    P.pcg_fused = spy
    try:
        x_ref = amd.pcg.pcg(A, rhs, None, M=amd.pcg.DivPrecond(sigmainv), tol=0.0, maxit=9, minit=9, verbosity=0)
        x_lam = amd.pcg.pcg(A, rhs, None, M=lambda v: v / sigmainv, tol=0.0, maxit=9, minit=9, verbosity=0)
        assert len(calls) == 2 and abs(calls[1] - sigmainv) < 1e-12 * sigmainv
        assert relerr(x_lam, x_ref) < 1e-12
        w = 1.0 + np.arange(rhs.size).reshape(rhs.shape) % 3
        amd.pcg.pcg(A, rhs, None, M=lambda v: v / w, tol=0.0, maxit=3, minit=3, verbosity=0)
        amd.pcg.pcg(A, rhs, None, M=lambda v: np.sign(v) * np.abs(v) ** 0.9, tol=0.0, maxit=3, minit=3, verbosity=0)
        assert len(calls) == 2                                  # both went the generic way
    finally:
        P.pcg_fused = orig


@pmp('bt', [True, False])
def test_pcg_one_iteration_lookahead_is_invisible(amd, golden, bt, monkeypatch):
    """Past minit the driver may run one iteration ahead of the host's look at eps (small problems do by
    default): the speculative iteration must be a no-op once the device-side stopping rule has fired, so
    every stop regime -- tolerance, tolerance below minit, maxit, breakdown -- gives bit-identical
    x, r, k, eps with PFB_PCG_LOOKAHEAD=1 and =0, and both agree with the oracle's iteration count."""
    g = golden('pcg')
    psfhat, b = g['psfhat'], g['b']
    sigmainv, Q = float(g['sigmainv']), int(g['Q'])
    nb, nx, ny = b.shape
    A = amd.hessian.HessianPsf(psfhat, nx, ny, Q, sigmainv=sigmainv, wsum=1.0)
    bt_ = torch.from_numpy(b).cuda()
    xpad, xhat, xout = ofc.make_scratch(psfhat, Q, b.shape, np.float64)
    Ao = lambda v: ofc.hessian_psf_cube(xpad, xhat, xout, None, psfhat, Q, v, sigmainv=sigmainv, wsum=1.0)
    cases = [dict(tol=1e-3, maxit=100, minit=1), dict(tol=1e-6, maxit=100, minit=3),
             dict(tol=1e-2, maxit=100, minit=15), dict(tol=1e-12, maxit=9, minit=2),
             dict(tol=0.5, maxit=50, minit=0), dict(tol=1e-4, maxit=4, minit=4)]
    for kw in cases:
        out = {}
        for la in ('1', '0'):
            monkeypatch.setenv('PFB_PCG_LOOKAHEAD', la)
            x, r, res = amd.pcg.pcg_fused(A, bt_, None, mdiv=sigmainv, backtrack=bt, return_resid=True, **kw)
            out[la] = (x.cpu().numpy().copy(), r.cpu().numpy().copy(), res.iters, res.eps, res.status, res.matvecs)
        for a, c in zip(out['1'], out['0']):
            assert np.array_equal(a, c), kw
        tr = osv.PCGTrace()
        xo = osv.pcg(Ao, b, None, M=lambda v: v / sigmainv, backtrack=bt, trace=tr, **kw)
        assert out['1'][2] == tr.k_exit, (kw, out['1'][2], tr.k_exit)
        # the fixture's operator is not positive definite (83 backtracks in 100 iterations): without
        # backtracking the recurrence amplifies rounding differences (1e-5 after 100 iterations)
        assert relerr(out['1'][0], xo) < (1e-9 if bt else 1e-4)
    # breakdown two looks late: identity operator converges exactly in one step
    rng = np.random.default_rng(5)
    b1 = rng.standard_normal((1, 64, 128))
    A1 = amd.hessian.HessianPsf(np.zeros((1, 128, 129), dtype=np.complex128), 64, 128, 256, sigmainv=1.0)
    for la in ('1', '0'):
        monkeypatch.setenv('PFB_PCG_LOOKAHEAD', la)
        x, r, res = amd.pcg.pcg_fused(A1, torch.from_numpy(b1).cuda(), None, tol=1e-8, maxit=10, minit=0,
                                      backtrack=bt, return_resid=True)
        assert res.status == 3 and res.iters == 0 and res.matvecs == 2
        assert np.array_equal(x.cpu().numpy(), b1) and not r.cpu().numpy().any()


def test_pcg_degenerate_iteration_limits(amd, golden):
    """maxit = 0 (the reference's while loop is never entered: x0 comes back, one matvec for the initial
    residual), maxit < minit (maxit wins), minit = 0 with a tolerance met after the first iteration."""
    g = golden('pcg')
    psfhat, b = g['psfhat'], g['b']
    sigmainv, Q = float(g['sigmainv']), int(g['Q'])
    nb, nx, ny = b.shape
    A = amd.hessian.HessianPsf(psfhat, nx, ny, Q, sigmainv=sigmainv, wsum=1.0)
    bt_ = torch.from_numpy(b).cuda()
    x0 = torch.from_numpy(g['cube_x0']).cuda()
    xpad, xhat, xout = ofc.make_scratch(psfhat, Q, b.shape, np.float64)
    Ao = lambda v: ofc.hessian_psf_cube(xpad, xhat, xout, None, psfhat, Q, v, sigmainv=sigmainv, wsum=1.0)
    x, _, res = amd.pcg.pcg_fused(A, bt_, x0, mdiv=sigmainv, tol=1e-3, maxit=0, minit=5)
    assert res.iters == 0 and res.matvecs == 1 and torch.equal(x, x0)
    for kw in (dict(tol=1e-3, maxit=3, minit=10), dict(tol=10.0, maxit=20, minit=0)):
        x, _, res = amd.pcg.pcg_fused(A, bt_, x0, mdiv=sigmainv, **kw)
        tr = osv.PCGTrace()
        xo = osv.pcg(Ao, b, g['cube_x0'].copy(), M=lambda v: v / sigmainv, trace=tr, **kw)
        assert res.iters == tr.k_exit and relerr(x.cpu().numpy(), xo) < 1e-10, kw


def test_one_plan_shared_by_concurrent_host_threads(amd, golden):
    """plan_for() hands the SAME PsfConvPlan to every host thread that presents the same psfhat (what the
    reference's dask threads do with one functools.partial, pcg.py:346-356).  The plan's spectrum workspace
    and dot partials are single-owner (include/pfb_hip.h), so the Python layer serialises on plan.lock:
    convolutions and fused solves on different band ranges from four threads, default stream and private
    streams, must equal the sequential results bitwise."""
    import threading
    g = golden('pcg')
    psfhat, b = g['psfhat'], g['b']
    sigmainv, Q = float(g['sigmainv']), int(g['Q'])
    nband, nx, ny = b.shape
    dev = torch.device('cuda')
    ph = torch.from_numpy(psfhat).to(dev)
    amd.psf.clear_plan_cache()
    plan = amd.psf.plan_for(ph, nx, ny, Q)
    assert amd.psf.plan_for(ph, nx, ny, Q) is plan
    ops = [amd.hessian.HessianPsf(plan, nx, ny, Q, sigmainv=sigmainv, band0=k, nb=1) for k in range(nband)]
    rhs = [torch.from_numpy(b[k:k + 1]).to(dev) for k in range(nband)]
    rng = np.random.default_rng(5)
    xs = [torch.from_numpy(rng.standard_normal((1, nx, ny))).to(dev) for _ in range(nband)]

    def job(k):
        y = plan.apply(xs[k], band0=k, sigmainv=0.5).clone()
        s = amd.pcg.pcg_fused(ops[k], rhs[k], None, mdiv=sigmainv, tol=0.0, maxit=8, minit=8)[0].clone()
        return y, s
    seq = [job(k) for k in range(nband)]
    for own_stream in (False, True):
        for _ in range(3):
            out = [None] * nband

            def work(k):
                if own_stream:
                    with torch.cuda.stream(torch.cuda.Stream()):
                        out[k] = job(k)
                        torch.cuda.current_stream().synchronize()
                else:
                    out[k] = job(k)
            ts = [threading.Thread(target=work, args=(k,)) for k in range(nband)]
            for t in ts:
                t.start()
            for t in ts:
                t.join()
            torch.cuda.synchronize()
            for k in range(nband):
                assert torch.equal(out[k][0], seq[k][0]) and torch.equal(out[k][1], seq[k][1]), (own_stream, k)
    amd.psf.clear_plan_cache()


@pmp('op', ['apply', 'param_hessian', 'convolve2gaussres'])
def test_embedded_plan_on_two_streams_of_one_host_thread(amd, op):
    """An embedded plan goes through padded staging buffers that live on the plan.  ONE host thread that uses the plan
    on stream A and at once on stream B must not overwrite on B what A's kernels have yet to read: the buffers are per
    stream and are filled inside the plan's critical section, behind the stream dependency.  A is kept busy with
    unrelated work, the operation is enqueued on A for input a and straight away on B for input b, no host
    synchronisation in between; both results must equal the one-stream, synchronised ones bitwise.  fp64:
    2 x 100 x 120 embedded in 128 x 128 (plan.apply), 2 x 64 x 64 with a 128 x 128 PSF grid (ParamHessian), and
    2 x 64 x 64 on the 64 x 128 engine grid of the restoring beam (model branch: one staging pair serves band after band)."""
    dev = torch.device('cuda')
    gen = torch.Generator(device=dev).manual_seed(11)

    def rand(*shape, dtype=torch.float64):
        return torch.randn(shape, dtype=dtype, device=dev, generator=gen)
    amd.misc.clear_beam_cache()
    if op == 'apply':
        nb, nx, ny = 2, 100, 120
        plan = amd.psf.PsfConvPlan(rand(nb, 2 * nx, ny + 1, dtype=torch.complex128), nx, ny, 2 * ny)

        def f(x):
            return plan.apply(x, sigmainv=0.5)
    elif op == 'param_hessian':
        nb, nx, ny = 2, 64, 64
        _, _, dfunc, dhfunc = amd.misc.setup_parametrisation('exp', sigma=0.8, freq=np.linspace(1e9, 2e9, nb), lscale=0.5)
        f = amd.hessian.ParamHessian(rand(nb, 128, 65, dtype=torch.complex128), nx, ny, 128, 0.1 * rand(nb, nx, ny), 0.5,
                                     dfunc, dhfunc)
        assert f.fused
        plan = f.plan
    else:
        nb, nx, ny = 2, 64, 64
        xx, yy = torch.meshgrid(torch.arange(-nx / 2, nx / 2, dtype=torch.float64, device=dev),
                                torch.arange(-ny / 2, ny / 2, dtype=torch.float64, device=dev), indexing='ij')

        def f(x):
            return amd.misc.convolve2gaussres(x, xx, yy, (40.0, 24.0, 33.0), 1)
    a, b = rand(nb, nx, ny), rand(nb, nx, ny)
    ya = f(a).clone()
    torch.cuda.synchronize()
    yb = f(b).clone()
    torch.cuda.synchronize()
    if op == 'convolve2gaussres':
        plan = next(reversed(amd.misc._beam_cache._entries.values()))[0].plan
    assert plan.embed == {'apply': (128, 128), 'param_hessian': (64, 128), 'convolve2gaussres': (64, 128)}[op]
    m = rand(4096, 4096, dtype=torch.float32)
    m @ m                                           # the first product's one-off set-up stays out of the overlap
    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(A):
        for _ in range(8):                          # a few milliseconds of unrelated work ahead of the operation
            m @ m
        ga = f(a)
    with torch.cuda.stream(B):
        gb = f(b)
    A.synchronize()
    B.synchronize()
    assert torch.equal(ga, ya), "stream A computed on what stream B staged"
    assert torch.equal(gb, yb), "stream B computed on what stream A staged after it"
    amd.misc.clear_beam_cache()


@pmp('n,nb', [(512, 2), (1024, 1)])
def test_fp32_predictive_backtracking_matches_reference_loop(amd, n, nb):
    """fp32 parity of the default line search: backtrack=True runs the PREDICTIVE search (three fused
    scalars, beta from the predicted rho); the reference's loop recomputes <r', M r'> after every rejected step
    (pcg.py:96-101, backtrack='exact' here).  On a bench-like fp32 problem (Poisson uv weights, noisy dirty
    image, many rejected steps) both must take the same number of iterations and backtracking steps and give
    the same iterates to the fp32 PCG tolerance; and both must match the fp64 oracle solve to that tolerance."""
    rng = np.random.default_rng(420 + n)
    P = Q = 2 * n
    u = np.fft.fftfreq(P)[:, None]
    v = np.fft.rfftfreq(Q)[None, :]
    W = rng.poisson(4.0 * np.exp(-(u ** 2 + v ** 2) / (2 * 0.12 ** 2)), size=(nb, P, Q // 2 + 1)).astype(np.float64)
    psfhat64 = W / (nb * np.fft.irfft2(W, s=(P, Q))[:, 0, 0].max())
    model = np.zeros((nb, n, n))
    for _ in range(12):
        i, j = rng.integers(n // 8, 7 * n // 8, size=2)
        model[:, i, j] += 1 + rng.random()
    xpad, xhat, xout = ofc.make_scratch(psfhat64.astype(np.complex128), Q, model.shape, np.float64)
    ph128 = psfhat64.astype(np.complex128)
    b64 = ofc.psf_convolve_cube(xpad, xhat, xout, ph128, Q, model).copy() + 1e-3 * rng.standard_normal(model.shape)
    sigmainv = 1e-3 * np.abs(b64).max()
    A = amd.hessian.HessianPsf(torch.from_numpy(psfhat64.astype(np.complex64)).cuda(), n, n, Q, sigmainv=sigmainv)
    b32 = torch.from_numpy(b64.astype(np.float32)).cuda()
    kw = dict(mdiv=sigmainv, tol=0.0, maxit=25, minit=25)
    xp_, _, rp = amd.pcg.pcg_fused(A, b32, None, backtrack=True, **kw)
    xe_, _, re_ = amd.pcg.pcg_fused(A, b32, None, backtrack='exact', **kw)
    assert rp.iters == re_.iters == 25
    assert rp.backtracks > 0, "the problem must exercise the line search"
    scale = xe_.abs().max().item()
    assert (xp_ - xe_).abs().max().item() < TOL_PCG[np.float32] * scale
    assert abs(rp.backtracks - re_.backtracks) <= max(2, re_.backtracks // 10), (rp.backtracks, re_.backtracks)
    Ao = lambda w: ofc.hessian_psf_cube(xpad, xhat, xout, None, ph128, Q, w, sigmainv=sigmainv)
    tr = osv.PCGTrace()
    xo = osv.pcg(Ao, b64, None, M=lambda w: w / sigmainv, tol=0.0, maxit=25, minit=25, trace=tr)
    # Against the fp64 oracle: the line search compares rnorm_next > rnorm; where the two are equal to fp32 rounding
    # an fp32 run may take the other branch than the fp64 reference (alpha vs 0.75 alpha) and then follows a
    # different -- equally valid -- trajectory.  Same backtracking history => iterates agree to the fp32 PCG tolerance;
    # otherwise the solution quality (residual of the normal equations) must still match the oracle's.
    nbt_ref = int(np.sum(tr.nbacktrack))
    for xg, res in ((xp_, rp), (xe_, re_)):
        xh = xg.cpu().numpy().astype(np.float64)
        if res.backtracks == nbt_ref:
            assert relerr(xh, xo) < 5 * TOL_PCG[np.float32]
        r_gpu = np.linalg.norm(Ao(xh) - b64)
        r_ref = np.linalg.norm(Ao(xo) - b64)
        assert r_gpu < 1.5 * r_ref + 1e-6 * np.linalg.norm(b64), (res.backtracks, nbt_ref, r_gpu, r_ref)


@pmp('rdt', [np.float64, np.float32])
def test_config1_fifty_iterations_through_the_reference_entry_point(amd, rdt):
    """BASELINE config #1 as it is worded: 1024 x 1024, one band, dirty + PSF, FIFTY PCG iterations (tol = 0,
    minit = maxit = 50 -> 51 matvecs) through the drop-in `pcg(A, b, x0, M, ...)` with A = _hessian_psf_slice bound by
    functools.partial, the way the reference's workers bind it (pcg.py:262-267), against the fp64 oracle on the same
    inputs: fp64 iterates to 1e-9 (every backtracking decision must coincide), fp32 to the stated 1e-3 when the
    backtracking histories coincide and otherwise through the residual of the normal equations (see
    test_fp32_predictive_backtracking_matches_reference_loop for why fp32 is pinned only up to line-search ties)."""
    n, nit = 1024, 50
    rng = np.random.default_rng(420)
    P = Q = 2 * n
    u = np.fft.fftfreq(P)[:, None]
    v = np.fft.rfftfreq(Q)[None, :]
    W = rng.poisson(4.0 * np.exp(-(u ** 2 + v ** 2) / (2 * 0.12 ** 2)), size=(P, Q // 2 + 1)).astype(np.float64)
    ph128 = (W / np.fft.irfft2(W, s=(P, Q))[0, 0]).astype(np.complex128)
    model = np.zeros((n, n))
    for _ in range(25):
        i, j = rng.integers(n // 8, 7 * n // 8, size=2)
        model[i, j] += 1 + rng.random()
    xpad, xhat, xout = ofc.make_scratch(ph128, Q, model.shape, np.float64)
    b64 = ofc.psf_convolve_slice(xpad, xhat, xout, ph128, Q, model).copy() + 1e-3 * rng.standard_normal(model.shape)
    sigmainv = 1e-3 * np.abs(b64).max()
    Ao = lambda w: ofc._hessian_psf_slice(xpad, xhat, xout, ph128, None, Q, w, sigmainv=sigmainv)
    tr = osv.PCGTrace()
    xo = osv.pcg(Ao, b64, None, M=lambda w: w / sigmainv, tol=0.0, maxit=nit, minit=nit, trace=tr)
    assert tr.k_exit == nit
    cdt = np.complex128 if rdt == np.float64 else np.complex64
    ph = torch.from_numpy(ph128.astype(cdt)).cuda()
    b = torch.from_numpy(b64.astype(rdt)).cuda()
    A = partial(amd.hessian._hessian_psf_slice, None, None, None, ph, None, Q, sigmainv=sigmainv)
    x = amd.pcg.pcg(A, b, None, M=lambda w: w / sigmainv, tol=0.0, maxit=nit, minit=nit, verbosity=0)
    xh = x.cpu().numpy().astype(np.float64)
    if rdt == np.float64:
        assert relerr(xh, xo) < TOL_PCG[np.float64]
    else:
        r_gpu, r_ref = np.linalg.norm(Ao(xh) - b64), np.linalg.norm(Ao(xo) - b64)
        assert r_gpu < 1.5 * r_ref + 1e-6 * np.linalg.norm(b64), (r_gpu, r_ref)
        if relerr(xh, xo) >= 5 * TOL_PCG[np.float32]:
            # a different -- equally valid -- backtracking history: allowed only if the solve says so itself
            res = amd.pcg.pcg_fused(amd.hessian.HessianPsf(ph, n, n, Q, sigmainv=sigmainv), b[None], None, mdiv=sigmainv,
                                    tol=0.0, maxit=nit, minit=nit)[2]
            assert res.backtracks != int(np.sum(tr.nbacktrack)), (relerr(xh, xo), res.backtracks)
    amd.psf.clear_plan_cache()


def test_long_line_coverage_path_runs_the_fused_pcg(amd):
    """A grid neither the LDS kernels nor the fast path can hold (nx = 9000 > 8192, nx_psf = 18000): the plan takes the
    long-line coverage path (every FFT as global-memory passes) and the fused PCG on it -- fused dots out of its
    epilogue included -- follows the oracle's iterates."""
    rng = np.random.default_rng(9)
    nb, nx, ny = 1, 9000, 24
    P, Q = 2 * nx, 2 * ny
    psf = np.zeros((nb, P, Q))
    psf[:, P // 2 - 3:P // 2 + 4, Q // 2 - 3:Q // 2 + 4] = rng.random((nb, 7, 7))
    psf[:, P // 2, Q // 2] += 30.0
    psfhat = ofc.psfhat_from_psf(psf)
    b = rng.standard_normal((nb, nx, ny))
    sig = 0.5
    A = amd.hessian.HessianPsf(torch.from_numpy(psfhat).cuda(), nx, ny, Q, sigmainv=sig)
    assert not A.plan.fast_path and A.plan.embed is None
    xpad, xhat, xout = ofc.make_scratch(psfhat, Q, b.shape, np.float64)
    Ao = lambda v: ofc.hessian_psf_cube(xpad, xhat, xout, None, psfhat, Q, v, sigmainv=sig)
    assert relerr(A(torch.from_numpy(b).cuda()).cpu().numpy(), Ao(b)) < 1e-12
    x, _, res = amd.pcg.pcg_fused(A, torch.from_numpy(b).cuda(), None, mdiv=sig, tol=0.0, maxit=6, minit=6)
    xo = osv.pcg(Ao, b, None, M=lambda v: v / sig, tol=0.0, maxit=6, minit=6)
    assert res.iters == 6 and relerr(x.cpu().numpy(), xo) < 1e-9
