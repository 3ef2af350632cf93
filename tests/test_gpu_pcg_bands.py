"""
GPU tests of the batched per-band PCG (pfb_pcg_solve_bands, pcg_fused_bands, pcg_psf) and of the per-band
inner products out of the convolution (pfb_psfconv_apply_dots_bands): every band of one solve is its own
system, and its result must be the one a separate single-band solve gives, up to the order of the fp64 sums.
"""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from oracle import fftconv as ofc          # noqa: E402  (checker only)
from oracle import solvers as osv          # noqa: E402

pmp = pytest.mark.parametrize

TOL_PCG = {np.float64: 1e-9, np.float32: 1e-3}
TOL_DOT = {np.float64: 1e-12, np.float32: 1e-9}


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


def relerr(a, ref):
    a = np.asarray(a, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300)


def cdt(rdt):
    return np.complex64 if rdt == np.float32 else np.complex128


def _dots_bands(amd, plan, x, w, beam, nb, w2=True):
    """(per-band dots [nb, 3], cube dots [3], out) of one convolution on the plan's (possibly padded) arrays."""
    lib, _dev = amd.lib, amd.dev
    out = torch.empty_like(x)
    per = torch.full((nb, 3), float('nan'), dtype=torch.float64, device=x.device)
    _lib = amd._lib
    _lib.check(lib.pfb_psfconv_apply_dots_bands(plan.handle, 0, nb, _dev.ptr(x), _dev.ptr(beam), 1.3, 0.7,
                                                _dev.ptr(out), _dev.ptr(x), _dev.ptr(w) if w2 else None,
                                                _dev.ptr(per), _dev.stream()))
    out_b = out.clone()
    cube = torch.zeros(3, dtype=torch.float64, device=x.device)
    _lib.check(lib.pfb_psfconv_apply_dots(plan.handle, 0, nb, _dev.ptr(x), _dev.ptr(beam), 1.3, 0.7, _dev.ptr(out),
                                          _dev.ptr(x), _dev.ptr(w) if w2 else None, _dev.ptr(cube), _dev.stream()))
    torch.cuda.synchronize()
    # where both calls run the same kernel the per-band sums change nothing in the apply; per band the 4096-point fp32
    # rows and the one-product form take the plain inverse-row kernel (its own FFT rounding)
    same = bool(torch.equal(out, out_b))
    return per.cpu().numpy(), cube.cpu().numpy(), out_b.cpu().numpy().astype(np.float64), same


@pmp('case', [
    (3, 1024, 4096, np.float32, None),      # persistent inverse rows (2048 points), tiles cross band boundaries
    (3, 4096, 2048, np.float32, None),      # persistent inverse rows (1024 points)
    (2, 512, 8192, np.float32, None),       # 4096-point fp32 rows: the whole-cube persistent kernel once per band
    (2, 512, 8192, np.float64, None),       # fp64 2-row 16-element tile
    (4, 256, 8192, np.float64, None),       # 128 tiles per band < grid: band boundaries inside a trip, unvisited bands
    (4, 128, 4096, np.float32, None),       # 32 tiles per band, one tile per workgroup: three zero slots each
    (2, 2048, 4096, np.float64, None),      # fp64 2048-point rows
    (3, 256, 128, np.float64, None),        # plain fast-path kernels
    (2, 48, 40, np.float64, None),          # generic (line-per-workgroup) kernels
    (2, 100, 120, np.float64, 'embed'),     # embedded in a power-of-two plan
    (2, 9000, 24, np.float64, None),        # long-line coverage path
    (3, 64, 2048, np.float64, None),        # fp64 1024-point rows (4-row 512-thread tiles): 16 tiles per band, boundaries inside a trip
])
@pmp('with_beam', [False, True])
def test_conv_dots_per_band(amd, case, with_beam):
    nb, nx, ny, rdt, kind = case
    dev = torch.device('cuda')
    g = torch.Generator(device=dev).manual_seed(nx * 7 + ny)
    P, Q = 2 * nx, 2 * ny
    ctype = torch.complex64 if rdt == np.float32 else torch.complex128
    rtype = torch.float32 if rdt == np.float32 else torch.float64
    psfhat = torch.randn((nb, P, Q // 2 + 1), dtype=ctype, device=dev, generator=g)
    plan = amd.psf.PsfConvPlan(psfhat, nx, ny, Q)
    assert (plan.embed is not None) == (kind == 'embed')
    x = torch.randn((nb, nx, ny), dtype=rtype, device=dev, generator=g)
    w = torch.randn((nb, nx, ny), dtype=rtype, device=dev, generator=g)
    beam = (0.5 + torch.rand((nb, nx, ny), dtype=rtype, device=dev, generator=g)) if with_beam else None
    x, w, beam = plan.to_grid(x, nb), plan.to_grid(w, nb), plan.grid_beam(beam, nb)      # themselves unless embedded
    for w2 in (True, False):
        per, cube, o, same = _dots_bands(amd, plan, x, w, beam, nb, w2)
        xn, wn = x.cpu().numpy().astype(np.float64), w.cpu().numpy().astype(np.float64)
        for bl in range(nb):
            ref = [np.vdot(xn[bl], o[bl]), np.vdot(wn[bl], o[bl]) if w2 else 0.0, np.vdot(o[bl], o[bl])]
            scale = [np.linalg.norm(xn[bl]) * np.linalg.norm(o[bl]), np.linalg.norm(wn[bl]) * np.linalg.norm(o[bl]),
                     np.vdot(o[bl], o[bl])]
            for q in range(3):
                assert abs(per[bl, q] - ref[q]) <= TOL_DOT[rdt] * scale[q], (bl, q, per[bl, q], ref[q])
        ctol = TOL_DOT[rdt] if same else {np.float64: 1e-12, np.float32: 1e-5}[rdt]
        for q in range(3):
            assert abs(per[:, q].sum() - cube[q]) <= ctol * max(abs(per[:, q]).sum(), 1e-300), (q, cube)


def test_conv_dots_per_band_errors(amd):
    plan = amd.psf.PsfConvPlan(torch.randn((2, 128, 65), dtype=torch.complex128, device='cuda'), 64, 64, 128)
    x = torch.randn((2, 64, 64), dtype=torch.float64, device='cuda')
    out = torch.empty_like(x)
    d = torch.zeros(6, dtype=torch.float64, device='cuda')
    _dev = amd.dev
    assert amd.lib.pfb_psfconv_apply_dots_bands(plan.handle, 0, 2, _dev.ptr(x), None, 0.0, 0.0, _dev.ptr(out),
                                                _dev.ptr(x), None, None, _dev.stream()) == amd._lib.PFB_ERR_INVALID
    assert amd.lib.pfb_psfconv_apply_dots_bands(plan.handle, 1, 2, _dev.ptr(x), None, 0.0, 0.0, _dev.ptr(out),
                                                _dev.ptr(x), None, _dev.ptr(d), _dev.stream()) == amd._lib.PFB_ERR_INVALID


# ------------------------------------------------------------------------------------- golden band histories
@pmp('rdt', [np.float64, np.float32])
def test_band_history_golden_batched(amd, golden, rdt):
    """The reference's pcg_psf histories (tests/golden/pcg.npz), through pcg_fused_bands and through pcg_psf."""
    g = golden('pcg')
    psfhat, b, beam = g['psfhat'].astype(cdt(rdt)), g['b'].astype(rdt), g['beam'].astype(rdt)
    sigmainv, Q = float(g['sigmainv']), int(g['Q'])
    nband, nx, ny = b.shape
    tol = TOL_PCG[rdt]
    bd = torch.from_numpy(b).cuda()
    cases = [(f'band_{tag}_k{k}_bt{int(bt)}', bm, dict(tol=0.0, maxit=k, minit=k, backtrack=bt))
             for tag, bm in (('nobeam', None), ('beam', beam)) for k in (1, 2, 5, 20) for bt in (True, False)]
    if rdt == np.float64:       # exit iteration is tolerance-controlled: fp64 only
        cases += [('band_tol1e-2', None, dict(tol=1e-2, maxit=100, minit=1, backtrack=True)),
                  ('band_tol1e-2_minit15', None, dict(tol=1e-2, maxit=100, minit=15, backtrack=True))]
    for key, bm, kw in cases:
        A = amd.hessian.HessianPsf(psfhat, nx, ny, Q, beam=bm, sigmainv=sigmainv)
        x, _, res = amd.pcg.pcg_fused_bands(A, bd, torch.zeros_like(bd), mdiv=sigmainv, **kw)
        assert len(res) == nband
        assert relerr(x.cpu().numpy(), g[key]) < tol, key
        m = amd.pcg.pcg_psf(psfhat, b, np.zeros_like(b), bm, Q, 1, sigmainv, dict(verbosity=0, **kw))
        assert m.dtype == rdt
        assert relerr(m, g[key]) < tol, key


# ----------------------------------------------------------------------------------- mixed states in one solve
def _mixed_problem(nx=64, ny=128):
    """Five fp64 bands, A = conv + I, M = identity: band 0 b = A x0 (zero residual), band 1 a zero PSF (A = I:
    exact in one step, then an all-zero direction), bands 2 and 3 mild PSFs that meet the tolerance at different
    k, band 4 a strong, ill-conditioned PSF that runs to maxit."""
    rng = np.random.default_rng(77)
    P, Q = 2 * nx, 2 * ny
    u = np.fft.fftfreq(P)[:, None]
    v = np.fft.rfftfreq(Q)[None, :]
    psfhat = np.zeros((5, P, Q // 2 + 1), dtype=np.complex128)
    for bl, (amp, width) in enumerate([(1.0, 0.1), (0.0, 0.1), (0.5, 0.2), (8.0, 0.05), (3000.0, 0.02)]):
        psfhat[bl] = amp * np.exp(-(u ** 2 + v ** 2) / (2 * width ** 2))
    b = rng.standard_normal((5, nx, ny))
    b[1] = rng.integers(-3, 4, (nx, ny))       # small integers: <r, r> is exact in any summation order, so alpha = 1
    x0 = np.zeros((5, nx, ny))
    x0[0] = rng.standard_normal((nx, ny))
    xpad, xhat, xout = ofc.make_scratch(psfhat[:1], Q, (1, nx, ny), np.float64)
    b[0] = ofc.hessian_psf_cube(xpad, xhat, xout, None, psfhat[:1], Q, x0[:1], sigmainv=1.0)[0]
    return psfhat, b, x0, Q


def test_mixed_band_states_match_separate_solves(amd, monkeypatch):
    psfhat, b, x0, Q = _mixed_problem()
    nband, nx, ny = b.shape
    kw = dict(tol=1e-6, maxit=25, minit=2)
    A = amd.hessian.HessianPsf(psfhat, nx, ny, Q, sigmainv=1.0)
    # b of band 0 as the DEVICE operator computes it, so that its initial residual is exactly zero
    b[0] = amd.hessian.HessianPsf(A.plan, nx, ny, Q, sigmainv=1.0, band0=0, nb=1)(
        torch.from_numpy(x0[:1]).cuda()).cpu().numpy()[0]
    bd, x0d = torch.from_numpy(b).cuda(), torch.from_numpy(x0).cuda()
    for la in ('1', '0'):
        monkeypatch.setenv('PFB_PCG_LOOKAHEAD', la)
        for bt in (True, False):
            x, r, res = amd.pcg.pcg_fused_bands(A, bd, x0d, backtrack=bt, return_resid=True, **kw)
            x, r = x.cpu().numpy(), r.cpu().numpy()
            sep = []
            for bl in range(nband):
                Ab = amd.hessian.HessianPsf(A.plan, nx, ny, Q, sigmainv=1.0, band0=bl, nb=1)
                xs, rs, rb = amd.pcg.pcg_fused(Ab, bd[bl:bl + 1], x0d[bl:bl + 1], backtrack=bt, return_resid=True, **kw)
                sep.append(rb)
                for f in ('status', 'iters', 'matvecs', 'backtracks'):
                    assert getattr(res[bl], f) == getattr(rb, f), (la, bt, bl, f, getattr(res[bl], f), getattr(rb, f))
                assert relerr(x[bl], xs.cpu().numpy()[0]) < 1e-12, (la, bt, bl)
                assert np.abs(r[bl] - rs.cpu().numpy()[0]).max() <= 1e-12 * max(np.abs(b[bl]).max(), 1.0), (la, bt, bl)
            # the states this problem is built to hold
            st = [_status(amd, s) for s in sep]
            assert st[0] == 'zero-residual' and np.array_equal(x[0], x0[0])
            assert st[1] == 'breakdown' and sep[1].iters == 0
            assert st[2] == st[3] == 'converged' and sep[2].iters != sep[3].iters
            assert st[4] == 'maxit' and sep[4].iters == kw['maxit']


def _status(amd, res):
    return amd._lib.PCG_STATUS[res.status]


# ------------------------------------------------------------------------------------------ large persistent
@pmp('case', [(3, 1024, 4096, np.float32), (2, 512, 8192, np.float64)])
def test_large_persistent_bands_vs_oracle(amd, case):
    nb, nx, ny, rdt = case
    rng = np.random.default_rng(11)
    P, Q = 2 * nx, 2 * ny
    u = np.fft.fftfreq(P)[:, None]
    v = np.fft.rfftfreq(Q)[None, :]
    psfhat = np.stack([np.exp(-(u ** 2 + v ** 2) / (2 * (0.05 + 0.03 * k) ** 2)) * (1 + k)
                       for k in range(nb)]).astype(np.complex128)
    b = rng.standard_normal((nb, nx, ny))
    sig = 0.2
    A = amd.hessian.HessianPsf(torch.from_numpy(psfhat.astype(cdt(rdt))).cuda(), nx, ny, Q, sigmainv=sig)
    x, _, res = amd.pcg.pcg_fused_bands(A, torch.from_numpy(b.astype(rdt)).cuda(), None, mdiv=sig, tol=0.0,
                                        maxit=6, minit=6)
    x = x.cpu().numpy()
    for bl in range(nb):
        xpad, xhat, xout = ofc.make_scratch(psfhat[bl:bl + 1], Q, (1, nx, ny), np.float64)
        Ao = lambda w: ofc.hessian_psf_cube(xpad, xhat, xout, None, psfhat[bl:bl + 1], Q, w, sigmainv=sig)
        xo = osv.pcg(Ao, b[bl:bl + 1], None, M=lambda w: w / sig, tol=0.0, maxit=6, minit=6)
        assert res[bl].iters == 6 and _status(amd, res[bl]) == 'maxit'
        assert relerr(x[bl], xo[0]) < TOL_PCG[rdt], bl


# ----------------------------------------------------------------------------------------------- routing
def test_pcg_psf_routes_to_one_batched_solve(amd, golden, monkeypatch):
    g = golden('pcg')
    psfhat, b = g['psfhat'], g['b']
    sigmainv, Q = float(g['sigmainv']), int(g['Q'])
    P = amd.pcg
    calls = {'bands': 0, 'single': 0}
    orig_b, orig_s = P.pcg_fused_bands, P.pcg_fused

    def spy_b(*a, **k):
        calls['bands'] += 1
        return orig_b(*a, **k)

    def spy_s(*a, **k):
        calls['single'] += 1
        return orig_s(*a, **k)
    monkeypatch.setattr(P, 'pcg_fused_bands', spy_b)
    monkeypatch.setattr(P, 'pcg_fused', spy_s)
    opts = dict(tol=0.0, maxit=3, minit=3, verbosity=0)
    m = P.pcg_psf(psfhat, b, np.zeros_like(b), None, Q, 1, sigmainv, dict(opts, backtrack=True))
    assert calls == {'bands': 1, 'single': 0}
    me = P.pcg_psf(psfhat, b, np.zeros_like(b), None, Q, 1, sigmainv, dict(opts, backtrack='exact'))
    assert calls == {'bands': 1, 'single': b.shape[0]}
    monkeypatch.setenv('PFB_PCG_EXACT_BACKTRACK', '1')
    P.pcg_psf(psfhat, b, np.zeros_like(b), None, Q, 1, sigmainv, dict(opts, backtrack=True))
    assert calls == {'bands': 1, 'single': 2 * b.shape[0]}
    assert relerr(m, me) < 1e-9


def test_pcg_psf_keeps_the_loop_on_fp32_8192_pixel_rows(amd, monkeypatch):
    """fp32 plans of 8192-pixel rows have no per-band persistent inverse kernel: pcg_psf stays band by band there
    (also for an image embedded in such a plan), and pcg_fused_bands still gives each band's single-band result."""
    P = amd.pcg
    calls = {'bands': 0, 'single': 0}
    orig_b, orig_s = P.pcg_fused_bands, P.pcg_fused

    def spy_b(*a, **k):
        calls['bands'] += 1
        return orig_b(*a, **k)

    def spy_s(*a, **k):
        calls['single'] += 1
        return orig_s(*a, **k)
    monkeypatch.setattr(P, 'pcg_fused_bands', spy_b)
    monkeypatch.setattr(P, 'pcg_fused', spy_s)
    rng = np.random.default_rng(3)
    opts = dict(tol=0.0, maxit=3, minit=3, verbosity=0)
    for nx, ny in ((64, 8192), (64, 6000)):
        Q = 2 * ny
        u = np.fft.fftfreq(2 * nx)[:, None]
        v = np.fft.rfftfreq(Q)[None, :]
        psfhat = np.stack([np.exp(-(u ** 2 + v ** 2) / (2 * w ** 2)) for w in (0.1, 0.2)]).astype(np.complex64)
        b = rng.standard_normal((2, nx, ny)).astype(np.float32)
        before = dict(calls)
        m = P.pcg_psf(psfhat, b, np.zeros_like(b), None, Q, 1, 0.5, dict(opts, backtrack=True))
        assert calls['bands'] == before['bands'] and calls['single'] == before['single'] + 2
        A = amd.hessian.HessianPsf(psfhat, nx, ny, Q, sigmainv=0.5)
        x, _, res = P.pcg_fused_bands(A, torch.from_numpy(b).cuda(), None, mdiv=0.5, tol=0.0, maxit=3, minit=3)
        assert [r.iters for r in res] == [3, 3]
        assert relerr(x.cpu().numpy(), m) < TOL_PCG[np.float32]


def test_pcg_psf_batched_log_lines(amd, golden, capfd):
    g = golden('pcg')
    psfhat, b = g['psfhat'], g['b']
    sigmainv, Q = float(g['sigmainv']), int(g['Q'])
    nband = b.shape[0]
    bz = b.copy()
    bz[0] = 0.0                                     # x0 = 0, b = 0: the initial residual is zero
    m = amd.pcg.pcg_psf(psfhat, bz, np.zeros_like(bz), None, Q, 1, sigmainv,
                        dict(tol=0.0, maxit=4, minit=4, verbosity=1, backtrack=True))
    err = capfd.readouterr().err
    assert err.count("Initial residual is zero") == 1
    assert err.count("Max iters reached") == nband - 1
    assert not m[0].any()


# ------------------------------------------------------------------------------------------ argument errors
def test_solve_bands_argument_errors(amd):
    lib, _dev, _lib = amd.lib, amd.dev, amd._lib
    nx, ny = 64, 128
    A = amd.hessian.HessianPsf(torch.randn((2, 2 * nx, ny + 1), dtype=torch.complex128, device='cuda'), nx, ny,
                               2 * ny, sigmainv=1.0)
    b = torch.randn((2, nx, ny), dtype=torch.float64, device='cuda')
    x = torch.zeros_like(b)
    nbytes = lib.pfb_pcg_bands_work_bytes(A.plan.handle, 2)
    assert nbytes > 3 * b.numel() * 8
    work = torch.empty(nbytes + 256, dtype=torch.uint8, device='cuda')
    res = (_lib.PcgResult * 2)()

    def call(band0=0, nb=2, results=res, w=_dev.ptr(work), backtrack=2):
        return lib.pfb_pcg_solve_bands(A.plan.handle, band0, nb, _dev.ptr(b), _dev.ptr(x), None, None, 0.0, 1.0, 1.0,
                                       1e-5, 5, 1, backtrack, w, results, _dev.stream())
    assert call(band0=1) == _lib.PFB_ERR_INVALID
    assert call(nb=0) == _lib.PFB_ERR_INVALID
    assert call(band0=-1) == _lib.PFB_ERR_INVALID
    assert call(results=None) == _lib.PFB_ERR_INVALID
    assert call(w=_dev.ptr(work) + 8) == _lib.PFB_ERR_INVALID
    assert call(backtrack=1) == _lib.PFB_ERR_UNSUPPORTED
    assert not x.any()                              # nothing ran
    assert call() == 0
    with pytest.raises(_lib.PfbHipError):
        amd.pcg.pcg_fused_bands(A, b, None, backtrack='exact')


# ------------------------------------------------------------------------------------------ work buffer bounds
GUARD, SENTINEL = 4096, 0xA5


def _guarded_solve(amd, plan, solve, nb, bt, b, L, slack):
    """One native solve (3 fixed iterations, x0 = 0) whose `work` is a slice of a larger buffer: exactly the entry
    point's *_work_bytes (+ slack) usable bytes with GUARD bytes of SENTINEL on either side.  Returns (x, result
    fields, the two guard regions after the solve)."""
    lib, _dev, _lib = amd.lib, amd.dev, amd._lib
    nbytes = {'cube': lib.pfb_pcg_work_bytes, 'bands': lib.pfb_pcg_bands_work_bytes,
              'param': lib.pfb_pcg_param_work_bytes}[solve](plan.handle, nb) + slack
    assert nbytes > slack
    big = torch.full((GUARD + nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device='cuda')
    work = big.data_ptr() + GUARD
    assert work % 256 == 0
    x, LH = torch.zeros_like(b), L.T.contiguous()
    res = (_lib.PcgResult * nb)()
    tail = (1.0, 1.0, 0.0, 3, 3, bt, work)           # sigmainv, mdiv, tol, maxit, minit, backtrack, work
    if solve == 'cube':
        plan.run('pfb_pcg_solve', 0, nb, _dev.ptr(b), _dev.ptr(x), None, None, 0.0, *tail, _lib.ALLREDUCE_FN(0), None, res)
    elif solve == 'bands':
        plan.run('pfb_pcg_solve_bands', 0, nb, _dev.ptr(b), _dev.ptr(x), None, None, 0.0, *tail, res)
    else:
        plan.run('pfb_pcg_solve_param', nb, _dev.ptr(L), _dev.ptr(LH), None, _dev.ptr(b), _dev.ptr(x), None, *tail, res)
    torch.cuda.synchronize()
    nres = nb if solve == 'bands' else 1
    fields = [tuple(getattr(r, f) for f, _ in _lib.PcgResult._fields_) for r in res[:nres]]
    return x.cpu().numpy(), fields, (big[:GUARD].cpu().numpy(), big[GUARD + nbytes:].cpu().numpy())


@pmp('rdt', [np.float32, np.float64])
@pmp('solve,nb,bt', [('cube', 2, 2), ('cube', 2, 1), ('bands', 2, 2), ('param', 3, 2)])
def test_solves_stay_inside_their_work_bytes(amd, solve, nb, bt, rdt):
    """Every native solve writes inside the *_work_bytes it asks for: with exactly that many usable bytes between two
    guard regions the guards stay untouched, and x and the results equal those of a solve with 64 KB to spare.
    64 x 128 is the smallest fast-path image (the persistent kernels' partial layout); backtrack 1 is the one mode that
    reaches the alternates through the exact loop; the layout does not depend on the plan class."""
    nx, ny = 64, 128
    u = np.fft.fftfreq(2 * nx)[:, None]
    v = np.fft.rfftfreq(2 * ny)[None, :]
    psfhat = np.stack([(1 + k) * np.exp(-(u ** 2 + v ** 2) / (2 * (0.1 + 0.05 * k) ** 2)) for k in range(nb)])
    plan = amd.psf.PsfConvPlan(psfhat.astype(cdt(rdt)), nx, ny, 2 * ny)
    assert plan.fast_path and plan.embed is None
    rng = np.random.default_rng(5)
    b = torch.from_numpy(rng.standard_normal((nb, nx, ny)).astype(rdt)).cuda()
    L = torch.from_numpy(np.tril(0.5 + rng.random((nb, nb))).astype(rdt)).cuda()
    x, res, guards = _guarded_solve(amd, plan, solve, nb, bt, b, L, 0)
    for g in guards:
        assert g.size == GUARD and (g == SENTINEL).all()
    assert all(r[1] == 3 for r in res) and x.any(), res
    x2, res2, guards2 = _guarded_solve(amd, plan, solve, nb, bt, b, L, 65536)
    for g in guards2:
        assert g.size == GUARD and (g == SENTINEL).all()
    assert np.array_equal(x, x2)
    assert res == res2
