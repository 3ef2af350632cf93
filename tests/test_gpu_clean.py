"""
The CLEAN minor cycle and the band coupling on the MI355X (csrc/clark.hip: pfb_clark_subminor, pfb_hogbom, pfb_freqmul)
through the C ABI, against oracle/clark.py in float64 and np.einsum in float64.  tests/clean_cases.py builds the inputs,
tests/test_cpu_clean.py checks what the comparisons lean on.

Bounds:
  exact cases   integer cubes, a PSF of 0 / +-0.5 / 1, dyadic wsums, gamma 0.5 or 1, at most 16 iterations: every operation
                is exact in float32 and float64, so model, residual / active set and iteration count equal the oracle's with
                np.array_equal in both precisions.  Exact ties at the maximum occur in every case of more than one pixel;
                the first index has to win.  The last Hogbom peak: == in float64, within one float32 ulp in float32.
  smooth cases  float64 1e-11 max|ref|; float32 2e-4 max|ref| (sub-minor loop, clark) and 5e-4 max|ref| (Hogbom), the bounds
                of test_clark_minor_cycle / test_hogbom, on the model and on the residual / active set.  The reference runs
                in float64 on the inputs rounded to the dtype.  A greedy loop is comparable only while rounding cannot flip a
                choice: every test first asserts that each decision of the reference run keeps a relative margin of 2e-3
                (float32) / 1e-9 (float64), ten times the tolerance.
  freqmul       |got - ref| <= (nband + 3) eps sum_l |A_kl| |x_l| |pre_l| |post_k|: one rounding for x pre, nband for the
                products and the sum, one for post, one to spare; eps the unit roundoff 2^-24 / 2^-53.
Launch geometry the shapes are chosen for (csrc/clark.hip): the sub-minor loop is ONE workgroup of 1024 threads (16 waves),
so nact > 1024 makes a thread loop and nact > 64 merges waves through LDS; k_hogbom_step is 1024 workgroups of 256 threads,
so 520 x 509 = 264 680 pixels make 2 536 threads loop twice; pfb_hogbom looks at the loop state every 64 iterations;
k_freqmul runs at most 4096 workgroups of 256 threads and keeps nband values per thread and nband^2 in LDS (nband <= 64).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import clean_cases as cc

pytestmark = pytest.mark.gpu

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
DTYPES = [F32, F64]
TOL_CLARK = {F32: 2e-4, F64: 1e-11}
TOL_HOGBOM = {F32: 5e-4, F64: 1e-11}
EPS = {F32: 2.0 ** -24, F64: 2.0 ** -53}
_dcache = {}


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cached(a, dtype):
    """A device copy of a memoised host array in `dtype` (the 2 x 1040 x 1018 PSFs are shared between tests)."""
    key = (id(a), np.dtype(dtype))
    if key not in _dcache:
        _dcache[key] = (a, cuda(a.astype(dtype)))
    return _dcache[key][1]


def close(tag, got, ref, tol):
    ref = np.asarray(ref, dtype=np.float64)
    err, scale = float(np.abs(np.asarray(got, dtype=np.float64) - ref).max()), float(np.abs(ref).max())
    print(f'{tag}: err {err:.3e} = {err / scale if scale else 0:.2e} max|ref| (bound {tol:.0e})')
    assert err <= tol * scale, (tag, err, tol * scale)


def assert_margin(tr, dtype, extra=np.inf):
    m = min(tr.margin(), extra)
    print(f'least margin of the reference run {m:.3e}')
    assert m >= cc.MARGIN[dtype], m


def sub_call(c, dtype, maxit, th=None, psf_shape=None, nband=None):
    """pfb_clark_subminor on case c in `dtype`.  Returns (rc, model, A, iters)."""
    from pfb_clean_amd import _lib, _dev
    lib = _lib.load()
    A, model = cuda(c['A'].astype(dtype)), cuda(c['model0'].astype(dtype))
    psf, w = cached(c['psf'], dtype), cuda(c['wsums'].astype(dtype))
    ip, iq = cuda(c['Ip'].astype(np.int32)), cuda(c['Iq'].astype(np.int32))
    it = torch.full((1,), -7, dtype=torch.int32, device='cuda')
    P, Q = psf.shape[1:] if psf_shape is None else psf_shape
    rc = lib.pfb_clark_subminor(_dev.code(A.dtype), _dev.ptr(A), A.shape[1], A.shape[0] if nband is None else nband,
                                _dev.ptr(psf), P, Q, _dev.ptr(ip), _dev.ptr(iq), _dev.ptr(model), c['nx'], c['ny'],
                                _dev.ptr(w), float(c['gamma']), float(c['th'] if th is None else th), int(maxit),
                                _dev.ptr(it), _dev.stream())
    torch.cuda.synchronize()
    return rc, model.cpu().numpy(), A.cpu().numpy(), int(it.item())


def hog_call(c, dtype, maxit, work_bytes=cc.HOG_WORK, psf_shape=None, nband=None, **kw):
    """pfb_hogbom on case c in `dtype`, wsums = the PSF peaks as deconv/hogbom.py passes them.
    Returns (rc, model, IR, k, irmax)."""
    from pfb_clean_amd import _lib, _dev
    lib = _lib.load()
    IR = cuda(c['ID'].astype(dtype))
    psf = cached(c['psf'], dtype)
    with np.errstate(invalid='ignore'):
        w = cuda(np.amax(c['psf'].astype(dtype), axis=(1, 2)))
    model = torch.zeros_like(IR)
    work = torch.zeros(cc.HOG_WORK, dtype=torch.uint8, device='cuda')
    k, irmax = C.c_int(-7), C.c_double(-7.0)
    a = dict(threshold=c['threshold'], gamma=c['gamma'], pf=c['pf'])
    a.update(kw)
    P, Q = psf.shape[1:] if psf_shape is None else psf_shape
    rc = lib.pfb_hogbom(_dev.code(IR.dtype), _dev.ptr(IR), _dev.ptr(psf), _dev.ptr(model), _dev.ptr(w),
                        IR.shape[0] if nband is None else nband, IR.shape[1], IR.shape[2], P, Q, float(a['gamma']),
                        float(a['pf']), float(a['threshold']), int(maxit), _dev.ptr(work), int(work_bytes),
                        C.addressof(k), C.addressof(irmax), _dev.stream())
    torch.cuda.synchronize()
    return rc, model.cpu().numpy(), IR.cpu().numpy(), k.value, irmax.value


def same_irmax(got, ref, dtype):
    if dtype == F64:
        return got == float(ref)
    r32 = np.float32(ref)
    return abs(got - float(r32)) <= float(np.spacing(r32))


# ------------------------------------------------------------------------------------------------ pfb_clark_subminor
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', list(cc.SUB_EXACT_CASES))
def test_subminor_exact(name, dtype):
    """nact 1 .. 2 x 1024 + 37 on 40 x 53 (one lane, one wave, two waves, the full workgroup, one and 37 pixels into the
    second and third trip), constructed ties, nband 1 / 64, a zero wsum, even and oversized PSFs, a non-zero model on
    entry with a pixel taken twice.  maxit 1 shows which pixel is taken FIRST."""
    c = cc.sub_exact(**cc.SUB_EXACT_CASES[name])
    for maxit in (1, 16):
        model, k, A, tr = cc.run_sub(c, maxit)
        rc, gm, gA, gk = sub_call(c, dtype, maxit)
        assert rc == 0 and gk == k, (maxit, gk, k)
        assert np.array_equal(gm, model), (name, maxit, np.argwhere(gm != model)[:4].tolist())
        assert np.array_equal(gA, A), (name, maxit)
        if maxit == 1 and name.startswith('tie_'):
            first = min(cc.SUB_TIES[name[4:]])
            assert tr.pick[0] == first and np.all(gm[:, c['Ip'][first], c['Iq'][first]] != 0)
            assert np.count_nonzero(gm) == gm.shape[0]


@pytest.mark.parametrize('dtype', DTYPES)
def test_subminor_stops(dtype):
    """maxit 0, and a threshold above the first maximum: no iteration, model and active set untouched."""
    c = cc.sub_exact(model0=True)
    first = float(np.sqrt((c['A'].sum(axis=0) ** 2).max()))
    for maxit, th in ((0, None), (16, first + 1.0), (16, first)):           # `>`: the maximum itself does not pass
        model, k, A, _ = cc.run_sub(c, maxit, th=th)
        rc, gm, gA, gk = sub_call(c, dtype, maxit, th=th)
        assert rc == 0 and gk == k == 0
        assert np.array_equal(gm, c['model0']) and np.array_equal(gA, c['A'])
    rc, gm, gA, gk = sub_call(c, dtype, 16, th=np.nextafter(np.float32(first), np.float32(0)))
    assert rc == 0 and gk == cc.run_sub(c, 16, th=float(np.nextafter(np.float32(first), np.float32(0))))[1] > 0


def test_subminor_rejects():
    from pfb_clean_amd import _lib
    lib = _lib.load()
    c = dict(cc.sub_exact(nact=65))
    nx, ny = c['nx'], c['ny']
    c['psf'] = cc.memo('psf_small', lambda: np.zeros((3, 2 * nx - 2, 2 * ny - 1)))
    rc, gm, gA, gk = sub_call(c, F64, 16)
    assert rc == _lib.PFB_ERR_UNSUPPORTED and b'must cover' in lib.pfb_last_error()
    assert gk == -7 and not gm.any() and np.array_equal(gA, c['A'])                 # nothing launched
    c = dict(cc.sub_exact(nact=65))
    c['psf'] = cc.memo('psf_short', lambda: np.zeros((3, 2 * nx - 1, 2 * ny - 2)))
    assert sub_call(c, F32, 16)[0] == _lib.PFB_ERR_UNSUPPORTED
    c = cc.sub_exact(nact=65, nband=65)                                             # every buffer holds 65 bands
    rc, gm, gA, gk = sub_call(c, F64, 16)
    assert rc == _lib.PFB_ERR_UNSUPPORTED and gk == -7 and not gm.any()
    assert sub_call(cc.sub_exact(nact=65), F64, 16, nband=0)[0] == _lib.PFB_ERR_UNSUPPORTED


@pytest.mark.parametrize('dtype', DTYPES)
def test_subminor_smooth(dtype):
    """70 x 90, 1499 active pixels, stopped by the threshold after a dozen components, some from a thread's second trip."""
    c = cc.sub_smooth(dtype)
    maxit = cc.SUB_SMOOTH[dtype]['maxit']
    model, k, A, tr = cc.run_sub(cc.f64(c), maxit)
    assert_margin(tr, dtype)
    rc, gm, gA, gk = sub_call(c, dtype, maxit)
    assert rc == 0 and gk == k and 0 < k < maxit
    assert np.array_equal(gm != 0, model != 0)
    close(f'sub-minor smooth {dtype.name} model', gm, model, TOL_CLARK[dtype])
    close(f'sub-minor smooth {dtype.name} active set', gA, A, TOL_CLARK[dtype])


@pytest.mark.parametrize('dtype', DTYPES)
def test_subminor_nan_stops_the_loop(dtype):
    """np.argmax returns the first NaN and `NaN > th` is false: no component is taken once a NaN is among the band sums."""
    base = cc.sub_exact(model0=True)
    for where in (0, 70, 684, 300):                 # lane 0, another wave, the last pixel, and two NaNs (300 and 684)
        c = dict(base)
        c['A'] = base['A'].copy()
        c['A'][1, where] = np.nan
        if where == 300:
            c['A'][0, 684] = np.nan
        rc, gm, gA, gk = sub_call(c, dtype, 16)
        assert rc == 0 and gk == 0, (where, gk)
        assert np.array_equal(gm, c['model0']) and np.array_equal(gA, c['A'], equal_nan=True)
    c = cc.sub_nan_case()                           # the NaN appears when the second component is subtracted
    model, k, A, tr = cc.run_sub(c, 16)
    rc, gm, gA, gk = sub_call(c, dtype, 16)
    assert rc == 0 and gk == k == 2
    assert np.array_equal(gm, model) and np.array_equal(gA, A, equal_nan=True) and np.isnan(gA).sum() == 1


# ------------------------------------------------------------------------------------------------ pfb_hogbom
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', list(cc.HOG_EXACT_CASES))
def test_hogbom_exact(name, dtype):
    """1 x 1, 1 x 7, 7 x 1, 31 x 17 (the i / j split and the two PSF centres differ), nband 1 / 64, even and oversized
    PSFs; stopped by threshold 2.0 or by 16 iterations."""
    c = cc.hog_exact(**cc.HOG_EXACT_CASES[name])
    for maxit in (16, 1):
        x, status, IR, k, irmax, tr = cc.run_hog(c, maxit)
        rc, gm, gIR, gk, girmax = hog_call(c, dtype, maxit)
        assert rc == 0 and gk == k, (maxit, gk, k)
        assert np.array_equal(gm, x) and np.array_equal(gIR, IR), (name, maxit)
        assert same_irmax(girmax, irmax, dtype), (girmax, irmax)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', list(cc.HOG_BIG_CASES))
def test_hogbom_grid_stride_ties(name, dtype):
    """2 x 520 x 509: the first maximum shared by flat indices (5, 262144 + 5), one thread's two trips; by
    (300, 262144 + 7), the lower index in the higher workgroup; by all four.  The lowest flat index is taken first."""
    kw = cc.HOG_BIG_CASES[name]
    c = cc.hog_exact(**kw)
    ny = kw['ny']
    for maxit in (1, 16):
        x, status, IR, k, irmax, tr = cc.run_hog(c, maxit)
        rc, gm, gIR, gk, girmax = hog_call(c, dtype, maxit)
        assert rc == 0 and gk == k == maxit
        if maxit == 1:
            first = min(kw['tie'])
            assert tr.pick[0] == first and np.all(gm[:, first // ny, first % ny] != 0)
            assert np.count_nonzero(gm) == gm.shape[0]
        assert np.array_equal(gm, x) and np.array_equal(gIR, IR), (name, maxit)
        assert same_irmax(girmax, irmax, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
def test_hogbom_grid_stride_smooth(dtype):
    c = cc.hog_smooth_big(dtype)
    maxit = cc.HOG_SMOOTH_BIG[dtype]['maxit']
    x, status, IR, k, irmax, tr = cc.run_hog(cc.f64(c), maxit)
    assert_margin(tr, dtype)
    assert any(p >= cc.HOG_THREADS for p in tr.pick[:k]) and any(p < cc.HOG_THREADS for p in tr.pick[:k])
    rc, gm, gIR, gk, girmax = hog_call(c, dtype, maxit)
    assert rc == 0 and gk == k == maxit
    assert np.array_equal(gm != 0, x != 0)
    close(f'hogbom 520 x 509 {dtype.name} model', gm, x, TOL_HOGBOM[dtype])
    close(f'hogbom 520 x 509 {dtype.name} residual', gIR, IR, TOL_HOGBOM[dtype])
    close(f'hogbom 520 x 509 {dtype.name} peak', girmax, irmax, TOL_HOGBOM[dtype])


@pytest.mark.parametrize('maxit', cc.HOG_BATCH_MAXIT)
def test_hogbom_batch_boundary(maxit):
    """pf = 0 and threshold = 0: maxit alone stops the loop, one short of, at and one past the 64-iteration batch after
    which the host looks at the loop state, and in the third batch."""
    from pfb_clean_amd.deconv.hogbom import hogbom
    c = cc.hog_smooth(F64, **cc.HOG_SMOOTH_SMALL)
    x, status, IR, k, irmax, tr = cc.run_hog(c, maxit)
    assert_margin(tr, F64)
    rc, gm, gIR, gk, girmax = hog_call(c, F64, maxit)
    assert rc == 0 and gk == k == maxit
    close(f'maxit {maxit} model', gm, x, TOL_HOGBOM[F64])
    close(f'maxit {maxit} residual', gIR, IR, TOL_HOGBOM[F64])
    close(f'maxit {maxit} peak', girmax, irmax, TOL_HOGBOM[F64])
    wm, wstatus = hogbom(c['ID'], c['psf'], threshold=0.0, gamma=c['gamma'], pf=0.0, maxit=maxit, verbosity=0)
    assert wstatus == status == 1 and np.array_equal(wm, gm)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('maxit', [0, 1, 16])
def test_hogbom_maxit_exact(maxit, dtype):
    from pfb_clean_amd.deconv.hogbom import hogbom
    c = cc.hog_exact(31, 17)
    x, status, IR, k, irmax, tr = cc.run_hog(c, maxit, pf=0.0, threshold=0.0)
    rc, gm, gIR, gk, girmax = hog_call(c, dtype, maxit, pf=0.0, threshold=0.0)
    assert rc == 0 and gk == k == maxit and np.array_equal(gm, x) and np.array_equal(gIR, IR)
    assert same_irmax(girmax, irmax, dtype)
    wm, wstatus = hogbom(c['ID'].astype(dtype), c['psf'].astype(dtype), threshold=0.0, gamma=1.0, pf=0.0, maxit=maxit,
                         verbosity=0)
    assert wstatus == status == 1 and wm.dtype == dtype and np.array_equal(wm, x)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('stop', list(cc.HOG_STOPS))
def test_hogbom_stop_rules(stop, dtype):
    """Stopped by pf alone (tol = pf x the first peak) and by the threshold alone, 2 x 37 x 22 smooth."""
    c = cc.hog_smooth(dtype, **cc.HOG_SMOOTH_STOP)
    kw = cc.HOG_STOPS[stop]
    x, status, IR, k, irmax, tr = cc.run_hog(cc.f64(c), 10000, **kw)
    assert_margin(tr, dtype)
    rc, gm, gIR, gk, girmax = hog_call(c, dtype, 10000, **kw)
    assert rc == 0 and gk == k and 0 < k < 64 and status == 0
    close(f'stop by {stop} {dtype.name} model', gm, x, TOL_HOGBOM[dtype])
    close(f'stop by {stop} {dtype.name} residual', gIR, IR, TOL_HOGBOM[dtype])
    close(f'stop by {stop} {dtype.name} peak', girmax, irmax, TOL_HOGBOM[dtype])


def test_hogbom_rejects():
    from pfb_clean_amd import _lib
    lib = _lib.load()
    c = dict(cc.hog_exact(31, 17))
    rc, gm, gIR, gk, _ = hog_call(c, F64, 16, work_bytes=cc.HOG_NEED - 1)
    assert rc == _lib.PFB_ERR_INVALID and b'work buffer' in lib.pfb_last_error()
    assert gk == -7 and not gm.any() and np.array_equal(gIR, c['ID'])               # nothing launched
    assert hog_call(c, F64, 16, work_bytes=cc.HOG_NEED)[0] == 0
    for shape in ((2, 60, 33), (2, 61, 32)):                                        # (2 nx - 2, .) and (., 2 ny - 2)
        c['psf'] = cc.memo(('hog_psf_small', shape), lambda: np.ones(shape))
        rc, gm, gIR, gk, _ = hog_call(c, F32, 16)
        assert rc == _lib.PFB_ERR_UNSUPPORTED and b'must cover' in lib.pfb_last_error() and gk == -7 and not gm.any()
    c = cc.hog_exact(7, 5, nband=65)                                                # every buffer holds 65 bands
    assert hog_call(c, F64, 16)[0] == _lib.PFB_ERR_INVALID
    assert hog_call(cc.hog_exact(7, 5), F64, 16, nband=0)[0] == _lib.PFB_ERR_INVALID


@pytest.mark.parametrize('dtype', DTYPES)
def test_hogbom_wrapper(dtype):
    """deconv.hogbom.hogbom on 2 x 37 x 22: numpy in, numpy out; tensors in, tensor out; status and values the oracle's."""
    from pfb_clean_amd.deconv.hogbom import hogbom
    c = cc.hog_smooth(dtype, **cc.HOG_SMOOTH_STOP)
    kw = cc.HOG_STOPS['pf']
    x, status, IR, k, irmax, tr = cc.run_hog(cc.f64(c), 10000, **kw)
    assert_margin(tr, dtype)
    keep = c['ID'].copy()
    m, st = hogbom(c['ID'], c['psf'], gamma=c['gamma'], maxit=10000, verbosity=0, **kw)
    assert isinstance(m, np.ndarray) and m.dtype == dtype and st == status == 0 and np.array_equal(c['ID'], keep)
    close(f'wrapper numpy {dtype.name}', m, x, TOL_HOGBOM[dtype])
    IDt = cuda(c['ID'])
    mt, st = hogbom(IDt, cuda(c['psf']), gamma=c['gamma'], maxit=10000, verbosity=0, **kw)
    assert isinstance(mt, torch.Tensor) and mt.is_cuda and mt.dtype == IDt.dtype and st == 0
    assert np.array_equal(mt.cpu().numpy(), m) and np.array_equal(IDt.cpu().numpy(), keep)      # the input is not cleaned
    m, st = hogbom(c['ID'], c['psf'], gamma=c['gamma'], pf=kw['pf'], maxit=k, verbosity=0)
    assert st == 1                                                                  # k >= maxit, as the reference counts
    close(f'wrapper maxit = k {dtype.name}', m, x, TOL_HOGBOM[dtype])


@pytest.mark.parametrize('dtype', DTYPES)
def test_hogbom_nan_stops_the_loop(dtype):
    """A NaN in the cube: the reference's peak is NaN, `NaN > tol` is false, no component is taken."""
    base = cc.hog_exact(31, 17)
    for flat in (0, 300, 526):                      # workgroup 0, workgroup 1, the last pixel
        c = dict(base)
        c['ID'] = base['ID'].copy()
        c['ID'][flat % 2, flat // 17, flat % 17] = np.nan
        x, status, IR, k, irmax, _ = cc.run_hog(c, 16)
        rc, gm, gIR, gk, girmax = hog_call(c, dtype, 16)
        assert rc == 0 and gk == k == 0 and np.isnan(irmax) and np.isnan(girmax), (flat, gk, girmax)
        assert not gm.any() and np.array_equal(gIR, c['ID'], equal_nan=True)
    c = dict(cc.hog_exact(**cc.HOG_BIG_CASES['both']))      # the NaN on a thread's second trip, behind every maximum
    c['ID'] = c['ID'].copy()
    c['ID'][0, -1, -3] = np.nan
    rc, gm, gIR, gk, girmax = hog_call(c, dtype, 16, pf=0.1)
    assert rc == 0 and gk == 0 and np.isnan(girmax) and not gm.any() and np.array_equal(gIR, c['ID'], equal_nan=True)


# ------------------------------------------------------------------------------------------------ clark(...)
@pytest.mark.parametrize('dtype', DTYPES)
def test_clark_full_minor_cycle(dtype):
    """deconv.clark.clark on 3 x 48 x 40 with a 96 x 80 PSF, four major iterations, against oracle.clark.clark: the outer
    peak, the membership of every active set and every sub-minor step keep the margin."""
    from pfb_clean_amd.deconv.clark import clark
    c = cc.clark_full(dtype)
    r = cc.f64(c)
    model, status, k, tr, member = cc.clark_traced(r['ID'], r['psf'], r['psfhat'], r['wsums'], **cc.CLARK_KW)
    assert_margin(tr, dtype, member)
    d = cc.as_dtype(c, dtype)
    m, st = clark(d['ID'], d['psf'], d['psfhat'], d['wsums'], verbosity=0, **cc.CLARK_KW)
    assert isinstance(m, np.ndarray) and m.dtype == dtype and st == status
    assert np.array_equal(m != 0, model != 0)
    close(f'clark {dtype.name}', m, model, TOL_CLARK[dtype])


# ------------------------------------------------------------------------------------------------ pfb_freqmul
def freqmul_call(dtype, A, x, pre, post, nband=None):
    """pfb_freqmul with `out` pre-filled and a guard band behind it.  Returns (rc, out, guard intact)."""
    from pfb_clean_amd import _lib, _dev
    lib = _lib.load()
    nb, npix = x.shape
    sentinel = -777.25
    Ad, xd = cuda(A), cuda(x)
    pd, qd = (None if pre is None else cuda(pre)), (None if post is None else cuda(post))
    buf = torch.full((nb * npix + cc.FM_GUARD,), sentinel, dtype=xd.dtype, device='cuda')
    rc = lib.pfb_freqmul(_dev.code(xd.dtype), _dev.ptr(Ad), _dev.ptr(xd), _dev.ptr(buf), nb if nband is None else nband,
                         npix, _dev.ptr(pd), _dev.ptr(qd), _dev.stream())
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    return rc, host[:nb * npix].reshape(nb, npix), bool(np.all(host[nb * npix:] == sentinel))


def check_freqmul(dtype, nband, npix):
    A, x, pre, post = cc.freqmul_case(dtype, nband, npix)
    worst = 0.0
    for p, q in ((None, None), (pre, None), (None, post), (pre, post)):
        ref, mag = cc.freqmul_ref(A, x, p, q)
        rc, out, guard = freqmul_call(dtype, A, x, p, q)
        assert rc == 0 and guard and out.dtype == dtype
        ratio = float((np.abs(out.astype(np.float64) - ref) / (EPS[dtype] * mag)).max())
        worst = max(worst, ratio)
        assert ratio <= nband + 3, (nband, npix, p is not None, q is not None, ratio)
    print(f'freqmul {dtype.name} nband {nband} npix {npix}: worst error {worst:.2f} eps sum|A||x||pre||post| '
          f'(bound {nband + 3})')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('nband', cc.FM_NBAND)
def test_freqmul(nband, dtype):
    """npix 1, 255, 256, 257 (one lane, a workgroup less one, full, plus one); nband 64 keeps 64 values per thread and
    32 KiB (float64) of LDS; pre / post absent and present."""
    for npix in cc.FM_NPIX:
        check_freqmul(dtype, nband, npix)


@pytest.mark.parametrize('dtype', DTYPES)
def test_freqmul_capped_grid(dtype):
    """1 048 576 + 257 pixels ask for 4098 workgroups; 4096 run and 513 threads take a second trip."""
    check_freqmul(dtype, 2, cc.FM_NPIX_BIG)


def test_freqmul_rejects():
    from pfb_clean_amd import _lib
    A, x, pre, post = cc.freqmul_case(np.float64, 65, 3)                            # every buffer holds 65 bands
    rc, out, guard = freqmul_call(F64, A, x, pre, post)
    assert rc == _lib.PFB_ERR_UNSUPPORTED and guard and np.all(out == -777.25)      # nothing written
    assert freqmul_call(F64, A, x, None, None, nband=0)[0] == _lib.PFB_ERR_UNSUPPORTED


def test_freqmul_wrapper_on_a_non_square_cube():
    from pfb_clean_amd.utils.misc import freqmul
    A, x, _, _ = cc.freqmul_case(np.float64, 5, 7 * 33)
    ref, mag = cc.freqmul_ref(A, x, None, None)
    got = freqmul(A, x.reshape(5, 7, 33))
    assert isinstance(got, np.ndarray) and got.shape == (5, 7, 33)
    assert np.all(np.abs(got.reshape(5, -1) - ref) <= 8 * EPS[F64] * mag)
