"""
The inputs of tests/test_gpu_clean.py, checked on the CPU (tests/clean_cases.py builds them).

  traced runs    clean_cases repeats the loops of oracle/clark.py to record margins, picks, the active set left over, the
                 Hogbom iteration count and the last peak.  Model, count / status and residual equal the oracle's bit for bit.
  exact cases    the float32 oracle equals the float64 oracle bit for bit, and at least one arg-max that the loop acts on
                 is an exact tie (a one-pixel case cannot tie).
  smooth cases   the float64 run on the dtype-rounded inputs keeps, at every decision, a selection margin
                 (best - second) / best and a stop margin |max - threshold| / threshold of at least 2e-3 (float32 inputs)
                 or 1e-9 (float64 inputs): ten times the value tolerance the GPU test allows.  The figures are printed.
"""
import numpy as np
import pytest

from oracle import clark as ocl
import clean_cases as cc

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
DTYPES = [F32, F64]


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ------------------------------------------------------------------------------------------------- generators
def test_exact_generators():
    rng = np.random.default_rng(0)
    cube = cc.exact_cube(rng, 3, 40, 53)
    assert np.array_equal(cube, np.rint(cube)) and cube.min() == -6 and cube.max() == 6
    psf = cc.exact_psf(rng, 3, 79, 105)
    assert np.all(psf[:, 39, 52] == 1.0) and set(np.unique(psf)) == {-0.5, 0.0, 0.5, 1.0}
    frac = (np.abs(psf) == 0.5).mean()
    assert 0.015 < frac < 0.025
    for nband in (1, 2, 3, 5, 64):
        w = cc.dyadic_wsums(nband)
        assert w.sum() == 1.0 and np.all(np.log2(w) == np.rint(np.log2(w)))
    assert cc.dyadic_wsums(3).tolist() == [0.5, 0.25, 0.25]
    Ip, Iq = cc.active_subset(rng, 40, 53, 2085)
    e = Ip * 53 + Iq
    assert np.all(np.diff(e) > 0) and e.max() < 40 * 53 and Ip.max() < 40 and Iq.max() < 53


def test_smooth_generators():
    psf = cc.smooth_psf(3, 96, 80)
    assert np.all(psf[:, 48, 40] == 1.0) and np.all(psf.max(axis=(1, 2)) == 1.0)
    far = psf[:, :20, :]
    assert 0.001 < np.abs(far).max() < 0.03 and far.min() < 0 < far.max()          # low, oscillating
    widths = [(psf[b] > 0.5).sum() for b in range(3)]
    assert widths[0] < widths[1] < widths[2]
    c = cc.hog_smooth_big(F32)
    assert c['ID'].dtype == F32 and c['ID'].shape == (2,) + cc.HOG_BIG and c['psf'].shape == (2, 1040, 1018)
    assert c['ID'].astype(np.float64).sum(axis=0).reshape(-1)[cc.HOG_THREADS + 1000] > 2.0      # a source past 262 144


# ------------------------------------------------------------------------------------------------- exact cases
@pytest.mark.parametrize('name', list(cc.SUB_EXACT_CASES))
def test_subminor_exact_precondition(name):
    c = cc.sub_exact(**cc.SUB_EXACT_CASES[name])
    runs = {}
    for dt in DTYPES:
        cd = cc.as_dtype(c, dt)
        for maxit in (1, 16):
            model, k, A, tr = cc.run_sub(cd, maxit)
            om, ok = ocl.subminor(cd['A'], cd['psf'], cd['Ip'], cd['Iq'], cd['model0'].copy(), cd['wsums'],
                                  gamma=cd['gamma'], th=cd['th'], maxit=maxit)
            assert model.dtype == dt and A.dtype == dt and same(model, om) and k == ok      # the trace is the oracle
            runs[dt, maxit] = (model, k, A, tr)
    for maxit in (1, 16):
        (m32, k32, A32, _), (m64, k64, A64, tr) = runs[F32, maxit], runs[F64, maxit]
        assert k32 == k64 and np.array_equal(m32, m64) and np.array_equal(A32, A64)
    model, k, A, tr = runs[F64, 16]
    print(f'{name}: nact {c["A"].shape[1]} k {k} ties {tr.ties}')
    assert k == 16 or c['A'].shape[1] == 1
    if c['A'].shape[1] > 1:
        assert tr.tied()


@pytest.mark.parametrize('tie', list(cc.SUB_TIES))
def test_subminor_constructed_ties(tie):
    """The named indices share the first maximum and nothing else does; the lowest of them is taken first."""
    c = cc.sub_exact(**cc.SUB_EXACT_CASES[f'tie_{tie}'])
    idx = cc.SUB_TIES[tie]
    search = c['A'].sum(axis=0) ** 2
    assert sorted(np.flatnonzero(search == search.max()).tolist()) == sorted(idx)
    assert max(idx) < c['A'].shape[1] and len({i % cc.CLT for i in idx}) == len(idx)
    model, k, A, tr = cc.run_sub(c, 1)
    assert k == 1 and tr.pick[0] == min(idx) and tr.ties[0] == len(idx)
    p, q = c['Ip'][min(idx)], c['Iq'][min(idx)]
    assert np.all(model[:, p, q] != 0) and np.count_nonzero(model) == model.shape[0]


def test_subminor_special_cases():
    c = cc.sub_exact(**cc.SUB_EXACT_CASES['accumulate'])
    model, k, A, tr = cc.run_sub(c, 16)
    picks = tr.pick[:k]
    assert len(set(picks)) < len(picks)                                 # a pixel taken more than once
    assert np.any(c['model0'] != 0) and np.any((model != c['model0']) & (c['model0'] != 0))
    c = cc.sub_exact(**cc.SUB_EXACT_CASES['wsum_zero'])
    model, k, A, tr = cc.run_sub(c, 16)
    _, _, A3, _ = cc.run_sub(cc.sub_exact(), 16)
    assert not model[1].any() and model[0].any() and model[2].any() and np.array_equal(A, A3)   # band 1 still subtracted
    c = cc.sub_exact()
    first = float(np.sqrt((c['A'].sum(axis=0) ** 2).max()))
    model, k, A, tr = cc.run_sub(c, 16, th=first + 1.0)
    assert k == 0 and not model.any() and np.array_equal(A, c['A'])
    assert cc.run_sub(c, 0)[1] == 0 and cc.run_sub(cc.sub_exact(nact=1), 16)[1] == 1


def test_nan_cases_stop_the_reference():
    c = cc.sub_nan_case()
    model, k, A, tr = cc.run_sub(c, 16)
    om, ok = ocl.subminor(c['A'], c['psf'], c['Ip'], c['Iq'], c['model0'].copy(), c['wsums'], gamma=0.5, th=2.0, maxit=16)
    assert k == ok == 2 and same(model, om) and np.isnan(A).sum() == 1 and np.isfinite(model).all()
    assert tr.pick[:2] == cc.run_sub(cc.sub_exact(), 16)[3].pick[:2] and tr.pick[2] == int(np.flatnonzero(np.isnan(A[1]))[0])
    c = dict(cc.sub_exact())
    c['A'] = c['A'].copy()
    c['A'][2, 1500 % c['A'].shape[1]] = np.nan
    model, k, A, tr = cc.run_sub(c, 16)
    assert k == 0 and not model.any() and cc.run_sub(cc.sub_exact(), 16)[1] == 16
    h = dict(cc.hog_exact(31, 17))
    h['ID'] = h['ID'].copy()
    h['ID'][1, 300 // 17, 300 % 17] = np.nan
    x, status, IR, k, irmax, tr = cc.run_hog(h, 16)
    ox, ostatus, oIR = ocl.hogbom(h['ID'], h['psf'], threshold=2.0, gamma=1.0, pf=0.0, maxit=16)
    assert k == 0 and status == ostatus == 0 and not x.any() and not ox.any() and np.isnan(irmax) and same(IR, oIR)


@pytest.mark.parametrize('name', list(cc.HOG_EXACT_CASES) + list(cc.HOG_BIG_CASES))
def test_hogbom_exact_precondition(name):
    kw = cc.HOG_EXACT_CASES[name] if name in cc.HOG_EXACT_CASES else cc.HOG_BIG_CASES[name]
    c = cc.hog_exact(**kw)
    runs = {}
    for dt in DTYPES:
        cd = cc.as_dtype(c, dt)
        x, status, IR, k, irmax, tr = cc.run_hog(cd, 16)
        ox, ostatus, oIR = ocl.hogbom(cd['ID'], cd['psf'], threshold=cd['threshold'], gamma=cd['gamma'], pf=cd['pf'],
                                      maxit=16)
        assert x.dtype == dt and same(x, ox) and same(IR, oIR) and status == ostatus
        runs[dt] = (x, status, IR, k, irmax, tr)
    (x32, s32, r32, k32, i32, _), (x64, s64, r64, k64, i64, tr) = runs[F32], runs[F64]
    assert k32 == k64 and s32 == s64 and np.array_equal(x32, x64) and np.array_equal(r32, r64) and float(i32) == float(i64)
    print(f'{name}: k {k64} ties {tr.ties}')
    if kw['nx'] * kw['ny'] > 1:
        assert tr.tied()
    if name in cc.HOG_BIG_CASES:
        tie = kw['tie']
        assert tr.ties[0] == len(tie) and tr.pick[0] == min(tie) and max(tie) >= cc.HOG_THREADS


def test_hogbom_big_tie_geometry():
    """(262144 + 5, 5): one thread's second and first trip.  (300, 262144 + 7): the lower index belongs to workgroup 1,
    the higher one to workgroup 0."""
    a, b = cc.HOG_BIG_TIES['second_pass']
    assert a - b == cc.HOG_THREADS and a < cc.HOG_BIG[0] * cc.HOG_BIG[1]
    lo, hi = cc.HOG_BIG_TIES['across_workgroups']
    assert lo < hi and (lo % cc.HOG_THREADS) // 256 > (hi % cc.HOG_THREADS) // 256
    assert cc.HOG_NEED <= cc.HOG_WORK


# ------------------------------------------------------------------------------------------------- smooth cases
def check_margin(tag, tr, dtype, extra=None):
    m = tr.margin() if extra is None else min(tr.margin(), extra)
    print(f'{tag} {dtype.name}: {len(tr.pick)} searches, least margin {m:.3e} (selection '
          f'{min([s for s, u in zip(tr.sel, tr.used) if u], default=np.inf):.3e}, stop {min(tr.stop):.3e}'
          + (f', membership {extra:.3e})' if extra is not None else ')'))
    assert m >= cc.MARGIN[dtype], (tag, m)


@pytest.mark.parametrize('dtype', DTYPES)
def test_subminor_smooth_margin(dtype):
    c = cc.f64(cc.sub_smooth(dtype))
    maxit = cc.SUB_SMOOTH[dtype]['maxit']
    model, k, A, tr = cc.run_sub(c, maxit)
    om, ok = ocl.subminor(c['A'], c['psf'], c['Ip'], c['Iq'], c['model0'].copy(), c['wsums'], gamma=c['gamma'],
                          th=c['th'], maxit=maxit)
    assert same(model, om) and k == ok and c['A'].shape[1] > cc.CLT and 3 < k < maxit
    assert max(tr.pick[:k]) >= cc.CLT                       # a component from a thread's second trip
    check_margin('sub-minor smooth', tr, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
def test_hogbom_big_smooth_margin(dtype):
    c = cc.f64(cc.hog_smooth_big(dtype))
    maxit = cc.HOG_SMOOTH_BIG[dtype]['maxit']
    x, status, IR, k, irmax, tr = cc.run_hog(c, maxit)
    ox, ostatus, oIR = ocl.hogbom(c['ID'], c['psf'], threshold=0.0, gamma=c['gamma'], pf=0.0, maxit=maxit)
    assert same(x, ox) and same(IR, oIR) and status == ostatus == 1 and k == maxit
    assert any(p >= cc.HOG_THREADS for p in tr.pick[:k]) and any(p < cc.HOG_THREADS for p in tr.pick[:k])
    check_margin('hogbom 520 x 509', tr, dtype)


@pytest.mark.parametrize('maxit', cc.HOG_BATCH_MAXIT)
def test_hogbom_batch_margin(maxit):
    c = cc.hog_smooth(F64, **cc.HOG_SMOOTH_SMALL)
    x, status, IR, k, irmax, tr = cc.run_hog(c, maxit)
    ox, ostatus, oIR = ocl.hogbom(c['ID'], c['psf'], threshold=0.0, gamma=c['gamma'], pf=0.0, maxit=maxit)
    assert same(x, ox) and same(IR, oIR) and status == ostatus == 1 and k == maxit
    check_margin(f'hogbom batch maxit {maxit}', tr, F64)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('stop', list(cc.HOG_STOPS))
def test_hogbom_stop_margin(stop, dtype):
    c = cc.f64(cc.hog_smooth(dtype, **cc.HOG_SMOOTH_STOP))
    kw = cc.HOG_STOPS[stop]
    x, status, IR, k, irmax, tr = cc.run_hog(c, 10000, **kw)
    ox, ostatus, oIR = ocl.hogbom(c['ID'], c['psf'], gamma=c['gamma'], maxit=10000, **kw)
    assert same(x, ox) and same(IR, oIR) and status == ostatus == 0 and 5 < k < 64
    check_margin(f'hogbom stop by {stop}', tr, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
def test_clark_full_margin(dtype):
    c = cc.f64(cc.clark_full(dtype))
    model, status, k, tr, member = cc.clark_traced(c['ID'], c['psf'], c['psfhat'], c['wsums'], **cc.CLARK_KW)
    om, ostatus = ocl.clark(c['ID'], c['psf'], c['psfhat'], c['wsums'], **cc.CLARK_KW)
    assert same(model, om) and status == ostatus and 3 <= k <= 5
    check_margin('clark 3 x 48 x 40', tr, dtype, extra=member)


def test_freqmul_reference():
    A, x, pre, post = cc.freqmul_case(np.float32, 5, 257)
    ref, mag = cc.freqmul_ref(A, x, pre, post)
    want = np.einsum('kl,lp->kp', A.astype(np.float64), (x.astype(np.float64) * pre)) * post
    assert ref.dtype == np.float64 and np.array_equal(ref, want) and np.all(mag >= np.abs(ref))
    ref2, mag2 = cc.freqmul_ref(A, x, None, None)
    assert np.array_equal(ref2, np.einsum('kl,lp->kp', A.astype(np.float64), x.astype(np.float64)))
