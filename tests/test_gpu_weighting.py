"""
The imaging weights on the MI355X (pfb_clean_amd.utils.weighting, csrc/imweight.hip) against the reference's own outputs
stored in tests/golden/weighting.npz (tests/weighting_cases.py; test_cpu_weighting_cases.py shows that every stored case
keeps the reference inside its arrays).

Bounds -- derived, not tuned (weighting_cases.counts_bound / briggs_bound / l2_bound / wsum_bound)
  counts, k = 0     exactly the reference's, per partial grid, both types: they are integers.
  counts, k > 0     per cell |got - ref| <= (n_cell + 128 [k / 6 at k = 12]) u(T) ref: n_cell positive terms in any
                    order, and phi -- two exponentials of arguments up to 13.8 k / 6, four roundings each.  The case
                    `hot` has n_cell = 4096 under contention.
  weights           uniform: exactly equal.  Briggs: relative (4 (16 + ceil(log2(nx ny))) + 8) u(T) per visibility (two
                    positive-term sums on both sides and the closing arithmetic).  An empty cell looked up gives exactly
                    0 under uniform weighting and exactly 1 under Briggs, as in the reference (it replaces the counts by
                    1 + counts ssq before the lookup); all-zero counts give zeros.
  filter            exactly equal: a median and a max.
  l2 reweight       wgt relative (32 + ceil(log2(nvis))) u(T) against the numpy statement; sum mask == 0 gives None;
                    residual_vis exactly; the fused sum within 2 (16 + ceil(log2(nvis))) u(T) of wgt[mask].sum().
"""
import ctypes as C

import numpy as np
import pytest
import torch

import weighting_cases as wcs
from weighting_cases import COUNT_RUNS, COUNT_RUN_IDS, WEIGHT_CASES, FILTER_CASES, L2_CASES, DTYPES, U

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def geometry(case):
    return case['nx'], case['ny'], case['cell'][0], case['cell'][1]


def gpu_counts(case, k, ngrid, dtype):
    from pfb_clean_amd.utils.weighting import _compute_counts
    return _compute_counts(case['uvw'], case['freq'], case['mask'], *geometry(case), dtype, k=k, ngrid=ngrid)


@pytest.mark.parametrize('run', COUNT_RUNS, ids=COUNT_RUN_IDS)
def test_counts_against_the_reference(run):
    case, r, k, ngrid, tag = run
    ref = case['ref'][(r, tag)]
    got = gpu_counts(case, k, ngrid, DTYPES[tag])
    assert isinstance(got, np.ndarray) and got.dtype == ref.dtype and got.shape == ref.shape
    if k == 0:
        assert np.array_equal(got, ref)
        return
    _, n_cell = wcs.np_counts(case, k, ngrid, DTYPES[tag])
    err = np.abs(got.astype(np.float64) - ref)
    bound = wcs.counts_bound(ref.astype(np.float64), n_cell, k, tag)
    worst = (err / np.where(bound > 0, bound, 1.0)).max()
    print(f"{COUNT_RUN_IDS[COUNT_RUNS.index(run)]}: worst |got - ref| / bound {worst:.3f}, n_cell up to {n_cell.max()}")
    assert (err <= bound).all()
    assert not got[ref == 0].any()


def test_compute_counts_sums_the_partial_grids_on_the_device():
    from pfb_clean_amd.utils.weighting import compute_counts, _compute_counts
    case = wcs.case_named('r300x3')
    args = (dev(case['uvw']), dev(case['freq']), dev(case['mask']), *geometry(case))
    got = compute_counts(*args, torch.float64, k=0, ngrid=7)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float64
    assert np.array_equal(got.cpu().numpy(), case['ref'][(0, 'f64')].sum(axis=0))
    part = _compute_counts(*args, np.float32, k=6, ngrid=7)
    assert part.is_cuda and part.dtype == torch.float32 and tuple(part.shape) == (7, case['nx'], case['ny'])
    # a bool mask is the same mask
    again = _compute_counts(args[0], args[1], dev(case['mask'] != 0), *geometry(case), 'float64', k=0, ngrid=7)
    assert np.array_equal(again.cpu().numpy(), case['ref'][(0, 'f64')])


def test_visibilities_and_footprints_outside_the_grid_are_dropped():
    """The one defined difference: the reference wraps / writes past the array, here the contribution is dropped."""
    from pfb_clean_amd.utils.weighting import _counts_to_weights
    base = wcs.case_named('r85x3')
    case = dict(base, uvw=base['uvw'] * np.array([3.0, 3.0, 1.0]))         # three times as far from the centre
    ug, vg = wcs.grid_coords(case)
    outside = (ug < 0) | (ug >= case['nx']) | (vg < 0) | (vg >= case['ny'])
    assert 0.2 < outside.mean() < 0.9
    for k in (0, 6, 12):
        exp, n_cell = wcs.np_counts(case, k, 2, np.float64, clip=True)
        got = gpu_counts(case, k, 2, np.float64)
        assert n_cell.sum() < np.count_nonzero(case['mask']) * max(k, 1) ** 2
        if k == 0:
            assert np.array_equal(got, exp)
        else:
            assert (np.abs(got - exp) <= wcs.counts_bound(exp, n_cell, k, 'f64')).all() and not got[exp == 0].any()
    counts = wcs.np_counts(case, 0, 1, np.float64, clip=True)[0][0]
    for robust in (-3, 0):
        got = _counts_to_weights(counts, case['uvw'], case['freq'], *geometry(case), robust)
        exp = wcs.np_weights(counts, case, robust, clip=True)
        assert not got[outside].any()
        assert (np.abs(got - exp) <= wcs.briggs_bound(case['nx'], case['ny'], 'f64') * exp).all()
    nan = dict(case, uvw=case['uvw'].copy())
    nan['uvw'][::5, 0] = np.nan
    nan['uvw'][1::5, 1] = np.inf
    got = gpu_counts(nan, 6, 1, np.float32)
    assert np.isfinite(got).all()


@pytest.mark.parametrize('w', WEIGHT_CASES, ids=[w['name'] for w in WEIGHT_CASES])
def test_weights_from_the_stored_counts(w):
    from pfb_clean_amd.utils.weighting import _counts_to_weights, counts_to_weights
    case = w['case']
    ug, vg = wcs.grid_coords(case)
    for tag in DTYPES:
        counts = w['counts'][tag]
        empty = counts[np.floor(ug).astype(int), np.floor(vg).astype(int)] == 0
        for q, robust in enumerate(w['robust']):
            ref = w['ref'][(q, tag)]
            got = _counts_to_weights(counts, case['uvw'], case['freq'], *geometry(case), robust)
            assert isinstance(got, np.ndarray) and got.dtype == ref.dtype and got.shape == ref.shape
            if robust <= -2 or w['zero']:
                assert np.array_equal(got, ref)
                assert not got[empty].any()
            else:
                rel = np.abs(got.astype(np.float64) - ref) / ref
                print(f"{w['name']} {tag} robust {robust}: worst relative error {rel.max() / U[tag]:.2f} u")
                assert (rel <= wcs.briggs_bound(case['nx'], case['ny'], tag)).all()
                assert (got[empty] == 1).all()
    got_t = counts_to_weights(dev(w['counts']['f32']), dev(case['uvw']), dev(case['freq']), *geometry(case), -3)
    assert got_t.is_cuda and np.array_equal(got_t.cpu().numpy(), w['ref'][(0, 'f32')])


@pytest.mark.parametrize('f', FILTER_CASES, ids=[f['name'] for f in FILTER_CASES])
def test_filter_extreme_counts(f):
    from pfb_clean_amd.utils.weighting import _filter_extreme_counts, filter_extreme_counts
    for tag in DTYPES:
        counts = f['counts'][tag]
        keep = counts.copy()
        got = _filter_extreme_counts(counts, level=f['level'])
        assert isinstance(got, np.ndarray) and got.dtype == counts.dtype and np.array_equal(got, f['ref'][tag])
        assert np.array_equal(counts, keep)                                    # a new array, the input untouched
    t = dev(f['counts']['f64'])
    got_t = filter_extreme_counts(t, nlevel=f['level'])
    assert got_t.is_cuda and got_t.data_ptr() != t.data_ptr() and np.array_equal(got_t.cpu().numpy(), f['ref']['f64'])
    assert np.array_equal(t.cpu().numpy(), f['counts']['f64'])


@pytest.mark.parametrize('l', L2_CASES, ids=[l['name'] for l in L2_CASES])
def test_l2_reweight(l):
    from pfb_clean_amd.utils.weighting import l2_reweight
    nvis = l['vis'].size
    for tag, cdt in (('f32', np.complex64), ('f64', np.complex128)):
        vis, mvis, mask = l['vis'].astype(cdt), l['model_vis'].astype(cdt), l['mask']
        ref_res, ref_w = wcs.np_l2(vis, mvis, mask, l['dof'])
        res, wgt, wsum = l2_reweight(vis, mvis, mask, l['dof'])
        assert res.dtype == cdt and np.array_equal(res, ref_res)
        if ref_w is None:
            assert wgt is None and wsum is None
            continue
        assert wgt.dtype == DTYPES[tag] and wgt.shape == vis.shape and wsum.shape == (1,) and wsum.dtype == DTYPES[tag]
        rel = np.abs(wgt.astype(np.float64) - ref_w) / ref_w
        print(f"{l['name']} {tag}: wgt worst relative error {rel.max() / U[tag]:.2f} u")
        assert (rel <= wcs.l2_bound(nvis, tag)).all()
        exact = wgt.astype(np.float64)[mask != 0].sum()
        assert abs(float(wsum[0]) - exact) <= wcs.wsum_bound(nvis, tag) * exact
        # imaging weights ride in the same kernel: one more rounded product
        imwgt = np.random.default_rng(3).uniform(0.1, 1.0, vis.shape).astype(DTYPES[tag])
        _, wgt2, wsum2 = l2_reweight(vis, mvis, mask, l['dof'], imwgt)
        assert np.array_equal(wgt2, wgt * imwgt)
        exact2 = wgt2.astype(np.float64)[mask != 0].sum()
        assert abs(float(wsum2[0]) - exact2) <= wcs.wsum_bound(nvis, tag) * exact2
        # no dof: the residual alone, nothing read back
        res0, wgt0, wsum0 = l2_reweight(dev(vis), dev(mvis), dev(mask), None)
        assert res0.is_cuda and wgt0 is None and wsum0 is None and np.array_equal(res0.cpu().numpy(), ref_res)


def test_masked_sum():
    from pfb_clean_amd.utils.weighting import masked_sum
    rng = np.random.default_rng(11)
    for n in (1, 255, 256, 257, 70001):
        for tag, dt in DTYPES.items():
            wgt = rng.uniform(0.0, 2.0, n).astype(dt)
            mask = (rng.uniform(size=n) < 0.8).astype(np.uint8)
            got = masked_sum(dev(wgt), dev(mask))
            assert got.is_cuda and tuple(got.shape) == (1,) and got.dtype == (torch.float32 if tag == 'f32' else torch.float64)
            exact = wgt.astype(np.float64)[mask != 0].sum()
            assert abs(float(got[0]) - exact) <= wcs.wsum_bound(max(n, 2), tag) * exact
    assert float(masked_sum(dev(np.ones(300)), dev(np.zeros(300, np.uint8)))[0]) == 0.0


def test_refusals():
    from pfb_clean_amd.utils import weighting
    from pfb_clean_amd import _lib
    case = wcs.case_named('r85x3')
    args = (case['uvw'], case['freq'], case['mask'], *geometry(case))
    for k in (-2, 1, 3, 7, 18, 6.5):
        with pytest.raises(ValueError):
            weighting._compute_counts(*args, np.float64, k=k)
    for dtype in (np.float16, np.int32, np.complex64, torch.float16, 'int8'):
        with pytest.raises(ValueError):
            weighting._compute_counts(*args, dtype)
    with pytest.raises(ValueError):
        weighting._compute_counts(*args, np.float64, ngrid=0)
    with pytest.raises(ValueError):
        weighting._compute_counts(case['uvw'], case['freq'], case['mask'][:, :2], *geometry(case), np.float64)
    with pytest.raises(TypeError):
        weighting._compute_counts(case['uvw'].astype(np.float32), case['freq'], case['mask'], *geometry(case), np.float64)
    with pytest.raises(ValueError):
        weighting._counts_to_weights(np.zeros((5, 5)), case['uvw'], case['freq'], *geometry(case), 0)
    # the C ABI itself: refused before any launch, the pointers real all the same
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    INV = _lib.PFB_ERR_INVALID
    f64 = torch.zeros(64, dtype=torch.float64, device='cuda')
    u8 = torch.ones(16, dtype=torch.uint8, device='cuda')
    p, m = f64.data_ptr(), u8.data_ptr()
    good = [_lib.PFB_F64, p, p, m, 2, 2, 4, 4, 1.0, 2.5, 1.0, 2.5, 6, 1, p]
    assert lib.pfb_imw_counts(*good, stream) == _lib.PFB_OK

    def changed(**at):
        out = list(good)
        for key, v in at.items():
            out[int(key[1:])] = v
        return out
    for bad in (changed(a0=2), changed(a1=None), changed(a3=None), changed(a14=None), changed(a12=5), changed(a12=18),
                changed(a13=0), changed(a8=0.0), changed(a9=float('nan')), changed(a1=p + 4)):
        assert lib.pfb_imw_counts(*bad, stream) == INV
    assert lib.pfb_imw_counts(*changed(a4=0), stream) == _lib.PFB_ERR_UNSUPPORTED
    work = torch.zeros(6144, dtype=torch.float64, device='cuda')            # PFB_IMW_WORK_DOUBLES
    ws = work.data_ptr()
    assert lib.pfb_imw_moments(_lib.PFB_F32, p + 2, 4, p, ws, stream) == INV
    assert lib.pfb_imw_moments(_lib.PFB_F64, p, 4, None, ws, stream) == INV
    assert lib.pfb_imw_moments(_lib.PFB_F64, p, 4, p, None, stream) == INV
    assert lib.pfb_imw_wsum(_lib.PFB_F64, p, None, 4, p, ws, stream) == INV
    assert lib.pfb_imw_l2_weights(_lib.PFB_F64, p, m, None, 4, float('inf'), p, p, ws, stream) == INV
    assert lib.pfb_imw_l2_residual(_lib.PFB_F64, p + 8, p, m, 4, p, p, ws, stream) == INV
    torch.cuda.synchronize()
