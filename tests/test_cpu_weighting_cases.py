"""
The imaging weights' case table on the CPU (no GPU): it is well formed, every stored case keeps the reference inside
its arrays, and the plain-numpy statement of tests/weighting_cases.py reproduces the stored reference outputs -- exactly
where the arithmetic is exact (k = 0 counts, uniform weights, the filter), within the bounds of the GPU tests elsewhere.
"""
import os
import re

import numpy as np
import pytest

import weighting_cases as wcs
from weighting_cases import COUNT_CASES, COUNT_RUNS, COUNT_RUN_IDS, WEIGHT_CASES, FILTER_CASES, L2_CASES, DTYPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_table_covers_what_it_is_there_for():
    assert {(c['nx'], c['ny']) for c in COUNT_CASES} == wcs.GRIDS
    shapes = {c['mask'].shape for c in COUNT_CASES}
    assert wcs.VIS_COUNTS <= shapes
    nvis = {r * c for r, c in shapes}
    assert {wcs.BLOCK - 1, wcs.BLOCK, wcs.BLOCK + 1} <= nvis                   # 85x3, 64x4, 257x1 straddle the block
    assert {n for c in COUNT_CASES for _, n in c['runs']} == wcs.NGRIDS
    assert {k for c in COUNT_CASES for k, _ in c['runs']} == wcs.SUPPORTS
    assert any(n > c['uvw'].shape[0] for c in COUNT_CASES for _, n in c['runs'])          # empty bins
    dens = [c['mask'].mean() for c in COUNT_CASES]
    assert 0.0 in dens and any(0.7 < d < 0.9 for d in dens) and 1.0 in dens
    for c in COUNT_CASES:
        assert c['uvw'].dtype == np.float64 and c['freq'].dtype == np.float64 and c['mask'].dtype == np.uint8
        assert c['uvw'].shape == (c['mask'].shape[0], 3) and c['freq'].shape == (c['mask'].shape[1],)
        for r, (k, n) in enumerate(c['runs']):
            for tag, dt in DTYPES.items():
                assert c['ref'][(r, tag)].dtype == dt and c['ref'][(r, tag)].shape == (n, c['nx'], c['ny'])
    assert {q for w in WEIGHT_CASES for q in w['robust']} == set(wcs.ROBUST)
    assert any(w['zero'] for w in WEIGHT_CASES)
    assert any(not l['mask'].any() for l in L2_CASES)


def test_edge_tie_and_hot_cases_are_what_they_claim():
    for k in sorted(wcs.SUPPORTS):
        c = wcs.case_named(f'edge-k{k}')
        assert wcs.cell_ranges(c, k) == (0, c['nx'] - 1, 0, c['ny'] - 1)
    ties = wcs.case_named('ties')
    assert ties['freq'][0] == wcs.C_LIGHT
    ug, vg = wcs.grid_coords(ties)
    for g in (ug, vg):
        frac = g - np.floor(g)
        assert set(np.unique(frac)) == {0.0, 0.5}
        half = g[frac == 0.5]
        assert (np.floor(half) % 2 == 0).any() and (np.floor(half) % 2 == 1).any()        # ties that round down and up
    hot = wcs.case_named('hot')
    ref = hot['ref'][(0, 'f64')]
    assert ref.max() == 4096 and np.count_nonzero(ref) == 1
    one = wcs.case_named('one')
    assert wcs.cell_ranges(one, 12)[2:] == (0, one['ny'] - 1)


@pytest.mark.parametrize('case', COUNT_CASES, ids=[c['name'] for c in COUNT_CASES])
def test_reference_stays_inside_the_grid(case):
    for k in {k for k, _ in case['runs']}:
        rng = wcs.cell_ranges(case, k)
        if rng is not None:
            assert 0 <= rng[0] and rng[1] <= case['nx'] - 1 and 0 <= rng[2] and rng[3] <= case['ny'] - 1
    ug, vg = wcs.grid_coords(case)                  # the weights look every visibility up, masked or not
    assert 0 <= np.floor(ug).min() and np.floor(ug).max() <= case['nx'] - 1
    assert 0 <= np.floor(vg).min() and np.floor(vg).max() <= case['ny'] - 1


@pytest.mark.parametrize('run', COUNT_RUNS, ids=COUNT_RUN_IDS)
def test_statement_reproduces_the_counts(run):
    case, r, k, ngrid, tag = run
    ref = case['ref'][(r, tag)]
    got, n_cell = wcs.np_counts(case, k, ngrid, DTYPES[tag])
    assert got.dtype == ref.dtype
    assert np.array_equal(n_cell > 0, ref > 0)
    if k == 0:
        assert np.array_equal(got, ref) and np.array_equal(n_cell, ref)
    else:
        assert (np.abs(got.astype(np.float64) - ref) <= wcs.counts_bound(ref.astype(np.float64), n_cell, k, tag)).all()
    assert n_cell.sum() == np.count_nonzero(case['mask']) * max(k, 1) ** 2


@pytest.mark.parametrize('w', WEIGHT_CASES, ids=[w['name'] for w in WEIGHT_CASES])
def test_statement_reproduces_the_weights(w):
    case = w['case']
    for tag in DTYPES:
        for q, robust in enumerate(w['robust']):
            ref = w['ref'][(q, tag)]
            got = wcs.np_weights(w['counts'][tag], case, robust)
            assert got.dtype == ref.dtype and got.shape == ref.shape
            if robust <= -2 or w['zero']:
                assert np.array_equal(got, ref)
            else:
                assert (np.abs(got.astype(np.float64) - ref) <= wcs.briggs_bound(case['nx'], case['ny'], tag) * ref).all()
            if w['zero']:
                assert not ref.any()
    # an empty cell looked up: 0 under uniform weighting, 1 under Briggs (the counts are replaced before the lookup)
    if w['name'] == 'r85x3-k0':
        ug, vg = wcs.grid_coords(case)
        empty = w['counts']['f64'][np.floor(ug).astype(int), np.floor(vg).astype(int)] == 0
        assert empty.any() and not w['ref'][(0, 'f64')][empty].any() and (w['ref'][(2, 'f64')][empty] == 1).all()


@pytest.mark.parametrize('f', FILTER_CASES, ids=[f['name'] for f in FILTER_CASES])
def test_statement_reproduces_the_filter(f):
    for tag in DTYPES:
        got = wcs.np_filter(f['counts'][tag], f['level'])
        assert got.dtype == f['ref'][tag].dtype and np.array_equal(got, f['ref'][tag])
    assert np.array_equal(f['ref']['f64'] == 0, f['counts']['f64'] == 0)


def test_filter_cases_change_something_and_have_both_parities():
    npos = [int(np.count_nonzero(f['counts']['f64'] > 0)) for f in FILTER_CASES]
    assert {n % 2 for n in npos if n} == {0, 1} and 0 in npos
    assert any(not np.array_equal(f['ref']['f64'], f['counts']['f64']) for f in FILTER_CASES)


def test_declarations_match():
    from pfb_clean_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'pfb_hip.h')).read()
    names = ('pfb_imw_counts', 'pfb_imw_moments', 'pfb_imw_weights', 'pfb_imw_l2_residual', 'pfb_imw_l2_weights',
             'pfb_imw_wsum')
    for name in names:
        assert name in _lib.SIGNATURES and name + '(' in header
    assert int(re.search(r'#define PFB_IMW_RECORD (\d+)', header).group(1)) == 3
    from pfb_clean_amd.utils import weighting
    assert weighting.RECORD == 3
    assert weighting.uv_cells(32, 24, 2.0e-5, 3.1e-5) == wcs.uv_cells(32, 24, 2.0e-5, 3.1e-5)
    from pfb_clean_amd.operators.gridder import image_data_products  # noqa: F401
    makefile = open(os.path.join(ROOT, 'pfb_clean_amd', 'csrc', 'Makefile')).read()
    assert 'imweight.hip' in makefile
