"""
The Stokes conversion's case table without a GPU (tests/stokes_cases.py over tests/golden/stokes.npz): the table covers
every instantiation of the kernel and every edge that test_gpu_stokes.py runs, the closed form -- written in numpy in
stokes_cases.closed_form -- reproduces every stored output of the reference within the tests' bound, and stokes_basis
is the table's matrix.
"""
import numpy as np
import pytest

import stokes_cases as sc

SETS, CASES = sc.load()
IDS = [c['name'] for c in CASES]


def test_inputs_are_fp32_values():
    for s in SETS:
        for key in ('data', 'data2', 'jones'):
            if key in s:
                assert np.array_equal(s[key].astype(np.complex64).astype(np.complex128), s[key])
        for key in ('weight', 'sigma', 'wrow'):
            if key in s:
                assert np.array_equal(s[key].astype(np.float32).astype(np.float64), s[key])


def test_the_table_covers_every_instantiation():
    """5 Jones modes x 4 basis matrices (both types run every case); all 24 variants of weight_data at 85 x 3."""
    seen = {(c['mode'], sc.BASIS[(c['pol'], c['product'])]) for c in CASES}
    assert seen == {(m, b) for m in sc.MODES + ('noj4', 'noj2') for b in range(4)}
    sweep = {(c['mode'], c['pol'], c['product']) for c in sc.cases_of('wd', 'sweep-')}
    assert sweep == {(m, *v) for m in sc.MODES for v in sc.VARIANTS}
    assert all(c['set']['data'].shape[:2] == sc.SWEEP_SHAPE for c in sc.cases_of('wd', 'sweep-'))
    for mode in ('noj4', 'noj2'):
        assert {(c['pol'], c['product']) for c in sc.cases_of('sv', f'noj-{mode}-')} == set(sc.VARIANTS)


def test_the_table_covers_every_shape_edge():
    shapes = {}
    for c in sc.cases_of('wd', 'shape-'):
        shapes.setdefault(c['set']['data'].shape[:2], set()).add(c['mode'])
    assert set(shapes) == set(sc.SHAPES) and all(m == set(sc.MODES) for m in shapes.values())
    assert {n for _, n in sc.SHAPES} >= {1, 3, 64, 65}
    for nchan in (1, 3, 64, 65):
        rows = {r for r, n in sc.SHAPES + [sc.SWEEP_SHAPE] if n == nchan}
        per = sc.rows_per_group(nchan)
        assert 1 in rows
        assert any(r % per == per - 1 for r in rows) and any(r % per == 1 and r > per for r in rows)
    assert any(n > sc.BLOCK for _, n in sc.SHAPES)                  # a row that one workgroup strides over


def test_the_table_covers_every_time_bin_edge():
    def bins(name):
        s = sc.case_named(name)['set']
        return s['tbin_idx'], s['tbin_counts'], s['data'].shape[0]
    idx, counts, nrow = bins('tbin-one')
    assert idx.size == 1 and counts[0] == nrow
    idx, counts, nrow = bins('tbin-empty')
    assert 0 in counts[1:-1] and (sc.row_bins(nrow, idx, counts) >= 0).all()
    idx, counts, nrow = bins('tbin-gaps')
    covered = sc.row_bins(nrow, idx, counts) >= 0
    assert not covered[0] and not covered[-1] and covered.any()
    idx, counts, nrow = bins('tbin-offset')
    assert idx.min() > 0 and (sc.row_bins(nrow, idx, counts) >= 0).all()


def test_the_table_covers_every_form_of_stokes_vis():
    sv = sc.cases_of('sv')
    assert {c['wform'] for c in sv} == {'none', 'sigma', 'spectrum', 'row'}
    assert {c['op'] for c in sv} == {'none', '+', '-'}
    assert {(c['use_flag'], c['use_frow']) for c in sv} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {c['mode'] for c in sv} == {'noj4', 'noj2', 'diag4', 'diag2', 'full4'}
    s = sv[0]['set']
    assert all(c['set'] is s for c in sv) and s['layout'] == 'qcal' and s['data'].shape[:2] == sc.COMPOSE_SHAPE
    assert (s['ant1'] == s['ant2']).any() and s['jones'].shape[3] > 1
    assert all(c['set']['flag'].any() and not c['set']['flag'].all() for c in CASES if c['set']['flag'].size > 3)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_the_closed_form_reproduces_the_reference(case):
    vis, wgt, mask, vis_unit, wgt_unit = sc.closed_form(case)
    assert case['ref_vis'].dtype == np.complex128 and case['ref_wgt'].dtype == np.float64
    ev, ew = sc.worst(vis, wgt, case['ref_vis'], case['ref_wgt'], vis_unit, wgt_unit, 'f64')
    assert ev <= sc.K and ew <= sc.K, (ev, ew)
    if case['kind'] == 'sv':
        assert np.array_equal(mask, case['ref_mask'])
    # zeros where flagged or uncovered, exactly
    dead = (mask == 0) | (sc.row_bins(mask.shape[0], case['set']['tbin_idx'], case['set']['tbin_counts']) < 0)[:, None]
    assert not case['ref_vis'][dead].any() and not case['ref_wgt'][dead].any()
    if sc.ncorr(case['mode']) == 2 and sc.BASIS[(case['pol'], case['product'])] >= 2:
        assert not case['ref_vis'].any() and case['ref_wgt'][~dead].all()       # vis = 0 with a non-zero wgt


def test_stokes_basis_is_the_table():
    from pfb_clean_amd.utils.stokes import stokes_basis
    table = {('linear', 'I'): [[1, 0], [0, 1]], ('circular', 'I'): [[1, 0], [0, 1]],
             ('linear', 'Q'): [[1, 0], [0, -1]], ('circular', 'V'): [[1, 0], [0, -1]],
             ('linear', 'U'): [[0, 1], [1, 0]], ('circular', 'Q'): [[0, 1], [1, 0]],
             ('linear', 'V'): [[0, 1j], [-1j, 0]], ('circular', 'U'): [[0, 1j], [-1j, 0]]}
    for (pol, product), want in table.items():
        got = stokes_basis(pol, product)
        assert got.shape == (2, 2) and np.array_equal(got, np.array(want, complex))
        assert np.array_equal(got, sc.MATRICES[sc.BASIS[(pol, product)]])
    for bad in (('linear', 'X'), ('elliptic', 'I')):
        with pytest.raises(ValueError):
            stokes_basis(*bad)
