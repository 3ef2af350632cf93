"""
The channel averaging's oracle, case table and bounds (tests/chanavg_cases.py) on the CPU: the oracle on hand-written
inputs, average_freq, what the table must contain, and a simulated fp32 evaluation of the statement against the bounds.
"""
import numpy as np
import pytest

import chanavg_cases as ca
import stokes_cases as sc

CASES = ca.all_cases()


def hand(vis, wgt, mask, n, live=None):
    vis, wgt, mask = np.asarray(vis, complex), np.asarray(wgt, float), np.asarray(mask, np.uint8)
    return ca.average(vis, wgt, mask, mask != 0 if live is None else np.asarray(live, bool), n)


# ----------------------------------------------------------------------------------------------------- the oracle
def test_one_live_channel_gives_its_visibility():
    vis = [[1 + 2j, np.nan, 3 - 1j, 7j]]
    wgt = [[2.0, np.inf, 0.5, 4.0]]
    vo, wo, mo = hand(vis, wgt, [[1, 0, 0, 1]], 2)
    assert vo.tolist() == [[1 + 2j, 7j]] and wo.tolist() == [[2.0, 4.0]] and mo.tolist() == [[1, 1]]


def test_weighted_mean_and_short_last_bin():
    vo, wo, mo = hand([[1.0, 3.0, 5.0, 2j, 4j]], [[1.0, 3.0, 4.0, 1.0, 3.0]], [[1, 1, 1, 1, 1]], 3)
    assert wo.tolist() == [[8.0, 4.0]] and mo.tolist() == [[1, 1]]
    assert vo[0, 0] == (1 + 9 + 20) / 8 and vo[0, 1] == (2j + 12j) / 4


def test_fully_flagged_bin_is_zero_whatever_it_holds():
    vo, wo, mo = hand([[np.nan, np.inf, 1.0, 2.0]], [[np.nan, 1.0, 1.0, 1.0]], [[0, 0, 1, 1]], 2)
    assert vo.tolist() == [[0, 1.5]] and wo.tolist() == [[0, 2.0]] and mo.tolist() == [[0, 1]]


def test_unflagged_but_uncovered_bin():
    """mask 1, not live: vis = wgt = 0 and mask stays 1."""
    vo, wo, mo = hand([[5.0, 6.0]], [[1.0, 1.0]], [[1, 1]], 2, live=[[False, False]])
    assert vo.tolist() == [[0]] and wo.tolist() == [[0]] and mo.tolist() == [[1]]


def test_live_nan_propagates_and_zero_weight_sum_is_zero():
    vo, wo, mo = hand([[np.nan, 1.0, 3.0, 4.0]], [[1.0, 1.0, 1.0, -1.0]], [[1, 1, 1, 1]], 2)
    assert np.isnan(vo[0, 0]) and wo[0, 0] == 2.0
    assert vo[0, 1] == 0 and wo[0, 1] == 0 and mo[0, 1] == 1


def test_n_one_is_the_identity_and_n_past_nchan_is_one_bin():
    rng = np.random.default_rng(3)
    vis = rng.standard_normal((4, 5)) + 1j * rng.standard_normal((4, 5))
    wgt = rng.uniform(0.5, 2, (4, 5))
    mask = (rng.uniform(size=(4, 5)) < 0.7).astype(np.uint8)
    vis, wgt = np.where(mask != 0, vis, 0), np.where(mask != 0, wgt, 0)
    vo, wo, mo = hand(vis, wgt, mask, 1)
    assert np.array_equal(vo, vis) and np.array_equal(wo, wgt) and np.array_equal(mo, mask)
    for n in (5, 6, 1000):
        vo, wo, mo = hand(vis, wgt, mask, n)
        assert vo.shape == wo.shape == mo.shape == (4, 1)
        assert np.allclose(wo[:, 0], wgt.sum(axis=1), rtol=1e-15)
        assert np.allclose(vo[:, 0] * wo[:, 0], (wgt * vis).sum(axis=1), rtol=1e-14)
        assert np.array_equal(mo[:, 0], mask.any(axis=1))


def test_average_freq():
    from pfb_clean_amd.utils.stokes import average_freq
    freq = 1e9 + 1e6 * np.arange(7) ** 2
    width = np.full(7, 1e6) + np.arange(7)
    f, w = average_freq(freq, width, 3)
    assert f.dtype == w.dtype == np.float64 and f.shape == w.shape == (3,)
    assert f.tolist() == [freq[0:3].mean(), freq[3:6].mean(), freq[6]]
    assert w.tolist() == [width[0:3].sum(), width[3:6].sum(), width[6]]
    f, w = average_freq(freq.astype(np.float32), list(width), 1)
    assert np.array_equal(f, freq.astype(np.float32).astype(np.float64)) and np.array_equal(w, width)
    for n in (7, 8, 10 ** 6):
        f, w = average_freq(freq, width, n)
        assert f.tolist() == [freq.mean()] and w.tolist() == [width.sum()]
    for bad in (0, -1, 2.0, None, True):
        with pytest.raises(ValueError):
            average_freq(freq, width, bad)
    with pytest.raises(ValueError):
        average_freq(freq, width[:-1], 2)


# --------------------------------------------------------------------------------------------------- the table
def test_the_table_holds_every_shape_and_run():
    assert [c['shape'] for c in ca.shape_cases()] == ca.SHAPES + ca.EXTRA_SHAPES and len(ca.SHAPES) == 16
    for shape in [(5, 1, 2), (86, 3, 2), (86, 3, 3), (5, 64, 2), (5, 64, 7), (5, 64, 64), (4, 65, 2), (4, 65, 13), (2, 255, 4),
                  (2, 256, 4), (2, 257, 4), (2, 300, 7), (2, 300, 256), (2, 600, 256), (2, 600, 257), (1, 600, 600)]:
        assert shape in ca.SHAPES
    sweep = ca.sweep_cases()
    for shape in [(86, 3, 2), (2, 300, 7)]:
        got = {(c['mode'], sc.BASIS[(c['pol'], c['product'])]) for c in sweep if c['shape'] == shape}
        assert got == {(m, b) for m in ca.ALL_MODES for b in range(4)}
    stack = ca.stack_cases()
    assert {c['product'] for c in stack} == {'IQUV', 'QU'} and len({c['shape'] for c in stack}) == 3
    forms = ca.form_cases()
    assert {c['wform'] for c in forms} == {'none', 'sigma', 'spectrum', 'row'}
    assert {c['op'] for c in forms} == {'none', '+', '-'} and {c['use_frow'] for c in forms} == {True, False}
    assert len({c['name'] for c in CASES}) == len(CASES)
    # past the LDS kernel's largest n, and at it
    assert any(c['n'] > ca.LDS_MAX for c in CASES) and any(c['n'] == ca.LDS_MAX for c in CASES)
    assert any(c['n'] == ca.LANE_MAX for c in CASES) and any(c['n'] == ca.LANE_MAX + 1 for c in CASES)


def test_the_inputs_are_fp32_values():
    for c in ca.shape_cases():
        s = c['set']
        for k in ('data', 'data2', 'weight', 'sigma', 'wrow', 'jones'):
            a = s[k]
            narrow = a.astype(np.complex64 if np.iscomplexobj(a) else np.float32).astype(a.dtype)
            assert np.array_equal(narrow, a, equal_nan=True), (c['name'], k)


def test_every_feature_occurs():
    with np.errstate(all='ignore'):
        seen = {c['name']: ca.features(c) for c in CASES}
    assert set().union(*seen.values()) == set(ca.FEATURES)
    for shape in ca.SWEEP_SHAPES:
        together = set().union(*(seen[c['name']] for c in CASES if c['shape'] == shape))
        assert together == set(ca.FEATURES), (shape, together)
    # with three rows or more one set holds them all
    assert seen[ca.shape_cases()[1]['name']] == set(ca.FEATURES)


# --------------------------------------------------------------------------------------------------- the bounds
@pytest.mark.parametrize('c', CASES, ids=ca.ids(CASES))
def test_simulated_fp32_evaluation_stays_within_the_bounds(c):
    """The oracle's samples rounded to fp32 -- one rounding each, far inside the K of the Stokes pass -- and the
    statement evaluated sequentially in fp32: within the K bounds of the fp64 oracle, and within the K = 0 bounds of
    the fp64 average of the rounded samples.  Elements with a zero bound are exact; NaN reaches no output."""
    o = ca.oracle(c)
    vis, wgt, mask = ca.exact_inputs(c, 'f32')
    t = ca.tight(vis, wgt, np.where(o['live'], 1, 0), c['n'])
    stacked = vis.ndim == 3
    for k in range(vis.shape[0] if stacked else 1):
        pick = (lambda a: a[k]) if stacked else (lambda a: a)
        gv, gw = ca.sequential(pick(vis), pick(wgt), np.where(o['live'], 1, 0), c['n'])
        assert gv.dtype == np.complex64 and gw.dtype == np.float32
        assert np.isfinite(gv).all() and np.isfinite(gw).all()
        loose = (ca.worst(gv, pick(o['vis']), pick(o['vis_unit']), 'f32'), ca.worst(gw, pick(o['wgt']), pick(o['wgt_unit']), 'f32'))
        close = (ca.worst(gv, pick(t['vis']), pick(t['vis_unit']), 'f32'), ca.worst(gw, pick(t['wgt']), pick(t['wgt_unit']), 'f32'))
        assert max(loose) <= 1 and max(close) <= 1, (loose, close)


def test_zero_bounds_occur():
    o = ca.oracle(ca.shape_cases()[1])
    assert (o['wgt_unit'] == 0).any() and (o['vis_unit'] == 0).any() and (o['wgt_unit'] > 0).any()
    assert not o['vis'][o['vis_unit'] == 0].any() and not o['wgt'][o['wgt_unit'] == 0].any()
