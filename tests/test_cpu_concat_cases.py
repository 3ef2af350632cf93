"""
The concatenation and beam-resampling case table on the CPU (no GPU): every stored case keeps the reference inside its
own conditions, the table holds what it is there for, and the plain-numpy statement of tests/concat_cases.py reproduces
the stored reference outputs within the bounds of the GPU tests -- the reference alone stays inside them.
"""
import os
import re

import numpy as np
import pytest

import concat_cases as cc
from concat_cases import OVERLAP_CASES, BEAM_SUM_CASES, BEAM_EVAL_CASES, CHAN_IN, CHAN_REF, ROW_IN, ROW_REF, TAGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cases_keep_the_reference_inside_its_conditions():
    for c in OVERLAP_CASES:
        assert len({s['vis'].shape[0] for s in c['src']}) == 1
        for s in c['src']:
            assert set(np.unique(s['mask'])) <= {0, 1} and np.unique(s['freq']).size == s['freq'].size
            assert s['vis'].shape == s['wgt'].shape == s['mask'].shape == (s['vis'].shape[0], s['freq'].size)
    for xds in (CHAN_IN, ROW_IN):
        for ds in xds:
            assert set(np.unique(ds['MASK'])) <= {0, 1}
            assert ds['attrs']['freq_min'] == ds['chan'].min() and ds['attrs']['freq_max'] == ds['chan'].max()
    for nband_out in (2, 3):
        plan = cc.chan_plan(CHAN_IN, nband_out)
        assert len(plan) == 2 * nband_out
        for *_, fb, sel in plan:
            assert sel and fb.size and len({CHAN_IN[k]['VIS'].shape[0] for k in sel}) == 1
    for c in BEAM_EVAL_CASES:
        for g in (c['l_in'], c['m_in']):
            d = np.diff(g)
            assert g.size >= 2 and ((d > 0).all() or (d < 0).all())


def test_table_covers_what_it_is_there_for():
    shapes = {(c['src'][0]['vis'].shape[0], c['ufreq'].size, len(c['src'])) for c in OVERLAP_CASES}
    assert {s[0] for s in shapes} == {1, 3, 257} and {s[1] for s in shapes} == {1, 5, 33} and {s[2] for s in shapes} == {1, 2, 9}
    assert any(r * c > cc.BLOCK for r, c, _ in shapes) and any(n > cc.BATCH for _, _, n in shapes)
    maps = {c['name']: cc.channel_map(c['src'], c['ufreq']) for c in OVERLAP_CASES}
    counts = {name: (m >= 0).sum(axis=0) for name, m in maps.items()}
    assert (counts['disjoint'] == 1).all()                                             # disjoint
    assert set(counts['partial']) == {1, 2}                                            # partly overlapping
    assert (counts['nine-full'] == 9).all()                                            # fully overlapping
    nine = maps['nine-interleaved']
    assert (nine[5] == -1).all()                                                       # a source without a channel
    assert any((np.diff(m[m >= 0]) != 1).any() for m in nine)                          # a non-contiguous map
    assert any((np.diff(m[m >= 0]) < 0).any() for m in nine)                           # and one that runs backwards
    assert (nine[8] >= 0).any()                                                        # the second batch contributes
    for name in ('partial', 'nine-interleaved'):
        viso, wgto, masko = named_ref(name, 'f64')
        assert (masko == 0).all(axis=0).any()                                          # a column flagged in every source
        bad = ~np.isfinite(viso)
        assert bad.any() and (masko[bad] == 1).all() and (wgto[bad] == 0).all()        # unflagged, weights all zero
    sizes = [sorted(w.size for w in c['wgt']) for c in BEAM_SUM_CASES]
    assert {len(s) for s in sizes} == {1, 2, 9}
    big = cc.named(BEAM_SUM_CASES, 'nine')
    assert {1, 129, 70000} <= {w.size for w in big['wgt']}
    assert not any(w.any() for w in cc.named(BEAM_SUM_CASES, 'zero')['wgt'])
    grids = {c['beam'].shape for c in BEAM_EVAL_CASES}
    outs = {c['ref']['f64'].shape for c in BEAM_EVAL_CASES}
    assert grids == {(2, 2), (9, 7)} and outs == {(1, 1), (5, 4), (37, 300)}
    assert {c['l_out'].ndim for c in BEAM_EVAL_CASES} == {1, 2}
    assert any(np.unique(np.round(np.diff(c['l_in']), 12)).size > 1 for c in BEAM_EVAL_CASES)       # non-uniform
    assert any(c['l_in'][0] > c['l_in'][-1] for c in BEAM_EVAL_CASES)                   # descending
    for name in ('9x7-5x4', '9x7-37x300', 'nonuniform-37x300', '2x2-5x4-2d'):
        c = cc.named(BEAM_EVAL_CASES, name)
        for g, x in ((c['l_in'], c['l_out']), (c['m_in'], c['m_out'])):
            assert (x < g.min()).any() and (x > g.max()).any()                         # outside on each side of each axis
            assert (x == g.min()).any() and (x == g.max()).any()                       # the first and the last node
    assert np.isin(cc.named(BEAM_EVAL_CASES, '9x7-37x300')['l_out'], cc.named(BEAM_EVAL_CASES, '9x7-37x300')['l_in'][1:-1]).any()
    # concat_chan: 2 times x 4 bands whose neighbours share their edge channel; concat_row: 3 times x 2 bands
    assert len(CHAN_IN) == 8 and len({ds['attrs']['time_out'] for ds in CHAN_IN}) == 2
    assert all(CHAN_IN[b]['chan'][-1] == CHAN_IN[b + 1]['chan'][0] for b in range(3))
    assert len(ROW_IN) == 6 and len({ds['VIS'].shape[0] for ds in ROW_IN}) == 3
    assert cc.chan_plan(CHAN_IN, 4) is None and cc.chan_plan(CHAN_IN[:1], 3) is None and cc.row_plan(ROW_IN[:2]) is None
    with pytest.raises(ValueError):
        cc.chan_plan(CHAN_IN, cc.NBAND_NONE)


def named_ref(name, tag):
    return cc.named(OVERLAP_CASES, name)['ref'][tag]


@pytest.mark.parametrize('tag', list(TAGS))
@pytest.mark.parametrize('case', OVERLAP_CASES, ids=[c['name'] for c in OVERLAP_CASES])
def test_statement_reproduces_sum_overlap(case, tag):
    src = cc.typed_sources(case['src'], tag)
    cc.check_overlap(cc.np_sum_overlap(src, case['ufreq']), case['ref'][tag], src, case['ufreq'], tag, case['name'])


@pytest.mark.parametrize('case', BEAM_SUM_CASES, ids=[c['name'] for c in BEAM_SUM_CASES])
def test_statement_reproduces_sum_beam(case):
    for wtag, btag in cc.BEAM_TAGS:
        wgts = [w.astype(TAGS[wtag][1]) for w in case['wgt']]
        beams = [b.astype(TAGS[btag][1]) for b in case['beam']]
        for w in wgts:                                  # the reference's own sum of the weights, in their type
            exact = float(w.sum(dtype=np.float64))
            assert abs(float(w.sum()) - exact) <= cc.wsum_bound(w.size, wtag) * exact
        cc.check_beam_sum(cc.np_sum_beam(beams, wgts), case['ref'][(wtag, btag)], beams, wgts, wtag, btag, case['name'])


@pytest.mark.parametrize('case', BEAM_EVAL_CASES, ids=[c['name'] for c in BEAM_EVAL_CASES])
def test_statement_reproduces_eval_beam(case):
    for tag, (_, rdt) in TAGS.items():
        c = dict(case, beam=case['beam'].astype(rdt))
        got = cc.np_eval_beam(c['beam'], c['l_in'], c['m_in'], c['l_out'], c['m_out'])
        cc.check_beam_eval(got, case['ref'][tag], c, label=f"{case['name']} {tag}")


@pytest.mark.parametrize('tag', list(TAGS))
@pytest.mark.parametrize('nband_out', [2, 3])
def test_statement_reproduces_concat_chan(nband_out, tag):
    xds = cc.typed_datasets(CHAN_IN, tag)
    got, ref, plan = cc.np_concat_chan(xds, nband_out), CHAN_REF[(nband_out, tag)], cc.chan_plan(xds, nband_out)
    assert len(got) == len(ref) == len(plan)
    for k, (g, r, p) in enumerate(zip(got, ref, plan)):
        cc.check_chan_dataset(g, r, [xds[i] for i in p[-1]], tag, f'chan{nband_out}[{k}]')
    assert cc.np_concat_chan(xds, 4) is xds and cc.np_concat_chan(xds[:1], 3) is not None


@pytest.mark.parametrize('tag', list(TAGS))
def test_statement_reproduces_concat_row(tag):
    xds = cc.typed_datasets(ROW_IN, tag)
    got, ref, plan = cc.np_concat_row(xds), ROW_REF[tag], cc.row_plan(xds)
    assert len(got) == len(ref) == len(plan) == 2
    for k, (g, r, sel) in enumerate(zip(got, ref, plan)):
        assert g['VIS'].shape[0] == sum(ROW_IN[i]['VIS'].shape[0] for i in sel) == 11
        cc.check_row_dataset(g, r, [xds[i] for i in sel], tag, f'row[{k}]')
        assert r['attrs']['timeid'] == 0 and r['attrs']['time_out'] == round(r['attrs']['time_out'], 5)


def test_declarations_match():
    from pfb_clean_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'pfb_hip.h')).read()
    for name in ('pfb_vis_sum_overlap', 'pfb_vis_weight_sums', 'pfb_beam_combine', 'pfb_beam_eval'):
        assert name in _lib.SIGNATURES and name + '(' in header
    assert int(re.search(r'#define PFB_VIS_BATCH (\d+)', header).group(1)) == cc.BATCH
    assert len(re.findall(r'#define PFB_VIS_BATCH', header)) == 1
    from pfb_clean_amd.utils import concat, beam, misc
    assert concat.BATCH == cc.BATCH
    for name in ('VisDataset', 'concat_row', 'concat_chan', 'sum_overlap', 'sum_beam', '_sum_beam'):
        assert getattr(misc, name) is getattr(concat, name)
    assert beam.eval_beam is beam._eval_beam
    makefile = open(os.path.join(ROOT, 'pfb_clean_amd', 'csrc', 'Makefile')).read()
    assert 'visconcat.hip' in makefile
