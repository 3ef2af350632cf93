"""
The fastim chain on the CPU (no GPU): chunk_plan of pfb_clean_amd/utils/stokes2im.py against hand-written tables, and
the case tables of tests/fastim_cases.py -- the kernel test's element counts against the launch constants of
csrc/imweight.hip as built, the golden fixture's keys and shapes against the case table.
"""
import os
import re

import numpy as np
import pytest

import fastim_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mapping(idx, cnt):
    return {'start_indices': np.array(idx, np.int64), 'counts': np.array(cnt, np.int64)}


def as_tuples(chunks):
    return [(c['ti'], c['fi'], (c['It'].start, c['It'].stop), (c['Irow'].start, c['Irow'].stop),
             (c['Inu'].start, c['Inu'].stop), c['ridx'].tolist(), c['rcnts'].tolist(), c['fidx'].tolist(),
             c['fcnts'].tolist()) for c in chunks]


# five unique times in two output times of unequal row counts; nine channels in five bins, the last of one channel
TIMES = mapping([0, 3], [3, 2])
ROWS = mapping([0, 10, 20, 30, 45], [10, 10, 10, 15, 5])
FREQS = mapping([0, 2, 4, 6, 8], [2, 2, 2, 2, 1])


def test_chunk_plan_with_a_ragged_last_band():
    """cpgi = 4 = 2 cpdi: two bins per image, five bins: three bands, the last of one bin and one channel."""
    from pfb_clean_amd.utils.stokes2im import chunk_plan
    want = []
    for ti, It, Irow, ridx, rcnts in ((0, (0, 3), (0, 30), [0, 10, 20], [10, 10, 10]),
                                      (1, (3, 5), (30, 50), [30, 45], [15, 5])):
        want += [(ti, 0, It, Irow, (0, 4), ridx, rcnts, [0, 2], [2, 2]),
                 (ti, 1, It, Irow, (4, 8), ridx, rcnts, [4, 6], [2, 2]),
                 (ti, 2, It, Irow, (8, 9), ridx, rcnts, [8], [1])]
    assert as_tuples(chunk_plan(TIMES, ROWS, FREQS, 4, 2)) == want


@pytest.mark.parametrize('cpgi', (None, 0, -1))
def test_chunk_plan_all_channels_on_one_image(cpgi):
    """cpgi of None, 0 or -1: the channel count; with cpdi = 2, int(9 / 2) = 4 bins per image and two bands."""
    from pfb_clean_amd.utils.stokes2im import chunk_plan
    got = as_tuples(chunk_plan(TIMES, ROWS, FREQS, cpgi, 2))
    assert [(g[0], g[1], g[4], g[7], g[8]) for g in got] == [
        (0, 0, (0, 8), [0, 2, 4, 6], [2, 2, 2, 2]), (0, 1, (8, 9), [8], [1]),
        (1, 0, (0, 8), [0, 2, 4, 6], [2, 2, 2, 2]), (1, 1, (8, 9), [8], [1])]
    # one channel per bin of the degridder: every bin on the one image
    one = as_tuples(chunk_plan(TIMES, ROWS, FREQS, cpgi, 1))
    assert [(g[0], g[1], g[4]) for g in one] == [(0, 0, (0, 9)), (1, 0, (0, 9))]


def test_chunk_plan_one_time_chunk_and_offset_rows():
    """One output time over all unique times; rows that do not start at zero stay as the mapping has them."""
    from pfb_clean_amd.utils.stokes2im import chunk_plan
    rows = mapping([100, 110, 125], [10, 15, 7])
    got = as_tuples(chunk_plan(mapping([0], [3]), rows, mapping([0, 3], [3, 3]), 3, 3))
    assert got == [(0, 0, (0, 3), (100, 132), (0, 3), [100, 110, 125], [10, 15, 7], [0], [3]),
                   (0, 1, (0, 3), (100, 132), (3, 6), [100, 110, 125], [10, 15, 7], [3], [3])]
    with pytest.raises(ValueError):
        chunk_plan(mapping([0], [3]), rows, mapping([0, 3], [3, 3]), 1, 3)          # no bin fits on an image
    with pytest.raises(ValueError):
        chunk_plan({'start': [0]}, rows, mapping([0], [6]), None, 1)


# ------------------------------------------------------------------------------------------- the kernel's table
def source(name):
    return open(os.path.join(ROOT, *name.split('/'))).read()


def constant(text, pattern):
    m = re.search(pattern, text)
    assert m, pattern
    return m.group(1)


def test_launch_constants_are_the_source_s():
    header, entry, imw = source('include/pfb_hip.h'), source('pfb_clean_amd/csrc/entry.hpp'), \
        source('pfb_clean_amd/csrc/imweight.hip')
    assert int(constant(header, r'#define PFB_IMW_WORK_DOUBLES (\d+)')) == fc.WORK_DOUBLES
    assert int(constant(header, r'#define PFB_IMW_MAX_PROD (\d+)')) == fc.MAX_PROD
    assert int(constant(entry, r'constexpr int ENTRY_BLOCK = (\d+);')) == fc.BLOCK
    assert constant(imw, r'constexpr int IMW_BLOCK = (\w+);') == 'ENTRY_BLOCK'
    assert int(constant(imw, r'constexpr int IMW_RW_MAX_PROD = (\d+);')) == fc.MAX_PROD
    assert constant(imw, r'constexpr int IMW_RW_MAX_GROUPS = ([^;]+);') == 'PFB_IMW_WORK_DOUBLES / IMW_RW_MAX_PROD'
    # the kernel as built: one element per lane and trip, a stride of the whole grid
    kernel = imw[imw.index('k_residual_weigh('):imw.index('emit_partials<NP>')]
    assert 'i += (size_t)gridDim.x * IMW_BLOCK' in kernel and 'reinterpret_cast' not in kernel
    assert fc.MAX_GROUPS == fc.WORK_DOUBLES // fc.MAX_PROD and fc.CAP == fc.MAX_GROUPS * fc.BLOCK
    from pfb_clean_amd import _lib
    from pfb_clean_amd.utils import stokes2im
    assert stokes2im.MAX_PROD == fc.MAX_PROD and fc.WORK_DOUBLES <= _lib.REDUCE_WS_DOUBLES
    assert 'pfb_imw_residual_weigh' in _lib.SIGNATURES and 'pfb_imw_residual_weigh(' in header


def groups(n):
    return -(-min(n, fc.CAP) // fc.BLOCK)


def test_kernel_table_covers_every_launch_edge():
    ns = fc.KERNEL_N
    assert 1 in ns                                                       # one lane
    assert any(1 < n < 64 for n in ns)                                   # below one wave
    assert any(groups(n) >= 2 and n % fc.BLOCK for n in ns)              # two workgroups, the last one partly idle
    assert any(n > fc.CAP and n < 2 * fc.CAP for n in ns)                # a second grid-stride trip for some lanes only
    assert all(groups(n) <= fc.MAX_GROUPS for n in ns)
    assert all(groups(n) * fc.MAX_PROD <= fc.WORK_DOUBLES for n in ns)   # the partials fit the scratch
    for nprod, maps in fc.MODEL_MAPS.items():
        assert all(len(m) == nprod for m in maps)
        assert all(x < 0 for x in maps[0]) and all(x >= 0 for x in maps[-1])          # none, all
        assert nprod == 1 or (any(x < 0 for x in maps[1]) and any(x >= 0 for x in maps[1]))      # some
        used = sorted(x for x in maps[-1])
        assert used == list(range(nprod))


# --------------------------------------------------------------------------------------------------- the fixture
def test_fixture_matches_the_case_table():
    assert os.path.getsize(fc.GOLDEN) < 1 << 20
    with np.load(fc.GOLDEN, allow_pickle=False) as g:
        keys = set(g.files)
    assert keys == {f'{n}_{t}_{k}' for n in fc.CASE_IDS for t in fc.TAGS for k in fc.RESULT_KEYS}
    for case in fc.CASES:
        for tag in fc.TAGS:
            g = fc.golden(case['name'], tag)
            assert g['residual'].shape == (case['nx'], case['ny']) and g['residual'].dtype == np.float64
            assert all(g[k].shape == () and np.isfinite(g[k]) for k in fc.RESULT_KEYS[1:])
            assert g['wsum'] > 0 and g['rms'] > 0 and g['S'] > 0
            assert (g['norm_model'] > 0) == (case['mds'] is not None)
            assert g['rms'] == np.std(g['residual'])


def test_cases_cover_what_the_issue_lists():
    by = {c['name']: c for c in fc.CASES}
    assert {(c['nx'], c['ny']) for c in fc.CASES} == {(32, 24), (16, 64)}
    assert all(60 <= c['nrow'] <= 260 and 3 <= c['nchan'] <= 5 for c in fc.CASES)
    c = by['linear-I']
    assert c['ncorr'] == 4 and c['weight'].ndim == 3 and c['jones'] is None and c['robustness'] is None
    c = by['jones-sigma-minus']
    assert c['jones'].shape[-1] == 2 and c['sigma'] is not None and c['operator'] == '-' and c['frow'].any()
    assert (c['ant1'] == c['ant2']).any() and c['robustness'] == 0 and c['tbin_idx'].size == 2
    c = by['model-two-bins']
    assert c['fbin_idx'].tolist() == [0, 2] and c['fbin_counts'].tolist() == [2, 1] and c['robustness'] == -1
    c = by['circular-V-nowgrid']
    assert (c['poltype'], c['product'], c['ncorr'], c['do_wgridding']) == ('circular', 'V', 2, False)
    assert by['row-weights']['weight'].ndim == 2
    for c in fc.CASES:                           # every baseline inside the counts grid, footprint and all
        for axis, n in ((0, c['nx']), (1, c['ny'])):
            cells = np.abs(c['uvw'][:, axis:axis + 1] * c['freq'][None, :] / fc.C_LIGHT) * n * c['cell']
            assert cells.max() <= n / 2 - 4 + 1e-9
