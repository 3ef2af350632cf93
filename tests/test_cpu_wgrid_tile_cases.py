"""
The references and the table of tests/wgrid_tile_cases.py, proved on the CPU.

  - The emulation of the tile gridder -- target map by the general rule, then per-cell sums in list order -- equals
    wgrid_kernel_cases.ref_grid_plane on every entry, plane and product to fp64 rounding (another sum order: 64 U S).
    That is the proof of the target rule: a footprint cell whose tile did not list the slot's segment would be missing,
    a segment listed twice would count twice.
  - Each edge the table claims is hit: a grid that is one tile; a partial last tile narrower than W - 1 that a footprint
    crosses on its way into tile 0; first cells at N - 1 on both axes at once; a target that walks exactly one staging
    batch, one whose batch ends between two segments and one whose batch ends inside a segment; planes that hold
    nothing; a slot exactly on the zero of the w weight.
  - The wrong rule ("the tile and its next neighbour, no dedup") fails on the entries built for it by far more than
    the bound, and passes where it is right (two full tiles): the table has teeth.
  - package-free: nothing here imports pfb_clean_amd.
"""
import numpy as np
import pytest

import wgrid_kernel_cases as kc
import wgrid_tile_cases as tc

pmp = pytest.mark.parametrize
F64 = [e for e in tc.TILE if e['geom']['dtype'] == 'f64']
F64_IDS = [e['id'] for e in F64]
SUM_ORDER_C = 64.0          # two fp64 sums of the same terms in different orders: far below any kernel's C


def excess(got, ref, S):
    """max |got - ref| / (U S) over both components; exact where S is zero."""
    worst = 0.0
    for d, s in ((np.abs(got.real - ref.real), S.real), (np.abs(got.imag - ref.imag), S.imag)):
        assert not d[s == 0].any()
        if (s > 0).any():
            worst = max(worst, float((d[s > 0] / s[s > 0]).max()) / kc.U['f64'])
    return worst


@pmp('entry', F64, ids=F64_IDS)
def test_emulation_equals_the_reference(entry):
    geom = entry['geom']
    coord, val, plane_off, tmap = tc.tile_data(entry)
    for plane in entry['planes']:
        for k in (0, tc.NPROD - 1):
            got, _ = tc.emulate_grid_plane(geom, coord, val[k], plane, tmap)
            ref, S = kc.ref_grid_plane(geom, coord, val[k], plane, 0, entry['n'])
            assert excess(got, ref, S) <= SUM_ORDER_C, (entry['id'], plane, k)


@pmp('entry', F64, ids=F64_IDS)
def test_map_is_a_csr_sorted_by_first_plane_and_source(entry):
    geom = entry['geom']
    coord, _, plane_off, tmap = tc.tile_data(entry)
    tgt_tile, tgt_ptr, pstart, pcount, pp0, psrc = tmap
    nfu, nfv = tc.fine_tiles(geom)
    assert (np.diff(tgt_tile) > 0).all() and 0 <= tgt_tile.min() and tgt_tile.max() < nfu * nfv
    assert tgt_ptr[0] == 0 and tgt_ptr[-1] == pstart.size and (np.diff(tgt_ptr) > 0).all()
    for t in range(tgt_tile.size):
        order = [(int(pp0[p]), int(psrc[p])) for p in range(tgt_ptr[t], tgt_ptr[t + 1])]
        assert order == sorted(set(order))                         # ascending, each source once
    assert (pstart + pcount <= entry['n']).all() and (pcount >= 1).all()
    assert pstart.size <= 9 * np.unique(tc.coord_keys(geom, coord)).size
    # slots stay grouped by first plane
    p0 = tc.coord_keys(geom, coord) // (nfu * nfv)
    assert (np.diff(p0) >= 0).all() and plane_off == np.searchsorted(p0, np.arange(geom['np0'] + 1)).tolist()


@pmp('entry', [e for e in F64 if e['tag'] == 'one-tile'], ids=lambda e: e['id'])
def test_one_tile_is_its_own_neighbour_once(entry):
    geom = entry['geom']
    coord, _, _, tmap = tc.tile_data(entry)
    assert tc.fine_tiles(geom) == (1, 1)
    nseg = np.unique(tc.coord_keys(geom, coord)).size
    assert tmap[0].tolist() == [0] and tmap[2].size == nseg
    wrong = tc.ref_tile_map(geom, *tc.segments(np.sort(tc.coord_keys(geom, coord))), rule='wrong')
    assert wrong[2].size == 4 * nseg


@pmp('entry', [e for e in F64 if e['tag'] == 'partial'], ids=lambda e: e['id'])
def test_partial_last_tiles_wraps_and_planes(entry):
    geom, W = entry['geom'], entry['geom']['W']
    coord, _, plane_off, tmap = tc.tile_data(entry)
    Nu, Nv = geom['Nu'], geom['Nv']
    assert (Nu, Nv) == (40, 36) and tc.fine_tiles(geom) == (3, 3)          # tiles 16, 16, 8 and 16, 16, 4
    a, b = kc.wrap(kc.first(coord[0], geom['h']), Nu), kc.wrap(kc.first(coord[1], geom['h']), Nv)
    assert ((a == Nu - 1) & (b == Nv - 1)).any()                           # N - 1 on both axes at once
    below = (kc.first(coord[0], geom['h']) == -2) & (kc.first(coord[1], geom['h']) == -2)
    assert (below & (a == Nu - 2) & (b == Nv - 2)).any()                   # the last tiles, from a first cell below zero
    for first, N, last in ((a, Nu, 8), (b, Nv, 4)):
        crossing = (first == 31) & (31 + W - 1 >= N)          # starts before the last tile, ends in tile 0
        assert crossing.any() == (last < W - 1)
    feeds_u, feeds_v = tc.axis_feeds(Nu, W), tc.axis_feeds(Nv, W)
    assert (feeds_u[1] == [0, 1, 2]) == (W >= 10) and (feeds_v[1] == [0, 1, 2]) == (W >= 6)
    # planes: first planes 0 .. 2 only, so the planes beyond W + 1 hold nothing; the exact zeros of the weight
    assert plane_off[3] == entry['n'] and plane_off[1] > 0
    for plane in (W + 2, W + 5):
        grid, walked = tc.emulate_grid_plane(geom, coord, np.ones(entry['n'], complex), plane, tmap)
        assert not walked and not grid.any()
    ww0 = kc.footprint(geom, coord, 0, 0, entry['n'])['ww']
    ww1 = kc.footprint(geom, coord, 1, 0, entry['n'])['ww']
    p0 = tc.coord_keys(geom, coord) // 9
    assert ((ww0 == 0) & (p0 == 0)).sum() == 1 and ((ww1 == 0) & (p0 == 1)).sum() == 1


@pmp('entry', [e for e in F64 if e['tag'] == 'batches'], ids=lambda e: e['id'])
def test_batch_boundaries(entry):
    geom = entry['geom']
    coord, val, _, tmap = tc.tile_data(entry)
    assert tc.fine_tiles(geom) == (4, 4)
    _, walked = tc.emulate_grid_plane(geom, coord, val[0], 0, tmap)
    assert walked[1 * 4 + 1] == [30, 34, 5, 70]          # 64 falls between two segments, 128 inside the last
    assert walked[3 * 4 + 3] == [tc.BATCH]               # exactly one batch
    assert sum(walked[0]) > tc.BATCH                     # tile 0: its own 30 and what wraps in from (3, 3)


def _wrong_excess(entry):
    geom = entry['geom']
    coord, val, _, _ = tc.tile_data(entry)
    wrong = tc.ref_tile_map(geom, *tc.segments(np.sort(tc.coord_keys(geom, coord))), rule='wrong')
    worst = 0.0
    for plane in entry['planes'][:3]:
        got, _ = tc.emulate_grid_plane(geom, coord, val[0], plane, wrong)
        ref, S = kc.ref_grid_plane(geom, coord, val[0], plane, 0, entry['n'])
        d = np.abs(got - ref)
        worst = max(worst, float((d[np.abs(S) > 0] / np.abs(S)[np.abs(S) > 0]).max()) / kc.U['f64'])
    return worst


@pmp('entry', [e for e in F64 if e['tag'] == 'one-tile' or (e['tag'] == 'partial' and e['geom']['W'] >= 6)],
     ids=lambda e: e['id'])
def test_the_wrong_rule_fails_where_the_table_was_built_for_it(entry):
    assert _wrong_excess(entry) > 16 * kc.TOLERANCE_C['grid']['f32'] * kc.U['f32'] / kc.U['f64']


@pmp('entry', [e for e in F64 if e['tag'] == 'two-tiles'], ids=lambda e: e['id'])
def test_the_wrong_rule_is_right_on_two_full_tiles(entry):
    assert _wrong_excess(entry) <= SUM_ORDER_C


def test_orders_are_stable_and_grouped():
    for entry in tc.ORDER:
        geom, uvw, freq, mask = kc.order_data(entry)
        idx, coord, plane_off, skeys = tc.ref_tile_order(geom, uvw, freq, mask)
        keys = tc.ref_keys64(geom, uvw, freq, mask)
        assert np.array_equal(np.sort(idx), np.flatnonzero(keys != tc.MASKED))
        assert (np.diff(skeys) >= 0).all() and (np.diff(idx)[np.diff(skeys) == 0] > 0).all()      # ascending t in a key
        assert np.array_equal(tc.coord_keys(geom, coord), skeys) and len(plane_off) == geom['np0'] + 1
        # the same slots per first plane as the default order
        assert plane_off == list(kc.ref_order(geom, uvw, freq, mask)[2])
