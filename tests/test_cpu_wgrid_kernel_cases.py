"""
The per-kernel references and geometry tables of tests/wgrid_kernel_cases.py, on the CPU (no GPU):

  composition   chained over the planes' slot ranges with numpy's plane transforms, the references reproduce
                wgrid_cases.model_vis2dirty / model_dirty2vis to 1e-13: they inherit test_model_meets_epsilon_both_
                directions of test_cpu_wgrid.py, and with it the direct Fourier sums.
  properties    every table entry has the edge it is listed for.
  sensitivity   five defects a kernel could have, applied to the references: what each changes, in units of U S, is at
                least 16 x the constant C the GPU test allows -- in fp64 at every support, in fp32 everywhere but for
                the dropped last footprint row at W > 8.  There the last tap is of the order of the fp32 unit roundoff
                (phi at the last row lies in (0, exp(-2.3 W (1 - sqrt(1 - (1 - 2/W)^2)))], median 6e-8 at W = 12): a
                cell or a slot that has any other contribution hides it, and no fp32 comparison can see it.  The
                figures are printed; the fp64 kernels run the same code and are held to the bound.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import wgrid_cases as wc                                       # noqa: E402
import wgrid_kernel_cases as kc                                # noqa: E402

pmp = pytest.mark.parametrize


# ------------------------------------------------------------------------------------------------- composition
def _geom_of(case):
    nplanes, w0, dw = wc.planes(case)
    return kc.geometry('f64', case['nx'], case['ny'], wc.support(case['eps']), nplanes=nplanes, w0=w0, dw=dw,
                       px=case['px'], py=case['py'], cx=case['cx'], cy=case['cy'])


@pmp('name', ['centre', '48x16-eps1e-05', '6x8-eps1e-10'])
def test_references_compose_to_the_model(name):
    case = wc.CASES[wc.CASE_IDS.index(name)]
    geom = _geom_of(case)
    setup = wc._setup(case)
    corr, nm1 = setup['corr'], (setup['nm1'] if case['do_wgridding'] else None)
    idx, coord, plane_off = kc.ref_order(geom, case['uvw'], case['freq'], case['mask'])
    assert np.array_equal(np.sort(idx), setup['sel']) and plane_off[-1] == idx.size
    ranges = list(kc.plane_ranges(geom, plane_off))
    assert len(ranges) > geom['W']
    # vis2dirty
    val, _ = kc.ref_prep(geom, case['vis'], case['wgt'], idx, coord)
    img = np.zeros((case['nx'], case['ny']), complex)
    for p, s0, s1 in ranges:
        grid, _ = kc.ref_grid_plane(geom, coord, val, p, s0, s1)
        img, _ = kc.ref_image_adjoint(geom, np.fft.ifft2(grid, norm='forward'), nm1, p, img)
    dirty, _ = kc.ref_image_correct(img, corr, None)
    assert wc.rel_l2(dirty, wc.model_vis2dirty(case, case['vis'])) <= 1e-13
    # dirty2vis
    acc = np.zeros(idx.size, complex)
    for p, s0, s1 in ranges:
        grid, _ = kc.ref_image_forward(geom, case['dirty'], None, corr, nm1, p)
        acc += kc.ref_degrid_plane(geom, coord, np.fft.fft2(grid), p, s0, s1)[0]
    vis, _ = kc.ref_finish(geom, acc, case['wgt'], idx, coord, case['vis'].size)
    assert wc.rel_l2(vis.reshape(case['vis'].shape), wc.model_dirty2vis(case, case['dirty'])) <= 1e-13
    # the Hessian's hand-over is the weight alone
    wv, _ = kc.ref_weight(acc, case['wgt'], idx)
    assert np.array_equal(wv, acc if case['wgt'] is None else acc * case['wgt'].reshape(-1).astype(np.float64)[idx])


# -------------------------------------------------------------------------------------------------- properties
def test_foot_table_covers_supports_types_and_shapes():
    assert {(e['geom']['W'], e['geom']['dtype']) for e in kc.FOOT} == {(W, d) for W in kc.SUPPORTS for d in kc.DTYPES}
    assert len(kc.FOOT) == 90 and len(set(kc.FOOT_IDS)) == 90
    for W in kc.SUPPORTS:
        m = 2 * kc.narrow(W)
        assert m % 4 == 0 and W <= m <= W + 3 and (m == W) == (W % 4 == 0)
        if W % 2 == 1 and (W + 1) % 4 == 0:
            assert m == W + 1
        es = [e for e in kc.FOOT if e['geom']['W'] == W and e['geom']['dtype'] == 'f64']
        nb = 256 // (2 * W)
        assert {e['n'] for e in es} == {1, nb, nb + 1, 300}
        assert {(e['geom']['Nu'], e['geom']['Nv']) for e in es} == {(m, 16), (16, m), (m, m), (68, 52)}
        assert any(0 < e['s0'] < e['s1'] < e['n'] for e in es) and any((e['s0'], e['s1']) == (0, e['n']) for e in es)
        assert {e['geom']['nplanes'] for e in es} == {1, W + 3}


@pmp('entry', kc.FOOT, ids=kc.FOOT_IDS)
def test_foot_entry_has_its_edges(entry):
    geom, n, s0, s1 = entry['geom'], entry['n'], entry['s0'], entry['s1']
    W, Nu, Nv = geom['W'], geom['Nu'], geom['Nv']
    coord, val, grid = kc.foot_data(entry)
    assert coord.shape == (3, n) and np.isfinite(coord).all()
    # a slot's 2 W lanes straddle two blocks wherever 256 is no multiple of 2 W
    lanes = 2 * W
    straddles = [(s * lanes) // 256 != ((s + 1) * lanes - 1) // 256 for s in range(s1 - s0)]
    if 256 % lanes and s1 - s0 > 256 // lanes:
        assert any(straddles)
    if s1 - s0 == 256 // lanes + 1:
        assert 256 % lanes == 0 or straddles[-1]
    fp = kc.footprint(geom, coord, entry['planes'][0], s0, s1)
    if Nu == W:                                     # every row of the grid is hit by every slot
        assert all(np.array_equal(np.sort(r), np.arange(Nu)) for r in fp['rows'])
    if Nv == W:
        assert all(np.array_equal(np.sort(c), np.arange(Nv)) for c in fp['cols'])
    assert all(np.unique(r).size == W for r in fp['rows']) and all(np.unique(c).size == W for c in fp['cols'])
    if n == 300:
        ug, vg = coord[0, s0:s1], coord[1, s0:s1]
        for g, N in ((ug, Nu), (vg, Nv)):
            assert (g == 0.5 * N).any() and (g == -0.5 * N).any()                       # on the seam
            assert (np.abs(g) < 0.5 * N).any()
            assert ((g > 2 * N) & (g < 7 * N)).any() and ((g < -2 * N) & (g > -7 * N)).any()
            assert (g > 9e5).any() and (g < -9e5).any() and np.abs(g).max() < 2e6
        wu, wv = fp['rows'][:, -1] < fp['rows'][:, 0], fp['cols'][:, -1] < fp['cols'][:, 0]
        assert (wu & wv).any() and (wu & ~wv).any() and (~wu & wv).any() and (~wu & ~wv).any()
        # three planes: one with weight everywhere, one at each end with exact zeros
        p_lo, p_mid, p_hi = entry['planes']
        assert (p_lo, p_hi) == (0, geom['nplanes'] - 1) and geom['nplanes'] > W
        assert (kc.footprint(geom, coord, p_mid, s0, s1)['ww'] > 0).all()
        for p in (p_lo, p_hi):
            ww = kc.footprint(geom, coord, p, s0, s1)['ww']
            assert (ww == 0).any() and (ww > 0).sum() >= 10
        if s0 == 0:
            assert kc.footprint(geom, coord, p_lo, 0, 1)['ww'][0] == 0 and abs((p_lo - coord[2, 0]) / geom['h']) == 1
            assert kc.footprint(geom, coord, p_hi, 1, 2)['ww'][0] == 0 and abs((p_hi - coord[2, 1]) / geom['h']) == 1
            assert kc.footprint(geom, coord, p_mid, 2, 3)['ww'][0] == 1
    else:
        assert geom['nplanes'] == 1 and (fp['ww'] == 1).all()


@pmp('entry', kc.ORDER, ids=kc.ORDER_IDS)
def test_order_entry_has_its_edges(entry):
    geom, uvw, freq, mask = kc.order_data(entry)
    nrow, nchan = entry['nrow'], entry['nchan']
    assert geom['tile'] == entry['tile'] and geom['ntu'] * geom['ntv'] <= 4096
    half = geom['tile'] // 2
    assert half < 16 or ((geom['Nu'] + half - 1) // half) * ((geom['Nv'] + half - 1) // half) > 4096
    if (entry['nx'], entry['ny']) == (512, 512):
        assert geom['ntu'] * geom['ntv'] == 4096 and geom['tile'] == 16
    if (entry['nx'], entry['ny']) == (2050, 130):
        assert geom['Nu'] == 4100 and geom['Nu'] % geom['tile'] == 4 and geom['Nv'] % geom['tile'] == 4
    keys, hist = kc.ref_keys(geom, uvw, freq, mask)
    nvis = nrow * nchan
    live = np.ones(nvis, bool) if mask is None else mask != 0
    assert keys.shape == (nvis,) and (keys[~live] == -1).all() and (keys[live] >= 0).all()
    assert keys.max() < geom['nkeys'] and hist.sum() == live.sum() >= 1 and hist.size == geom['nkeys']
    if entry['mask'] == 'all-but-one':
        assert live.sum() == 1
    if entry['mask'] == 'partial' and nvis > 3:
        assert 1 <= live.sum() < nvis
    # where the unmasked and the masked visibilities sit (the reference's own keys, decoded)
    ug, vg, pg = kc.vis_coords(geom, uvw, freq)
    a = kc.wrap(kc.first(ug, geom['h']), geom['Nu'])
    b = kc.wrap(kc.first(vg, geom['h']), geom['Nv'])
    ntiles = geom['ntu'] * geom['ntv']
    assert np.array_equal(keys[live] % ntiles, ((a // geom['tile']) * geom['ntv'] + b // geom['tile'])[live])
    if nrow >= 85:
        if geom['Nu'] % geom['tile']:
            last = a // geom['tile'] == geom['ntu'] - 1                  # the partial last tile is populated
            assert last.any() and (last & (ug < 0)).any() and a[last].min() >= geom['Nu'] - geom['Nu'] % geom['tile']
        assert (a == geom['Nu'] - 1).any() and (b == geom['Nv'] - 1).any() and (a // geom['tile'] == 0).any()
        p = kc.first(pg, geom['h'])
        p0 = keys // ntiles
        below, above = live & (p < 0), live & (p > geom['np0'] - 1)
        if entry['mask'] != 'all-but-one':
            assert below.any() and above.any()                            # both sides of the clamp
        assert (p0[below] == 0).all() and (p0[above] == geom['np0'] - 1).all()
        inside = live & (p >= 0) & (p <= geom['np0'] - 1)
        assert np.array_equal(p0[inside], p[inside].astype(int))
    idx, coord, plane_off = kc.ref_order(geom, uvw, freq, mask)
    assert np.array_equal(np.sort(idx), np.flatnonzero(live)) and (np.diff(keys[idx]) >= 0).all()
    assert len(plane_off) == geom['np0'] + 1 and plane_off[0] == 0 and plane_off[-1] == idx.size


def test_order_table_covers_blocks_channels_and_masks():
    assert {e['nrow'] * e['nchan'] for e in kc.ORDER} >= {1, 3, 255, 256, 257, 513}
    assert {e['nchan'] for e in kc.ORDER} == {1, 3} and {e['tile'] for e in kc.ORDER} == {16, 32, 64}
    for name, *_ in kc.ORDER_IMAGES:
        assert {e['mask'] for e in kc.ORDER if e['id'].startswith(name + '-')} == set(kc.ORDER_MASKS)
    assert kc.ORDER_NPLANES > kc.ORDER_W


def test_image_and_slot_tables():
    for e in kc.IMAGE:
        g = e['geom']
        assert (g['nx'] * g['ny']) % 256 != 0 and (g['nx'] // 2) % 2 == 1
        d = kc.image_data(e)
        assert (d['beam'] is not None) == e['beam'] and (d['nm1'] is not None) == e['nm1']
        assert 0 <= e['plane'] < g['nplanes']
    npix = {e['geom']['nx'] * e['geom']['ny'] for e in kc.IMAGE}
    assert min(npix) == 4 and any(n < 256 for n in npix) and any(n > 256 for n in npix) and any(n > 768 for n in npix)
    assert any((e['geom']['ny'] // 2) % 2 == 0 for e in kc.IMAGE) and any((e['geom']['ny'] // 2) % 2 == 1 for e in kc.IMAGE)
    for dtype in kc.DTYPES:
        vs = {(e['beam'], e['nm1'], e['geom']['nplanes'] == 1, e['plane'] > 0) for e in kc.IMAGE if e['geom']['dtype'] == dtype}
        assert vs == {(True, True, True, False), (False, True, False, False), (True, True, False, True),
                      (False, False, True, False)}
    # nplanes == 1 with nm1: the plane lies at w0, not at 0
    one = next(e for e in kc.IMAGE if e['nm1'] and e['geom']['nplanes'] == 1)
    assert kc.plane_w(one['geom'], 0) == one['geom']['w0'] != 0.0
    assert {(e['dtype'], e['wgt'], e['centre']) for e in kc.SLOT} == {(d, w, c) for d in kc.DTYPES for w in (True, False)
                                                                     for c in (True, False)}
    for e in kc.SLOT:
        d = kc.slot_data(e)
        assert 256 < d['idx'].size < d['nvis'] and d['idx'].size % 256 != 0
        assert (np.abs(kc.centre_turns(d['geom'], d['coord'])).max() > 1.0) == e['centre']


# -------------------------------------------------------------------------------------------------- sensitivity
def _ratio(defect, ref, S, u):
    """max over the elements of |defect - ref| / (u S), per component."""
    worst = 0.0
    for d, s in ((np.abs((defect - ref).real), S.real), (np.abs((defect - ref).imag), S.imag)):
        on = s > 0
        assert not d[~on].any()
        if on.any():
            worst = max(worst, (d[on] / (u * s[on])).max())
    return worst


def _foot_defects(entry):
    """{(entry point, defect): |defect - ref| / S worst element} on the middle plane of a 34 x 26 entry."""
    geom, s0, s1 = entry['geom'], entry['s0'], entry['s1']
    coord, val, grid = kc.foot_data(entry)
    plane = entry['planes'][1]
    fp = kc.footprint(geom, coord, plane, s0, s1)
    past = fp['rows'] < fp['rows'][:, :1]
    assert past.any()
    variants = {
        '1 last row dropped': (dict(fp, fu=np.where(np.arange(geom['W']) == geom['W'] - 1, 0.0, fp['fu'])), s0, s1),
        '2 rows past the seam dropped': (dict(fp, fu=np.where(past, 0.0, fp['fu'])), s0, s1),
        '3 w weight of plane + 1': (dict(fp, ww=kc.footprint(geom, coord, plane + 1, s0, s1)['ww']), s0, s1),
        '3 w weight of plane - 1': (dict(fp, ww=kc.footprint(geom, coord, plane - 1, s0, s1)['ww']), s0, s1),
        '4 first slot dropped': (None, s0 + 1, s1),
        '4 last slot dropped': (None, s0, s1 - 1),
    }
    g_ref, g_S = kc.ref_grid_plane(geom, coord, val, plane, s0, s1, fp)
    d_ref, d_S = kc.ref_degrid_plane(geom, coord, grid, plane, s0, s1, fp)
    out = {}
    for tag, (f, a, b) in variants.items():
        out['grid', tag] = _ratio(kc.ref_grid_plane(geom, coord, val, plane, a, b, f)[0], g_ref, g_S, 1.0)
        out['degrid', tag] = _ratio(kc.ref_degrid_plane(geom, coord, grid, plane, a, b, f)[0], d_ref, d_S, 1.0)
    return out


@pmp('W', kc.SUPPORTS)
def test_defects_of_the_footprint_kernels_exceed_the_tolerance(W):
    entry = kc.FOOT[kc.FOOT_IDS.index(f'W{W}-f64-34x26-interior')]
    for (name, tag), rel in _foot_defects(entry).items():
        for dtype in kc.DTYPES:
            r, need = rel / kc.U[dtype], 16 * kc.TOLERANCE_C[name][dtype]
            print(f"W {W} {name:6s} {dtype} {tag:30s} {r:.3e} (16 C = {need:g})")
            if dtype == 'f32' and tag.startswith('1') and W > 8:
                continue                    # not detectable in fp32: see the docstring
            assert r >= need, (name, tag, dtype)


@pmp('entry', [e for e in kc.IMAGE if e['geom']['nx'] * e['geom']['ny'] > 256 and e['geom']['dtype'] == 'f64'],
     ids=[e['id'] for e in kc.IMAGE if e['geom']['nx'] * e['geom']['ny'] > 256 and e['geom']['dtype'] == 'f64'])
def test_an_unwritten_last_block_of_an_image_kernel_exceeds_the_tolerance(entry):
    """Defect 5: the last npix % 256 pixels left as they were (zero in the cleared grid, img and dirty untouched)."""
    geom, d = entry['geom'], kc.image_data(entry)
    nx, ny = geom['nx'], geom['ny']
    tail = np.zeros(nx * ny, bool)
    tail[-((nx * ny) % 256):] = True
    tail = tail.reshape(nx, ny)
    win = kc._window(geom)
    f_ref, f_S = kc.ref_image_forward(geom, d['dirty'], d['beam'], d['corr'], d['nm1'], entry['plane'])
    f_def = f_ref.copy()
    f_def[win] = np.where(tail, 0.0, f_ref[win])
    a_ref, a_S = kc.ref_image_adjoint(geom, d['grid'], d['nm1'], entry['plane'], d['img'])
    a_def = np.where(tail, d['img'], a_ref)
    c_ref, c_S = kc.ref_image_correct(d['img'], d['corr'], d['beam'])
    c_def = np.where(tail, 0.0, c_ref)
    for name, rel in (('image_forward', _ratio(f_def, f_ref, f_S, 1.0)), ('image_adjoint', _ratio(a_def, a_ref, a_S, 1.0)),
                      ('image_correct', _ratio(c_def + 0j, c_ref + 0j, c_S + 0j, 1.0))):
        for dtype in kc.DTYPES:
            r, need = rel / kc.U[dtype], 16 * kc.TOLERANCE_C[name][dtype]
            print(f"{entry['id']} {name} {dtype}: {r:.3e} (16 C = {need:g})")
            assert r >= need, (name, dtype)
