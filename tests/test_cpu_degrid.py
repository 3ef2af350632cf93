"""
The predict step's fixtures on the CPU (tests/degrid_cases.py, tests/golden/degrid.npz): what makes the bounds of
test_gpu_degrid.py meaningful.

  golden      the numpy model of the block mapping (render, then the direct sum per block) equals what the reference's
              own _comps2vis_impl / _im2vis_impl / _restore_corrs / _loc2psf_vis_impl gave, to 1e-12 relative: both are
              exact sums in fp64.
  mapping     bins with non-zero minima (tbin_idx from 5, rbin_idx from 100, fbin_idx from 7) and uneven counts (1, 3, 2)
              map to the blocks written out below, and the minima do not matter.
  recipe      on every block of every accuracy and golden case the w-gridder's recipe in numpy
              (wgrid_cases.model_dirty2vis) stays below RECIPE_MARGIN = 0.6 of the case's epsilon against the direct
              sum, for the sparse component images and for a dense cube: the GPU, held to epsilon, has room.
  finish      ref_finish_block's bound holds for the kernel's arithmetic imitated in its types, and each of five seeded
              defects -- row0 dropped, chan0 dropped, the last correlation written at index 1, t % nchan_out instead of
              t % nchan_blk, accumulate overwriting -- exceeds it at least 16 times.  The sixth defect one would seed, adding
              BEFORE the cast where the output is narrowed, cannot exceed a bound that admits one rounding of the cast and
              one of the sum: it differs from the contract by one rounding of the narrowed value.  It is therefore pinned
              by bits instead: without a centre phase nothing in the kernel is uncertain, the result is
              fl(old + fl(acc)) exactly, and the defect is shown here to differ from that in some cell;
              test_gpu_degrid.py asserts those bits on the device.
"""
import numpy as np
import pytest

import degrid_cases as dc
import wgrid_cases as wc
import wgrid_kernel_cases as kc

pmp = pytest.mark.parametrize


@pytest.fixture(scope='module')
def npz(golden):
    return golden('degrid')


def close(a, b):
    return np.abs(a - b).max() <= 1e-12 * np.abs(b).max()


@pmp('c', dc.GOLDEN, ids=dc.GOLDEN_IDS)
def test_model_equals_the_reference(npz, c):
    ncorr = dc.GOLDEN_NCORR[c['name']]
    ref = npz[c['name'] + '_comps2vis']
    assert ref.shape == (c['uvw'].shape[0], c['freq'].size, ncorr) and ref.dtype == np.complex128
    assert close(dc.model_comps2vis(c, ncorr), ref)
    assert not ref[:, :, 1:-1].any() and np.array_equal(ref[:, :, 0], ref[:, :, -1]) and ref[:, :, 0].all()
    assert close(dc.model_im2vis(c, c['cube']), npz[c['name'] + '_im2vis'])


def test_restore_corrs_and_loc2psf_fixtures(npz):
    v = npz[dc.GOLDEN_IDS[0] + '_im2vis']
    for ncorr in (1, 2, 4):
        assert np.array_equal(dc.ref_restore_corrs(v, ncorr), npz[f'restore_corrs_{ncorr}'])
    L = dc.LOC2PSF
    c = dc.GOLDEN[dc.GOLDEN_IDS.index(L['case'])]
    delta = np.zeros((128, 128))
    delta[64, 64] = 1.0
    for wg in (True, False):
        blk = dict(dc.block_case(c, 0, c['uvw'].shape[0], 0, c['freq'].size), nx=128, ny=128, px=L['cell'], py=L['cell'],
                   cx=L['x0'], cy=L['y0'], do_wgridding=wg, divide_by_n=False)
        tag = 'wg' if wg else 'nowg'
        assert close(wc.direct_dirty2vis(blk, delta), npz[f'loc2psf_centre_{tag}'])
        # the recipe at the reference's fixed 1e-7 on the 128 x 128 delta
        err = wc.rel_l2(wc.model_dirty2vis(dict(blk, eps=1e-7), delta), npz[f'loc2psf_centre_{tag}'])
        print(f"loc2psf delta, do_wgridding {wg}: recipe at {err / 1e-7:.3f} epsilon")
        assert err <= dc.RECIPE_MARGIN * 1e-7
        assert np.array_equal(npz[f'loc2psf_origin_{tag}'], np.ones(blk['uvw'].shape[:1] + (c['freq'].size,), complex))


def test_mapping_of_offset_uneven_bins():
    c = dc.GOLDEN[0]
    assert (c['tbin_idx'].min(), c['rbin_idx'].min(), c['fbin_idx'].min()) == (5, 100, 7)
    assert tuple(c['tbin_cnts']) == (1, 3, 2) and tuple(c['fbin_cnts']) == (1, 3, 2)
    rc = c['rbin_cnts']
    row_edges = [0, rc[:1].sum(), rc[:4].sum(), rc[:6].sum()]                  # unique times 0 | 1 2 3 | 4 5
    chan_edges = [0, 1, 4, 6]
    want = [(t, b, row_edges[t], row_edges[t + 1], chan_edges[b], chan_edges[b + 1]) for t in range(3) for b in range(3)]
    got = dc.blocks(c)
    assert [g[:6] for g in got] == want
    ut, fr = c['utime'], c['freq']
    assert got[4][6] == dc.tfunc(ut[1:4].mean()) and got[4][7] == dc.ffunc(fr[1:4].mean())
    # the minima are the chunk's position in the data set: they change nothing
    z = dict(c, tbin_idx=c['tbin_idx'] - 5, rbin_idx=c['rbin_idx'] - 100, fbin_idx=c['fbin_idx'] - 7)
    assert dc.blocks(z) == got
    # one time bin per call, concatenated, is the whole call
    vis = dc.model_comps2vis(c, 2)
    for t in range(3):
        one, r0, r1 = dc.time_bin_case(c, t)
        assert np.array_equal(dc.model_comps2vis(one, 2), vis[r0:r1])


@pmp('c', dc.ACCURACY + dc.GOLDEN, ids=dc.ACCURACY_IDS + dc.GOLDEN_IDS)
def test_recipe_meets_epsilon_on_every_block(c):
    ref = dc.model_comps2vis(c, 1)[:, :, 0]
    got = dc.model_comps2vis(c, 1, degrid=wc.model_dirty2vis)[:, :, 0]
    errs = dc.block_errors(c, got, ref)
    cube_errs = dc.band_errors(c, dc.model_im2vis(c, c['cube'], degrid=wc.model_dirty2vis), dc.model_im2vis(c, c['cube']))
    worst = max(errs + cube_errs) / c['eps']
    print(f"{c['name']}: recipe against the direct sum, worst block {max(errs) / c['eps']:.3f} epsilon (components), "
          f"{max(cube_errs) / c['eps']:.3f} epsilon (cube)")
    assert len(errs) == 6 or c['name'] == 'g-mapping'
    assert worst <= dc.RECIPE_MARGIN


CONFIGS = [(dtype, out_tag, centre, accumulate) for dtype in ('f32', 'f64') for out_tag in ('f32', 'f64')
           for centre in (False, True) for accumulate in (False, True) if not (dtype == 'f32' and out_tag == 'f64')]


def _entry(dtype, out_tag, centre, seed=11):
    nchan_blk, row0, chan0, nchan_out, ncorr = 3, 5, 2, 6, 4
    geom, acc, idx, coord, nrow_blk = dc.finish_data(257, nchan_blk, dtype, centre, True, seed)
    acc = acc.astype(dc.NP_C[dtype])
    rng = np.random.default_rng(seed + 3)
    shape = (row0 + nrow_blk + 2, nchan_out, ncorr)
    out0 = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape) + 7.25).astype(dc.NP_C[out_tag])
    return geom, acc, idx, coord, nchan_blk, out0, out_tag, row0, chan0


@pmp('dtype,out_tag,centre,accumulate', CONFIGS)
def test_finish_block_bound_holds_and_defects_exceed_it(dtype, out_tag, centre, accumulate):
    args = _entry(dtype, out_tag, centre)
    ref, B, written = dc.ref_finish_block(*args, accumulate)
    assert written.sum() == 2 * 257 and not written[:, :, 1:3].any() and not written[:5].any()
    clean = dc.excess(dc.finish_block_like(*args, accumulate), ref, B)
    print(f"{dtype}->{out_tag} centre {centre} accumulate {accumulate}: the imitation at {clean:.3g} of the bound")
    assert clean <= 1.0
    for defect in dc.DEFECTS:
        if defect == 'accumulate_overwrites' and not accumulate:
            continue
        over = dc.excess(dc.finish_block_like(*args, accumulate, defect=defect), ref, B)
        assert over >= 16.0, (defect, over)


@pmp('centre', (False, True))
def test_add_before_cast_is_within_the_bound_and_caught_by_bits(centre):
    args = _entry('f64', 'f32', centre)
    ref, B, _ = dc.ref_finish_block(*args, True)
    good, bad = dc.finish_block_like(*args, True), dc.finish_block_like(*args, True, defect='add_before_cast')
    assert dc.excess(bad, ref, B) <= 1.0            # no magnitude bound of this form can tell it from the contract
    differ = int((good != bad).sum())
    print(f"add before cast (centre {centre}): {differ} of {2 * 257} written cells differ in their bits")
    assert differ >= 16
    if not centre:                                  # nothing uncertain: the contract in bits
        geom, acc, idx, coord, nchan_blk, out0, out_tag, row0, chan0 = args
        cell = dc.cells_of(idx, nchan_blk, row0, out0.shape[1], chan0, out0.shape[2])
        want = out0.reshape(-1).copy()
        for k in (0, 3):
            want[cell + k] = want[cell + k] + acc.astype(np.complex64)
        assert np.array_equal(good.reshape(-1), want)


def test_finish_data_shapes():
    for nsorted in (1, 255, 256, 257):
        for nchan_blk in (1, 3):
            for skip in (False, True):
                geom, acc, idx, coord, nrow_blk = dc.finish_data(nsorted, nchan_blk, 'f64', True, skip, 5)
                assert idx.size == nsorted == np.unique(idx).size and idx.max() < nrow_blk * nchan_blk and idx.min() >= 0
                assert (nrow_blk * nchan_blk > nsorted) == (skip or nsorted % nchan_blk != 0)
                assert coord.shape == (3, nsorted) and np.abs(kc.centre_turns(geom, coord)).max() < 4.0
