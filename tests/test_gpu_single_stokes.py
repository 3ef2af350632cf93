"""
single_stokes (pfb_clean_amd/utils/stokes2vis.py, the init worker's per-chunk conversion) on the MI355X: its VIS, WEIGHT
and MASK against the fp64 oracle of tests/chanavg_cases.py at that file's bounds, its FREQ, BEAM, coords and attrs, what
it refuses, and four of its outputs (2 times x 2 bands) through concat_row and concat_chan into image_data_products with
device tensors throughout, against the same chain fed from stokes_vis by hand.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import chanavg_cases as ca
import stokes_cases as sc

pytestmark = pytest.mark.gpu

TAGS = ('f32', 'f64')
SHAPE = (86, 3, 3)
RADEC = np.array([0.3, -0.7])
CELL = 2e-4
FOV = 1.0
# (data_column, sigma_column, weight_column, FLAG_ROW in ds) and the case fields they stand for
COLUMNS = {'minus-spectrum': ('DATA - MODEL_DATA', None, 'WEIGHT_SPECTRUM', True, dict(op='-', wform='spectrum')),
           'plus-sigma': ('DATA+MODEL_DATA', 'SIGMA_SPECTRUM', 'WEIGHT_SPECTRUM', True, dict(op='+', wform='sigma')),
           'row': ('DATA', None, 'WEIGHT', True, dict(wform='row')),
           'ones-no-frow': ('DATA', None, None, False, dict(wform='none', use_frow=False))}


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def the_case(key, product='V', n=SHAPE[2]):
    return ca.case((SHAPE[0], SHAPE[1], n), 'full4', 'circular', product, label='ss', **COLUMNS[key][4])


def dataset(c, tag, key, conv=lambda a: a):
    """The case's set as the chunk an init worker holds, and the opts that read it."""
    from pfb_clean_amd.utils.concat import VisDataset
    s = c['set']
    cdt, rdt = sc.CDT[tag], sc.RDT[tag]
    nrow = s['data'].shape[0]
    rng = np.random.default_rng(5)
    cols = {'DATA': (('row', 'chan', 'corr'), conv(s['data'].astype(cdt))),
            'MODEL_DATA': (('row', 'chan', 'corr'), conv(s['data2'].astype(cdt))),
            'WEIGHT_SPECTRUM': (('row', 'chan', 'corr'), conv(s['weight'].astype(rdt))),
            'SIGMA_SPECTRUM': (('row', 'chan', 'corr'), conv(s['sigma'].astype(rdt))),
            'WEIGHT': (('row', 'corr'), conv(s['wrow'].astype(rdt))),
            'FLAG': (('row', 'chan', 'corr'), conv(s['flag3'])),
            'ANTENNA1': (('row',), conv(s['ant1'])), 'ANTENNA2': (('row',), conv(s['ant2'])),
            'UVW': (('row', 'uvw'), conv(rng.standard_normal((nrow, 3)) * 50.0))}
    data_column, sigma_column, weight_column, has_frow = COLUMNS[key][:4]
    if has_frow:
        cols['FLAG_ROW'] = (('row',), conv(s['frow']))
    ds = VisDataset(cols, attrs=dict(FIELD_ID=3, DATA_DESC_ID=1, SCAN_NUMBER=7))
    opts = SimpleNamespace(precision={'f32': 'single', 'f64': 'double'}[tag], data_column=data_column,
                           sigma_column=sigma_column, weight_column=weight_column, flag_column='FLAG',
                           product=c['product'], chan_average=c['n'], max_field_of_view=FOV, beam_model=None, radec=None)
    return ds, opts


def call(c, tag, key, conv=lambda a: a, mutate=None, **over):
    from pfb_clean_amd.utils.stokes2vis import single_stokes
    s = c['set']
    nchan = s['data'].shape[1]
    ds, opts = dataset(c, tag, key, conv)
    if mutate:
        mutate(ds)
    for k, v in over.items():
        setattr(opts, k, v)
    freq = 1.0e9 + 2.0e6 * np.arange(nchan) ** 1.5
    width = np.full(nchan, 2.0e6) + np.arange(nchan)
    utime = np.array([10.0, 20.0, 40.0])
    out = single_stokes(ds=ds, jones=conv(s['jones'].astype(sc.CDT[tag])), opts=opts, freq=freq, chan_width=width,
                        cell_rad=CELL, utime=utime, tbin_idx=s['tbin_idx'], tbin_counts=s['tbin_counts'], radec=RADEC,
                        antpos=np.zeros((5, 3)), poltype=c['pol'])
    return out, ds, freq, width, utime


@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('key', list(COLUMNS))
def test_against_the_oracle(key, n, tag):
    from pfb_clean_amd.utils.concat import VisDataset
    from pfb_clean_amd.utils.stokes import average_freq
    c = the_case(key, n=n)
    out, ds, freq, width, utime = call(c, tag, key)
    o = ca.oracle(c)
    assert isinstance(out, VisDataset)
    assert set(out) == {'FREQ', 'WEIGHT', 'UVW', 'VIS', 'MASK', 'BEAM', 'chan', 'l_beam', 'm_beam'}
    vis, wgt, mask = out.VIS.values, out.WEIGHT.values, out.MASK.values
    assert all(isinstance(a, np.ndarray) for a in (vis, wgt, mask, out.UVW.values, out.BEAM.values))
    assert vis.dtype == sc.CDT[tag] and wgt.dtype == sc.RDT[tag] and mask.dtype == np.uint8
    assert out.VIS.dims == out.WEIGHT.dims == out.MASK.dims == ('row', 'chan')
    assert vis.shape == o['vis'].shape == (SHAPE[0], -(-SHAPE[1] // n))
    ev, ew = ca.worst(vis, o['vis'], o['vis_unit'], tag), ca.worst(wgt, o['wgt'], o['wgt_unit'], tag)
    print(f"{c['name']} {tag}: vis {ev:.3f}, wgt {ew:.3f} of the bound")
    assert np.isfinite(vis).all() and np.isfinite(wgt).all() and ev <= 1 and ew <= 1
    assert np.array_equal(mask, o['mask'])
    # rows and UVW as they came
    assert out.UVW.values is ds.UVW.values and out.UVW.dims == ('row', 'uvw')
    # the channels: averaged; the attrs: of the un-averaged freq
    want_freq = freq if n == 1 else average_freq(freq, width, n)[0]
    assert np.array_equal(out.FREQ.values, want_freq) and np.array_equal(out.chan.values, want_freq)
    assert out.FREQ.values.dtype == np.float64
    if n == 3:
        assert out.FREQ.values.tolist() == [freq.mean()]
    assert out.attrs == {'ra': RADEC[0], 'dec': RADEC[1], 'fieldid': 3, 'ddid': 1, 'scanid': 7, 'freq_out': np.mean(freq),
                         'freq_min': freq.min(), 'freq_max': freq.max(), 'time_out': np.mean(utime), 'time_min': 10.0,
                         'time_max': 40.0, 'product': c['product']}
    # the beam of ones on int(deg2rad(1.1 fov) / cell) pixels, its axes in degrees
    npix = int(np.deg2rad(FOV * 1.1) / CELL)
    assert npix == 95
    beam = out.BEAM.values
    assert beam.shape == (npix, npix) and beam.dtype == np.float64 and (beam == 1).all()
    assert out.BEAM.dims == ('l_beam', 'm_beam')
    axis = (-(npix // 2) + np.arange(npix)) * np.rad2deg(CELL)
    assert np.array_equal(out.l_beam.values, axis) and np.array_equal(out.m_beam.values, axis)


@pytest.mark.parametrize('tag', TAGS)
def test_two_products_carry_a_leading_axis(tag):
    c = the_case('minus-spectrum', product='IV')
    out = call(c, tag, 'minus-spectrum')[0]
    o = ca.oracle(c)
    assert out.VIS.dims == out.WEIGHT.dims == ('product', 'row', 'chan') and out.MASK.dims == ('row', 'chan')
    assert out.VIS.values.shape == o['vis'].shape == (2, SHAPE[0], 1)
    ev = ca.worst(out.VIS.values, o['vis'], o['vis_unit'], tag)
    ew = ca.worst(out.WEIGHT.values, o['wgt'], o['wgt_unit'], tag)
    print(f"{c['name']} {tag}: vis {ev:.3f}, wgt {ew:.3f} of the bound")
    assert ev <= 1 and ew <= 1 and np.array_equal(out.MASK.values, o['mask'])
    assert out.product == 'IV'


def test_the_callers_arrays_are_not_written():
    c = the_case('plus-sigma')
    from pfb_clean_amd.utils.stokes2vis import single_stokes
    ds, opts = dataset(c, 'f32', 'plus-sigma')
    keep = {k: v.values.copy() for k, v in ds.items()}
    tbin = c['set']['tbin_idx'].copy()
    nchan = SHAPE[1]
    single_stokes(ds=ds, jones=None, opts=opts, freq=np.arange(1.0, nchan + 1), chan_width=np.ones(nchan), cell_rad=CELL,
                  utime=np.array([1.0]), tbin_idx=c['set']['tbin_idx'], tbin_counts=c['set']['tbin_counts'], radec=RADEC,
                  antpos=None, poltype='linear')
    assert all(np.array_equal(ds[k].values, v, equal_nan=True) for k, v in keep.items())
    assert np.array_equal(c['set']['tbin_idx'], tbin)


def test_refusals():
    c = the_case('row')
    with pytest.raises(NotImplementedError):
        call(c, 'f32', 'row', radec='J2000,0deg,-30deg')
    with pytest.raises(NotImplementedError):
        call(c, 'f32', 'row', radec=RADEC + 1e-9)
    call(c, 'f32', 'row', radec=RADEC.copy())                           # the field's own: fine
    for model in ('kbl', 'katbeam_uhf', 'beam.npz'):
        with pytest.raises(NotImplementedError):
            call(c, 'f32', 'row', beam_model=model)
    with pytest.raises(ValueError, match='chan_average'):
        call(c, 'f32', 'row', chan_average=0)
    with pytest.raises(ValueError, match='precision'):
        call(c, 'f32', 'row', precision='half')
    # a row weight under another column's name, a spectrum under WEIGHT's
    def swap(ds):
        ds['WEIGHT'], ds['WEIGHT_SPECTRUM'] = ds['WEIGHT_SPECTRUM'], ds['WEIGHT']
    for column in ('WEIGHT', 'WEIGHT_SPECTRUM'):
        with pytest.raises(ValueError, match='row weight'):
            call(c, 'f32', 'row', weight_column=column, mutate=swap)


# --------------------------------------------------------------------------------------------------- the chain
def test_four_outputs_merge_and_image_on_the_device():
    """2 times x 2 bands of 6 channels, averaged by 2, device tensors throughout: single_stokes -> concat_row ->
    concat_chan(nband_out=1) -> image_data_products, against the same chain over datasets built by hand from
    stokes_vis(chan_average=2) and average_freq.  The merged VIS, WEIGHT, MASK, UVW, FREQ and WSUM are the same bits --
    both sides run the same kernels on the same inputs; DIRTY differs by the order of the gridder's atomic adds only:
    per pixel at most nvis eps S (1 + epsilon), S = sum wgt |vis| over the unmasked merged visibilities."""
    from pfb_clean_amd.operators.gridder import image_data_products
    from pfb_clean_amd.utils.concat import VisDataset
    from pfb_clean_amd.utils.misc import concat_chan, concat_row
    from pfb_clean_amd.utils.stokes import average_freq, stokes_vis
    from pfb_clean_amd.utils.stokes2vis import single_stokes
    rng = np.random.default_rng(41)
    nrow, nchan, nant, n, eps = 24, 6, 4, 2, 1e-6
    nx, ny = 32, 24
    opts = SimpleNamespace(precision='double', data_column='DATA', sigma_column=None, weight_column='WEIGHT_SPECTRUM',
                           flag_column='FLAG', product='I', chan_average=n, max_field_of_view=FOV, beam_model=None,
                           radec=RADEC)
    got, hand = [], []
    for t, utime in enumerate((np.array([100.0, 110.0]), np.array([200.0, 210.0]))):
        ant1 = rng.integers(0, nant - 1, nrow).astype(np.int32)
        ant2 = (ant1 + 1 + rng.integers(0, nant, nrow) % (nant - 1 - ant1)).astype(np.int32)
        ant2[3] = ant1[3]
        uvw = dev(rng.standard_normal((nrow, 3)) * 50.0)
        frow = dev(rng.uniform(size=nrow) < 0.1)
        tbin_idx, tbin_counts = np.array([0, nrow // 2]), np.array([nrow // 2, nrow - nrow // 2])
        for b in range(2):
            freq = 1.0e9 + 1.0e7 * (b * nchan + np.arange(nchan))
            width = np.full(nchan, 1.0e7)
            data = dev(rng.standard_normal((nrow, nchan, 4)) + 1j * rng.standard_normal((nrow, nchan, 4)))
            weight = dev(rng.uniform(0.5, 2.0, (nrow, nchan, 4)))
            flag = dev(rng.uniform(size=(nrow, nchan, 4)) < 0.05)
            jones = dev(rng.uniform(0.5, 2.0, (2, nchan, nant, 1, 2)) * np.exp(2j * np.pi * rng.uniform(size=(2, nchan, nant, 1, 2))))
            ds = VisDataset({'DATA': (('row', 'chan', 'corr'), data), 'WEIGHT_SPECTRUM': (('row', 'chan', 'corr'), weight),
                             'FLAG': (('row', 'chan', 'corr'), flag), 'FLAG_ROW': (('row',), frow),
                             'ANTENNA1': (('row',), dev(ant1)), 'ANTENNA2': (('row',), dev(ant2)), 'UVW': (('row', 'uvw'), uvw)},
                            attrs=dict(FIELD_ID=0, DATA_DESC_ID=b, SCAN_NUMBER=t))
            out = single_stokes(ds=ds, jones=jones, opts=opts, freq=freq, chan_width=width, cell_rad=CELL, utime=utime,
                                tbin_idx=tbin_idx, tbin_counts=tbin_counts, radec=RADEC, antpos=np.zeros((nant, 3)),
                                poltype='linear')
            assert all(out[k].values.is_cuda for k in ('VIS', 'WEIGHT', 'MASK', 'UVW', 'BEAM'))
            got.append(out)
            vis, wgt, mask, _ = stokes_vis(data, ant1, ant2, tbin_idx, tbin_counts, 'linear', 'I', weight=weight, flag=flag,
                                           frow=frow, jones=jones, precision='double', chan_average=n)
            favg = average_freq(freq, width, n)[0]
            npix = int(np.deg2rad(FOV * 1.1) / CELL)
            axis = (-(npix // 2) + np.arange(npix)) * np.rad2deg(CELL)
            hand.append(VisDataset(
                {'FREQ': (('chan',), favg), 'WEIGHT': (('row', 'chan'), wgt), 'UVW': (('row', 'uvw'), uvw),
                 'VIS': (('row', 'chan'), vis), 'MASK': (('row', 'chan'), mask),
                 'BEAM': (('l_beam', 'm_beam'), torch.ones((npix, npix), dtype=torch.float64, device='cuda'))},
                coords={'chan': favg, 'l_beam': axis, 'm_beam': axis},
                attrs=dict(ra=RADEC[0], dec=RADEC[1], freq_out=np.mean(freq), freq_min=freq.min(), freq_max=freq.max(),
                           time_out=np.mean(utime), time_min=utime.min(), time_max=utime.max())))

    def chain(xds):
        rows = concat_row(xds)
        assert len(rows) == 2 and all(d.VIS.shape == (2 * nrow, nchan // n) for d in rows)
        merged = concat_chan(rows, nband_out=1)
        assert len(merged) == 1
        d = merged[0]
        assert d.VIS.shape == (2 * nrow, 2 * nchan // n) and d.VIS.values.is_cuda
        out = image_data_products(d.UVW.values, dev(np.asarray(d.FREQ.values)), d.VIS.values, d.WEIGHT.values,
                                  d.MASK.values, None, nx, ny, 2 * nx, 2 * ny, CELL, CELL, robustness=None, epsilon=eps,
                                  do_wgridding=True, do_psf=False)
        assert all(v.is_cuda for v in out.values())
        return d, out
    dg, og = chain(got)
    dh, oh = chain(hand)
    for name in ('VIS', 'WEIGHT', 'MASK', 'UVW', 'BEAM'):
        assert torch.equal(dg[name].values, dh[name].values), name
    assert np.array_equal(dg.FREQ.values, dh.FREQ.values)
    assert torch.equal(og['WSUM'], oh['WSUM']) and float(og['WSUM'][0]) > 0
    live = dg.MASK.values != 0
    nvis = int(live.sum())
    s = float((dg.WEIGHT.values * dg.VIS.values.abs())[live].sum()) * (1 + eps)
    diff = float((og['DIRTY'] - oh['DIRTY']).abs().max())
    print(f"chain: worst |DIRTY - DIRTY by hand| {diff:.3e}, bound {nvis * sc.EPS['f64'] * s:.3e}; "
          f"max |DIRTY| {float(og['DIRTY'].abs().max()):.3e}")
    assert og['DIRTY'].abs().max() > 0 and diff <= nvis * sc.EPS['f64'] * s
