"""
The init worker's per-chunk conversion on MI355X -- pfb/utils/stokes2vis.py:24-280, with the reference's name and keyword
list (csrc/stokes.hip through utils/stokes.py).

    single_stokes(ds, jones, opts, freq, chan_width, cell_rad, utime, tbin_idx, tbin_counts, radec, antpos, poltype)
        the raw columns of one chunk `ds` to a VisDataset (utils/concat.py) with FREQ, WEIGHT, UVW, VIS, MASK and BEAM:
        what concat_row, concat_chan and image_data_products take.  One kernel: the column arithmetic, the weight form,
        the flags, the Stokes product(s) and, with opts.chan_average > 1, the channel averaging.

`ds` is any object with the columns as attributes that have `.values` or `.data` (a VisDataset, an xarray Dataset
already computed) holding numpy arrays or device tensors, `'FLAG_ROW' in ds`, and FIELD_ID, DATA_DESC_ID, SCAN_NUMBER;
`opts` any object with data_column, flag_column, sigma_column, weight_column, product, precision, chan_average,
max_field_of_view, beam_model and radec.  numpy columns give numpy variables, device tensors give device tensors, and
then nothing but metadata is read on the host.

Where this differs from the reference, by definition:
  * the averaged channels are ceil(nchan / chan_average), the last bin short (the reference re-chunks its result to
    nchan // chan_average channels, which breaks on a remainder);
  * rows and UVW stay in the input's order (africanus.averaging sorts by time, then baseline; a measurement set in the
    standard order is not affected);
  * the caller's arrays are never written;
  * beam_model must be None -- the beam of ones -- anything else is a NotImplementedError (katbeam is not here);
  * opts.product may hold 2 to 4 letters: VIS and WEIGHT then carry a leading product axis;
  * a weight_column 'WEIGHT' must be the row form (nrow, ncorr), any other column (nrow, nchan, ncorr): ValueError.
"""
import numpy as np
import torch

from .concat import VisDataset
from .stokes import average_freq, check_chan_average, stokes_vis


def _column(ds, name):
    """Column `name` of ds as a numpy array or a tensor: ds.NAME.values, else ds.NAME.data, else ds.NAME itself."""
    v = getattr(ds, name)
    if not isinstance(v, (np.ndarray, torch.Tensor)):
        v = v.values if hasattr(v, 'values') else v.data
    return v if isinstance(v, torch.Tensor) else np.asarray(v)


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def single_stokes(ds=None, jones=None, opts=None, freq=None, chan_width=None, cell_rad=None, utime=None, tbin_idx=None,
                  tbin_counts=None, radec=None, antpos=None, poltype=None):
    """stokes2vis.py:24-280 for one chunk: a VisDataset with
        FREQ (chan)   WEIGHT, VIS ([product,] row, chan)   MASK (row, chan)   UVW (row, uvw)   BEAM (l_beam, m_beam)
    coords chan, l_beam, m_beam (degrees, as interp_beam has them) and the reference's attrs: ra, dec, fieldid, ddid,
    scanid, freq_out / freq_min / freq_max -- of the UN-averaged freq, as there --, time_out / time_min / time_max of
    utime, product.

    opts.data_column 'A', 'A+B' or 'A-B'; opts.sigma_column, else opts.weight_column ('WEIGHT': the row weight), else
    ones; opts.flag_column or None; FLAG_ROW where ds has it; autocorrelations are flagged.  jones in QuartiCal's layout
    (ntime, nchan, nant, ndir, 2 or 4) or None.  opts.chan_average = n > 1 averages bins of n channels:
    FREQ and chan are then the bins' mean frequencies.  A string opts.radec, or an array that is not `radec`, and a
    beam_model are a NotImplementedError.  antpos and chan_width (without averaging) are not read."""
    if str(opts.precision).lower() not in ('single', 'double'):
        raise ValueError(f"opts.precision must be 'single' or 'double', got {opts.precision!r}")
    n = check_chan_average(getattr(opts, 'chan_average', 1))
    oradec = getattr(opts, 'radec', None)
    if isinstance(oradec, str):
        raise NotImplementedError("opts.radec as a string: rephasing is not provided (the reference raises here too)")
    if isinstance(oradec, np.ndarray) and not np.array_equal(radec, oradec):
        raise NotImplementedError("opts.radec differs from the field's radec: rephasing is not provided (as in the "
                                  "reference)")
    if getattr(opts, 'beam_model', None) is not None:
        raise NotImplementedError(f"beam_model {opts.beam_model!r}: only None, the beam of ones")

    # crude arithmetic, as the reference has it
    dc = str(opts.data_column).replace(" ", "")
    operator = '+' if '+' in dc else '-' if '-' in dc else None
    dc1, dc2 = dc.split(operator) if operator else (dc, None)
    data = _column(ds, dc1)
    data2 = _column(ds, dc2) if dc2 is not None else None
    frow = _column(ds, 'FLAG_ROW') if 'FLAG_ROW' in ds else None
    flag = _column(ds, opts.flag_column) if opts.flag_column is not None else None
    sigma = weight = None
    if opts.sigma_column is not None:
        sigma = _column(ds, opts.sigma_column)
    elif opts.weight_column is not None:
        weight = _column(ds, opts.weight_column)
        if (weight.ndim == 2) != (opts.weight_column == 'WEIGHT'):
            raise ValueError(f"weight_column {opts.weight_column!r} with {weight.ndim} dimensions: 'WEIGHT' is the row "
                             "weight (nrow, ncorr), any other column a spectrum (nrow, nchan, ncorr)")

    vis, wgt, mask, _ = stokes_vis(data, _column(ds, 'ANTENNA1'), _column(ds, 'ANTENNA2'), tbin_idx, tbin_counts, poltype,
                                   opts.product, data2=data2, operator=operator, sigma=sigma, weight=weight, flag=flag,
                                   frow=frow, jones=jones, precision=opts.precision, chan_average=n)

    freq = _host(freq).astype(np.float64)
    utime = _host(utime)
    if freq.ndim != 1 or freq.size != data.shape[1]:
        raise ValueError(f"freq must hold the data's {data.shape[1]} channels")
    freq_avg = freq if n == 1 else average_freq(freq, chan_width, n)[0]

    npix = int(np.deg2rad(opts.max_field_of_view * 1.1) / cell_rad)
    cell_deg = np.rad2deg(cell_rad)
    l_beam = (-(npix // 2) + np.arange(npix)) * cell_deg
    beam = np.ones((npix, npix), dtype=np.float64)
    if isinstance(vis, torch.Tensor):
        beam = torch.from_numpy(beam).to(vis.device)

    lead = ('product',) if vis.ndim == 3 else ()
    data_vars = {
        'FREQ': (('chan',), freq_avg),
        'WEIGHT': (lead + ('row', 'chan'), wgt),
        'UVW': (('row', 'uvw'), _column(ds, 'UVW')),
        'VIS': (lead + ('row', 'chan'), vis),
        'MASK': (('row', 'chan'), mask),
        'BEAM': (('l_beam', 'm_beam'), beam),
    }
    coords = {'chan': (('chan',), freq_avg), 'l_beam': (('l_beam',), l_beam), 'm_beam': (('m_beam',), l_beam.copy())}
    attrs = {
        'ra': radec[0],
        'dec': radec[1],
        'fieldid': ds.FIELD_ID,
        'ddid': ds.DATA_DESC_ID,
        'scanid': ds.SCAN_NUMBER,
        'freq_out': np.mean(freq),
        'freq_min': freq.min(),
        'freq_max': freq.max(),
        'time_out': np.mean(utime),
        'time_min': utime.min(),
        'time_max': utime.max(),
        'product': opts.product,
    }
    return VisDataset(data_vars, coords=coords, attrs=attrs)
