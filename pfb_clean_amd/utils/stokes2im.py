"""
fastim on MI355X -- the raw columns of one (scan, band, time chunk) to Stokes residual images:
pfb/utils/stokes2im.py::single_stokes_image with the reference's keyword list, and the loop of its worker over the
chunks of a dataset (pfb/workers/fastim.py:318-368).

    single_stokes_image   one chunk: (residual, attrs)
    chunk_plan            host only: the row, time and channel slices and the bin tables of every (time chunk, band)
    stokes_image_cube     every chunk of one dataset: residual (ntime_out, nband_out[, nprod], nx, ny), wsum, rms

The chain of a chunk, all on the device:

    stokes_vis (utils/stokes.py)                          vis, wgt, mask of the product(s), one kernel
    compute_counts(..., float64) [filter_extreme_counts]  with a robustness
    counts_to_weights                                     imwgt, fp64
    eval_coeffs_to_slice per band, _im2vis_impl           with a model, on the model's own grid and cell
    pfb_imw_residual_weigh (csrc/imweight.hip)            (vis - model_vis) * mask, wgt *= imwgt, sum wgt[mask != 0]:
                                                          one pass for the reference's three (stokes2im.py:268, 279-295)
    WgridPlan.vis2dirty, divide_by_n=False                one plan and one call for all products
    pfb_bandsum_stats, nband = 1, nset = nprod            np.std of every plane

wsum and rms stay on the device as records; single_stokes_image reads them in one copy, stokes_image_cube gathers the
chunks' records on the device and reads them once at the end.  numpy in gives numpy out, tensors in give tensors out;
there is no CPU path.  Nothing is written to disk.
"""
import ctypes as C
import datetime
from collections.abc import Mapping

import numpy as np
import torch

from .. import _dev, _lib
from ..operators import gridder
from . import comps, cycle, weighting
from . import stokes as _stokes

MAX_PROD = 4                    # PFB_IMW_MAX_PROD
UNIX_OFFSET = 3506716800.0      # seconds from the MJD epoch to the Unix epoch: casacore's quantity(..).to_unix_time()
OPTS = ('precision', 'product', 'robustness', 'filter_extreme_counts', 'filter_nbox', 'filter_level', 'nvthreads',
        'epsilon', 'do_wgridding', 'double_accum', 'l2reweight_dof', 'target')


# ------------------------------------------------------------------------------------------------------ the kernel
def residual_weigh(vis, wgt, mask, model_vis=None, model_of=None, imwgt=None):
    """pfb_imw_residual_weigh on device tensors, IN PLACE: vis (nprod, ...) complex and wgt (nprod, ...) of its real
    type, mask uint8 and imwgt float64 (or None) of one plane's shape, model_vis (nmodel, ...) of vis's type with
    model_of[p] the model plane of product p or -1.  Returns the nprod float64 device sums of wgt over mask != 0."""
    if vis.dtype not in _dev.REAL_OF or wgt.dtype != _dev.REAL_OF[vis.dtype] or wgt.shape != vis.shape:
        raise TypeError("vis must be complex64 or complex128 and wgt of its real type and shape")
    nprod = int(vis.shape[0])
    n = vis[0].numel() if nprod else 0
    if not 1 <= nprod <= MAX_PROD:
        raise ValueError(f"{nprod} planes: 1 to {MAX_PROD} products share a call")
    if not (vis.is_contiguous() and wgt.is_contiguous()):
        raise ValueError("vis and wgt are written in place and must be contiguous")
    if mask.dtype != torch.uint8 or mask.numel() != n or not mask.is_contiguous():
        raise ValueError("mask must be a contiguous uint8 plane")
    if imwgt is not None and (imwgt.dtype != torch.float64 or imwgt.numel() != n or not imwgt.is_contiguous()):
        raise TypeError("imwgt must be a contiguous float64 plane, whatever the type of wgt")
    table = [-1] * nprod if model_of is None else [int(m) for m in model_of]
    nmodel = 0
    if model_vis is not None:
        if model_vis.dtype != vis.dtype or not model_vis.is_contiguous() or model_vis[0].numel() != n:
            raise TypeError("model_vis must be contiguous planes of the type and shape of vis's")
        nmodel = int(model_vis.shape[0])
    if len(table) != nprod or any(m >= nmodel for m in table):
        raise ValueError(f"model_of {table} does not map {nprod} planes into {nmodel} model planes")
    rec = torch.empty(nprod, dtype=torch.float64, device=vis.device)
    _lib.check(_lib.load().pfb_imw_residual_weigh(
        _dev.code(wgt.dtype), nprod, _dev.ptr(vis), _dev.ptr(model_vis), nmodel, (C.c_int * nprod)(*table),
        _dev.ptr(mask), _dev.ptr(imwgt), n, _dev.ptr(wgt),
        _dev.ptr(rec), weighting._work(), _dev.stream()))
    return rec


# ---------------------------------------------------------------------------------------------------- one chunk
def _check_opts(opts):
    missing = [k for k in OPTS if not hasattr(opts, k)]
    if missing:
        raise AttributeError(f"opts lacks {missing}")
    if opts.l2reweight_dof:
        raise NotImplementedError(
            "l2reweight_dof: the reference's branch cannot run (stokes2im.py:275 reads a name that does not exist: "
            "NameError) and the weights it would compute are not used afterwards")
    if opts.target is not None:
        raise NotImplementedError("target: only target=None; the image centre is given by the keywords x0, y0")
    if str(opts.precision).lower() not in ('single', 'double'):
        raise ValueError(f"precision must be 'single' or 'double', got {opts.precision!r}")


def _models(mds, letters):
    """[(plane, model)] of the products that have a model: `mds` is the model of a one-letter product, or a mapping
    from letter to model (a letter without an entry has nothing subtracted)."""
    if mds is None:
        return []
    if isinstance(mds, Mapping):
        unknown = [k for k in mds if k not in letters]
        if unknown:
            raise ValueError(f"mds holds models for {unknown}, which are not among the products {letters}")
        return [(p, mds[k]) for p, k in enumerate(letters) if k in mds and mds[k] is not None]
    if len(letters) != 1:
        raise ValueError("a product of several letters takes its models as a mapping from letter to model")
    return [(0, mds)]


def _model_vis(m, uvw, freq, fhost, time_out, start, stop, fbin_idx, fbin_counts, rdt, opts):
    """The model visibilities (nrow, nchan) of one model: eval_coeffs_to_slice per band at (time_out, mean of the
    band's frequencies), on the model's own grid, then _im2vis_impl (stokes2im.py:220-266)."""
    nxm, nym = int(m.npix_x), int(m.npix_y)
    coeffs = _dev.to_dev(np.asarray(m.coefficients.values) if not isinstance(m.coefficients.values, torch.Tensor)
                         else m.coefficients.values)
    loc = [v.values if isinstance(v.values, torch.Tensor) else np.asarray(v.values) for v in (m.location_x, m.location_y)]
    params = [str(p) for p in (m.params.values.tolist() if hasattr(m.params.values, 'tolist') else m.params.values)]
    geom = (nxm, nym, m.cell_rad_x, m.cell_rad_y, m.center_x, m.center_y)
    model = torch.zeros((start.size, nxm, nym), dtype=rdt, device=uvw.device)
    for b in range(start.size):
        if stop[b] > start[b]:
            fout = np.mean(fhost[start[b]:stop[b]])
            model[b] = comps.eval_coeffs_to_slice(time_out, fout, coeffs, loc[0], loc[1], m.parametrisation, params,
                                                  m.texpr, m.fexpr, *geom, *geom, dtype=rdt)
    return gridder._im2vis_impl(uvw, freq, model, m.cell_rad_x, m.cell_rad_y, fbin_idx, fbin_counts, x0=m.center_x,
                                y0=m.center_y, epsilon=opts.epsilon, flip_v=False, do_wgridding=opts.do_wgridding,
                                divide_by_n=False)


def _single_stokes_image_dev(data, data2, operator, ant1, ant2, uvw, frow, flag, sigma, weight, mds, jones, opts, nx, ny,
                             freq, cell_rad, time_out, tbin_idx, tbin_counts, fbin_idx, fbin_counts, poltype, x0=0.0,
                             y0=0.0, freq_host=None):
    """The device level of single_stokes_image: columns of either kind in (they go to the device as they are), device
    tensors out and no host read of a result: (residual, wsum, rms) with residual (nprod, nx, ny) in the working
    type of opts.precision and wsum, rms (nprod,) float64 -- nprod = 1 for a one-letter product.  freq_host: the
    frequencies as a host array, where the caller has them (a model's bands are averaged on the host)."""
    _check_opts(opts)
    letters = _stokes.product_letters(opts.product) or (str(opts.product),)
    precision = str(opts.precision).lower()
    nx, ny = int(nx), int(ny)
    ud, fd = _dev.uvw_freq(uvw, freq)
    up = _dev.to_dev
    vis, wgt, mask, _ = _stokes.stokes_vis(up(data), up(ant1), up(ant2), tbin_idx, tbin_counts, poltype, letters,
                                             data2=up(data2), operator=operator, sigma=up(sigma), weight=up(weight),
                                             flag=up(flag), frow=up(frow), jones=up(jones), precision=precision)
    rdt = wgt.dtype
    nprod, nrow, nchan = (int(n) for n in vis.shape)
    if tuple(ud.shape) != (nrow, 3) or fd.numel() != nchan:
        raise ValueError(f"uvw {tuple(ud.shape)} / freq {tuple(fd.shape)} do not match data {(nrow, nchan)}")
    # ---- imaging weights
    imwgt = None
    if opts.robustness is not None and nrow * nchan:
        counts = weighting.compute_counts(ud, fd, mask, nx, ny, cell_rad, cell_rad, torch.float64,
                                          ngrid=max(1, int(opts.nvthreads)))
        if opts.filter_extreme_counts:
            counts = weighting.filter_extreme_counts(counts, nbox=opts.filter_nbox, nlevel=opts.filter_level)
        imwgt = weighting.counts_to_weights(counts, ud, fd, nx, ny, cell_rad, cell_rad, opts.robustness)
    # ---- the models
    models = _models(mds, letters)
    model_vis, model_of = None, [-1] * nprod
    if models and nrow * nchan:
        start, stop = gridder._bins(fbin_idx, fbin_counts, nchan, 'fbin')
        fhost = gridder._host_floats(freq if freq_host is None else freq_host)
        planes = []
        for p, m in models:
            model_of[p] = len(planes)
            planes.append(_model_vis(m, ud, fd, fhost, time_out, start, stop, fbin_idx, fbin_counts, rdt, opts))
        model_vis = torch.stack(planes)
    # ---- residual visibilities, the weight product and its masked sums: one pass, in place on this call's own arrays
    # (without a model and without imaging weights it only sums: wsum in fp64 whatever the precision)
    wsum = residual_weigh(vis, wgt, mask, model_vis, model_of, imwgt)
    # ---- the image: this chunk's plan, built directly and closed after use, its tables the geometry's
    gdt = torch.float64 if opts.double_accum else rdt
    plan = gridder.WgridPlan(ud, fd, mask, nx, ny, cell_rad, cell_rad, x0, y0, opts.epsilon, opts.do_wgridding, gdt)
    try:
        residual = plan.vis2dirty(vis.to(_dev.CPLX_OF[gdt]), wgt.to(gdt), False).to(rdt).contiguous()
    finally:
        plan.close()
    # ---- np.std of every plane
    st = cycle._stats(residual, 1, nprod, nx * ny, None, None)
    return residual, wsum, torch.sqrt(st[:, 2] / st[:, 0])


def _host_scalar(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _out_dtype(dtype):
    return weighting._real_dtype(np.float32 if dtype is None else dtype)


def single_stokes_image(data=None, data2=None, operator=None, ant1=None, ant2=None, uvw=None, frow=None, flag=None,
                        sigma=None, weight=None, mds=None, jones=None, opts=None, nx=None, ny=None, freq=None,
                        cell_rad=None, utime=None, tbin_idx=None, tbin_counts=None, fbin_idx=None, fbin_counts=None,
                        radec=None, antpos=None, poltype=None, fieldid=None, ddid=None, scanid=None, fds_store=None,
                        bandid=None, timeid=None, wid=None, x0=0.0, y0=0.0, out_dtype=None):
    """pfb/utils/stokes2im.py:40-358 with the reference's keyword list: (residual, attrs) of one chunk.

    The columns are arrays or device tensors (the reference takes dask collections): data [data2 with operator '+' /
    '-'] (nrow, nchan, ncorr), flag of that shape, frow (nrow,), sigma or weight ((nrow, nchan, ncorr), weight also
    (nrow, ncorr)), ant1, ant2, uvw (nrow, 3), freq (nchan,), utime, jones in QuartiCal's layout, tbin_idx / tbin_counts
    the rows of every unique time, fbin_idx / fbin_counts the channels of every model band.  `opts` is any object with
    the attributes precision, product, robustness, filter_extreme_counts, filter_nbox, filter_level, nvthreads, epsilon,
    do_wgridding, double_accum, l2reweight_dof, target; `mds` any object with coefficients.values, location_x.values,
    location_y.values, parametrisation, params.values, texpr, fexpr, npix_x/y, cell_rad_x/y, center_x/y.  fds_store, wid
    and antpos are accepted and not used; fieldid, ddid, scanid, bandid and timeid are copied into the attributes.

    residual is (nx, ny) float32 as the reference stores it (`out_dtype` float64 keeps the working type of 'double');
    attrs holds the reference's keys: ra, dec, x0, y0, cell_rad, fieldid, ddid, scanid, freq_out, freq_min, freq_max,
    bandid, time_out, time_min, time_max, timeid, product, utc, wsum, rms -- wsum and rms Python floats read from the
    device in one copy, utc from time_out - 3506716800 seconds.

    Differences from the reference, by definition:
      * a product of 2 to 4 letters works as in stokes_vis: residual (nprod, nx, ny), wsum and rms lists per product,
        from one stokes_vis pass, one counts grid, one imwgt and one gridder plan; `mds` may then be a mapping from
        letter to model, and planes without an entry have nothing subtracted;
      * filter_extreme_counts=True works, through filter_extreme_counts(counts, nbox=opts.filter_nbox,
        nlevel=opts.filter_level) on the summed counts (the reference's call is a TypeError: it passes `nlevel` to a
        function whose keyword is `level`);
      * a true l2reweight_dof is a NotImplementedError: the reference's branch cannot run (NameError at line 275) and
        its result is unused there;
      * target=None only, anything else is a NotImplementedError (the reference's branch reads names that do not
        exist); the new keywords x0, y0 give the image centre;
      * fbin_idx is shifted by its minimum, as _im2vis_impl shifts it, for the band frequencies too (the reference
        indexes the chunk's freq with the unshifted fbin_idx);
      * the caller's data, weight and tbin_idx are never written (the reference combines data2 into data, multiplies
        imwgt into weight and rebases tbin_idx in place);
      * the chunk's gridder plan is built directly and closed after use; it never enters the plan cache;
      * a chunk with no unflagged visibility gives zeros, wsum == 0 and rms == 0, without an error;
      * nothing is written to disk: the reference's zarr store is the caller's."""
    if opts is None or data is None:
        raise TypeError("data and opts are required")
    odt = _out_dtype(out_dtype)
    ut = _host_scalar(utime).astype(np.float64)
    fh = _host_scalar(freq).astype(np.float64)
    time_out = float(np.mean(ut))
    residual, wsum, rms = _single_stokes_image_dev(data, data2, operator, ant1, ant2, uvw, frow, flag, sigma, weight, mds,
                                                   jones, opts, nx, ny, freq, cell_rad, time_out, tbin_idx, tbin_counts,
                                                   fbin_idx, fbin_counts, poltype, x0, y0, fh)
    record = torch.stack([wsum, rms]).cpu().tolist()            # the one copy to the host
    stacked = _stokes.product_letters(opts.product) is not None
    residual = residual.to(odt)
    if not stacked:
        residual, record = residual[0], [record[0][0], record[1][0]]
    rd = None if radec is None else _host_scalar(radec)
    utc = (datetime.datetime(1970, 1, 1) + datetime.timedelta(seconds=time_out - UNIX_OFFSET)).strftime('%Y-%m-%d %H:%M:%S')
    attrs = {'ra': None if rd is None else rd[0], 'dec': None if rd is None else rd[1], 'x0': x0, 'y0': y0,
             'cell_rad': cell_rad, 'fieldid': fieldid, 'ddid': ddid, 'scanid': scanid, 'freq_out': float(np.mean(fh)),
             'freq_min': float(fh.min()), 'freq_max': float(fh.max()), 'bandid': bandid, 'time_out': time_out,
             'time_min': float(ut.min()), 'time_max': float(ut.max()), 'timeid': timeid, 'product': opts.product,
             'utc': utc, 'wsum': record[0], 'rms': record[1]}
    return _dev.host_like(residual, data), attrs


# ------------------------------------------------------------------------------------------------ the worker's loop
def _mapping(m, name):
    try:
        idx, cnt = m['start_indices'], m['counts']
    except (KeyError, TypeError, IndexError):
        raise ValueError(f"{name} must hold 'start_indices' and 'counts'") from None
    return gridder._host_ints(idx, name + ' start_indices'), gridder._host_ints(cnt, name + ' counts')


def chunk_plan(time_mapping, row_mapping, freq_mapping, channels_per_grid_image, channels_per_degrid_image):
    """pfb/workers/fastim.py:318-368, host only: one dict per (ti, fi), time chunks outermost, of

        ti, fi      the chunk's output time and band
        It          slice(tlow, tlow + tcounts) into the unique times (and the Jones terms' time axis)
        Irow        slice(ridx[0], ridx[-1] + rcnts[-1]) into the rows
        Inu         slice(fidx.min(), fidx.min() + sum(fcnts)) into the channels
        ridx, rcnts the rows of the chunk's unique times (row_mapping[It]): the chunk's tbin_idx / tbin_counts
        fidx, fcnts the channels of the chunk's model bands: its fbin_idx / fbin_counts

    Every mapping holds 'start_indices' and 'counts'.  channels_per_grid_image in (0, -1, None) means all channels;
    fbins_per_band = int(cpgi / cpdi) bins of freq_mapping go onto one image and nband = ceil(nbins / fbins_per_band)."""
    tidx, tcnt = _mapping(time_mapping, 'time_mapping')
    ridx_all, rcnt_all = _mapping(row_mapping, 'row_mapping')
    fidx_all, fcnt_all = _mapping(freq_mapping, 'freq_mapping')
    nbandi = fidx_all.size
    nfreqs = int(np.sum(fcnt_all))
    cpgi = nfreqs if channels_per_grid_image in (0, -1, None) else channels_per_grid_image
    fbins_per_band = int(cpgi / channels_per_degrid_image)
    if fbins_per_band < 1:
        raise ValueError(f"channels_per_grid_image {cpgi} holds no bin of {channels_per_degrid_image} channels")
    nband = int(np.ceil(nbandi / fbins_per_band))
    chunks = []
    for ti, (tlow, tcounts) in enumerate(zip(tidx.tolist(), tcnt.tolist())):
        It = slice(tlow, tlow + tcounts)
        ridx, rcnts = ridx_all[It], rcnt_all[It]
        Irow = slice(int(ridx[0]), int(ridx[-1] + rcnts[-1]))
        for fi in range(nband):
            idx0 = fi * fbins_per_band
            idxf = min((fi + 1) * fbins_per_band, nfreqs)
            fidx, fcnts = fidx_all[idx0:idxf], fcnt_all[idx0:idxf]
            Inu = slice(int(fidx.min()), int(fidx.min() + np.sum(fcnts)))
            chunks.append(dict(ti=ti, fi=fi, It=It, Irow=Irow, Inu=Inu, ridx=ridx, rcnts=rcnts, fidx=fidx, fcnts=fcnts))
    return chunks


def stokes_image_cube(data, ant1, ant2, uvw, freq, utime, time_mapping, row_mapping, freq_mapping, opts, nx, ny, cell_rad,
                      poltype, data2=None, operator=None, frow=None, flag=None, sigma=None, weight=None, jones=None,
                      mds=None, channels_per_grid_image=None, channels_per_degrid_image=1, x0=0.0, y0=0.0,
                      out_dtype=None):
    """The loop of the fastim worker over one dataset (fastim.py:318-368 around single_stokes_image): every (time chunk,
    band) of chunk_plan(time_mapping, row_mapping, freq_mapping, channels_per_grid_image, channels_per_degrid_image)
    imaged from the dataset's columns, sliced as the worker slices them -- rows Irow, channels Inu, unique times It, and
    Jones terms (QuartiCal's layout) on their time and channel axes by It and Inu.

    Returns (residual, wsum, rms): residual (ntime_out, nband_out[, nprod], nx, ny), float32 unless `out_dtype`, and
    wsum, rms (ntime_out, nband_out[, nprod]) float64.  The columns go to the device once; the chunks' records are
    gathered on the device and read once at the end (numpy in), or not at all (tensors in give tensors out).  No plan of
    a chunk enters the plan cache; the chunks of one geometry share its correction tables."""
    _check_opts(opts)
    odt = _out_dtype(out_dtype)
    chunks = chunk_plan(time_mapping, row_mapping, freq_mapping, channels_per_grid_image, channels_per_degrid_image)
    stacked = _stokes.product_letters(opts.product) is not None
    nprod = len(_stokes.product_letters(opts.product) or 'I')
    ntime, nband = chunks[-1]['ti'] + 1, chunks[-1]['fi'] + 1
    up = _dev.to_dev
    cols = {k: up(v) for k, v in dict(data=data, data2=data2, ant1=ant1, ant2=ant2, uvw=uvw, frow=frow, flag=flag,
                                      sigma=sigma, weight=weight, jones=jones, freq=freq).items()}
    ut, fh = _host_scalar(utime).astype(np.float64), _host_scalar(freq).astype(np.float64)
    dev = cols['uvw'].device
    residual = torch.empty((ntime, nband, nprod, int(nx), int(ny)), dtype=odt, device=dev)
    record = torch.empty((2, ntime, nband, nprod), dtype=torch.float64, device=dev)

    def cut(name, rows, chans=None):
        t = cols[name]
        if t is None:
            return None
        return t[rows] if chans is None or t.ndim < 3 else t[rows, chans]

    for c in chunks:
        Irow, Inu, It = c['Irow'], c['Inu'], c['It']
        res, wsum, rms = _single_stokes_image_dev(
            cut('data', Irow, Inu), cut('data2', Irow, Inu), operator, cut('ant1', Irow), cut('ant2', Irow),
            cut('uvw', Irow), cut('frow', Irow), cut('flag', Irow, Inu), cut('sigma', Irow, Inu),
            cut('weight', Irow, Inu), mds, cut('jones', It, Inu), opts, nx, ny, cols['freq'][Inu], cell_rad,
            float(np.mean(ut[It])), c['ridx'], c['rcnts'], c['fidx'], c['fcnts'], poltype, x0, y0, fh[Inu])
        residual[c['ti'], c['fi']] = res
        record[0, c['ti'], c['fi']] = wsum
        record[1, c['ti'], c['fi']] = rms
    if not stacked:
        residual, record = residual[:, :, 0], record[..., 0]
    record = _dev.host_like(record, data)
    return _dev.host_like(residual, data), record[0], record[1]
