"""
Band and time concatenation of the grid worker's input datasets on MI355X -- pfb/utils/misc.py:776-1067 and the image
geometry of pfb/workers/grid.py:226-285, with the reference's names and signatures (csrc/visconcat.hip).

    VisDataset                    the package's in-memory dataset (what dds2cubes and hessian_xds accept)
    sum_overlap(ufreq, flow, fhigh, **kwargs)   the weighted mean of the sources' visibilities per output channel
    _sum_beam(nx, ny, btype, **kwargs), sum_beam(xds)   the beams' mean, weighted by every source's sum of weights
    concat_row(xds)               the datasets of one band merged over time
    concat_chan(xds, nband_out)   the datasets of one time re-binned onto nband_out imaging bands
    image_geometry(xds, ...)      cell size and image / PSF sizes from the longest baseline

numpy in gives numpy out, tensors in give tensors out; there is no CPU path.  With tensors in, VIS, WEIGHT, MASK, UVW and
BEAM never cross to the host: what is read there is metadata (frequencies, times, the channel map).

Where this differs from the reference, by definition:
  * masko is 0 / 1 for any number of sources (the reference's uint8 count wraps at 256 sources);
  * concat_chan raises ValueError, naming the bin and the time, where no dataset is selected (the reference: IndexError);
  * sources of one sum_overlap must share nrow (the reference broadcasts or fails inside numpy).
"""
import ctypes as C

import numpy as np
import torch

from .. import _dev, _lib

LIGHTSPEED = 299792458.0
BATCH = 8           # PFB_VIS_BATCH


# ------------------------------------------------------------------------------------------------- the dataset
class Variable:
    """A named array of a VisDataset: `.values` (a device tensor or numpy array, `.data` the same), `.dims`."""
    __slots__ = ('dims', 'values')

    def __init__(self, dims, values):
        self.dims = tuple(dims)
        self.values = values if isinstance(values, (np.ndarray, torch.Tensor)) else np.asarray(values)

    data = property(lambda self: self.values)
    dtype = property(lambda self: self.values.dtype)
    shape = property(lambda self: tuple(self.values.shape))
    ndim = property(lambda self: len(self.values.shape))
    size = property(lambda self: int(np.prod(self.values.shape, dtype=np.int64)))

    def __repr__(self):
        return f"Variable({self.dims}, {self.dtype}, {self.shape})"


class VisDataset(dict):
    """A small dict of Variables with attributes: ds[name], name in ds, ds.NAME, ds.attribute.  data_vars and coords
    map a name to (dims, array), a Variable or (for a coordinate) a 1-D array; attrs become plain attributes, also kept
    in `ds.attrs`.  A dimension without a coordinate (row) reads as its index range, as in xarray."""

    def __init__(self, data_vars=None, coords=None, attrs=None):
        super().__init__()
        object.__setattr__(self, 'attrs', dict(attrs or {}))
        for name, v in (coords or {}).items():
            self[name] = v if isinstance(v, (Variable, tuple)) else ((name,), v)
        for name, v in (data_vars or {}).items():
            self[name] = v

    def __setitem__(self, name, v):
        if isinstance(v, tuple):
            v = Variable(*v)
        if not isinstance(v, Variable):
            raise TypeError(f"{name}: a Variable or (dims, array) expected")
        super().__setitem__(name, v)

    def __getattr__(self, name):
        if name in self:
            return self[name]
        attrs = object.__getattribute__(self, 'attrs')
        if name in attrs:
            return attrs[name]
        for v in self.values():
            if name in v.dims:
                return Variable((name,), np.arange(v.shape[v.dims.index(name)]))
        raise AttributeError(name)

    def __setattr__(self, name, value):
        self.attrs[name] = value


def _host(a):
    """Metadata (frequencies, beam axes) as a numpy array."""
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _work():
    return _dev.ptr(_dev.scratch()[0])


def _ptrs(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


# ------------------------------------------------------------------------------------------------- sum_overlap
def channel_map(freqs, ufreq):
    """(nds, nchan_out) int32: the channel of source i at output channel c or -1, from np.intersect1d(nu_i, ufreq,
    assume_unique=True, return_indices=True) as the reference calls it."""
    ufreq = _host(ufreq)
    cmap = np.full((len(freqs), ufreq.size), -1, np.int32)
    for i, nu in enumerate(freqs):
        _, idx0, idx1 = np.intersect1d(_host(nu), ufreq, assume_unique=True, return_indices=True)
        cmap[i, idx1] = idx0
    return cmap


def _sum_overlap_dev(vis, wgt, mask, cmap):
    """Device tensors in and out: (viso, wgto, masko) of the sources vis[i], wgt[i], mask[i] under the host map cmap."""
    nds, nchan_out = cmap.shape
    cdt = vis[0].dtype
    if cdt not in _dev.REAL_OF:
        raise TypeError(f"vis must be complex64 or complex128, got {cdt}")
    rdt = _dev.REAL_OF[cdt]
    nrow = int(vis[0].shape[0])
    for i in range(nds):
        if vis[i].dtype != cdt or wgt[i].dtype != rdt:
            raise TypeError(f"source {i}: vis / wgt must be {cdt} / {rdt} like source 0")
        if vis[i].ndim != 2 or wgt[i].shape != vis[i].shape or mask[i].shape != vis[i].shape:
            raise ValueError(f"source {i}: vis, wgt and mask must be (nrow, nchan) arrays of one shape")
        if int(cmap[i].max(initial=-1)) >= vis[i].shape[1]:
            raise ValueError(f"source {i}: the channel map reaches past its {vis[i].shape[1]} channels")
    dev = vis[0].device
    viso = torch.zeros((nrow, nchan_out), dtype=cdt, device=dev)
    wgto = torch.zeros((nrow, nchan_out), dtype=rdt, device=dev)
    masko = torch.zeros((nrow, nchan_out), dtype=torch.uint8, device=dev)
    live = [i for i in range(nds) if vis[i].shape[1]]               # a source without channels adds nothing
    vis, wgt, mask, cmap, nds = [vis[i] for i in live], [wgt[i] for i in live], [mask[i] for i in live], cmap[live], len(live)
    if nrow * nchan_out == 0 or nds == 0:
        return viso, wgto, masko
    map_d = torch.from_numpy(np.ascontiguousarray(cmap, np.int32)).to(dev)
    nrows = (C.c_size_t * nds)(*[int(v.shape[0]) for v in vis])
    nchans = (C.c_int * nds)(*[int(v.shape[1]) for v in vis])
    _lib.check(_lib.load().pfb_vis_sum_overlap(_dev.code(rdt), nds, _ptrs(vis), _ptrs(wgt), _ptrs(mask), nrows, nchans,
                                               _dev.ptr(map_d), nrow, nchan_out, _dev.ptr(viso), _dev.ptr(wgto),
                                               _dev.ptr(masko), _dev.stream()))
    return viso, wgto, masko


def sum_overlap(ufreq, flow, fhigh, **kwargs):
    """misc.py:1030-1067: {'viso', 'wgto', 'masko'}, each (nrow, ufreq.size), of the sources vis{i}, wgt{i}, mask{i},
    freq{i}: viso = sum vis wgt mask / sum wgt mask where any source is unflagged, wgto = sum wgt mask, masko 0 / 1;
    exactly 0 where masko == 0.  Summed in source order in the data's type.  flow and fhigh are unused, as in the
    reference."""
    nitems = len(kwargs) // 4
    vis = [_dev.to_dev(kwargs[f'vis{i}']) for i in range(nitems)]
    wgt = [_dev.to_dev(kwargs[f'wgt{i}']) for i in range(nitems)]
    mask = [_dev.byte_mask(kwargs[f'mask{i}'], vis[i].shape, f'mask{i}') for i in range(nitems)]
    cmap = channel_map([kwargs[f'freq{i}'] for i in range(nitems)], ufreq)
    like = kwargs['vis0']
    viso, wgto, masko = _sum_overlap_dev(vis, wgt, mask, cmap)
    return {'viso': _dev.host_like(viso, like), 'wgto': _dev.host_like(wgto, like), 'masko': _dev.host_like(masko, like)}


# ---------------------------------------------------------------------------------------------------- sum_beam
def weight_sums(wgts):
    """The device record of the sources' sums of ALL their weights (no mask, as the reference has it): (nds,) float64."""
    lib = _lib.load()
    rec = torch.zeros(len(wgts), dtype=torch.float64, device=wgts[0].device)
    for i, w in enumerate(wgts):
        if w.numel():
            _lib.check(lib.pfb_vis_weight_sums(_dev.code(w.dtype), _dev.ptr(w), w.numel(), _dev.ptr(rec) + 8 * i, _work(),
                                               _dev.stream()))
    return rec


def _sum_beam_dev(beams, wgts, shape, bdt):
    beams = [b if b.dtype == bdt else b.to(bdt) for b in beams]
    for i, b in enumerate(beams):
        if tuple(b.shape) != tuple(shape):
            raise ValueError(f"beam{i} is {tuple(b.shape)}, not {tuple(shape)}")
    out = torch.zeros(tuple(shape), dtype=bdt, device=_dev.require_device())
    if beams and out.numel():
        rec = weight_sums(wgts)
        _lib.check(_lib.load().pfb_beam_combine(_dev.code(bdt), len(beams), _ptrs(beams), _dev.ptr(rec), out.numel(),
                                                _dev.ptr(out), _dev.stream()))
    return out


def _sum_beam(nx, ny, btype, **kwargs):
    """misc.py:1009-1028: {'beam'}: sum_i wgt{i}.sum() beam{i}, divided by sum_i wgt{i}.sum() where that is not zero,
    of type btype (float32 / float64).  The sums stay on the device."""
    from .weighting import _real_dtype
    bdt = _real_dtype(btype)
    nitems = len(kwargs) // 2
    beams = [_dev.to_dev(kwargs[f'beam{i}']) for i in range(nitems)]
    wgts = [_dev.to_dev(kwargs[f'wgt{i}']) for i in range(nitems)]
    out = _sum_beam_dev(beams, wgts, (int(nx), int(ny)), bdt)
    return {'beam': _dev.host_like(out, kwargs['beam0']) if nitems else out}


def sum_beam(xds):
    """misc.py:990-1007: the weighted mean of the BEAMs of xds, each weighted by the sum of its WEIGHT."""
    nx, ny = xds[0].BEAM.shape
    kwargs = {}
    for i, ds in enumerate(xds):
        kwargs[f'beam{i}'] = ds.BEAM.values
        kwargs[f'wgt{i}'] = ds.WEIGHT.values
    return _sum_beam(nx, ny, xds[0].BEAM.dtype, **kwargs)['beam']


# -------------------------------------------------------------------------------------------------- concat_row
def _cat_rows(arrays):
    """The arrays joined along their first axis, on the device; in the kind of the first."""
    return _dev.host_like(torch.cat([_dev.to_dev(a) for a in arrays], dim=0), arrays[0])


def concat_row(xds):
    """misc.py:776-857: per band one dataset whose WEIGHT, VIS, MASK and UVW are those of the band's datasets joined
    along row in the order given, BEAM their sum_beam, everything else the band's first dataset's; xds itself when it
    holds one time."""
    times_in = np.unique([ds.time_out for ds in xds])
    freqs = np.unique([ds.freq_out for ds in xds])
    if times_in.size == 1:
        return xds
    xds_out = []
    for nu in freqs:
        xdsb = [ds for ds in xds if ds.freq_out == nu]
        first = xdsb[0]
        data_vars = {name: (first[name].dims, _cat_rows([ds[name].values for ds in xdsb]))
                     for name in ('WEIGHT', 'VIS', 'MASK', 'UVW')}
        data_vars['BEAM'] = (('l_beam', 'm_beam'), sum_beam(xdsb))
        data_vars['FREQ'] = (first.FREQ.dims, first.FREQ.values)
        coords = {'chan': (('chan',), first.chan.values), 'l_beam': (('l_beam',), first.l_beam.values),
                  'm_beam': (('m_beam',), first.m_beam.values)}
        attrs = {
            'dec': first.dec,
            'ra': first.ra,
            'time_out': np.round(np.mean(np.array([ds.time_out for ds in xdsb])), 5),
            'time_max': np.array([ds.time_max for ds in xdsb]).max(),
            'time_min': np.array([ds.time_min for ds in xdsb]).min(),
            'timeid': 0,
            'freq_out': nu,
            'freq_max': np.array([ds.freq_max for ds in xdsb]).max(),
            'freq_min': np.array([ds.freq_min for ds in xdsb]).min(),
        }
        xds_out.append(VisDataset(data_vars, coords, attrs))
    return xds_out


# ------------------------------------------------------------------------------------------------- concat_chan
def concat_chan(xds, nband_out=1):
    """misc.py:860-987: per time and output band one dataset.  The bands are the nband_out bins of linspace(min freq_min,
    max freq_max); a bin's channels are the unique input channels in [flow, fhigh) (the last bin: [flow, fhigh]); a
    dataset joins a bin when it has the bin's time_out and its freq_min or freq_max lies STRICTLY inside (flow, fhigh),
    the reference's rule.  VIS, WEIGHT, MASK: sum_overlap of the selected datasets; UVW: the first selected one's; BEAM:
    their sum_beam.  xds itself when nband_in == nband_out or nband_in == 1."""
    times = np.unique([ds.time_out for ds in xds])
    freqs_in = np.unique([ds.freq_out for ds in xds])
    freqs_min = np.unique([ds.freq_min for ds in xds])
    freqs_max = np.unique([ds.freq_max for ds in xds])
    all_freqs = np.unique(np.concatenate([_host(ds.chan.values) for ds in xds]))
    nband_in = freqs_in.size
    if nband_in == nband_out or nband_in == 1:
        return xds
    freq_bins = np.linspace(freqs_min.min(), freqs_max.max(), nband_out + 1)
    bin_centers = (freq_bins[1:] + freq_bins[0:-1]) / 2
    xds_out = []
    for time in times:
        for b in range(nband_out):
            flow, fhigh = freq_bins[b], freq_bins[b + 1]
            freqsb = all_freqs[all_freqs >= flow]
            freqsb = freqsb[freqsb <= fhigh] if b == nband_out - 1 else freqsb[freqsb < fhigh]
            xdst = []
            for ds in xds:
                low_in = ds.freq_min > flow and ds.freq_min < fhigh
                high_in = ds.freq_max > flow and ds.freq_max < fhigh
                if ds.time_out == time and (low_in or high_in):
                    xdst.append(ds)
            if not xdst:
                raise ValueError(f"concat_chan: no dataset has freq_min or freq_max strictly inside band {b} "
                                 f"({flow}, {fhigh}) at time_out {time}")
            first = xdst[0]
            kwargs = {}
            for i, ds in enumerate(xdst):
                kwargs[f'vis{i}'], kwargs[f'wgt{i}'] = ds.VIS.values, ds.WEIGHT.values
                kwargs[f'mask{i}'], kwargs[f'freq{i}'] = ds.MASK.values, ds.FREQ.values
            out = sum_overlap(freqsb, flow, fhigh, **kwargs)
            data_vars = {
                'VIS': (('row', 'chan'), out['viso']),
                'WEIGHT': (('row', 'chan'), out['wgto']),
                'MASK': (('row', 'chan'), out['masko']),
                'FREQ': (('chan',), freqsb),
                'UVW': (('row', 'three'), first.UVW.values),
                'BEAM': (('l_beam', 'm_beam'), sum_beam(xdst)),
            }
            coords = {'chan': (('chan',), freqsb), 'l_beam': (('l_beam',), first.l_beam.values),
                      'm_beam': (('m_beam',), first.m_beam.values)}
            attrs = {
                'freq_out': np.round(bin_centers[b], 5),
                'freq_max': fhigh,
                'freq_min': flow,
                'bandid': b,
                'dec': first.dec,
                'ra': first.ra,
                'time_out': time,
                'time_max': np.array([ds.time_max for ds in xdst]).max(),
                'time_min': np.array([ds.time_min for ds in xdst]).min(),
            }
            xds_out.append(VisDataset(data_vars, coords, attrs))
    return xds_out


# ---------------------------------------------------------------------------------------------- image geometry
def image_geometry(xds, cell_size=None, super_resolution_factor=2.0, field_of_view=None, nx=None, ny=None,
                   psf_oversize=2.0):
    """grid.py:226-285: dict of cell_N, cell_rad, cell_size (arcseconds), nx, ny, nx_psf, ny_psf.  uv_max is the max over
    the datasets of max(|u|, |v|), taken on the device; max_freq the max of their FREQ; cell_N = 1 / (2 uv_max max_freq
    / c).  cell_size (arcseconds) fixes the cell, else cell_N / super_resolution_factor.  Without nx the images are
    good_size(field_of_view [degrees] / cell) pixels, made even; the PSF is psf_oversize times as large.  The two
    scalars are the one host read: they set array sizes."""
    from .misc import good_size
    uv = torch.stack([_dev.to_dev(ds.UVW.values)[:, :2].abs().max() for ds in xds]).max()
    fmax = torch.stack([_dev.to_dev(ds.FREQ.values).max() for ds in xds]).max()
    uv_max, max_freq = torch.stack([uv.double(), fmax.double()]).tolist()
    cell_N = 1.0 / (2 * uv_max * max_freq / LIGHTSPEED)
    if cell_size is not None:
        cell_rad = cell_size * np.pi / 60 / 60 / 180
        if cell_N / cell_rad < 1:
            raise ValueError("Requested cell size too large. "
                             "Super resolution factor = ", cell_N / cell_rad)
    else:
        cell_rad = cell_N / super_resolution_factor
        cell_size = cell_rad * 60 * 60 * 180 / np.pi

    def even_good(n):
        n = good_size(n)
        while n % 2:
            n += 1
            n = good_size(n)
        return n

    if nx is None:
        if field_of_view is None:
            raise ValueError("image_geometry: give nx or field_of_view")
        nx = ny = even_good(int(field_of_view * 3600 / cell_size))
    else:
        ny = ny if ny is not None else nx
    return dict(cell_N=cell_N, cell_rad=cell_rad, cell_size=cell_size, nx=int(nx), ny=int(ny),
                nx_psf=even_good(int(psf_oversize * nx)), ny_psf=even_good(int(psf_oversize * ny)))
