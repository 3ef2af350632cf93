#!/usr/bin/env python
"""
Golden vectors for the band / time concatenation and the beam resampling (pfb_clean_amd/utils/concat.py, beam.py): inputs
and what the reference's own pfb/utils/misc.py (sum_overlap, _sum_beam, sum_beam, concat_row, concat_chan) and
pfb/utils/beam.py (_eval_beam) make of them, stored in concat.npz next to this file.

Run in the BUILD container only:   python tests/golden/make_golden_concat.py
(the reference's source is loaded by path and executed under tests/golden/_refstubs.py; the tests only read the .npz.)

Stand-ins defined HERE, all eager, so that every line of the five functions that runs is the reference's:
  xarray      Dataset (data_vars, coords, attrs; attribute and item access, a dimension without a coordinate reads as
              its index range; assign, assign_coords, assign_attrs return a new Dataset; chunk returns self), DataArray,
              concat (np.concatenate along the named dimension) and merge (the named arrays as one Dataset; a dimension
              two of them share must have one size, which is what xarray's alignment of coordinate-free dimensions asks)
  quartical   Blocker: add_input collects keyword arguments, get_dask_outputs calls the function on them
  dask.array  from_array is the identity
  katbeam, africanus.rime*, numba.core.errors   inert placeholders that beam.py imports at module level

Groups (tests/concat_cases.py reads them back by these names); inputs are stored once, in complex64 / float32 (beams and
axes float64), and are fed to the reference as they are (tag f32) and cast up to complex128 / float64 (tag f64):
  so{j}_*   a sum_overlap case: ufreq, nds, per source s{i}_vis, _wgt, _mask, _freq; viso_/wgto_/masko_{tag}
  sb{j}_*   a _sum_beam case: nds, per source s{i}_beam (float64), s{i}_wgt (float32); out_{wtag}{btag} for weights of
            wtag and beams of btag, (f32, f32), (f64, f64) and (f32, f64)
  eb{j}_*   an _eval_beam case: beam (float64), l_in, m_in, l_out, m_out (1-D or 2-D); out_{tag} for the beam cast to tag
  cc_*      concat_chan: the input datasets cc_in_*, the reference's outputs cc_o{nband_out}_{tag}_*
  cr_*      concat_row: the input datasets cr_in_*, the reference's outputs cr_o_{tag}_*
A dataset list P: P_n, and per dataset k P_{k}_{VIS, WEIGHT, MASK, UVW, FREQ, BEAM, chan, l_beam, m_beam} and P_{k}_attrs,
the attributes in the order of ATTRS (NaN: absent).

Fixed zip timestamps: two runs give identical bytes.
"""
import contextlib
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
MAX_BYTES = 1 << 20
ATTRS = ('time_out', 'time_min', 'time_max', 'timeid', 'freq_out', 'freq_min', 'freq_max', 'bandid', 'ra', 'dec')
VARS = ('VIS', 'WEIGHT', 'MASK', 'UVW', 'FREQ', 'BEAM', 'chan', 'l_beam', 'm_beam')
TAGS = {'f32': (np.complex64, np.float32), 'f64': (np.complex128, np.float64)}


def save(name, out):
    """np.savez_compressed with fixed member timestamps (bit-identical from run to run)."""
    path = os.path.join(HERE, name)
    with zipfile.ZipFile(path, 'w', compression=zipfile.ZIP_DEFLATED) as z:
        for key in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    size = os.path.getsize(path)
    assert size < MAX_BYTES, (name, size)
    print(f'{name}: {len(out)} arrays, {size} bytes')


# ------------------------------------------------------------------------------------------- the eager stand-ins
class DataArray:
    def __init__(self, data, dims, name=None):
        self.data, self.dims, self.name = np.asarray(data), tuple(dims), name
        assert self.data.ndim == len(self.dims), (name, dims, self.data.shape)

    values = property(lambda self: self.data)
    dtype = property(lambda self: self.data.dtype)
    shape = property(lambda self: self.data.shape)
    size = property(lambda self: self.data.size)

    def __array__(self, dtype=None, copy=None):
        return self.data if dtype is None else self.data.astype(dtype)


class Dataset:
    def __init__(self, data_vars=None, coords=None, attrs=None):
        self._vars, self._coords, self.attrs = {}, {}, dict(attrs or {})
        for name, v in (coords or {}).items():
            self._coords[name] = self._array(name, v)
        for name, v in (data_vars or {}).items():
            self._vars[name] = self._array(name, v)

    @staticmethod
    def _array(name, v):
        if isinstance(v, DataArray):
            return DataArray(v.data, v.dims, name)
        dims, data = v
        return DataArray(data, dims, name)

    def _copy(self):
        new = Dataset(attrs=self.attrs)
        new._vars, new._coords = dict(self._vars), dict(self._coords)
        return new

    def sizes(self):
        out = {}
        for v in list(self._vars.values()) + list(self._coords.values()):
            for d, n in zip(v.dims, v.shape):
                assert out.setdefault(d, n) == n, f"conflicting sizes for dimension {d!r}"
        return out

    def __getattr__(self, name):
        if name.startswith('_'):
            raise AttributeError(name)
        for src in (self._vars, self._coords, self.attrs):
            if name in src:
                return src[name]
        sizes = self.sizes()
        if name in sizes:
            return DataArray(np.arange(sizes[name]), (name,), name)
        raise AttributeError(name)

    def __getitem__(self, name):
        return self._vars[name] if name in self._vars else self._coords[name]

    def __setitem__(self, name, v):
        self._vars[name] = self._array(name, v)
        self.sizes()

    def __contains__(self, name):
        return name in self._vars or name in self._coords

    def assign(self, variables):
        new = self._copy()
        for name, v in variables.items():
            new._vars[name] = self._array(name, v)
        new.sizes()
        return new

    def assign_coords(self, coords):
        new = self._copy()
        for name, v in coords.items():
            new._coords[name] = self._array(name, v)
        new.sizes()
        return new

    def assign_attrs(self, attrs):
        new = self._copy()
        new.attrs.update(attrs)
        return new

    def chunk(self, chunks=None):
        return self


def xr_concat(arrays, dim):
    first = arrays[0]
    assert all(a.dims == first.dims and a.name == first.name for a in arrays)
    return DataArray(np.concatenate([a.data for a in arrays], axis=first.dims.index(dim)), first.dims, first.name)


def xr_merge(arrays):
    ds = Dataset(data_vars={a.name: a for a in arrays})
    ds.sizes()
    return ds


class Blocker:
    def __init__(self, func, index):
        self.func, self.kwargs = func, {}

    def add_input(self, name, value, index=None):
        self.kwargs[name] = value.data if isinstance(value, DataArray) else value

    def add_output(self, *args):
        pass

    def get_dask_outputs(self):
        return self.func(**self.kwargs)


def load_reference():
    sys.path.insert(0, HERE)
    import _refstubs
    _refstubs.install(ROOT)
    misc = sys.modules['pfb.utils.misc']
    misc.xr = types.SimpleNamespace(Dataset=Dataset, DataArray=DataArray, concat=xr_concat, merge=xr_merge)
    misc.Blocker = Blocker
    sys.modules['dask.array'].from_array = lambda a, chunks=None: a
    for name in ('katbeam', 'africanus.rime', 'africanus.rime.fast_beam_cubes'):
        sys.modules[name] = _refstubs._AnyModule(name)
    core = types.ModuleType('numba.core')
    errors = types.ModuleType('numba.core.errors')
    errors.NumbaDeprecationWarning = type('NumbaDeprecationWarning', (Warning,), {})
    sys.modules['numba.core'], sys.modules['numba.core.errors'] = core, errors
    spec = importlib.util.spec_from_file_location('pfb_ref_beam', '/root/reference/pfb/utils/beam.py')
    beam = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(beam)
    return misc, beam


# ----------------------------------------------------------------------------------------------------- the cases
F0, DF = 1.0e9, 1.0e6


def source(rng, nrow, freq, density=0.8):
    n = len(freq)
    vis = (rng.standard_normal((nrow, n)) + 1j * rng.standard_normal((nrow, n))).astype(np.complex64)
    wgt = rng.uniform(0.5, 1.5, (nrow, n)).astype(np.float32)
    mask = (rng.uniform(size=(nrow, n)) < density).astype(np.uint8)
    return dict(vis=vis, wgt=wgt, mask=mask, freq=np.asarray(freq, np.float64))


def overlap_cases(rng):
    cases = []
    grid = F0 + DF * np.arange(40)
    cases.append(dict(name='one', ufreq=grid[:1], src=[source(rng, 1, grid[:1], 1.0)]))
    # partly overlapping: channels 0-2 and 2-4; column 1 flagged in every source that has it; at (row 1, channel 2) both
    # sources are unflagged with zero weight: 0 / 0
    a, b = source(rng, 3, grid[0:3], 1.0), source(rng, 3, grid[2:5], 1.0)
    a['mask'][:, 1] = 0
    a['mask'][0, 2] = 0                                               # one contributor flagged, the other not
    a['wgt'][1, 2] = b['wgt'][1, 0] = 0.0
    cases.append(dict(name='partial', ufreq=grid[:5], src=[a, b]))
    # disjoint, more than one workgroup: 257 x 5 outputs
    cases.append(dict(name='disjoint', ufreq=grid[:5], src=[source(rng, 257, grid[0:3]), source(rng, 257, grid[3:5])]))
    # 9 sources on 33 channels (crosses a batch of 8): two that cover everything, the even and the odd channels, a
    # reversed stretch, one that contributes no channel, one with channels outside the band, the first three, the last one
    u = grid[:33]
    freqs = [u, u, u[0::2], u[1::2], u[5:20][::-1].copy(), grid[34:38], np.concatenate([grid[35:38], u[10:30]]), u[:3],
             u[-1:]]
    src = [source(rng, 3, f) for f in freqs]
    for s in src:
        hit = np.flatnonzero(s['freq'] == u[7])
        s['mask'][:, hit] = 0                                          # output channel 7: flagged in every source
        hit = np.flatnonzero(s['freq'] == u[20])
        s['wgt'][1, hit] = 0.0                                         # (row 1, channel 20): weights all zero
        s['mask'][1, hit] = 1
    src[8]['vis'][0, 0], src[8]['wgt'][0, 0], src[8]['mask'][0, 0] = 3.0 - 2.0j, 1.25, 1     # the ninth source counts
    cases.append(dict(name='nine-interleaved', ufreq=u, src=src))
    # 9 sources that all hold the one output channel (and one more each), 257 rows
    src = [source(rng, 257, [grid[0], grid[1 + i]] if i % 2 else [grid[1 + i], grid[0]]) for i in range(9)]
    cases.append(dict(name='nine-full', ufreq=grid[:1], src=src))
    return cases


def beam_sum_cases(rng):
    def beams(n, shape=(9, 7)):
        return [rng.uniform(0.1, 1.0, shape) for _ in range(n)]

    def wgts(shapes):
        return [rng.uniform(0.5, 1.5, s).astype(np.float32) for s in shapes]
    nine = [(1, 1), (3, 43), (280, 250), (5, 4), (2, 2), (7, 1), (1, 9), (16, 16), (3, 3)]      # 1, 129, 70 000, ...
    cases = [dict(name='one', beam=beams(1), wgt=wgts([(1, 1)])),
             dict(name='two', beam=beams(2), wgt=wgts([(3, 43), (5, 4)])),
             dict(name='nine', beam=beams(9), wgt=wgts(nine)),
             dict(name='zero', beam=beams(2), wgt=[np.zeros((3, 4), np.float32), np.zeros((2, 2), np.float32)])]
    return cases


def beam_eval_cases(rng):
    l9 = -0.04 + 0.01 * np.arange(9)
    m7 = -0.03 + 0.01 * np.arange(7)
    l9n = np.array([-0.05, -0.041, -0.02, -0.013, 0.0, 0.004, 0.019, 0.03, 0.052])     # non-uniform
    m7n = np.array([-0.03, -0.022, -0.02, 0.001, 0.011, 0.012, 0.04])

    def points(g, n):
        """n >= 4 coordinates of axis g (ascending or not): outside on both sides, the first and the last node, nodes
        and interior points in between."""
        lo, hi, h = g.min(), g.max(), np.abs(np.diff(g)).max()
        k = min(g.size - 2, max(0, (n - 4) // 2))
        nodes = rng.choice(g[1:-1], k, replace=False) if k else np.zeros(0)
        inner = np.concatenate([[lo, hi], nodes, rng.uniform(lo, hi, n)])[:n - 2]
        return np.concatenate([[lo - 0.37 * h], inner, [hi + 0.61 * h]])

    cases = []
    cases.append(dict(name='2x2-1x1', beam=rng.uniform(0.1, 1.0, (2, 2)), l_in=np.array([-1.0, 2.0]),
                      m_in=np.array([0.5, 0.75]), l_out=np.array([0.3]), m_out=np.array([0.6])))
    b = rng.uniform(0.1, 1.0, (2, 2))
    lo, mo = points(np.array([-1.0, 2.0]), 5), points(np.array([0.5, 0.75]), 4)
    ll, mm = np.meshgrid(lo, mo, indexing='ij')
    cases.append(dict(name='2x2-5x4-2d', beam=b, l_in=np.array([-1.0, 2.0]), m_in=np.array([0.5, 0.75]), l_out=ll, m_out=mm))
    cases.append(dict(name='9x7-5x4', beam=rng.uniform(0.1, 1.0, (9, 7)), l_in=l9, m_in=m7, l_out=points(l9, 5),
                      m_out=points(m7, 4)))
    cases.append(dict(name='9x7-37x300', beam=rng.uniform(-1.0, 1.0, (9, 7)), l_in=l9, m_in=m7, l_out=points(l9, 37),
                      m_out=points(m7, 300)))
    cases.append(dict(name='nonuniform-37x300', beam=rng.uniform(0.1, 1.0, (9, 7)), l_in=l9n, m_in=m7n,
                      l_out=points(l9n, 37), m_out=points(m7n, 300)))
    # 2-D coordinates that are no mesh: a rotated, sheared lattice over the non-uniform grid, corners outside
    i, j = np.meshgrid(np.linspace(-1, 1, 5), np.linspace(-1, 1, 4), indexing='ij')
    cases.append(dict(name='nonuniform-5x4-2d', beam=rng.uniform(0.1, 1.0, (9, 7)), l_in=l9n, m_in=m7n,
                      l_out=0.055 * (0.9 * i - 0.4 * j), m_out=0.04 * (0.3 * i + 0.95 * j)))
    cases.append(dict(name='descending-5x4', beam=rng.uniform(0.1, 1.0, (9, 7)), l_in=l9n[::-1].copy(), m_in=m7,
                      l_out=points(l9n, 5), m_out=points(m7, 4)))
    return cases


def dataset(rng, nrow, chan, time, tid, bid, uvw):
    s = source(rng, nrow, chan)
    return Dataset(
        data_vars={'VIS': (('row', 'chan'), s['vis']), 'WEIGHT': (('row', 'chan'), s['wgt']),
                   'MASK': (('row', 'chan'), s['mask']), 'UVW': (('row', 'three'), uvw), 'FREQ': (('chan',), s['freq']),
                   'BEAM': (('l_beam', 'm_beam'), rng.uniform(0.1, 1.0, (5, 4)))},
        coords={'chan': (('chan',), s['freq']), 'l_beam': (('l_beam',), -0.02 + 0.01 * np.arange(5)),
                'm_beam': (('m_beam',), -0.015 + 0.01 * np.arange(4))},
        attrs={'time_out': time, 'time_min': time - 4.0, 'time_max': time + 4.0, 'timeid': tid,
               'freq_out': float(np.round(np.mean(chan), 5)), 'freq_min': float(np.min(chan)), 'freq_max': float(np.max(chan)),
               'bandid': bid, 'ra': 0.35, 'dec': -0.52})


def chan_datasets(rng):
    """2 times x 4 input bands of 4 channels; adjacent bands share their edge channel (band b: channels 3b .. 3b + 3 of
    13); 24 and 17 rows."""
    grid = F0 + DF * np.arange(13)
    xds = []
    for t, (time, nrow) in enumerate(((5.0e9 + 8.0, 24), (5.0e9 + 16.0, 17))):
        uvw = rng.uniform(-300.0, 300.0, (nrow, 3))
        for b in range(4):
            xds.append(dataset(rng, nrow, grid[3 * b:3 * b + 4], time, t, b, uvw))
    return xds


def row_datasets(rng):
    """3 times x 2 bands of 3 channels, 4, 1 and 6 rows."""
    grid = F0 + DF * np.arange(6)
    xds = []
    for t, (time, nrow) in enumerate(((5.0e9 + 8.0, 4), (5.0e9 + 16.123456789, 1), (5.0e9 + 24.0, 6))):
        uvw = rng.uniform(-300.0, 300.0, (nrow, 3))
        for b in range(2):
            xds.append(dataset(rng, nrow, grid[3 * b:3 * b + 3], time, t, b, uvw))
    return xds


def cast(ds, tag):
    cdt, rdt = TAGS[tag]
    return ds.assign({'VIS': (('row', 'chan'), ds.VIS.data.astype(cdt)),
                      'WEIGHT': (('row', 'chan'), ds.WEIGHT.data.astype(rdt)),
                      'BEAM': (('l_beam', 'm_beam'), ds.BEAM.data.astype(rdt))})


def put_datasets(out, prefix, xds):
    out[f'{prefix}_n'] = np.array(len(xds))
    for k, ds in enumerate(xds):
        for name in VARS:
            out[f'{prefix}_{k}_{name}'] = np.asarray(ds[name].data)
        out[f'{prefix}_{k}_attrs'] = np.array([float(ds.attrs.get(a, np.nan)) for a in ATTRS])
        assert set(ds.attrs) <= set(ATTRS), set(ds.attrs) - set(ATTRS)


if __name__ == '__main__':
    misc, beam = load_reference()
    rng = np.random.default_rng(2207)
    out = {}

    cases = overlap_cases(rng)
    out['so_names'] = np.array([c['name'] for c in cases])
    for j, c in enumerate(cases):
        out[f'so{j}_ufreq'], out[f'so{j}_nds'] = c['ufreq'], np.array(len(c['src']))
        for i, s in enumerate(c['src']):
            for key in ('vis', 'wgt', 'mask', 'freq'):
                out[f'so{j}_s{i}_{key}'] = s[key]
        for tag, (cdt, rdt) in TAGS.items():
            kwargs = {}
            for i, s in enumerate(c['src']):
                kwargs[f'vis{i}'], kwargs[f'wgt{i}'] = s['vis'].astype(cdt), s['wgt'].astype(rdt)
                kwargs[f'mask{i}'], kwargs[f'freq{i}'] = s['mask'].copy(), s['freq'].copy()
            with np.errstate(all='ignore'):
                res = misc.sum_overlap(c['ufreq'], c['ufreq'][0], c['ufreq'][-1], **kwargs)
            assert res['viso'].dtype == cdt and res['wgto'].dtype == rdt and res['masko'].dtype == np.uint8
            for key in ('viso', 'wgto', 'masko'):
                out[f'so{j}_{key}_{tag}'] = res[key]
    assert not np.isfinite(out['so1_viso_f64']).all() and not np.isfinite(out['so3_viso_f32']).all()

    cases = beam_sum_cases(rng)
    out['sb_names'] = np.array([c['name'] for c in cases])
    for j, c in enumerate(cases):
        out[f'sb{j}_nds'] = np.array(len(c['beam']))
        for i, (b, w) in enumerate(zip(c['beam'], c['wgt'])):
            out[f'sb{j}_s{i}_beam'], out[f'sb{j}_s{i}_wgt'] = b, w
        for wtag, btag in (('f32', 'f32'), ('f64', 'f64'), ('f32', 'f64')):
            wdt, bdt = TAGS[wtag][1], TAGS[btag][1]
            kwargs = {}
            for i, (b, w) in enumerate(zip(c['beam'], c['wgt'])):
                kwargs[f'beam{i}'], kwargs[f'wgt{i}'] = b.astype(bdt), w.astype(wdt)
            res = misc._sum_beam(9, 7, np.dtype(bdt), **kwargs)['beam']
            assert res.dtype == bdt and res.shape == (9, 7)
            out[f'sb{j}_out_{wtag}{btag}'] = res

    cases = beam_eval_cases(rng)
    out['eb_names'] = np.array([c['name'] for c in cases])
    for j, c in enumerate(cases):
        for key in ('beam', 'l_in', 'm_in', 'l_out', 'm_out'):
            out[f'eb{j}_{key}'] = c[key]
        for tag, (_, rdt) in TAGS.items():
            with contextlib.redirect_stdout(io.StringIO()):            # the reference prints the bounds error it catches
                res = beam._eval_beam(c['beam'].astype(rdt), c['l_in'], c['m_in'], c['l_out'], c['m_out'])
            assert res.dtype == np.float64
            out[f'eb{j}_out_{tag}'] = res

    xds = chan_datasets(rng)
    put_datasets(out, 'cc_in', xds)
    for tag in TAGS:
        typed = [cast(ds, tag) for ds in xds]
        for nband_out in (2, 3):
            with np.errstate(all='ignore'):
                res = misc.concat_chan(typed, nband_out=nband_out)
            assert len(res) == 2 * nband_out and res[0].VIS.dtype == TAGS[tag][0]
            put_datasets(out, f'cc_o{nband_out}_{tag}', res)
        assert misc.concat_chan(typed, nband_out=4) is typed and misc.concat_chan(typed[:1], nband_out=3) is not None
        try:
            misc.concat_chan(typed, nband_out=5)
            raise AssertionError('nband_out=5 selects a dataset for every bin')
        except IndexError:
            pass

    xds = row_datasets(rng)
    put_datasets(out, 'cr_in', xds)
    for tag in TAGS:
        typed = [cast(ds, tag) for ds in xds]
        res = misc.concat_row(typed)
        assert len(res) == 2 and res[0].VIS.shape == (11, 3)
        put_datasets(out, f'cr_o_{tag}', res)
        assert misc.concat_row(typed[:2]) is not None
    save('concat.npz', out)
