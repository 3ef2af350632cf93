#!/usr/bin/env python
"""
Golden vectors for the fastim chain (pfb_clean_amd/utils/stokes2im.py): what the reference's own single_stokes_image
(pfb/utils/stokes2im.py:40-358) makes of the chunks of tests/fastim_cases.py in 'single' and in 'double', stored in
fastim.npz next to this file.

Run in the BUILD container only:   python tests/golden/make_golden_fastim.py
(the reference's stokes2im.py, weighting.py, stokes.py, gridder.py and misc.py are loaded by path and executed under
tests/golden/_refstubs.py: every line that runs is the reference's; the tests only read the .npz file.)  Added here to
what _refstubs.py and make_golden_stokes.py substitute:
  * distributed.worker_client: a context whose compute() returns its list (the columns are arrays already);
  * xarray.Dataset: an object that records data_vars and attrs, and whose to_zarr returns it;
  * casacore.quanta.quantity: seconds - 3506716800 as the Unix time;
  * numba.literally: the str subclass of make_golden_stokes.py;
  * ducc0.wgridder.experimental.vis2dirty / dirty2vis: the exact direct sums of tests/wgrid_cases.py -- the operators'
    definition; epsilon plays no part in them.

The file holds results only, per case and precision: `residual` (the RESIDUAL image as vis2dirty returned it, before
the float32 cast), `wsum`, `rms`, and three scalars that the tests' bounds are stated in, formed here from the arrays
the reference handed to vis2dirty: S = sum over the unflagged visibilities of weight (|residual vis + model vis| +
|model vis|), norm_data = |R^H W vis| and norm_model = |R^H W R model| (0 without a model).  The inputs come from
fastim_cases, seeded.

Two readings of the reference are put on record by assertion: filter_extreme_counts=True is a TypeError (the call passes
`nlevel`, the function's keyword is `level`), and l2reweight_dof=5 with a model is a NameError (line 275).

Fixed zip timestamps: two runs give identical bytes.
"""
import contextlib
import importlib.util
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, HERE)

import fastim_cases as fc                               # noqa: E402
import wgrid_cases as wc                                # noqa: E402
import make_golden_stokes as mgs                        # noqa: E402
from make_golden_weighting import save                  # noqa: E402

seen = {}           # what the last call handed to the gridder


def _case(uvw, freq, nx, ny, px, py, cx, cy, do_wgridding, divide_by_n, mask):
    return dict(uvw=uvw, freq=np.asarray(freq), nx=nx, ny=ny, px=px, py=py, cx=cx, cy=cy, do_wgridding=do_wgridding,
                divide_by_n=divide_by_n, mask=mask, wgt=None)


def direct_vis2dirty(uvw=None, freq=None, vis=None, wgt=None, mask=None, npix_x=None, npix_y=None, pixsize_x=None,
                     pixsize_y=None, center_x=0.0, center_y=0.0, epsilon=None, flip_v=False, do_wgridding=None,
                     divide_by_n=True, nthreads=1, sigma_min=1.1, sigma_max=3.0, double_precision_accumulation=False,
                     verbosity=0):
    assert not flip_v
    case = _case(uvw, freq, npix_x, npix_y, pixsize_x, pixsize_y, center_x, center_y, do_wgridding, divide_by_n, mask)
    seen.update(case=case, vis=vis.copy(), wgt=wgt.copy())
    seen['residual'] = wc.direct_vis2dirty(case, vis, wgt=wgt)
    return seen['residual']


def direct_dirty2vis(uvw=None, freq=None, dirty=None, pixsize_x=None, pixsize_y=None, center_x=0.0, center_y=0.0,
                     epsilon=None, do_wgridding=None, divide_by_n=True, nthreads=1, flip_v=False):
    assert not flip_v
    nx, ny = dirty.shape
    case = _case(uvw, freq, nx, ny, pixsize_x, pixsize_y, center_x, center_y, do_wgridding, divide_by_n, None)
    return wc.direct_dirty2vis(case, dirty, wgt=None)


class Dataset:
    def __init__(self, data_vars, attrs=None):
        self.data_vars, self.attrs = data_vars, attrs

    def to_zarr(self, *a, **k):
        return self


class Client:
    def compute(self, things, **k):
        return things


def load_reference():
    ref_weighting = mgs.load_reference()                 # stubs, pfb.utils.stokes, the memoised stokes_funcs
    import _refstubs
    sys.modules['pfb.utils.weighting'] = ref_weighting
    sys.modules['numba'].literally = mgs.Lit
    sys.modules['numba.core'].errors = sys.modules['numba.core.errors']
    dist = sys.modules['distributed']
    dist.worker_client = lambda: contextlib.nullcontext(Client())
    sys.modules['xarray'] = xr = _refstubs._AnyModule('xarray')
    xr.Dataset = Dataset
    quanta = _refstubs._mod('casacore.quanta')
    quanta.quantity = lambda s: type('Q', (), {'to_unix_time': lambda self: float(s[:-1]) - fc.UNIX_OFFSET})()
    sys.modules['casacore'] = _refstubs._mod('casacore', quanta=quanta)
    ducc = sys.modules['ducc0.wgridder.experimental']
    ducc.vis2dirty, ducc.dirty2vis = direct_vis2dirty, direct_dirty2vis
    mods = {}
    for name, path, alias in (('gridder', 'operators/gridder.py', 'pfb.operators.gridder'),
                              ('stokes2im', 'utils/stokes2im.py', None)):
        spec = importlib.util.spec_from_file_location('pfb_ref_' + name, '/root/reference/pfb/' + path)
        mods[name] = mod = importlib.util.module_from_spec(spec)
        if name == 'gridder':
            sys.modules.setdefault('pfb.operators', _refstubs._mod('pfb.operators'))
        spec.loader.exec_module(mod)
        if alias:
            sys.modules[alias] = mod
    model_vis = mods['stokes2im'].im2vis

    def im2vis(*a, **k):
        seen['model_vis'] = model_vis(*a, **k)
        return seen['model_vis']
    mods['stokes2im'].im2vis = im2vis
    return mods['stokes2im']


def run(ref, case, tag, **over):
    seen.clear()
    kw = fc.call_kwargs(case, tag)
    for k, v in over.items():
        setattr(kw['opts'], k, v)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        ds = ref.single_stokes_image(**kw)
    return ds


if __name__ == '__main__':
    ref = load_reference()
    out = {}
    for case in fc.CASES:
        for tag in fc.TAGS:
            ds = run(ref, case, tag)
            residual = seen['residual']
            assert residual.shape == (case['nx'], case['ny']) and residual.dtype == np.float64
            stored = ds.data_vars['RESIDUAL'][1]
            assert stored.dtype == np.float32 and np.array_equal(stored, residual.astype(np.float32))
            rdt = np.float32 if tag == 'single' else np.float64
            assert seen['wgt'].dtype == rdt and np.asarray(ds.attrs['wsum']).dtype == rdt
            assert ds.attrs['rms'] == np.std(residual)
            live = seen['case']['mask'] != 0
            w = seen['wgt'].astype(np.float64)
            model_vis = seen.get('model_vis')
            assert (model_vis is not None) == (case['mds'] is not None)
            mv = np.zeros_like(seen['vis'], dtype=np.complex128) if model_vis is None else model_vis.astype(np.complex128)
            vis = seen['vis'].astype(np.complex128) + mv * live           # the Stokes visibilities before the model
            res = dict(residual=residual, wsum=np.float64(ds.attrs['wsum']), rms=np.float64(ds.attrs['rms']),
                       S=np.float64(((np.abs(vis) + np.abs(mv)) * w)[live].sum()),
                       norm_data=np.float64(np.linalg.norm(wc.direct_vis2dirty(seen['case'], vis, wgt=w))),
                       norm_model=np.float64(np.linalg.norm(wc.direct_vis2dirty(seen['case'], mv, wgt=w))
                                             if model_vis is not None else 0.0))
            assert set(res) == set(fc.RESULT_KEYS)
            for k, v in res.items():
                out[f"{case['name']}_{tag}_{k}"] = v
            print(f"{case['name']} {tag}: wsum {res['wsum']:.6g} rms {res['rms']:.6g} utc {ds.attrs['utc']}", flush=True)
    # ---- the two readings
    robust = fc.case_named('row-weights')
    try:
        run(ref, robust, 'double', filter_extreme_counts=True)
        raise AssertionError('the reference ran filter_extreme_counts=True')
    except TypeError as e:
        print(f'filter_extreme_counts=True: TypeError: {e}')
    try:
        run(ref, fc.case_named('model-two-bins'), 'double', l2reweight_dof=5)
        raise AssertionError('the reference ran l2reweight_dof=5')
    except NameError as e:
        print(f'l2reweight_dof=5: NameError: {e}')
    save('fastim.npz', out)
