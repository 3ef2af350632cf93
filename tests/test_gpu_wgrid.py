"""
The w-gridder on the MI355X (pfb_clean_amd.operators.gridder, the visibility-space Hessian of operators.hessian) against
the direct Fourier sums of tests/wgrid_cases.py.

Bounds
  accuracy      ducc0's statement: |result - exact|_2 / |exact|_2 <= epsilon, every case, both directions.
                tests/test_cpu_wgrid.py shows that the recipe in exact arithmetic sits at 0.11 - 0.51 epsilon on these
                cases, so the bound leaves room for rounding only.  An all-zero mask gives exact zeros.
  adjointness   Re<v, dirty2vis(d)> against <vis2dirty(v), d>, fp64, relative to the product, worst of four random
                pairs.  The two sides differ by rounding and summation order alone, as they do in the numpy model: the
                GPU may show 100 times the model's mismatch on the same case and pairs.  The model's figure is a
                difference of two fp64 numbers and is quantised in their ulp: where it comes out below half an ulp
                (2^-53) it is taken as that.
  Hessian       beam vis2dirty(wgt dirty2vis(beam x)) against the composed direct sums at 2 epsilon; <y, H x> against
                <H y, x> like the adjointness; hessian_xds over three datasets on two bands at 2 epsilon.
  no w term     H x against psf_convolve_slice with psfhat_from_psf(vis2dirty(ones, wgt) on (2 nx, 2 ny)) at 3 epsilon:
                one epsilon for each of the three gridder applications (test_cpu_wgrid.py has the exact identity).
"""
import numpy as np
import pytest
import torch

import wgrid_cases as wc
from wgrid_cases import CASES, CASE_IDS

pytestmark = pytest.mark.gpu

_memo = {}


def memo(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def case_named(name):
    return CASES[CASE_IDS.index(name)]


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def kw(case):
    return dict(pixsize_x=case['px'], pixsize_y=case['py'], center_x=case['cx'], center_y=case['cy'],
                epsilon=case['eps'], do_wgridding=case['do_wgridding'], divide_by_n=case['divide_by_n'])


def gpu_vis2dirty(case, vis, **extra):
    from pfb_clean_amd.operators.gridder import vis2dirty
    return vis2dirty(case['uvw'], case['freq'], vis, wgt=case['wgt'], mask=case['mask'], npix_x=case['nx'],
                     npix_y=case['ny'], **kw(case), **extra)


def gpu_dirty2vis(case, dirty):
    from pfb_clean_amd.operators.gridder import dirty2vis
    return dirty2vis(case['uvw'], case['freq'], dirty, wgt=case['wgt'], mask=case['mask'], **kw(case))


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_accuracy_against_the_direct_sum(case):
    got_d = gpu_vis2dirty(case, case['vis'])
    got_v = gpu_dirty2vis(case, case['dirty'])
    rdt, cdt = (np.float32, np.complex64) if case['dtype'] == 'f32' else (np.float64, np.complex128)
    assert got_d.dtype == rdt and got_d.shape == (case['nx'], case['ny'])
    assert got_v.dtype == cdt and got_v.shape == case['vis'].shape
    if case['mask'] is not None:
        assert not got_v[case['mask'] == 0].any()
        if not case['mask'].any():
            assert not got_d.any() and not got_v.any()
            return
    e1 = wc.rel_l2(got_d.astype(np.float64), wc.direct_vis2dirty(case, case['vis']))
    e2 = wc.rel_l2(got_v.astype(np.complex128), wc.direct_dirty2vis(case, case['dirty']))
    print(f"{case['name']}: eps {case['eps']:g} vis2dirty {e1:.3e} dirty2vis {e2:.3e}")
    assert e1 <= case['eps'] and e2 <= case['eps']


@pytest.mark.parametrize('name', ['32x24-eps1e-09', '48x16-eps1e-07', '16x64-eps1e-05', 'centre', 'one-cell'])
def test_fp32_at_its_lower_bound(name):
    """Single precision at the smallest epsilon it accepts (gridder.EPS_MIN, measured: DESIGN 4.10), |w| up to 200."""
    from pfb_clean_amd.operators import gridder
    eps = gridder.EPS_MIN[torch.float32]
    case = wc.as_f32(dict(case_named(name), eps=eps))
    e1 = wc.rel_l2(gpu_vis2dirty(case, case['vis']).astype(np.float64), wc.direct_vis2dirty(case, case['vis']))
    e2 = wc.rel_l2(gpu_dirty2vis(case, case['dirty']).astype(np.complex128), wc.direct_dirty2vis(case, case['dirty']))
    print(f"{name} fp32 at eps {eps:g}: vis2dirty {e1:.3e} dirty2vis {e2:.3e}")
    assert e1 <= eps and e2 <= eps


@pytest.mark.parametrize('name', ['32x24-eps1e-05', '16x64-eps1e-09', 'centre', 'seam', 'one-cell', 'no-wgrid'])
def test_adjointness(name):
    case = case_named(name)
    model = wc.adjoint_mismatch(lambda v: wc.model_vis2dirty(case, v), lambda d: wc.model_dirty2vis(case, d), case)
    gpu = wc.adjoint_mismatch(lambda v: gpu_vis2dirty(case, v), lambda d: gpu_dirty2vis(case, d), case)
    print(f"{name}: adjoint mismatch model {model:.3e} gpu {gpu:.3e}")
    assert gpu <= 100 * max(model, wc.HALF_ULP)


# ------------------------------------------------------------------------------------------------- the Hessian
def hess_case(name):
    """A table case on square pixels (the Hessian takes one `cell`), with a beam and two probes."""
    def make():
        c = dict(case_named(name), divide_by_n=False)
        c['py'] = c['px'] = min(c['px'], c['py'])
        rng = np.random.default_rng(21)
        c['beam'] = rng.uniform(0.5, 1.0, (c['nx'], c['ny']))
        c['x'], c['y'] = rng.standard_normal((2, c['nx'], c['ny']))
        return c
    return memo(('hess', name), make)


def hopts(c):
    return dict(x0=c['cx'], y0=c['cy'], cell=c['px'], do_wgridding=c['do_wgridding'], epsilon=c['eps'],
                double_accum=True, nthreads=4)


def gpu_hessian(c, x, beam='case'):
    from pfb_clean_amd.operators.hessian import _hessian_impl
    return _hessian_impl(x, c['uvw'], c['wgt'], c['mask'], c['freq'], c['beam'] if isinstance(beam, str) else beam,
                         **hopts(c))


@pytest.mark.parametrize('name', ['32x24-eps1e-05', '48x16-eps1e-07', 'centre', 'no-wgrid'])
def test_hessian_impl(name):
    c = hess_case(name)
    Hx = gpu_hessian(c, c['x'])
    assert isinstance(Hx, np.ndarray) and Hx.dtype == np.float64
    err = wc.rel_l2(Hx, wc.direct_hessian(c, c['x'], c['beam']))
    print(f"{name}: hessian rel err {err:.3e} (eps {c['eps']:g})")
    assert err <= 2 * c['eps']
    assert wc.rel_l2(gpu_hessian(c, c['x'], beam=None), wc.direct_hessian(c, c['x'], None)) <= 2 * c['eps']
    # symmetry, measured like the adjointness and against the model's own figure
    def model_H(z):
        return c['beam'] * wc.model_vis2dirty(c, wc.model_dirty2vis(dict(c, wgt=None), c['beam'] * z))

    def sym(H):
        lhs, rhs = np.vdot(c['y'], H(c['x'])), np.vdot(H(c['y']), c['x'])
        return abs(lhs - rhs) / abs(lhs)
    model, gpu = sym(model_H), sym(lambda z: gpu_hessian(c, z))
    print(f"{name}: hessian symmetry model {model:.3e} gpu {gpu:.3e}")
    assert gpu <= 100 * max(model, wc.HALF_ULP)
    # an all-zero x: zeros, and no plan is looked up for it
    from pfb_clean_amd.operators import gridder
    before = dict(gridder.cache_stats)
    gridder.clear_plan_cache()
    z = gpu_hessian(c, np.zeros_like(c['x']))
    assert z.shape == c['x'].shape and not z.any() and gridder.cache_stats == before
    zt = gpu_hessian(c, torch.zeros(c['x'].shape, dtype=torch.float32, device='cuda'))
    assert zt.is_cuda and zt.dtype == torch.float32 and not zt.any()


class _Var:
    def __init__(self, a):
        self.values, self.dtype, self.shape = a, a.dtype, a.shape


class _DS(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def test_hessian_xds_three_datasets_two_bands():
    from pfb_clean_amd.operators.hessian import hessian_xds, hessian
    names, bands = ['32x24-eps1e-05', 'centre', 'seam'], [0, 1, 1]
    cs = [dict(hess_case(n), cx=0.0, cy=0.0, eps=1e-5, do_wgridding=True) for n in names]
    rng = np.random.default_rng(5)
    nx, ny = cs[0]['nx'], cs[0]['ny']
    x = rng.standard_normal((2, nx, ny))
    mask = (rng.uniform(size=(nx, ny)) < 0.8).astype(np.float64)
    wsum, sigmainv = 37.0, 0.3
    opts = dict(cell=cs[0]['px'], do_wgridding=True, epsilon=1e-5, double_accum=False, nthreads=1)
    xds = [_DS(UVW=_Var(c['uvw']), FREQ=_Var(c['freq']), WEIGHT=_Var(c['wgt'] if c['wgt'] is not None else
                                                                   np.ones(c['vis'].shape)),
               MASK=_Var(c['mask'] if c['mask'] is not None else np.ones(c['vis'].shape, np.uint8)),
               BEAM=_Var(c['beam']), bandid=b) for c, b in zip(cs, bands)]
    for use_beam in (True, False):
        ref = np.zeros_like(x)
        for c, b in zip(cs, bands):
            ref[b] += wc.direct_hessian(c, x[b], c['beam'] * mask if use_beam else mask)
        ref = ref / wsum + x * sigmainv ** 2
        got = hessian_xds(x, xds, opts, wsum, sigmainv, mask, compute=True, use_beam=use_beam)
        assert isinstance(got, np.ndarray) and got.shape == x.shape
        # the Tikhonov term is exact: the bound applies to the gridded part
        assert np.linalg.norm(got - ref) <= 2e-5 * np.linalg.norm(ref - x * sigmainv ** 2)
    got_t = hessian_xds(dev(x), xds, opts, wsum, 0.0, dev(mask))
    assert got_t.is_cuda
    c = cs[0]
    one = hessian(x[0], c['uvw'], c['wgt'], c['mask'], c['freq'], c['beam'], opts)
    assert wc.rel_l2(one, wc.direct_hessian(c, x[0], c['beam'])) <= 2e-5


def test_no_wgridding_hessian_is_the_psf_convolution():
    from pfb_clean_amd.operators.gridder import vis2dirty
    from pfb_clean_amd.operators.fft import psfhat_from_psf
    from pfb_clean_amd.operators.psf import psf_convolve_slice
    c = hess_case('no-wgrid')
    nx, ny, eps = c['nx'], c['ny'], c['eps']
    psf = vis2dirty(c['uvw'], c['freq'], np.ones(c['vis'].shape, np.complex128), wgt=c['wgt'], mask=c['mask'],
                    npix_x=2 * nx, npix_y=2 * ny, pixsize_x=c['px'], pixsize_y=c['py'], epsilon=eps,
                    do_wgridding=False, divide_by_n=False)
    conv = psf_convolve_slice(None, None, None, psfhat_from_psf(psf), 2 * ny, c['x'])
    Hx = gpu_hessian(c, c['x'], beam=None)
    err = wc.rel_l2(Hx, conv)
    print(f"no w term: H x against psf_convolve_slice {err:.3e} (eps {eps:g})")
    assert err <= 3 * eps


def test_compute_residual_on_a_dataset_with_visibilities():
    from pfb_clean_amd.operators.gridder import vis2dirty
    from pfb_clean_amd.operators.fft import psfhat_from_psf
    from pfb_clean_amd.operators.hessian import hessian_psf_slice
    c = dict(hess_case('48x16-eps1e-07'))
    c['mask'] =np.ones(c['vis'].shape, np.uint8) if c['mask'] is None else c['mask']
    nx, ny, eps = c['nx'], c['ny'], c['eps']
    psf = vis2dirty(c['uvw'], c['freq'], np.ones(c['vis'].shape, np.complex128), wgt=c['wgt'], mask=c['mask'],
                    npix_x=2 * nx, npix_y=2 * ny, pixsize_x=c['px'], pixsize_y=c['py'], epsilon=eps,
                    do_wgridding=True, divide_by_n=False)
    dirty = np.random.default_rng(9).standard_normal((nx, ny))
    for wrap in (lambda a: a, dev):
        ds = _DS(DIRTY=_Var(wrap(dirty)), PSF=_Var(wrap(psf)), PSFHAT=_Var(wrap(psfhat_from_psf(psf))),
                 BEAM=_Var(wrap(c['beam'])), WSUM=_Var(np.array([1.0])), bandid=0, UVW=_Var(wrap(c['uvw'])),
                 WEIGHT=_Var(wrap(c['wgt'])), VIS_MASK=_Var(wrap(c['mask'])), FREQ=_Var(wrap(c['freq'])))
        A = hessian_psf_slice(ds, 2, 10, 1, 0.1, c['px'], True, eps, False)
        x = wrap(c['x'])
        res = A.compute_residual(x)
        assert isinstance(res, type(x))
        Hbx = wc.direct_hessian(c, c['beam'] * c['x'], None)
        got = res.cpu().numpy() if isinstance(res, torch.Tensor) else res
        # residual = dirty - H(beam x): the error bound is the Hessian's
        assert np.linalg.norm(got - (dirty - Hbx)) <= 2 * eps * np.linalg.norm(Hbx)


# ------------------------------------------------------------------------------------------------ conventions
def test_io_conventions_and_argument_checks():
    from pfb_clean_amd.operators.gridder import vis2dirty, dirty2vis
    c = case_named('32x24-eps1e-07')             # weights and a bool mask
    ref = gpu_vis2dirty(c, c['vis'])
    assert isinstance(ref, np.ndarray)
    got = vis2dirty(dev(c['uvw']), dev(c['freq']), dev(c['vis']), wgt=dev(c['wgt']), mask=dev(c['mask']),
                    npix_x=c['nx'], npix_y=c['ny'], nthreads=8, **kw(c))
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float64
    assert wc.rel_l2(got.cpu().numpy(), ref) <= 1e-12          # the same sums in another atomic order
    gv = dirty2vis(dev(c['uvw']), dev(c['freq']), dev(c['dirty']), wgt=dev(c['wgt']), mask=dev(c['mask']), **kw(c))
    assert isinstance(gv, torch.Tensor) and gv.is_cuda and gv.dtype == torch.complex128
    assert np.array_equal(gv.cpu().numpy(), gpu_dirty2vis(c, c['dirty']))      # no atomics: bit for bit
    # complex64 in, float32 out; double_precision_accumulation runs the fp64 kernels on the same data
    c32 = wc.as_f32(dict(c, eps=1e-3))
    d32 = gpu_vis2dirty(c32, c32['vis'])
    d32d = gpu_vis2dirty(c32, c32['vis'], double_precision_accumulation=True)
    assert d32.dtype == np.float32 and d32d.dtype == np.float32
    exact = wc.direct_vis2dirty(c32, c32['vis'])
    assert wc.rel_l2(d32.astype(np.float64), exact) <= 1e-3 and wc.rel_l2(d32d.astype(np.float64), exact) <= 1e-3
    # what is refused
    with pytest.raises(TypeError):
        vis2dirty(c['uvw'], c['freq'], c['vis'], npix_x=32, npix_y=24, flip_v=True, **kw(c))
    with pytest.raises(TypeError):
        dirty2vis(c['uvw'], c['freq'], c['dirty'], sigma_min=1.1, **kw(c))
    with pytest.raises(TypeError):
        vis2dirty(c['uvw'].astype(np.float32), c['freq'], c['vis'], npix_x=32, npix_y=24, **kw(c))
    with pytest.raises(TypeError):
        vis2dirty(c['uvw'], c['freq'], c['vis'], wgt=c['wgt'].astype(np.float32), npix_x=32, npix_y=24, **kw(c))
    with pytest.raises(ValueError):
        vis2dirty(c['uvw'], c['freq'], c['vis'], npix_x=31, npix_y=24, **kw(c))
    for eps in (0.1, 1e-11):
        with pytest.raises(ValueError):
            vis2dirty(c['uvw'], c['freq'], c['vis'], npix_x=32, npix_y=24, **dict(kw(c), epsilon=eps))
    from pfb_clean_amd.operators import gridder
    with pytest.raises(ValueError):
        gpu_vis2dirty(dict(c32, eps=0.5 * gridder.EPS_MIN[torch.float32]), c32['vis'])


def test_plan_reuse_builds_no_new_order():
    from pfb_clean_amd.operators import gridder
    from pfb_clean_amd.operators.hessian import _hessian_impl
    c = hess_case('48x16-eps1e-07')
    gridder.clear_plan_cache()
    arrays = [dev(c[k]) for k in ('uvw', 'wgt', 'mask', 'freq')]
    uvw, wgt, mask, freq = arrays
    x = dev(c['x'])
    start = gridder.cache_stats['miss']
    first = _hessian_impl(x, uvw, wgt, mask, freq, None, **hopts(c))
    assert gridder.cache_stats['miss'] == start + 1
    for _ in range(3):                                       # a major cycle: the same arrays, a new model
        again = _hessian_impl(x * 2, uvw, wgt, mask, freq, None, **hopts(c))
    assert gridder.cache_stats['miss'] == start + 1
    assert wc.rel_l2(again.cpu().numpy(), 2 * first.cpu().numpy()) <= 1e-12
    # both directions of the plain operators share the plan of the geometry as well
    kws = dict(pixsize_x=c['px'], pixsize_y=c['py'], epsilon=c['eps'], do_wgridding=True)
    gridder.dirty2vis(uvw, freq, x, mask=mask, **kws)
    gridder.vis2dirty(uvw, freq, dev(c['vis']), mask=mask, npix_x=c['nx'], npix_y=c['ny'], **kws)
    assert gridder.cache_stats['miss'] == start + (1 if (c['cx'], c['cy']) == (0.0, 0.0) else 2)
    # another geometry, or new contents behind the same tensor, is another plan
    gridder.vis2dirty(uvw, freq, dev(c['vis']), mask=mask, npix_x=c['nx'] + 2, npix_y=c['ny'], **kws)
    n = gridder.cache_stats['miss']
    uvw.mul_(1.0)
    gridder.dirty2vis(uvw, freq, x, mask=mask, **kws)
    assert gridder.cache_stats['miss'] == n + 1


# ------------------------------------------------------------------------------------------- the native refusals
def test_native_entry_points_refuse_as_before():
    """What csrc/wgrid.hip refuses, status by status, through the C ABI itself.  Every case but the last is refused
    before any launch; the pointers are real device arrays all the same, so that a check that wrongly let one through
    would address nothing wild."""
    import ctypes as C
    from pfb_clean_amd import _lib
    lib = _lib.load()
    OK, INV, UNS = _lib.PFB_OK, _lib.PFB_ERR_INVALID, _lib.PFB_ERR_UNSUPPORTED
    stream = torch.cuda.current_stream().cuda_stream

    def create(dtype=_lib.PFB_F32, nx=16, ny=16, support=4, nplanes=1, w0=0.0, dw=1.0):
        h = C.c_void_p()
        return lib.pfb_wgrid_plan_create(dtype, nx, ny, 1e-3, 1e-3, 0.0, 0.0, support, nplanes, w0, dw, C.byref(h)), h

    assert lib.pfb_wgrid_plan_create(_lib.PFB_F32, 16, 16, 1e-3, 1e-3, 0.0, 0.0, 4, 1, 0.0, 1.0, None) == INV
    assert create(dtype=2)[0] == INV
    assert create(support=3)[0] == UNS and create(support=13)[0] == UNS
    assert create(nx=15)[0] == INV
    assert create(nplanes=2)[0] == INV and create(nplanes=4)[0] == INV       # nplanes == 1 || nplanes > support
    assert lib.pfb_wgrid_plan_info(None, None, None, None) == INV

    def call(name, args):
        return getattr(lib, 'pfb_wgrid_' + name)(*args, stream)

    def changed(args, **at):
        out = list(args)
        for k, v in at.items():
            out[int(k[1:])] = v
        return out

    # entry point -> positions of the plane, the slot count and the required pointers in its argument list
    where = {'order_count': (None, None, (1, 2, 6, 7)), 'order_fill': (None, None, (1, 2, 5, 6, 7, 9, 10)),
             'prep': (None, 5, (1, 3, 4, 6)), 'finish': (None, 5, (1, 3, 4, 6)), 'weight': (None, 4, (1, 3, 5)),
             'grid': (1, None, (2, 3, 7)), 'degrid': (1, None, (2, 3, 7)), 'image_forward': (1, None, (2, 4, 6)),
             'image_adjoint': (1, None, (2, 4)), 'image_correct': (None, None, (1, 2, 4))}
    plans = []
    try:
        for dtype, rdt, cdt, nplanes in ((_lib.PFB_F32, torch.float32, torch.complex64, 1),
                                         (_lib.PFB_F64, torch.float64, torch.complex128, 6)):
            rc, h = create(dtype=dtype, nplanes=nplanes)
            assert rc == OK
            plans.append(h)
            n, nrow, nchan = 8, 4, 2
            bufs = [torch.zeros(32 * 32 + 1, dtype=cdt, device='cuda'), torch.zeros(16 * 16 + 1, dtype=rdt, device='cuda'),
                    torch.zeros(16 * 16 + 1, dtype=torch.float64, device='cuda'),
                    torch.zeros(64, dtype=torch.int32, device='cuda'), torch.zeros(16, dtype=torch.int64, device='cuda')]
            c, r, f64, i32, i64 = (b.data_ptr() for b in bufs)
            good = {'order_count': [h, f64, f64, None, nrow, nchan, i32, i32],
                    'order_fill': [h, f64, f64, nrow, nchan, i32, i64, i32, n, i32, f64],
                    'prep': [h, c, r, i32, f64, n, c], 'finish': [h, c, r, i32, f64, n, c, n],
                    'weight': [h, c, r, i32, n, c], 'grid': [h, 0, c, f64, n, 0, n, c],
                    'degrid': [h, 0, c, f64, n, 0, n, c], 'image_forward': [h, 0, r, r, f64, f64, c],
                    'image_adjoint': [h, 0, c, f64, c], 'image_correct': [h, c, f64, r, r]}
            for name, args in good.items():
                plane, slots, required = where[name]
                assert call(name, changed(args, a0=None)) == INV, name
                if plane is not None:
                    assert call(name, changed(args, a1=-1)) == INV and call(name, changed(args, a1=nplanes)) == INV, name
                if slots is not None:
                    assert call(name, changed(args, **{f'a{slots}': 0})) == INV, name
                for k in required:
                    assert call(name, changed(args, **{f'a{k}': None})) == INV, (name, k)
            for name in ('grid', 'degrid'):
                assert call(name, changed(good[name], a5=5, a6=4)) == INV and call(name, changed(good[name], a6=n + 1)) == INV
            # each kind of pointer off by half its element
            half_r = bufs[1].element_size() // 2
            assert call('prep', changed(good['prep'], a1=c + 2 * half_r)) == INV           # complex of the plan's type
            assert call('prep', changed(good['prep'], a2=r + half_r)) == INV               # real of the plan's type
            assert call('grid', changed(good['grid'], a3=f64 + 4)) == INV                  # fp64 coord
            assert call('order_fill', changed(good['order_fill'], a9=i32 + 2)) == INV      # int32 idx
            # the optional pointers may be null: one launch on 16 x 16
            assert call('image_correct', changed(good['image_correct'], a3=None)) == OK
            torch.cuda.synchronize()
    finally:
        for h in plans:
            lib.pfb_wgrid_plan_destroy(h)
