"""
image_data_products on the MI355X (pfb_clean_amd.operators.gridder) against the direct Fourier sums of
tests/wgrid_cases.py, on four cases of its table with nx_psf, ny_psf = 2 nx, 2 ny.

Bounds
  DIRTY, PSF   against the direct sum with the returned WEIGHT at epsilon (ducc0's statement, as in test_gpu_wgrid.py).
  RESIDUAL     against the direct R^H W (vis - R model): the difference is at most
               2 epsilon (|R^H W vis| + |R^H W R model|), two gridder applications (the precedent of test_hessian_impl).
  PSFHAT       against np.fft.rfft2(np.fft.ifftshift(PSF)) of the returned PSF within 1e-11 max|ref| in fp64
               (test_gpu_dist_compose.py's bound for psfhat_from_psf).
  WEIGHT       natural: the input, which is unchanged; Briggs: wgt * _counts_to_weights(...) of the GPU functions at
               2 u(T); l2: the numpy statement fed with the GPU's own dirty2vis(model) at the l2 bound of
               test_gpu_weighting.py (degridding is a gather with a fixed sum order: the same input as inside).
  WSUM         shape (1,), within 2 (16 + ceil(log2(nvis))) u(T) of WEIGHT[mask].sum().
  consumer     hessian_xds, fed with the returned WEIGHT and WSUM on a delta model, reproduces the PSF's centre crop at
               3 epsilon.
"""
import numpy as np
import pytest
import torch

import weighting_cases as wcs
import wgrid_cases as wc

pytestmark = pytest.mark.gpu

NAMES = ['32x24-eps1e-05', '48x16-eps1e-07', 'centre', 'no-wgrid']
_memo = {}


def memo(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def idp_case(name):
    """A table case with everything image_data_products takes: weights and a mask where the table has none, a model."""
    def make():
        base = wc.CASES[wc.CASE_IDS.index(name)]
        c = dict(base, divide_by_n=False)
        if c['cx'] or c['cy']:
            # the delta of the PSF branch lives on 128 x 128 pixels, which at the table's pixel sizes reach beyond the
            # horizon (64 * 0.03 rad): the same case on pixels a quarter the size, the baselines four times as long
            # -- every visibility keeps its place on the uv grid
            c.update(px=c['px'] / 4, py=c['py'] / 4, uvw=c['uvw'] * 4.0)
        rng = np.random.default_rng(31)
        shape = c['vis'].shape
        if c['wgt'] is None:
            c['wgt'] = rng.uniform(0.5, 1.5, shape)
        if c['mask'] is None:
            c['mask'] = (rng.uniform(size=shape) < 0.8).astype(np.uint8)
        c['mask'] = c['mask'].astype(np.uint8)
        c['model'] = np.zeros((c['nx'], c['ny']))
        c['model'][rng.integers(0, c['nx'], 6), rng.integers(0, c['ny'], 6)] = rng.uniform(0.5, 2.0, 6)
        return c
    return memo(('case', name), make)


def psf_geometry(c):
    return dict(c, nx=2 * c['nx'], ny=2 * c['ny'])


def products(c, **kw):
    from pfb_clean_amd.operators.gridder import image_data_products
    args = dict(model=None, robustness=None, x0=c['cx'], y0=c['cy'], nthreads=2, epsilon=c['eps'],
                do_wgridding=c['do_wgridding'])
    args.update(kw)
    wgt = args.pop('wgt', c['wgt'])
    counts = args.pop('counts', None)
    vis, mask = args.pop('vis', c['vis']), args.pop('mask', c['mask'])
    return image_data_products(c['uvw'], c['freq'], vis, wgt, mask, counts, c['nx'], c['ny'], 2 * c['nx'], 2 * c['ny'],
                               c['px'], c['py'], **args)


def gpu_counts(c, dtype=np.float64):
    from pfb_clean_amd.utils.weighting import compute_counts
    return memo(('counts', c['name'], dtype), lambda: compute_counts(c['uvw'], c['freq'], c['mask'], c['nx'], c['ny'],
                                                                     c['px'], c['py'], dtype, k=6, ngrid=2))


def psf_vis_of(c):
    """The visibilities the PSF is made of: ones, or for a centre off the origin the degridded 128 x 128 delta."""
    if not (c['cx'] or c['cy']):
        return np.ones(c['vis'].shape, np.complex128)
    delta = np.zeros((128, 128))
    delta[64, 64] = 1.0
    return wc.direct_dirty2vis(dict(c, nx=128, ny=128, mask=None), delta, wgt=None)


def check_images(c, out, vis, model=None):
    eps, W, mask = c['eps'], out['WEIGHT'].astype(np.float64), c['mask']
    e_dirty = wc.rel_l2(out['DIRTY'].astype(np.float64), wc.direct_vis2dirty(c, vis, wgt=W))
    e_psf = wc.rel_l2(out['PSF'].astype(np.float64), wc.direct_vis2dirty(psf_geometry(c), psf_vis_of(c), wgt=W))
    print(f"{c['name']}: eps {eps:g} DIRTY {e_dirty:.3e} PSF {e_psf:.3e}")
    assert out['DIRTY'].shape == (c['nx'], c['ny']) and out['PSF'].shape == (2 * c['nx'], 2 * c['ny'])
    assert e_dirty <= eps and e_psf <= eps
    ref_hat = np.fft.rfft2(np.fft.ifftshift(out['PSF'].astype(np.float64)))
    assert out['PSFHAT'].shape == ref_hat.shape
    if out['PSF'].dtype == np.float64:
        assert np.abs(out['PSFHAT'] - ref_hat).max() <= 1e-11 * np.abs(ref_hat).max()
    tag = 'f64' if out['WEIGHT'].dtype == np.float64 else 'f32'
    exact = W[mask != 0].sum()
    assert out['WSUM'].shape == (1,) and out['WSUM'].dtype == out['WEIGHT'].dtype
    assert abs(float(out['WSUM'][0]) - exact) <= wcs.wsum_bound(mask.size, tag) * exact
    if model is not None:
        Rm = wc.direct_dirty2vis(c, model, wgt=None)
        a, b = wc.direct_vis2dirty(c, vis, wgt=W), wc.direct_vis2dirty(c, Rm, wgt=W)
        err = np.linalg.norm(out['RESIDUAL'].astype(np.float64) - (a - b))
        print(f"{c['name']}: RESIDUAL err {err:.3e} bound {2 * eps * (np.linalg.norm(a) + np.linalg.norm(b)):.3e}")
        assert err <= 2 * eps * (np.linalg.norm(a) + np.linalg.norm(b))


@pytest.mark.parametrize('name', NAMES)
def test_natural_weights(name):
    from pfb_clean_amd.operators import gridder
    c = idp_case(name)
    keep = c['wgt'].copy()
    gridder.clear_plan_cache()
    start = gridder.cache_stats['miss']
    out = products(c)
    # one plan per geometry: (nx, ny) and (nx_psf, ny_psf); a centre off the origin adds the delta's 128 x 128
    assert gridder.cache_stats['miss'] == start + (3 if (c['cx'] or c['cy']) else 2)
    assert set(out) == {'WEIGHT', 'WSUM', 'DIRTY', 'PSF', 'PSFHAT'}
    assert all(isinstance(v, np.ndarray) for v in out.values())
    assert np.array_equal(out['WEIGHT'], keep) and np.array_equal(c['wgt'], keep)
    check_images(c, out, c['vis'])
    again = products(c, model=c['model'])               # the model, dirty and residual images share the first plan
    assert gridder.cache_stats['miss'] == start + (3 if (c['cx'] or c['cy']) else 2)
    assert set(again) == set(out) | {'RESIDUAL'}


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('robust', [-3, 0])
def test_briggs_weights_and_the_residual(name, robust):
    from pfb_clean_amd.utils.weighting import _counts_to_weights
    c = idp_case(name)
    keep = c['wgt'].copy()
    counts = gpu_counts(c)
    out = products(c, counts=counts, robustness=robust, model=c['model'])
    assert set(out) == {'WEIGHT', 'WSUM', 'DIRTY', 'PSF', 'PSFHAT', 'RESIDUAL'}
    imwgt = _counts_to_weights(counts, c['uvw'], c['freq'], c['nx'], c['ny'], c['px'], c['py'], robust)
    exp = c['wgt'] * imwgt
    assert np.array_equal(c['wgt'], keep)                         # the reference's `wgt *= imwgt` writes; this does not
    assert (np.abs(out['WEIGHT'] - exp) <= 2 * wcs.U['f64'] * exp).all()
    check_images(c, out, c['vis'], c['model'])


@pytest.mark.parametrize('name', NAMES)
def test_l2_reweight(name):
    from pfb_clean_amd.operators.gridder import dirty2vis
    from pfb_clean_amd.utils.weighting import _counts_to_weights
    c = idp_case(name)
    dof = 2
    model_vis = dirty2vis(c['uvw'], c['freq'], c['model'], mask=c['mask'], pixsize_x=c['px'], pixsize_y=c['py'],
                          center_x=c['cx'], center_y=c['cy'], epsilon=c['eps'], do_wgridding=c['do_wgridding'],
                          divide_by_n=False)
    _, ref_w = wcs.np_l2(c['vis'], model_vis, c['mask'], dof)
    out = products(c, model=c['model'], l2reweight_dof=dof)
    rel = np.abs(out['WEIGHT'] - ref_w) / ref_w
    print(f"{name}: l2 WEIGHT worst relative error {rel.max() / wcs.U['f64']:.2f} u")
    assert (rel <= wcs.l2_bound(c['mask'].size, 'f64')).all()
    check_images(c, out, c['vis'], c['model'])
    # with a robustness on top: the product is formed in the same kernel
    counts = gpu_counts(c)
    both = products(c, model=c['model'], l2reweight_dof=dof, counts=counts, robustness=0.5)
    imwgt = _counts_to_weights(counts, c['uvw'], c['freq'], c['nx'], c['ny'], c['px'], c['py'], 0.5)
    assert np.array_equal(both['WEIGHT'], out['WEIGHT'] * imwgt)
    exact = both['WEIGHT'][c['mask'] != 0].sum()
    assert abs(float(both['WSUM'][0]) - exact) <= wcs.wsum_bound(c['mask'].size, 'f64') * exact


def test_single_precision_and_tensors():
    c = wc.as_f32(dict(idp_case('32x24-eps1e-05'), eps=1e-5))
    c['wgt'] = c['wgt'].astype(np.float32)
    counts = gpu_counts(c, np.float32)
    out = products(c, counts=counts, robustness=0, model=c['model'].astype(np.float32))
    assert all(out[k].dtype == np.float32 for k in ('WEIGHT', 'WSUM', 'DIRTY', 'PSF', 'RESIDUAL'))
    assert out['PSFHAT'].dtype == np.complex64
    check_images(c, out, c['vis'], c['model'])
    from pfb_clean_amd.operators.gridder import image_data_products
    t = image_data_products(dev(c['uvw']), dev(c['freq']), dev(c['vis']), dev(c['wgt']), dev(c['mask']), dev(counts),
                            c['nx'], c['ny'], 2 * c['nx'], 2 * c['ny'], c['px'], c['py'], robustness=0, epsilon=c['eps'],
                            do_wgridding=True, double_accum=False)
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in t.values())
    assert np.array_equal(t['WEIGHT'].cpu().numpy(), out['WEIGHT'])           # no atomics after the counts: bit for bit
    assert wc.rel_l2(t['DIRTY'].cpu().numpy().astype(np.float64), out['DIRTY'].astype(np.float64)) <= 2 * c['eps']


def test_key_presence_and_errors():
    c = idp_case('32x24-eps1e-05')
    assert set(products(c, do_psf=False)) == {'WEIGHT', 'WSUM', 'DIRTY'}
    assert set(products(c, do_weight=False)) == {'WSUM', 'DIRTY', 'PSF', 'PSFHAT'}
    assert set(products(c, do_psf=False, do_weight=False, model=c['model'])) == {'WSUM', 'DIRTY', 'RESIDUAL'}
    with pytest.raises(ValueError, match='Requested l2 reweight but no model passed in'):
        products(c, l2reweight_dof=2)
    with pytest.raises(ValueError, match='counts are None but robustness specified'):
        products(c, robustness=0.0)
    with pytest.raises(ValueError):
        products(c, wgt=None)
    # robustness alone supplies the weights
    only = products(c, wgt=None, counts=gpu_counts(c), robustness=-1.0, do_psf=False)
    assert only['WEIGHT'].shape == c['vis'].shape and only['WEIGHT'].dtype == np.float64


def test_all_zero_mask():
    c = idp_case('32x24-eps1e-05')
    out = products(c, mask=np.zeros(c['vis'].shape, np.uint8))
    assert not out['DIRTY'].any() and not out['PSF'].any() and not out['PSFHAT'].any()
    assert out['WSUM'].shape == (1,) and out['WSUM'][0] == 0
    # the l2 reweight finds no sample: the reference's `wgt = None`, and the robustness supplies the weights
    z = products(c, mask=np.zeros(c['vis'].shape, np.uint8), model=c['model'], l2reweight_dof=2, counts=gpu_counts(c),
                 robustness=0.0, do_psf=False)
    assert z['WSUM'][0] == 0 and not z['RESIDUAL'].any()


class _Var:
    def __init__(self, a):
        self.values, self.dtype, self.shape = a, a.dtype, a.shape


class _DS(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


@pytest.mark.parametrize('name', ['32x24-eps1e-05', 'no-wgrid'])
def test_the_hessian_of_a_delta_is_the_psf(name):
    """The product and its consumer: hessian_xds with the returned WEIGHT and WSUM on a centre delta gives
    PSF[centre crop] / WSUM."""
    from pfb_clean_amd.operators.hessian import hessian_xds
    c = dict(idp_case(name))
    c['px'] = c['py'] = min(c['px'], c['py'])                     # the Hessian takes one cell size
    c['name'] = name + '-square'
    nx, ny, eps = c['nx'], c['ny'], c['eps']
    out = products(c, counts=gpu_counts(c), robustness=0.0)
    ds = _DS(UVW=_Var(c['uvw']), FREQ=_Var(c['freq']), WEIGHT=_Var(out['WEIGHT']), MASK=_Var(c['mask']), bandid=0)
    x = np.zeros((1, nx, ny))
    x[0, nx // 2, ny // 2] = 1.0
    opts = dict(cell=c['px'], do_wgridding=c['do_wgridding'], epsilon=eps, double_accum=True, nthreads=1)
    got = hessian_xds(x, [ds], opts, float(out['WSUM'][0]), 0.0, np.ones((nx, ny)), use_beam=False)
    crop = out['PSF'][nx - nx // 2:nx - nx // 2 + nx, ny - ny // 2:ny - ny // 2 + ny] / out['WSUM'][0]
    err = wc.rel_l2(got[0], crop)
    print(f"{name}: hessian_xds(delta) against the PSF crop {err:.3e} (eps {eps:g})")
    assert err <= 3 * eps
