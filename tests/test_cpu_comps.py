"""
Component model, the part that needs no GPU: the public names and their signatures, the host design step (design
matrix + the strings that go into the .mds) against the REFERENCE's stored outputs (tests/golden/comps*.npz, written by
tests/golden/make_golden_comps.py), the ValueError cases and the 1-D geometry of the regrid.

The design matrix is checked through the stored coefficients: solving the weighted normal equations of Xfit in numpy
on the stored image must give the reference's coeffs within 1e-12 + 50 * spread (spread: the stored sensitivity of the
reference's own solve to a 1-ulp perturbation of the image), the bound of the GPU test.
"""
import inspect
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIT_TAGS = [f'fit{c}' for c in range(11)] + ['edge_zero', 'edge_full', 'edge_mixed']
_cache = {}


def load(name):
    if name not in _cache:
        with np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False) as z:
            _cache[name] = {k: z[k] for k in z.files}
    return _cache[name]


def fit_args(g, tag):
    nbt, nbf = (None if v < 0 else int(v) for v in g[tag + '_nbasis'])
    return dict(time=g[tag + '_time'], freq=g[tag + '_freq'], wgt=g.get(tag + '_wgt'), nbasist=nbt, nbasisf=nbf,
                method=str(g[tag + '_method']), sigmasq=float(g[tag + '_sigmasq']))


def test_public_names_and_signatures():
    from pfb_clean_amd.utils.misc import fit_image_cube, eval_coeffs_to_cube, eval_coeffs_to_slice
    g = load('comps_fit')
    for fn in (fit_image_cube, eval_coeffs_to_cube, eval_coeffs_to_slice):
        pars = inspect.signature(fn).parameters
        positional = [n for n, p in pars.items() if p.kind is p.POSITIONAL_OR_KEYWORD]
        assert positional == list(g['sig_' + fn.__name__]), fn.__name__
        extra = [n for n in pars if n not in positional]
        assert extra == ([] if fn is fit_image_cube else ['dtype']), fn.__name__
        if extra:
            assert pars['dtype'].kind is pars['dtype'].KEYWORD_ONLY and pars['dtype'].default is None
    sig = inspect.signature(fit_image_cube).parameters
    assert [sig[n].default for n in ('wgt', 'nbasist', 'nbasisf', 'method', 'sigmasq')] == [None, None, None, 'poly', 0]


def test_case_list_is_complete():
    g = load('comps_fit')
    assert int(g['nfit']) == 11
    for tag in FIT_TAGS:
        assert float(g[tag + '_spread']) <= 1e-11, tag
    assert sum((tag + '_wgt') in g for tag in FIT_TAGS) == 5
    assert g['edge_zero_coeffs'].shape == (4, 0) and g['edge_zero_Ix'].size == 0
    assert g['edge_mixed_Ix'].tolist() == [0, 4, 8] and g['edge_mixed_Iy'].tolist() == [0, 4, 6]
    assert np.array_equal(np.isnan(g['edge_mixed_coeffs']), np.array([[False, True, False]] * 4))


@pytest.mark.parametrize('tag', FIT_TAGS + ['sfit0', 'sfit1'])
def test_design_strings_and_matrix(tag):
    from pfb_clean_amd.utils.comps import fit_design
    g = load('comps_slice' if tag.startswith('sfit') else 'comps_fit')
    a = fit_args(g, tag)
    Xfit, expr, params, texpr, fexpr = fit_design(a['time'], a['freq'], a['nbasist'], a['nbasisf'], a['method'])
    assert [expr, texpr, fexpr] == list(g[tag + '_strings'])
    assert params == list(g[tag + '_params'])
    image = g[tag + '_image'].astype(np.float64)
    nrow = image.shape[0] * image.shape[1]
    ref = g[tag + '_coeffs']
    assert Xfit.shape == (nrow, ref.shape[0]) and Xfit.dtype == np.float64
    beta = image[:, :, g[tag + '_Ix'], g[tag + '_Iy']].reshape(nrow, -1)
    w = np.ones((nrow, 1)) if a['wgt'] is None else a['wgt'].reshape(nrow, 1)
    H = Xfit.T @ (w * Xfit) + a['sigmasq'] * np.eye(Xfit.shape[1])
    got = np.linalg.solve(H, Xfit.T @ (w * beta))
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = np.isfinite(ref)
    if ok.any():
        err = np.abs(got - ref)[ok].max() / np.abs(ref[ok]).max()
        assert err <= 1e-12 + 50 * float(g[tag + '_spread']), err


def test_fifteen_digit_floats_in_the_strings():
    """str() of a sympy float keeps 15 digits; the .mds stores these strings."""
    from pfb_clean_amd.utils.comps import fit_design
    _, expr, params, texpr, fexpr = fit_design(np.array([3600.0]), np.array([0.9e9, 1.2e9, 1.5e9]), 1, 3, 'poly')
    assert (expr, params) == ('f**2*f2 + f*f1 + t0', ['t0', 'f1', 'f2'])
    assert texpr == '0.000277777777777778*t' and fexpr == '1.11111111111111e-9*f'


def test_value_errors():
    from pfb_clean_amd.utils.comps import fit_design, basis_values, slice_geometry
    from pfb_clean_amd.utils.misc import fit_image_cube
    time, freq = np.array([3600.0]), np.linspace(1e9, 2e9, 4)
    img = np.ones((1, 4, 3, 3))
    for method in ('poly', 'Legendre'):
        with pytest.raises(ValueError):
            fit_image_cube(time, freq[:1], img[:, :1], method=method)
    with pytest.raises(ValueError):
        fit_image_cube(time, freq, img, method='spline')
    with pytest.raises(AssertionError):
        fit_design(time, freq, 2, 2, 'poly')
    with pytest.raises(AssertionError):
        fit_design(time, freq, 1, 5, 'Legendre')
    with pytest.raises(ValueError):
        basis_values(time, freq, 't0 + f1**2*f', ['t0', 'f1'], 't', 'f')
    with pytest.raises(ValueError):
        basis_values(time, freq, 't0*f1 + f', ['t0', 'f1'], 't', 'f')
    # RegularGridInterpolator(bounds_error=True): the padding always covers a finite output grid, a NaN centre
    # is neither padded for nor inside
    with pytest.raises(ValueError):
        slice_geometry(8, 8, 1.0, 1.0, 0.0, 0.0, 8, 8, 1.0, 1.0, np.nan, 0.0)


def test_basis_values():
    from pfb_clean_amd.utils.comps import basis_values
    E = basis_values(np.array([1.0, 2.0]), np.array([0.5, 1.0, 2.0]), 'f*f1 + f2*(3*f**2/2 - 1/2) + t*t1 + t0',
                     ['t0', 't1', 'f1', 'f2'], 't - 1.0', '2.0*f')
    assert E.shape == (6, 4)
    f = 2.0 * np.array([0.5, 1.0, 2.0])
    for i, t in enumerate((0.0, 1.0)):
        for j in range(3):
            assert np.array_equal(E[3 * i + j], [1.0, t, f[j], 3 * f[j] ** 2 / 2 - 1 / 2])


def test_slice_geometry():
    from pfb_clean_amd.utils.comps import slice_geometry
    c = 1.3e-3
    xin, yin, xo, yo, pads, interp = slice_geometry(40, 36, c, c, 0.0, 0.0, 40, 36, c, c, 0.0, 0.0)
    assert pads == (0, 0, 0, 0) and not interp and xin.size == 40 and np.array_equal(xin, xo)
    xin, yin, xo, yo, pads, interp = slice_geometry(40, 36, c, c, 0.0, 0.0, 80, 72, c, c, 5 * c, -3 * c)
    assert interp and xin.size == 40 + pads[0] + pads[1] and yin.size == 36 + pads[2] + pads[3]
    assert pads[0] >= 15 and pads[1] >= 25 and pads[2] >= 21 and pads[3] >= 15
    assert xin[0] <= xo[0] and xo[-1] <= xin[-1] and yin[0] <= yo[0] and yo[-1] <= yin[-1]
    assert np.allclose(xin[pads[0]:pads[0] + 40], (-20 + np.arange(40)) * c, rtol=1e-15, atol=0)
    # same centre and cell, two pixels more: padded, not interpolated
    _, _, _, _, pads, interp = slice_geometry(40, 36, 1.0, 1.0, 0.0, 0.0, 42, 38, 1.0, 1.0, 0.0, 0.0)
    assert pads == (1, 1, 1, 1) and not interp


def test_archives_are_small():
    for name in ('comps_fit', 'comps_eval', 'comps_slice'):
        assert os.path.getsize(os.path.join(GOLDEN, name + '.npz')) < (1 << 20), name
