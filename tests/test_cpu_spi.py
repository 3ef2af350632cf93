"""
The spectral-index oracles and cases (tests/spi_cases.py) on the CPU: the per-component oracle against
scipy.optimize.curve_fit, the conditions on the stored cases, the numpy oracle of fit_spi on hand-made cubes, and the
argument checks of pfb_clean_amd.utils.spi.fit_spi that run before anything touches a device.

Oracle against curve_fit (sigma = 1 / sqrt(w), absolute_sigma=False, xtol = ftol = gtol = 1e-15, the oracle run to
tol = 1e-13) at 3, 4, 8 and 64 bands.  curve_fit differentiates by finite differences, which is what separates the
two.  Largest deviations measured over the four cases (CPU, numpy 2.2, scipy 1.15):
    alpha      1.29e-7 absolute           bound 2.6e-6
    alpha_err  4.55e-6 relative           bound 9.1e-5
    I0         6.34e-9 relative           bound 1.3e-7
    I0_err     5.32e-7 relative           bound 1.1e-5
The bounds are 20 x the measured values.
"""
import numpy as np
import pytest
from scipy.optimize import curve_fit

import spi_cases as sc

CURVE_FIT_BOUND = {'alpha': 2.6e-6, 'alpha_err': 9.1e-5, 'I0': 1.3e-7, 'I0_err': 1.1e-5}
NCASE = len(sc.CASES)


def test_case_table():
    assert sorted(c[0] for c in sc.CASES) == [2, 3, 4, 8, 63, 64]
    assert {c[2] for c in sc.CASES} == {0.01, 0.10}
    for i in range(NCASE):
        c = sc.case(i)
        for k in ('data', 'beam'):
            assert c[k].dtype == np.float32 and c[k].shape == (c['ncomps'], c['nband'])
        assert c['beam'].min() >= np.float32(0.3) and c['beam'].max() <= 1.0
        assert c['weights'].min() >= 0.5 and c['weights'].max() <= 2.0
        assert -2.0 <= c['alpha'].min() and c['alpha'].max() <= 1.0
        assert 1e-3 <= c['I0'].min() and c['I0'].max() <= 10.0


@pytest.mark.parametrize('i', [i for i in range(NCASE) if sc.CASES[i][0] in (3, 4, 8, 64)])
def test_oracle_against_curve_fit(i):
    c = sc.case(i)
    got = sc.oracle(c, tol=1e-13)
    x = c['freqs'] / c['ref_freq']
    sigma = 1.0 / np.sqrt(c['weights'])
    ref = int(np.argmin(np.abs(c['freqs'] - c['ref_freq'])))
    dev = np.zeros(4)
    for k in range(c['ncomps']):
        d, B = c['data'][k].astype(np.float64), c['beam'][k].astype(np.float64)
        p, cov = curve_fit(lambda x_, a, I: I * B * x_ ** a, x, d, p0=(-0.7, d[ref]), sigma=sigma,
                           absolute_sigma=False, xtol=1e-15, ftol=1e-15, gtol=1e-15, maxfev=10000)
        e = np.sqrt(np.diag(cov))
        dev = np.maximum(dev, [abs(p[0] - got[0, k]), abs(e[0] - got[1, k]) / got[1, k],
                               abs(p[1] - got[2, k]) / abs(got[2, k]), abs(e[1] - got[3, k]) / got[3, k]])
    print(sc.CASES[i], dict(zip(sc.OUTPUTS, dev)))
    for name, v in zip(sc.OUTPUTS, dev):
        assert v <= CURVE_FIT_BOUND[name], (name, v)


@pytest.mark.parametrize('i', range(NCASE))
def test_case_conditions(i):
    c = sc.case(i)
    held = [0, 2] if c['nband'] == 2 else [0, 1, 2, 3]
    for tol in (1e-5, 1e-10, 1e-13):
        out, info = sc.oracle(c, tol=tol, info=True)
        s = sc.spread(c, tol)
        print(sc.CASES[i], tol, 'steps', info['steps'].max(), 'spread', s)
        assert np.isfinite(out[held]).all()
        assert info['late'] == 0 and info['steps'].max() < 100
        assert (s[held] <= 1e-11).all()
    r = sc.rho(c)
    print(sc.CASES[i], 'rho', r)
    assert r <= 0.5
    # the run to the default tol lies within tol of the converged one: the last step is <= tol and rho <= 0.5
    assert np.abs(sc.oracle(c)[held] - sc.oracle(c, tol=1e-13)[held]).max() <= 1e-5


def test_oracle_recovers_noiseless_power_law():
    freqs = np.linspace(1e9, 2e9, 5)
    alpha, I0 = np.array([-1.3, 0.4]), np.array([2.0, 0.05])
    B = np.array([[0.9, 0.8, 0.7, 0.6, 0.5], [1.0, 1.0, 1.0, 1.0, 1.0]])
    d = I0[:, None] * B * (freqs / 1.5e9)[None, :] ** alpha[:, None]
    out, info = sc.fit_components(d, np.ones(5), freqs, 1.5e9, beam=B, tol=1e-12, info=True)
    assert np.allclose(out[0], alpha, rtol=0, atol=1e-12) and np.allclose(out[2], I0, rtol=1e-12, atol=0)
    assert info['late'] == 0
    # beam=None is a beam of ones; starting values are honoured: started at the solution the first step is rounding
    out1, info1 = sc.fit_components(d[1:], np.ones(5), freqs, 1.5e9, alphai=alpha[1:], I0i=I0[1:], info=True)
    assert info1['steps'].tolist() == [1] and abs(out1[0, 0] - alpha[1]) < 1e-12


def test_oracle_step_limit_and_degenerate():
    c = sc.case(3)
    one, info = sc.oracle(c, maxiter=1, info=True)
    assert info['late'] == c['ncomps'] and (info['steps'] == 1).all()
    assert np.abs(one[0] - sc.oracle(c)[0]).max() > 1e-3                     # one step is not the answer
    d = c['data'].astype(np.float64)
    assert np.isnan(sc.fit_components(d, np.zeros(c['nband']), c['freqs'], c['ref_freq'])).all()
    d0 = np.vstack((d[:3], np.zeros((1, c['nband']))))
    ref = int(np.argmin(np.abs(c['freqs'] - c['ref_freq'])))
    out = sc.fit_components(d0, c['weights'], c['freqs'], c['ref_freq'], I0i=np.array([*d[:3, ref], 0.0]))
    assert np.isnan(out[:, 3]).all() and np.isfinite(out[:, :3]).all()


def _cube():
    c = sc.case(3)
    image, beam = sc.cube_of(c, 5, 7, [(0, 0), (2, 3), (4, 6), (1, 1), (3, 2), (4, 0)])
    image[2, 1, 1] = np.nan                      # NaN in one band
    beam[5, 3, 2] = np.nan                       # NaN beam: cut to 0 in that band
    beam[:, 4, 0] = 0.25                         # beam == pb_min exactly: cut
    return c, image, beam


def test_fit_spi_oracle_mask_and_maps():
    c, image, beam = _cube()
    am, aem, im, iem, idx = sc.fit_spi(image, beam, c['freqs'], c['weights'], 0.0, 0.25, c['ref_freq'])
    assert idx.tolist() == [[0, 0], [2, 3], [4, 6]]
    ref = sc.oracle(c)
    for k, m in enumerate((am, aem, im, iem)):
        assert m.dtype == np.float32 and m.shape == (5, 7)
        assert np.array_equal(~np.isnan(m), np.isin(np.arange(35).reshape(5, 7), [0, 17, 34]))
        assert np.array_equal(m[idx[:, 0], idx[:, 1]], ref[k, :3].astype(np.float32))
    # a negative threshold admits the pixel with one band cut to zero; the NaN pixel stays out
    idx = sc.fit_spi(image, beam, c['freqs'], c['weights'], -1.0, 0.25, c['ref_freq'])[4]
    assert [3, 2] in idx.tolist() and [1, 1] not in idx.tolist() and len(idx) == 35 - 1


def test_fit_spi_oracle_empty_mask_text():
    c, image, beam = _cube()
    with pytest.raises(ValueError) as e:
        sc.fit_spi(image, beam, c['freqs'], c['weights'], 1e3, 0.25, c['ref_freq'])
    assert str(e.value) == ("No components found above threshold. Try lowering your threshold."
                            "Max of convolved model is nan")
    image[2, 1, 1] = 0.0
    with pytest.raises(ValueError) as e:
        sc.fit_spi(image, beam, c['freqs'], c['weights'], 1e3, 0.25, c['ref_freq'])
    top = np.where(beam > 0.25, image, 0).max()
    assert str(e.value).endswith("threshold.Max of convolved model is %3.2e" % top) and top > 0


def test_fit_spi_argument_checks():
    from pfb_clean_amd.utils import spi
    assert spi.EMPTY_MASK == sc.EMPTY_MASK
    f, w = np.linspace(1e9, 2e9, 4), np.ones(4)
    cube = np.ones((4, 3, 3), dtype=np.float32)
    args = (0.0, 1, 0.1, 0.0, 1.5e9)
    bad = [(cube[0], cube, f, w), (cube, cube[0], f, w), (cube, cube[:, :2], f, w), (cube[:1], cube[:1], f[:1], w[:1]),
           (cube, cube, f[:3], w), (cube, cube, f, w[:3])]
    for image, beam, freqs, weights in bad:
        with pytest.raises(AssertionError):
            spi.fit_spi(image, beam, freqs, weights, *args)
