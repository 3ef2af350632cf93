"""
The w-gridder's recipe on the CPU (no GPU): the support rule, the plane layout and the correction tables of
operators/gridder.py; the numpy model of the recipe against the direct sums on every case of wgrid_cases.CASES, which is
the condition under which the GPU tests' bound `epsilon` means something; and a proof that the table holds every edge
it claims.
"""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import wgrid_cases as wc                                       # noqa: E402
from wgrid_cases import CASES, CASE_IDS                        # noqa: E402


def test_support_rule_and_epsilon_range():
    import torch
    from pfb_clean_amd.operators import gridder
    for eps, W in ((1e-2, 4), (1e-3, 5), (1e-4, 6), (1e-5, 7), (3e-6, 8), (1e-7, 9), (1e-9, 11), (1e-10, 12)):
        assert gridder.support_for(eps) == W == wc.support(eps)
    assert gridder.EPS_MIN[torch.float64] == 1e-10 and gridder.EPS_MAX == 1e-2
    for eps, dt in ((2e-2, torch.float64), (5e-11, torch.float64), (0.0, torch.float64), (float('nan'), torch.float32),
                    (0.5 * gridder.EPS_MIN[torch.float32], torch.float32)):
        with pytest.raises(ValueError):
            gridder.check_epsilon(eps, dt)
    assert gridder.check_epsilon(1e-10, torch.float64) == 1e-10 and gridder.check_epsilon(1e-2, torch.float32) == 1e-2


def test_plane_layout():
    from pfb_clean_amd.operators import gridder
    counts = []
    for c in CASES:
        pl = wc.planes(c)
        if pl is None:
            continue
        w = wc.coords(c)[2]
        w = w if c['mask'] is None else w[c['mask'] != 0]
        max_nm1 = float(np.abs(wc.lmn(c)[2]).max())
        W = wc.support(c['eps'])
        got = gridder.plane_layout(float(w.min()), float(w.max()), max_nm1, W, c['eps'], c['do_wgridding'])
        assert got == pytest.approx(pl, rel=1e-15)
        nplanes, w0, dw = pl
        if nplanes > 1:
            assert dw == 1.0 / (4.0 * max_nm1) and w0 == w.min() - 0.5 * W * dw
            assert nplanes == math.ceil((w.max() - w.min()) / dw) + W + 1
            # every visibility's W planes exist
            first = np.ceil((w - w0) / dw - 0.5 * W)
            assert first.min() >= 0 and first.max() + W - 1 <= nplanes - 1
            counts.append(nplanes)
        else:
            assert not c['do_wgridding'] or w.min() == w.max()
    assert min(counts) <= 25 and max(counts) >= 100 and any(40 <= n <= 70 for n in counts), sorted(counts)


@pytest.mark.parametrize('W', [4, 5, 8, 9, 12])
def test_correction_tables_against_brute_force(W):
    from pfb_clean_amd.operators import gridder
    ts = np.array([0.0, 0.03, 0.125, 0.2, 0.25, -0.25])
    got = gridder.kernel_correction(W, ts)
    assert np.array_equal(got, wc.correction(W, ts))
    for t, g in zip(ts, got):
        assert abs(g - wc.correction_brute(W, t)) <= 1e-9 * abs(g)
    assert got[4] == got[5] and got[0] > got[4] > 0.0
    # more nodes change nothing: the quadrature has converged
    assert np.abs(wc.correction(W, ts, nodes=256) - got).max() <= 1e-14 * got[0]


@pytest.mark.parametrize('W', [4, 9, 12])
def test_correction_tables_keep_their_bits(W):
    """kernel_correction through the shared quadrature against the formula as it stood before there was one, operation
    for operation: the same bits."""
    from pfb_clean_amd.operators import gridder
    t = np.linspace(-0.25, 0.25, 33)
    h = 0.5 * W
    th, wq = np.polynomial.legendre.leggauss(128)
    th, wq = th * (np.pi / 2), wq * (np.pi / 2)
    f = np.exp(2.3 * W * (np.cos(th) - 1.0)) * np.cos(th) * wq
    was = h * (np.cos(2 * np.pi * h * t[..., None] * np.sin(th)) * f).sum(-1)
    assert np.array_equal(gridder.kernel_correction(W, t), was)
    # the device table's nodes: the same frequencies and weights, in the same order
    x, fq = gridder._quadrature(W)
    assert np.array_equal(2 * np.pi * h * x, 2 * np.pi * h * np.sin(th)) and np.array_equal(fq, f)


_model_err = {}


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_model_meets_epsilon_both_directions(case):
    """The recipe itself: relative L2 error of the numpy model against the direct sum <= epsilon, both directions."""
    if case['mask'] is not None and not case['mask'].any():
        assert not wc.model_vis2dirty(case, case['vis']).any() and not wc.model_dirty2vis(case, case['dirty']).any()
        assert not wc.direct_vis2dirty(case, case['vis']).any() and not wc.direct_dirty2vis(case, case['dirty']).any()
        return
    e1 = wc.rel_l2(wc.model_vis2dirty(case, case['vis']), wc.direct_vis2dirty(case, case['vis']))
    e2 = wc.rel_l2(wc.model_dirty2vis(case, case['dirty']), wc.direct_dirty2vis(case, case['dirty']))
    _model_err[case['name']] = (e1, e2)
    print(f"{case['name']}: eps {case['eps']:g} vis2dirty {e1:.3e} dirty2vis {e2:.3e}")
    assert e1 <= case['eps'] and e2 <= case['eps']


@pytest.mark.parametrize('name', ['32x24-eps1e-05', '48x16-eps1e-07', 'no-wgrid', 'centre'])
def test_model_hessian_meets_twice_epsilon(name):
    """The composition the GPU Hessian test bounds by 2 epsilon, and the symmetry of the model's H."""
    case = dict(CASES[CASE_IDS.index(name)], divide_by_n=False)
    rng = np.random.default_rng(11)
    beam = rng.uniform(0.5, 1.0, (case['nx'], case['ny']))
    x, y = rng.standard_normal((2, case['nx'], case['ny']))

    def H(z):
        vis = wc.model_dirty2vis(dict(case, wgt=None), beam * z)
        return beam * wc.model_vis2dirty(case, vis)
    Hx = H(x)
    assert wc.rel_l2(Hx, wc.direct_hessian(case, x, beam)) <= 2 * case['eps']
    assert abs(np.vdot(y, Hx) - np.vdot(H(y), x)) <= 1e-12 * np.linalg.norm(y) * np.linalg.norm(Hx)


def test_model_is_adjoint_to_rounding():
    """<v, A d> = <A^T v, d> in the model: the two directions are exact adjoints, step by step."""
    for name in ('32x24-eps1e-05', 'centre', 'seam', 'no-wgrid'):
        case = CASES[CASE_IDS.index(name)]
        mm = wc.adjoint_mismatch(lambda v: wc.model_vis2dirty(case, v), lambda d: wc.model_dirty2vis(case, d), case)
        print(f"{name}: model adjoint mismatch {mm:.3e}")
        assert mm <= 1e-12          # a few hundred ulp of a sum of some thousand terms


def test_no_wgridding_hessian_is_the_psf_convolution():
    """Without the w term H x = psf (*) x with psf = vis2dirty(ones, wgt) on (2 nx, 2 ny): exact, to rounding."""
    case = dict(CASES[CASE_IDS.index('no-wgrid')], divide_by_n=False)
    nx, ny = case['nx'], case['ny']
    big = dict(case, nx=2 * nx, ny=2 * ny)
    psf = wc.direct_vis2dirty(big, np.ones(case['vis'].shape, complex))
    x = np.random.default_rng(3).standard_normal((nx, ny))
    xpad = np.zeros((2 * nx, 2 * ny))
    xpad[:nx, :ny] = x
    conv = np.fft.irfft2(np.fft.rfft2(xpad) * np.fft.rfft2(np.fft.ifftshift(psf)), s=(2 * nx, 2 * ny))[:nx, :ny]
    assert wc.rel_l2(conv, wc.direct_hessian(case, x, None)) <= 1e-12


def test_table_covers_every_axis_and_edge():
    """Each axis value and each placement edge of the table is really there."""
    by_edge = {}
    for c in CASES:
        for e in c['edges']:
            by_edge.setdefault(e, []).append(c)
    # ---- axes
    f64 = [c for c in CASES if c['dtype'] == 'f64']
    assert list(wc.IMAGES)[:3] == ['32x24', '48x16', '16x64']
    for image in list(wc.IMAGES)[:3]:
        assert {c['eps'] for c in f64 if c['image'] == image} >= {1e-3, 1e-5, 1e-7, 1e-9}
    # every support 4 .. 12 is launched, the first and the last rung of the dispatch included (W = 6 in fp32 only:
    # test_gpu_wgrid_kernels.py runs every support in both types)
    assert {wc.support(c['eps']) for c in CASES} == set(range(4, 13))
    assert {wc.support(c['eps']) for c in f64} == set(range(4, 13)) - {6}
    for W in (4, 10, 12):
        assert any(wc.support(c['eps']) == W and (c['nx'] * c['ny']) % 256 != 0 for c in f64)
    # a partial last block of the image kernels, nx / 2 and ny / 2 odd, and a grid exactly as wide as the footprint
    for c in by_edge['partial_block']:
        assert (c['nx'] * c['ny']) % 256 != 0 and (c['nx'] // 2) % 2 == 1
        assert c['wgt'] is not None and 0 < c['mask'].sum() < c['mask'].size and c['uvw'].shape[0] == 257
    assert any(c['nx'] * c['ny'] > 256 for c in by_edge['partial_block'])
    assert any(c['nx'] * c['ny'] < 256 for c in by_edge['partial_block'])
    narrow = by_edge['grid_eq_support']
    assert {(2 * c['nx'] == wc.support(c['eps']), 2 * c['ny'] == wc.support(c['eps'])) for c in narrow} \
        == {(True, False), (False, True)}
    assert {c['eps'] for c in CASES if c['dtype'] == 'f32'} == {1e-3, 1e-4}
    shapes = {(c['uvw'].shape[0], c['freq'].size) for c in CASES}
    assert {n for n, _ in shapes} >= {1, 63, 65, 257} and {k for _, k in shapes} == {1, 3}
    assert any(c['wgt'] is None for c in CASES) and any(c['wgt'] is not None for c in CASES)
    assert any(c['mask'] is None for c in CASES)
    assert any(c['mask'] is not None and c['mask'].dtype == np.uint8 and 0 < c['mask'].sum() < c['mask'].size for c in CASES)
    assert any(c['mask'] is not None and c['mask'].dtype == bool for c in CASES)
    assert all(not c['mask'].any() for c in by_edge['mask0'])
    assert all(c['cx'] != 0 and c['cy'] != 0 for c in by_edge['centre'])
    assert all(not c['divide_by_n'] for c in by_edge['no_n']) and any(c['divide_by_n'] for c in CASES)
    assert all(not c['do_wgridding'] for c in by_edge['wgrid_off'])
    for c in CASES:
        l, m, _ = wc.lmn(c)
        assert (l * l + m * m).max() < 1.0
    for c in by_edge['wmin_eq_wmax']:
        w = wc.coords(c)[2]
        assert c['do_wgridding'] and w.min() == w.max() and wc.planes(c)[0] == 1
    for c in by_edge['w_one_sign']:
        assert wc.coords(c)[2].min() >= 0.0 and wc.planes(c)[0] > 1
    # ---- placement
    def cells(c):
        u, v, w = (a.reshape(-1) for a in wc.coords(c))
        return u * (c['px'] * 2 * c['nx']), v * (c['py'] * 2 * c['ny']), w
    for c in by_edge['seam_exact']:
        ug, vg, _ = cells(c)
        nx, ny, W = c['nx'], c['ny'], wc.support(c['eps'])
        assert (ug == nx).any() and (ug == -nx).any() and (vg == ny).any() and (vg == -ny).any()
        inside = (np.abs(ug) < nx) & (np.abs(ug) > nx - 1e-9)
        assert inside.any() and ((np.abs(vg) < ny) & (np.abs(vg) > ny - 1e-9)).any()
        a0 = np.ceil(ug - 0.5 * W)
        assert ((a0 < -nx) | (a0 + W - 1 >= nx)).any()           # a footprint crosses the seam of the (2 nx) grid
    ties = by_edge['ug_integer']
    assert {wc.support(c['eps']) % 2 for c in ties} == {0, 1}     # an even and an odd support: both are ceil ties
    for c in ties:
        ug, vg, _ = cells(c)
        for g in (ug, vg):
            fr = g - np.floor(g)
            assert (fr == 0.0).sum() >= 20 and (fr == 0.5).sum() >= 20
    for c in by_edge['uvw_zero']:
        assert (np.abs(c['uvw']).sum(axis=1) == 0).any()
    for c in by_edge['one_cell']:
        ug, vg, _ = cells(c)
        assert np.unique(np.floor(ug)).size == 1 and np.unique(np.floor(vg)).size == 1 and ug.size >= 200
    wp = by_edge['w_on_plane']
    assert {wc.support(c['eps']) % 2 for c in wp} == {0, 1}
    for c in wp:
        _, _, w = cells(c)
        nplanes, w0, dw = wc.planes(c)
        fr = (w - w0) / dw
        fr = fr - np.floor(fr)
        on = np.minimum(fr, 1 - fr) < 1e-9
        half = np.abs(fr - 0.5) < 1e-9
        assert on.sum() >= 50 and half.sum() >= 50
    assert len(CASES) <= 40 and all(c['uvw'].shape[0] * c['freq'].size <= 260 for c in CASES)
