"""
Clean-beam fit, the part that needs no GPU: the public name and its signature, the invariants of the golden file
(tests/golden/beamfit.npz, written by tests/golden/make_golden_beamfit.py) that the GPU tests rely on, and the host
helper that turns a lobe record into the optimiser's start point.
"""
import inspect
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'beamfit.npz')
SPREAD_CAP = 1e-11
_cache = {}


def load():
    if not _cache:
        with np.load(GOLDEN, allow_pickle=False) as z:
            _cache.update({k: z[k] for k in z.files})
    return _cache


def test_public_name_and_signature():
    from pfb_clean_amd.utils.misc import fitcleanbeam
    g = load()
    pars = inspect.signature(fitcleanbeam).parameters
    assert list(pars) == list(g['sig_fitcleanbeam'])
    assert [pars[k].default for k in ('level', 'pixsize', 'extent')] == g['sig_defaults'].tolist()


def test_bindings_declared():
    from pfb_clean_amd import _lib
    header = open(os.path.join(os.path.dirname(GOLDEN), '..', '..', 'include', 'pfb_hip.h')).read()
    for name in ('pfb_beamfit_work_bytes', 'pfb_beamfit_max', 'pfb_beamfit_lobe', 'pfb_beamfit_objective'):
        assert name in _lib.SIGNATURES and name + '(' in header
    from pfb_clean_amd.utils import beamfit
    assert f'#define PFB_BEAMFIT_RECORD {beamfit.RECORD}\n' in header


def test_golden_spreads_below_the_cap():
    g = load()
    assert float(g['spread_cap']) == SPREAD_CAP and int(g['nfit']) >= 3
    for k in range(int(g['nfit'])):
        for b in (32, 64):
            assert 0.0 <= float(g[f'fit{k}_spread{b}']) <= SPREAD_CAP
            ref = g[f'fit{k}_ref{b}']
            assert ref.shape == (g[f'fit{k}_psf'].shape[0], 3)
            # an all-zero band, and only that, is NaN
            assert np.array_equal(np.isnan(ref).all(axis=1), ~g[f'fit{k}_psf'].any(axis=(1, 2)))
            assert np.array_equal(np.isnan(ref).any(axis=1), np.isnan(ref).all(axis=1))


def test_golden_lobe_properties():
    g = load()
    n = int(g['nlobe'])
    assert any(bool(g[f'lobe{k}_conn_differs']) for k in range(n))
    assert any(bool(g[f'lobe{k}_second_island']) for k in range(n))
    shapes = [g[f'lobe{k}_psf'].shape for k in range(n)]
    assert (1, 37, 29) in shapes and (3, 64, 48) in shapes
    assert any(s[1] >= 2049 and s[2] == 33 for s in shapes)
    for k in range(n):
        psf = g[f'lobe{k}_psf']
        assert psf.dtype == np.float32 and np.array_equal(g[f'lobe{k}_rec32'], g[f'lobe{k}_rec64'])
        for v in range(psf.shape[0]):
            assert psf[v].any() or not g[f'lobe{k}_rec64'][v].any()
    assert any(s[0] == 3 and not g[f'lobe{k}_psf'][1].any() for k, s in enumerate(shapes))
    # a pixel exactly at the level next to the centre island, and outside it
    a, rec = g['lobe1_psf'][0], g['lobe1_rec64'][0]
    assert a[29, 24] / a.max() == float(g['lobe1_level']) and a[30, 24] / a.max() > 0.5 and rec[3] == 30 - 64 / 2


def test_golden_objective_points():
    g = load()
    for k in range(int(g['nobj'])):
        for b in (32, 64):
            pts, f, gr, gabs = (g[f'obj{k}_{name}{b}'] for name in ('pts', 'f', 'g', 'gabs'))
            assert pts.shape == (4, 3) and f.shape == (4,) and gr.shape == gabs.shape == (4, 3)
            assert np.all(np.abs(gr) <= gabs * (1 + 1e-12)) and np.all(f > 0) and int(g[f'obj{k}_n{b}']) > 0
            assert any(x[0] < x[1] for x in pts) and any(x[0] > x[1] for x in pts)
            ties = [i for i, x in enumerate(pts) if x[0] == x[1]]
            assert ties and all(gr[i, 0] == gr[i, 1] for i in ties)


@pytest.mark.parametrize('b', [32, 64])
def test_start_point_from_the_record(b):
    """misc.py:563-564, 574-578 on the stored records against the start points the reference handed to its optimiser."""
    from pfb_clean_amd.utils.beamfit import start_point, RECORD, FIELDS
    assert len(FIELDS) <= RECORD
    g = load()
    seen = 0
    for k in range(int(g['nlobe'])):
        for rec, x0 in zip(g[f'lobe{k}_rec{b}'], g[f'lobe{k}_x0_{b}']):
            if rec[1]:
                got = start_point(np.concatenate((rec, np.zeros(RECORD - rec.size))))
                assert got.dtype == np.float64 and np.array_equal(got, x0)
                seen += 1
    assert seen >= 8
