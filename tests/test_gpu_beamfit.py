"""
The clean-beam fit on the MI355X (fitcleanbeam and the three kernels under it) against the REFERENCE's stored outputs
(tests/golden/beamfit.npz, written by tests/golden/make_golden_beamfit.py from the reference's own
pfb/utils/misc.py:506-584).

Bounds:
  lobe record   every value equal to the reference's, exactly: the maximum, np.any, the extents of the centre island
                (half-integers for odd sizes), the island's and the fit region's pixel counts, extent * rsq.
  objective     |f - ref| <= 4 n 2.2e-16 sum res_i^2 and |g_k - ref_k| <= 4 n 2.2e-16 sum_i |term_ik|, n the fit-region
                count and the sums the generator's: the worst case of an n-term sum in another order, the factor 4 for
                the rounding of a term (exp's argument error is damped, a e^-a <= 1/e).  Points: the fitted point, the
                start point, one with emaj < emin and a tie emaj == emin (the half-and-half split).
  end to end    |got - ref| <= 1e-12 max(1, |ref|) + 50 spread per parameter, spread = the stored change of the
                reference's own result under a 1-ulp perturbation of the PSF and 1e-14 of every objective value and
                gradient (the form and head-room of test_gpu_comps.py).  Only stable cases are stored
                (spread <= 1e-11); a lobe with xdiff == ydiff is compared at the objective level only.
The float32 runs are compared with the reference run on the float32 array.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'beamfit.npz')
EPS = 2.2e-16
NLOBE, NFIT, NOBJ, NREC = 4, 3, 5, 12
_cache = {}


def load():
    if not _cache:
        with np.load(GOLDEN, allow_pickle=False) as z:
            _cache.update({k: z[k] for k in z.files})
    return _cache


def bits(dtype):
    return 8 * np.dtype(dtype).itemsize


def as_kind(a, kind):
    return torch.from_numpy(a).cuda() if kind == 'tensor' else a


def test_case_counts():
    g = load()
    assert (int(g['nlobe']), int(g['nfit']), int(g['nobj'])) == (NLOBE, NFIT, NOBJ)


# ------------------------------------------------------------------------------------------------ lobe record
def records(cube, level, extent):
    from pfb_clean_amd.utils import beamfit
    recs, _ = beamfit.lobe_records(cube, level, extent)
    assert recs.shape == (cube.shape[0], beamfit.RECORD) and not recs[:, NREC:].any()
    return recs[:, :NREC]


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('k', range(NLOBE))
def test_lobe_record(k, dtype):
    g = load()
    cube = torch.from_numpy(g[f'lobe{k}_psf'].astype(dtype)).cuda()
    ref = g[f'lobe{k}_rec{bits(dtype)}']
    got = records(cube, float(g[f'lobe{k}_level']), float(g[f'lobe{k}_extent']))
    print(f"lobe{k} {g['lobe_names'][k]} {tuple(cube.shape)} {np.dtype(dtype).name}:\n{got}")
    assert np.array_equal(got, ref)


@pytest.mark.parametrize('dtype,shift', [(np.float32, 1), (np.float32, 2), (np.float32, 3), (np.float64, 1)])
@pytest.mark.parametrize('k', [2, 3])
def test_lobe_record_any_base_alignment(k, dtype, shift):
    """The cube itself `shift` elements past a 16-byte boundary: every head length of the max pass's peel."""
    g = load()
    psf = g[f'lobe{k}_psf'].astype(dtype)
    flat = torch.empty(psf.size + 4, dtype=torch.from_numpy(psf).dtype, device='cuda')
    assert flat.data_ptr() % 16 == 0
    cube = flat[shift:shift + psf.size].view(psf.shape)
    cube.copy_(torch.from_numpy(psf))
    assert cube.data_ptr() % 16 == shift * psf.itemsize
    got = records(cube, float(g[f'lobe{k}_level']), float(g[f'lobe{k}_extent']))
    assert np.array_equal(got, g[f'lobe{k}_rec{bits(dtype)}'])


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_max_propagates_nan_and_any_counts_it(dtype):
    g = load()
    psf = g['lobe2_psf'].astype(dtype)
    psf[0, 1500, 7] = np.nan                      # in the vectors
    psf[1] = 0.0
    psf[1, 2048, 32] = np.nan                     # the only non-zero of the plane, in the loose tail
    psf[2, 0, 0] = -0.0
    got = records(torch.from_numpy(psf).cuda(), 0.5, 15.0)
    ref = g[f'lobe2_rec{bits(dtype)}']
    assert np.isnan(got[0, 0]) and got[0, 1] == 1 and not got[0, 2:].any()
    assert np.isnan(got[1, 0]) and got[1, 1] == 1 and not got[1, 2:].any()
    assert np.array_equal(got[2], ref[2])


# -------------------------------------------------------------------------------------------------- objective
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('k', range(NOBJ))
def test_objective(k, dtype):
    from pfb_clean_amd.utils import beamfit
    g = load()
    b, band = bits(dtype), int(g[f'obj{k}_band'])
    cube = torch.from_numpy(g[str(g[f'obj{k}_psfkey'])].astype(dtype)).cuda()
    recs, work = beamfit.lobe_records(cube)
    n = int(g[f'obj{k}_n{b}'])
    assert recs[band, beamfit.FIELDS.index('nfit')] == n
    func = beamfit.objective(cube, work, band)
    failed = []
    for x, f_ref, g_ref, gabs in zip(g[f'obj{k}_pts{b}'], g[f'obj{k}_f{b}'], g[f'obj{k}_g{b}'], g[f'obj{k}_gabs{b}']):
        f, grad = func(x)
        ferr, fbound = abs(f - f_ref), 4 * n * EPS * f_ref            # f_ref = sum res^2
        gerr, gbound = np.abs(grad - g_ref), 4 * n * EPS * gabs
        print(f'obj{k} fp{b} x = {x.tolist()}: f err {ferr:.2e} (bound {fbound:.2e}), g err {gerr.tolist()} '
              f'(bound {gbound.tolist()})')
        if not (ferr <= fbound and np.all(gerr <= gbound)):
            failed.append(x.tolist())
        if x[0] == x[1]:
            assert grad[0] == grad[1]
    assert not failed


# ------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize('kind', ['numpy', 'tensor'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('k', range(NFIT))
def test_fitcleanbeam_golden(k, dtype, kind):
    from pfb_clean_amd.utils.misc import fitcleanbeam
    g = load()
    psf = as_kind(g[f'fit{k}_psf'].astype(dtype), kind)
    keep = psf.clone() if kind == 'tensor' else psf.copy()
    res = fitcleanbeam(psf)
    assert isinstance(res, list) and all(isinstance(r, list) and len(r) == 3 for r in res)
    assert torch.equal(psf, keep) if kind == 'tensor' else np.array_equal(psf, keep)
    got, ref = np.array(res, dtype=np.float64), g[f'fit{k}_ref{bits(dtype)}']
    spread = float(g[f'fit{k}_spread{bits(dtype)}'])
    assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref))
    ok = np.isfinite(ref)
    err = np.abs(got - ref)[ok]
    bound = (1e-12 * np.maximum(1.0, np.abs(ref)) + 50 * spread)[ok]
    print(f'fit{k} {np.dtype(dtype).name} {kind}: {got.tolist()} err {err.tolist()} (bound {bound.tolist()})')
    assert np.all(err <= bound)


def test_pixsize_scales_the_axes_only():
    from pfb_clean_amd.utils.misc import fitcleanbeam
    psf = torch.from_numpy(load()['fit1_psf']).cuda()
    (a, b, pa), = fitcleanbeam(psf)
    (a2, b2, pa2), = fitcleanbeam(psf, pixsize=2.5)
    assert (a2, b2, pa2) == (a * 2.5, b * 2.5, pa)


def test_all_zero_band_gives_nans():
    from pfb_clean_amd.utils.misc import fitcleanbeam
    res = fitcleanbeam(np.zeros((2, 37, 29), dtype=np.float32))
    assert np.isnan(np.array(res)).all() and np.array(res).shape == (2, 3)


@pytest.mark.parametrize('what', ['off_centre', 'nan'])
def test_centre_not_above_level_raises(what):
    from pfb_clean_amd.utils.misc import fitcleanbeam
    psf = load()['fit0_psf'].copy()             # band 1 is all zero
    if what == 'off_centre':
        psf[2] = np.roll(psf[2], (20, 15), axis=(0, 1))
    else:
        psf[2, 3, 3] = np.nan
    with pytest.raises(ValueError, match='band 2'):
        fitcleanbeam(torch.from_numpy(psf).cuda())


def test_rejects_what_is_not_a_cube():
    from pfb_clean_amd.utils.misc import fitcleanbeam
    with pytest.raises(ValueError):
        fitcleanbeam(np.zeros((37, 29)))
    with pytest.raises(TypeError):
        fitcleanbeam(torch.zeros((1, 8, 8), dtype=torch.float16, device='cuda'))
