"""
Restoring-beam convolution and restore_image on the MI355X against the REFERENCE's stored outputs
(tests/golden/restore*.npz, written by tests/golden/make_golden_restore.py from the reference's own
pfb/utils/misc.py:109-238 and pfb/utils/restoration.py:6-57).

Bounds, all relative to max|ref|:
  Gaussian2D     1e-14.  A value e^{-t} whose t carries k ~ 5 roundings has absolute error <= k eps t e^{-t} <=
                 k eps / e ~ 4e-16 of the peak, plus 1-2 ulp of exp; 1e-14 leaves > 10x over that.  On integer (and
                 half-integer) coordinates the truncation test is exact, so the zero pattern must match exactly.
  model branch   the project's convolution tolerances: fp64 1e-12, fp32 1e-5.
  ratio branch   fp64 1e-12 + 50 * spread, spread = the stored change of the reference's own output under a 1-ulp
                 perturbation of its kernel transforms' inputs (a different FFT factorisation differs from pocketfft
                 by O(log2 N) ~ 8-9 roundings per axis, two axes, head-room x3); fp32 images 1e-5 (kernels and ratio
                 are fp64 and only cast at the end).  Only stable cases are stored (spread <= 1e-11); the
                 ill-conditioned regime (initial FWHM >= 3 pixels) is not compared against anything.
Every input image is the stored float32 array; the fp64 runs use its upcast, as the reference run did.
"""
import os

import numpy as np
import pytest
import scipy.fft as sfft
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
NCONV = 5
NGAUSS = 25
TOL = {np.float64: 1e-12, np.float32: 1e-5}
_cache = {}


def load(name):
    if name not in _cache:
        with np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False) as z:
            _cache[name] = {k: z[k] for k in z.files}
    return _cache[name]


def coords(nx, ny, cell=1.0):
    x = np.arange(-nx / 2, nx / 2) * cell
    y = np.arange(-ny / 2, ny / 2) * cell
    return np.meshgrid(x, y, indexing='ij')


def relerr(got, ref):
    return np.abs(np.asarray(got, dtype=np.float64) - ref).max() / np.abs(ref).max()


def last_plan():
    """The convolution plan of the most recent convolve2gaussres / restore_image kernel build."""
    from pfb_clean_amd.utils import misc
    return next(reversed(misc._beam_cache._entries.values()))[0].plan


@pytest.fixture(autouse=True)
def _fresh_cache():
    from pfb_clean_amd.utils import misc
    misc.clear_beam_cache()
    yield
    misc.clear_beam_cache()


# ------------------------------------------------------------------------------------------- Gaussian2D
def test_gauss_case_count():
    assert len(load('restore')['gauss_cases']) == NGAUSS


@pytest.mark.parametrize('c', range(NGAUSS))
def test_gaussian2d(c):
    from pfb_clean_amd.utils.misc import Gaussian2D
    g = load('restore')
    nx, ny, emaj, emin, pa, norm, nsigma, cell = g['gauss_cases'][c]
    xx, yy = coords(int(nx), int(ny), cell)
    ref = g[f'gauss{c}']
    got = Gaussian2D(xx, yy, (emaj * cell, emin * cell, pa), normalise=bool(norm), nsigma=int(nsigma))
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == xx.shape
    err = relerr(got, ref)
    print(f'Gaussian2D case {c}: rel err {err:.2e}')
    assert err <= 1e-14
    if cell == 1.0:
        assert np.array_equal(got == 0, ref == 0)


def test_gaussian2d_defaults_and_tensors():
    from pfb_clean_amd.utils.misc import Gaussian2D
    g = load('restore')
    c = 0
    nx, ny, emaj, emin, pa, norm, nsigma, cell = g['gauss_cases'][c]
    assert (norm, nsigma) == (1, 5)                       # the defaults
    xx, yy = coords(int(nx), int(ny))
    got = Gaussian2D(torch.from_numpy(xx).cuda(), torch.from_numpy(yy).cuda(), (emaj, emin, pa))
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float64
    assert relerr(got.cpu().numpy(), g[f'gauss{c}']) <= 1e-14
    # float32 coordinates: still an fp64 result
    got = Gaussian2D(xx.astype(np.float32), yy.astype(np.float32), (emaj, emin, pa))
    assert got.dtype == np.float64 and relerr(got, g[f'gauss{c}']) <= 1e-14


# ------------------------------------------------------------------------------------ convolve2gaussres
def model_variants(g):
    img = g['image']
    nb, nx, ny = img.shape
    out = [('model', img, {})]
    if 'model_norm' in g:
        pt = np.zeros_like(img)
        pt[:, nx // 2, ny // 2] = 1.0
        out += [('model_norm', img, dict(norm_kernel=True)), ('model_pfrac25', img, dict(pfrac=0.25)),
                ('model_point', pt, {})]
    return out


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('c', range(NCONV))
def test_model_branch(c, dtype):
    from pfb_clean_amd.utils.misc import convolve2gaussres
    g = load(f'restore_conv{c}')
    nb, nx, ny = g['image'].shape
    xx, yy = coords(nx, ny)
    par = tuple(g['model_par'])
    variants = model_variants(g)
    assert len(variants) == (4 if c >= 3 else 1)
    for key, img, kw in variants:
        x = img.astype(dtype)
        keep = x.copy()
        got = convolve2gaussres(x, xx, yy, par, 1, **kw)
        assert isinstance(got, np.ndarray) and got.dtype == dtype and got.shape == x.shape
        assert np.array_equal(x, keep), "image was modified"
        err = relerr(got, g[key])
        print(f'model branch conv{c} {key} {np.dtype(dtype).name}: rel err {err:.2e} fast_path={last_plan().fast_path}')
        assert err <= TOL[dtype], key
        assert last_plan().fast_path, "the gathered kernel must feed the register-FFT kernels"


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('c', range(NCONV))
def test_ratio_branch(c, dtype):
    from pfb_clean_amd.utils.misc import convolve2gaussres
    g = load(f'restore_conv{c}')
    nb, nx, ny = g['image'].shape
    xx, yy = coords(nx, ny)
    tags = list(g['ratio_tags'])
    assert len(tags) == (4 if c >= 3 else 2)
    for tag in tags:
        pars, spread, ref = g[tag + '_par'], float(g[tag + '_spread']), g[tag]
        assert spread <= 1e-11
        x = g['image'].astype(dtype)
        keep = x.copy()
        got = convolve2gaussres(x, xx, yy, tuple(pars[0]), 1, gausspari=[tuple(p) for p in pars[1:]], norm_kernel=True)
        assert got.dtype == dtype and np.array_equal(x, keep)
        err = relerr(got, ref)
        bound = 1e-12 + 50 * spread if dtype == np.float64 else 1e-5
        print(f'ratio branch conv{c} {tag} {np.dtype(dtype).name}: rel err {err:.2e} bound {bound:.2e} spread {spread:.2e}')
        assert err <= bound, tag


def np_gauss(xx, yy, par):
    emaj, emin, pa = par
    t = np.deg2rad(-pa)
    R = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
    A = R.T @ np.diag([1.0 / emin ** 2, 1.0 / emaj ** 2]) @ R
    q = A[0, 0] * xx * xx + 2 * A[0, 1] * xx * yy + A[1, 1] * yy * yy
    return np.where(xx ** 2 + yy ** 2 <= (5 * emaj) ** 2, np.exp(-2 * np.sqrt(2 * np.log(2)) * q), 0.0)


def topleft_reference(img, xx, yy, par, pfrac=0.5):
    """The reference statement in its top-left form (tests/test_cpu_restore.py checks it against the reference's
    outputs): circular convolution on the reference's own (P, Q) grid with the centred-padded kernel."""
    from pfb_clean_amd.utils.misc import get_padding_info
    nb, nx, ny = img.shape
    pad = get_padding_info(nx, ny, pfrac)[0]
    P, Q = nx + sum(pad[1]), ny + sum(pad[2])
    khat = sfft.rfft2(np.fft.ifftshift(np.pad(np_gauss(xx, yy, par), (pad[1], pad[2]))), workers=16)
    out = np.empty(img.shape)
    for b in range(nb):
        xp = np.zeros((P, Q))
        xp[:nx, :ny] = img[b]
        out[b] = sfft.irfft2(sfft.rfft2(xp, workers=16) * khat, s=(P, Q), workers=16)[:nx, :ny]
    return out


@pytest.mark.parametrize('nband,n,dtype', [(2, 2048, np.float32), (1, 1500, np.float64)])
def test_model_branch_large(nband, n, dtype):
    """Sizes the fixtures cannot hold: 2048^2 x 2 fp32 (reference grid 3072^2) and 1500^2 fp64 (reference grid 2250^2),
    both on the 4096^2 engine grid, device tensors in and out."""
    from pfb_clean_amd.utils.misc import convolve2gaussres
    rng = np.random.default_rng(420)
    img = rng.standard_normal((nband, n, n)).astype(np.float32)
    xx, yy = coords(n, n)
    par = (40.0, 24.0, 33.0)
    ref = topleft_reference(img.astype(np.float64), xx, yy, par)
    x = torch.from_numpy(img.astype(dtype)).cuda()
    got = convolve2gaussres(x, torch.from_numpy(xx).cuda(), torch.from_numpy(yy).cuda(), par, 1)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == x.dtype
    plan = last_plan()
    assert plan.fast_path and (plan.nx_psf, plan.lastsize) == (4096, 4096)
    err = relerr(got.cpu().numpy(), ref)
    print(f'model branch {nband}x{n}x{n} {np.dtype(dtype).name}: rel err {err:.2e}')
    assert err <= TOL[dtype]


# ----------------------------------------------------------------------------------------- restore_image
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('conv', [True, False])
def test_restore_image(conv, dtype):
    from pfb_clean_amd.utils.restoration import restore_image
    g = load('restore_image')
    gpf, gpi = [tuple(p) for p in g['gaussparf']], [tuple(p) for p in g['gausspari']]
    spread = float(g['spread'])
    assert spread <= 1e-11
    ref = g['image_conv' if conv else 'image_noconv']
    bound = (1e-12 + 50 * spread) if dtype == np.float64 else 1e-5
    # numpy in -> numpy out
    model, resid = g['model'].astype(dtype), g['residual'].astype(dtype)
    rkeep = resid.copy()
    out = restore_image(model, resid, 1.0, 1.0, gpf, gpi, conv, 1, 0.5)
    assert isinstance(out, np.ndarray) and out.dtype == dtype and out is not model and out is not resid
    e_img, e_mod = relerr(out, ref), relerr(model, g['model_mutated'])
    print(f'restore_image conv={conv} {np.dtype(dtype).name}: image rel err {e_img:.2e}, mutated model {e_mod:.2e}, '
          f'bound {bound:.2e}')
    assert e_img <= bound
    assert e_mod <= TOL[dtype], "model must hold its convolved self"
    assert np.array_equal(resid, rkeep), "residual must not be modified"
    # tensors in -> device tensor out, same numbers
    mt, rt = torch.from_numpy(g['model'].astype(dtype)).cuda(), torch.from_numpy(resid).cuda()
    ot = restore_image(mt, rt, 1.0, 1.0, gpf, gpi, conv, 1, 0.5)
    assert isinstance(ot, torch.Tensor) and ot.is_cuda and ot.data_ptr() not in (mt.data_ptr(), rt.data_ptr())
    assert np.array_equal(ot.cpu().numpy(), out) and np.array_equal(mt.cpu().numpy(), model)
    assert np.array_equal(rt.cpu().numpy(), rkeep)


def test_restore_image_errors():
    from pfb_clean_amd.utils.restoration import restore_image
    gp = [(8., 6., 20.)] * 2
    gi = [(2., 2., 0.)] * 2
    sq = np.zeros((2, 64, 64))
    with pytest.raises(ValueError, match=r'\(2, 64, 48\)'):
        restore_image(np.zeros((2, 64, 48)), np.zeros((2, 64, 48)), 1.0, 1.0, gp, gi, True, 1, 0.5)
    with pytest.raises(AssertionError):
        restore_image(sq.copy(), sq.copy(), 1.0, 1.0, gp[:1], gi, True, 1, 0.5)
    with pytest.raises(AssertionError):
        restore_image(sq.copy(), sq.copy(), 1.0, 1.0, gp, gi + gi, True, 1, 0.5)
    with pytest.raises(AssertionError):
        restore_image(sq.copy(), np.zeros((2, 64, 32)), 1.0, 1.0, gp, gi, True, 1, 0.5)
    with pytest.raises(AssertionError):
        restore_image(sq[0].copy(), sq[0].copy(), 1.0, 1.0, gp, gi, True, 1, 0.5)


# ---------------------------------------------------------------------------------------------- contract
def test_tensor_in_tensor_out_and_plan_reuse(monkeypatch):
    from pfb_clean_amd.utils import misc
    from pfb_clean_amd.operators.psf import PsfConvPlan
    built = []
    init = PsfConvPlan.__init__

    def counting(self, *a, **kw):
        built.append(1)
        return init(self, *a, **kw)
    monkeypatch.setattr(PsfConvPlan, '__init__', counting)

    g = load('restore_conv3')
    nb, nx, ny = g['image'].shape
    xx, yy = coords(nx, ny)
    par = tuple(g['model_par'])
    x = torch.from_numpy(g['image'].astype(np.float64)).cuda()
    keep = x.clone()
    got = misc.convolve2gaussres(x, xx, yy, par, 1)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.data_ptr() != x.data_ptr()
    assert torch.equal(x, keep)
    assert relerr(got.cpu().numpy(), g['model']) <= 1e-12
    assert len(built) == 1
    # same beam, another cube, coordinates rebuilt by the caller: the kernel is not built again
    xx2, yy2 = coords(nx, ny)
    again = misc.convolve2gaussres(2 * x, xx2, yy2, par, 1)
    assert len(built) == 1
    assert relerr(again.cpu().numpy(), 2 * g['model']) <= 1e-12
    # another beam, dtype, padding or normalisation is another kernel
    misc.convolve2gaussres(x, xx, yy, (par[0], par[1], par[2] + 1), 1)
    assert len(built) == 2
    misc.convolve2gaussres(x.float(), xx, yy, par, 1)
    assert len(built) == 3
    misc.convolve2gaussres(x, xx, yy, par, 1, pfrac=0.25)
    assert len(built) == 4
    misc.convolve2gaussres(x, xx, yy, par, 1, norm_kernel=True)
    assert len(built) == 5
    # scaled coordinates are other coordinates
    misc.convolve2gaussres(x, 2 * xx, 2 * yy, par, 1)
    assert len(built) == 6


def test_restore_image_reuses_its_plans(monkeypatch):
    from pfb_clean_amd.utils.restoration import restore_image
    from pfb_clean_amd.operators.psf import PsfConvPlan
    built = []
    init = PsfConvPlan.__init__

    def counting(self, *a, **kw):
        built.append(1)
        return init(self, *a, **kw)
    monkeypatch.setattr(PsfConvPlan, '__init__', counting)
    g = load('restore_image')
    gpf, gpi = [tuple(p) for p in g['gaussparf']], [tuple(p) for p in g['gausspari']]
    outs, counts = [], []
    for _ in range(2):
        m = torch.from_numpy(g['model'].astype(np.float64)).cuda()
        r = torch.from_numpy(g['residual'].astype(np.float64)).cuda()
        outs.append(restore_image(m, r, 1.0, 1.0, gpf, gpi, True, 1, 0.5))
        counts.append(len(built))
    assert counts[0] >= 2, "one plan for the nband model kernels, one for the residual ratios"
    assert counts[1] == counts[0], "the second cube must reuse both plans"
    assert torch.equal(outs[0], outs[1])


def test_c_abi_rejects_bad_geometry():
    """The gather kernels index the coordinate arrays and the source grid from these numbers: inconsistent ones are
    refused on the host."""
    from pfb_clean_amd import _lib, _dev
    lib = _lib.load()
    d = torch.zeros(64 * 64, dtype=torch.float64, device='cuda')
    pars = torch.zeros(4, dtype=torch.float64, device='cuda')
    out = torch.zeros(128 * 128, dtype=torch.float64, device='cuda')
    p = _dev.ptr
    st = _dev.stream()
    # output grid too small for the offsets of a 64 x 64 image
    assert lib.pfb_gauss_kernel_grid(1, p(d), p(d), 64, 64, 16, 16, 96, 96, p(pars), None, 1, 1, 126, 128, p(out), st) \
        == _lib.PFB_ERR_INVALID
    # padding that puts the image outside the padded grid
    assert lib.pfb_gauss_kernel_grid(1, p(d), p(d), 64, 64, 40, 16, 96, 96, p(pars), None, 1, 1, 128, 128, p(out), st) \
        == _lib.PFB_ERR_INVALID
    # unclipped output must be the padded grid itself
    assert lib.pfb_gauss_kernel_grid(1, p(d), p(d), 64, 64, 16, 16, 96, 96, p(pars), None, 1, 0, 128, 128, p(out), st) \
        == _lib.PFB_ERR_INVALID
    assert lib.pfb_kernel_gather(1, p(d), 1, 64, 64, 64, 64, 64, 0, 128, 128, p(out), st) == _lib.PFB_ERR_INVALID
    assert lib.pfb_kernhat_ratio(None, p(d), 1, 16, p(out), st) == _lib.PFB_ERR_INVALID
