"""
The component model on the MI355X (fit_image_cube, eval_coeffs_to_cube, eval_coeffs_to_slice) against the REFERENCE's
stored outputs (tests/golden/comps*.npz, written by tests/golden/make_golden_comps.py from the reference's own
pfb/utils/misc.py:1084-1313).

Bounds:
  Ix, Iy        equal to the reference's, order included (np.where's row-major order), int64.
  strings       equal character for character.
  coeffs        max|coeffs - ref| / max|ref| <= 1e-12 + 50 * spread, spread = the stored change of the reference's own
                coeffs under a 1-ulp perturbation of the image (the form and head-room of test_gpu_restore.py's ratio
                branch).  The arithmetic is fp64 for both image dtypes and every stored image is exactly a float32
                array, so the fp32 and the fp64 run have the same bound.  Only stable cases are stored
                (spread <= 1e-11); full-order 'poly' at 8 or 16 bands is not compared with anything.
  eval          |got - ref| <= 16 nparam 2.2e-16 eval_scale: two nparam-term dot products (ours and the reference's)
                plus the rounding of the basis values, head-room x4; eval_scale = max sum_p |E_p c_p| (stored).
                dtype=float32 adds the final rounding 6e-8 |ref|.  Pixels off the component list are exactly 0.
  slice         the eval bound + 32 * 2.2e-16 max|ref| for the bilinear weights and their four-term sum.
  at scale      Ix, Iy equal to np.where(np.any(image, axis=(0, 1))); eval(fit) equals the cube on the components
                within atol 1e-10, the criterion of the reference's own test (test_model2comps.py:106).
  mask edges    Ix, Iy equal to np.where(np.any(cube, axis=0)) at every base offset and around every word, wave and
                workgroup edge of the mask pass.
Every input image is the stored float32 array; the fp64 runs use its upcast, as the reference run did.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIT_TAGS = [f'fit{c}' for c in range(11)] + ['edge_zero', 'edge_full', 'edge_mixed']
EVAL_OF = [0, 2, 7, 9]
EPS = 2.2e-16
_cache = {}


def load(name):
    if name not in _cache:
        with np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False) as z:
            _cache[name] = {k: z[k] for k in z.files}
    return _cache[name]


def fit_args(g, tag):
    nbt, nbf = (None if v < 0 else int(v) for v in g[tag + '_nbasis'])
    return (g[tag + '_time'], g[tag + '_freq']), (g.get(tag + '_wgt'), nbt, nbf, str(g[tag + '_method']),
                                                   float(g[tag + '_sigmasq']))


def model_of(g, tag):
    """(coeffs, Ix, Iy, expr, params, texpr, fexpr) as the reference returned them."""
    expr, texpr, fexpr = (str(s) for s in g[tag + '_strings'])
    return g[tag + '_coeffs'], g[tag + '_Ix'], g[tag + '_Iy'], expr, [str(p) for p in g[tag + '_params']], texpr, fexpr


def as_kind(a, kind):
    return torch.from_numpy(a).cuda() if kind == 'tensor' else a


def to_np(a, kind):
    if kind == 'tensor':
        assert isinstance(a, torch.Tensor) and a.is_cuda
        return a.cpu().numpy()
    assert isinstance(a, np.ndarray)
    return a


# ------------------------------------------------------------------------------------------------- fit
def test_fit_case_count():
    assert int(load('comps_fit')['nfit']) == 11 and load('comps_eval')['eval_of'].tolist() == EVAL_OF


@pytest.mark.parametrize('kind', ['numpy', 'tensor'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('tag', FIT_TAGS + ['sfit0', 'sfit1'])
def test_fit_golden(tag, dtype, kind):
    from pfb_clean_amd.utils.misc import fit_image_cube
    g = load('comps_slice' if tag.startswith('sfit') else 'comps_fit')
    (time, freq), rest = fit_args(g, tag)
    image = as_kind(g[tag + '_image'].astype(dtype), kind)
    coeffs, Ix, Iy, expr, params, texpr, fexpr = fit_image_cube(time, freq, image, *rest)
    coeffs, Ix, Iy = to_np(coeffs, kind), to_np(Ix, kind), to_np(Iy, kind)
    ref, rIx, rIy, rexpr, rparams, rtexpr, rfexpr = model_of(g, tag)
    assert Ix.dtype == np.int64 and Iy.dtype == np.int64
    assert np.array_equal(Ix, rIx) and np.array_equal(Iy, rIy)
    assert (expr, params, texpr, fexpr) == (rexpr, rparams, rtexpr, rfexpr)
    assert all(isinstance(s, str) for s in [expr, texpr, fexpr] + params) and isinstance(params, list)
    assert coeffs.dtype == np.float64 and coeffs.shape == ref.shape
    assert np.array_equal(np.isnan(coeffs), np.isnan(ref))
    ok = np.isfinite(ref)
    if ok.any():
        spread = float(g[tag + '_spread'])
        err = np.abs(coeffs - ref)[ok].max() / np.abs(ref[ok]).max()
        print(f'{tag} {np.dtype(dtype).name} {kind}: ncomps {Ix.size} rel err {err:.2e} (spread {spread:.2e})')
        assert err <= 1e-12 + 50 * spread


def scale_cube(rng, dtype, shape):
    """~5000 random pixels, one dense 64 x 64 block, the first and the last pixel."""
    ntime, nband, nx, ny = shape
    img = np.zeros(shape, dtype=dtype)
    n = 5000
    px, py = rng.integers(0, nx, n), rng.integers(0, ny, n)
    img[:, :, px, py] = rng.standard_normal((ntime, nband, n))
    img[:, :, 100:164, 90:154] = 1.0 + rng.random((ntime, nband, 64, 64))
    img[:, :, 0, 0] = 1.5
    img[:, -1, -1, -1] = -2.5
    return img


# odd npix (no plane but the first is 16-byte aligned: the peel kernel) and npix a multiple of 16 bytes that is no
# multiple of 64 pixels (the aligned kernel, a partial last word); the fp32 shapes have more workgroups (258 / 259 of
# 4096 pixels) than one tile of the scan (256), so that its carry is exercised
@pytest.mark.parametrize('dtype,shape', [(np.float32, (1, 3, 1031, 1025)), (np.float64, (1, 2, 257, 193)),
                                         (np.float32, (1, 3, 1030, 1026)), (np.float64, (1, 2, 258, 194))])
def test_compaction_at_scale(dtype, shape):
    from pfb_clean_amd.utils.misc import fit_image_cube, eval_coeffs_to_cube
    rng = np.random.default_rng(420)
    img = scale_cube(rng, dtype, shape)
    ntime, nband, nx, ny = shape
    time, freq = np.array([3600.0]), np.linspace(0.9e9, 1.7e9, nband)
    wIx, wIy = np.where(np.any(img, axis=(0, 1)))
    imd = torch.from_numpy(img).cuda()
    coeffs, Ix, Iy, expr, params, texpr, fexpr = fit_image_cube(time, freq, imd, nbasisf=nband, method='Legendre')
    assert Ix.dtype == torch.int64 and Iy.dtype == torch.int64 and coeffs.dtype == torch.float64
    assert np.array_equal(Ix.cpu().numpy(), wIx) and np.array_equal(Iy.cpu().numpy(), wIy)
    assert coeffs.shape == (nband, wIx.size)
    cube = eval_coeffs_to_cube(time, freq, nx, ny, coeffs, Ix, Iy, expr, params, texpr, fexpr)
    assert cube.dtype == torch.float64 and cube.shape == shape
    diff = (cube - imd.double()).abs().max().item()
    print(f'{shape} {np.dtype(dtype).name}: ncomps {wIx.size}, max |eval(fit) - cube| {diff:.2e}')
    assert diff <= 1e-10


def edge_pixels(npix, V):
    """Flat indices of the first and the last pixel, both sides of the 64-pixel (mask word) boundaries near the start
    and near the end, and the first V - 1 pixels of wave iterations (64 V pixels each; the pixels lane 0 reads singly
    when a plane is off the 16-byte grid) at the start, around a wave's share (1024 px), around a workgroup (4096 px)
    and at the end."""
    q = {0, npix - 1}
    nb = (npix - 1) // 64
    for b in (1, 2, 3, nb - 2, nb - 1, nb):
        q |= {64 * b - 1, 64 * b}
    span = 64 * V
    its = {0, 1, 2, (npix - 1) // span - 1, (npix - 1) // span}
    for edge in (1024 // span, 4096 // span):
        its |= {edge - 1, edge, edge + 1}
    for s in its:
        q |= {span * s + j for j in range(V - 1)}
    return np.array(sorted(p for p in q if 0 <= p < npix))


def device_where(cube, a):
    """Ix, Iy of the device route (mask, scan, count read, compaction) on a copy of the (nplane, nx, ny) cube that
    starts `a` elements past a 16-byte boundary."""
    from pfb_clean_amd.utils.comps import _components
    nplane, nx, ny = cube.shape
    buf = torch.zeros(cube.size + 8, dtype=torch.from_numpy(cube).dtype, device='cuda')
    buf[a:a + cube.size] = torch.from_numpy(cube).cuda().reshape(-1)
    dev = buf[a:a + cube.size].view(nplane, nx * ny)
    assert dev.is_contiguous() and dev.data_ptr() % 16 == a * cube.itemsize
    Ix, Iy = _components(dev, nx, ny)
    assert Ix.dtype == torch.int64 and Iy.dtype == torch.int64
    return Ix.cpu().numpy(), Iy.cpu().numpy()


# On either side of a word (64 px), a wave's share (1024 px) and a workgroup (4096 px); every value of npix % V, a
# vector straddling npix included.  With 3 planes and npix % V != 0 every plane has a head of its own.
@pytest.mark.parametrize('shape', [(1, 1), (1, 3), (7, 9), (8, 8), (5, 13), (63, 65), (64, 64), (17, 241), (3, 2731)])
@pytest.mark.parametrize('dtype,a', [(np.float32, 0), (np.float32, 1), (np.float32, 2), (np.float32, 3),
                                     (np.float64, 0), (np.float64, 1)])
def test_mask_edges(dtype, a, shape):
    """Ix, Iy equal np.where(np.any(cube, axis=0)) with every edge pixel set in exactly one plane, every plane in
    turn, so that each plane's head is the only witness; a NaN counts, -0.0 does not."""
    nx, ny = shape
    npix, V = nx * ny, 16 // np.dtype(dtype).itemsize
    q = edge_pixels(npix, V)
    assert q[0] == 0 and q[-1] == npix - 1

    def check(cube, what):
        wIx, wIy = np.where(np.any(cube, axis=0))
        Ix, Iy = device_where(cube, a)
        assert np.array_equal(Ix, wIx) and np.array_equal(Iy, wIy), (what, shape, a)
        return Ix.size

    for value in (1.5, np.nan):
        for turn in range(3):
            cube = np.zeros((3, npix), dtype=dtype)
            cube[(np.arange(q.size) + turn) % 3, q] = value
            assert check(cube.reshape(3, nx, ny), f'{value} turn {turn}') == q.size
    cube = np.zeros((3, npix), dtype=dtype)
    cube[np.arange(q.size) % 3, q] = -0.0
    assert np.signbit(cube).sum() == q.size and check(cube.reshape(3, nx, ny), '-0.0') == 0
    assert check(np.zeros((3, nx, ny), dtype=dtype), 'zeros') == 0
    assert check(np.ones((3, nx, ny), dtype=dtype), 'ones') == npix


# ------------------------------------------------------------------------------------------------ eval
@pytest.mark.parametrize('kind', ['numpy', 'tensor'])
@pytest.mark.parametrize('dtype', [None, np.float32])
@pytest.mark.parametrize('which', ['fitted', 'other'])
@pytest.mark.parametrize('c', EVAL_OF)
def test_eval_golden(c, which, dtype, kind):
    from pfb_clean_amd.utils.misc import eval_coeffs_to_cube
    gf, ge = load('comps_fit'), load('comps_eval')
    tag = f'fit{c}'
    coeffs, Ix, Iy, expr, params, texpr, fexpr = model_of(gf, tag)
    time, freq = gf[tag + '_time'], ge[f'eval{c}_{which}_freq']
    ref = ge[f'eval{c}_{which}']
    nx, ny = ref.shape[2:]
    kw = {} if dtype is None else {'dtype': dtype}
    got = eval_coeffs_to_cube(time, freq, nx, ny, as_kind(coeffs, kind), as_kind(Ix, kind), as_kind(Iy, kind), expr,
                              params, texpr, fexpr, **kw)
    got = to_np(got, kind)
    assert got.shape == ref.shape and got.dtype == (np.float64 if dtype is None else dtype)
    bound = 16 * coeffs.shape[0] * EPS * float(ge[f'eval{c}_{which}_scale'])
    err = np.abs(got - ref)
    print(f'eval fit{c} {which} {got.dtype} {kind}: max err {err.max():.2e} (bound {bound:.2e})')
    assert np.all(err <= bound + (6e-8 * np.abs(ref) if dtype is not None else 0.0))
    off = np.ones((nx, ny), dtype=bool)
    off[Ix, Iy] = False
    assert np.all(got[:, :, off] == 0)


def test_eval_torch_dtype_and_empty_model():
    from pfb_clean_amd.utils.misc import eval_coeffs_to_cube
    g = load('comps_fit')
    coeffs, Ix, Iy, expr, params, texpr, fexpr = model_of(g, 'edge_zero')
    time, freq = g['edge_zero_time'], g['edge_zero_freq']
    got = eval_coeffs_to_cube(time, freq, 9, 7, torch.from_numpy(coeffs).cuda(), torch.from_numpy(Ix).cuda(),
                              torch.from_numpy(Iy).cuda(), expr, params, texpr, fexpr, dtype=torch.float32)
    assert got.dtype == torch.float32 and got.shape == (1, 4, 9, 7) and not got.any().item()


# ----------------------------------------------------------------------------------------------- slice
def slice_call(g, s, k, kind, **kw):
    from pfb_clean_amd.utils.misc import eval_coeffs_to_slice
    tag = f'sfit{s}'
    coeffs, Ix, Iy, expr, params, texpr, fexpr = model_of(g, tag)
    nxi, nyi = (int(v) for v in g['fits'][s])
    nxo, nyo, ratio, sx, sy = g['cases'][k]
    cell, band = float(g['cell']), int(g[tag + '_band'])
    got = eval_coeffs_to_slice(g[tag + '_time'][0], g[tag + '_freq'][band], as_kind(coeffs, kind), as_kind(Ix, kind),
                               as_kind(Iy, kind), expr, params, texpr, fexpr, nxi, nyi, cell, cell, 0.0, 0.0,
                               int(nxo), int(nyo), ratio * cell, ratio * cell, sx * cell, sy * cell, **kw)
    return to_np(got, kind)


@pytest.mark.parametrize('kind', ['numpy', 'tensor'])
@pytest.mark.parametrize('k', range(5))
@pytest.mark.parametrize('s', range(2))
def test_slice_golden(s, k, kind):
    g = load('comps_slice')
    ref = g[f'slice{s}_{k}']
    nparam = g[f'sfit{s}_coeffs'].shape[0]
    bound = 16 * nparam * EPS * float(g[f'sfit{s}_slice_scale']) + 32 * EPS * np.abs(ref).max()
    got = slice_call(g, s, k, kind)
    assert got.shape == ref.shape and got.dtype == np.float64
    err = np.abs(got - ref).max()
    print(f'slice fit {s} case {k} {kind}: max err {err:.2e} (bound {bound:.2e})')
    assert err <= bound
    got32 = slice_call(g, s, k, kind, dtype=np.float32)
    assert got32.shape == ref.shape and got32.dtype == np.float32
    assert np.all(np.abs(got32 - ref) <= bound + 6e-8 * np.abs(ref))


@pytest.mark.parametrize('k', range(3))
@pytest.mark.parametrize('s', range(2))
def test_slice_integer_shift(s, k):
    """test_model2comps.py:111-134: with equal cells and a centre shifted by whole pixels the pixel centres coincide,
    so the output is the input model, shifted and zero outside it."""
    g = load('comps_slice')
    nxo, nyo, ratio, sx, sy = g['cases'][k]
    assert ratio == 1.0 and sx == int(sx) and sy == int(sy)
    tag = f'sfit{s}'
    model = g[tag + '_image'][0, int(g[tag + '_band'])].astype(np.float64)
    nxi, nyi = model.shape
    nxo, nyo = int(nxo), int(nyo)
    # output pixel i sits at input index i - nxo//2 + sx + nxi//2
    ii = np.arange(nxo) - nxo // 2 + int(sx) + nxi // 2
    jj = np.arange(nyo) - nyo // 2 + int(sy) + nyi // 2
    inx, iny = (ii >= 0) & (ii < nxi), (jj >= 0) & (jj < nyi)
    expect = np.zeros((nxo, nyo))
    expect[np.ix_(inx, iny)] = model[np.ix_(ii[inx], jj[iny])]
    got = slice_call(g, s, k, 'numpy')
    np.testing.assert_allclose(1.0 + got, 1.0 + expect, rtol=1e-7)


# ---------------------------------------------------------------------------------------------- limits
@pytest.mark.parametrize('nband,nbasisf', [(65, 2), (40, 33)])
def test_fit_limits(nband, nbasisf):
    from pfb_clean_amd import _lib
    from pfb_clean_amd.utils.misc import fit_image_cube
    img = torch.ones((1, nband, 4, 4), dtype=torch.float64, device='cuda')
    with pytest.raises(_lib.PfbHipError) as e:
        fit_image_cube(np.array([3600.0]), np.linspace(0.9e9, 1.7e9, nband), img, nbasisf=nbasisf, method='Legendre')
    assert e.value.code == _lib.PFB_ERR_UNSUPPORTED


def test_fit_at_the_limits():
    """nrow = 64 and nparam = 32, the largest supported system: the residual of the normal equations."""
    from pfb_clean_amd.utils.misc import fit_image_cube
    from pfb_clean_amd.utils.comps import fit_design
    rng = np.random.default_rng(420)
    time, freq = np.array([3600.0]), np.linspace(0.9e9, 1.7e9, 64)
    img = np.zeros((1, 64, 12, 11))
    img[:, :, rng.integers(0, 12, 40), rng.integers(0, 11, 40)] = rng.standard_normal((1, 64, 40))
    coeffs, Ix, Iy = fit_image_cube(time, freq, img, nbasisf=32, method='Legendre')[:3]
    X = fit_design(time, freq, None, 32, 'Legendre')[0]
    beta = img[0][:, Ix, Iy]
    ref = np.linalg.solve(X.T @ X, X.T @ beta)
    assert coeffs.shape == ref.shape == (32, Ix.size)
    # cond(X^T X) of 32 Legendre polynomials on 64 equispaced points is 1.5e4, so two backward-stable solves differ
    # by a small multiple of cond * eps = 3e-12; 1e-10 leaves a factor of 30
    assert np.abs(coeffs - ref).max() <= 1e-10 * np.abs(ref).max()
