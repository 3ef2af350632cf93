"""
Major-cycle statistics, mop mask and masked problem on the MI355X (pfb_clean_amd/utils/cycle.py over csrc/cycle.hip)
against numpy / scipy.ndimage results stored in tests/golden/cycle.npz (tests/golden/make_golden_cycle.py).

Bounds:
  band sum     residual_mfs and np.sum(alpha, 0) equal numpy's bit for bit (same dtype, same band order).
  statistics   ref64 = np.std of the exact band sum cast to float64 over the n selected pixels, m their mean:
               |rms - ref64| <= 4 n 2.2e-16 (|m| + ref64), the worst case of an n-term moment sum in another order (the
               form of the beamfit tests).  float32 also against numpy's own float32 np.std:
               (log2 n + 4) 6e-8 (|m| + ref64), numpy's pairwise float32 sums.  rmax exact.
  rms_comps    float64 numpy on the coefficients the device holds, rounded to the dtype; within one ulp of the dtype
               (np.spacing of the expected value).
  closing      equal to the stored scipy result for dirosion 0, 1, 2, 3.
  masked       b, x0, beam_eff array_equal to numpy's products.
Launch geometry the shapes are chosen for (csrc/cycle.hip): the statistics pass runs up to 1024 workgroups of 256 threads
per set, one 16-byte pack (4 float32 / 2 float64; one element on the unaligned path) per thread and trip; the closing
works on output tiles of 32 rows x 64 columns.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'cycle.npz')
EPS64, EPS32 = 2.2e-16, 6e-8
NSTAT = 4
CLOSE_SHAPES = [(1, 1), (1, 9), (9, 1), (7, 5), (64, 64), (65, 129), (130, 70)]
DTYPES = [np.float32, np.float64]
_cache = {}


def load():
    if not _cache:
        with np.load(GOLDEN, allow_pickle=False) as z:
            _cache.update({k: z[k] for k in z.files})
    return _cache


def bits(dtype):
    return 8 * np.dtype(dtype).itemsize


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stat_input(k, dtype):
    """(residual, model, stored band sum) of statistics case k in `dtype`; float64 is x32 / 3 as the generator defines."""
    g = load()
    x32 = g[f'st{k}_x32']
    x = x32 if dtype == np.float32 else x32.astype(np.float64) / 3.0
    return x, g[f'st{k}_model'].astype(dtype), g[f'st{k}_mfs{bits(dtype)}']


def check_stats(tag, mfs, quiet, rms, rmax, np_std=None):
    """rms / rmax against the exact band sum `mfs` (numpy, the cube's dtype) over the bool selection `quiet` (None: all)."""
    assert isinstance(rms, float) and isinstance(rmax, float)
    sel = (mfs if quiet is None else mfs[quiet]).astype(np.float64).ravel()
    n = sel.size
    assert rmax == float(np.abs(mfs).max()), (tag, rmax)
    if n == 0:
        assert np.isnan(rms), (tag, rms)
        return
    ref64, m = float(np.std(sel)), float(sel.mean())
    err, bound = abs(rms - ref64), 4 * n * EPS64 * (abs(m) + ref64)
    print(f'{tag}: n {n} rms {rms!r} ref64 {ref64!r} err {err:.2e} (bound {bound:.2e})')
    assert err <= bound, (tag, err, bound)
    if np_std is not None:
        err32, bound32 = abs(rms - float(np_std)), (np.log2(n) + 4) * EPS32 * (abs(m) + ref64)
        print(f'{tag}: against numpy float32 std {float(np_std)!r}: err {err32:.2e} (bound {bound32:.2e})')
        assert err32 <= bound32, (tag, err32, bound32)


# ------------------------------------------------------------------------------------- band sum and statistics
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('k', range(NSTAT))
def test_residual_stats_golden(k, dtype):
    """(1,1,1); (3,5,7) and (2,33,65): odd planes, unaligned in float32; (8,96,130): 16-byte packs, several workgroups."""
    from pfb_clean_amd.utils import cycle
    g = load()
    x, model, ref = stat_input(k, dtype)
    keep = x.copy()
    mfs, rms, rmax = cycle.residual_stats(cuda(x))
    assert mfs.shape == x.shape[1:] and np.array_equal(mfs.cpu().numpy(), ref)
    check_stats(f'st{k} fp{bits(dtype)}', ref, None, rms, rmax, g[f'st{k}_std32'] if dtype == np.float32 else None)
    mfs2, rms2, rmax2 = cycle.residual_stats(cuda(x), cuda(model))
    assert np.array_equal(mfs2.cpu().numpy(), ref) and np.array_equal(x, keep)
    quiet = ~np.any(model, axis=0)
    assert int(quiet.sum()) == int(g[f'st{k}_nquiet'])
    check_stats(f'st{k} fp{bits(dtype)} model', ref, quiet, rms2, rmax2,
                g[f'st{k}_qstd32'] if dtype == np.float32 and quiet.any() else None)


@pytest.mark.parametrize('dtype,shape', [(np.float32, (2, 1025, 1024)), (np.float64, (2, 1025, 1024)),
                                         (np.float32, (3, 513, 515)), (np.float64, (3, 513, 515))])
def test_residual_stats_grid_stride(dtype, shape):
    """More packs than the 1024 x 256 threads of the largest grid, so the grid-stride loop runs at least twice:
    1025 x 1024 pixels are 262400 float32 packs (2 trips) / 524800 float64 packs (3 trips); 513 x 515 = 264195 is odd,
    the one-element path, 264195 > 262144 threads (2 trips).  Also: two calls give the same bits."""
    from pfb_clean_amd.utils import cycle
    rng = np.random.default_rng(7)
    x = (0.3 + rng.standard_normal(shape)).astype(dtype)
    model = np.zeros((2,) + shape[1:], dtype=dtype)
    on = rng.random(shape[1:]) < 0.1
    model[1][on] = 1.5
    xd, md = cuda(x), cuda(model)
    mfs, rms, rmax = cycle.residual_stats(xd, md)
    ref = np.sum(x, axis=0)
    assert np.array_equal(mfs.cpu().numpy(), ref)
    check_stats(f'{shape} {np.dtype(dtype).name}', ref, ~on, rms, rmax)
    mfs_b, rms_b, rmax_b = cycle.residual_stats(xd, md)
    assert torch.equal(mfs, mfs_b) and rms == rms_b and rmax == rmax_b


def offset_view(a, shift):
    """A device copy of `a` that starts `shift` elements past a 16-byte boundary."""
    t = torch.from_numpy(a)
    flat = torch.empty(a.size + 4, dtype=t.dtype, device='cuda')
    assert flat.data_ptr() % 16 == 0
    view = flat[shift:shift + a.size].view(a.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == shift * a.itemsize
    return view


@pytest.mark.parametrize('dtype,shift', [(np.float32, 1), (np.float32, 2), (np.float32, 3), (np.float64, 1)])
@pytest.mark.parametrize('which', ['residual', 'model'])
def test_residual_stats_any_base_alignment(which, dtype, shift):
    """(8,96,130) has aligned planes; the residual or the model `shift` elements past a 16-byte boundary."""
    from pfb_clean_amd.utils import cycle
    x, model, ref = stat_input(3, dtype)
    xd = offset_view(x, shift) if which == 'residual' else cuda(x)
    md = offset_view(model, shift) if which == 'model' else cuda(model)
    mfs, rms, rmax = cycle.residual_stats(xd, md)
    assert np.array_equal(mfs.cpu().numpy(), ref)
    check_stats(f'{which} + {shift}', ref, ~np.any(model, axis=0), rms, rmax)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('k', [1, 3])
def test_residual_stats_model_cases(k, dtype):
    from pfb_clean_amd.utils import cycle
    x, model, ref = stat_input(k, dtype)
    xd = cuda(x)
    # a support that covers everything: no quiet pixel, rms is nan like np.std of an empty selection
    full = np.zeros_like(model)
    full[1] = 1.0
    mfs, rms, rmax = cycle.residual_stats(xd, cuda(full))
    assert np.array_equal(mfs.cpu().numpy(), ref) and np.isnan(rms) and rmax == float(np.abs(ref).max())
    # -0.0 is quiet
    negz = np.zeros_like(model)
    negz[0, ::2] = -0.0
    negz[2, :, 1::3] = -0.0
    assert np.signbit(negz).any() and not np.any(negz, axis=0).any()
    _, rms, rmax = cycle.residual_stats(xd, cuda(negz))
    check_stats(f'st{k} -0.0', ref, None, rms, rmax)
    # a NaN in the model is not quiet
    nanm = np.zeros_like(model)
    nanm[1, 2, 3] = np.nan
    nanm[2, -1, -1] = np.nan
    quiet = ~np.any(nanm, axis=0)
    assert quiet.sum() == quiet.size - 2
    _, rms, rmax = cycle.residual_stats(xd, cuda(nanm))
    check_stats(f'st{k} nan model', ref, quiet, rms, rmax)


@pytest.mark.parametrize('dtype', DTYPES)
def test_residual_stats_nan_in_the_residual(dtype):
    from pfb_clean_amd.utils import cycle
    x, model, _ = stat_input(3, dtype)
    x = x.copy()
    x[5, 40, 77] = np.nan
    mfs, rms, rmax = cycle.residual_stats(cuda(x))
    assert np.array_equal(mfs.cpu().numpy(), np.sum(x, axis=0), equal_nan=True)
    assert np.isnan(rms) and np.isnan(rmax)
    # under the model's support the NaN reaches rmax only
    model = np.zeros_like(model)
    model[0, 40, 77] = 1.0
    _, rms, rmax = cycle.residual_stats(cuda(x), cuda(model))
    assert np.isfinite(rms) and np.isnan(rmax)


def test_residual_stats_large_mean_does_not_cancel():
    """1e8 + randn in float64: std ~ 1 on a mean of 1e8.  Sums of x and x^2 lose about six digits here."""
    from pfb_clean_amd.utils import cycle
    rng = np.random.default_rng(11)
    x = 1e8 + rng.standard_normal((1, 96, 130))
    mfs, rms, rmax = cycle.residual_stats(cuda(x))
    assert np.array_equal(mfs.cpu().numpy(), x[0])
    check_stats('1e8 + randn', x[0], None, rms, rmax)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('source', ['random', 'psi'])
def test_rms_comps(source, dtype):
    from pfb_clean_amd.utils import cycle
    tdtype = torch.float32 if dtype == np.float32 else torch.float64
    rng = np.random.default_rng(5)
    if source == 'random':
        alpha = cuda(rng.standard_normal((3, 2, 21, 19)).astype(dtype))
    else:
        from pfb_clean_amd.operators.psi import Psi
        psi = Psi(2, 32, 48, ('self', 'db2'), 2, dtype=tdtype)
        alpha = torch.zeros((2, 2, psi.Nymax, psi.Nxmax), dtype=tdtype, device='cuda')
        psi.dot(cuda(rng.standard_normal((2, 32, 48)).astype(dtype)), alpha)
        psi.close()
    got = cycle.rms_comps(alpha)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == tdtype and got.shape == (alpha.shape[1], 1, 1)
    a = alpha.cpu().numpy()
    assert np.array_equal(np.sum(a, axis=0), _bandsum_of(alpha))
    exp = np.std(np.sum(a, axis=0).astype(np.float64), axis=(-1, -2)).astype(dtype)[:, None, None]
    err, ulp = np.abs(got.cpu().numpy() - exp), np.spacing(exp)
    print(f'rms_comps {source} {np.dtype(dtype).name}: {got.flatten().tolist()} err {err.ravel().tolist()} '
          f'(ulp {ulp.ravel().tolist()})')
    assert np.all(err <= ulp)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', [(3, 2, 21, 19), (2, 3, 16, 24)])
def test_bandsum_of_several_sets_with_sum_out(shape, dtype):
    """pfb_bandsum_stats with nset > 1 AND a sum_out: every set's plane of the band sum lands at its own offset, and
    the records are those of float64 numpy on that band sum.  21 x 19 is odd (one element per lane), 16 x 24 aligned."""
    from pfb_clean_amd.utils import cycle
    rng = np.random.default_rng(23)
    a = (0.2 + rng.standard_normal(shape)).astype(dtype)
    nband, nset, ny, nx = shape
    ad = cuda(a)
    sum_out = torch.full((nset, ny, nx), float('nan'), dtype=ad.dtype, device='cuda')
    rec = cycle._stats(ad, nband, nset, ny * nx, None, sum_out).cpu().numpy()
    ref = np.sum(a, axis=0)
    assert np.array_equal(sum_out.cpu().numpy(), ref)
    assert rec.shape == (nset, cycle.RECORD)
    for s in range(nset):
        count, mean, m2, amax = rec[s].tolist()
        assert count == ny * nx
        check_stats(f'set {s} of {shape}', ref[s], None, float(np.sqrt(m2 / count)), amax)
        assert abs(mean - ref[s].astype(np.float64).mean()) <= 4 * count * EPS64 * np.abs(ref[s]).max()


def _bandsum_of(alpha):
    """np.sum(alpha, 0) as the device forms it: the band sum of the (nband, nbasis * Nymax, Nxmax) view."""
    from pfb_clean_amd.utils import cycle
    nband, nbasis, ny, nx = alpha.shape
    mfs, _, _ = cycle.residual_stats(alpha.view(nband, nbasis * ny, nx))
    return mfs.view(nbasis, ny, nx).cpu().numpy()


def test_model_change():
    from pfb_clean_amd.utils import cycle
    rng = np.random.default_rng(3)
    model = rng.standard_normal((3, 33, 65)).astype(np.float32)
    modelp = model + 0.01 * rng.standard_normal(model.shape).astype(np.float32)
    ref = np.linalg.norm((model.astype(np.float64) - modelp).ravel()) / np.linalg.norm(model.astype(np.float64).ravel())
    for got in (cycle.model_change(cuda(model), cuda(modelp)), cycle.model_change(model, modelp)):
        assert isinstance(got, float) and abs(got - ref) <= 1e-6 * ref
    zero = torch.zeros((2, 8, 8), dtype=torch.float64, device='cuda')
    assert np.isnan(cycle.model_change(zero, zero)) and np.isinf(cycle.model_change(zero, zero + 1.0))


# ---------------------------------------------------------------------------------------------------- closing
def close_cases(shape):
    g = load()
    return [k for k in range(int(g['nclose'])) if g[f'cl{k}_mask'].shape == shape]


@pytest.mark.parametrize('shape', CLOSE_SHAPES)
def test_close_mask_golden(shape):
    """Every stored pattern of the shape: single pixels at the corners, on the edges (they vanish) and inside, pairs
    with gaps of 1, 2 and 3 along each axis, diagonal pairs, random densities 0.02 / 0.2 / 0.6, pixels and gaps across
    columns 63 / 64 / 65 and rows 31 / 32 / 33 (the 32 x 64 tile), all ones, all zeros."""
    from pfb_clean_amd.utils import cycle
    g = load()
    cases = close_cases(shape)
    assert cases
    for k in cases:
        mask = cuda(g[f'cl{k}_mask'])
        for d in (0, 1, 2, 3):
            got = cycle.close_mask(mask, d)
            assert got.dtype == torch.bool and got.shape == mask.shape
            assert np.array_equal(got.cpu().numpy(), g[f'cl{k}_out{d}']), (str(g['close_names'][k]), d)


def test_close_mask_kinds():
    from pfb_clean_amd.utils import cycle
    g = load()
    k = close_cases((65, 129))[10]
    mask = g[f'cl{k}_mask']
    got = cycle.close_mask(mask, 2)
    assert isinstance(got, np.ndarray) and got.dtype == bool and np.array_equal(got, g[f'cl{k}_out2'])
    got = cycle.close_mask(cuda(mask.astype(np.uint8) * 7), 2)          # uint8: anything non-zero is in
    assert np.array_equal(got.cpu().numpy(), g[f'cl{k}_out2'])
    assert np.array_equal(cycle.close_mask(mask), g[f'cl{k}_out1'])     # the default is the cross


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', [(7, 5), (65, 129), (130, 70)])
def test_mop_mask_from_a_cube(shape, dtype):
    """The support of a 3-band cube whose non-zero values are spread over the bands, then the closing."""
    from pfb_clean_amd.utils import cycle
    g = load()
    rng = np.random.default_rng(9)
    for k in close_cases(shape):
        mask = g[f'cl{k}_mask']
        ii, jj = np.nonzero(mask)
        cube = np.zeros((3,) + shape, dtype=dtype)
        cube[(ii + 2 * jj) % 3, ii, jj] = rng.choice([-1.0, 1.0], ii.size) * (0.1 + rng.random(ii.size))
        assert np.array_equal(np.any(cube, axis=0), mask)
        cd = cuda(cube)
        assert np.array_equal(cycle.support(cd).cpu().numpy(), mask)
        for d in (0, 1, 2, 3):
            got = cycle.mop_mask(cd, d)
            assert np.array_equal(got.cpu().numpy(), g[f'cl{k}_out{d}']), (str(g['close_names'][k]), d)
    # a NaN is in the support, -0.0 is not
    cube = np.zeros((3,) + shape, dtype=dtype)
    cube[1, 3, 2], cube[2, 4, 4], cube[0, 1, 1] = np.nan, -0.0, -0.0
    assert np.array_equal(cycle.support(cube), np.any(cube, axis=0)) and cycle.support(cube).sum() == 1


@pytest.mark.parametrize('dtype', DTYPES)
def test_support_with_a_threshold(dtype):
    from pfb_clean_amd.utils import cycle
    cube = np.zeros((3, 33, 65), dtype=dtype)
    cube[0, 1, 1], cube[1, 1, 2], cube[2, 1, 3] = 0.5, 0.25, 0.75           # equal to, below, above 0.5
    cube[0, 2, 1], cube[2, 2, 1] = 0.25, 0.75                               # above in another band only
    cube[1, 3, 3], cube[1, 3, 4], cube[1, 3, 5] = -2.0, np.nan, np.inf
    cube[0, 4, 1], cube[0, 4, 2] = np.nextafter(dtype(0.5), dtype(1)), np.nextafter(dtype(0.5), dtype(0))
    cube[2, 5, 1], cube[2, 5, 2] = dtype(0.1), np.nextafter(dtype(0.1), dtype(1))   # the bound rounded to the dtype
    for thr in (0.5, 0.1, 0.0, -3.0):
        ref = np.any(cube > thr, axis=0)
        got = cycle.support(cuda(cube), thr)
        assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), ref), thr
    ref = np.any(cube > 0.5, axis=0)
    assert ref[1, 3] and not ref[1, 1] and not ref[1, 2] and ref[2, 1] and ref[4, 1] and not ref[4, 2] and not ref[3, 4]
    assert not np.any(cube > 0.1, axis=0)[5, 1] and np.any(cube > 0.1, axis=0)[5, 2]


# --------------------------------------------------------------------------------------------- masked problem
def masked_ref(residual, mask, beam, seed):
    maskf = mask.astype(residual.dtype)
    with np.errstate(invalid='ignore'):
        be = beam * maskf[None] if beam is not None else maskf[None]
        b = be * residual
    x0 = np.zeros_like(residual)
    if seed is not None:
        x0[:, mask] = seed[mask]
    return b, x0, be


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', [(3, 5, 7), (2, 33, 65), (2, 32, 64)])
def test_masked_problem(shape, dtype):
    """(3,5,7) and (2,33,65) have odd planes (one element per lane); (2,32,64) takes the 16-byte form."""
    from pfb_clean_amd.utils import cycle
    rng = np.random.default_rng(13)
    nband, nx, ny = shape
    residual = rng.standard_normal(shape).astype(dtype)
    mask = rng.random((nx, ny)) < 0.4
    seed = rng.standard_normal((nx, ny)).astype(dtype)
    beams = {'none': None, 'cube': (0.5 + rng.random(shape)).astype(dtype),
             'one': (0.5 + rng.random((1, nx, ny))).astype(dtype)}
    nanres = residual.copy()
    out_i, out_j = np.argwhere(~mask)[0]
    in_i, in_j = np.argwhere(mask)[0]
    nanres[0, out_i, out_j] = np.nan                        # outside the mask: 0 * nan stays nan
    nanres[nband - 1, in_i, in_j] = np.nan
    rd, nd, md, sd = cuda(residual), cuda(nanres), cuda(mask), cuda(seed)
    for bname, beam in beams.items():
        bd = None if beam is None else cuda(beam)
        for sname, (s, sdev) in {'seed': (seed, sd), 'noseed': (None, None)}.items():
            for res, resd in ((residual, rd), (nanres, nd)):
                ref = masked_ref(res, mask, beam, s)
                got = cycle.masked_problem(resd, md, bd, sdev)
                for name, r, t in zip(cycle.ALL_OUTPUTS, ref, got):
                    assert t.dtype == rd.dtype and tuple(t.shape) == r.shape, (bname, sname, name)
                    assert np.array_equal(t.cpu().numpy(), r, equal_nan=True), (bname, sname, name)
        # each output left out in turn
        ref = masked_ref(residual, mask, beam, seed)
        for skip in range(3):
            names = tuple(n for i, n in enumerate(cycle.ALL_OUTPUTS) if i != skip)
            got = cycle.masked_problem(rd, md, bd, sd, outputs=names)
            assert got[skip] is None
            for i in range(3):
                if i != skip:
                    assert np.array_equal(got[i].cpu().numpy(), ref[i]), (bname, skip, i)
    ref = masked_ref(nanres, mask, None, None)
    assert np.isnan(ref[0][0, out_i, out_j]) and np.isnan(ref[0][nband - 1, in_i, in_j])
    # a uint8 mask, and a cube off the 16-byte boundary
    got = cycle.masked_problem(offset_view(residual, 1), cuda(mask.astype(np.uint8) * 3), cuda(beams['cube']), sd)
    for r, t in zip(masked_ref(residual, mask, beams['cube'], seed), got):
        assert np.array_equal(t.cpu().numpy(), r)


# ------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize('dtype', DTYPES)
def test_mop_end_to_end(dtype):
    """klean.py:278-317 at 64 x 64 x 3 bands with this module's tensors, and again with numpy-built inputs of the same
    values: the inputs are identical, so pcg_psf returns the same x bit for bit."""
    from pfb_clean_amd.utils import cycle
    from pfb_clean_amd.opt.pcg import pcg_psf
    rng = np.random.default_rng(17)
    nband, nx, ny = 3, 64, 64
    Q = 2 * ny
    u = np.fft.fftfreq(2 * nx)[:, None]
    v = np.fft.rfftfreq(Q)[None, :]
    psfhat = np.stack([np.exp(-(u ** 2 + v ** 2) / (2 * w ** 2)) for w in (0.1, 0.15, 0.2)])
    psfhat = psfhat.astype(np.complex64 if dtype == np.float32 else np.complex128)
    residual = rng.standard_normal((nband, nx, ny)).astype(dtype)
    model = np.zeros((nband, nx, ny), dtype=dtype)
    for _ in range(12):
        i, j = rng.integers(2, nx - 4), rng.integers(2, ny - 5)
        model[rng.integers(0, nband), i:i + 2, j:j + 3:2] = 1.0 + rng.random()
    cgopts = dict(tol=0.0, maxit=5, minit=5, verbosity=0, backtrack=True)

    rd, md = cuda(residual), cuda(model)
    mfs, rms, rmax = cycle.residual_stats(rd, md)
    mask = cycle.mop_mask(md, 2)
    b, x0, beam = cycle.masked_problem(rd, mask, seed=mfs)
    x = pcg_psf(psfhat, b, x0, beam, Q, 1, rmax, cgopts)
    assert isinstance(x, torch.Tensor) and x.shape == rd.shape

    mask_np = mask.cpu().numpy()
    assert mask_np.sum() > np.any(model, axis=0).sum() > 0          # the closing filled the gaps of the components
    mfs_np = np.sum(residual, axis=0)
    rmax_np = float(np.abs(mfs_np).max())
    x0_np = np.zeros_like(residual)
    x0_np[:, mask_np] = mfs_np[mask_np]
    mopmask = mask_np[None, :, :].astype(dtype)
    assert rmax_np == rmax
    assert np.array_equal(b.cpu().numpy(), mopmask * residual) and np.array_equal(x0.cpu().numpy(), x0_np)
    assert np.array_equal(beam.cpu().numpy(), mopmask)
    x_np = pcg_psf(psfhat, mopmask * residual, x0_np, mopmask, Q, 1, rmax_np, cgopts)
    assert isinstance(x_np, np.ndarray) and np.array_equal(x.cpu().numpy(), x_np)
    assert np.isfinite(x_np).all() and np.any(x_np != x0_np)


# ------------------------------------------------------------------------------------------------------ kinds
def test_numpy_in_numpy_out_tensors_in_tensors_out():
    from pfb_clean_amd.utils import cycle
    x, model, ref = stat_input(2, np.float32)
    mask = ~np.any(model, axis=0)
    for conv, kind in ((lambda a: a, np.ndarray), (cuda, torch.Tensor)):
        mfs, rms, rmax = cycle.residual_stats(conv(x), conv(model))
        assert isinstance(mfs, kind) and isinstance(rms, float) and isinstance(rmax, float)
        for res in (cycle.support(conv(model)), cycle.mop_mask(conv(model)), cycle.close_mask(conv(mask))):
            assert isinstance(res, kind) and res.dtype in (bool, torch.bool)
        for res in cycle.masked_problem(conv(x), conv(mask), seed=conv(ref)):
            assert isinstance(res, kind)
        alpha = conv(np.stack([x, x[::-1]], axis=1))
        rc = cycle.rms_comps(alpha)
        assert isinstance(rc, kind) and rc.shape == (2, 1, 1) and rc.dtype == alpha.dtype
        assert isinstance(cycle.model_change(conv(x), conv(x + 1)), float)
    assert cycle.rms_comps(cuda(np.stack([x, x], axis=1))).is_cuda


def test_rejects_wrong_shapes_and_dtypes():
    from pfb_clean_amd.utils import cycle
    x = np.zeros((2, 8, 9), dtype=np.float32)
    half = torch.zeros((2, 8, 9), dtype=torch.float16, device='cuda')
    with pytest.raises(ValueError, match=r'\(8, 9\)'):
        cycle.residual_stats(x[0])
    with pytest.raises(ValueError, match=r'\(2, 8, 8\)'):
        cycle.residual_stats(x, np.zeros((2, 8, 8), dtype=np.float32))
    with pytest.raises(TypeError):
        cycle.residual_stats(x, np.zeros((2, 8, 9), dtype=np.float64))
    with pytest.raises(TypeError):
        cycle.residual_stats(half)
    with pytest.raises(TypeError):
        cycle.residual_stats([[1.0]])
    with pytest.raises(ValueError):
        cycle.rms_comps(x)
    with pytest.raises(ValueError):
        cycle.mop_mask(x[0])
    with pytest.raises(ValueError):
        cycle.close_mask(np.zeros((2, 8, 9), dtype=bool))
    with pytest.raises(TypeError):
        cycle.close_mask(np.zeros((8, 9), dtype=np.float32))
    with pytest.raises(ValueError, match=r'\(8, 8\)'):
        cycle.masked_problem(x, np.zeros((8, 8), dtype=bool))
    with pytest.raises(ValueError):
        cycle.masked_problem(x, np.zeros((8, 9), dtype=bool), beam=np.zeros((3, 8, 9), dtype=np.float32))
    with pytest.raises(TypeError):
        cycle.masked_problem(x, np.zeros((8, 9), dtype=bool), seed=np.zeros((8, 9), dtype=np.float64))
    with pytest.raises(ValueError):
        cycle.masked_problem(x, np.zeros((8, 9), dtype=bool), outputs=('b', 'c'))
    with pytest.raises(ValueError):
        cycle.model_change(x, x[:1])
