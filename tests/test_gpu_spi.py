"""
Spectral index and reference-flux maps on the MI355X (pfb_clean_amd.utils.spi: fit_spi, fit_spi_components) against
the numpy oracles of tests/spi_cases.py.  The oracle always runs on the float64 upcast of the stored float32 inputs.

Bounds (scale = the largest magnitude of an output over the compared components, spread = the change of the oracle's
own output under a 1-ulp move of every datum, relative to scale; tests/test_cpu_spi.py holds spread <= 1e-11,
rho <= 0.5 on the stored cases):
  values        with tol = 1e-10 on both sides: |got - oracle| <= (1e-12 + 50 spread) scale per output.  Both sides
                take the same number of steps, what separates them is rounding: x ** alpha against exp(alpha ln x),
                fused against unfused sums.  float32 maps add their final rounding, 6e-8 |oracle|.
  default tol   tol = 1e-5 against the oracle converged at tol = 1e-13: the same bound + tol.  The last step is at
                most tol, and with rho <= 0.5 what is left of the way to the limit is at most tol as well.
  nband = 2     only alpha and I0 are compared: the fit interpolates, chi2 is rounding noise, the errors are noise
                over noise.
  mask          equal to numpy's, the maps NaN exactly off it; also with more workgroups (259) than one 256-entry tile
                of the scan, where the counts' carry and the maximum must cross tiles.
threshold and pb_min are exactly representable in float32, so numpy's scalar casting cannot matter.
"""
import io
import warnings

import numpy as np
import pytest
import torch

import spi_cases as sc

pytestmark = pytest.mark.gpu

NCASE = len(sc.CASES)
THRESHOLD = 2.0 ** -14
PB_MIN = 0.25
_memo = {}


def memo(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def as_kind(a, kind):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if kind == 'tensor' else a


def to_np(a, kind):
    if kind == 'tensor':
        assert isinstance(a, torch.Tensor) and a.is_cuda
        return a.cpu().numpy()
    assert isinstance(a, np.ndarray)
    return a


def held(nband):
    return [0, 2] if nband == 2 else [0, 1, 2, 3]


def check_values(got, ref, spread, rows, extra_abs=0.0, rel32=False, what=''):
    """got, ref: (4, n); NaN exactly where the oracle has NaN, the bound of the header elsewhere."""
    assert got.shape == ref.shape
    scale = sc.scale(ref)
    for k in rows:
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), (what, sc.OUTPUTS[k])
        ok = ~np.isnan(ref[k])
        err = np.abs(got[k][ok].astype(np.float64) - ref[k][ok])
        bound = (1e-12 + 50 * spread[k]) * scale[k] + extra_abs + (6e-8 * np.abs(ref[k][ok]) if rel32 else 0.0)
        worst = float(np.max(err / bound)) if err.size else 0.0
        print(f"{what} {sc.OUTPUTS[k]}: max err / bound {worst:.3g} (spread {spread[k]:.2e}, scale {scale[k]:.3g})")
        assert np.all(err <= bound), (what, sc.OUTPUTS[k], float(err.max()), worst)


def run_components(c, kind, **kw):
    from pfb_clean_amd.utils.spi import fit_spi_components
    out = fit_spi_components(as_kind(c['data'].astype(np.float64), kind), c['weights'], c['freqs'], c['ref_freq'],
                             beam=as_kind(c['beam'].astype(np.float64), kind), **kw)
    out = to_np(out, kind)
    assert out.dtype == np.float64 and out.shape == (4, c['ncomps'])
    return out


def run_cube(image, beam, c, kind, threshold=THRESHOLD, pb_min=PB_MIN, **kw):
    """The device maps as a (4, nx, ny) numpy array of the image's dtype, and what fit_spi printed."""
    from pfb_clean_amd.utils.spi import fit_spi
    dest = io.StringIO()
    maps = fit_spi(as_kind(image, kind), as_kind(beam, kind), c['freqs'], c['weights'], threshold, 4, pb_min, 0.1,
                   c['ref_freq'], dest, **kw)
    assert isinstance(maps, tuple) and len(maps) == 4
    maps = np.stack([to_np(m, kind) for m in maps])
    assert maps.dtype == image.dtype and maps.shape == (4,) + image.shape[1:]
    return maps, dest.getvalue()


def oracle_cube(image, beam, c, threshold=THRESHOLD, pb_min=PB_MIN, **kw):
    """(maps (4, nx, ny) float64, maskindices, fit (4, ncomps), spread (4,)) of the float64 upcast."""
    i64, b64 = image.astype(np.float64), beam.astype(np.float64)
    *maps, idx = sc.fit_spi(i64, b64, c['freqs'], c['weights'], threshold, pb_min, c['ref_freq'], **kw)
    cut = np.where(b64 > pb_min, i64, 0)
    d, B = cut[:, idx[:, 0], idx[:, 1]].T.copy(), b64[:, idx[:, 0], idx[:, 1]].T.copy()
    spread = sc.spread_of(d, B, c['weights'], c['freqs'], c['ref_freq'], **kw)
    return np.stack(maps), idx, np.stack([m[idx[:, 0], idx[:, 1]] for m in maps]), spread


def check_cube(maps, omaps, idx, spread, nband, what, extra_abs=0.0):
    on = np.zeros(omaps.shape[1:], dtype=bool)
    on[idx[:, 0], idx[:, 1]] = True
    assert np.isnan(maps[:, ~on]).all(), what
    got = np.stack([m[idx[:, 0], idx[:, 1]] for m in maps])
    ref = np.stack([m[idx[:, 0], idx[:, 1]] for m in omaps])
    check_values(got, ref, spread, held(nband), extra_abs=extra_abs, rel32=maps.dtype == np.float32, what=what)


# ------------------------------------------------------------------------------------------- component-list form
@pytest.mark.parametrize('kind', ['numpy', 'tensor'])
@pytest.mark.parametrize('i', range(NCASE))
def test_components_values(i, kind):
    c = sc.case(i)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        got = run_components(c, kind, tol=1e-10)
    ref = memo(('o10', i), lambda: sc.oracle(c, tol=1e-10))
    check_values(got, ref, sc.spread(c, 1e-10), held(c['nband']), what=f'list {sc.CASES[i]}')


@pytest.mark.parametrize('i', range(NCASE))
def test_components_default_tol(i):
    c = sc.case(i)
    got = run_components(c, 'tensor')
    ref = memo(('o13', i), lambda: sc.oracle(c, tol=1e-13))
    check_values(got, ref, sc.spread(c, 1e-13), held(c['nband']), extra_abs=1e-5, what=f'default tol {sc.CASES[i]}')


@pytest.mark.parametrize('n', [1, 63, 64, 65, 255, 256, 257, 3 * 256 + 17])
def test_components_dispatch_edges(n):
    """One lane per component in workgroups of 256: a wave and a workgroup, each - 1 / exact / + 1, and a tail."""
    from pfb_clean_amd.utils.spi import fit_spi_components
    c = sc.case(3)
    rows = np.arange(n) % c['ncomps']
    got = fit_spi_components(c['data'].astype(np.float64)[rows], c['weights'], c['freqs'], c['ref_freq'],
                             beam=c['beam'].astype(np.float64)[rows], tol=1e-10)
    ref = memo(('o10', 3), lambda: sc.oracle(c, tol=1e-10))[:, rows]
    check_values(got, ref, sc.spread(c, 1e-10), [0, 1, 2, 3], what=f'ncomps {n}')


def test_components_start_values_and_no_beam():
    """alphai, I0i and beam=None are honoured: one step from a given start depends on the start."""
    from pfb_clean_amd.utils.spi import fit_spi_components
    c = sc.case(2)
    d = c['data'].astype(np.float64)
    rng = np.random.default_rng(7)
    a0, i0 = rng.uniform(-1.5, 0.5, c['ncomps']), d[:, 0] * rng.uniform(0.8, 1.2, c['ncomps'])
    args = (c['weights'], c['freqs'], c['ref_freq'])
    for kw in ({'alphai': a0}, {'I0i': i0}, {'alphai': a0, 'I0i': i0}, {}):
        with pytest.warns(UserWarning):
            got = fit_spi_components(d, *args, maxiter=1, **kw)
        ref = sc.fit_components(d, *args, maxiter=1, **kw)
        spread = sc.spread_of(d, None, *args, maxiter=1, **kw)
        check_values(got, ref, spread, [0, 1, 2, 3], what=f'start {sorted(kw)}')
    plain = sc.fit_components(d, *args, maxiter=1)
    assert np.abs(sc.fit_components(d, *args, maxiter=1, alphai=a0)[0] - plain[0]).max() > 1e-3
    assert np.abs(sc.fit_components(d, *args, maxiter=1, I0i=i0)[0] - plain[0]).max() > 1e-3
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        got = fit_spi_components(as_kind(d, 'tensor'), *args, tol=1e-10)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float64
    ref = sc.fit_components(d, *args, tol=1e-10)
    check_values(got.cpu().numpy(), ref, sc.spread_of(d, None, *args, tol=1e-10), [0, 1, 2, 3], what='beam=None')


@pytest.mark.parametrize('form', ['list', 'cube'])
def test_single_step(form):
    """maxiter = 1 returns exactly one oracle step and warns once with the number of components."""
    c = sc.case(3)
    if form == 'list':
        with pytest.warns(UserWarning) as rec:
            got = run_components(c, 'numpy', maxiter=1)
        ref, info = sc.oracle(c, maxiter=1, info=True)
        assert info['late'] == c['ncomps']
        check_values(got, ref, sc.spread(c, 1e-5, 1), [0, 1, 2, 3], what='one step, list')
        n = c['ncomps']
    else:
        image, beam = sc.cube_of(c, 37, 29, sc.pixels_of(c['ncomps'], 37, 29, 3))
        with pytest.warns(UserWarning) as rec:
            maps, _ = run_cube(image, beam, c, 'numpy', maxiter=1)
        omaps, idx, _, spread = oracle_cube(image, beam, c, maxiter=1)
        check_cube(maps, omaps, idx, spread, c['nband'], 'one step, cube')
        n = len(idx)
    assert len(rec) == 1 and str(rec[0].message).startswith(f"{n} components")


def test_degenerate_component_only():
    """All-zero data with I0i = 0 makes j0 zero, hence det = 0: NaN for that component only."""
    from pfb_clean_amd.utils.spi import fit_spi_components
    c = sc.case(3)
    d = np.vstack((c['data'].astype(np.float64)[:70], np.zeros((1, c['nband']))))
    B = np.vstack((c['beam'].astype(np.float64)[:70], np.full((1, c['nband']), 0.5)))
    ref_band = int(np.argmin(np.abs(c['freqs'] - c['ref_freq'])))
    i0 = d[:, ref_band].copy()
    args = (c['weights'], c['freqs'], c['ref_freq'])
    got = fit_spi_components(d, *args, I0i=i0, beam=B, tol=1e-10)
    assert np.isnan(got[:, 70]).all() and np.isfinite(got[:, :70]).all()
    ref = sc.fit_components(d, *args, I0i=i0, beam=B, tol=1e-10)
    check_values(got, ref, sc.spread_of(d, B, *args, I0i=i0, tol=1e-10), [0, 1, 2, 3], what='degenerate')


def test_unsupported_band_count():
    from pfb_clean_amd import _lib
    from pfb_clean_amd.utils.spi import fit_spi, fit_spi_components
    freqs, w = np.linspace(0.9e9, 1.7e9, 65), np.ones(65)
    with pytest.raises(_lib.PfbHipError) as e:
        fit_spi_components(np.ones((3, 65)), w, freqs, 1.3e9)
    assert e.value.code == _lib.PFB_ERR_UNSUPPORTED
    cube = np.ones((65, 4, 4), dtype=np.float32)
    with pytest.raises(_lib.PfbHipError) as e:
        fit_spi(cube, cube, freqs, w, 0.0, 1, 0.1, 0.0, 1.3e9, io.StringIO())
    assert e.value.code == _lib.PFB_ERR_UNSUPPORTED


# ----------------------------------------------------------------------------------------------------- cube form
@pytest.mark.parametrize('kind', ['numpy', 'tensor'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('i', range(NCASE))
def test_cube_values(i, dtype, kind):
    """37 x 29: npix = 1073 is odd, so the planes of the fp32 cube (and of the fp64 cube) leave the 16-byte grid."""
    c = sc.case(i)
    image, beam = sc.cube_of(c, 37, 29, sc.pixels_of(c['ncomps'], 37, 29, i), dtype=dtype)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        maps, said = run_cube(image, beam, c, kind, tol=1e-10)
    omaps, idx, _, spread = memo(('cube', i), lambda: oracle_cube(image, beam, c, tol=1e-10))
    assert len(idx) == c['ncomps'] and idx[0].tolist() == [0, 0] and idx[-1].tolist() == [36, 28]
    assert said == "Fitting %i components\nDone. Writing output. \n\n" % c['ncomps']
    check_cube(maps, omaps, idx, spread, c['nband'], f'cube {sc.CASES[i]} {np.dtype(dtype).name} {kind}')


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_cube_default_tol(dtype):
    c = sc.case(3)
    image, beam = sc.cube_of(c, 37, 29, sc.pixels_of(c['ncomps'], 37, 29, 3), dtype=dtype)
    maps, _ = run_cube(image, beam, c, 'tensor')
    omaps, idx, _, spread = memo('cube13', lambda: oracle_cube(image, beam, c, tol=1e-13))
    check_cube(maps, omaps, idx, spread, c['nband'], f'cube default tol {np.dtype(dtype).name}', extra_abs=1e-5)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_cube_single_pixel(dtype):
    c = sc.case(1)
    image, beam = sc.cube_of(c, 1, 1, [(0, 0)], dtype=dtype)
    maps, said = run_cube(image, beam, c, 'numpy', tol=1e-10)
    assert said.startswith("Fitting 1 components\n")
    ref = memo(('o10', 1), lambda: sc.oracle(c, tol=1e-10))[:, :1]
    check_values(maps.reshape(4, 1), ref, sc.spread(c, 1e-10), [0, 1, 2, 3], rel32=dtype == np.float32,
                 what=f'1 x 1 {np.dtype(dtype).name}')


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_cube_full_mask(dtype):
    """64 x 64 with every pixel fitted: 4096 components, 16 workgroups of the fit, aligned planes, all-ones words."""
    c = sc.case(3)
    rows = np.arange(64 * 64) % c['ncomps']
    image = np.ascontiguousarray(c['data'][rows].T.reshape(c['nband'], 64, 64).astype(dtype))
    beam = np.ascontiguousarray(c['beam'][rows].T.reshape(c['nband'], 64, 64).astype(dtype))
    maps, said = run_cube(image, beam, c, 'tensor', tol=1e-10)
    assert said.startswith("Fitting 4096 components\n")
    ref = memo(('o10', 3), lambda: sc.oracle(c, tol=1e-10))[:, rows]
    check_values(maps.reshape(4, -1), ref, sc.spread(c, 1e-10), [0, 1, 2, 3], rel32=dtype == np.float32,
                 what=f'full mask {np.dtype(dtype).name}')


def edge_cube(nx, ny, dtype):
    """Case 3 (8 bands) with, beside ordinary components at (0, 0), (nx - 1, ny - 1) and seeded pixels: a NaN in one
    band, a NaN beam, a beam equal to pb_min, a minimum equal to the threshold.  Returns the cubes and those four."""
    c = sc.case(3)
    pix = sc.pixels_of(40, nx, ny, 11)
    image, beam = sc.cube_of(c, nx, ny, pix, dtype=dtype)
    nan_band, nan_beam, at_pb_min, at_threshold = pix[5], pix[6], pix[7], pix[8]
    image[2][nan_band] = np.nan
    beam[5][nan_beam] = np.nan
    beam[1][at_pb_min] = PB_MIN
    image[6][at_threshold] = THRESHOLD                       # not the reference band: the start I0 stays ordinary
    return c, image, beam, (nan_band, nan_beam, at_pb_min, at_threshold)


@pytest.mark.parametrize('kind', ['numpy', 'tensor'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('shape', [(37, 29), (64, 64)])
def test_mask_edges(shape, dtype, kind):
    c, image, beam, special = edge_cube(*shape, dtype)
    maps, said = run_cube(image, beam, c, kind, tol=1e-10)
    omaps, idx, _, spread = oracle_cube(image, beam, c, tol=1e-10)
    listed = idx.tolist()
    assert len(listed) == 36 and all(list(p) not in listed for p in special)
    assert listed[0] == [0, 0] and listed[-1] == [shape[0] - 1, shape[1] - 1]
    assert said.startswith("Fitting 36 components\n")
    check_cube(maps, omaps, idx, spread, c['nband'], f'mask edges {shape} {np.dtype(dtype).name} {kind}')


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('shape', [(37, 29), (64, 64)])
def test_negative_threshold(shape, dtype):
    """threshold = -1 admits every pixel without a NaN after the cut: empty pixels (all-zero data: NaN outputs, on the
    mask), the pixel whose beam equals pb_min in one band (fitted with data 0 and the raw beam there) and the pixel
    with a NaN beam (cut to 0 there; the raw NaN beam enters the fit: NaN outputs)."""
    c, image, beam, (nan_band, nan_beam, at_pb_min, at_threshold) = edge_cube(*shape, dtype)
    maps, said = run_cube(image, beam, c, 'tensor', threshold=-1.0, tol=1e-10)
    omaps, idx, fit, spread = oracle_cube(image, beam, c, threshold=-1.0, tol=1e-10)
    listed = idx.tolist()
    assert len(listed) == shape[0] * shape[1] - 1 and list(nan_band) not in listed
    assert said.startswith("Fitting %i components\n" % len(listed))
    k = listed.index(list(at_pb_min))
    assert np.isfinite(fit[:, k]).all() and np.isnan(fit[:, listed.index(list(nan_beam))]).all()
    assert np.isfinite(fit[0]).sum() == 38
    check_cube(maps, omaps, idx, spread, c['nband'], f'negative threshold {shape} {np.dtype(dtype).name}')
    # the fit of that pixel with the cut band's beam replaced would differ: the raw beam is what was used
    other = beam.astype(np.float64)[:, at_pb_min[0], at_pb_min[1]].copy()
    cut = np.where(other > PB_MIN, image.astype(np.float64)[:, at_pb_min[0], at_pb_min[1]], 0)
    other[1] = 1.0
    moved = sc.fit_components(cut[None], c['weights'], c['freqs'], c['ref_freq'], beam=other[None], tol=1e-10)
    assert abs(moved[0, 0] - fit[0, k]) > 1e-3


@pytest.mark.parametrize('offsets', [(1, 3), (2, 0), (0, 1)])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_cube_unaligned_bases(dtype, offsets):
    """Image and beam start 1-3 elements past a 16-byte boundary, each by its own amount."""
    if dtype == np.float64:
        offsets = tuple(o % 2 for o in offsets)
    c, image, beam, _ = edge_cube(37, 29, dtype)
    dev = []
    for a, off in zip((image, beam), offsets):
        buf = torch.zeros(a.size + 8, dtype=torch.from_numpy(a).dtype, device='cuda')
        buf[off:off + a.size] = torch.from_numpy(a).cuda().reshape(-1)
        dev.append(buf[off:off + a.size].view(a.shape))
        assert dev[-1].is_contiguous() and dev[-1].data_ptr() % 16 == off * a.itemsize
    from pfb_clean_amd.utils.spi import fit_spi
    maps = fit_spi(dev[0], dev[1], c['freqs'], c['weights'], THRESHOLD, 1, PB_MIN, 0.0, c['ref_freq'], io.StringIO(),
                   tol=1e-10)
    maps = np.stack([m.cpu().numpy() for m in maps])
    omaps, idx, _, spread = oracle_cube(image, beam, c, tol=1e-10)
    check_cube(maps, omaps, idx, spread, c['nband'], f'offsets {offsets} {np.dtype(dtype).name}')


@pytest.mark.parametrize('kind', ['numpy', 'tensor'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_empty_mask(dtype, kind):
    """The ValueError's text with a NaN maximum and with a finite one, equal to the numpy oracle's."""
    c, image, beam, (nan_band, *_) = edge_cube(37, 29, dtype)
    for with_nan in (True, False):
        if not with_nan:
            image[2][nan_band] = 0.5
        with pytest.raises(ValueError) as want:
            sc.fit_spi(image, beam, c['freqs'], c['weights'], 1024.0, PB_MIN, c['ref_freq'])
        with pytest.raises(ValueError) as got:
            run_cube(image, beam, c, kind, threshold=1024.0)
        assert str(got.value) == str(want.value)
        assert str(got.value).endswith("threshold.Max of convolved model is " + ("nan" if with_nan else
                                       "%3.2e" % np.where(beam > PB_MIN, image, 0).max()))


# ------------------------------------------------------------------------------------ more than one tile of the scan
# 259 workgroups of 4096 pixels each, one more than a 256-entry tile of the scan, so that its carry and its maximum
# across tiles are exercised: odd npix (no plane but the first on the 16-byte grid) and npix a multiple of 16 bytes
SCAN_SHAPES = [(1031, 1025), (1030, 1026)]


def scan_cube(nx, ny):
    """Case 0 (2 bands), fp32, with 36 components: the first and the last pixel, the first, one inner and the last
    pixel of workgroups 255, 256 and 257, the rest seeded.  Returns the case, the cubes and the flat pixel indices."""
    c = sc.case(0)
    npix = nx * ny
    assert (npix + 4095) // 4096 == 259
    flat = [0] + [4096 * g + o for g in (255, 256, 257) for o in (0, 1234, 4095)]
    rng = np.random.default_rng([422, nx])
    flat += [int(q) for q in rng.choice(npix, size=64, replace=False) if q not in flat][:25] + [npix - 1]
    assert len(set(flat)) == 36
    image, beam = sc.cube_of(c, nx, ny, [(q // ny, q % ny) for q in flat])
    return c, image, beam, sorted(flat)


def device_idx(image, beam, threshold):
    """(ncomps, 2) int64: what pfb_spi_mask and pfb_comps_compact make of the device cubes, as fit_spi calls them."""
    from pfb_clean_amd import _lib, _dev
    lib = _lib.load()
    nband, nx, ny = image.shape
    npix = nx * ny
    img, bm = torch.from_numpy(image).cuda(), torch.from_numpy(beam).cuda()
    work = torch.empty(lib.pfb_spi_work_bytes(npix) // 8, dtype=torch.int64, device='cuda')
    _lib.check(lib.pfb_spi_mask(_dev.code(img.dtype), _dev.ptr(img), _dev.ptr(bm), nband, npix, PB_MIN, threshold,
                                _dev.ptr(work), _dev.stream()))
    ncomps = int(work[lib.pfb_comps_work_bytes(npix) // 8 - 1].item())
    Ix, Iy = (torch.empty(ncomps, dtype=torch.int64, device='cuda') for _ in range(2))
    _lib.check(lib.pfb_comps_compact(npix, ny, _dev.ptr(work), _dev.ptr(Ix), _dev.ptr(Iy), _dev.stream()))
    return torch.stack((Ix, Iy), dim=1).cpu().numpy()


@pytest.mark.parametrize('shape', SCAN_SHAPES)
def test_scan_beyond_one_tile(shape):
    c, image, beam, flat = scan_cube(*shape)
    omaps, idx, _, spread = oracle_cube(image, beam, c, tol=1e-10)
    assert (idx[:, 0] * shape[1] + idx[:, 1]).tolist() == flat
    assert np.array_equal(device_idx(image, beam, THRESHOLD), idx)
    maps, said = run_cube(image, beam, c, 'tensor', tol=1e-10)
    assert said.startswith("Fitting 36 components\n")
    check_cube(maps, omaps, idx, spread, c['nband'], f'scan beyond one tile {shape}')


@pytest.mark.parametrize('shape', SCAN_SHAPES)
def test_empty_mask_beyond_one_tile(shape):
    """The maximum of the cut, then a NaN, in the last workgroup only: both must cross the scan's tiles."""
    c, image, beam, flat = scan_cube(*shape)
    npix = shape[0] * shape[1]
    top, bad = npix - 2, npix - 3
    assert min(top, bad) >= 4096 * 258 and top not in flat and bad not in flat
    image = image.copy()
    image[1].reshape(-1)[top] = 100.0
    cut = np.where(beam > PB_MIN, image, 0).reshape(2, -1)
    assert cut[:, :4096 * 258].max() < 100.0 == cut.max()
    for with_nan in (False, True):
        if with_nan:
            image[0].reshape(-1)[bad] = np.nan
        with pytest.raises(ValueError) as want:
            sc.fit_spi(image, beam, c['freqs'], c['weights'], 1024.0, PB_MIN, c['ref_freq'])
        with pytest.raises(ValueError) as got:
            run_cube(image, beam, c, 'tensor', threshold=1024.0)
        assert str(got.value) == str(want.value)
        assert str(got.value).endswith("threshold.Max of convolved model is " + ("nan" if with_nan else "1.00e+02"))


def test_zero_weights():
    """All-zero weights: det = 0 for every component, NaN in all four maps; the mask is what it was."""
    c, image, beam, _ = edge_cube(37, 29, np.float32)
    zero = dict(c, weights=np.zeros(c['nband']))
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        maps, said = run_cube(image, beam, zero, 'numpy')
    assert said.startswith("Fitting 36 components\n") and np.isnan(maps).all()
