"""
The w-gridder's contract, a numpy model of its recipe, and the case table of test_cpu_wgrid.py / test_gpu_wgrid.py.

direct_vis2dirty / direct_dirty2vis   the operators' definition (include/pfb_hip.h, "w-gridder"): the direct Fourier
                                      sums in fp64, vectorised over pixels.  THE reference of every accuracy test.
model_vis2dirty / model_dirty2vis     the recipe of DESIGN 4.10 in plain numpy fp64: w-stacking on a (2 nx, 2 ny) grid,
                                      kernel exp(2.3 W (sqrt(1 - x^2) - 1)), W = ceil(log10(1/eps)) + 2.  It shows on
                                      the CPU that the recipe meets epsilon on every case, which is what makes the GPU
                                      bound meaningful, and gives the adjointness mismatch the GPU is compared with.
CASES                                 the table: every case is a dict of inputs and tags (`edges`).
"""
import math

import numpy as np

C_LIGHT = 299792458.0
IMAGES = {'32x24': (32, 24, 0.012, 0.03), '48x16': (48, 16, 0.012, 0.03), '16x64': (16, 64, 0.03, 0.008),
          # npix % 256 != 0, nx / 2 and ny / 2 odd; 6x8 and 10x6: a grid as narrow as the footprint of W = 12
          '34x26': (34, 26, 0.012, 0.03), '6x8': (6, 8, 0.05, 0.04), '10x6': (10, 6, 0.05, 0.06)}


# ------------------------------------------------------------------------------------------------- the contract
def coords(case):
    """(u, v, w), each (nrow, nchan): uvw[r] * freq[k] / c."""
    uvw, freq = case['uvw'], case['freq']
    return tuple(uvw[:, a:a + 1] * freq[None, :] / C_LIGHT for a in range(3))


def lmn(case):
    nx, ny = case['nx'], case['ny']
    l = ((np.arange(nx) - nx // 2) * case['px'] + case['cx'])[:, None]
    m = ((np.arange(ny) - ny // 2) * case['py'] + case['cy'])[None, :]
    r2 = l * l + m * m
    nm1 = -r2 / (1.0 + np.sqrt(1.0 - r2))
    if not case['do_wgridding']:
        nm1 = np.zeros_like(nm1)
    return l, m, nm1


def _phases(case):
    """exp(+2 pi i phase) as (nvis, nx, ny), and the mask as (nvis,) bool."""
    u, v, w = (a.reshape(-1) for a in coords(case))
    l, m, nm1 = lmn(case)
    ph = u[:, None, None] * l[None] + v[:, None, None] * m[None] - w[:, None, None] * nm1[None]
    nvis = u.size
    mask = np.ones(nvis, bool) if case['mask'] is None else case['mask'].reshape(-1) != 0
    return np.exp(2j * np.pi * ph), mask, (1.0 / (1.0 + nm1) if case['divide_by_n'] else np.ones_like(nm1))


def direct_vis2dirty(case, vis, wgt='case'):
    E, mask, f = _phases(case)
    wgt = case['wgt'] if isinstance(wgt, str) else wgt
    val = vis.reshape(-1).astype(np.complex128) * (1.0 if wgt is None else wgt.reshape(-1).astype(np.float64))
    return f * np.einsum('v,vij->ij', val * mask, E).real


def direct_dirty2vis(case, dirty, wgt='case'):
    E, mask, f = _phases(case)
    wgt = case['wgt'] if isinstance(wgt, str) else wgt
    vis = np.einsum('ij,vij->v', f * dirty.astype(np.float64), E.conj())
    vis = vis * (1.0 if wgt is None else wgt.reshape(-1).astype(np.float64)) * mask
    return vis.reshape(case['uvw'].shape[0], case['freq'].size)


def direct_hessian(case, x, beam):
    """beam * vis2dirty(wgt * dirty2vis(beam * x)), divide_by_n=False both ways (the case's flag is ignored)."""
    c = dict(case, divide_by_n=False)
    b = 1.0 if beam is None else beam
    return b * direct_vis2dirty(c, direct_dirty2vis(c, b * x, wgt=None))


def rel_l2(a, b):
    return np.linalg.norm((a - b).ravel()) / np.linalg.norm(np.asarray(b).ravel())


# ---------------------------------------------------------------------------------------------- the numpy model
def support(eps):
    return int(math.ceil(-math.log10(eps) - 1e-9)) + 2


def phi(x, W):
    q = 1.0 - x * x
    return np.where(q > 0, np.exp(2.3 * W * (np.sqrt(np.maximum(q, 0.0)) - 1.0)), 0.0)


def correction(W, t, nodes=128):
    """h int phi(x) cos(2 pi h t x) dx by Gauss-Legendre in theta, x = sin(theta)."""
    th, wq = np.polynomial.legendre.leggauss(nodes)
    th, wq = th * (np.pi / 2), wq * (np.pi / 2)
    f = np.exp(2.3 * W * (np.cos(th) - 1.0)) * np.cos(th) * wq
    return 0.5 * W * (np.cos(np.pi * W * np.asarray(t, float)[..., None] * np.sin(th)) * f).sum(-1)


def correction_brute(W, t, n=400001):
    """The same integral by the trapezoid rule in x on a dense grid (the integrand vanishes to e^(-2.3 W) at the ends)."""
    x = np.linspace(-1.0, 1.0, n)
    y = phi(x, W) * np.cos(np.pi * W * t * x)
    y[0] = y[-1] = math.exp(-2.3 * W) * math.cos(np.pi * W * t)
    return 0.5 * W * (y.sum() - 0.5 * (y[0] + y[-1])) * (x[1] - x[0])


def planes(case):
    """(nplanes, w0, dw) over the unmasked visibilities; None when there are none."""
    w = coords(case)[2]
    if case['mask'] is not None:
        w = w[case['mask'] != 0]
    if w.size == 0:
        return None
    W = support(case['eps'])
    wmin, wmax = w.min(), w.max()
    max_nm1 = np.abs(lmn(case)[2]).max()
    if not case['do_wgridding']:
        return 1, 0.0, 1.0
    if math.pi * max_nm1 * (wmax - wmin) <= 0.01 * case['eps']:
        return 1, 0.5 * (wmin + wmax), 1.0
    dw = 1.0 / (4.0 * max_nm1)
    return int(math.ceil((wmax - wmin) / dw)) + W + 1, wmin - 0.5 * W * dw, dw


def _setup(case):
    nx, ny, W = case['nx'], case['ny'], support(case['eps'])
    Nu, Nv, h = 2 * nx, 2 * ny, 0.5 * W
    u, v, w = (a.reshape(-1) for a in coords(case))
    sel = np.arange(u.size) if case['mask'] is None else np.flatnonzero(case['mask'].reshape(-1))
    u, v, w = u[sel], v[sel], w[sel]
    nplanes, w0, dw = planes(case)
    ug, vg = u * (case['px'] * Nu), v * (case['py'] * Nv)
    a0, b0 = np.ceil(ug - h), np.ceil(vg - h)
    k = np.arange(W)
    fu, fv = phi((a0[:, None] + k - ug[:, None]) / h, W), phi((b0[:, None] + k - vg[:, None]) / h, W)
    rows = (a0[:, None] + k).astype(np.int64) % Nu
    cols = (b0[:, None] + k).astype(np.int64) % Nv
    _, _, nm1 = lmn(case)
    cu = correction(W, (np.arange(nx) - nx // 2) / Nu)
    cv = correction(W, (np.arange(ny) - ny // 2) / Nv)
    cw = correction(W, dw * nm1) if nplanes > 1 else 1.0
    corr = 1.0 / (cu[:, None] * cv[None, :] * cw)
    if case['divide_by_n']:
        corr = corr / (1.0 + nm1)
    centre = np.exp(2j * np.pi * (u * case['cx'] + v * case['cy']))
    gi = (np.arange(nx) - nx // 2) % Nu
    gj = (np.arange(ny) - ny // 2) % Nv
    return dict(W=W, h=h, Nu=Nu, Nv=Nv, sel=sel, nplanes=nplanes, w0=w0, dw=dw, pg=(w - w0) / dw, fu=fu, fv=fv,
                rows=rows, cols=cols, nm1=nm1, corr=corr, centre=centre, gi=gi, gj=gj)


def _wweights(s, p):
    return phi((p - s['pg']) / s['h'], s['W']) if s['nplanes'] > 1 else np.ones_like(s['pg'])


def model_vis2dirty(case, vis):
    nx, ny = case['nx'], case['ny']
    if planes(case) is None:
        return np.zeros((nx, ny))
    s = _setup(case)
    val = vis.reshape(-1).astype(np.complex128)[s['sel']]
    if case['wgt'] is not None:
        val = val * case['wgt'].reshape(-1).astype(np.float64)[s['sel']]
    val = val * s['centre']
    img = np.zeros((nx, ny), complex)
    for p in range(s['nplanes']):
        ww = _wweights(s, p)
        if not ww.any():
            continue
        grid = np.zeros((s['Nu'], s['Nv']), complex)
        contrib = (val * ww)[:, None, None] * s['fu'][:, :, None] * s['fv'][:, None, :]
        np.add.at(grid, (s['rows'][:, :, None], s['cols'][:, None, :]), contrib)
        F = np.fft.ifft2(grid, norm='forward')
        img += F[np.ix_(s['gi'], s['gj'])] * np.exp(-2j * np.pi * (s['w0'] + p * s['dw']) * s['nm1'])
    return img.real * s['corr']


def model_dirty2vis(case, dirty):
    nrow, nchan = case['uvw'].shape[0], case['freq'].size
    out = np.zeros(nrow * nchan, complex)
    if planes(case) is None:
        return out.reshape(nrow, nchan)
    s = _setup(case)
    acc = np.zeros(s['sel'].size, complex)
    for p in range(s['nplanes']):
        ww = _wweights(s, p)
        if not ww.any():
            continue
        grid = np.zeros((s['Nu'], s['Nv']), complex)
        grid[np.ix_(s['gi'], s['gj'])] = dirty * s['corr'] * np.exp(2j * np.pi * (s['w0'] + p * s['dw']) * s['nm1'])
        F = np.fft.fft2(grid)
        foot = F[s['rows'][:, :, None], s['cols'][:, None, :]]
        acc += ww * np.einsum('vab,va,vb->v', foot, s['fu'], s['fv'])
    acc = acc * s['centre'].conj()
    if case['wgt'] is not None:
        acc = acc * case['wgt'].reshape(-1).astype(np.float64)[s['sel']]
    out[s['sel']] = acc
    return out.reshape(nrow, nchan)


ADJOINT_SEEDS = (7, 8, 9, 10)
HALF_ULP = 2.0 ** -53


def adjoint_mismatch(v2d, d2v, case, seeds=ADJOINT_SEEDS):
    """max over the seeds of |Re<v, d2v(d)> - <v2d(v), d>| / |Re<v, d2v(d)>| for random v, d in fp64 (wgt and mask as
    the case has them).  The two products are fp64 numbers: a mismatch below HALF_ULP cannot be told from zero."""
    worst = 0.0
    nrow, nchan = case['uvw'].shape[0], case['freq'].size
    for seed in seeds:
        rng = np.random.default_rng(seed)
        v = rng.standard_normal((nrow, nchan)) + 1j * rng.standard_normal((nrow, nchan))
        d = rng.standard_normal((case['nx'], case['ny']))
        lhs = np.vdot(v, d2v(d)).real
        rhs = np.vdot(v2d(v), d).real
        worst = max(worst, abs(lhs - rhs) / abs(lhs))
    return worst


# --------------------------------------------------------------------------------------------------- the table
def _delta_w(image, cx=0.0, cy=0.0):
    c = dict(zip(('nx', 'ny', 'px', 'py'), IMAGES[image]), cx=cx, cy=cy, do_wgridding=True)
    return 1.0 / (4.0 * np.abs(lmn(c)[2]).max())


def make_case(name, image, eps, seed, nrow=257, nchan=1, wmax=20.0, wgt=False, mask=None, cx=0.0, cy=0.0,
              divide_by_n=True, do_wgridding=True, dtype='f64', wsign=0, uvfrac=0.96, edges=(), uvw_wl=None,
              freq=None):
    """Random visibilities with |u| <= uvfrac * 0.5 / pixsize and |w| <= wmax wavelengths at the top channel (w >= 0
    with wsign=1), unless `uvw_wl` gives (u, v, w) in wavelengths of a single channel at frequency c."""
    nx, ny, px, py = IMAGES[image]
    rng = np.random.default_rng(seed)
    if uvw_wl is not None:
        uvw = np.asarray(uvw_wl, dtype=np.float64).reshape(-1, 3)
        freq = np.array([C_LIGHT])
        nrow, nchan = uvw.shape[0], 1
    else:
        freq = 1.0e9 * (1.0 + 0.02 * np.arange(nchan)) if freq is None else np.asarray(freq, float)
        lam = C_LIGHT / freq.max()
        lo = 0.0 if wsign else -1.0
        uvw = np.stack([rng.uniform(-1, 1, nrow) * uvfrac * 0.5 / px, rng.uniform(-1, 1, nrow) * uvfrac * 0.5 / py,
                        rng.uniform(lo, 1, nrow) * wmax], axis=1) * lam
    case = dict(name=name, image=image, nx=nx, ny=ny, px=px, py=py, cx=cx, cy=cy, eps=eps, dtype=dtype,
                divide_by_n=divide_by_n, do_wgridding=do_wgridding, uvw=np.ascontiguousarray(uvw), freq=freq,
                edges=tuple(edges), seed=seed)
    rdt = np.float32 if dtype == 'f32' else np.float64
    case['wgt'] = rng.uniform(0.5, 1.5, (nrow, nchan)).astype(rdt) if wgt else None
    if mask == 'partial':
        case['mask'] = (rng.uniform(size=(nrow, nchan)) < 0.7).astype(np.uint8)
    elif mask == 'bool':
        case['mask'] = rng.uniform(size=(nrow, nchan)) < 0.7
    elif mask == 'zero':
        case['mask'] = np.zeros((nrow, nchan), np.uint8)
    else:
        case['mask'] = None
    cdt = np.complex64 if dtype == 'f32' else np.complex128
    case['vis'] = (rng.standard_normal((nrow, nchan)) + 1j * rng.standard_normal((nrow, nchan))).astype(cdt)
    case['dirty'] = rng.standard_normal((nx, ny)).astype(rdt)
    return case


def _exact_cells(image, axis, offsets, want_frac):
    """u (axis 0) or v (axis 1) in wavelengths whose grid coordinate, computed as the operators compute it at frequency
    c, has EXACTLY the fractional part want_frac (0 or 0.5)."""
    nx, ny, px, py = IMAGES[image]
    scale = (px * 2 * nx) if axis == 0 else (py * 2 * ny)
    out = []
    for a in offsets:
        x = (a + want_frac) / scale
        g = (x * C_LIGHT / C_LIGHT) * scale
        if g - math.floor(g) == want_frac:
            out.append(x)
    return out


def _build():
    cases = []
    add = cases.append
    # ---- image x epsilon (fp64); |w| range, row / channel counts, weights and masks rotate through them
    rows = [(257, 1), (63, 3), (65, 3), (85, 3)]
    wmaxs = [20.0, 60.0, 200.0]
    k = 0
    for image in ('32x24', '48x16', '16x64'):
        for eps in (1e-3, 1e-5, 1e-7, 1e-9):
            nrow, nchan = rows[k % 4]
            add(make_case(f'{image}-eps{eps:g}', image, eps, 100 + k, nrow=nrow, nchan=nchan, wmax=wmaxs[k % 3],
                          wgt=k % 2 == 0, mask=(None, 'partial', 'bool')[k % 3], uvfrac=1.0 if k % 5 == 0 else 0.96))
            k += 1
    # ---- fp32
    for image, eps in (('32x24', 1e-3), ('16x64', 1e-3), ('32x24', 1e-4), ('48x16', 1e-4)):
        add(make_case(f'{image}-f32-eps{eps:g}', image, eps, 200 + k, nrow=85, nchan=3, wmax=60.0, wgt=True,
                      mask='partial', dtype='f32'))
        k += 1
    # ---- row counts 1 (one and three channels), all-zero mask, no weights and no mask
    add(make_case('one-row', '32x24', 1e-5, 301, nrow=1, nchan=1, edges=('nrow1',)))
    add(make_case('one-row-3chan', '32x24', 1e-5, 302, nrow=1, nchan=3, wgt=True, edges=('nrow1',)))
    add(make_case('mask-zero', '32x24', 1e-5, 303, nrow=63, nchan=3, wgt=True, mask='zero', edges=('mask0',)))
    # ---- centre, divide_by_n
    add(make_case('centre', '32x24', 1e-7, 304, wmax=60.0, cx=0.05, cy=-0.08, wgt=True, edges=('centre',)))
    add(make_case('centre-no-n', '16x64', 1e-5, 305, nrow=65, nchan=3, cx=-0.1, cy=0.03, divide_by_n=False,
                  edges=('centre', 'no_n')))
    add(make_case('no-n', '48x16', 1e-7, 306, wmax=60.0, divide_by_n=False, mask='partial', edges=('no_n',)))
    # ---- do_wgridding off; on with one w; on with w of one sign
    add(make_case('no-wgrid', '32x24', 1e-7, 307, do_wgridding=False, wgt=True, edges=('wgrid_off',)))
    c = make_case('one-w', '48x16', 1e-7, 308, wmax=60.0, edges=('wmin_eq_wmax',))
    c['uvw'][:, 2] = 37.5 * C_LIGHT / c['freq'][0]
    add(c)
    add(make_case('w-positive', '16x64', 1e-5, 309, wmax=200.0, wsign=1, wgt=True, edges=('w_one_sign',)))
    # ---- placement edges
    rng = np.random.default_rng(400)
    nx, ny, px, py = IMAGES['32x24']
    n = 250
    u = rng.uniform(-0.5 / px, 0.5 / px, n)
    v = rng.uniform(-0.5 / py, 0.5 / py, n)
    w = rng.uniform(-20, 20, n)
    ue, ve = u.copy(), v.copy()
    ue[:60] = np.where(np.arange(60) % 2, 0.5 / px, -0.5 / px)                       # exactly on the seam
    ue[60:120] = np.where(np.arange(60) % 2, 1, -1) * (0.5 / px) * (1 - 1e-12)       # just inside
    ve[120:180] = np.where(np.arange(60) % 2, 0.5 / py, -0.5 / py)
    ve[180:240] = np.where(np.arange(60) % 2, 1, -1) * (0.5 / py) * (1 - 1e-12)
    add(make_case('seam', '32x24', 1e-7, 401, uvw_wl=np.stack([ue, ve, w], 1), edges=('seam_exact', 'seam_inside')))
    for eps, tag in ((1e-6, 'even'), (1e-7, 'odd')):                                 # W = 8 and W = 9: both tie kinds
        ui = _exact_cells('32x24', 0, range(-30, 31), 0.0) + _exact_cells('32x24', 0, range(-30, 30), 0.5)
        vi = _exact_cells('32x24', 1, range(-22, 23), 0.0) + _exact_cells('32x24', 1, range(-22, 22), 0.5)
        uu, vv = rng.choice(ui, n), rng.choice(vi, n)
        add(make_case(f'ties-{tag}', '32x24', eps, 402, uvw_wl=np.stack([uu, vv, w], 1),
                      edges=('ug_integer', 'ug_half')))
    z = np.stack([u, v, w], 1)
    z[:5] = 0.0
    add(make_case('origin', '32x24', 1e-7, 403, uvw_wl=z, edges=('uvw_zero',)))
    one = np.stack([np.full(n, 7.3 / (px * 2 * nx)) + rng.uniform(-0.2, 0.2, n) / (px * 2 * nx),
                    np.full(n, -5.6 / (py * 2 * ny)) + rng.uniform(-0.2, 0.2, n) / (py * 2 * ny),
                    np.full(n, 3.0)], 1)
    add(make_case('one-cell', '32x24', 1e-7, 404, uvw_wl=one, wgt=True, edges=('one_cell',)))
    dw = _delta_w('32x24')
    for eps, tag in ((1e-6, 'even'), (1e-7, 'odd')):
        j = rng.integers(0, 12, n)
        wp = -15.0 + (j + np.where(np.arange(n) % 2, 0.5, 0.0)) * dw
        wp[0] = -15.0                                                                  # wmin itself
        add(make_case(f'w-planes-{tag}', '32x24', eps, 405, uvw_wl=np.stack([u, v, wp], 1),
                      edges=('w_on_plane', 'w_half_plane')))
    # ---- the supports no case above launches (W = 4, 10, 12), on images of npix % 256 != 0 and on grids of W cells
    for j, (image, eps) in enumerate((('34x26', 1e-2), ('34x26', 1e-8), ('34x26', 1e-10), ('6x8', 1e-2), ('6x8', 1e-10),
                                      ('10x6', 1e-10))):
        add(make_case(f'{image}-eps{eps:g}', image, eps, 500 + j, wgt=True, mask='partial',
                      edges=('partial_block',) + (('grid_eq_support',) if image != '34x26' and eps == 1e-10 else ())))
    return cases


CASES = _build()
CASE_IDS = [c['name'] for c in CASES]
F64_CASES = [c for c in CASES if c['dtype'] == 'f64']


def as_f32(case):
    """The case with its data in single precision (coordinates stay fp64)."""
    c = dict(case, dtype='f32', vis=case['vis'].astype(np.complex64), dirty=case['dirty'].astype(np.float32))
    c['wgt'] = None if case['wgt'] is None else case['wgt'].astype(np.float32)
    return c
