#!/usr/bin/env python
"""
Golden vectors for the clean-beam fit: runs the REFERENCE's own pfb/utils/misc.py (psf_errorsq and fitcleanbeam, lines
506-584) under the stub third-party modules of _refstubs.py and stores inputs + reference outputs in beamfit.npz next to
this file.

Run in the BUILD container only:   python tests/golden/make_golden_beamfit.py
(the reference tree is absent on the GPU box; the tests only read the .npz file.)

Stubs registered here, before _refstubs.install (which only fills in what is missing):
  jax                        jit = identity; value_and_grad(f) = (f's own value, the analytic gradient below)
  jax.numpy                  the numpy functions psf_errorsq uses
  skimage.morphology.label   scipy.ndimage.label with a full 3 x 3 structure (skimage's default in 2-D is 8-connected)
jax is not installed in the build container.  The gradient that jax would derive is replaced by grad_terms(): analytic,
through Smin = min(emaj, emin) and Smaj = max(emaj, emin), with the half-and-half split that jax's documentation states
for minimum / maximum at a tie.  It is asserted against a 4th-order central difference (h = 1e-3) of the reference's
psf_errorsq to 1e-10 max|g| at every stored point that is neither a tie (where the function has a kink) nor the fitted
point (where max|g| ~ 1e-6 is below the rounding of the difference quotient).

The reference's fmin_l_bfgs_b is wrapped by a recorder: it stores the start point, the selected data and xy (hence the
fit-region count), then calls scipy's.  The lobe records (extents, counts) are recomputed here with the reference's
statements and asserted against what the recorder saw of the reference's own run.

Three groups:
  lobe{k}   crafted planes (values exact in float32): the record of every band and the start point that the
            reference handed to its optimiser, for both dtypes
  fit{k}    end-to-end cases: the reference's result per dtype and `spread`, the largest change of that result over
            seeds 1, 2, 3 when the PSF is multiplied by 1 + 2.2e-16 randn and every objective value and gradient
            component by 1 + 1e-14 randn (another summation order, another exp).  A case with spread > SPREAD_CAP is
            dropped, never the cap raised (a lobe with xdiff == ydiff starts on the tie and sits at 2e-2)
  obj{k}    objective points on the data the reference selected: f, g, sum res^2 and sum |term| per component

The float32 run is the reference given the float32 array.  Fixed zip timestamps: two runs give identical bytes.
"""
import inspect
import io
import os
import sys
import types
import zipfile

import numpy as np
import scipy.ndimage
import scipy.optimize

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import _refstubs  # noqa: E402

SPREAD_CAP = 1e-11
MAX_BYTES = 1 << 20
FWHM_CONV = 2 * np.sqrt(2 * np.log(2))
NOISE = {'rng': None}
CALLS = []


# ------------------------------------------------------------------------------------------------ the gradient
def grad_terms(x, data, xy):
    """Per-pixel terms (3, n) of the gradient of psf_errorsq and the residuals (n)."""
    emaj, emin, pa = x
    smin, smaj = np.minimum(emaj, emin), np.maximum(emaj, emin)
    t = np.deg2rad(-pa)
    c, s = np.cos(t), np.sin(t)
    u = c * xy[0] - s * xy[1]
    v = s * xy[0] + c * xy[1]
    with np.errstate(all='ignore'):
        model = np.exp(-FWHM_CONV * (u * u / smin ** 2 + v * v / smaj ** 2))
        res = data - model
        w = 2 * FWHM_CONV * res * model                     # df/dQ per pixel
        tmin = w * (-2 * u * u / smin ** 3)
        tmaj = w * (-2 * v * v / smaj ** 3)
        tpa = -(np.pi / 180) * w * 2 * u * v * (1 / smaj ** 2 - 1 / smin ** 2)
    if emaj < emin:
        terms = (tmin, tmaj, tpa)
    elif emaj > emin:
        terms = (tmaj, tmin, tpa)
    else:
        terms = (0.5 * (tmin + tmaj), 0.5 * (tmin + tmaj), tpa)
    return np.array(terms), res


def value_and_grad(fn):
    def vg(x, data, xy):
        f = np.float64(fn(x, data, xy))
        g = grad_terms(x, data, xy)[0].sum(axis=1)
        rng = NOISE['rng']
        if rng is not None:
            f = f * (1 + 1e-14 * rng.standard_normal())
            g = g * (1 + 1e-14 * rng.standard_normal(3))
        return f, g
    return vg


def label8(mask):
    return scipy.ndimage.label(mask, structure=np.ones((3, 3)))[0]


def install_stubs():
    def ident(f):
        return f
    jnp = types.ModuleType('jax.numpy')
    for name in ('minimum', 'maximum', 'array', 'cos', 'sin', 'deg2rad', 'dot', 'einsum', 'sqrt', 'log', 'exp', 'vdot'):
        setattr(jnp, name, getattr(np, name))
    jax = types.ModuleType('jax')
    jax.jit, jax.value_and_grad, jax.numpy = ident, value_and_grad, jnp
    sk = types.ModuleType('skimage')
    sk.morphology = types.ModuleType('skimage.morphology')
    sk.morphology.label = label8
    sys.modules.update({'jax': jax, 'jax.numpy': jnp, 'skimage': sk, 'skimage.morphology': sk.morphology})


install_stubs()
_refstubs.install(ROOT)

import pfb.utils.misc as refmisc  # noqa: E402

assert refmisc.label is label8 and refmisc.fmin_l_bfgs_b is scipy.optimize.fmin_l_bfgs_b


def recorder(func, x0, args=(), **kw):
    CALLS.append({'x0': np.array(x0, dtype=np.float64), 'data': args[0], 'xy': args[1], 'kw': kw})
    return scipy.optimize.fmin_l_bfgs_b(func, x0, args=args, **kw)


refmisc.fmin_l_bfgs_b = recorder


def ref_fit(psf, **kw):
    """(result (nband, 3), recorded calls by band; None for an all-zero band) of the reference's fitcleanbeam."""
    del CALLS[:]
    with np.errstate(all='ignore'):
        res = np.array(refmisc.fitcleanbeam(psf, **kw), dtype=np.float64)
    calls, it = [], iter(list(CALLS))
    for v in range(psf.shape[0]):
        calls.append(next(it) if psf[v].any() else None)
    for c in calls:
        if c is not None:
            assert c['kw'] == {'bounds': ((0, None), (0, None), (None, None)), 'factr': 1e11}
    return res, calls


def save(name, out):
    """np.savez_compressed with fixed member timestamps (bit-identical from run to run)."""
    path = os.path.join(HERE, name)
    with zipfile.ZipFile(path, 'w', compression=zipfile.ZIP_DEFLATED) as z:
        for key in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    size = os.path.getsize(path)
    assert size < MAX_BYTES, (name, size)
    print(f'{name}: {len(out)} arrays, {size} bytes')


# ------------------------------------------------------------------------------------------------- lobe records
NREC = 12       # max, any, centre_above, xmin, xmax, ymin, ymax, max|x|, max|y|, island pixels, fit pixels, extent * rsq


def record_of(plane, level, extent, connectivity=8):
    """misc.py:549-567 for one band, with the island's and the fit region's pixel counts."""
    nx, ny = plane.shape
    rec = np.zeros(NREC)
    rec[0], rec[1] = plane.max(), plane.any()
    if not rec[1]:
        return rec, None
    xx, yy = np.meshgrid(np.arange(-nx / 2, nx / 2), np.arange(-ny / 2, ny / 2), indexing='ij')
    psfv = plane / plane.max()
    mask = np.where(psfv > level, 1.0, 0)
    islands = label8(mask) if connectivity == 8 else scipy.ndimage.label(mask)[0]
    ncenter = islands[nx // 2, ny // 2]
    assert ncenter != 0
    x, y = xx[islands == ncenter], yy[islands == ncenter]
    rsq = np.abs(x).max() ** 2 + np.abs(y).max() ** 2
    idxs = xx ** 2 + yy ** 2 < extent * rsq
    rec[2:] = [1.0, x.min(), x.max(), y.min(), y.max(), np.abs(x).max(), np.abs(y).max(), x.size, idxs.sum(),
               extent * rsq]
    return rec, (islands, ncenter)


def spiral(nx, ny, hi):
    """Square spiral of width 1 from the centre, arms two pixels apart, until it reaches the border."""
    on = np.zeros((nx, ny), dtype=bool)
    i, j = nx // 2, ny // 2
    on[i, j] = True
    steps, d = 2, 0
    while True:
        for _ in range(2):
            di, dj = ((0, 1), (1, 0), (0, -1), (-1, 0))[d % 4]
            for _ in range(steps):
                i, j = i + di, j + dj
                if not (0 <= i < nx and 0 <= j < ny):
                    return on
                on[i, j] = True
            d += 1
        steps += 2


BG, HI, TOP, AT = 0.25, 1.5, 2.0, 1.0          # with max = TOP: HI / TOP = 0.75, AT / TOP = 0.5 exactly (excluded)


def lobe_cases():
    cases = []
    # 0: odd sizes (half-integer coordinates), one band: a spiral that needs ~nx sweeps, reaches the border, its
    # maximum at the centre; a detached island in the corner
    p = np.full((37, 29), BG)
    p[spiral(37, 29, HI)] = HI
    p[18, 14] = TOP
    p[34:37, 0:2] = HI
    cases.append(('spiral', p[None], 0.5, 15.0))
    # 1: even sizes, three bands with an all-zero band in the middle
    a = np.full((64, 48), BG)
    a[30:35, 22:27] = HI                        # the block around the centre (32, 24)
    a[35:38, 27:30] = HI                        # joined to it by the diagonal (34, 26) - (35, 27) only
    a[29, 24] = AT                              # exactly at the level, next to the block: excluded
    a[5:8, 5:10] = HI                           # detached island, which also holds the maximum
    a[6, 6] = TOP
    c = np.full((64, 48), BG)
    c[0:41, 20] = HI                            # a U from the border, the centre on a stub of its left arm
    c[40, 20:29] = HI
    c[10:41, 28] = HI
    c[32, 20:25] = HI
    c[0, 20] = TOP
    cases.append(('blocks_zero_u', np.stack([a, np.zeros_like(a), c]), 0.5, 15.0))
    # 2: 2049 x 33: several workgroups of the max pass; npix is odd, so planes 1 and 2 start off a 16-byte boundary.
    # The maxima sit in the first vector, in the last (loose) elements and in the loose head
    b = np.full((3, 2049, 33), BG)
    b[0, 1022:1027, 15:18] = HI
    b[0, 0, 0] = TOP
    b[1, 1023:1026, 13:20] = HI
    b[1, 2048, 32] = TOP
    b[2, 1020:1029, 14:19] = HI
    b[2, 0, 1] = TOP
    cases.append(('tall', b, 0.5, 15.0))
    # 3: odd sizes in float64 planes that start off a 16-byte boundary (1073 pixels), another level and extent
    d = np.full((3, 37, 29), BG)
    d[0, 16:21, 12:17] = HI
    d[0, 36, 28] = TOP
    d[2, 15:22, 13:16] = HI
    d[2, 22, 16] = HI                           # diagonal-only pixel
    d[2, 14, 14] = 0.75                         # at the level 0.375 of the maximum 2.0
    d[2, 0, 0] = TOP
    d[1] = 0.0
    cases.append(('odd3', d, 0.375, 4.0))
    return cases


def gen_lobes(out):
    names, any_conn, any_second = [], False, False
    for k, (name, cube, level, extent) in enumerate(lobe_cases()):
        cube32 = cube.astype(np.float32)
        assert np.array_equal(cube32.astype(np.float64), cube)
        out[f'lobe{k}_psf'], out[f'lobe{k}_level'], out[f'lobe{k}_extent'] = cube32, np.array(level), np.array(extent)
        conn, second = False, False
        for bits, arr in ((32, cube32), (64, cube)):
            _, calls = ref_fit(arr, level=level, extent=extent)
            recs = np.zeros((cube.shape[0], NREC))
            x0s = np.full((cube.shape[0], 3), np.nan)
            for v in range(cube.shape[0]):
                recs[v], lab = record_of(arr[v], level, extent)
                if lab is None:
                    assert calls[v] is None
                    continue
                # what the reference's own run shows of its extents and its fit region
                xd, yd = recs[v, 4] - recs[v, 3], recs[v, 6] - recs[v, 5]
                assert np.array_equal(calls[v]['x0'], [max(xd, yd), min(xd, yd), 0.0]), (name, v)
                assert calls[v]['xy'].shape == (2, int(recs[v, 10])) and calls[v]['data'].dtype == arr.dtype
                assert min(xd, yd) >= 2
                x0s[v] = calls[v]['x0']
                conn |= not np.array_equal(record_of(arr[v], level, extent, connectivity=4)[0][3:9], recs[v, 3:9])
                second |= len(set(np.unique(lab[0])) - {0, lab[1]}) > 0
            out[f'lobe{k}_rec{bits}'], out[f'lobe{k}_x0_{bits}'] = recs, x0s
        assert np.array_equal(out[f'lobe{k}_rec32'], out[f'lobe{k}_rec64'])
        out[f'lobe{k}_conn_differs'], out[f'lobe{k}_second_island'] = np.array(conn), np.array(second)
        print(f'  lobe{k} {name} {cube.shape}: 4- and 8-connected extents differ {conn}, second island {second}')
        any_conn |= conn
        any_second |= second
        names.append(name)
    assert any_conn and any_second
    out['lobe_names'] = np.array(names)


# -------------------------------------------------------------------------------------------------- end to end
def beam(nx, ny, emaj, emin, pa):
    xx, yy = np.meshgrid(np.arange(-nx / 2, nx / 2), np.arange(-ny / 2, ny / 2), indexing='ij')
    xy = np.vstack((xx.ravel(), yy.ravel()))
    terms, res = grad_terms((emaj, emin, pa), 0.0, xy)
    return (-res).reshape(nx, ny), np.sqrt(xx ** 2 + yy ** 2)


def psf_like(rng, nx, ny, emaj, emin, pa):
    """A Gaussian main lobe with 8 % of a decaying ripple (sidelobes) and 1e-3 of noise: like a real PSF it is not of the
    model's form, so the residuals at the fitted point are at the per cent level."""
    g, r = beam(nx, ny, emaj, emin, pa)
    return 0.92 * g + 0.08 * np.cos(0.9 * r / emin) * np.exp(-r / (4 * emaj)) + 1e-3 * rng.standard_normal((nx, ny))


# (nx, ny, [(emaj, emin, pa) or None for an all-zero band])
FIT_CASES = [
    (64, 48, [(6.0, 3.5, 30.0), None, (7.0, 3.0, -20.0)]),
    (128, 128, [(12.0, 4.0, 100.0)]),
    (96, 80, [(9.0, 7.0, 75.0)]),
]
ROUND = (48, 48, (5.0, 5.0, 0.0))               # xdiff == ydiff: compared at the objective level only


def spread_of(psf, ref):
    worst = 0.0
    good = np.isfinite(ref)
    for seed in (1, 2, 3):
        rng = np.random.default_rng(seed)
        jit = (psf.astype(np.float64) * (1.0 + 2.2e-16 * rng.standard_normal(psf.shape))).astype(psf.dtype)
        NOISE['rng'] = rng
        try:
            got = ref_fit(jit)[0]
        finally:
            NOISE['rng'] = None
        assert np.array_equal(np.isfinite(got), good)
        worst = max(worst, np.abs(got - ref)[good].max())
    return worst


def fd_gradient(x, data, xy, h=1e-3):
    g = np.zeros(3)
    for k in range(3):
        e = np.zeros(3)
        e[k] = h
        f = [np.float64(refmisc.psf_errorsq(np.asarray(x) + m * e, data, xy)) for m in (-2, -1, 1, 2)]
        g[k] = (f[0] - 8 * f[1] + 8 * f[2] - f[3]) / (12 * h)
    return g


def put_objective(out, tag, bits, call, points, kinds):
    """points (npts, 3) on the data / xy that the reference selected; kinds: 'fd' points are asserted against the
    central difference."""
    data, xy = call['data'], call['xy']
    f, g, gabs = [], [], []
    for x, kind in zip(points, kinds):
        terms, res = grad_terms(x, data, xy)
        val = np.float64(refmisc.psf_errorsq(np.asarray(x), data, xy))
        grad = terms.sum(axis=1)
        if kind == 'fd':
            err = np.abs(fd_gradient(x, data, xy) - grad).max() / np.abs(grad).max()
            print(f'    {tag} fp{bits} x = {np.round(x, 3)}: analytic against central difference {err:.1e}')
            assert err <= 1e-10, (tag, x, err)
        f.append(val)
        g.append(grad)
        gabs.append(np.abs(terms).sum(axis=1))
        assert abs((res * res).sum() - val) <= 1e-13 * val
    out[f'{tag}_pts{bits}'], out[f'{tag}_f{bits}'] = np.array(points), np.array(f)
    out[f'{tag}_g{bits}'], out[f'{tag}_gabs{bits}'] = np.array(g), np.array(gabs)
    out[f'{tag}_n{bits}'] = np.array(xy.shape[1])


def gen_fits(out, rng):
    nfit = nobj = 0
    for nx, ny, bands in FIT_CASES:
        psf = np.stack([np.zeros((nx, ny)) if b is None else psf_like(rng, nx, ny, *b) for b in bands])
        keep, per = True, {}
        for bits, arr in ((64, psf), (32, psf.astype(np.float32))):
            ref, calls = ref_fit(arr)
            for v, c in enumerate(calls):
                assert c is None or (c['x0'][0] != c['x0'][1] and c['x0'][1] >= 3), (nx, ny, v, c['x0'])
            sp = spread_of(arr, ref)
            print(f'  fit ({len(bands)}, {nx}, {ny}) fp{bits}: {np.round(ref, 4).tolist()} spread {sp:.1e}')
            keep &= sp <= SPREAD_CAP
            per[bits] = (ref, calls, sp)
        if not keep:
            print('    dropped: spread above the cap')
            continue
        tag = f'fit{nfit}'
        out[tag + '_psf'] = psf
        for bits, (ref, calls, sp) in per.items():
            out[f'{tag}_ref{bits}'], out[f'{tag}_spread{bits}'] = ref, np.array(sp)
        for v, b in enumerate(bands):
            if b is None:
                continue
            otag = f'obj{nobj}'
            out[otag + '_psfkey'], out[otag + '_band'] = np.array(tag + '_psf'), np.array(v)
            for bits, (ref, calls, sp) in per.items():
                p, x0 = ref[v], calls[v]['x0']
                tie = 0.5 * (p[0] + p[1])
                points = [p, x0, (0.7 * p[1], 1.3 * p[0], p[2] + 10.0), (tie, tie, 12.0)]
                put_objective(out, otag, bits, calls[v], points, ['fitted', 'fd', 'fd', 'tie'])
            nobj += 1
        nfit += 1
    assert nfit >= 3
    # the round lobe: its start point is the tie
    nx, ny, b = ROUND
    psf = psf_like(rng, nx, ny, *b)[None]
    otag = f'obj{nobj}'
    out['round_psf'], out[otag + '_psfkey'], out[otag + '_band'] = psf, np.array('round_psf'), np.array(0)
    for bits, arr in ((64, psf), (32, psf.astype(np.float32))):
        ref, calls = ref_fit(arr)
        x0 = calls[0]['x0']
        assert x0[0] == x0[1]
        points = [x0, (x0[0], 0.8 * x0[0], 25.0), (0.6 * x0[0], x0[0], -40.0), (x0[0], x0[0], 33.0)]
        put_objective(out, otag, bits, calls[0], points, ['tie', 'fd', 'fd', 'tie'])
    out['nfit'], out['nobj'], out['nlobe'] = np.array(nfit), np.array(nobj + 1), np.array(len(out['lobe_names']))
    out['spread_cap'] = np.array(SPREAD_CAP)


if __name__ == '__main__':
    sig = inspect.signature(refmisc.fitcleanbeam).parameters
    out = {'sig_fitcleanbeam': np.array(list(sig)),
           'sig_defaults': np.array([sig[k].default for k in ('level', 'pixsize', 'extent')])}
    gen_lobes(out)
    gen_fits(out, np.random.default_rng(420))
    save('beamfit.npz', out)
