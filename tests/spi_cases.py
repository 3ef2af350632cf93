"""
Oracles and seeded cases of the spectral-index fit (tests/test_cpu_spi.py, tests/test_gpu_spi.py).

fit_components   the per-component definition (include/pfb_hip.h, "spectral index"): Gauss-Newton on (alpha, I0) of
                 m_b = I0 B_b x_b^alpha, the model written as x ** alpha, every band sum accumulated band by band in
                 ascending order, float64 throughout.  Vectorised over the components; every component keeps its own
                 step count.
fit_spi          the image side in numpy: beam cut, amin over the bands against the threshold, np.argwhere's order,
                 the ValueError of an empty mask, NaN maps of the image's dtype filled at the components.
make_case        seeded inputs: power laws with alpha in [-2, 1], I0 in [1e-3, 10] (log-uniform), beam values in
                 [0.3, 1], band weights in [0.5, 2] and multiplicative Gaussian noise; every datum and beam value is
                 exactly a float32 value.
spread, rho      per case: how far the oracle's own outputs move when every datum moves 1 ulp (of float64) upward, and
                 the largest ratio of successive step sizes over the last steps of a component.

CASES is the stored table.  The CPU module asserts on every entry: spread <= 1e-11, rho <= 0.5 and every component
converged before maxiter.  For nband = 2 the fit interpolates, chi2 is rounding noise and the two errors are noise
over noise: there only alpha and I0 are held to the spread bound.

Plain numpy: no torch and no GPU.
"""
import numpy as np

OUTPUTS = ('alpha', 'alpha_err', 'I0', 'I0_err')
EMPTY_MASK = ("No components found above threshold. Try lowering your threshold."
              "Max of convolved model is %3.2e")

# (nband, ncomps, noise, seed)
CASES = [(2, 65, 0.01, 1), (3, 65, 0.10, 2), (4, 257, 0.01, 3), (8, 300, 0.10, 4), (63, 64, 0.10, 5),
         (64, 63, 0.01, 6)]


# --------------------------------------------------------------------------------------------------- the fit
def _normal(d, B, w, lnx, x, alpha, I0):
    """(h00, h01, h11, g0, g1, chi2) of the components in d (n, nband) at (alpha, I0), bands in ascending order."""
    n, nband = d.shape
    h00, h01, h11, g0, g1, chi2 = (np.zeros(n) for _ in range(6))
    for b in range(nband):
        j1 = B[:, b] * x[b] ** alpha
        j0 = I0 * j1 * lnx[b]
        r = d[:, b] - I0 * j1
        h00 += w[b] * j0 * j0
        h01 += w[b] * j0 * j1
        h11 += w[b] * j1 * j1
        g0 += w[b] * j0 * r
        g1 += w[b] * j1 * r
        chi2 += w[b] * r * r
    return h00, h01, h11, g0, g1, chi2


def fit_components(data, weights, freqs, freq0, alphai=None, I0i=None, beam=None, tol=1e-5, maxiter=100, info=False):
    """(4, ncomps) float64: alpha, alpha_err, I0, I0_err.  With info=True also a dict: 'steps' (ncomps) steps taken,
    'late' the number of components that took maxiter steps, 'eps' (ncomps, max steps) the step sizes (NaN behind a
    component's last step)."""
    d = np.array(data, dtype=np.float64)
    ncomps, nband = d.shape
    w = np.asarray(weights, dtype=np.float64)
    freqs = np.asarray(freqs, dtype=np.float64)
    x = freqs / freq0
    lnx = np.log(x)
    ref = int(np.argmin(np.abs(freqs - freq0)))
    B = np.ones_like(d) if beam is None else np.array(beam, dtype=np.float64)
    alpha = np.full(ncomps, -0.7) if alphai is None else np.array(alphai, dtype=np.float64)
    I0 = d[:, ref].copy() if I0i is None else np.array(I0i, dtype=np.float64)
    eps = np.ones(ncomps)
    steps = np.zeros(ncomps, dtype=np.int64)
    dead = np.zeros(ncomps, dtype=bool)
    hist = []
    with np.errstate(all='ignore'):
        while True:
            act = np.flatnonzero(~dead & (eps > tol) & (steps < maxiter))
            if not act.size:
                break
            h00, h01, h11, g0, g1, _ = _normal(d[act], B[act], w, lnx, x, alpha[act], I0[act])
            det = h00 * h11 - h01 * h01
            bad = ~np.isfinite(det) | (det == 0)
            dead[act[bad]] = True
            act, ok = act[~bad], ~bad
            da = (h11[ok] * g0[ok] - h01[ok] * g1[ok]) / det[ok]
            di = (-h01[ok] * g0[ok] + h00[ok] * g1[ok]) / det[ok]
            alpha[act] += da
            I0[act] += di
            eps[act] = np.maximum(np.abs(da), np.abs(di))
            steps[act] += 1
            e = np.full(ncomps, np.nan)
            e[act] = eps[act]
            hist.append(e)
        h00, h01, h11, _, _, chi2 = _normal(d, B, w, lnx, x, alpha, I0)
        det = h00 * h11 - h01 * h01
        dead |= ~np.isfinite(det) | (det == 0)
        dof = max(nband - 2, 1)
        out = np.stack((alpha, np.sqrt(h11 / det * chi2 / dof), I0, np.sqrt(h00 / det * chi2 / dof)))
    out[:, dead] = np.nan
    if not info:
        return out
    return out, {'steps': steps, 'late': int(np.count_nonzero(~dead & (steps >= maxiter))),
                 'eps': np.stack(hist, axis=1) if hist else np.zeros((ncomps, 0))}


def fit_spi(image, beam, freqs, weights, threshold, pb_min, ref_freq, tol=1e-5, maxiter=100):
    """(alphamap, alpha_err_map, i0map, i0_err_map, maskindices) for numpy cubes, or ValueError for an empty mask."""
    image = np.where(beam > pb_min, image, 0)
    minimage = np.amin(image, axis=0)
    maskindices = np.argwhere(minimage > threshold)
    if not maskindices.size:
        raise ValueError(EMPTY_MASK % image.max())
    ix, iy = maskindices[:, 0], maskindices[:, 1]
    fit = fit_components(image[:, ix, iy].T.astype(np.float64), np.asarray(weights, dtype=np.float64),
                         np.asarray(freqs, dtype=np.float64), ref_freq, beam=beam[:, ix, iy].T.astype(np.float64),
                         tol=tol, maxiter=maxiter)
    maps = []
    for k in range(4):
        m = np.full(image[0].shape, np.nan, dtype=image.dtype)
        m[ix, iy] = fit[k]
        maps.append(m)
    return (*maps, maskindices)


# ----------------------------------------------------------------------------------------------------- cases
def make_case(nband, ncomps, noise, seed):
    """dict: freqs, ref_freq, weights (float64), data, beam ((ncomps, nband) float32), alpha, I0 (the truth)."""
    rng = np.random.default_rng([420, seed])
    freqs = np.linspace(0.9e9, 1.7e9, nband)
    ref_freq = 1.3e9
    weights = rng.uniform(0.5, 2.0, nband)
    alpha = rng.uniform(-2.0, 1.0, ncomps)
    I0 = 10.0 ** rng.uniform(-3.0, 1.0, ncomps)
    beam = rng.uniform(0.3, 1.0, (ncomps, nband)).astype(np.float32)
    model = I0[:, None] * beam * (freqs / ref_freq)[None, :] ** alpha[:, None]
    data = (model * (1.0 + noise * rng.standard_normal((ncomps, nband)))).astype(np.float32)
    return {'nband': nband, 'ncomps': ncomps, 'freqs': freqs, 'ref_freq': float(ref_freq), 'weights': weights,
            'data': data, 'beam': beam, 'alpha': alpha, 'I0': I0}


_cache = {}


def case(i):
    """CASES[i], built once and shared (read-only)."""
    if i not in _cache:
        c = make_case(*CASES[i])
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[i] = c
    return _cache[i]


def oracle(c, tol=1e-5, maxiter=100, info=False):
    return fit_components(c['data'].astype(np.float64), c['weights'], c['freqs'], c['ref_freq'],
                          beam=c['beam'].astype(np.float64), tol=tol, maxiter=maxiter, info=info)


def scale(out):
    """(4,) the largest finite magnitude of each output over the case."""
    return np.nanmax(np.abs(out), axis=1)


def spread_of(data, beam, weights, freqs, ref_freq, **kw):
    """(4,) max |fit(data + 1 ulp) - fit(data)| / scale per output, for a float64 component list; components whose
    outputs are NaN are left out.  **kw goes to fit_components (tol, maxiter, alphai, I0i)."""
    base = fit_components(data, weights, freqs, ref_freq, beam=beam, **kw)
    moved = fit_components(np.nextafter(data, np.inf), weights, freqs, ref_freq, beam=beam, **kw)
    return np.nanmax(np.abs(moved - base), axis=1) / scale(base)


def spread(c, tol=1e-5, maxiter=100):
    """spread_of the case's own components."""
    key = ('spread', id(c), tol, maxiter)
    if key not in _cache:
        _cache[key] = spread_of(c['data'].astype(np.float64), c['beam'].astype(np.float64), c['weights'], c['freqs'],
                                c['ref_freq'], tol=tol, maxiter=maxiter)
    return _cache[key]


def rho(c, tol=1e-5):
    """The largest eps_k / eps_(k-1) over the last two ratios of every component of the run to `tol`."""
    eps = oracle(c, tol=tol, info=True)[1]['eps']
    worst = 0.0
    for e in eps:
        e = e[~np.isnan(e)]
        if e.size >= 2:
            worst = max(worst, float(np.max((e[1:] / e[:-1])[-2:])))
    return worst


# ------------------------------------------------------------------------------------------------- image cubes
def cube_of(c, nx, ny, pixels, dtype=np.float32, floor=0.0):
    """(image, beam) (nband, nx, ny) of `dtype`: component k of the case at pixels[k] = (ix, iy), `floor` elsewhere in
    the image, beam 0.5 elsewhere."""
    nband = c['nband']
    image = np.full((nband, nx, ny), floor, dtype=dtype)
    beam = np.full((nband, nx, ny), 0.5, dtype=dtype)
    for k, (ix, iy) in enumerate(pixels):
        image[:, ix, iy] = c['data'][k]
        beam[:, ix, iy] = c['beam'][k]
    return image, beam


def pixels_of(n, nx, ny, seed):
    """n distinct pixels of an (nx, ny) plane, (0, 0) first and (nx - 1, ny - 1) last (n >= 2), the rest seeded."""
    rng = np.random.default_rng([421, seed])
    inner = 1 + rng.choice(nx * ny - 2, size=max(n - 2, 0), replace=False)
    flat = np.concatenate(([0], inner, [nx * ny - 1]))[:n] if n >= 2 else np.array([0])
    return [(int(q // ny), int(q % ny)) for q in flat]
