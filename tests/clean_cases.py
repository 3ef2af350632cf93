"""
Case generators for the CLEAN minor-cycle tests (tests/test_cpu_clean.py, tests/test_gpu_clean.py), and traced runs of the
greedy loops of oracle/clark.py.

Two kinds of input.
  exact    integer cubes in [-6, 6], a PSF that is 1 (or 0.5) at the centre, +-0.5 at about 2 % of the other positions and
           0 elsewhere, dyadic wsums, gamma 0.5 (sub-minor loop) or 1.0 (Hogbom), at most 16 iterations.  Every operation
           is then exact in float32 and in float64, so the float32 oracle equals the float64 oracle bit for bit and a
           kernel has to reproduce both with np.array_equal, ties at the maximum included.
  smooth   Gaussian-core PSFs with a width per band and a low oscillating sidelobe; noise plus a dozen point sources seen
           through that PSF, rounded to the dtype under test.  The reference is the oracle in float64 on those rounded
           values (`f64`), compared within a tolerance, which only makes sense where rounding cannot flip a choice of the
           greedy loop: every search of the traced float64 run has to keep a margin (below).

A traced run repeats the statements of the oracle's loop and records, per search of the arg-max,
  sel    (best - second best over distinct pixels) / best of the search image (inf for a single pixel),
  stop   |max - threshold| / threshold (inf for threshold 0),
  ties   the number of pixels equal to the maximum,
  pick   the flat index taken,
  used   whether the loop went on to take that pixel.
Its results are asserted equal to the oracle's own, bit for bit, in tests/test_cpu_clean.py; the oracle does not hand out
the final active set, the iteration count of Hogbom or the last peak, the trace does.
"""
import numpy as np

MARGIN = {np.dtype(np.float32): 2e-3, np.dtype(np.float64): 1e-9}
CLT = 1024                      # threads of the sub-minor workgroup (csrc/clark.hip)
HOG_THREADS = 1024 * 256        # threads of one k_hogbom_step launch
HOG_WORK = 17408                # the work buffer of deconv/hogbom.py
HOG_NEED = 256 + 64 * 8 + 1024 * 16     # what pfb_hogbom asks for: state, components, 1024 arg-max partials


# ------------------------------------------------------------------------------------------------- inputs
def exact_cube(rng, nband, nx, ny):
    return rng.integers(-6, 7, size=(nband, nx, ny)).astype(np.float64)


def exact_psf(rng, nband, P, Q, centre=1.0):
    psf = np.zeros((nband, P, Q))
    on = rng.random(psf.shape) < 0.02
    psf[on] = rng.choice([-0.5, 0.5], int(on.sum()))
    psf[:, P // 2, Q // 2] = centre
    return psf


def dyadic_wsums(nband):
    """Powers of two that sum to one: 0.5, 0.25, 0.25 for three bands, 1 / nband for a power of two."""
    if nband & (nband - 1) == 0:
        return np.full(nband, 1.0 / nband)
    w = [0.5 ** (b + 1) for b in range(nband)]
    w[-1] = w[-2]
    return np.array(w)


def smooth_psf(nband, P, Q):
    i = np.arange(P)[:, None] - P // 2
    j = np.arange(Q)[None, :] - Q // 2
    r = np.hypot(i, 0.8 * j)
    out = np.empty((nband, P, Q))
    for b in range(nband):
        w = 1.6 * (1.0 + 0.2 * b)
        core = np.exp(-r ** 2 / (2 * w ** 2))
        out[b] = core + (1.0 - core) * 0.03 * np.cos(0.7 * r / w) / (1.0 + r / (4 * w))
    return out


def smooth_cube(rng, psf, nx, ny, nsrc=12, noise=0.02, must_hold=None):
    """noise + nsrc point sources of flux 1 .. 4 with a spectral slope, seen through psf (shifted windows, as Hogbom
    subtracts them).  must_hold: a flat index that gets the brightest source."""
    nband, P, Q = psf.shape
    nx0, ny0 = P // 2, Q // 2
    cube = noise * rng.standard_normal((nband, nx, ny))
    flux = np.sort(1.0 + 3.0 * rng.random(nsrc))[::-1]
    pos = rng.choice(nx * ny, nsrc, replace=False)
    if must_hold is not None:
        pos[0] = must_hold
    for f, e in zip(flux, pos):
        p, q = divmod(int(e), ny)
        spec = f * (1.0 + 0.1 * np.arange(nband) * (rng.random() - 0.5))
        cube += spec[:, None, None] * psf[:, nx0 - p:nx0 - p + nx, ny0 - q:ny0 - q + ny]
    return cube


def active_subset(rng, nx, ny, nact):
    """nact distinct pixels in row-major order, as np.where returns them."""
    e = np.sort(rng.choice(nx * ny, nact, replace=False))
    return (e // ny).astype(np.int64), (e % ny).astype(np.int64)


# ------------------------------------------------------------------------------------------------- traced loops
class Trace:
    def __init__(self):
        self.sel, self.stop, self.ties, self.pick, self.used = [], [], [], [], []

    def look(self, search, threshold, used):
        """One arg-max of `search` (any shape); returns (flat index, sqrt of the maximum)."""
        flat = search.reshape(-1)
        pq = int(flat.argmax())
        best = flat[pq]
        amax = np.sqrt(best)
        if flat.size > 1 and best == best:
            rest = np.delete(flat, pq)
            second = rest.max()
            self.sel.append(float((np.float64(best) - np.float64(second)) / np.float64(best)) if best > 0 else 0.0)
            self.ties.append(int((flat == best).sum()))
        else:
            self.sel.append(np.inf)
            self.ties.append(1)
        thr = float(threshold)
        self.stop.append(abs(float(amax) - thr) / thr if thr > 0 else np.inf)
        self.pick.append(pq)
        self.used.append(bool(used(amax)))
        return pq, amax

    def margin(self):
        """The least margin any decision of the run had: every stop test, and the selection wherever it was used."""
        m = [s for s in self.stop]
        m += [s for s, u in zip(self.sel, self.used) if u]
        return min(m) if m else np.inf

    def tied(self):
        return any(t > 1 and u for t, u in zip(self.ties, self.used))


def subminor_traced(A, psf, Ip, Iq, model, wsums, gamma, th, maxit, trace=None):
    """oracle.clark.subminor, statement by statement.  Returns (model, k, A left over, trace); `model` is copied."""
    tr = trace if trace is not None else Trace()
    nband, nx_psf, ny_psf = psf.shape
    nxo2, nyo2 = nx_psf // 2, ny_psf // 2
    A = A.copy()
    model = model.copy()
    fsel = wsums > 0
    k = 0
    with np.errstate(invalid='ignore'):
        pq, Amax = tr.look(np.sum(A, axis=0) ** 2, th, lambda a: a > th and 0 < maxit)
        p, q = Ip[pq], Iq[pq]
        while Amax > th and k < maxit:
            xhat = A[:, pq].copy()
            model[fsel, p, q] += gamma * xhat[fsel] / wsums[fsel]
            A = A - xhat[:, None] * psf[:, nxo2 - (p - Ip), nyo2 - (q - Iq)]
            k += 1
            pq, Amax = tr.look(np.sum(A, axis=0) ** 2, th, lambda a, k=k: a > th and k < maxit)
            p, q = Ip[pq], Iq[pq]
    return model, k, A, tr


def hogbom_traced(ID, PSF, threshold, gamma, pf, maxit):
    """oracle.clark.hogbom, statement by statement.  Returns (model, status, IR, k, IRmax, trace)."""
    tr = Trace()
    nband, nx, ny = ID.shape
    _, nx_psf, ny_psf = PSF.shape
    nx0, ny0 = nx_psf // 2, ny_psf // 2
    x = np.zeros((nband, nx, ny), dtype=ID.dtype)
    IR = ID.copy()
    with np.errstate(invalid='ignore'):
        wsums = np.amax(PSF, axis=(1, 2))
        first = np.sum(IR, axis=0) ** 2
        tol = np.maximum(pf * np.sqrt(first.max()), threshold)
        pq, IRmax = tr.look(first, tol, lambda a: a > tol and 0 < maxit)
        k = 0
        while IRmax > tol and k < maxit:
            p, q = divmod(pq, ny)
            xhat = IR[:, p, q] / wsums
            x[:, p, q] += gamma * xhat
            IR = IR - gamma * xhat[:, None, None] * PSF[:, nx0 - p:nx0 + nx - p, ny0 - q:ny0 + ny - q]
            k += 1
            pq, IRmax = tr.look(np.sum(IR, axis=0) ** 2, tol, lambda a, k=k: a > tol and k < maxit)
    return x, (1 if k >= maxit else 0), IR, k, IRmax, tr


def clark_traced(ID, PSF, PSFHAT, wsums, threshold, gamma, pf, maxit, subpf, submaxit):
    """oracle.clark.clark with every decision recorded: the outer peak against tol, the membership of the active set
    (`member`: the least |IRsearch - subth^2| / subth^2 over all pixels and major iterations) and every step of every
    sub-minor loop.  Returns (model, status, k, trace, member)."""
    from oracle import fftconv as ofc
    tr = Trace()
    nband, nx, ny = ID.shape
    _, nx_psf, ny_psf = PSF.shape
    model = np.zeros((nband, nx, ny), dtype=ID.dtype)
    IR = ID.copy()
    xpad, xhat, xout = ofc.make_scratch(PSFHAT, ny_psf, ID.shape, ID.dtype)
    IRsearch = np.sum(IR, axis=0) ** 2
    tol = np.maximum(pf * np.sqrt(IRsearch.max()), threshold)
    _, IRmax = tr.look(IRsearch, tol, lambda a: False)
    k, member = 0, np.inf
    while IRmax > tol and k < maxit:
        subth = subpf * IRmax
        member = min(member, float(np.abs(IRsearch.astype(np.float64) - float(subth) ** 2).min() / float(subth) ** 2))
        Ip, Iq = np.where(IRsearch > subth ** 2)
        model, _, _, _ = subminor_traced(IR[:, Ip, Iq], PSF, Ip, Iq, model, wsums, gamma, subth, submaxit, trace=tr)
        ofc.psf_convolve_cube(xpad, xhat, xout, PSFHAT, ny_psf, model)
        IR = ID - xout
        IRsearch = np.sum(IR, axis=0) ** 2
        _, IRmax = tr.look(IRsearch, tol, lambda a: False)
        k += 1
    return model, (1 if k >= maxit else 0), k, tr, member


# ------------------------------------------------------------------------------------------------- sub-minor cases
NX, NY = 40, 53                 # the exact sub-minor image; PSF 79 x 105 is the smallest that covers it
SUB_NACT = [1, 63, 64, 65, 1023, 1024, 1025, 2 * 1024 + 37]
SUB_TIES = {                    # active-set indices forced to share the maximum; the lowest has to be taken first
    'second_pass': (5, CLT + 3),                    # CLT + 3 sits in a lower lane, on the thread's second trip
    'across_waves': (70, 64 * 3 + 1),
    'last_lane_first_lane': (64 * 15 + 63, 0),
    'three_way': (64 * 7 + 9, CLT + 64 * 2 + 1, 64 * 11 + 40),
}
SUB_PSF_EXTENTS = {'odd': (2 * NX - 1, 2 * NY - 1), 'even': (2 * NX, 2 * NY), 'oversized': (3 * NX, 2 * NY + 5)}
_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def sub_exact(nact=685, nband=3, extent='odd', seed=0, tie=None, wsums=None, centre=1.0, model0=False, nx=NX, ny=NY):
    """dict(A, psf, Ip, Iq, model0, wsums, nx, ny, gamma, th) in float64; cast with `as_dtype`."""
    def make():
        rng = np.random.default_rng(1000 + seed)
        P, Q = {'odd': (2 * nx - 1, 2 * ny - 1), 'even': (2 * nx, 2 * ny), 'oversized': (3 * nx, 2 * ny + 5)}[extent]
        ID = exact_cube(rng, nband, nx, ny)
        psf = exact_psf(rng, nband, P, Q, centre)
        Ip, Iq = active_subset(rng, nx, ny, nact)
        A = np.ascontiguousarray(ID[:, Ip, Iq])
        if tie is not None:
            for n, i in enumerate(SUB_TIES[tie]):
                A[:, i] = (7.0 if n % 2 == 0 else -7.0) * nband / 3 * np.ones(nband)    # |band sum| above any other
                A[0, i] += 1.0 if n % 2 == 0 else -1.0
        m0 = rng.integers(-3, 4, size=(nband, nx, ny)).astype(np.float64) if model0 else np.zeros((nband, nx, ny))
        w = dyadic_wsums(nband) if wsums is None else np.asarray(wsums, dtype=np.float64)
        return dict(A=A, psf=psf, Ip=Ip, Iq=Iq, model0=m0, wsums=w, nx=nx, ny=ny, gamma=0.5, th=2.0)
    return memo(('sub_exact', nact, nband, extent, seed, tie, None if wsums is None else tuple(wsums), centre, model0,
                 nx, ny), make)


# seeds chosen on the CPU oracle alone: the margin of tests/test_cpu_clean.py holds for them
SUB_SMOOTH = {np.dtype(np.float32): dict(seed=3, maxit=20), np.dtype(np.float64): dict(seed=3, maxit=20)}


def sub_smooth(dtype, seed=None):
    """The sub-minor loop on a smooth 70 x 90 cube with nact > 1024; inputs rounded to `dtype`."""
    dtype = np.dtype(dtype)
    seed = SUB_SMOOTH[dtype]['seed'] if seed is None else seed

    def make():
        nband, nx, ny = 3, 70, 90
        rng = np.random.default_rng(2000 + seed)
        psf = smooth_psf(nband, 2 * nx, 2 * ny)
        ID = smooth_cube(rng, psf, nx, ny, noise=0.3)
        search = np.sum(ID, axis=0) ** 2
        cut = np.sort(search.ravel())[-1500]                     # the 1499 brightest pixels
        Ip, Iq = np.where(search > cut)
        th = float(0.35 * np.sqrt(search.max()))
        c = dict(A=np.ascontiguousarray(ID[:, Ip, Iq]), psf=psf, Ip=Ip, Iq=Iq, model0=np.zeros_like(ID),
                 wsums=np.array([0.5, 0.3, 0.2]), nx=nx, ny=ny, gamma=0.1, th=th)
        return as_dtype(c, dtype)
    return memo(('sub_smooth', dtype, seed), make)


def as_dtype(c, dtype):
    cd = {np.dtype(np.float32): np.complex64, np.dtype(np.float64): np.complex128}[np.dtype(dtype)]
    return {k: (v.astype(dtype) if isinstance(v, np.ndarray) and v.dtype.kind == 'f' else
                v.astype(cd) if isinstance(v, np.ndarray) and v.dtype.kind == 'c' else v) for k, v in c.items()}


def f64(c):
    """The case as the reference sees it: the same (rounded) values in float64."""
    return as_dtype(c, np.float64)


# name -> arguments of sub_exact; every case runs with maxit 16 (and some with fewer, see the tests)
SUB_EXACT_CASES = {f'nact{n}': dict(nact=n) for n in SUB_NACT}
SUB_EXACT_CASES.update({f'tie_{t}': dict(nact=SUB_NACT[-1], tie=t) for t in SUB_TIES})
SUB_EXACT_CASES.update({
    'nband1': dict(nband=1), 'nband64': dict(nband=64, nact=1025, seed=4), 'wsum_zero': dict(wsums=(0.5, 0.0, 0.5)),
    'psf_even': dict(extent='even'), 'psf_oversized': dict(extent='oversized'),
    'accumulate': dict(centre=0.5, model0=True, nact=65),       # half of the peak stays: the pixel is taken again
})


def sub_nan_case():
    """sub_exact() with one PSF entry set to NaN: an entry that the SECOND component's subtraction reads (for active pixel
    j) and the first one's does not read.  The loop takes two components, the active set then holds a NaN, and the
    reference stops: np.argmax returns the NaN and `NaN > th` is false."""
    def make():
        c = dict(sub_exact())
        tr = run_sub(c, 16)[3]
        i0, i1 = tr.pick[0], tr.pick[1]
        Ip, Iq = c['Ip'], c['Iq']
        P, Q = c['psf'].shape[1:]
        read0 = set(zip((P // 2 - (Ip[i0] - Ip)).tolist(), (Q // 2 - (Iq[i0] - Iq)).tolist()))
        for j in range(len(Ip)):
            e = (int(P // 2 - (Ip[i1] - Ip[j])), int(Q // 2 - (Iq[i1] - Iq[j])))
            if j != i1 and e not in read0:
                break
        c['psf'] = c['psf'].copy()
        c['psf'][1, e[0], e[1]] = np.nan
        return c
    return memo('sub_nan', make)


def run_sub(c, maxit, th=None, gamma=None, dtype=None):
    """The traced sub-minor loop on case c (cast to dtype when given)."""
    if dtype is not None:
        c = as_dtype(c, dtype)
    return subminor_traced(c['A'], c['psf'], c['Ip'], c['Iq'], c['model0'], c['wsums'],
                           c['gamma'] if gamma is None else gamma, c['th'] if th is None else th, maxit)


# ------------------------------------------------------------------------------------------------- Hogbom cases
HOG_EXACT_SHAPES = [(1, 1), (1, 7), (7, 1), (31, 17)]
HOG_BIG = (520, 509)            # 264 680 pixels: more than the 262 144 threads of one launch
HOG_BATCH_MAXIT = [0, 1, 63, 64, 65, 129]
HOG_BIG_TIES = {                # flat indices that share the first maximum
    'second_pass': (HOG_THREADS + 5, 5),                 # one thread, its first and its second trip
    'across_workgroups': (300, HOG_THREADS + 7),         # the lower index in the higher workgroup
}


def hog_extent(nx, ny, extent):
    return {'odd': (2 * nx - 1, 2 * ny - 1), 'even': (2 * nx, 2 * ny), 'oversized': (3 * nx, 2 * ny + 5)}[extent]


def hog_exact(nx, ny, nband=2, extent='odd', seed=0, tie=None):
    """dict(ID, psf, gamma, pf, threshold) in float64."""
    def make():
        rng = np.random.default_rng(3000 + seed)
        P, Q = hog_extent(nx, ny, extent)
        ID = exact_cube(rng, nband, nx, ny)
        psf = exact_psf(rng, nband, P, Q)
        if tie is not None:
            for n, e in enumerate(tie):
                ID[:, e // ny, e % ny] = (7.0 if n % 2 == 0 else -7.0)
        return dict(ID=ID, psf=psf, gamma=1.0, pf=0.0, threshold=2.0)
    return memo(('hog_exact', nx, ny, nband, extent, seed, tie), make)


HOG_EXACT_CASES = {f'{nx}x{ny}': dict(nx=nx, ny=ny) for nx, ny in HOG_EXACT_SHAPES}
HOG_EXACT_CASES.update({
    'nband1': dict(nx=31, ny=17, nband=1), 'nband64': dict(nx=31, ny=17, nband=64),
    'psf_even': dict(nx=31, ny=17, extent='even'), 'psf_oversized': dict(nx=31, ny=17, extent='oversized'),
})
HOG_BIG_CASES = {t: dict(nx=HOG_BIG[0], ny=HOG_BIG[1], tie=HOG_BIG_TIES[t]) for t in HOG_BIG_TIES}
HOG_BIG_CASES['both'] = dict(nx=HOG_BIG[0], ny=HOG_BIG[1], tie=HOG_BIG_TIES['second_pass'] + HOG_BIG_TIES['across_workgroups'])

# seeds and iteration counts chosen on the CPU oracle alone: the margin of tests/test_cpu_clean.py holds for them
HOG_SMOOTH_BIG = {np.dtype(np.float32): dict(seed=0, maxit=20), np.dtype(np.float64): dict(seed=0, maxit=40)}
HOG_SMOOTH_SMALL = dict(nx=12, ny=9, seed=2, nsrc=6)        # float64, up to 129 iterations
HOG_SMOOTH_STOP = dict(nx=37, ny=22, seed=0)                # both dtypes, about 18 iterations
HOG_STOPS = {'pf': dict(pf=0.55, threshold=0.0), 'threshold': dict(pf=0.0, threshold=6.3)}


def hog_smooth_big(dtype):
    """2 x 520 x 509 with the brightest source past the first 262 144 pixels."""
    return hog_smooth(dtype, *HOG_BIG, seed=HOG_SMOOTH_BIG[np.dtype(dtype)]['seed'], must_hold=HOG_THREADS + 1000)


def hog_smooth(dtype, nx, ny, nband=2, seed=0, must_hold=None, noise=0.02, nsrc=12):
    dtype = np.dtype(dtype)

    def make():
        rng = np.random.default_rng(4000 + seed)
        psf = smooth_psf(nband, 2 * nx, 2 * ny)
        ID = smooth_cube(rng, psf, nx, ny, nsrc=min(nsrc, nx * ny), noise=noise, must_hold=must_hold)
        return dict(ID=ID.astype(dtype), psf=psf.astype(dtype), gamma=0.1, pf=0.0, threshold=0.0)
    return memo(('hog_smooth', dtype, nx, ny, nband, seed, must_hold, noise, nsrc), make)


def run_hog(c, maxit, dtype=None, **kw):
    if dtype is not None:
        c = as_dtype(c, dtype)
    a = dict(threshold=c['threshold'], gamma=c['gamma'], pf=c['pf'])
    a.update(kw)
    return hogbom_traced(c['ID'], c['psf'], a['threshold'], a['gamma'], a['pf'], maxit)


# ------------------------------------------------------------------------------------------------- full minor cycle
CLARK_FULL = {np.dtype(np.float32): dict(seed=0), np.dtype(np.float64): dict(seed=0)}
CLARK_KW = dict(threshold=0.0, gamma=0.1, pf=0.2, maxit=4, subpf=0.6, submaxit=15)


def clark_full(dtype, seed=None):
    """3 bands, 48 x 40, PSF 96 x 80, PSFHAT from the oracle; inputs rounded to dtype."""
    from oracle import fftconv as ofc
    dtype = np.dtype(dtype)
    seed = CLARK_FULL[dtype]['seed'] if seed is None else seed

    def make():
        nband, nx, ny = 3, 48, 40
        rng = np.random.default_rng(5000 + seed)
        psf = smooth_psf(nband, 2 * nx, 2 * ny)
        ID = smooth_cube(rng, psf, nx, ny, nsrc=8, noise=0.02).astype(dtype)
        psf = psf.astype(dtype)
        psfhat = ofc.psfhat_from_psf(psf.astype(np.float64))        # complex128; as_dtype rounds it for the device
        return dict(ID=ID, psf=psf, psfhat=psfhat, wsums=np.array([0.5, 0.25, 0.25], dtype=dtype))
    return memo(('clark_full', dtype, seed), make)


# ------------------------------------------------------------------------------------------------- freqmul
FM_NBAND = [1, 2, 5, 64]
FM_NPIX = [1, 255, 256, 257]
FM_NPIX_BIG = 1048576 + 257     # more than 4096 workgroups of 256: the capped grid strides
FM_GUARD = 64


def freqmul_case(dtype, nband, npix, seed=0):
    rng = np.random.default_rng(6000 + seed + 7 * nband + npix % 1000)
    return tuple(rng.standard_normal(s).astype(dtype) for s in ((nband, nband), (nband, npix), (nband, npix), (nband, npix)))


def freqmul_ref(A, x, pre, post):
    """(ref, bound / eps): float64 einsum on the given (dtype-rounded) values and sum_l |A_kl| |x_l| |pre_l| |post_k|."""
    A64, x64 = A.astype(np.float64), x.astype(np.float64)
    if pre is not None:
        x64 = x64 * pre.astype(np.float64)
    ref = np.einsum('kl,lp->kp', A64, x64)
    mag = np.einsum('kl,lp->kp', np.abs(A64), np.abs(x64))
    if post is not None:
        ref = ref * post.astype(np.float64)
        mag = mag * np.abs(post.astype(np.float64))
    return ref, mag
