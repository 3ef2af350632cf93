"""
GPU tests of the elementwise layer every solver iteration runs through (csrc/wavelet.hip, csrc/cgvec.hip on the packs,
can_vec and partial sums of csrc/common.hpp): the l21 dual update and its two-phase / chunked form, prox_21m, prox_21,
dual_update_l2, the primal-dual image update, and the scalar (V = 1) forms of the fused PCG's vector kernels.

Every entry point picks one of several kernels on the host -- by element count, pointer alignment, band count, cube
size and which optional pointers are given.  The cases below are the smallest that cross each of those boundaries; the
C ABI is called through pfb_clean_amd._lib / _dev with raw device pointers, and the Python wrappers where they hand a
contiguous GPU tensor's pointer through unchanged.

  * every array a kernel writes is a slice of a larger device tensor with PAD sentinel elements on either side, which
    must come back bit-identical; every array a kernel only reads must come back bit-identical as well;
  * `torch.empty(n + k)[k:]` views give pointers aligned to the element but not to 16 bytes (the documented "any
    alignment" case);
  * the reference is oracle.prox / the primal statement of oracle/solvers.py:374-379 in float64 on the inputs as the
    kernel sees them (arrays and the scalars lam, sigma, tau rounded to the kernel's dtype).

Tolerances: PER ELEMENT, not max-norm (a max-norm bound hides a wrong value in every small element, and those are what
the threshold branches produce).  With eps the dtype's epsilon, vt = vp + sigma v:
    dual update (band sum)  K eps (|vp| + |sigma v|) (1 + (nband + 1) sum_b(|vp| + |sigma v|) / |sum_b vt|)
    prox_21m                K eps |v| / sigma (1 + (nband + 1) sum_b|v| / |sum_b v|)
    prox_21, dual_update_l2 the two rows above with the cancellation factor replaced by (nband + 4)
    primal update           K eps (|xp| + |tau| (2|xout| + |xout_prev| + |g| + |gsub|))
K = 4 (prox / dual forms), 8 (primal step): four times what the reference formula itself needs when it is evaluated in
working precision (test_bound_constants_hold_for_the_reference_in_working_precision, a CPU test, re-measures that on the
inputs used here).  PCG: TOL_PCG of test_gpu_conv_pcg.py (fp64 1e-9, fp32 1e-3 of max|reference|); fp64 reductions 1e-12.

Only the GPU tests carry the gpu mark (one by one, not through pytestmark): the check of the constants runs anywhere.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import fftconv as ofc          # checker only
from oracle import prox as oprox
from oracle import solvers as osv

torch = None        # imported by the `amd` fixture, which every GPU test takes: the CPU tests need numpy alone

gpu = pytest.mark.gpu
pmp = pytest.mark.parametrize

DTYPES = [np.float32, np.float64]
TOL_PCG = {np.float64: 1e-9, np.float32: 1e-3}      # as tests/test_gpu_conv_pcg.py
TOL_SUM = 1e-12                                      # fp64 reductions, as test_vector_kernels

# The constants of the per-element bounds.  max |formula in working precision - formula in float64| / bound(K = 1),
# numpy on the inputs of this file (prox_inputs / primal_inputs, 100003 coefficients, nband 1/2/3/8/12, every pair of
# LAMSIG), float32 against float64 | float64 against the x87 long double:
#     band-sum dual update  0.32 | 0.28        prox_21m  0.46 | 0.47
#     l2 forms              0.28 | 0.28        primal    1.62 | 1.63
# so K = 4 and K = 8 leave the reference a factor of four; the CPU test below asserts that quarter.
K_PROX = 4.0
K_PRIMAL = 8.0
# positivity 2: columns whose reference value lies within the bound of zero in some band are "tied" and left out.
# Observed share with these inputs (reference and bound alone, 3 x 1048652 pixels): 1.9e-6 in fp32, 0 in fp64.
TIE_CAP = 1e-3

LAMSIG = [(1.0, 75.0), (0.1, 1.0), (1e-3, 1e-3), (0.5, 2.0)]

PAD = 64                 # sentinel elements on either side of every device array
SENT = -1234.5           # a finite value no kernel here produces (exact in fp32 and fp64)


# ------------------------------------------------------------------------------------------------ inputs (CPU)
def rounded(dt, *vals):
    """Host scalars as the kernels see them: rounded to the kernel's dtype."""
    return tuple(float(dt(v)) for v in vals)


def prox_inputs(dt, nband, nper, seed):
    """vp, v (nband, nper) standard normal; w (nper) in [0.5, 1.5): with lam > 0 the threshold is positive and the
    operators are continuous at a zero band sum."""
    rng = np.random.default_rng(seed)
    vp = rng.standard_normal((nband, nper), dtype=dt)
    v = rng.standard_normal((nband, nper), dtype=dt)
    w = (0.5 + rng.random(nper, dtype=dt)).astype(dt)
    return vp, v, w


def primal_inputs(dt, nband, npix, seed):
    rng = np.random.default_rng(seed)
    return {k: rng.standard_normal((nband, npix), dtype=dt) for k in ('xp', 'xout', 'xprev', 'g', 'gsub')}


def f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


# ------------------------------------------------------------------- reference and bounds (any precision)
def ref_dual(vp, v, w, lam, sigma):
    out = v.copy()
    oprox.dual_update_numba(vp, out, lam, sigma=sigma, weight=w)
    return out


def ref_dual_l2(vp, v, w, lam, sigma):
    out = v.copy()
    oprox.dual_update_numba_l2(vp, out, lam, sigma=sigma, weight=w)
    return out


def ref_prox(fn, v, w, lam, sigma):
    out = np.empty_like(v)
    fn(v, out, lam, sigma=sigma, weight=w)
    return out


def ref_primal(xp, xout, xprev, g, gsub, tau, positivity):
    """oracle/solvers.py:374-379 with the two fusions of pfb_pd_primal_update2 spelled out.  Returns (x, x before the
    positivity step)."""
    xo = xout if xprev is None else 2 * xout - xprev
    if g is not None:
        xo = xo + (g if gsub is None else g - gsub)
    x = xp - tau * xo                                     # primal_dual.py:140
    raw = x.copy()
    if positivity == 1:
        x[x < 0.0] = 0.0
    elif positivity == 2:
        msk = np.any(x <= 0, axis=0)
        x[:, msk] = 0.0
    return x, raw


def _scaled(K, eps, terms, total, l2):
    """K eps terms times the cancellation factor of the band sum `total` (l2: nband + 4 instead).  Where a term is zero
    the result is exactly zero in any precision: bound 0 (not 0 * inf)."""
    nband = terms.shape[0]
    with np.errstate(divide='ignore', invalid='ignore'):
        fac = float(nband + 4) if l2 else 1.0 + (nband + 1) * terms.sum(axis=0) / np.abs(total)
        b = K * eps * terms * fac
    b[terms == 0] = 0.0
    return b


def bound_dual(vp, v, sigma, eps, l2=False, K=K_PROX):
    vp, v = f64(vp), f64(v)
    return _scaled(K, eps, np.abs(vp) + np.abs(sigma * v), (vp + sigma * v).sum(axis=0), l2)


def bound_prox(v, sigma, eps, l2=False, K=K_PROX):
    v = f64(v)
    return _scaled(K, eps, np.abs(v), v.sum(axis=0), l2) / sigma


def bound_primal(xp, xout, xprev, g, gsub, tau, eps, K=K_PRIMAL):
    s = 2 * np.abs(f64(xout))
    for a in (xprev, g, gsub):
        if a is not None:
            s = s + np.abs(f64(a))
    return K * eps * (np.abs(f64(xp)) + abs(tau) * s)


def assert_within(got, ref, bound, what, skip_cols=()):
    """|got - ref| <= bound in every element (a NaN anywhere fails), columns `skip_cols` left out."""
    err = np.abs(f64(got) - ref)
    bad = ~(err <= bound)
    for c in skip_cols:
        bad[..., c] = False
    if bad.any():
        i = tuple(int(k[0]) for k in np.nonzero(bad))
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.size} elements outside their bound; first at {i}: "
                    f"got {f64(got)[i]!r} ref {ref[i]!r} err {err[i]:.3e} bound {np.broadcast_to(bound, err.shape)[i]:.3e}")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def tied_columns(raw, bound):
    return np.any(np.abs(raw) <= bound, axis=0)


# ------------------------------------------------------------------------------------------- the CPU test
def _hi(dt):
    return np.float64 if dt == np.float32 else np.longdouble


def _ratio(work, ref, bound):
    r = np.abs(work.astype(ref.dtype) - ref) / bound
    return float(np.nanmax(np.where(np.isfinite(r), r, 0.0)))


@pmp('dt', [np.float32] + ([np.float64] if np.finfo(np.longdouble).eps < 1e-18 else []))
@pmp('ls', range(len(LAMSIG)))
def test_bound_constants_hold_for_the_reference_in_working_precision(dt, ls):
    """K comes from the reference, never from the kernels: the oracle's formulas evaluated in the kernel's precision
    (numpy, arrays and scalars of that dtype) stay within a QUARTER of each bound of their evaluation one precision up,
    on the inputs the GPU tests use."""
    hi = _hi(dt)
    eps = float(np.finfo(dt).eps)
    lam, sigma = rounded(dt, *LAMSIG[ls])
    worst = {}
    for nband in (1, 2, 3, 8, 12):
        vp, v, w = prox_inputs(dt, nband, 100003, seed=1000 * nband + ls)
        H = [a.astype(hi) for a in (vp, v, w)]
        cases = {
            'dual': (ref_dual(vp, v, w, dt(lam), dt(sigma)), ref_dual(*H, hi(lam), hi(sigma)),
                     bound_dual(vp, v, sigma, eps, K=1.0)),
            'dual_l2': (ref_dual_l2(vp, v, w, dt(lam), dt(sigma)), ref_dual_l2(*H, hi(lam), hi(sigma)),
                        bound_dual(vp, v, sigma, eps, l2=True, K=1.0)),
            'prox_21m': (ref_prox(oprox.prox_21m_numba, v, w, dt(lam), dt(sigma)),
                         ref_prox(oprox.prox_21m_numba, H[1], H[2], hi(lam), hi(sigma)),
                         bound_prox(v, sigma, eps, K=1.0)),
            'prox_21': (ref_prox(oprox.prox_21_numba, v, w, dt(lam), dt(sigma)),
                        ref_prox(oprox.prox_21_numba, H[1], H[2], hi(lam), hi(sigma)),
                        bound_prox(v, sigma, eps, l2=True, K=1.0)),
        }
        for name, (work, ref, bnd) in cases.items():
            assert work.dtype == dt and ref.dtype == hi
            worst[name] = max(worst.get(name, 0.0), _ratio(work, ref, bnd))
        p = primal_inputs(dt, nband, 100003, seed=77 * nband + ls)
        tau, = rounded(dt, 0.37 * (ls + 1))
        for keys in (('g',), ('g', 'gsub'), ('xprev',), ('xprev', 'g', 'gsub'), ()):
            a = {k: (p[k] if k in keys else None) for k in ('xprev', 'g', 'gsub')}
            work = ref_primal(p['xp'], p['xout'], a['xprev'], a['g'], a['gsub'], dt(tau), 0)[0]
            ref = ref_primal(p['xp'].astype(hi), p['xout'].astype(hi), *(None if a[k] is None else a[k].astype(hi)
                                                                        for k in ('xprev', 'g', 'gsub')), hi(tau), 0)[0]
            assert work.dtype == dt
            worst['primal'] = max(worst.get('primal', 0.0),
                                  _ratio(work, ref, bound_primal(p['xp'], p['xout'], a['xprev'], a['g'], a['gsub'],
                                                                 tau, eps, K=1.0)))
    print(f"reference in {np.dtype(dt).name}, (lam, sigma) = {LAMSIG[ls]}: ratios at K = 1: "
          + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    for name, r in worst.items():
        K = K_PRIMAL if name == 'primal' else K_PROX
        assert r <= 0.25 * K, (name, r)


def test_tie_share_of_the_reference():
    """positivity 2: the share of columns the per-element bound cannot decide stays far below TIE_CAP on this file's
    inputs (a property of reference and bound alone)."""
    for dt in DTYPES:
        eps = float(np.finfo(dt).eps)
        p = primal_inputs(dt, 3, 1048652, seed=5)
        tau, = rounded(dt, 0.37)
        raw = ref_primal(*(f64(p[k]) for k in ('xp', 'xout', 'xprev', 'g', 'gsub')), tau, 0)[1]
        share = tied_columns(raw, bound_primal(p['xp'], p['xout'], p['xprev'], p['g'], p['gsub'], tau, eps)).mean()
        print(f"tie share {np.dtype(dt).name}: {share:.2e}")
        assert share <= TIE_CAP / 10


# ------------------------------------------------------------------------------------------ device helpers
@pytest.fixture(scope='module')
def amd():
    global torch
    torch = pytest.importorskip('torch')
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from pfb_clean_amd import _lib, _dev
    from pfb_clean_amd.operators import psf
    from pfb_clean_amd.prox import prox_21m, prox_21

    class NS:
        pass
    ns = NS()
    ns.lib, ns._lib, ns.dev, ns.psf, ns.prox_21m, ns.prox_21 = _lib.load(), _lib, _dev, psf, prox_21m, prox_21
    ns.ncu = torch.cuda.get_device_properties(0).multi_processor_count
    return ns


def vwidth(dt):
    return 16 // np.dtype(dt).itemsize


def misalignments(dt):
    """Element offsets that leave a pointer off a 16-byte boundary: 1 (both dtypes), 2 (fp32: 8-byte aligned)."""
    return (1, 2) if dt == np.float32 else (1,)


class Buf:
    """A device array inside a larger tensor: PAD sentinels, k more (the misalignment), the data, PAD sentinels.
    Buf(data) holds a copy of the numpy array `data`; Buf.out(shape, dt) is all sentinel (an array a kernel writes)."""

    def __init__(self, data, k=0):
        data = np.ascontiguousarray(data)
        self.shape, self.n, self.dt = data.shape, data.size, data.dtype.type
        self.lo = PAD + k
        self.full = torch.full((self.lo + self.n + PAD,), SENT, device='cuda',
                               dtype=torch.float32 if self.dt == np.float32 else torch.float64)
        self.t = self.full[self.lo:self.lo + self.n]
        self.t.copy_(torch.from_numpy(data.reshape(-1)))
        assert self.full.data_ptr() % 16 == 0 and self.t.is_contiguous()
        assert (self.t.data_ptr() % 16 == 0) == ((k * data.itemsize) % 16 == 0)
        self.before = self.full.clone()

    @classmethod
    def out(cls, shape, dt, k=0):
        return cls(np.full(shape, SENT, dtype=dt), k)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def at(self, off):
        return self.t.data_ptr() + off * self.t.element_size()

    def view(self):
        """The data as a device tensor of the array's shape (what the Python wrappers are handed)."""
        return self.t.view(self.shape)

    def numpy(self):
        return self.t.cpu().numpy().reshape(self.shape)

    def guards_ok(self):
        return bool((self.full[:self.lo] == SENT).all()) and bool((self.full[self.lo + self.n:] == SENT).all())

    def unchanged(self):
        it = torch.int32 if self.dt == np.float32 else torch.int64
        return torch.equal(self.full.view(it), self.before.view(it))


def check_buffers(written=(), read=()):
    torch.cuda.synchronize()
    for i, b in enumerate(written):
        assert b.guards_ok(), f"sentinels around written array {i} changed"
    for i, b in enumerate(read):
        assert b.unchanged(), f"read-only array {i} (or its sentinels) changed"


def code_of(amd, dt):
    return amd._lib.PFB_F32 if dt == np.float32 else amd._lib.PFB_F64


def ok(amd, rc):
    amd._lib.check(rc)


# ---------------------------------------------------------------------------------- 1. pfb_dual_update
def run_dual_update(amd, dt, vp, v, w, lam, sigma, mode, k=None, via='abi'):
    """One pfb_dual_update.  mode: 'none' (no vp_out), 'out' (a separate vp_out), 'alias' (vp_out = vp).  k: element
    offsets of (vp, v, w, vp_out).  Returns (v_new, vp_out | None) after checking guards and read-only inputs."""
    nband, nper = vp.shape
    k = k or (0, 0, 0, 0)
    bvp, bv, bw = Buf(vp, k[0]), Buf(v, k[1]), Buf(w, k[2])
    bo = {'none': None, 'out': Buf.out(vp.shape, dt, k[3]), 'alias': bvp}[mode]
    if via == 'abi':
        ok(amd, amd.lib.pfb_dual_update(code_of(amd, dt), bvp.ptr, bv.ptr, bw.ptr, lam, sigma, nband, nper,
                                         None if bo is None else bo.ptr, amd.dev.stream()))
    else:           # contiguous GPU tensors go through the wrapper as they are
        r = amd.prox_21m.dual_update_numba(bvp.view(), bv.view(), lam, sigma=sigma, weight=bw.view(),
                                           vp_out=None if bo is None else bo.view())
        assert r.data_ptr() == bv.ptr
    check_buffers(written=[bv] + ([bo] if bo is not None else []), read=[bw] + ([bvp] if mode != 'alias' else []))
    return bv.numpy(), None if bo is None else bo.numpy()


def dual_refs(dt, vp, v, w, lam, sigma):
    """(v_new, its bound, vp_out, its bound).  vp_out = 2 v_new - vp costs one more rounding of a value no larger than
    3 (|vp| + |sigma v|) on top of twice v_new's error."""
    eps = float(np.finfo(dt).eps)
    ref = ref_dual(f64(vp), f64(v), f64(w), lam, sigma)
    bnd = bound_dual(vp, v, sigma, eps)
    t = np.abs(f64(vp)) + np.abs(sigma * f64(v))
    return ref, bnd, 2.0 * ref - f64(vp), 2.0 * bnd + 3.0 * eps * t


@gpu
@pmp('dt', DTYPES)
@pmp('nband', [1, 2, 3, 4, 5, 6, 7, 8, 9, 12])
def test_dual_update_kernel_selection(amd, dt, nband):
    """nband <= 8 and a multiple of the pack width: k_dual_update_vec<T, nband, false>; nband 9 / 12 or any other
    count: the scalar k_dual_apply<T, false>.  Sizes: vector tails; counts that are no multiple of V; a second, partly
    filled trip of the vector kernel's grid-stride loop (its grid is capped at one workgroup per CU) and of the scalar
    kernel's (2048 workgroups).  Without vp_out, with one, and with vp_out aliasing vp."""
    V = vwidth(dt)
    lam, sigma = rounded(dt, *LAMSIG[nband % 4])
    for nper in (V, 3 * V, 256 * V + V, 1, V + 1, 257, (amd.ncu * 256 + 37) * V, 2048 * 256 + 259):
        vp, v, w = prox_inputs(dt, nband, nper, seed=nband * 131 + nper)
        ref, bnd, refo, bndo = dual_refs(dt, vp, v, w, lam, sigma)
        for mode in ('none', 'out', 'alias'):
            got, goto = run_dual_update(amd, dt, vp, v, w, lam, sigma, mode)
            assert_within(got, ref, bnd, f"v, nper {nper}, {mode}")
            if goto is not None:        # against the vp saved before the call when aliased
                assert_within(goto, refo, bndo, f"vp_out, nper {nper}, {mode}")


@gpu
@pmp('dt', DTYPES)
@pmp('nband', [1, 3, 8])
def test_dual_update_misaligned_operand(amd, dt, nband):
    """A count that would take the vector kernel, with one operand off the 16-byte boundary: the scalar kernel, the same
    bound, nothing written outside the arrays.  Through the C ABI and through prox_21m.dual_update_numba."""
    V = vwidth(dt)
    nper = 256 * V + V
    lam, sigma = rounded(dt, *LAMSIG[(nband + 1) % 4])
    vp, v, w = prox_inputs(dt, nband, nper, seed=9 + nband)
    ref, bnd, refo, bndo = dual_refs(dt, vp, v, w, lam, sigma)
    for which in range(4):
        for off in misalignments(dt):
            k = tuple(off if i == which else 0 for i in range(4))
            for via in ('abi', 'py'):
                got, goto = run_dual_update(amd, dt, vp, v, w, lam, sigma, 'out', k, via)
                assert_within(got, ref, bnd, f"v, operand {which} + {off}, {via}")
                assert_within(goto, refo, bndo, f"vp_out, operand {which} + {off}, {via}")
    for off in misalignments(dt):       # vp_out = vp, both off the boundary
        got, goto = run_dual_update(amd, dt, vp, v, w, lam, sigma, 'alias', (off, 0, 0, 0))
        assert_within(got, ref, bnd, f"v, aliased vp + {off}")
        assert_within(goto, refo, bndo, f"vp_out, aliased vp + {off}")


@gpu
@pmp('dt', DTYPES)
@pmp('nband', [2, 8])
@pmp('below', [False, True])
def test_dual_update_non_temporal_switch(amd, dt, nband, below):
    """nband nper sizeof(T) >= 64 MiB switches k_dual_update_vec to its non-temporal loads (NTL = true): one cube
    exactly there, one a pack below it (NTL = false), both pointwise, with a
    separate vp_out and with vp_out = vp."""
    V = vwidth(dt)
    nper = (64 << 20) // (nband * np.dtype(dt).itemsize) - (V if below else 0)
    lam, sigma = rounded(dt, *LAMSIG[3])
    vp, v, w = prox_inputs(dt, nband, nper, seed=nband + 2 * below)
    ref, bnd, refo, bndo = dual_refs(dt, vp, v, w, lam, sigma)
    for mode in ('out', 'alias'):       # vp_out may alias vp in the non-temporal form as well
        got, goto = run_dual_update(amd, dt, vp, v, w, lam, sigma, mode)
        assert_within(got, ref, bnd, f"v, {mode}")
        assert_within(goto, refo, bndo, f"vp_out, {mode}")


# ---------------------------------------------------------------------------------- 2. exact branches
ZERO_SUM, BELOW, NAN_COL, ALL_ZERO = 1, 2, 5, 6     # columns; each shares its 16-byte pack with ordinary columns


def planted_inputs(dt, nband, nper):
    """Random columns, and: a band sum that is exactly zero from exactly representable values; a column strictly below
    the threshold whose vt = vp + 2 v is exact with or without FMA; one NaN in one band; an all-zero column (the zero
    branch of the l2 forms).  lam = 0.5, sigma = 2: the threshold lam w / sigma is at least 0.125."""
    assert nband >= 3 and nper > ALL_ZERO + 1
    vp, v, w = prox_inputs(dt, nband, nper, seed=nband + nper)
    for c in (ZERO_SUM, BELOW, ALL_ZERO):
        vp[:, c] = 0
        v[:, c] = 0
    vp[0, ZERO_SUM], vp[1, ZERO_SUM] = 1, -1
    vp[0, BELOW], vp[1, BELOW] = 2.0 ** -10, 2.0 ** -11
    v[0, BELOW], v[2, BELOW] = 2.0 ** -12, 2.0 ** -12
    vp[1, NAN_COL] = np.nan
    return vp, v, w, 0.5, 2.0


@gpu
@pmp('dt', DTYPES)
@pmp('path', ['vector', 'scalar: odd count', 'scalar: 9 bands', 'scalar: misaligned', 'two-phase'])
def test_dual_update_exact_branches(amd, dt, path):
    V = vwidth(dt)
    nband = 9 if path == 'scalar: 9 bands' else 3
    nper = 4 * V + (1 if path == 'scalar: odd count' else 0)
    vp, v, w, lam, sigma = planted_inputs(dt, nband, nper)
    vt = vp + dt(sigma) * v                         # exact in the planted columns
    if path == 'two-phase':
        bvp, bv, bw, bs, bo = Buf(vp), Buf(v), Buf(w), Buf.out(nper, dt), Buf.out(vp.shape, dt)
        ok(amd, amd.lib.pfb_dual_bandsum(code_of(amd, dt), bvp.ptr, bv.ptr, sigma, nband, nper, bs.ptr, amd.dev.stream()))
        ok(amd, amd.lib.pfb_dual_apply(code_of(amd, dt), bvp.ptr, bv.ptr, bw.ptr, bs.ptr, lam, sigma, nband, nper,
                                        bo.ptr, amd.dev.stream()))
        check_buffers(written=[bv, bs, bo], read=[bvp, bw])
        got, goto = bv.numpy(), bo.numpy()
    else:
        k = (0, 1, 0, 0) if path == 'scalar: misaligned' else None
        got, goto = run_dual_update(amd, dt, vp, v, w, lam, sigma, 'out', k)
    for c in (ZERO_SUM, BELOW, ALL_ZERO):           # v = vt bitwise, vp_out = 2 vt - vp (exact there)
        assert np.array_equal(bits(got[:, c]), bits(vt[:, c])), (c, got[:, c], vt[:, c])
        assert np.array_equal(bits(goto[:, c]), bits(dt(2) * vt[:, c] - vp[:, c])), (c, goto[:, c])
    assert np.isnan(got[:, NAN_COL]).all() and np.isnan(goto[:, NAN_COL]).all()
    ref, bnd, refo, bndo = dual_refs(dt, vp, v, w, lam, sigma)
    assert_within(got, ref, bnd, "v", skip_cols=(NAN_COL,))          # its pack neighbours are finite and right
    assert_within(goto, refo, bndo, "vp_out", skip_cols=(NAN_COL,))


def run_plane(amd, dt, form, a, b, w, lam, sigma, k=None, via='abi'):
    """prox_21m / prox_21: result = f(a) (b unused); dual_update_l2: in place on b with vp = a.  k: element offsets of
    (input, output, weight).  Returns the result."""
    nband, nper = a.shape
    k = k or (0, 0, 0)
    ba, bw = Buf(a, k[0]), Buf(w, k[2])
    bout = Buf(b, k[1]) if form == 'dual_update_l2' else Buf.out(a.shape, dt, k[1])
    fn = getattr(amd.lib, 'pfb_' + form)
    if via == 'abi':
        ok(amd, fn(code_of(amd, dt), ba.ptr, bout.ptr, bw.ptr, lam, sigma, nband, nper, amd.dev.stream()))
    elif form == 'prox_21m':
        amd.prox_21m.prox_21m_numba(ba.view(), bout.view(), lam, sigma=sigma, weight=bw.view())
    elif form == 'prox_21':
        amd.prox_21.prox_21_numba(ba.view(), bout.view(), lam, sigma=sigma, weight=bw.view())
    else:
        amd.prox_21.dual_update_numba(ba.view(), bout.view(), lam, sigma=sigma, weight=bw.view())
    check_buffers(written=[bout], read=[ba, bw])
    return bout.numpy()


def plane_ref(dt, form, a, b, w, lam, sigma):
    eps = float(np.finfo(dt).eps)
    if form == 'prox_21m':
        return ref_prox(oprox.prox_21m_numba, f64(a), f64(w), lam, sigma), bound_prox(a, sigma, eps)
    if form == 'prox_21':
        return ref_prox(oprox.prox_21_numba, f64(a), f64(w), lam, sigma), bound_prox(a, sigma, eps, l2=True)
    return ref_dual_l2(f64(a), f64(b), f64(w), lam, sigma), bound_dual(a, b, sigma, eps, l2=True)


@gpu
@pmp('dt', DTYPES)
@pmp('form', ['prox_21m', 'prox_21', 'dual_update_l2'])
@pmp('nband', [3, 9])
def test_prox_exact_branches(amd, dt, form, nband):
    V = vwidth(dt)
    vp, v, w, lam, sigma = planted_inputs(dt, nband, 4 * V + 1)
    got = run_plane(amd, dt, form, vp, v, w, lam, sigma)
    vt = vp + dt(sigma) * v
    if form == 'dual_update_l2':                    # zero norm and below the threshold: v = vt bitwise
        for c in (BELOW, ALL_ZERO):
            assert np.array_equal(bits(got[:, c]), bits(vt[:, c])), (c, got[:, c])
    else:                                           # zero sum (prox_21m) / zero norm, and below the threshold: exactly 0
        for c in (BELOW, ALL_ZERO) + ((ZERO_SUM,) if form == 'prox_21m' else ()):
            assert (got[:, c] == 0).all(), (c, got[:, c])
    assert np.isnan(got[:, NAN_COL]).all()
    ref, bnd = plane_ref(dt, form, vp, v, w, lam, sigma)
    assert_within(got, ref, bnd, form, skip_cols=(NAN_COL,))


# ----------------------------------------------------------------------- 3. two-phase and chunked update
@gpu
@pmp('dt', DTYPES)
def test_dual_update_two_phase(amd, dt):
    """Two ranks on one GPU: 5 bands split 2 + 3, local band sums (k_dual_bandsum), their sum, k_dual_apply<T, true>
    on each part -- against the reference over all 5 bands."""
    nper = 1000
    lam, sigma = rounded(dt, *LAMSIG[1])
    vp, v, w = prox_inputs(dt, 5, nper, seed=3)
    ref, bnd, refo, bndo = dual_refs(dt, vp, v, w, lam, sigma)
    code, st = code_of(amd, dt), amd.dev.stream()
    parts = [slice(0, 2), slice(2, 5)]
    bvp, bv = [Buf(vp[p]) for p in parts], [Buf(v[p]) for p in parts]
    bs = [Buf.out(nper, dt) for _ in parts]
    bo = [Buf.out(vp[p].shape, dt) for p in parts]
    bw = Buf(w)
    for i, p in enumerate(parts):
        ok(amd, amd.lib.pfb_dual_bandsum(code, bvp[i].ptr, bv[i].ptr, sigma, p.stop - p.start, nper, bs[i].ptr, st))
    check_buffers(written=bs, read=bvp + bv)
    total = Buf((bs[0].t + bs[1].t).cpu().numpy())
    for i, p in enumerate(parts):
        ok(amd, amd.lib.pfb_dual_apply(code, bvp[i].ptr, bv[i].ptr, bw.ptr, total.ptr, lam, sigma, p.stop - p.start,
                                        nper, bo[i].ptr, st))
    check_buffers(written=bv + bo, read=bvp + [bw, total])
    for i, p in enumerate(parts):
        assert_within(bv[i].numpy(), ref[p], bnd[p], f"v, part {i}")
        assert_within(bo[i].numpy(), refo[p], bndo[p], f"vp_out, part {i}")


@gpu
@pmp('dt', DTYPES)
def test_dual_update_chunked(amd, dt):
    """The same two steps chunk by chunk, at offsets that are no multiple of the pack width and with band_stride !=
    count: a chunk leaves its neighbours alone, and all three give the whole-plane result."""
    nper, nband = 1000, 5
    lam, sigma = rounded(dt, *LAMSIG[3])
    vp, v, w = prox_inputs(dt, nband, nper, seed=4)
    ref, bnd, refo, bndo = dual_refs(dt, vp, v, w, lam, sigma)
    code, st = code_of(amd, dt), amd.dev.stream()
    bvp, bv, bw, bs, bo = Buf(vp), Buf(v), Buf(w), Buf.out(nper, dt), Buf.out(vp.shape, dt)
    for n, (a, z) in enumerate([(0, 333), (333, 667), (667, 1000)]):
        ok(amd, amd.lib.pfb_dual_bandsum_chunk(code, bvp.at(a), bv.at(a), sigma, nband, z - a, nper, bs.at(a), st))
        ok(amd, amd.lib.pfb_dual_apply_chunk(code, bvp.at(a), bv.at(a), bw.at(a), bs.at(a), lam, sigma, nband, z - a,
                                              nper, bo.at(a), st))
        check_buffers(written=[bv, bs, bo], read=[bvp, bw])
        if n == 0:      # the rest of v is still the input, the rest of vp_out and of the sum plane still sentinel
            assert np.array_equal(bits(bv.numpy()[:, z:]), bits(v[:, z:]))
            assert (bo.numpy()[:, z:] == SENT).all() and (bs.numpy()[z:] == SENT).all()
            assert_within(bv.numpy()[:, :z], ref[:, :z], bnd[:, :z], "v, first chunk")
    assert_within(bv.numpy(), ref, bnd, "v")
    assert_within(bo.numpy(), refo, bndo, "vp_out")
    s64 = (f64(vp) + sigma * f64(v)).sum(axis=0)
    t = (np.abs(f64(vp)) + np.abs(sigma * f64(v))).sum(axis=0)
    assert_within(bs.numpy(), s64, (nband + 1) * float(np.finfo(dt).eps) * t, "band sum")


@gpu
@pmp('dt', DTYPES)
def test_dual_update_argument_checks(amd, dt):
    nper, nband = 64, 2
    vp, v, w = prox_inputs(dt, nband, nper, seed=6)
    code, st, INV = code_of(amd, dt), amd.dev.stream(), amd._lib.PFB_ERR_INVALID
    bvp, bv, bw, bs, bo = Buf(vp), Buf(v), Buf(w), Buf.out(nper, dt), Buf.out(vp.shape, dt)
    everything = [bvp, bv, bw, bs, bo]
    # count = 0: fine, and nothing is written
    assert amd.lib.pfb_dual_bandsum_chunk(code, bvp.ptr, bv.ptr, 1.0, nband, 0, nper, bs.ptr, st) == amd._lib.PFB_OK
    assert amd.lib.pfb_dual_apply_chunk(code, bvp.ptr, bv.ptr, bw.ptr, bs.ptr, 0.5, 1.0, nband, 0, nper, bo.ptr,
                                        st) == amd._lib.PFB_OK
    # bands closer together than the chunk is long
    assert amd.lib.pfb_dual_bandsum_chunk(code, bvp.ptr, bv.ptr, 1.0, nband, 32, 31, bs.ptr, st) == INV
    assert amd.lib.pfb_dual_apply_chunk(code, bvp.ptr, bv.ptr, bw.ptr, bs.ptr, 0.5, 1.0, nband, 32, 31, bo.ptr, st) == INV
    # the l2 forms divide by sigma on the host side of the contract
    assert amd.lib.pfb_prox_21(code, bvp.ptr, bo.ptr, bw.ptr, 0.5, 0.0, nband, nper, st) == INV
    assert amd.lib.pfb_dual_update_l2(code, bvp.ptr, bv.ptr, bw.ptr, 0.5, 0.0, nband, nper, st) == INV
    check_buffers(read=everything)


# -------------------------------------------------------------- 4. prox_21m, prox_21, dual_update_l2
@gpu
@pmp('dt', DTYPES)
@pmp('form', ['prox_21m', 'prox_21', 'dual_update_l2'])
@pmp('nband', [1, 3, 9])
def test_prox_planes(amd, dt, form, nband):
    """Plain grid-stride kernels behind prox_plane_t: one element, a count off every power of two, a second trip of
    the 2048-workgroup grid; then one operand at a time off the 16-byte boundary, through the C ABI and the wrappers."""
    lam, sigma = rounded(dt, *LAMSIG[(nband + len(form)) % 4])
    for nper in (1, 257, 2048 * 256 + 259):
        a, b, w = prox_inputs(dt, nband, nper, seed=nband * 17 + nper)
        ref, bnd = plane_ref(dt, form, a, b, w, lam, sigma)
        assert_within(run_plane(amd, dt, form, a, b, w, lam, sigma), ref, bnd, f"{form}, nper {nper}")
        if nper == 257:
            for which in range(3):
                for off in misalignments(dt):
                    k = tuple(off if i == which else 0 for i in range(3))
                    for via in ('abi', 'py'):
                        assert_within(run_plane(amd, dt, form, a, b, w, lam, sigma, k, via), ref, bnd,
                                      f"{form}, operand {which} + {off}, {via}")


# ------------------------------------------------------------------------------ 5. primal-dual image update
COMBOS = {'g': ('g',), 'g + gsub': ('g', 'gsub'), 'xout_prev': ('xprev',), 'all three': ('xprev', 'g', 'gsub'),
          'g = NULL': ()}


class Primal:
    """One pfb_pd_primal_update[2] call on guarded buffers: x, sums (device doubles, guarded as well) and the raw
    return code."""

    def __init__(self, amd, dt, p, keys, tau, positivity, k=None, second_call=False):
        nband, npix = p['xp'].shape
        k = k or {}
        self.inputs = {n: Buf(p[n], k.get(n, 0)) for n in ('xp', 'xout') + tuple(keys)}
        self.x = Buf.out(p['xp'].shape, dt, k.get('x', 0))
        self.sums = Buf.out(3, np.float64)
        ws = amd.dev.scratch()[0]
        ptr = {n: (self.inputs[n].ptr if n in self.inputs else None) for n in ('xp', 'xout', 'xprev', 'g', 'gsub')}
        code, st = code_of(amd, dt), amd.dev.stream()
        for _ in range(2 if second_call else 1):
            if 'xprev' in keys or 'gsub' in keys:
                self.rc = amd.lib.pfb_pd_primal_update2(code, ptr['xp'], ptr['xout'], ptr['xprev'], ptr['g'],
                                                        ptr['gsub'], tau, positivity, nband, npix, self.x.ptr,
                                                        self.sums.ptr, ws.data_ptr(), st)
            else:
                self.rc = amd.lib.pfb_pd_primal_update(code, ptr['xp'], ptr['xout'], ptr['g'], tau, positivity, nband,
                                                       npix, self.x.ptr, self.sums.ptr, ws.data_ptr(), st)
            check_buffers(written=[self.x, self.sums], read=list(self.inputs.values()))
            self.first_sums, self.got_sums = getattr(self, 'got_sums', None), self.sums.numpy().copy()
        self.got = self.x.numpy()


def check_primal(dt, p, keys, tau, positivity, run, what, planted_col=None):
    """x against the reference within the per-element bound; the positivity branches exactly; the three sums."""
    eps = float(np.finfo(dt).eps)
    a = {n: (p[n] if n in keys else None) for n in ('xprev', 'g', 'gsub')}
    ref, raw = ref_primal(f64(p['xp']), f64(p['xout']), f64(a['xprev']), f64(a['g']), f64(a['gsub']), tau, positivity)
    bnd = bound_primal(p['xp'], p['xout'], a['xprev'], a['g'], a['gsub'], tau, eps)
    got = run.got
    skip = ()
    if positivity == 1:                 # clearly negative in the reference: exactly zero
        neg = raw < -bnd
        assert (got[neg] == 0).all(), f"{what}: positivity 1 left a negative element non-zero"
    if positivity == 2:                 # the kill decision equals the reference's wherever the bound can tell
        tied = tied_columns(raw, bnd)
        if planted_col is not None:
            tied[planted_col] = False
        assert tied.mean() <= TIE_CAP, f"{what}: {tied.mean():.2e} of the columns tied"
        killed_ref = np.any(raw <= 0, axis=0)
        killed_got = np.all(got == 0, axis=0)
        decided = ~tied
        assert np.array_equal(killed_got[decided], killed_ref[decided]), f"{what}: kill decisions differ"
        assert (got[:, killed_ref & decided] == 0).all()
        skip = tuple(np.nonzero(tied)[0])
    assert_within(got, ref, bnd, what, skip_cols=skip)
    g64, xp64 = f64(got), f64(p['xp'])
    s0, s1 = float(np.sum((g64 - xp64) ** 2)), float(np.sum(g64 ** 2))
    assert abs(run.got_sums[0] - s0) <= TOL_SUM * s0 + 1e-300, (what, run.got_sums, s0)
    assert abs(run.got_sums[1] - s1) <= TOL_SUM * s1 + 1e-300, (what, run.got_sums, s1)
    assert (run.got_sums[2] != 0) == bool(np.any(got != 0)), (what, run.got_sums)
    if run.first_sums is not None:      # deterministic: a second call on the same input, bitwise the same sums
        assert np.array_equal(bits(run.first_sums), bits(run.got_sums)), what


def primal_sizes(dt):
    """One pack; a count off every power of two (the V = 1 form); beyond the 1024-workgroup cap of the 16-byte form and
    of the V = 1 form."""
    V = vwidth(dt)
    return [V, 257, (1024 * 256 + 19) * V, 1024 * 256 + 19]


@gpu
@pmp('dt', DTYPES)
@pmp('nband', [1, 3])
@pmp('size', range(4))
@pmp('positivity', [0, 1, 2])
def test_pd_primal_update(amd, dt, nband, size, positivity):
    npix = primal_sizes(dt)[size]
    p = primal_inputs(dt, nband, npix, seed=nband * 10 + size)
    tau, = rounded(dt, 0.37)
    for name, keys in COMBOS.items():
        run = Primal(amd, dt, p, keys, tau, positivity, second_call=(name == 'all three'))
        assert run.rc == amd._lib.PFB_OK
        check_primal(dt, p, keys, tau, positivity, run, f"{name}, npix {npix}")


@gpu
@pmp('dt', DTYPES)
def test_pd_primal_update_misaligned_operand(amd, dt):
    """A count that would take the 16-byte form with one pointer off the boundary: k_pd_primal_vec<T, 1>."""
    V = vwidth(dt)
    nband, npix = 3, 65 * V
    p = primal_inputs(dt, nband, npix, seed=21)
    tau, = rounded(dt, 0.61)
    keys = COMBOS['all three']
    for positivity in (0, 1, 2):
        for which in ('xp', 'xout', 'xprev', 'g', 'gsub', 'x'):
            for off in misalignments(dt):
                run = Primal(amd, dt, p, keys, tau, positivity, k={which: off})
                assert run.rc == amd._lib.PFB_OK
                check_primal(dt, p, keys, tau, positivity, run, f"{which} + {off}, positivity {positivity}")


@gpu
@pmp('dt', DTYPES)
def test_pd_primal_update_argument_checks(amd, dt):
    p = primal_inputs(dt, 2, 64, seed=22)
    run = Primal(amd, dt, p, ('gsub',), 0.5, 0)         # gsub without g
    assert run.rc == amd._lib.PFB_ERR_INVALID
    assert (run.got == SENT).all() and (run.got_sums == SENT).all()


@gpu
@pmp('dt', DTYPES)
@pmp('positivity', [1, 2])
@pmp('vec', [True, False])
@pmp('combo', ['g', 'all three'])
def test_pd_primal_update_exact_zero(amd, dt, positivity, vec, combo):
    """xp = 1.5, tau = 0.5, xout = 1, g = 2 (all three: 2 xout - xout_prev = 1, g - gsub = 2) gives exactly 0 with or
    without FMA, inside a pack whose other elements are clearly positive.  positivity 2 tests `<= 0`: the whole column
    goes; positivity 1 tests `< 0`: the element is 0 anyway and its neighbours are untouched."""
    V = vwidth(dt)
    nband, npix, col = 3, 4 * V + (0 if vec else 1), 2
    rng = np.random.default_rng(30 + positivity)
    p = {k: (rng.random((nband, npix)) - 0.5).astype(dt) for k in ('xout', 'xprev', 'g', 'gsub')}
    p['xp'] = (5.0 + rng.random((nband, npix))).astype(dt)
    p['xp'][1, col], p['xout'][1, col], p['xprev'][1, col], p['g'][1, col], p['gsub'][1, col] = 1.5, 1.0, 1.0, 3.0, 1.0
    if combo == 'g':
        p['g'][1, col] = 2.0
    keys = COMBOS[combo]
    run = Primal(amd, dt, p, keys, 0.5, positivity)
    assert run.rc == amd._lib.PFB_OK
    check_primal(dt, p, keys, 0.5, positivity, run, combo, planted_col=col)
    if positivity == 2:
        assert (run.got[:, col] == 0).all()
    else:
        assert run.got[1, col] == 0 and (run.got[[0, 2], col] > 3).all()
    assert (np.delete(run.got, col, axis=1) > 3).all()
    assert run.got_sums[2] != 0


@gpu
@pmp('dt', DTYPES)
@pmp('vec', [True, False])
def test_pd_primal_update_all_zero(amd, dt, vec):
    """positivity 1 zeroes every element: sums[2] (and sums[1]) are exactly 0, sums[0] = |xp|^2."""
    V = vwidth(dt)
    nband, npix = 2, 300 * V + (0 if vec else 1)
    rng = np.random.default_rng(40)
    p = {'xp': (-1.0 - rng.random((nband, npix))).astype(dt), 'xout': rng.random((nband, npix)).astype(dt),
         'g': rng.random((nband, npix)).astype(dt)}
    run = Primal(amd, dt, p, ('g',), 0.5, 1)
    assert run.rc == amd._lib.PFB_OK
    assert (run.got == 0).all()
    assert run.got_sums[2] == 0 and run.got_sums[1] == 0
    check_primal(dt, p, ('g',), 0.5, 1, run, "all zero")


# --------------------------------------------------------------------------- 7. the scalar PCG kernels
def relerr(a, ref):
    a, ref = f64(a), f64(ref)
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300)


def cdt(rdt):
    return np.complex64 if rdt == np.float32 else np.complex128


def odd_problem():
    """45 x 33 pixels (odd per band and over the cube) on a 90 x 66 PSF grid, 3 bands: a valid real PSF, a beam, a
    right-hand side in the range of the operator plus noise."""
    nx, ny, P, Q, nb = 45, 33, 90, 66, 3
    rng = np.random.default_rng(nx + P)
    u = np.fft.fftfreq(P)[:, None]
    v = np.fft.rfftfreq(Q)[None, :]
    W = rng.poisson(4 * np.exp(-(u ** 2 + v ** 2) / (2 * 0.12 ** 2)), size=(nb, P, Q // 2 + 1)).astype(np.float64)
    W /= nb * np.fft.irfft2(W, s=(P, Q)).max(axis=(1, 2))[:, None, None]
    psfhat = ofc.psfhat_from_psf(np.fft.fftshift(np.fft.irfft2(W, s=(P, Q)), axes=(1, 2)))
    x = rng.standard_normal((nb, nx, ny))
    beam = 0.5 + rng.random((nb, nx, ny))
    xpad, xhat, xout = ofc.make_scratch(psfhat, Q, x.shape, np.float64)
    b = ofc.psf_convolve_cube(xpad, xhat, xout, psfhat, Q, x).copy() + 0.01 * rng.standard_normal(x.shape)
    return dict(psfhat=psfhat, b=b, beam=beam, sigmainv=0.05, Q=Q)


_problems = {}


def pcg_problem(name, golden):
    """The problem and its oracle solutions, computed once: ref[(cube | bands, beam, backtrack)] = (x, r)."""
    if name in _problems:
        return _problems[name]
    if name == 'odd':
        pr = odd_problem()
    else:
        g = golden('pcg')
        pr = dict(psfhat=g['psfhat'], b=g['b'], beam=g['beam'], sigmainv=float(g['sigmainv']), Q=int(g['Q']))
    psfhat, b, Q, sig = pr['psfhat'], pr['b'], pr['Q'], pr['sigmainv']
    nb = b.shape[0]
    cube = ofc.make_scratch(psfhat, Q, b.shape, np.float64)
    band = ofc.make_scratch(psfhat[0], Q, b.shape[1:], np.float64)
    kw = dict(M=lambda t: t / sig, tol=0.0, maxit=8, minit=8, return_resid=True)
    pr['ref'], pr['A'] = {}, {}
    for with_beam in (False, True):
        beam = pr['beam'] if with_beam else None

        def A_cube(t, beam=beam):
            return ofc.hessian_psf_cube(*cube, beam, psfhat, Q, t, sigmainv=sig).copy()

        def A_band(t, k, beam=beam):
            return ofc._hessian_psf_slice(*band, psfhat[k], None if beam is None else beam[k], Q, t, sigmainv=sig).copy()

        def A_bands(t, A_band=A_band):
            return np.stack([A_band(t[k], k) for k in range(nb)])
        pr['A'][('cube', with_beam)], pr['A'][('bands', with_beam)] = A_cube, A_bands
        for bt in (0, 2):
            pr['ref'][('cube', with_beam, bt)] = osv.pcg(A_cube, b, None, backtrack=bool(bt), **kw)
            per = [osv.pcg(lambda t, k=k: A_band(t, k), b[k], None, backtrack=bool(bt), **kw) for k in range(nb)]
            pr['ref'][('bands', with_beam, bt)] = (np.stack([q[0] for q in per]), np.stack([q[1] for q in per]))
        pr['ref'][('cube', with_beam, 1)] = pr['ref'][('cube', with_beam, 2)]      # the exact loop: the same reference
    _problems[name] = pr
    return pr


def native_solve(amd, plan, kind, rdt, b, beam, sig, bt, k=0):
    """pfb_pcg_solve (kind 'cube') / pfb_pcg_solve_bands straight through the C ABI: x0 = 0, tol 0, maxit = minit = 8.
    k: element offset of x, b and r_out.  Returns (x, r, [results])."""
    nb = b.shape[0]
    bb, bx, br = Buf(b.astype(rdt), k), Buf(np.zeros(b.shape, rdt), k), Buf.out(b.shape, rdt, k)
    bbeam = None if beam is None else Buf(beam.astype(rdt))
    bands = kind == 'bands'
    nbytes = (amd.lib.pfb_pcg_bands_work_bytes if bands else amd.lib.pfb_pcg_work_bytes)(plan.handle, nb)
    work = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    assert work.data_ptr() % 256 == 0
    res = (amd._lib.PcgResult * nb)()
    head = (0, nb, bb.ptr, bx.ptr, br.ptr, None if bbeam is None else bbeam.ptr, 0.0, sig, sig, 0.0, 8, 8, bt,
            work.data_ptr())
    if bands:
        plan.run('pfb_pcg_solve_bands', *head, res)
    else:
        plan.run('pfb_pcg_solve', *head, amd._lib.ALLREDUCE_FN(0), None, C.byref(res[0]))
    check_buffers(written=[bx, br], read=[bb] + ([bbeam] if bbeam is not None else []))
    return bx.numpy(), br.numpy(), [(r.status, r.iters, r.matvecs, r.backtracks) for r in res[:nb if bands else 1]]


@gpu
@pmp('rdt', DTYPES)
@pmp('kind', ['cube', 'bands'])
@pmp('name', ['odd', 'golden'])
def test_pcg_scalar_kernels(amd, golden, monkeypatch, rdt, kind, name):
    """The V = 1 forms of the PCG vector kernels, which only the C ABI reaches (the Python layer clones x0 into an
    aligned buffer, and every other PCG test has a pixel count that is a multiple of the pack width):
      odd    -- a pixel count per band (and per cube) that is odd, on a non-embedded generic plan;
      golden -- tests/golden/pcg.npz (48 x 40) with x, b and r_out one element off the 16-byte boundary, also against
                the aligned solve of the same problem (the 16-byte kernels): same counters, x and r to TOL_PCG.
    backtrack 0 and 2 (the sync-free driver: k_pcg_init<T, 1>, k_pcg_update_dir<T, 1, ..>) and, for the cube solve
    (pfb_pcg_solve_bands has no exact loop), backtrack 1: the host-driven loop, which picks the form per launch while x
    and its alternate in `work` swap roles -- k_pcg_update<T, 1> on both problems, k_pcg_dir<T, 1> on the odd one (p
    and r live in `work`, aligned: the golden cube's 5760 elements take the 16-byte k_pcg_dir).  With and without a
    beam, against oracle.solvers.pcg; r_out is A x - b recomputed with the oracle, to TOL_PCG of max|A x - b|."""
    monkeypatch.setenv('PFB_NO_EMBED', '1')
    pr = pcg_problem(name, golden)
    b, sig = pr['b'], pr['sigmainv']
    nx, ny = b.shape[1:]
    assert name != 'odd' or (nx * ny) % 2 == 1
    plan = amd.psf.PsfConvPlan(pr['psfhat'].astype(cdt(rdt)), nx, ny, pr['Q'])
    assert plan.embed is None and not plan.fast_path
    tol = TOL_PCG[rdt]
    for with_beam in (False, True):
        beam = pr['beam'] if with_beam else None
        for bt in ((0, 1, 2) if kind == 'cube' else (0, 2)):
            what = (name, kind, with_beam, bt)
            xo = pr['ref'][(kind, with_beam, bt)][0]
            x, r, res = native_solve(amd, plan, kind, rdt, b, beam, sig, bt, k=0 if name == 'odd' else 1)
            r_again = pr['A'][(kind, with_beam)](f64(x)) - f64(b.astype(rdt))
            print(what, f"x relerr {relerr(x, xo):.2e} r_out relerr {relerr(r, r_again):.2e} "
                  f"max|r| / max|b| {np.abs(r_again).max() / np.abs(b).max():.2e}", res)
            assert relerr(x, xo) < tol, what
            assert all(q[1] == 8 and q[2] == 9 for q in res), (what, res)
            assert relerr(r, r_again) < tol, what
            if name == 'golden':
                xa, ra, resa = native_solve(amd, plan, kind, rdt, b, beam, sig, bt, k=0)
                assert res == resa, (what, res, resa)
                assert relerr(x, xa) < tol and relerr(r, ra) < tol, what
    plan.close()
