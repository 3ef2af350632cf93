"""
Case table of the coverage FFT paths (tests/test_cpu_coverage_cases.py, tests/test_gpu_coverage_edges.py): the
one-workgroup-per-line Stockham FFT in LDS (csrc/fft_generic.hpp), the same passes as global-memory launches
(csrc/fft_long.hpp) and the stage entries of csrc/fftconv.hip around them.

Every case names an entry point ('producer': pfb_psfhat_from_psf, 'regrid': pfb_psfhat_regrid, 'apply': a coverage plan
of pfb_psfconv_plan_create and the three apply entries), its sizes, the number formats it runs in and the PROPERTY IT
EXISTS FOR: a predicate over the mirror below of the library's bookkeeping (plan_factors, line_fits_lds, the plan's
long_lines rule, long_grid, the pass count of long_fft).  The predicates are asserted on the CPU, so a case cannot
silently stop exercising its edge when a limit or the factor order changes, and the CPU module builds from the table the
matrix {radix} x {LDS, global} x {rows, columns} x {forward, inverse} x {fp32, fp64} x {p == 1, p > 1} of the passes
that run.

Sizes per entry point:
  producer  (P, Q)                    psf (nband, P, Q) -> psfhat (nband, P, Q/2 + 1)
  regrid    (nx, ny, P, Q, P2, Q2)    psfhat on (P, Q) -> psfhat2 on (P2, Q2) for images of (nx, ny)
  apply     (nx, ny, P, Q)            images (nband, nx, ny) on a (P, Q) PSF grid
M = Q / 2 is the length of a row transform (real rows run as packed complex transforms), P that of a column transform.

Groups: (a) each radix alone, (b) repeated and mixed radices, (c) the LDS boundary and the global passes, (d) the grid
caps, (e) the regrid rule at tiny sizes, (f) the epilogue and the reductions of `apply`.

Not in the table: the 65536-workgroup cap of long_fft.  A pass strides only above 65536 * 256 = 16.7 M butterflies, a
batch of more than 33 M complex values with its copy beside it; no test of a few seconds reaches it.

Plain Python, numpy and scipy: no GPU and no torch.  The references are float64.
"""
import numpy as np
import scipy.fft as sfft

from oracle import fftconv as ofc

F32, F64 = 'float32', 'float64'
DTYPES = (F32, F64)
CSZ = {F32: 8, F64: 16}                 # bytes of one complex value
LDS_BYTES = 160 * 1024                  # dynamic LDS of one gfx950 workgroup
RADICES = (2, 3, 4, 5, 7, 11, 13)


# ------------------------------------------------------------------------------------------------- bookkeeping mirror
def plan_factors(n):
    """csrc/fft_generic.hpp plan_factors: the radices of the passes in the order they run (4s first, then 2, 3, 5, 7, 11,
    13), or None when n has a prime factor above 13."""
    out, m = [], n
    while m % 4 == 0:
        out.append(4)
        m //= 4
    for p in (2, 3, 5, 7, 11, 13):
        while m % p == 0:
            out.append(p)
            m //= p
    return out if m == 1 and len(out) <= 24 else None


def passes(n):
    """[(radix, p)] of the transform of length n: p is the product of the radices already done."""
    out, p = [], 1
    for r in plan_factors(n):
        out.append((r, p))
        p *= r
    return out


def line_fits_lds(n, dtype):
    """csrc/fftconv.hip line_fits_lds<T>: the two ping-pong buffers of a line of n complex values fit the LDS."""
    return 2 * CSZ[dtype] * n <= LDS_BYTES


def long_lines(P, M, dtype):
    """pfb_psfconv_plan_create: a coverage plan runs every transform as global passes.  128 B beside the two buffers are
    kept for the block sums of k_rows_c2r, so a line that fills the LDS exactly is already long here."""
    return 128 + 2 * CSZ[dtype] * max(P, M) > LDS_BYTES


def long_grid(n):
    """csrc/fft_long.hpp long_grid: workgroups of 256 threads along a line of n elements, capped at 64."""
    return min(64, max(1, -(-n // 256)))


def long_grid_strides(n):
    return n > long_grid(n) * 256


def npass(n):
    return len(plan_factors(n))


def copies_back(n):
    """long_fft ping-pongs between data and work: after an odd number of passes the result is in work and is copied."""
    return npass(n) % 2 == 1


COL_MUL_GRID = 4096 * 256               # k_long_col_mul's fixed launch: threads of one sweep


def is_smooth(n):
    return n >= 1 and plan_factors(n) is not None


def next_smooth(n, even_half=False):
    """Smallest 13-smooth length >= n; with even_half the smallest even length >= n whose half is 13-smooth."""
    m = n
    while True:
        if (m % 2 == 0 and is_smooth(m // 2)) if even_half else is_smooth(m):
            return m
        m += 1


# ------------------------------------------------------------------------------------------------- cases
class Case:
    def __init__(self, group, name, entry, nband, dims, prop, dtypes=DTYPES, why='', nonherm=False):
        self.group, self.name, self.entry, self.nband, self.dims = group, name, entry, nband, tuple(dims)
        self.prop, self.dtypes, self.why, self.nonherm = prop, tuple(dtypes), why, nonherm

    @property
    def id(self):
        return f"{self.group}-{self.name}"

    def holds(self, dtype):
        return bool(self.prop(self, dtype))

    def transforms(self, dtype):
        """[(length, 'lds' | 'global', 'rows' | 'cols', 'fwd' | 'inv')] in the order the entry point runs them."""
        mem = lambda n: 'lds' if line_fits_lds(n, dtype) else 'global'      # noqa: E731
        if self.entry == 'producer':
            P, Q = self.dims
            return [(Q // 2, mem(Q // 2), 'rows', 'fwd'), (P, mem(P), 'cols', 'fwd')]
        if self.entry == 'regrid':
            _, _, P, Q, P2, Q2 = self.dims
            return [(P, mem(P), 'cols', 'inv'), (Q // 2, mem(Q // 2), 'rows', 'inv'),
                    (Q2 // 2, mem(Q2 // 2), 'rows', 'fwd'), (P2, mem(P2), 'cols', 'fwd')]
        _, _, P, Q = self.dims
        m = 'global' if long_lines(P, Q // 2, dtype) else 'lds'
        return [(Q // 2, m, 'rows', 'fwd'), (P, m, 'cols', 'fwd'), (P, m, 'cols', 'inv'), (Q // 2, m, 'rows', 'inv')]

    def cells(self, dtype):
        """The cells of the coverage matrix this case runs in `dtype`."""
        return {(r, mem, orient, direction, dtype, 'p1' if p == 1 else 'pn')
                for n, mem, orient, direction in self.transforms(dtype) for r, p in passes(n)}

    def lengths(self):
        if self.entry == 'producer':
            P, Q = self.dims
            return [P, Q // 2]
        if self.entry == 'regrid':
            _, _, P, Q, P2, Q2 = self.dims
            return [P, Q // 2, P2, Q2 // 2]
        return [self.dims[2], self.dims[3] // 2]

    def __repr__(self):
        return f"Case({self.id}: {self.entry} nband {self.nband} {self.dims})"


# ---- predicates
def runs(length, mem=None, orient=None, direction=None):
    """A transform of `length` runs, in that memory / orientation / direction where given."""
    def prop(case, dtype):
        return any(n == length and mem in (None, m) and orient in (None, o) and direction in (None, d)
                   for n, m, o, d in case.transforms(dtype))
    return prop


def p_single_pass(length, orient):
    """`length` is one radix (or 1: no pass at all) and runs along `orient` in LDS."""
    def prop(case, dtype):
        return npass(length) <= 1 and runs(length, 'lds', orient)(case, dtype)
    return prop


def p_twiddled(length, orient, direction):
    """`length` has a pass with p > 1 and runs along `orient` in `direction`."""
    def prop(case, dtype):
        return npass(length) >= 2 and runs(length, None, orient, direction)(case, dtype)
    return prop


def p_fills_lds(length, orient):
    """The line uses all 160 KB: it fits, one element more would not."""
    def prop(case, dtype):
        return (2 * CSZ[dtype] * length == LDS_BYTES and line_fits_lds(length, dtype)
                and not line_fits_lds(length + 1, dtype) and runs(length, 'lds', orient)(case, dtype))
    return prop


def p_regrid_mems(cl, rl, rl2, cl2):
    """pfb_psfhat_regrid's four choices: True = in LDS."""
    def prop(case, dtype):
        return [m == 'lds' for _, m, _, _ in case.transforms(dtype)] == [cl, rl, rl2, cl2]
    return prop


def p_long_both(length, orient, parity):
    """`length` runs as global passes in both directions along `orient`, with an odd / even number of passes; the odd
    ones with two bands or more, so that the copy back of band b runs before band b + 1 is transformed."""
    def prop(case, dtype):
        return (all(runs(length, 'global', orient, d)(case, dtype) for d in ('fwd', 'inv'))
                and copies_back(length) == (parity == 'odd') and (parity == 'even' or case.nband >= 2))
    return prop


def p_apply_long_but_fits(case, dtype):
    """The plan's 128 B turn a line that line_fits_lds admits into a long_lines plan."""
    _, _, P, Q = case.dims
    n = max(P, Q // 2)
    return line_fits_lds(n, dtype) and long_lines(P, Q // 2, dtype) and 2 * CSZ[dtype] * n == LDS_BYTES


def p_apply(long, also=lambda c, d: True):
    def prop(case, dtype):
        _, _, P, Q = case.dims
        return long_lines(P, Q // 2, dtype) == long and also(case, dtype)
    return prop


def p_col_mul(above):
    """(M + 1) P against the threads of k_long_col_mul's one sweep, on a long_lines plan."""
    def prop(case, dtype):
        _, _, P, Q = case.dims
        n = (Q // 2 + 1) * P
        return long_lines(P, Q // 2, dtype) and (n > COL_MUL_GRID if above else 0.95 * COL_MUL_GRID < n < COL_MUL_GRID)
    return prop


def p_regrid_shape(check):
    return lambda case, dtype: bool(check(*case.dims))


# ---- the table
# (b) repeated and mixed radices.  5005 = 5 7 11 13 fits the fp64 LDS, 9240 = 4 2 3 5 7 11 the fp32 LDS only
MIXED = (8, 9, 16, 25, 49, 121, 169, 52, 91, 143, 385, 1001, 5005, 9240)
# (c, d) lines beyond the LDS in both formats: (length, parity of the pass count, what it adds)
LONG = ((10780, 'odd', '4 5 7 7 11: radix 7 with p > 1 over its own radix'),
        (10530, 'odd', '2 3 3 3 3 5 13: seven passes, radix 2 first'),
        (11011, 'even', '7 11 11 13: radix 7 first, radix 11 with k over its own radix'),
        (10296, 'even', '4 2 3 3 11 13: among the first lengths above the fp32 limit'),
        (10395, 'even', '3 3 3 5 7 11: radix 3 first'),
        (11375, 'odd', '5 5 5 7 13: radix 5 first'),
        (14641, 'even', '11 11 11 11: radix 11 first'),
        (28561, 'even', '13 13 13 13: radix 13 first; above 16384, the row kernels stride'),
        (10400, 'even', '4 4 2 5 5 13: radix 4 with p > 1'),
        (16500, 'even', '4 3 5 5 5 11: above 16384, the row kernels stride'),
        (16562, 'odd', '2 7 7 13 13: above 16384, odd pass count'))
LDS_FULL = {F32: 10240, F64: 5120}
JUST_ABOVE = {F32: (10290, 10296), F64: (5145, 5148)}       # 2 3 5 7^3, 2^3 3^2 11 13 | 3 5 7^3, 2^2 3^2 11 13


def half(n):
    """The largest image length whose offsets a grid of n holds (n >= 2 half - 1): they reach every sample of a source
    line of up to n values, so an error anywhere in its inverse transform shows in the result."""
    return (n + 1) // 2


def _cases():
    out = []

    def add(*a, **k):
        out.append(Case(*a, **k))

    # a. each radix alone: one pass, no twiddles (length 1: no pass)
    for n in (1, 2, 3, 4, 5, 7, 11, 13):
        add('a', f'rows-{n}', 'producer', 2, (3, 2 * n), p_single_pass(n, 'rows'))
        add('a', f'cols-{n}', 'producer', 2, (n, 6), p_single_pass(n, 'cols'))
    # b. repeated and mixed radices along rows and down columns, forward (producer) and inverse (the source grid of a
    # regrid whose image is large enough for its offsets to reach every sample of the source line)
    for n in MIXED:
        add('b', f'prod-rows-{n}', 'producer', 2, (2, 2 * n), p_twiddled(n, 'rows', 'fwd'))
        add('b', f'prod-cols-{n}', 'producer', 2, (n, 4), p_twiddled(n, 'cols', 'fwd'))
        h = half(n)                                             # offsets up to +-(h - 1): (nearly) every sample of the line
        add('b', f'regrid-rows-{n}', 'regrid', 2, (2, n, 4, 2 * n, 3, next_smooth(2 * n - 1, True)),
            p_twiddled(n, 'rows', 'inv'))
        add('b', f'regrid-cols-{n}', 'regrid', 2, (h, 2, n, 4, next_smooth(2 * h - 1), 4), p_twiddled(n, 'cols', 'inv'))
    # c. the LDS boundary: a line that fills the LDS exactly, in the producer and as source and target of the regrid with
    # the first 13-smooth lengths above it on the other side; the same line makes a long_lines plan
    for d in DTYPES:
        n, (up7, up13) = LDS_FULL[d], JUST_ABOVE[d]
        t = d[-2:]
        add('c', f'prod-rows-{n}-f{t}', 'producer', 2, (2, 2 * n), p_fills_lds(n, 'rows'), dtypes=(d,))
        add('c', f'prod-cols-{n}-f{t}', 'producer', 2, (n, 4), p_fills_lds(n, 'cols'), dtypes=(d,))
        add('c', f'prod-rows-{up7}-f{t}', 'producer', 2, (2, 2 * up7), runs(up7, 'global', 'rows'), dtypes=(d,))
        add('c', f'prod-cols-{up13}-f{t}', 'producer', 2, (up13, 4), runs(up13, 'global', 'cols'), dtypes=(d,))
        add('c', f'regrid-cols-{n}-{up7}-f{t}', 'regrid', 3, (half(n), 2, n, 4, up7, 6),
            p_regrid_mems(True, True, True, False), dtypes=(d,), why='source columns fill the LDS, target columns long')
        add('c', f'regrid-cols-{up13}-{n}-f{t}', 'regrid', 1, (half(n), 2, up13, 4, n, 6),
            p_regrid_mems(False, True, True, True), dtypes=(d,), why='source columns long, target columns fill the LDS')
        add('c', f'regrid-rows-{n}-{up13}-f{t}', 'regrid', 1, (2, n, 4, 2 * n, 6, 2 * up13),
            p_regrid_mems(True, True, False, True), dtypes=(d,), why='source rows fill the LDS, target rows long')
        add('c', f'regrid-rows-{up7}-{n}-f{t}', 'regrid', 3, (2, n, 4, 2 * up7, 6, 2 * n),
            p_regrid_mems(True, False, True, True), dtypes=(d,), why='source rows long, target rows fill the LDS')
        add('c', f'apply-cols-{n}-f{t}', 'apply', 2, (3, 2, n, 4), p_apply_long_but_fits, dtypes=(d,))
        add('c', f'apply-rows-{n}-f{t}', 'apply', 2, (2, 5, 3, 2 * n), p_apply_long_but_fits, dtypes=(d,))
    # c / d. global passes in both formats, both orientations and both directions: every radix, first and later passes,
    # both parities of the pass count (two bands), three lengths above 16384
    for n, parity, why in LONG:
        add('c' if n <= 16384 else 'd', f'regrid-rows-{n}', 'regrid', 2, (2, n, 4, 2 * n, 3, 2 * n),
            p_long_both(n, 'rows', parity), why=why)
        add('c' if n <= 16384 else 'd', f'regrid-cols-{n}', 'regrid', 2, (half(n), 3, n, 6, n, 8),
            p_long_both(n, 'cols', parity), why=why)
    # d. the grid caps.  long_grid: 64 workgroups a line, so the row kernels (pack, post, pre, finish) and the column
    # load / store of a long_lines plan stride above 16384 elements
    add('d', 'prod-rows-16500', 'producer', 2, (2, 33000), lambda c, d: long_grid_strides(16500) and runs(16500, 'global', 'rows')(c, d))
    add('d', 'apply-rows-16500', 'apply', 1, (2, 16450, 2, 33000),
        p_apply(True, lambda c, d: long_grid_strides(16500) and c.dims[1] > 16384), why='pack, post, pre stride; finish: one workgroup')
    add('d', 'apply-cols-16562', 'apply', 1, (16500, 1, 16562, 2),
        p_apply(True, lambda c, d: long_grid_strides(16562) and long_grid_strides(c.dims[0])),
        why='k_long_col_load / _store stride; 16500 row partials')
    add('d', 'apply-colmul-above', 'apply', 1, (3, 5, 5120, 416), p_col_mul(True), dtypes=(F64,),
        why='209 x 5120 = 1 070 080 elements: k_long_col_mul strides')
    add('d', 'apply-colmul-below', 'apply', 1, (3, 5, 5120, 400), p_col_mul(False), dtypes=(F64,),
        why='201 x 5120 = 1 029 120 elements: one sweep')
    # e. the regrid rule, tiny
    add('e', '2x-larger', 'regrid', 3, (4, 5, 8, 10, 12, 16),
        p_regrid_shape(lambda nx, ny, P, Q, P2, Q2: (P, Q) == (2 * nx, 2 * ny) and P2 > P and Q2 > Q))
    add('e', 'full-wrap-smallest', 'regrid', 1, (6, 8, 6, 8, 11, 16),
        p_regrid_shape(lambda nx, ny, P, Q, P2, Q2: (P, Q) == (nx, ny) and P2 == 2 * nx - 1 and is_smooth(P2)
                       and Q2 == next_smooth(2 * ny - 1, True)),
        why='P = nx, Q = ny; the smallest target the entry accepts')
    add('e', 'odd-P-between', 'regrid', 3, (5, 4, 7, 6, 9, 8),
        p_regrid_shape(lambda nx, ny, P, Q, P2, Q2: P % 2 == 1 and nx < P < 2 * nx and P2 == 2 * nx - 1))
    add('e', 'P-above-2nx', 'regrid', 1, (3, 2, 15, 12, 5, 4),
        p_regrid_shape(lambda nx, ny, P, Q, P2, Q2: P > 2 * nx and Q > 2 * ny and P2 < P and Q2 < Q),
        why='target smaller than the source')
    # f. apply on coverage plans.  LDS form: ny parity, ny = 1, nx = 1, no padding, nx nb = 1, < 64, > 256
    lds = lambda chk: p_apply(False, chk)       # noqa: E731
    add('f', 'lds-1x1', 'apply', 1, (1, 1, 1, 2), lds(lambda c, d: c.nband * c.dims[0] == 1 and c.lengths() == [1, 1]))
    add('f', 'lds-odd-ny', 'apply', 2, (5, 7, 9, 14), lds(lambda c, d: c.dims[1] % 2 == 1 and c.nband * c.dims[0] < 64))
    add('f', 'lds-even-ny', 'apply', 3, (6, 6, 10, 12), lds(lambda c, d: c.dims[1] % 2 == 0 and c.nband == 3),
        why='three bands: the band sub-ranges; P = 10, M = 6 start with radix 2')
    add('f', 'lds-no-padding', 'apply', 3, (10, 13, 10, 26), lds(lambda c, d: c.dims[0] == c.dims[2]), why='P = nx')
    add('f', 'lds-circular', 'apply', 2, (10, 12, 10, 12), lds(lambda c, d: c.dims[:2] == c.dims[2:]), why='P = nx, Q = ny')
    add('f', 'lds-ny1', 'apply', 2, (7, 1, 14, 2), lds(lambda c, d: c.dims[1] == 1))
    add('f', 'lds-nx1', 'apply', 2, (1, 9, 1, 18), lds(lambda c, d: c.dims[0] == 1 and c.dims[2] == 1))
    add('f', 'lds-270-rows', 'apply', 3, (90, 3, 91, 6), lds(lambda c, d: c.nband * c.dims[0] > 256),
        why='k_sum_partials strides over 270 partials, k_sum_partials_bands over 90')
    add('f', 'lds-nonhermitian', 'apply', 2, (5, 6, 11, 12), lds(lambda c, d: c.nonherm), nonherm=True,
        why='imaginary parts of the DC and Nyquist bins are dropped, here as in the oracle')
    # long form
    add('f', 'long-f64-2574', 'apply', 3, (2574, 2, 5148, 4), p_apply(True, lambda c, d: c.nband * c.dims[0] > 256),
        dtypes=(F64,))
    add('f', 'long-f32-rows', 'apply', 3, (3, 300, 4, 2 * 10296), p_apply(True, lambda c, d: c.dims[1] > 256), dtypes=(F32,),
        why="ny = 300: k_long_finish's one workgroup strides along the row")
    add('f', 'long-nonhermitian', 'apply', 2, (3, 4, 5148, 8), p_apply(True, lambda c, d: c.nonherm), dtypes=(F64,), nonherm=True)
    return out


CASES = _cases()
RUN_CASES = [c for c in CASES if c.dtypes]


def wraps(case):
    """regrid: the old grid is too small for the image, so that its convolution wraps around."""
    nx, ny, P, Q = case.dims[:4]
    return P < 2 * nx - 1 or Q < 2 * ny - 1


def by_id(cid):
    return next(c for c in CASES if c.id == cid)


def run_params(entry):
    """(case, dtype) pairs of one entry point, for pytest.mark.parametrize."""
    return [(c, d) for c in RUN_CASES if c.entry == entry for d in c.dtypes]


# ------------------------------------------------------------------------------------------------- the coverage matrix
def matrix():
    """cell -> ids of the cases that run it; a cell is (radix, 'lds' | 'global', 'rows' | 'cols', 'fwd' | 'inv', dtype,
    'p1' | 'pn')."""
    out = {}
    for c in RUN_CASES:
        for d in c.dtypes:
            for cell in c.cells(d):
                out.setdefault(cell, []).append(c.id)
    return out


ALL_CELLS = [(r, m, o, di, d, p) for r in RADICES for m in ('lds', 'global') for o in ('rows', 'cols')
             for di in ('fwd', 'inv') for d in DTYPES for p in ('p1', 'pn')]
# cell -> reason, for cells that cannot exist.  There is none: for every radix there are 13-smooth lengths on both sides of
# either LDS limit that start with it (p == 1) and that hold it after another factor (p > 1)
IMPOSSIBLE = {}


# ------------------------------------------------------------------------------------------------- references
def f32_exact(a):
    """Round to float32 / complex64 and back: both number formats then see the same values and share one reference."""
    a = np.asarray(a)
    return a.astype(np.complex64).astype(np.complex128) if np.iscomplexobj(a) else a.astype(np.float32).astype(np.float64)


def producer_reference(psf):
    """rfft2(ifftshift(psf)) over the last two axes."""
    return sfft.rfft2(sfft.ifftshift(psf, axes=(-2, -1)), axes=(-2, -1))


def embed_psf(psf, nx, ny, P2, Q2):
    """The rule above k_psf_embed: psf2[u2, v2] = psf[du mod P, dv mod Q] with du = u2 if u2 < nx else u2 - P2 (dv
    likewise), zero unless du > -nx and dv > -ny.  psf has its origin at index 0."""
    P, Q = psf.shape[-2:]
    u2, v2 = np.arange(P2), np.arange(Q2)
    du, dv = np.where(u2 < nx, u2, u2 - P2), np.where(v2 < ny, v2, v2 - Q2)
    keep = (du > -nx)[:, None] & (dv > -ny)[None, :]
    return psf[..., (du % P)[:, None], (dv % Q)[None, :]] * keep


def regrid_reference(psfhat, nx, ny, P, Q, P2, Q2):
    psf = sfft.irfft2(psfhat, s=(P, Q), axes=(-2, -1))
    return sfft.rfft2(embed_psf(psf, nx, ny, P2, Q2), axes=(-2, -1))


def oracle_convolve(psfhat, Q, x):
    return ofc.psf_convolve_cube(*ofc.make_scratch(psfhat, Q, x.shape, np.float64), psfhat, Q, x).copy()


def oracle_hessian(psfhat, Q, x, beam, wsum, sigmainv):
    """out = [beam] conv([beam] x) [/ wsum] + sigmainv x by oracle.fftconv.hessian_psf_cube."""
    return ofc.hessian_psf_cube(*ofc.make_scratch(psfhat, Q, x.shape, np.float64), beam, psfhat, Q, x,
                                sigmainv=sigmainv, wsum=wsum).copy()


def dots(w, w2, out):
    """(<w, out>, <w2, out> or 0, <out, out>) in float64."""
    return np.array([np.vdot(w, out), np.vdot(w2, out) if w2 is not None else 0.0, np.vdot(out, out)])


def _rng(case, salt):
    return np.random.default_rng(7000 + 16 * CASES.index(case) + salt)


INPUT_KINDS = ('noise', 'impulse')
_refs = {}


def _freeze(*arrs):
    for a in arrs:
        if a is not None:
            a.setflags(write=False)
    return arrs


def producer_input(case, kind):
    """(psf, reference psfhat).  'impulse': one unit sample per band, off the centre (P/2, Q/2) where the grid has room:
    every bin of the reference has modulus 1."""
    key = (case.id, kind)
    if key not in _refs:
        P, Q = case.dims
        if kind == 'noise':
            psf = f32_exact(_rng(case, 0).standard_normal((case.nband, P, Q)))
        else:
            psf = np.zeros((case.nband, P, Q))
            for b in range(case.nband):
                psf[b, (P // 2 + 1 + b) % P, (Q // 2 + Q // 3 + 1) % Q] = 1.0
        _refs[key] = _freeze(psf, producer_reference(psf))
    return _refs[key]


def regrid_input(case, kind):
    """(psfhat on the old grid, reference psfhat2).  'impulse': the PSF is one unit sample at the offset
    (-(nx - 1), ny - 1) from the origin, the last one the embed rule keeps: every bin of source and reference has
    modulus 1 -- unless the old grid wraps (P < 2 nx - 1 or Q < 2 ny - 1), where the sample stands for several offsets."""
    key = (case.id, kind)
    if key not in _refs:
        nx, ny, P, Q, P2, Q2 = case.dims
        if kind == 'noise':
            psf = _rng(case, 1).standard_normal((case.nband, P, Q))
        else:
            psf = np.zeros((case.nband, P, Q))
            psf[:, (-(nx - 1)) % P, (ny - 1) % Q] = 1.0
        ph = f32_exact(sfft.rfft2(psf, axes=(-2, -1)))
        _refs[key] = _freeze(ph, regrid_reference(ph, nx, ny, P, Q, P2, Q2))
    return _refs[key]


def apply_input(case, kind):
    """(psfhat, x, w, w2, beam).  'impulse': images of one unit sample in the last row and column (and half a unit in the
    first), which reach the PSF offsets -(nx - 1) .. nx - 1 and -(ny - 1) .. ny - 1."""
    key = (case.id, kind)
    if key not in _refs:
        nx, ny, P, Q = case.dims
        nb, rng = case.nband, _rng(case, 2)
        if case.nonherm:
            ph = rng.standard_normal((nb, P, Q // 2 + 1)) + 1j * rng.standard_normal((nb, P, Q // 2 + 1))
        else:
            ph = producer_reference(rng.standard_normal((nb, P, Q)))
        if kind == 'noise':
            x = rng.standard_normal((nb, nx, ny))
        else:
            x = np.zeros((nb, nx, ny))
            x[:, 0, 0] = 0.5
            x[:, nx - 1, ny - 1] = 1.0
        w, w2 = rng.standard_normal((2, nb, nx, ny))
        beam = 0.5 + rng.random((nb, nx, ny))
        _refs[key] = _freeze(*(f32_exact(a) for a in (ph, x, w, w2, beam)))
    return _refs[key]
