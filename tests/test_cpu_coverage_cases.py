"""
The case table of tests/test_gpu_coverage_edges.py (tests/coverage_cases.py), checked on the CPU:

  * every case has the property it exists for, in every number format it runs in;
  * the coverage matrix {radix 2, 3, 4, 5, 7, 11, 13} x {LDS, global} x {rows, columns} x {forward, inverse} x {fp32,
    fp64} x {first pass (p == 1), later pass (p > 1)} built from the table has no empty cell (none is impossible: for
    every radix there is a 13-smooth length on either side of the LDS limit that starts with it, and one that repeats it);
    beyond the matrix: the repeated large radices, both parities of the global pass count along rows and down columns,
    the sixteen LDS / global choices of the regrid as far as a test can hold them, the grid caps;
  * the mirror of plan_factors reproduces the pass lists the table was chosen by;
  * the references agree with each other without the GPU: the producer reference is the oracle's, and for every regrid
    case a random image convolved with the reference psfhat2 on the new grid equals the oracle's convolution on the old
    grid to 1e-12 -- the embed rule is sound before a kernel is measured against it.
"""
import numpy as np
import pytest

from oracle import fftconv as ofc

import coverage_cases as cc

pmp = pytest.mark.parametrize
ids = [c.id for c in cc.CASES]
REGRID = [c for c in cc.RUN_CASES if c.entry == 'regrid']


def test_table_is_well_formed():
    assert len(set(ids)) == len(ids)
    assert {c.group for c in cc.CASES} == set('abcdef')
    assert cc.RUN_CASES == cc.CASES
    for c in cc.CASES:
        assert c.entry in ('producer', 'regrid', 'apply') and c.dtypes and set(c.dtypes) <= set(cc.DTYPES), c
        assert 1 <= c.nband <= 3 and all(cc.is_smooth(n) for n in c.lengths()), c
        if c.entry == 'producer':
            P, Q = c.dims
            assert Q % 2 == 0
        elif c.entry == 'regrid':
            nx, ny, P, Q, P2, Q2 = c.dims
            # what pfb_psfhat_regrid requires, and nx <= P, ny <= Q so that the oracle can convolve on the old grid
            assert Q % 2 == 0 and Q2 % 2 == 0 and P2 >= 2 * nx - 1 and Q2 >= 2 * ny - 1 and nx <= P and ny <= Q, c
        else:
            nx, ny, P, Q = c.dims
            assert Q % 2 == 0 and 1 <= nx <= P and 1 <= ny <= Q, c
        # small enough for a test of a few seconds: no array above 2^22 values
        sizes = {'producer': lambda d: d[0] * d[1], 'regrid': lambda d: max(d[2] * d[3], d[4] * d[5]),
                 'apply': lambda d: d[2] * d[3]}[c.entry](c.dims)
        assert c.nband * sizes <= 1 << 22, c


@pmp('case', cc.CASES, ids=ids)
def test_case_has_its_property(case):
    for d in case.dtypes:
        assert case.holds(d), (case, d, case.transforms(d))


def test_mirror_reproduces_the_pass_lists():
    f = cc.plan_factors
    assert f(1) == [] and f(2) == [2] and f(4) == [4] and f(8) == [4, 2] and f(16) == [4, 4] and f(13) == [13]
    assert f(49) == [7, 7] and f(121) == [11, 11] and f(169) == [13, 13] and f(52) == [4, 13] and f(1001) == [7, 11, 13]
    assert f(5005) == [5, 7, 11, 13] and f(9240) == [4, 2, 3, 5, 7, 11]
    assert f(10780) == [4, 5, 7, 7, 11] and cc.npass(10780) == 5 and cc.copies_back(10780)
    assert f(10530) == [2, 3, 3, 3, 3, 5, 13] and cc.npass(10530) == 7 and cc.copies_back(10530)
    assert f(16500) == [4, 3, 5, 5, 5, 11] and f(16562) == [2, 7, 7, 13, 13]
    assert f(10400) == [4, 4, 2, 5, 5, 13] and f(10500) == [4, 3, 5, 5, 5, 7] and cc.npass(10000) == 6
    assert f(7200) == [4, 4, 2, 3, 3, 5, 5] and f(12000) == [4, 4, 2, 3, 5, 5, 5] and cc.copies_back(12000)
    assert f(17) is None and f(34) is None and f(2 * 19 * 4) is None
    assert cc.passes(5005) == [(5, 1), (7, 5), (11, 35), (13, 385)]
    # the first 13-smooth lengths above the LDS limits
    above = lambda n, k: [m for m in range(n + 1, n + 400) if cc.is_smooth(m)][:k]      # noqa: E731
    assert above(10240, 5) == [10290, 10296, 10368, 10395, 10400]
    assert above(5120, 4) == [5145, 5148, 5184, 5200]
    # the limits themselves
    assert cc.line_fits_lds(10240, cc.F32) and not cc.line_fits_lds(10241, cc.F32)
    assert cc.line_fits_lds(5120, cc.F64) and not cc.line_fits_lds(5121, cc.F64)
    assert cc.long_lines(10240, 2, cc.F32) and not cc.long_lines(10232, 2, cc.F32)
    assert cc.long_lines(2, 5120, cc.F64) and not cc.long_lines(2, 5116, cc.F64)
    assert cc.long_grid(1) == 1 and cc.long_grid(257) == 2 and cc.long_grid(16384) == 64 and cc.long_grid(10 ** 6) == 64
    assert not cc.long_grid_strides(16384) and cc.long_grid_strides(16385)


def test_coverage_matrix_has_no_empty_cell():
    m = cc.matrix()
    assert len(cc.ALL_CELLS) == 7 * 2 * 2 * 2 * 2 * 2
    empty = [c for c in cc.ALL_CELLS if c not in m and c not in cc.IMPOSSIBLE]
    assert not empty, empty
    assert not [c for c in cc.IMPOSSIBLE if c in m], "a cell listed as impossible runs"
    assert all(isinstance(why, str) and why for why in cc.IMPOSSIBLE.values())


def _transforms():
    for c in cc.RUN_CASES:
        for d in c.dtypes:
            for t in c.transforms(d):
                yield (c, d) + t


def test_repeated_large_radices_run_everywhere():
    """A radix 7 / 11 / 13 pass with p > 1 and k running over its own radix (lengths with the radix squared), in LDS and
    as a global pass, along rows and down columns, forward and inverse, in both formats."""
    seen = set()
    for c, d, n, mem, orient, direction in _transforms():
        for r in (7, 11, 13):
            if n % (r * r) == 0:
                seen.add((r, mem, orient, direction, d))
    want = {(r, mem, o, di, d) for r in (7, 11, 13) for mem in ('lds', 'global') for o in ('rows', 'cols')
            for di in ('fwd', 'inv') for d in cc.DTYPES}
    assert want <= seen, sorted(want - seen)


def test_global_pass_count_parities():
    """Odd (copy back) and even pass counts of long_fft, rows and columns, both directions and formats; an odd one down
    columns with two bands or more (the column form transforms and copies band by band)."""
    seen, odd_cols_bands = set(), set()
    for c, d, n, mem, orient, direction in _transforms():
        if mem == 'global':
            seen.add((cc.copies_back(n), orient, direction, d))
            if cc.copies_back(n) and orient == 'cols' and c.nband >= 2 and c.entry != 'apply':
                odd_cols_bands.add((direction, d))
    assert len(seen) == 2 * 2 * 2 * 2, seen
    assert odd_cols_bands == {(di, d) for di in ('fwd', 'inv') for d in cc.DTYPES}


def test_regrid_memory_choices():
    """(cl, rl, rl2, cl2) of pfb_psfhat_regrid: each is LDS in one case and global in another, with a long source onto an
    LDS target and the reverse, for columns and for rows.  Combinations with a long row AND a long column on one grid
    need 10^8 values per array and stay out."""
    for d in cc.DTYPES:
        combos = {tuple(m == 'lds' for _, m, _, _ in c.transforms(d)) for c in REGRID if d in c.dtypes}
        for k in range(4):
            assert {cb[k] for cb in combos} == {True, False}, (d, k, combos)
        for want in ((True, True, True, False), (False, True, True, True), (True, True, False, True),
                     (True, False, True, True), (False, True, True, False), (True, False, False, True),
                     (True, True, True, True)):
            assert want in combos, (d, want)


def test_boundary_and_grid_cap_cases_exist():
    for d in cc.DTYPES:
        n = cc.LDS_FULL[d]
        for orient in ('rows', 'cols'):
            for direction in ('fwd', 'inv'):
                assert any(tuple(t) == (n, 'lds', orient, direction) for c, dd, *t in _transforms() if dd == d and c.entry != 'apply')
                assert any(tuple(t) == (n, 'global', orient, direction) for c, dd, *t in _transforms() if dd == d and c.entry == 'apply')
        # long_grid: a line above 16384 in the row kernels of both directions and in the column load / store
        assert any(n > 16384 and mem == 'global' and o == 'rows' and di == 'fwd' for c, dd, n, mem, o, di in _transforms() if dd == d)
        assert any(n > 16384 and mem == 'global' and o == 'rows' and di == 'inv' for c, dd, n, mem, o, di in _transforms() if dd == d)
        assert any(c.entry == 'apply' and n > 16384 and o == 'cols' and c.dims[0] > 16384
                   for c, dd, n, mem, o, di in _transforms() if dd == d)
    above, below = cc.by_id('d-apply-colmul-above'), cc.by_id('d-apply-colmul-below')
    assert (above.dims[3] // 2 + 1) * above.dims[2] > cc.COL_MUL_GRID > (below.dims[3] // 2 + 1) * below.dims[2]
    # k_sum_partials: one partial, fewer than 64, more than 256
    counts = {c.nband * c.dims[0] for c in cc.RUN_CASES if c.entry == 'apply'}
    assert 1 in counts and any(1 < n < 64 for n in counts) and any(n > 256 for n in counts)


@pmp('case', [c for c in cc.RUN_CASES if c.entry == 'producer'], ids=lambda c: c.id)
def test_producer_reference_is_the_oracle(case):
    for kind in cc.INPUT_KINDS:
        psf, ref = cc.producer_input(case, kind)
        want = ofc.psfhat_from_psf(psf)
        assert ref.shape == (case.nband, case.dims[0], case.dims[1] // 2 + 1)
        assert np.abs(ref - want).max() <= 1e-12 * np.abs(want).max()
        if kind == 'impulse':
            assert np.abs(np.abs(ref) - 1.0).max() < 1e-12


@pmp('case', REGRID, ids=lambda c: c.id)
def test_regrid_reference_convolves_like_the_old_grid(case):
    nx, ny, P, Q, P2, Q2 = case.dims
    x = np.random.default_rng(len(case.id) + P + Q2).standard_normal((case.nband, nx, ny))
    for kind in cc.INPUT_KINDS:
        ph, ph2 = cc.regrid_input(case, kind)
        assert ph.shape == (case.nband, P, Q // 2 + 1) and ph2.shape == (case.nband, P2, Q2 // 2 + 1)
        want = cc.oracle_convolve(ph, Q, x)
        got = cc.oracle_convolve(ph2, Q2, x)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), kind
        if kind == 'impulse':
            assert np.abs(np.abs(ph) - 1.0).max() < 1e-6
            assert cc.wraps(case) or np.abs(np.abs(ph2) - 1.0).max() < 1e-6


def test_only_the_wrap_cases_wrap():
    assert sorted(c.id for c in REGRID if cc.wraps(c)) == ['e-full-wrap-smallest', 'e-odd-P-between']


def test_embed_rule_by_hand():
    """The rule on one line, written out: nx = 3 on P = 4 -> P2 = 6 keeps the offsets -2 .. 2, read modulo 4."""
    psf = np.arange(1.0, 5.0).reshape(4, 1) * np.ones((1, 2))
    got = cc.embed_psf(psf, 3, 1, 6, 2)
    assert got.shape == (6, 2)
    assert np.array_equal(got[:, 0], [1, 2, 3, 0, 3, 4]) and np.array_equal(got[:, 1], [0] * 6)


@pmp('case', [c for c in cc.RUN_CASES if c.entry == 'apply'], ids=lambda c: c.id)
def test_apply_inputs(case):
    nx, ny, P, Q = case.dims
    for kind in cc.INPUT_KINDS:
        ph, x, w, w2, beam = cc.apply_input(case, kind)
        assert ph.shape == (case.nband, P, Q // 2 + 1) and x.shape == w.shape == w2.shape == beam.shape == (case.nband, nx, ny)
        for a in (ph, x, w, w2, beam):
            assert np.array_equal(a, cc.f32_exact(a))
    if case.nonherm:
        assert np.abs(ph[:, :, 0].imag).max() > 0.1 and np.abs(ph[:, :, -1].imag).max() > 0.1
    # the impulse image reaches the last offsets: the oracle's answer in the first pixel is half the PSF's origin plus the
    # sample at (-(nx - 1), -(ny - 1))
    if not case.nonherm and nx * ny > 1:
        psf = np.fft.irfft2(ph, s=(P, Q))
        y = cc.oracle_convolve(ph, Q, x)
        want = 0.5 * psf[:, 0, 0] + psf[:, (-(nx - 1)) % P, (-(ny - 1)) % Q]
        assert np.abs(y[:, 0, 0] - want).max() <= 1e-11 * np.abs(psf).max()
