"""
Case table of the wavelet dictionary edge tests (tests/test_cpu_psi_cases.py, tests/test_gpu_psi_edges.py).

Every case is (nband, nx, ny, bases, nlevel) with a name and the PROPERTY IT EXISTS FOR, a predicate over the bookkeeping
(oracle.wavelets.Bookkeeping: sx, sy, spx, spy, Ntotx, Ntoty) and the kernels' tile constants mirrored below.  The
predicates are asserted on the CPU, so a case cannot silently stop exercising its edge when a tile size changes.

`need` says for which number formats the predicate has to hold: 'both', 'any' (at least one of the two) or one name.

Plain Python and numpy, no GPU and no torch.  The references (`oracle_dot`, `oracle_hdot`) are the statements of
oracle.wavelets.Psi on the image zero-padded to even sizes, with the planes sized as pfb_psi_plan_create sizes them
(max(Ntot, n)), so that they also cover odd image sizes and dictionaries of 'self' alone, which oracle.wavelets.Psi
cannot run.
"""
import numpy as np

from oracle import daubechies as odb
from oracle import wavelets as owv

F32, F64 = 'float32', 'float64'
DTYPES = (F32, F64)
# csrc/wavelet.hip: Tile<T>::TA (analysis: coefficients per quadrant edge of a tile), Tile<T>::TS (synthesis: image pixels
# per tile edge) and DwtFast<T>::EV = SynFast<T, TS>::EV (elements per 16-byte access, the VW of dwt_tile / psi_dot_t)
TA = {F32: 32, F64: 16}
TS = {F32: 64, F64: 32}
VW = {F32: 4, F64: 2}
MAXLEV = 12


def ceil_div(a, b):
    return -(-a // b)


class Case:
    def __init__(self, group, name, nband, nx, ny, bases, nlevel, prop, need='both', why=''):
        self.group, self.name = group, name
        self.nband, self.nx, self.ny, self.bases, self.nlevel = nband, nx, ny, tuple(bases), nlevel
        self.prop, self.need, self.why = prop, need, why

    @property
    def id(self):
        return f"{self.group}-{self.name}"

    @property
    def wavelets(self):
        return [w for w in self.bases if w != 'self']

    @property
    def odd(self):
        return bool(self.nx % 2 or self.ny % 2)

    @property
    def refused(self):
        """The level count is beyond pywt.dwt_max_level for some basis: the reference, the oracle and Psi raise ValueError."""
        return any(self.nlevel > odb.dwt_max_level(min(self.nx, self.ny), w) for w in self.wavelets)

    def bk(self, w):
        """Bookkeeping of wavelet w.  For an odd size it equals that of the size rounded up (tests/test_cpu_psi_cases.py)."""
        return owv.Bookkeeping(self.nx, self.ny, 2 * int(w[2:]), self.nlevel)

    def plane(self):
        """(Nymax, Nxmax) as pfb_psi_plan_create computes them."""
        bks = [self.bk(w) for w in self.wavelets]
        return (max([b.Ntoty for b in bks] + [self.ny]), max([b.Ntotx for b in bks] + [self.nx]))

    def holds(self, dtype):
        return bool(self.prop(self, dtype))

    def __repr__(self):
        return f"Case({self.id}: {self.nband}x{self.nx}x{self.ny} {list(self.bases)} L{self.nlevel})"


# ------------------------------------------------------------------------------------------------- launch grids
def l0_fused(case, dtype):
    """psi_dot_t: level 0 of all bases runs in k_dwt_l1_fused (16-byte aligned image rows; the pointer is assumed
    aligned, as a fresh allocation is), else in k_dwt_batched."""
    return bool(case.wavelets) and case.ny % VW[dtype] == 0 and TA[dtype] % (2 * VW[dtype]) == 0


def ana_tiles(case, dtype, level, w):
    b = case.bk(w)
    return ceil_div(b.sx[level], TA[dtype]), ceil_div(b.sy[level], TA[dtype])


def syn_tiles(case, dtype, level, w):
    """Tiles of the image that synthesis level `level` >= 1 of basis w writes (spx x spy pixels)."""
    b = case.bk(w)
    return ceil_div(b.spx[level], TS[dtype]), ceil_div(b.spy[level], TS[dtype])


def ana_grid(case, dtype, level):
    """(gridDim.x, .y, .z) of the analysis launch of `level`: psi_plan_device_setup's maxima over the wavelet bases
    (gx_ana, gy_ana); z is nband in k_dwt_l1_fused and nband * nwb in k_dwt_batched.  None without a wavelet basis."""
    ws = case.wavelets
    if not ws:
        return None
    t = [ana_tiles(case, dtype, level, w) for w in ws]
    gz = case.nband if level == 0 and l0_fused(case, dtype) else case.nband * len(ws)
    return max(a for a, _ in t), max(b for _, b in t), gz


def syn_grid(case, dtype, level):
    """Level >= 1: k_idwt_batched2's grid (gx_syn, gy_syn maxima, nband * nwb).  Level 0: the finest fused synthesis
    grid ceil(nx / TS) x ceil(ny / TS) x nband."""
    if level == 0:
        return ceil_div(case.nx, TS[dtype]), ceil_div(case.ny, TS[dtype]), case.nband
    ws = case.wavelets
    if not ws:
        return None
    t = [syn_tiles(case, dtype, level, w) for w in ws]
    return max(a for a, _ in t), max(b for _, b in t), case.nband * len(ws)


def grid_kind(grid):
    """How xcd_tile treats a grid: 'lt64' never enters the permutation, 'mult64' is permuted throughout, 'tail' has
    k >= 1 permuted runs of 64 and 0 < r < 64 workgroups left alone, with a gridDim.x that is no multiple of 8."""
    gx, gy, gz = grid
    total = gx * gy * gz
    if total < 64:
        return 'lt64'
    if total % 64 == 0:
        return 'mult64'
    return 'tail' if gx % 8 else 'tail-gx8'


FAMILIES = ('ana0', 'synfin', 'anacoarse', 'syncoarse')


def family_grid(case, dtype, family, level):
    if family == 'ana0':
        return ana_grid(case, dtype, 0)
    if family == 'synfin':
        return syn_grid(case, dtype, 0)
    return (ana_grid if family == 'anacoarse' else syn_grid)(case, dtype, level)


# ------------------------------------------------------------------------------------------------- predicates
def p_remainder_axes(case, _dtype=None):
    """Each axis hits a remainder in {0, 1, TA - 1} for at least one number format."""
    b = case.bk(case.wavelets[0])
    return all(any(c % TA[d] in (0, 1, TA[d] - 1) for d in DTYPES) for c in (b.sx[0], b.sy[0]))


def p_smaller_than_tile(case, dtype):
    b = case.bk(case.wavelets[0])
    return (max(b.sx[0], b.sy[0]) < TA[dtype] and max(case.nx, case.ny) < TS[dtype]
            and ana_grid(case, dtype, 0)[:2] == (1, 1) and syn_grid(case, dtype, 0)[:2] == (1, 1))


def deepest(sx, sy=None):
    """nlevel == dwt_max_level for every wavelet, with exactly these per-level coefficient counts."""
    def prop(case, dtype):
        ok = all(case.nlevel == odb.dwt_max_level(min(case.nx, case.ny), w) for w in case.wavelets)
        b = case.bk(case.wavelets[0])
        return ok and case.nlevel >= 3 and b.sx == list(sx) and b.sy == list(sy or sx)
    return prop


def p_coarse_rows_aligned(case, dtype):
    """Every coarse analysis input row length (the level above's Cy) is a multiple of 8: AL = true in both formats."""
    b = case.bk(case.wavelets[0])
    return all(c % 8 == 0 for c in b.sy[:-1]) and deepest(b.sx, b.sy)(case, dtype)


def grids_differ(level):
    """The per-basis tile counts differ at `level`, in analysis and (for level >= 1, where synthesis is batched) in
    synthesis: the smaller basis leaves k_dwt_batched / k_dwt_l1_fused / k_idwt_batched2 through its early exit."""
    def prop(case, dtype):
        a = {ana_tiles(case, dtype, level, w) for w in case.wavelets}
        s = {syn_tiles(case, dtype, level, w) for w in case.wavelets} if level >= 1 else {0, 1}
        return len(a) > 1 and len(s) > 1 and case.nband >= 3
    return prop


def alignment(expect):
    """expect[dtype] = (ny % VW == 0, sy[0] % VW == 0, spy[1] % VW == 0): the level-0 staging / store branch, the
    AL = true / false branch of the level-1 analysis input (ldin = nyin = sy[0]) and the vector / scalar store of the
    level-1 partial image (ldo = spy[1])."""
    def prop(case, dtype):
        if dtype not in expect:
            return True
        v = VW[dtype]
        return case.nlevel >= 2 and all(
            (case.ny % v == 0, case.bk(w).sy[0] % v == 0, case.bk(w).spy[1] % v == 0) == expect[dtype]
            for w in case.wavelets)
    return prop


def xcd(expect):
    """expect[(dtype, family, level)] = (total workgroups, kind)."""
    def prop(case, dtype):
        for (d, fam, lev), (total, kind) in expect.items():
            if d != dtype:
                continue
            g = family_grid(case, d, fam, lev)
            if g is None or g[0] * g[1] * g[2] != total or grid_kind(g) != kind:
                return False
        return True
    prop.expect = expect
    return prop


def p_odd(case, dtype):
    return case.odd and 'self' in case.bases


def dictionary(check):
    return lambda case, dtype: bool(check(case, dtype))


# ------------------------------------------------------------------------------------------------- the table
def _cases():
    out = []

    def add(*a, **k):
        out.append(Case(*a, **k))

    # a. tile remainders at level 0: one wavelet, one level, rectangular so that x and y hit different remainders
    for w, pairs in (('db1', [(30, 66), (64, 34), (130, 62), (32, 126), (34, 128), (62, 130), (66, 30), (126, 32),
                              (128, 64)]),
                     ('db4', [(24, 56), (26, 58), (28, 60), (56, 28), (58, 24), (60, 26)]),
                     ('db9', [(46, 48), (48, 50), (50, 46)])):
        for nx, ny in pairs:
            add('a', f'{w}-{nx}x{ny}', 2, nx, ny, [w], 1, p_remainder_axes, need='any',
                why='C % TA in {0, 1, TA - 1} on each axis for at least one format')
    # b. smaller than a tile
    add('b', 'db1-2x2', 2, 2, 2, ['db1'], 1, p_smaller_than_tile)
    add('b', 'db1-4x6-L2', 2, 4, 6, ['db1'], 2, p_smaller_than_tile)
    add('b', 'db2-8x10', 2, 8, 10, ['db2'], 1, p_smaller_than_tile)
    # c. deepest possible levels
    add('c', 'db1-16-L4', 2, 16, 16, ['db1'], 4, deepest([8, 4, 2, 1]))
    add('c', 'db1-32-L5', 2, 32, 32, ['db1'], 5, deepest([16, 8, 4, 2, 1]))
    add('c', 'db2-24-L3', 2, 24, 24, ['db2'], 3, deepest([13, 8, 5]))
    add('c', 'db4-64-L3', 2, 64, 64, ['db4'], 3, deepest([35, 21, 14]))
    add('c', 'db9-136-L3', 2, 136, 136, ['db9'], 3, deepest([76, 46, 31]))
    add('c', 'db9-272-L4', 2, 272, 272, ['db9'], 4, deepest([144, 80, 48, 32]))
    add('c', 'db5-72-L3', 2, 72, 72, ['db5'], 3, p_coarse_rows_aligned)
    add('c', 'db1-32x16-L4', 2, 32, 16, ['db1'], 4, deepest([16, 8, 4, 2], [8, 4, 2, 1]))
    # d. batched grids larger than one basis needs
    add('d', 'db1+db9-64', 3, 64, 64, ['db1', 'db9'], 1, grids_differ(0),
        why='level-0 C = 32 vs 40: 1 vs 2 (fp32) and 2 vs 3 (fp64) tiles per edge; k_dwt_l1_fused skips db1 on the last ones')
    add('d', 'db1+db9-248-L2', 3, 248, 248, ['db1', 'db9'], 2, grids_differ(1))
    # e. coarse-level alignment: (ny % VW, sy[0] % VW, spy[1] % VW) == 0
    T, N = True, False
    add('e', 'db1-50x72', 2, 50, 72, ['db1'], 2, alignment({F32: (T, T, T), F64: (T, T, T)}))
    add('e', 'db2-50x70', 2, 50, 70, ['db2'], 2, alignment({F32: (N, T, T), F64: (T, T, T)}))
    add('e', 'db2-50x72', 2, 50, 72, ['db2'], 2, alignment({F32: (T, N, N), F64: (T, N, T)}))
    add('e', 'db2-50x74', 2, 50, 74, ['db2'], 2, alignment({F32: (N, N, N), F64: (T, T, T)}))
    add('e', 'db2-50x69', 2, 50, 69, ['db2'], 2, alignment({F32: (N, T, T), F64: (N, T, T)}))
    add('e', 'db2-50x71', 2, 50, 71, ['db2'], 2, alignment({F32: (N, N, N), F64: (N, N, T)}))
    # f. XCD permutation: grid totals below 64, multiples of 64, and 64 k + r with gridDim.x % 8 != 0
    add('f', 'db1-256-b4-L2', 4, 256, 256, ['db1'], 2, xcd({
        (F32, 'ana0', 0): (64, 'mult64'), (F32, 'synfin', 0): (64, 'mult64'),
        (F32, 'anacoarse', 1): (16, 'lt64'), (F32, 'syncoarse', 1): (16, 'lt64'),
        (F64, 'ana0', 0): (256, 'mult64'), (F64, 'synfin', 0): (256, 'mult64'),
        (F64, 'anacoarse', 1): (64, 'mult64'), (F64, 'syncoarse', 1): (64, 'mult64')}))
    add('f', 'db1-260-b3', 3, 260, 260, ['db1'], 1, xcd({
        (F32, 'ana0', 0): (75, 'tail'), (F32, 'synfin', 0): (75, 'tail'),
        (F64, 'ana0', 0): (243, 'tail'), (F64, 'synfin', 0): (243, 'tail')}))
    add('f', 'db1-4-128-b4-L2', 4, 128, 128, ['db1', 'db2', 'db3', 'db4'], 2, xcd({
        (F32, 'anacoarse', 1): (64, 'mult64'), (F32, 'syncoarse', 1): (64, 'mult64'),
        (F64, 'anacoarse', 1): (144, 'tail'), (F64, 'syncoarse', 1): (144, 'tail')}))
    add('f', 'db1+db2-260-b4-L2', 4, 260, 260, ['db1', 'db2'], 2, xcd({
        (F32, 'anacoarse', 1): (72, 'tail'), (F32, 'syncoarse', 1): (72, 'tail'),
        (F64, 'anacoarse', 1): (200, 'tail'), (F64, 'syncoarse', 1): (200, 'tail')}))
    add('f', 'db2-40x24-b3-L2', 3, 40, 24, ['db2'], 2, xcd({
        (F32, 'ana0', 0): (3, 'lt64'), (F32, 'synfin', 0): (3, 'lt64'),
        (F32, 'anacoarse', 1): (3, 'lt64'), (F32, 'syncoarse', 1): (3, 'lt64'),
        (F64, 'ana0', 0): (6, 'lt64'), (F64, 'synfin', 0): (6, 'lt64'),
        (F64, 'anacoarse', 1): (3, 'lt64'), (F64, 'syncoarse', 1): (3, 'lt64')}))
    # g. odd sizes.  db5 allows 2 levels only from 36 pixels on: the smaller sizes are refused (and pinned as such);
    # ['self', 'db2', 'db3'] runs 2 levels on them instead
    for nx, ny in ((33, 64), (64, 33), (31, 45), (129, 67)):
        for nl in (1, 2):
            add('g', f'{nx}x{ny}-L{nl}', 2, nx, ny, ['self', 'db2', 'db5'], nl, p_odd)
    for nx, ny in ((33, 64), (64, 33), (31, 45)):
        add('g', f'{nx}x{ny}-db3-L2', 2, nx, ny, ['self', 'db2', 'db3'], 2, p_odd)
    # h. dictionary shapes, at sizes of (a)
    add('h', 'self', 3, 30, 66, ['self'], 1, dictionary(lambda c, d: not c.wavelets and c.plane() == (c.ny, c.nx)))
    add('h', 'self-db3-self', 3, 34, 64, ['self', 'db3', 'self'], 1,
        dictionary(lambda c, d: c.bases.count('self') == 2 and l0_fused(c, d)),
        why="the first 'self' rides in k_dwt_l1_fused, the second in k_transpose")
    add('h', 'db2-db2', 3, 58, 24, ['db2', 'db2'], 1, dictionary(lambda c, d: c.bases[0] == c.bases[1] != 'self'))
    add('h', 'db4-L3', 3, 130, 62, ['db4'], 3, dictionary(lambda c, d: len(c.bases) == 1 and c.nlevel == 3),
        why='fin_scratch and bscr hold one slice')
    add('h', 'db9-self-db1', 3, 50, 46, ['db9', 'self', 'db1'], 1,
        dictionary(lambda c, d: c.bases[1] == 'self' and max(2 * int(w[2:]) for w in c.wavelets) == 18))
    return out


CASES = _cases()
RUN_CASES = [c for c in CASES if not c.refused]
REFUSED_CASES = [c for c in CASES if c.refused]
# the stand-alone dwt2d / idwt2d entry points: one tiny, one deepest, one with a tile remainder
STANDALONE = ('b-db1-2x2', 'c-db1-32-L5', 'a-db1-30x66')


def by_id(cid):
    return next(c for c in CASES if c.id == cid)


# ------------------------------------------------------------------------------------------------- references
def _even(n):
    return n + n % 2


def oracle_dot(case, x, fill=np.nan):
    """psi.dot in float64 by the oracle's statements: (nband, nbasis, Nymax, Nxmax), cells nothing writes hold `fill`.
    Odd sizes: the wavelet planes are those of the image zero-padded to even sizes (zero extension makes the analysis of
    an odd-length signal that of the signal with one zero appended); 'self' is written on [0:ny, 0:nx] only."""
    nb, nx, ny = case.nband, case.nx, case.ny
    Ny, Nx = case.plane()
    xp = np.zeros((nb, _even(nx), _even(ny)))
    xp[:, :nx, :ny] = x
    out = np.full((nb, len(case.bases), Ny, Nx), fill, dtype=np.float64)
    for i, w in enumerate(case.bases):
        if w == 'self':
            out[:, i, :ny, :nx] = np.swapaxes(np.asarray(x, dtype=np.float64), 1, 2)
            continue
        bk = owv.Bookkeeping(_even(nx), _even(ny), 2 * int(w[2:]), case.nlevel)
        dl, dh, _, _ = odb.filter_bank(w)
        for b in range(nb):
            owv.dwt2d(xp[b], out[b, i, :bk.Ntoty, :bk.Ntotx], bk, dl, dh)
    return out


def oracle_hdot(case, c):
    """psi.hdot in float64 by the oracle's statements; odd sizes: the oracle's image of the even size, cropped."""
    nb, nx, ny = case.nband, case.nx, case.ny
    c = np.asarray(c, dtype=np.float64)
    out = np.zeros((nb, nx, ny))
    img = np.zeros((_even(nx), _even(ny)))
    for i, w in enumerate(case.bases):
        if w == 'self':
            out += np.swapaxes(c[:, i, :ny, :nx], 1, 2)
            continue
        bk = owv.Bookkeeping(_even(nx), _even(ny), 2 * int(w[2:]), case.nlevel)
        _, _, rl, rh = odb.filter_bank(w)
        for b in range(nb):
            owv.idwt2d(c[b, i, :bk.Ntoty, :bk.Ntotx], img, bk, rl, rh)
            out[b] += img[:nx, :ny]
    return out


_refs = {}


def reference(case):
    """Inputs exactly representable in float32 (so both number formats see the same values and share one reference) and
    the float64 oracle's results, computed once per case and read-only: x, psi.dot(x) over NaN (cells that stay NaN are
    never written), coefficients c that are random EVERYWHERE (margins included), psi.hdot(c)."""
    if case.id not in _refs:
        rng = np.random.default_rng(1000 + CASES.index(case))
        x = rng.standard_normal((case.nband, case.nx, case.ny)).astype(np.float32).astype(np.float64)
        a_ref = oracle_dot(case, x)
        c = rng.standard_normal(a_ref.shape).astype(np.float32).astype(np.float64)
        xo_ref = oracle_hdot(case, c)
        for arr in (x, a_ref, c, xo_ref):
            arr.setflags(write=False)
        _refs[case.id] = (x, a_ref, c, xo_ref)
    return _refs[case.id]
