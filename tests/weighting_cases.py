"""
The imaging weights' case table (tests/golden/weighting.npz, made from the reference's own source by
tests/golden/make_golden_weighting.py), a plain-numpy statement of the four functions and the tests' bounds; shared by
test_cpu_weighting_cases.py and test_gpu_weighting.py.

COUNT_CASES   dicts of name, nx, ny, cell, uvw, freq, mask, runs [(k, ngrid)] and ref[(run, 'f32' | 'f64')], the
              reference's (ngrid, nx, ny) counts
COUNT_RUNS    (case, run, k, ngrid, tag) of every stored run, ids COUNT_RUN_IDS
WEIGHT_CASES  dicts of case, counts {tag: (nx, ny)}, robust values and ref[(q, tag)], the reference's weights
FILTER_CASES  dicts of level, counts {tag} and ref {tag}
L2_CASES      dicts of vis, model_vis (complex128), mask, dof

The statement (np_*) is written from what the functions are documented to compute, vectorised; the CPU test
shows that it reproduces the stored reference outputs, which makes it the pointwise model where a test needs a value
that is not in the fixture.
"""
import math
import os

import numpy as np

C_LIGHT = 299792458.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'weighting.npz')
DTYPES = {'f32': np.float32, 'f64': np.float64}
U = {'f32': 2.0 ** -24, 'f64': 2.0 ** -53}
BLOCK = 256                                  # IMW_BLOCK of csrc/imweight.hip: the visibility counts straddle it
GRIDS = {(16, 12), (32, 24), (64, 40)}
VIS_COUNTS = {(1, 1), (85, 3), (64, 4), (257, 1), (300, 3)}
NGRIDS = {1, 2, 7}
SUPPORTS = {0, 2, 6, 12}
ROBUST = (-3, -2, 0, 2)


def _load():
    g = np.load(GOLDEN, allow_pickle=False)
    names = [str(n) for n in g['names']]
    count_cases = []
    for i, name in enumerate(names):
        nx, ny = (int(v) for v in g[f'c{i}_shape'])
        runs = [(int(k), int(n)) for k, n in g[f'c{i}_runs']]
        ref = {(r, tag): g[f'c{i}_r{r}_{tag}'] for r in range(len(runs)) for tag in DTYPES}
        count_cases.append(dict(name=name, nx=nx, ny=ny, cell=tuple(float(v) for v in g[f'c{i}_cell']),
                                uvw=g[f'c{i}_uvw'], freq=g[f'c{i}_freq'], mask=g[f'c{i}_mask'], runs=runs, ref=ref))
    weight_cases = []
    for j in range(int(g['nweight'])):
        ci, r = (int(v) for v in g[f'w{j}_src'])
        case = count_cases[ci]
        counts = {tag: case['ref'][(r, tag)][0] * (0 if g[f'w{j}_zero'] else 1) for tag in DTYPES}
        robust = [int(v) for v in g[f'w{j}_robust']]
        weight_cases.append(dict(name=f"{case['name']}-k{case['runs'][r][0]}" + ('-zero' if g[f'w{j}_zero'] else ''),
                                 case=case, counts=counts, robust=robust, zero=bool(g[f'w{j}_zero']),
                                 ref={(q, tag): g[f'w{j}_o{q}_{tag}'] for q in range(len(robust)) for tag in DTYPES}))
    filter_cases = [dict(name=f'f{j}', level=float(g[f'f{j}_level']), counts={t: g[f'f{j}_in_{t}'] for t in DTYPES},
                         ref={t: g[f'f{j}_out_{t}'] for t in DTYPES}) for j in range(int(g['nfilter']))]
    l2_cases = [dict(name=f"l{j}-{g[f'l{j}_vis'].shape[0]}x{g[f'l{j}_vis'].shape[1]}", vis=g[f'l{j}_vis'],
                     model_vis=g[f'l{j}_model_vis'], mask=g[f'l{j}_mask'], dof=float(g[f'l{j}_dof']))
                for j in range(int(g['nl2']))]
    return count_cases, weight_cases, filter_cases, l2_cases


COUNT_CASES, WEIGHT_CASES, FILTER_CASES, L2_CASES = _load()
COUNT_RUNS = [(c, r, k, n, tag) for c in COUNT_CASES for r, (k, n) in enumerate(c['runs']) for tag in DTYPES]
COUNT_RUN_IDS = [f"{c['name']}-k{k}-g{n}-{tag}" for c, r, k, n, tag in COUNT_RUNS]


def case_named(name):
    return next(c for c in COUNT_CASES if c['name'] == name)


# ------------------------------------------------------------------------------------------------ the statement
def uv_cells(nx, ny, cell_x, cell_y):
    u_cell = 1 / (nx * cell_x)
    v_cell = 1 / (ny * cell_y)
    return u_cell, abs(-1 / cell_x / 2 - u_cell / 2), v_cell, abs(-1 / cell_y / 2 - v_cell / 2)


def grid_coords(case):
    """(ug, vg), each (nrow, nchan): (uvw * (freq / c) + umax) / u_cell, every operation a rounded fp64 one."""
    u_cell, umax, v_cell, vmax = uv_cells(case['nx'], case['ny'], *case['cell'])
    nf = case['freq'] / C_LIGHT
    return ((case['uvw'][:, 0:1] * nf[None, :] + umax) / u_cell, (case['uvw'][:, 1:2] * nf[None, :] + vmax) / v_cell)


def bin_of_rows(nrow, ngrid):
    """The partial grid of every row: bins of nrow // ngrid rows, the first nrow % ngrid of them one longer."""
    sizes = [nrow // ngrid + (1 if b < nrow % ngrid else 0) for b in range(ngrid)]
    return np.repeat(np.arange(ngrid), sizes)


def phi(t, k):
    return np.exp(2.3 * k * (np.sqrt((1 - t) * (1 + t)) - 1))


def footprints(case, k):
    """Of the unmasked visibilities, in row-major order: rows (n,), cells xi (n, K), yi (n, K) and the factors fx, fy
    (n, K); K = max(k, 1), for k = 0 the one cell (floor ug, floor vg) with factor 1."""
    ug, vg = grid_coords(case)
    sel = case['mask'] != 0
    rows = np.nonzero(sel)[0]
    ug, vg = ug[sel], vg[sel]
    if k == 0:
        one = np.ones((ug.size, 1))
        return rows, np.floor(ug).astype(np.int64)[:, None], np.floor(vg).astype(np.int64)[:, None], one, one
    h = k // 2
    off = np.arange(-h, h)
    xi = np.rint(ug).astype(np.int64)[:, None] + off            # rint: halves to even, as np.round
    yi = np.rint(vg).astype(np.int64)[:, None] + off
    return rows, xi, yi, phi((xi - ug[:, None] + 0.5) / h, k), phi((yi - vg[:, None] + 0.5) / h, k)


def cell_ranges(case, k):
    """(xmin, xmax, ymin, ymax) of every cell the reference addresses for this case and support; None without any."""
    _, xi, yi, _, _ = footprints(case, k)
    return None if xi.size == 0 else (int(xi.min()), int(xi.max()), int(yi.min()), int(yi.max()))


def np_counts(case, k, ngrid, dtype, clip=False):
    """_compute_counts: (counts (ngrid, nx, ny) of dtype, summed in fp64 and rounded once; n_cell, the number of
    contributions to every cell).  clip: the defined difference of the GPU functions -- a visibility whose cell
    (floor ug, floor vg) is outside the grid is dropped, and so is every footprint cell outside it; without it such a
    case is an IndexError here."""
    nx, ny = case['nx'], case['ny']
    if clip:
        ug, vg = grid_coords(case)
        inside = (ug >= 0) & (ug < nx) & (vg >= 0) & (vg < ny)
        case = dict(case, mask=case['mask'] * inside)
    rows, xi, yi, fx, fy = footprints(case, k)
    if clip:
        fx = np.where((xi >= 0) & (xi < nx), fx, np.nan)
        fy = np.where((yi >= 0) & (yi < ny), fy, np.nan)
        keep = ~np.isnan(fx[:, :, None] * fy[:, None, :])
        xi, yi = np.clip(xi, 0, nx - 1), np.clip(yi, 0, ny - 1)
    acc = np.zeros((ngrid, nx, ny))
    n_cell = np.zeros((ngrid, nx, ny), np.int64)
    if rows.size:
        g = bin_of_rows(case['uvw'].shape[0], ngrid)[rows]
        shape = (rows.size, xi.shape[1], yi.shape[1])
        at = tuple(np.broadcast_to(a, shape) for a in (g[:, None, None], xi[:, :, None], yi[:, None, :]))
        val = fx[:, :, None] * fy[:, None, :]
        if clip:
            at, val = tuple(a[keep] for a in at), val[keep]
        np.add.at(acc, at, val)
        np.add.at(n_cell, at, 1)
    return acc.astype(dtype), n_cell


def np_weights(counts, case, robust, clip=False):
    """_counts_to_weights in the type of counts.  Briggs replaces the counts by 1 + counts * ssq BEFORE the lookup, so a
    visibility that looks up an empty cell gets 1 / (1 + 0) = 1 there and 0 under uniform weighting.  clip: a
    visibility outside the grid gets 0 (the GPU functions' defined difference) instead of failing the assertion."""
    ug, vg = grid_coords(case)
    w = np.zeros(ug.shape, counts.dtype)
    if not counts.any():
        return w
    if robust > -2:
        numsqrt = 5 * 10 ** (-robust)
        ssq = numsqrt * numsqrt / ((counts ** 2).sum() / counts.sum())
        counts = 1 + counts * ssq
    nx, ny = counts.shape
    inside = (ug >= 0) & (ug < nx) & (vg >= 0) & (vg < ny)
    if not clip:
        assert inside.all()
    c = counts[np.clip(np.floor(ug), 0, nx - 1).astype(np.int64), np.clip(np.floor(vg), 0, ny - 1).astype(np.int64)]
    np.divide(1, c, out=w, where=(c != 0) & inside)
    return w


def np_filter(counts, level):
    pos = counts > 0
    if not pos.any():
        return counts.copy()
    return np.where(pos, np.maximum(counts, np.median(counts[pos]) / level), counts)


def np_l2(vis, model_vis, mask, dof, imwgt=None):
    """(residual_vis, wgt): residual_vis = (vis - model_vis) * mask; wgt = (dof + 1) / (dof + |r|^2 / ovar) / ovar
    [* imwgt] with ovar = sum |r|^2 / sum mask, in the real type of vis; wgt None when sum mask == 0."""
    rdt = vis.real.dtype.type
    res = ((vis - model_vis) * mask).astype(vis.dtype)
    ressq = (res * res.conj()).real
    wcount = mask.sum()
    if not wcount:
        return res, None
    ovar = rdt(ressq.sum(dtype=np.float64) / wcount)
    wgt = rdt(dof + 1) / (rdt(dof) + ressq / ovar) / ovar
    return res, (wgt if imwgt is None else wgt * imwgt).astype(rdt)


# ---------------------------------------------------------------------------------------------------- the bounds
def counts_bound(ref, n_cell, k, tag):
    """|got - ref| per cell for k > 0: n_cell u for n_cell positive terms summed in any order, 128 u (times k / 6 at
    k = 12) for phi: two factors, each an exponential of an argument up to 13.8 k / 6 that carries up to 4 roundings."""
    return (n_cell + 128 * max(1.0, k / 6)) * U[tag] * ref


def briggs_bound(nx, ny, tag):
    """Relative, per visibility: the two positive-term sums on both sides (numpy's pairwise with 128-element leaves and
    any device tree) and the closing arithmetic."""
    return (4 * (16 + math.ceil(math.log2(nx * ny))) + 8) * U[tag]


def l2_bound(nvis, tag):
    return (32 + math.ceil(math.log2(nvis))) * U[tag]


def wsum_bound(nvis, tag):
    return 2 * (16 + math.ceil(math.log2(nvis))) * U[tag]
