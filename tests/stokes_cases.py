"""
The Stokes conversion's case table (tests/golden/stokes.npz, made from the reference's own source by
tests/golden/make_golden_stokes.py), the closed form of the reference's generated functions in plain numpy, and the
tests' per-element bounds; shared by make_golden_stokes.py, test_cpu_stokes_cases.py and test_gpu_stokes.py.

SETS    input sets, dicts of data (nrow, nchan, 4) complex, weight (nrow, nchan, 4), flag (nrow, nchan), ant1, ant2,
        tbin_idx, tbin_counts and jones, (ntime, nant, nchan, ndir, 2, 2) in the reference's layout ('layout' = 'ref') or
        (ntime, nchan, nant, ndir, 4) in QuartiCal's ('qcal'); the stokes_vis set also has data2, sigma, wrow (nrow, 4),
        flag3 (nrow, nchan, 4) and frow.  Every value is exactly representable in fp32 and stored so; loaded widened.
CASES   dicts of name, kind ('wd': weight_data, 'sv': stokes_vis), set, mode, pol, product and, for 'sv', wform, op,
        use_flag, use_frow; ref_vis, ref_wgt (and ref_mask for 'sv') are the reference's fp64 results.
        A two-correlation case reads correlations 0 and 3 of its set, a DIAG case the diagonal of its Jones terms.

The statement: with Gp, Gq the Jones matrices of a row's antennas at its time bin and channel, V the 2 x 2 matrix of its
correlations, w their weights and B the basis matrix of (pol, product),
    vis = 1/2 tr(B^H Gp^-1 V Gq^-H)          wgt = sum_ab w_ab |(Gp B Gq^H)_ab|^2
and zeros where the visibility is flagged or no time bin covers its row.  With two correlations V = diag(v0, v1) and
w01 = w10 = 1.

The bounds, per element (K = 16, eps the machine epsilon of the type under test):
    |vis - ref| <= K eps kp kq 1/2 sum_ab |B_ab| (|adj Gp| |V| |adj Gq|^T)_ab / |det Gp det Gq|,
                   k = (|g00 g11| + |g01 g10|) / |det G|
    |wgt - ref| <= K eps sum_ab w_ab ((|Gp| |B| |Gq|^T)_ab)^2
The longest path of the closed form has about ten roundings; on this input family the reference's own complex64
evaluation stays within 2.1 of the K = 1 vis bound and 4.0 eps of wgt, its complex128 evaluation within 3.2 and 3.9.
make_golden_stokes.py asserts, for every stored case, that the reference in both types lies within K / 2 of the fp64
closed form.
"""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'stokes.npz')
K = 16
EPS = {'f32': 2.0 ** -23, 'f64': 2.0 ** -52}
CDT = {'f32': np.complex64, 'f64': np.complex128}
RDT = {'f32': np.float32, 'f64': np.float64}
BLOCK = 256                                  # STK_BLOCK of csrc/stokes.hip: a workgroup takes BLOCK // nchan whole rows
MODES = ('diag4', 'diag2', 'full4')          # the Jones modes of weight_data; stokes_vis adds 'noj4', 'noj2'
VARIANTS = [(pol, product) for pol in ('linear', 'circular') for product in 'IQUV']
# the basis table: the four distinct matrices and the (pol, product) that read them
MATRICES = (np.array([[1, 0], [0, 1]], complex), np.array([[1, 0], [0, -1]], complex),
            np.array([[0, 1], [1, 0]], complex), np.array([[0, 1j], [-1j, 0]], complex))
BASIS = {('linear', 'I'): 0, ('linear', 'Q'): 1, ('linear', 'U'): 2, ('linear', 'V'): 3,
         ('circular', 'I'): 0, ('circular', 'V'): 1, ('circular', 'Q'): 2, ('circular', 'U'): 3}
# shape edges: nchan = 1, 3, 64, 65 and, per nchan, nrow = 1 and one below / above a multiple of the rows a workgroup
# takes (BLOCK // nchan = 256, 85, 4, 3); 300 channels: one row per workgroup, its lanes striding over the channels
SHAPES = [(1, 1), (255, 1), (257, 1), (1, 3), (84, 3), (86, 3), (1, 64), (3, 64), (5, 64), (1, 65), (2, 65), (4, 65),
          (2, 300)]
SHAPE_VARIANT = {'diag4': ('linear', 'Q'), 'diag2': ('circular', 'V'), 'full4': ('linear', 'V')}
SWEEP_SHAPE = (85, 3)
COMPOSE_SHAPE = (63, 3)                      # the visibilities of wgrid_cases' '32x24-eps1e-05'
SET_KEYS = ('data', 'weight', 'flag', 'ant1', 'ant2', 'tbin_idx', 'tbin_counts', 'jones')
SV_KEYS = ('data2', 'sigma', 'wrow', 'flag3', 'frow')
META = ('name', 'kind', 'set', 'mode', 'pol', 'product', 'wform', 'op', 'use_flag', 'use_frow')


def rows_per_group(nchan):
    return max(1, BLOCK // nchan)


def ncorr(mode):
    return 2 if mode.endswith('2') else 4


def encode(case):
    return '|'.join(str(case[k]) for k in META)


def decode(line):
    c = dict(zip(META, line.split('|')))
    c['set'] = int(c['set'])
    c['use_flag'], c['use_frow'] = c['use_flag'] == 'True', c['use_frow'] == 'True'
    return c


_loaded = None


def load():
    """(SETS, CASES) of the fixture, read once."""
    global _loaded
    if _loaded is None:
        g = np.load(GOLDEN, allow_pickle=False)
        sets = []
        for i in range(int(g['nsets'])):
            s = {k: g[f's{i}_{k}'] for k in SET_KEYS + SV_KEYS if f's{i}_{k}' in g.files}
            s['layout'] = str(g[f's{i}_layout'])
            for k in ('data', 'data2', 'jones'):
                if k in s:
                    s[k] = s[k].astype(np.complex128)
            for k in ('weight', 'sigma', 'wrow'):
                if k in s:
                    s[k] = s[k].astype(np.float64)
            sets.append(s)
        cases = []
        for j, line in enumerate(g['cases']):
            c = decode(str(line))
            c['set'] = sets[c['set']]
            c['ref_vis'], c['ref_wgt'] = g[f'k{j}_vis'], g[f'k{j}_wgt']
            if c['kind'] == 'sv':
                c['ref_mask'] = g[f'k{j}_mask']
            cases.append(c)
        _loaded = (sets, cases)
    return _loaded


def cases_of(kind=None, prefix=None):
    return [c for c in load()[1] if (kind is None or c['kind'] == kind) and (prefix is None or c['name'].startswith(prefix))]


def case_named(name):
    return next(c for c in load()[1] if c['name'] == name)


# ----------------------------------------------------------------------------------------------- a case's operands
def row_bins(nrow, tbin_idx, tbin_counts):
    """The time bin of every row, -1 where none covers it; bins count from min(tbin_idx)."""
    idx = np.asarray(tbin_idx, np.int64) - np.min(tbin_idx)
    out = np.full(nrow, -1, np.int64)
    for t, (i, n) in enumerate(zip(idx, tbin_counts)):
        out[i:min(i + n, nrow)] = t
    return out


def jones_ref_layout(s):
    """(ntime, nant, nchan, ndir, 2, 2) of a set."""
    j = s['jones']
    if s['layout'] == 'qcal':
        j = np.swapaxes(j, 1, 2)
        j = j.reshape(j.shape[:4] + (2, 2))
    return j


def jones_arg(case, layout=None):
    """The Jones argument of the case's call: None, (..., 2) for a DIAG mode, (..., 2, 2) (or QuartiCal's (..., 4)) for
    FULL, in the set's own layout."""
    s, mode = case['set'], case['mode']
    if mode.startswith('noj'):
        return None
    j = s['jones']
    if s['layout'] == 'qcal':
        return np.ascontiguousarray(j if mode == 'full4' else j[..., [0, 3]])
    return np.ascontiguousarray(j if mode == 'full4' else j[..., [0, 1], [0, 1]])


def corr_arg(case, a):
    """a (..., 4) as the case's number of correlations: all four, or the first and the last."""
    return np.ascontiguousarray(a if ncorr(case['mode']) == 4 else a[..., [0, 3]])


def prepared(case):
    """data, weight (nrow, nchan, 4) and flag (nrow, nchan) bool in fp64 as the case's call forms them before the
    per-visibility arithmetic: for 'sv' the two columns combined, the weight form expanded, and the flags of the
    correlations, of the rows and of the autocorrelations merged."""
    s = case['set']
    nrow, nchan = s['data'].shape[:2]
    data, weight = s['data'], s['weight']
    flag = s['flag'].astype(bool)
    if case['kind'] == 'sv':
        if case['op'] != 'none':
            data = data + s['data2'] if case['op'] == '+' else data - s['data2']
        weight = {'none': np.ones(data.shape), 'sigma': 1.0 / s['sigma'] ** 2 if 'sigma' in s else None,
                  'spectrum': weight, 'row': np.broadcast_to(s['wrow'][:, None, :], data.shape) if 'wrow' in s else None
                  }[case['wform']]
        frow = s['ant1'] == s['ant2']
        if case['use_frow']:
            frow = frow | s['frow'].astype(bool)
        flag = np.broadcast_to(frow[:, None], (nrow, nchan))
        if case['use_flag']:
            flag = corr_arg(case, s['flag3']).astype(bool).any(axis=2) | flag
    return data, weight, np.array(flag)


def operands(case):
    """V, W (nrow, nchan, 2, 2), flag (nrow, nchan) bool, covered (nrow,) bool, Gp, Gq (nrow, nchan, 2, 2) in fp64."""
    s, mode = case['set'], case['mode']
    nrow, nchan = s['data'].shape[:2]
    data, weight, flag = prepared(case)
    V = np.zeros((nrow, nchan, 2, 2), complex)
    W = np.ones((nrow, nchan, 2, 2))
    if ncorr(mode) == 4:
        V[:], W[:] = data.reshape(nrow, nchan, 2, 2), weight.reshape(nrow, nchan, 2, 2)
    else:
        for k, c in ((0, 0), (1, 3)):
            V[..., k, k], W[..., k, k] = data[..., c], weight[..., c]
    bins = row_bins(nrow, s['tbin_idx'], s['tbin_counts'])
    covered = bins >= 0
    G = np.zeros((2, nrow, nchan, 2, 2), complex)
    G[..., 0, 0] = G[..., 1, 1] = 1.0
    if not mode.startswith('noj'):
        J = jones_ref_layout(s)
        for k, ant in enumerate((s['ant1'], s['ant2'])):
            G[k] = J[np.maximum(bins, 0), ant, :, 0]
        if mode != 'full4':
            G[..., 0, 1] = G[..., 1, 0] = 0.0
    return V, W, flag, covered, G[0], G[1]


def _adj(G):
    A = np.empty_like(G)
    A[..., 0, 0], A[..., 0, 1], A[..., 1, 0], A[..., 1, 1] = G[..., 1, 1], -G[..., 0, 1], -G[..., 1, 0], G[..., 0, 0]
    return A


def _det(G):
    return G[..., 0, 0] * G[..., 1, 1] - G[..., 0, 1] * G[..., 1, 0]


def _h(G):
    return np.conj(np.swapaxes(G, -1, -2))


def closed_form(case):
    """(vis, wgt, mask, vis_unit, wgt_unit): the statement in fp64 and the bounds at K eps = 1."""
    V, W, flag, covered, Gp, Gq = operands(case)
    B = MATRICES[BASIS[(case['pol'], case['product'])]]
    dp, dq = _det(Gp), _det(Gq)
    X = _adj(Gp) @ V @ _h(_adj(Gq)) / (dp * np.conj(dq))[..., None, None]
    vis = 0.5 * (np.conj(B) * X).sum(axis=(-1, -2))
    wgt = (W * np.abs(Gp @ B @ _h(Gq)) ** 2).sum(axis=(-1, -2))
    kappa = [(np.abs(G[..., 0, 0] * G[..., 1, 1]) + np.abs(G[..., 0, 1] * G[..., 1, 0])) / np.abs(_det(G)) for G in (Gp, Gq)]
    aX = np.abs(_adj(Gp)) @ np.abs(V) @ np.swapaxes(np.abs(_adj(Gq)), -1, -2)
    vis_unit = kappa[0] * kappa[1] * 0.5 * (np.abs(B) * aX).sum(axis=(-1, -2)) / np.abs(dp * dq)
    wgt_unit = (W * (np.abs(Gp) @ np.abs(B) @ np.swapaxes(np.abs(Gq), -1, -2)) ** 2).sum(axis=(-1, -2))
    live = ~flag & covered[:, None]
    z = np.zeros_like
    return (np.where(live, vis, z(vis)), np.where(live, wgt, z(wgt)), (~flag).astype(np.uint8),
            np.where(live, vis_unit, z(vis_unit)), np.where(live, wgt_unit, z(wgt_unit)))


def worst(got_vis, got_wgt, ref_vis, ref_wgt, vis_unit, wgt_unit, tag):
    """The largest |got - ref| in units of eps x the per-element bound at K = 1, for vis and wgt; an element whose
    bound is zero (flagged, uncovered, a structural zero) must be exact: inf otherwise."""
    out = []
    for got, ref, unit in ((got_vis, ref_vis, vis_unit), (got_wgt, ref_wgt, wgt_unit)):
        err = np.abs(np.asarray(got).astype(ref.dtype) - ref)
        with np.errstate(divide='ignore', invalid='ignore'):
            q = np.where(unit > 0, err / (EPS[tag] * unit), np.where(err == 0, 0.0, np.inf))
        out.append(float(q.max()) if q.size else 0.0)
    return tuple(out)


def wsum_bound(wgt, tag):
    """|wsum - fsum(wgt)|: K eps_T sum wgt for the elements and the rounding of the result to T, plus an fp64 sum of
    n positive terms in any order."""
    total = math.fsum(np.asarray(wgt, np.float64).ravel())
    return (K * EPS[tag] + wgt.size * EPS['f64']) * total
