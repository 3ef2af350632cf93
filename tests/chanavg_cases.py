"""
Channel averaging (csrc/stokes.hip: k_chan_average, k_chan_average_lane): the seeded inputs, the oracle
and the bounds; shared by test_cpu_chanavg_cases.py, test_gpu_chanavg.py and test_gpu_single_stokes.py.

The statement.  With n = chan_average >= 1, nchan_out = ceil(nchan / n); bin j covers channels [j n, min((j + 1) n,
nchan)).  Per row, bin and product, over the bin's LIVE samples (unflagged and covered by a time bin):
    wgt_out = sum wgt_i     vis_out = sum wgt_i vis_i / wgt_out, exactly 0 where wgt_out == 0     mask_out = any(mask_i)
Samples that are not live are selected out: NaN or Inf in flagged data or weights reach no output.  There is no reference
program for this (africanus is not available); the oracle is stokes_cases.closed_form -- pinned to the reference within
K / 2 by make_golden_stokes.py -- followed by the statement in fp64.

Input sets are dicts in the form stokes_cases.closed_form accepts ('sv' cases, QuartiCal's Jones layout), every value
exactly representable in fp32, drawn from a seed per (nrow, nchan, n, variant).  Every set holds, where its shape has
room: a fully flagged bin in a live row, a bin with exactly one live channel, an autocorrelation row, an uncovered row
(unflagged: mask 1, vis = wgt = 0), and NaN / Inf in flagged data, data2, weights and sigma.  With fewer than three rows
one row cannot be both: variant 0 leaves the last row uncovered, variant 1 makes it an autocorrelation.

The bounds, per element, eps of the type under test, K = stokes_cases.K; U_i, Wu_i closed_form's vis_unit and wgt_unit,
m the bin's length, sums over the bin's live samples, W = sum w_i, S = sum w_i |v_i|, R the reference mean:
    |wgt - W| <= eps [K sum Wu_i + (m - 1) W]
    |vis - R| <= eps [(K sum (w_i U_i + Wu_i |v_i|) + m S) / W + |R| ((K sum Wu_i + (m - 1) W) / W + 2)]
first order: the inherited per-sample bounds, one rounding per product, m - 1 additions, the division.  For
average_channels alone, on inputs exact in the type, K = 0.  An element whose bound is zero must be exact.
wsum: stokes_cases.wsum_bound of the averaged reference weights.
"""
import math
import warnings

import numpy as np

import stokes_cases as sc

K = sc.K
# k_chan_average takes LANE_MAX < chan_average <= LDS_MAX (STK_AVG_LANE_MAX, STK_BLOCK), k_chan_average_lane the rest
LANE_MAX, LDS_MAX = 4, 256
# (nrow, nchan, n): the smallest shapes at which the grouping can go wrong
SHAPES = [(5, 1, 2), (86, 3, 2), (86, 3, 3), (5, 64, 2), (5, 64, 7), (5, 64, 64), (4, 65, 2), (4, 65, 13), (2, 255, 4),
          (2, 256, 4), (2, 257, 4), (2, 300, 7), (2, 300, 256), (2, 600, 256), (2, 600, 257), (1, 600, 600)]
# the 256-channel edge once more at the smallest n of the LDS kernel (n = 4 above is the lane kernel's)
EXTRA_SHAPES = [(2, 255, 5), (2, 256, 5), (2, 257, 5)]
SWEEP_SHAPES = [(86, 3, 2), (2, 300, 7)]     # 5 Jones modes x 4 bases
STACK_SHAPES = [(86, 3, 3), (2, 257, 4), (2, 600, 257)]      # whole rows per workgroup, one row, the wide kernel
FORM_SHAPE = (5, 64, 7)
ALL_MODES = ('diag4', 'diag2', 'full4', 'noj4', 'noj2')
FEATURES = ('flagged_bin', 'one_live', 'autocorr', 'uncovered', 'nan_flagged')


def nout_of(nchan, n):
    return -(-nchan // n)


# ----------------------------------------------------------------------------------------------------- the inputs
def _f32(a):
    return a.astype(np.complex64 if np.iscomplexobj(a) else np.float32)


def _cnormal(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


_sets = {}


def draw_set(nrow, nchan, n, variant=0):
    """The input set of a shape (cached; do not write into it)."""
    key = (nrow, nchan, n, variant)
    if key in _sets:
        return _sets[key]
    rng = np.random.default_rng([2611, nrow, nchan, n, variant])
    nant, ntime = 5, min(3, nrow)
    ant1 = rng.integers(0, nant - 1, nrow)
    ant2 = np.array([rng.integers(a + 1, nant) for a in ant1])
    # the rows: the last one uncovered (variant 0) or an autocorrelation (variant 1, and the last but one of >= 3 rows)
    uncovered = nrow >= 3 or (nrow == 2 and variant == 0)
    auto_row = nrow - 2 if nrow >= 3 else nrow - 1 if nrow == 2 and variant == 1 else None
    if auto_row is not None:
        ant2[auto_row] = ant1[auto_row]
    ncov = nrow - 1 if uncovered else nrow
    ntime = min(ntime, ncov)
    counts = np.array([ncov // ntime + (1 if t < ncov % ntime else 0) for t in range(ntime)], np.int64)
    tbin_idx = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64) + 1000      # counted from the minimum
    nlive_rows = ncov - (1 if auto_row is not None and auto_row < ncov else 0)
    jones = 0.2 * _cnormal(rng, (ntime, nchan, nant, 1, 4))
    for k in (0, 3):
        jones[..., k] = rng.uniform(0.5, 2.0, jones.shape[:4]) * np.exp(2j * np.pi * rng.uniform(size=jones.shape[:4]))
    data = _f32(_cnormal(rng, (nrow, nchan, 4)))
    data2 = _f32(0.5 * _cnormal(rng, (nrow, nchan, 4)))
    weight, sigma = (_f32(rng.uniform(0.5, 2.0, (nrow, nchan, 4))) for _ in range(2))
    wrow = _f32(rng.uniform(0.5, 2.0, (nrow, 4)))
    # flags on correlation 0, which the two-correlation cases read as well
    flag3 = np.zeros((nrow, nchan, 4), bool)
    flag3[..., 0] = rng.uniform(size=(nrow, nchan)) < 0.08
    flag3[..., 3] = rng.uniform(size=(nrow, nchan)) < 0.02
    frow = np.zeros(nrow, bool)
    if nlive_rows >= 4:
        frow[2] = True
    nout = nout_of(nchan, n)
    last = slice((nout - 1) * n, nchan)
    # row 0 is live: its last bin keeps exactly one channel, its first bin (a second live row's, when there is one
    # bin) none
    flag3[0, last, :] = False
    flag3[0, last, 0] = True
    flag3[0, (nout - 1) * n + (nchan - 1 - (nout - 1) * n) // 2, 0] = False
    if nout >= 2:
        flag3[0, 0:n, 0] = True
    elif nlive_rows >= 2:
        flag3[1, :, 0] = True
    # NaN and Inf where correlation 0 is flagged, and in the row weight of the autocorrelation
    rows, chans = np.nonzero(flag3[..., 0])
    for k, (r, c) in enumerate(zip(rows, chans)):
        data[r, c, k % 4] = (np.nan, np.inf, complex(-np.inf, np.nan))[k % 3]
        data2[r, c, (k + 2) % 4] = (np.inf, np.nan)[k % 2]
        weight[r, c, (k + 1) % 4] = (np.inf, np.nan, -np.inf)[k % 3]
        sigma[r, c, (k + 3) % 4] = (np.nan, np.inf, -np.inf)[k % 3]
    if auto_row is not None:
        wrow[auto_row, 1] = np.nan
    s = dict(data=data.astype(np.complex128), data2=data2.astype(np.complex128), weight=weight.astype(np.float64),
             sigma=sigma.astype(np.float64), wrow=wrow.astype(np.float64), flag=np.zeros((nrow, nchan), bool), flag3=flag3,
             frow=frow, ant1=ant1.astype(np.int32), ant2=ant2.astype(np.int32), tbin_idx=tbin_idx, tbin_counts=counts,
             jones=_f32(jones).astype(np.complex128), layout='qcal')
    _sets[key] = s
    return s


def case(shape, mode, pol, product, wform='spectrum', op='none', use_frow=True, variant=0, label='case'):
    """A case in stokes_cases' form plus n, shape and -- for a stacked product -- the letters; flag3 is always read (the
    sets hold NaN under it)."""
    nrow, nchan, n = shape
    return dict(name=f'{label}-{nrow}x{nchan}-n{n}-{mode}-{pol}-{product}-{wform}{op if op != "none" else ""}', kind='sv',
                set=draw_set(nrow, nchan, n, variant), mode=mode, pol=pol, product=product, wform=wform, op=op,
                use_flag=True, use_frow=use_frow, n=n, shape=shape)


def shape_cases():
    return [case(s, 'full4', 'linear', 'I', label='shape') for s in SHAPES + EXTRA_SHAPES]


def sweep_cases():
    """5 Jones modes x 4 bases; with two rows the bases alternate between the set's two variants."""
    return [case(s, mode, 'linear', product, variant=(b % 2 if s[0] < 3 else 0), label='sweep')
            for s in SWEEP_SHAPES for mode in ALL_MODES for b, product in enumerate('IQUV')]


def stack_cases():
    return [case(s, mode, pol, product, label='stack') for s in STACK_SHAPES
            for mode, pol, product in (('full4', 'linear', 'IQUV'), ('diag4', 'circular', 'QU'))]


def form_cases():
    """Every weight form, both column operators and a call without FLAG_ROW, once."""
    return [case(FORM_SHAPE, 'diag4', 'linear', 'Q', wform='none', use_frow=False, label='form'),
            case(FORM_SHAPE, 'full4', 'circular', 'V', wform='sigma', op='+', label='form'),
            case(FORM_SHAPE, 'diag2', 'linear', 'I', wform='spectrum', op='-', label='form'),
            case(FORM_SHAPE, 'noj4', 'linear', 'U', wform='row', label='form')]


def all_cases():
    return shape_cases() + sweep_cases() + stack_cases() + form_cases()


def ids(cases):
    return [c['name'] for c in cases]


def sv_args(c, tag, **over):
    """The keyword arguments of stokes_vis for a case (without chan_average): data, weights and Jones terms in the type
    under test."""
    s = c['set']
    cdt, rdt = sc.CDT[tag], sc.RDT[tag]
    j = sc.jones_arg(c)
    args = dict(data=sc.corr_arg(c, s['data']).astype(cdt), ant1=s['ant1'], ant2=s['ant2'], tbin_idx=s['tbin_idx'],
                tbin_counts=s['tbin_counts'], poltype=c['pol'], product=c['product'],
                jones=None if j is None else j.astype(cdt), precision={'f32': 'single', 'f64': 'double'}[tag],
                flag=sc.corr_arg(c, s['flag3']))
    if c['op'] != 'none':
        args.update(data2=sc.corr_arg(c, s['data2']).astype(cdt), operator=c['op'])
    if c['wform'] == 'sigma':
        args['sigma'] = sc.corr_arg(c, s['sigma']).astype(rdt)
    elif c['wform'] != 'none':
        args['weight'] = sc.corr_arg(c, s['wrow' if c['wform'] == 'row' else 'weight']).astype(rdt)
    if c['use_frow']:
        args['frow'] = s['frow']
    args.update(over)
    return args


# ----------------------------------------------------------------------------------------------------- the oracle
def average(vis, wgt, mask, live, n):
    """The statement in the arrays' own arithmetic (fp64 for the oracle): vis, wgt (nrow, nchan), mask bytes, live bool
    -> vis_out, wgt_out, mask_out with ceil(nchan / n) channels.  Selection, not multiplication by zero."""
    nrow, nchan = wgt.shape
    nout = nout_of(nchan, n)
    vo, wo = np.zeros((nrow, nout), vis.dtype), np.zeros((nrow, nout), wgt.dtype)
    mo = np.zeros((nrow, nout), np.uint8)
    for j in range(nout):
        sl = slice(j * n, min((j + 1) * n, nchan))
        L = live[:, sl]
        with np.errstate(invalid='ignore', over='ignore'):
            wv = wgt[:, sl] * vis[:, sl]
        W = np.where(L, wgt[:, sl], 0).sum(axis=1)
        S = np.where(L, wv, 0).sum(axis=1)
        with np.errstate(invalid='ignore', divide='ignore'):
            vo[:, j] = np.where(W != 0, S / np.where(W != 0, W, 1), 0)
        # the mean of one live sample is that sample: w v / w without its two roundings
        one = (L.sum(axis=1) == 1) & (W != 0)
        vo[:, j] = np.where(one, np.where(L, vis[:, sl], 0).sum(axis=1), vo[:, j])
        wo[:, j] = W
        mo[:, j] = (np.asarray(mask)[:, sl] != 0).any(axis=1)
    return vo, wo, mo


def units(vis, wgt, live, vis_unit, wgt_unit, n, k=K):
    """The bounds over eps: (vis_bound, wgt_bound) per averaged element, from the fp64 samples and their K = 1 units."""
    nrow, nchan = wgt.shape
    nout = nout_of(nchan, n)
    bv, bw = np.zeros((nrow, nout)), np.zeros((nrow, nout))
    for j in range(nout):
        sl = slice(j * n, min((j + 1) * n, nchan))
        m = sl.stop - sl.start
        L = live[:, sl]

        def tot(a):
            return np.where(L, a, 0).sum(axis=1)
        with np.errstate(invalid='ignore', over='ignore'):
            W, S = tot(wgt[:, sl]), tot(wgt[:, sl] * np.abs(vis[:, sl]))
            swu = tot(wgt_unit[:, sl])
            inh = tot(wgt[:, sl] * vis_unit[:, sl] + wgt_unit[:, sl] * np.abs(vis[:, sl]))
            R = np.abs(tot(wgt[:, sl] * vis[:, sl]))
        bw[:, j] = k * swu + (m - 1) * W
        ok = W != 0
        Ws = np.where(ok, W, 1)
        bv[:, j] = np.where(ok, (k * inh + m * S) / Ws + R / Ws * ((k * swu + (m - 1) * W) / Ws + 2), 0)
    return bv, bw


def live_of(c):
    """(live, covered) of a case: (nrow, nchan) and (nrow,) bool."""
    s = c['set']
    covered = sc.row_bins(s['data'].shape[0], s['tbin_idx'], s['tbin_counts']) >= 0
    return ~sc.prepared(c)[2] & covered[:, None], covered


_oracles = {}


def oracle(c, n=None):
    """dict of the case at chan_average n (the case's own by default): vis, wgt (fp64; a leading product axis for a
    stacked case), mask, the bounds over eps vis_unit, wgt_unit at K, and the un-averaged samples sample_vis,
    sample_wgt, sample_mask, live.  Computed once per (case, n); do not write into it."""
    n = c['n'] if n is None else n
    key = (c['name'], n)
    if key in _oracles:
        return _oracles[key]
    letters = list(c['product']) if len(c['product']) > 1 else [c['product']]
    live, _ = live_of(c)
    planes = []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                          # the NaN of the flagged samples, selected out below
        for p in letters:
            vis, wgt, mask, vu, wu = sc.closed_form(dict(c, product=p))
            vo, wo, mo = average(vis, wgt, mask, live, n)
            bv, bw = units(vis, wgt, live, vu, wu, n)
            planes.append((vo, wo, bv, bw, vis, wgt))
    stack = (lambda k: np.stack([p[k] for p in planes])) if len(c['product']) > 1 else (lambda k: planes[0][k])
    out = dict(vis=stack(0), wgt=stack(1), mask=mo, vis_unit=stack(2), wgt_unit=stack(3), sample_vis=stack(4),
               sample_wgt=stack(5), sample_mask=mask, live=live)
    _oracles[key] = out
    return out


def worst(got, ref, unit, tag):
    """max |got - ref| / (eps unit); an element whose bound is zero must be exact: inf otherwise."""
    err = np.abs(np.asarray(got).astype(ref.dtype) - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(unit > 0, err / (sc.EPS[tag] * unit), np.where(err == 0, 0.0, np.inf))
    q = np.where(np.isnan(q), np.inf, q)
    return float(q.max()) if q.size else 0.0


def wsum_check(wsum, ref_wgt, ref_mask, tag):
    """(error, bound) of one plane's wsum against math.fsum of the reference weights where the mask is set."""
    sel = ref_wgt[ref_mask != 0]
    return abs(float(wsum) - math.fsum(sel)), sc.wsum_bound(sel, tag)


def exact_inputs(c, tag):
    """The un-averaged oracle samples rounded to the type under test -- inputs that are exact in it -- as (vis, wgt,
    mask) in that type, for average_channels alone."""
    o = oracle(c)
    return o['sample_vis'].astype(sc.CDT[tag]), o['sample_wgt'].astype(sc.RDT[tag]), o['sample_mask']


def tight(vis, wgt, mask, n):
    """The reference and the K = 0 bounds over eps of average_channels on (vis, wgt, mask) as they are: live = mask != 0.
    Planes stacked when vis has three axes."""
    v, w = np.asarray(vis).astype(np.complex128), np.asarray(wgt).astype(np.float64)
    live = np.asarray(mask) != 0
    z = np.zeros(w.shape[-2:])
    res = []
    for vp, wp in (zip(v, w) if v.ndim == 3 else [(v, w)]):
        vo, wo, mo = average(vp, wp, mask, live, n)
        res.append((vo, wo, *units(vp, wp, live, z, z, n, k=0)))
    pick = (lambda k: np.stack([r[k] for r in res])) if v.ndim == 3 else (lambda k: res[0][k])
    return dict(vis=pick(0), wgt=pick(1), mask=mo, vis_unit=pick(2), wgt_unit=pick(3))


def sequential(vis, wgt, mask, n):
    """The statement evaluated in the arrays' own type the way a lane does: every product and every addition rounded on
    its own, in channel order, then the division."""
    nrow, nchan = wgt.shape
    nout = nout_of(nchan, n)
    vo, wo = np.zeros((nrow, nout), vis.dtype), np.zeros((nrow, nout), wgt.dtype)
    for j in range(nout):
        sw, sv = np.zeros(nrow, wgt.dtype), np.zeros(nrow, vis.dtype)
        for ch in range(j * n, min((j + 1) * n, nchan)):
            L = np.asarray(mask)[:, ch] != 0
            sw = np.where(L, sw + wgt[:, ch], sw).astype(wgt.dtype)
            sv = np.where(L, sv + (wgt[:, ch] * vis[:, ch]).astype(vis.dtype), sv).astype(vis.dtype)
        with np.errstate(invalid='ignore', divide='ignore'):
            vo[:, j] = np.where(sw != 0, sv / np.where(sw != 0, sw, 1), 0)
        wo[:, j] = sw
    return vo, wo


def features(c):
    """Which of FEATURES the case's inputs hold."""
    s = c['set']
    nrow, nchan = s['data'].shape[:2]
    n = c['n']
    live, covered = live_of(c)
    flag = sc.prepared(c)[2]
    out = set()
    auto = s['ant1'] == s['ant2']
    if auto.any():
        out.add('autocorr')
    if (~covered & ~flag.all(axis=1)).any():
        out.add('uncovered')
    row_live = live.any(axis=1)
    for j in range(nout_of(nchan, n)):
        sl = slice(j * n, min((j + 1) * n, nchan))
        cnt = live[:, sl].sum(axis=1)
        if (row_live & flag[:, sl].all(axis=1)).any():
            out.add('flagged_bin')
        if (cnt == 1).any() and (sl.stop - sl.start > 1 or nchan == 1):
            out.add('one_live')
    raw = np.concatenate([s['data'][flag].real.ravel(), s['data'][flag].imag.ravel(), s['weight'][flag].ravel()])
    if np.isnan(raw).any() and np.isinf(raw).any() and np.isfinite(s['data'][live]).all() \
            and np.isfinite(s['weight'][live]).all():
        out.add('nan_flagged')
    return out
