"""
The case table of the band / time concatenation and the beam resampling (tests/golden/concat.npz, made from the
reference's own source by tests/golden/make_golden_concat.py), a plain-numpy statement of each function and the tests'
bounds; shared by test_cpu_concat_cases.py and test_gpu_concat.py.

OVERLAP_CASES   dicts of name, ufreq, src [dicts of vis (complex64), wgt (float32), mask (uint8), freq] and
                ref[tag] = (viso, wgto, masko) of the reference for the sources cast to the tag's types
BEAM_SUM_CASES  dicts of name, beam [float64 (9, 7)], wgt [float32] and ref[(wtag, btag)]
BEAM_EVAL_CASES dicts of name, beam (float64), l_in, m_in, l_out, m_out (1-D or 2-D) and ref[tag] (float64) for the
                beam cast to the tag's type
CHAN_IN, CHAN_REF[(nband_out, tag)], ROW_IN, ROW_REF[tag]   dataset lists: dicts of the arrays VARS and attrs {name: value}

Inputs are stored once in single precision and cast up for tag f64 (typed_sources, typed_datasets), as the maker did.

The bounds (u = 2^-24 or 2^-53 for the type T in question)
  wgto       |got - ref| <= n_c u(T) ref, n_c the number of sources that hold the channel: both sides add the same
             non-negative terms in the same order; the bound only covers a contracted multiply-add, one u per term.
  viso       per component |got - ref| <= (n_c + 4) u(T) sum_i |vis_i| wgt_i mask_i / wgto: n_c terms of two roundings
             each summed in order (first-order: n_c + 1 on the sum of moduli), one division on either side, and the
             reference's division being numpy's complex one (a product with the reciprocal: one more rounding), rounded
             up to n_c + 4.
  masko, exact zeros where masko == 0, the non-finite pattern: equal.
  wsum_i     relative (19 + max(0, ceil(log2(n / 128))) + 1) u(Tw): numpy's pairwise sum of n non-negative terms is 8
             accumulators of at most 16 terms and a 3-level tree per block of 128 (19 roundings on any path), then one
             per level of the tree over blocks; the last 1 is the rounding of the device's fp64 sum.
  beam       the wsum_i bound plus (nds + 2) u(Tb), on sum_i wsum_i |beam_i| / sum_i wsum_i: nds products and additions
             in order, the division, and the rounding of the sums to Tb.
  eval_beam  |got - ref| <= 16 u(fp64) sum_corners |w_c| |v_c| with the weights of the interval rule (beyond 1 in
             extrapolation): each weight is a product of two factors (1 - t or t, t a quotient of two differences: 4
             roundings a factor), times the value, summed over 4 corners: at most 8 + 1 + 3 = 12 roundings on a path,
             rounded up to 16 for scipy's different association.  With dtype=float32 one u(fp32) |ref| more.
  UVW, FREQ, concatenated rows and every attribute: equal.
"""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'concat.npz')
TAGS = {'f32': (np.complex64, np.float32), 'f64': (np.complex128, np.float64)}
U = {'f32': 2.0 ** -24, 'f64': 2.0 ** -53}
BEAM_TAGS = (('f32', 'f32'), ('f64', 'f64'), ('f32', 'f64'))          # (weights, beams)
BATCH = 8                                    # PFB_VIS_BATCH of include/pfb_hip.h
BLOCK = 256                                  # ENTRY_BLOCK of csrc/entry.hpp
ATTRS = ('time_out', 'time_min', 'time_max', 'timeid', 'freq_out', 'freq_min', 'freq_max', 'bandid', 'ra', 'dec')
VARS = ('VIS', 'WEIGHT', 'MASK', 'UVW', 'FREQ', 'BEAM', 'chan', 'l_beam', 'm_beam')


def _datasets(g, prefix):
    out = []
    for k in range(int(g[f'{prefix}_n'])):
        ds = {name: g[f'{prefix}_{k}_{name}'] for name in VARS}
        ds['attrs'] = {a: float(v) for a, v in zip(ATTRS, g[f'{prefix}_{k}_attrs']) if not np.isnan(v)}
        out.append(ds)
    return out


def _load():
    g = np.load(GOLDEN, allow_pickle=False)
    overlap = []
    for j, name in enumerate(g['so_names']):
        src = [{k: g[f'so{j}_s{i}_{k}'] for k in ('vis', 'wgt', 'mask', 'freq')} for i in range(int(g[f'so{j}_nds']))]
        overlap.append(dict(name=str(name), ufreq=g[f'so{j}_ufreq'], src=src,
                            ref={t: tuple(g[f'so{j}_{k}_{t}'] for k in ('viso', 'wgto', 'masko')) for t in TAGS}))
    beam_sum = []
    for j, name in enumerate(g['sb_names']):
        n = int(g[f'sb{j}_nds'])
        beam_sum.append(dict(name=str(name), beam=[g[f'sb{j}_s{i}_beam'] for i in range(n)],
                             wgt=[g[f'sb{j}_s{i}_wgt'] for i in range(n)],
                             ref={wb: g[f'sb{j}_out_{wb[0]}{wb[1]}'] for wb in BEAM_TAGS}))
    beam_eval = [dict(name=str(name), ref={t: g[f'eb{j}_out_{t}'] for t in TAGS},
                      **{k: g[f'eb{j}_{k}'] for k in ('beam', 'l_in', 'm_in', 'l_out', 'm_out')})
                 for j, name in enumerate(g['eb_names'])]
    chan_ref = {(nb, t): _datasets(g, f'cc_o{nb}_{t}') for nb in (2, 3) for t in TAGS}
    row_ref = {t: _datasets(g, f'cr_o_{t}') for t in TAGS}
    return overlap, beam_sum, beam_eval, _datasets(g, 'cc_in'), chan_ref, _datasets(g, 'cr_in'), row_ref


OVERLAP_CASES, BEAM_SUM_CASES, BEAM_EVAL_CASES, CHAN_IN, CHAN_REF, ROW_IN, ROW_REF = _load()
NBAND_NONE = 5                               # concat_chan(CHAN_IN, 5): a bin that selects no dataset


def named(cases, name):
    return next(c for c in cases if c['name'] == name)


def typed_sources(src, tag):
    cdt, rdt = TAGS[tag]
    return [dict(vis=s['vis'].astype(cdt), wgt=s['wgt'].astype(rdt), mask=s['mask'], freq=s['freq']) for s in src]


def typed_datasets(xds, tag):
    cdt, rdt = TAGS[tag]
    return [dict(ds, VIS=ds['VIS'].astype(cdt), WEIGHT=ds['WEIGHT'].astype(rdt), BEAM=ds['BEAM'].astype(rdt)) for ds in xds]


def sources_of(xds):
    return [dict(vis=ds['VIS'], wgt=ds['WEIGHT'], mask=ds['MASK'], freq=ds['FREQ']) for ds in xds]


# ------------------------------------------------------------------------------------------------ the statement
def channel_map(src, ufreq):
    """(nds, nchan_out): the channel of source i at output channel c, or -1."""
    cmap = np.full((len(src), ufreq.size), -1, np.int64)
    for i, s in enumerate(src):
        _, idx0, idx1 = np.intersect1d(s['freq'], ufreq, assume_unique=True, return_indices=True)
        cmap[i, idx1] = idx0
    return cmap


def np_sum_overlap(src, ufreq):
    """(viso, wgto, masko) in the sources' types: per component (vis * wgt) * mask and wgt * mask added in source order,
    every operation rounded on its own; a plain division where any source is unflagged, zeros elsewhere."""
    cdt, rdt = src[0]['vis'].dtype, src[0]['wgt'].dtype
    nrow = src[0]['vis'].shape[0]
    cmap = channel_map(src, ufreq)
    re, im, w = (np.zeros((nrow, ufreq.size), rdt) for _ in range(3))
    live = np.zeros((nrow, ufreq.size), bool)
    for i, s in enumerate(src):
        c1 = np.flatnonzero(cmap[i] >= 0)
        c0 = cmap[i, c1]
        f = s['mask'][:, c0].astype(rdt)
        re[:, c1] += (s['vis'].real[:, c0] * s['wgt'][:, c0]) * f
        im[:, c1] += (s['vis'].imag[:, c0] * s['wgt'][:, c0]) * f
        w[:, c1] += s['wgt'][:, c0] * f
        live[:, c1] |= s['mask'][:, c0] != 0
    with np.errstate(all='ignore'):
        re, im = np.where(live, re / w, 0).astype(rdt), np.where(live, im / w, 0).astype(rdt)
    w = np.where(live, w, 0).astype(rdt)
    return (re + 1j * im).astype(cdt), w, live.astype(np.uint8)


def np_weight_sums(wgts):
    return np.array([float(w.sum(dtype=np.float64)) for w in wgts])


def np_sum_beam(beams, wgts):
    """sum_i wsum_i beam_i [/ sum_i wsum_i] in the beams' type, the sums of the weights taken in fp64."""
    bdt = beams[0].dtype.type
    wsum = np_weight_sums(wgts)
    acc = np.zeros(beams[0].shape, bdt)
    for ws, b in zip(wsum, beams):
        acc += bdt(ws) * b
    tot = 0.0
    for ws in wsum:
        tot += ws
    return acc / bdt(tot) if tot else acc


def _cells(g, x):
    i = np.clip(np.searchsorted(g, x, side='right') - 1, 0, g.size - 2)
    return i, (x - g[i]) / (g[i + 1] - g[i])


def np_eval_beam(beam, l_in, m_in, l_out, m_out, parts=False):
    """The bilinear form on the cell of the interval rule, fp64; parts: also sum_corners |w_c| |v_c|."""
    beam = beam.astype(np.float64)
    if l_in[0] > l_in[-1]:
        l_in, beam = l_in[::-1], beam[::-1]
    if m_in[0] > m_in[-1]:
        m_in, beam = m_in[::-1], beam[:, ::-1]
    ll, mm = (l_out, m_out) if l_out.ndim == 2 else np.meshgrid(l_out, m_out, indexing='ij')
    (i, tx), (j, ty) = _cells(l_in, ll), _cells(m_in, mm)
    val, mag = 0.0, 0.0
    for di, wx in ((0, 1 - tx), (1, tx)):
        for dj, wy in ((0, 1 - ty), (1, ty)):
            val = val + beam[i + di, j + dj] * (wx * wy)
            mag = mag + np.abs(beam[i + di, j + dj]) * np.abs(wx * wy)
    return (val, mag) if parts else val


def chan_plan(xds, nband_out):
    """concat_chan's selection: None for an early return, else [(time, b, flow, fhigh, fout, freqsb, indices of the
    selected datasets)]; ValueError where a bin selects none."""
    times = np.unique([ds['attrs']['time_out'] for ds in xds])
    nband_in = np.unique([ds['attrs']['freq_out'] for ds in xds]).size
    if nband_in == nband_out or nband_in == 1:
        return None
    all_freqs = np.unique(np.concatenate([ds['chan'] for ds in xds]))
    bins = np.linspace(min(ds['attrs']['freq_min'] for ds in xds), max(ds['attrs']['freq_max'] for ds in xds), nband_out + 1)
    centers = (bins[1:] + bins[:-1]) / 2
    plan = []
    for time in times:
        for b in range(nband_out):
            flow, fhigh = bins[b], bins[b + 1]
            fb = all_freqs[all_freqs >= flow]
            fb = fb[fb <= fhigh] if b == nband_out - 1 else fb[fb < fhigh]
            sel = [k for k, ds in enumerate(xds) if ds['attrs']['time_out'] == time and
                   (flow < ds['attrs']['freq_min'] < fhigh or flow < ds['attrs']['freq_max'] < fhigh)]
            if not sel:
                raise ValueError(f'band {b} at time {time} selects no dataset')
            plan.append((time, b, flow, fhigh, np.round(centers[b], 5), fb, sel))
    return plan


def np_concat_chan(xds, nband_out):
    plan = chan_plan(xds, nband_out)
    if plan is None:
        return xds
    out = []
    for time, b, flow, fhigh, fout, fb, sel in plan:
        xdst = [xds[k] for k in sel]
        vis, wgt, mask = np_sum_overlap(sources_of(xdst), fb)
        first = xdst[0]
        out.append(dict(VIS=vis, WEIGHT=wgt, MASK=mask, UVW=first['UVW'], FREQ=fb, chan=fb, l_beam=first['l_beam'],
                        m_beam=first['m_beam'], BEAM=np_sum_beam([d['BEAM'] for d in xdst], [d['WEIGHT'] for d in xdst]),
                        attrs=dict(freq_out=fout, freq_max=fhigh, freq_min=flow, bandid=b, dec=first['attrs']['dec'],
                                   ra=first['attrs']['ra'], time_out=time,
                                   time_max=max(d['attrs']['time_max'] for d in xdst),
                                   time_min=min(d['attrs']['time_min'] for d in xdst))))
    return out


def row_plan(xds):
    """concat_row's grouping: None for one time, else per band the indices of its datasets, in order."""
    if np.unique([ds['attrs']['time_out'] for ds in xds]).size == 1:
        return None
    return [[k for k, ds in enumerate(xds) if ds['attrs']['freq_out'] == nu]
            for nu in np.unique([ds['attrs']['freq_out'] for ds in xds])]


def np_concat_row(xds):
    plan = row_plan(xds)
    if plan is None:
        return xds
    out = []
    for sel in plan:
        xdsb = [xds[k] for k in sel]
        first = xdsb[0]
        ds = {name: np.concatenate([d[name] for d in xdsb], axis=0) for name in ('WEIGHT', 'VIS', 'MASK', 'UVW')}
        ds.update(BEAM=np_sum_beam([d['BEAM'] for d in xdsb], [d['WEIGHT'] for d in xdsb]), FREQ=first['FREQ'],
                  chan=first['chan'], l_beam=first['l_beam'], m_beam=first['m_beam'])
        at = [d['attrs'] for d in xdsb]
        ds['attrs'] = dict(dec=at[0]['dec'], ra=at[0]['ra'], time_out=np.round(np.mean([a['time_out'] for a in at]), 5),
                           time_max=max(a['time_max'] for a in at), time_min=min(a['time_min'] for a in at), timeid=0,
                           freq_out=at[0]['freq_out'], freq_max=max(a['freq_max'] for a in at),
                           freq_min=min(a['freq_min'] for a in at))
        out.append(ds)
    return out


# ---------------------------------------------------------------------------------------------------- the bounds
def wsum_bound(n, tag):
    return (19 + max(0, math.ceil(math.log2(n / 128))) + 1) * U[tag]


def check_overlap(got, ref, src, ufreq, tag, label=''):
    """got, ref: (viso, wgto, masko) of the typed sources `src`.  Prints the worst figures, then asserts the bounds."""
    cdt, rdt = TAGS[tag]
    (gv, gw, gm), (rv, rw, rm) = got, ref
    assert gv.dtype == cdt and gw.dtype == rdt and gm.dtype == np.uint8
    assert gv.shape == rv.shape and gw.shape == rw.shape and gm.shape == rm.shape
    assert np.array_equal(gm, rm)
    dead = rm == 0
    assert not gv[dead].any() and not gw[dead].any()
    cmap = channel_map(src, ufreq)
    n_c = (cmap >= 0).sum(axis=0)[None, :]
    mag = np.zeros(rv.shape)
    for i, s in enumerate(src):
        c1 = np.flatnonzero(cmap[i] >= 0)
        c0 = cmap[i, c1]
        mag[:, c1] += np.abs(s['vis'][:, c0].astype(np.complex128)) * s['wgt'][:, c0].astype(np.float64) * s['mask'][:, c0]
    fin = np.isfinite(rv)
    assert np.array_equal(np.isfinite(gv), fin)
    assert np.array_equal(np.isnan(gv.real), np.isnan(rv.real)) and np.array_equal(np.isnan(gv.imag), np.isnan(rv.imag))
    live = fin & ~dead
    ew = np.abs(gw.astype(np.float64) - rw)
    bw = n_c * U[tag] * rw.astype(np.float64)
    with np.errstate(all='ignore'):
        bv = (n_c + 4) * U[tag] * mag / rw.astype(np.float64)
    d = gv.astype(np.complex128) - rv
    ev = np.maximum(np.abs(d.real), np.abs(d.imag))
    if live.any():
        print(f"{label} {tag}: viso worst err / bound {np.max(ev[live] / bv[live]):.3f}, wgto worst err {ew.max() / U[tag]:.2f} u")
    assert (ew <= bw).all()
    assert (ev[live] <= bv[live]).all()


def check_beam_sum(got, ref, beams, wgts, wtag, btag, label=''):
    assert got.dtype == TAGS[btag][1] and got.shape == ref.shape
    wsum = np_weight_sums(wgts)
    if not wsum.sum():
        assert not ref.any() and not got.any()
        return
    scale = sum(ws * np.abs(b.astype(np.float64)) for ws, b in zip(wsum, beams)) / wsum.sum()
    bound = (wsum_bound(max(w.size for w in wgts), wtag) + (len(beams) + 2) * U[btag]) * scale
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{label} w {wtag} b {btag}: beam worst err / bound {np.max(err / bound):.3f}")
    assert (err <= bound).all()


def check_beam_eval(got, ref, case, dtype=None, label=''):
    assert got.dtype == (np.float64 if dtype is None else dtype) and got.shape == ref.shape
    _, mag = np_eval_beam(case['beam'], case['l_in'], case['m_in'], case['l_out'], case['m_out'], parts=True)
    bound = 16 * U['f64'] * mag + (U['f32'] * np.abs(ref) if dtype == np.float32 else 0.0)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{label}: eval_beam worst err / bound {np.max(err / bound):.3f}")
    assert (err <= bound).all()


def check_attrs(got, ref):
    """got: {name: value} of the attributes present; equal to the reference's, name for name."""
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    for name, v in ref.items():
        assert float(got[name]) == v, (name, got[name], v)


def check_chan_dataset(got, ref, xdst, tag, label=''):
    """One output dataset of concat_chan (dict of arrays and attrs) against the reference's, xdst the typed selected
    inputs."""
    check_attrs(got['attrs'], ref['attrs'])
    for name in ('UVW', 'FREQ', 'chan', 'l_beam', 'm_beam'):
        assert np.array_equal(got[name], ref[name]), name
    check_overlap((got['VIS'], got['WEIGHT'], got['MASK']), (ref['VIS'], ref['WEIGHT'], ref['MASK']), sources_of(xdst),
                  ref['FREQ'], tag, label)
    check_beam_sum(got['BEAM'], ref['BEAM'], [d['BEAM'] for d in xdst], [d['WEIGHT'] for d in xdst], tag, tag, label)


def check_row_dataset(got, ref, xdsb, tag, label=''):
    check_attrs(got['attrs'], ref['attrs'])
    for name in ('VIS', 'WEIGHT', 'MASK', 'UVW', 'FREQ', 'chan', 'l_beam', 'm_beam'):
        assert got[name].dtype == ref[name].dtype and np.array_equal(got[name], ref[name]), name
    check_beam_sum(got['BEAM'], ref['BEAM'], [d['BEAM'] for d in xdsb], [d['WEIGHT'] for d in xdsb], tag, tag, label)
