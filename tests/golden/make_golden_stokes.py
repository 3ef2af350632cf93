#!/usr/bin/env python
"""
Golden vectors for the Stokes conversion (pfb_clean_amd/utils/stokes.py, weight_data of utils/weighting.py): inputs and
what the reference's own _weight_data makes of them -- pfb/utils/weighting.py:298-350 over the functions that
pfb/utils/stokes.py generates with sympy -- stored in stokes.npz next to this file.

Run in the BUILD container only:   python tests/golden/make_golden_stokes.py
(the reference's two source files are loaded by path and executed under tests/golden/_refstubs.py, numba's decorators
being identities there: every line that runs is the reference's, as plain Python; the tests only read the .npz file.)
Two things are added here to what _refstubs.py substitutes: a stub module numba.core.errors with
NumbaPendingDeprecationWarning, which stokes.py imports, and a str subclass with a literal_value property for pol,
product and nc, which stokes_funcs reads where numba would hand it a literal type.  stokes_funcs is memoised per
(Jones dimensions, product, pol, nc): numba compiles it once per signature, the stand-in for numba.extending.overload
would run sympy again on every call.

The layout of the file, the case table and the bounds are those of tests/stokes_cases.py, which this script imports for
the closed form.  Rules of the fixture:
  * inputs are stored once per input set, rounded to fp32 (and stored so); one fixture serves both types and a
    comparison sees arithmetic error only;
  * expected outputs are the reference's fp64 results;
  * Jones terms: diagonal amplitudes uniform in [0.5, 2] with a free phase, off-diagonals 0.2 (N(0,1) + i N(0,1)), read
    by the FULL cases only; weights and sigma uniform in [0.5, 2]; data unit complex normal;
  * the 24-variant sweep of weight_data runs at 85 x 3, the shape cases one (pol, product) per Jones mode; the 16
    no-Jones variants run through the 'sv' statements, where the reference makes Jones terms of ones;
  * the 'sv' cases feed _weight_data what stokes_cases.prepared makes of the raw columns (the two data columns
    combined, the weight form expanded in fp64, the flags merged); the reference's own preparation sits inside its
    workers' functions and cannot be called.
For every stored case the script asserts that the reference evaluated in complex64 AND in complex128 lies within K / 2
of the fp64 closed form: a case where the reference alone does not is not a parity case.

Fixed zip timestamps: two runs give identical bytes.
"""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, HERE)

import stokes_cases as sc                               # noqa: E402
from make_golden_weighting import save                  # noqa: E402


class Lit(str):
    """What numba's `literally` hands to stokes_funcs: the value under .literal_value."""
    @property
    def literal_value(self):
        return str(self)


def load_reference():
    import _refstubs
    _refstubs.install(ROOT)
    const = types.ModuleType('africanus.constants')
    const.c = 299792458.0
    sys.modules['africanus.constants'] = const
    sys.modules['quartical.utils.dask'] = _refstubs._AnyModule('quartical.utils.dask')
    errors = types.ModuleType('numba.core.errors')
    errors.NumbaPendingDeprecationWarning = type('NumbaPendingDeprecationWarning', (Warning,), {})
    sys.modules['numba.core'] = types.ModuleType('numba.core')
    sys.modules['numba.core.errors'] = sys.modules['numba.core'].errors = errors
    mods = {}
    for name, alias in (('stokes', 'pfb.utils.stokes'), ('weighting', None)):
        spec = importlib.util.spec_from_file_location('pfb_ref_' + name, f'/root/reference/pfb/utils/{name}.py')
        mods[name] = mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        if alias:
            sys.modules[alias] = mod
    ref = mods['weighting']
    generate, memo = ref.stokes_funcs, {}

    def stokes_funcs(data, jones, product, pol, nc):
        key = (jones.ndim, str(product), str(pol), str(nc))
        if key not in memo:
            memo[key] = generate(data, jones, product, pol, nc)
        return memo[key]
    ref.stokes_funcs = stokes_funcs
    return ref


# --------------------------------------------------------------------------------------------------- the inputs
def f32(a):
    return a.astype(np.complex64 if np.iscomplexobj(a) else np.float32)


def cnormal(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def draw_jones(rng, ntime, nant, nchan, ndir):
    """(ntime, nant, nchan, ndir, 2, 2)."""
    j = 0.2 * cnormal(rng, (ntime, nant, nchan, ndir, 2, 2))
    for k in range(2):
        j[..., k, k] = rng.uniform(0.5, 2.0, j.shape[:4]) * np.exp(2j * np.pi * rng.uniform(size=j.shape[:4]))
    return j


def even_bins(nrow, ntime):
    counts = np.array([nrow // ntime + (1 if t < nrow % ntime else 0) for t in range(ntime)], np.int64)
    return np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64), counts


def draw_set(rng, nrow, nchan, tbin_idx, tbin_counts, nant=7, ndir=1, flagged=0.15, autocorr=False):
    ant1 = rng.integers(0, nant - 1, nrow)
    ant2 = np.array([rng.integers(a + 1, nant) for a in ant1])
    if autocorr:
        ant2[::9] = ant1[::9]
    return dict(data=f32(cnormal(rng, (nrow, nchan, 4))), weight=f32(rng.uniform(0.5, 2.0, (nrow, nchan, 4))),
                flag=rng.uniform(size=(nrow, nchan)) < flagged, ant1=ant1.astype(np.int32), ant2=ant2.astype(np.int32),
                tbin_idx=np.asarray(tbin_idx, np.int64), tbin_counts=np.asarray(tbin_counts, np.int64),
                jones=f32(draw_jones(rng, len(tbin_idx), nant, nchan, ndir)), layout='ref')


def build(rng):
    sets, cases = [], []

    def add(name, kind, s, mode, variant, wform='spectrum', op='none', use_flag=True, use_frow=False):
        cases.append(dict(name=name, kind=kind, set=s, mode=mode, pol=variant[0], product=variant[1], wform=wform, op=op,
                          use_flag=use_flag, use_frow=use_frow))

    # ---- all 24 variants of weight_data; two directions, of which the second must not be read
    sets.append(draw_set(rng, *sc.SWEEP_SHAPE, *even_bins(sc.SWEEP_SHAPE[0], 4), ndir=2))
    for mode in sc.MODES:
        for v in sc.VARIANTS:
            add(f'sweep-{mode}-{v[0]}-{v[1]}', 'wd', 0, mode, v)
    # ---- shape edges, one variant per Jones mode
    for nrow, nchan in sc.SHAPES:
        sets.append(draw_set(rng, nrow, nchan, *even_bins(nrow, min(3, nrow)), nant=3))
        for mode in sc.MODES:
            add(f'shape-{nrow}x{nchan}-{mode}', 'wd', len(sets) - 1, mode, sc.SHAPE_VARIANT[mode])
    # ---- time-bin edges at 85 x 3
    nrow, nchan = sc.SWEEP_SHAPE
    for name, mode, idx, counts in (
            ('one', 'diag4', [0], [nrow]),
            ('empty', 'full4', [0, 30, 30, 60], [30, 0, 30, 25]),               # a bin of count 0 between two others
            ('gaps', 'diag2', [0, 10, 40], [0, 30, 30]),                        # rows 0 .. 9 and 70 .. 84 uncovered
            ('offset', 'full4', [1000, 1030, 1060], [30, 30, 25])):             # counted from the minimum
        sets.append(draw_set(rng, nrow, nchan, idx, counts))
        add(f'tbin-{name}', 'wd', len(sets) - 1, mode, sc.SHAPE_VARIANT[mode])
    # ---- stokes_vis at the composition test's shape: autocorrelations, FLAG_ROW, QuartiCal's Jones layout
    nrow, nchan = sc.COMPOSE_SHAPE
    s = draw_set(rng, nrow, nchan, *even_bins(nrow, 3), nant=5, ndir=2, autocorr=True)
    j = s['jones']                                                              # (ntime, nant, nchan, ndir, 2, 2)
    s['jones'] = np.ascontiguousarray(np.swapaxes(j.reshape(j.shape[:4] + (4,)), 1, 2))
    s['layout'] = 'qcal'
    s.update(data2=f32(0.5 * cnormal(rng, (nrow, nchan, 4))), sigma=f32(rng.uniform(0.5, 2.0, (nrow, nchan, 4))),
             wrow=f32(rng.uniform(0.5, 2.0, (nrow, 4))), flag3=rng.uniform(size=(nrow, nchan, 4)) < 0.05,
             frow=rng.uniform(size=nrow) < 0.1)
    sets.append(s)
    k = len(sets) - 1
    add('sv-plain', 'sv', k, 'noj4', ('linear', 'I'), wform='none', use_flag=False)
    add('sv-sigma-plus-diag', 'sv', k, 'diag4', ('linear', 'Q'), wform='sigma', op='+', use_frow=True)
    add('sv-spectrum-minus-full', 'sv', k, 'full4', ('circular', 'V'), op='-')
    add('sv-row-diag2', 'sv', k, 'diag2', ('circular', 'I'), wform='row', use_flag=False, use_frow=True)
    add('sv-noj2-zero', 'sv', k, 'noj2', ('linear', 'U'), wform='none')
    add('sv-row-full', 'sv', k, 'full4', ('linear', 'V'), wform='row', use_frow=True)
    add('sv-sigma-minus-diag2', 'sv', k, 'diag2', ('linear', 'Q'), wform='sigma', op='-', use_frow=True)
    add('sv-spectrum-noj4', 'sv', k, 'noj4', ('circular', 'U'), op='+', use_frow=True)
    # ---- the no-Jones instantiations, all of them: the reference runs them with its Jones terms of ones
    for mode in ('noj4', 'noj2'):
        for v in sc.VARIANTS:
            add(f'noj-{mode}-{v[0]}-{v[1]}', 'sv', k, mode, v, use_frow=True)
    return sets, cases


# ------------------------------------------------------------------------------------------------ the reference
def reference(ref, case, tag):
    """The reference's _weight_data on the case, in the type `tag`: (vis, wgt, mask).  What an 'sv' call does in front of
    the per-visibility arithmetic is stokes_cases.prepared's; Jones terms go in in the reference's layout, and a case
    without any gets ones, which is what the reference's workers make when no gain table is given."""
    s = case['set']
    cdt, rdt = sc.CDT[tag], sc.RDT[tag]
    data, weight, flag = sc.prepared(case)
    if case['mode'].startswith('noj'):
        nant = int(max(s['ant1'].max(), s['ant2'].max())) + 1
        jones = np.ones((s['tbin_idx'].size, nant, data.shape[1], 1, 2), dtype=cdt)
    else:
        full = sc.jones_ref_layout(s)
        jones = np.ascontiguousarray(full if case['mode'] == 'full4' else full[..., [0, 1], [0, 1]]).astype(cdt)
    nc = sc.ncorr(case['mode'])
    vis, wgt = ref._weight_data(sc.corr_arg(case, data).astype(cdt), sc.corr_arg(case, weight).astype(rdt), flag.copy(),
                                jones, s['tbin_idx'].copy(), s['tbin_counts'].copy(), s['ant1'], s['ant2'],
                                Lit(case['pol']), Lit(case['product']), Lit(str(nc)))
    return vis, wgt, (~flag).astype(np.uint8)


if __name__ == '__main__':
    ref = load_reference()
    rng = np.random.default_rng(2281)
    sets, cases = build(rng)
    out = {'nsets': np.array(len(sets)), 'cases': np.array([sc.encode(c) for c in cases])}
    for i, s in enumerate(sets):
        for key in sc.SET_KEYS + sc.SV_KEYS:
            if key in s:
                out[f's{i}_{key}'] = s[key]
        out[f's{i}_layout'] = np.array(s['layout'])
    worst = {tag: [0.0, 0.0] for tag in sc.EPS}
    for j, case in enumerate(cases):
        c = dict(case, set={k: (v.astype(np.complex128) if np.iscomplexobj(v) else v.astype(np.float64)
                                if isinstance(v, np.ndarray) and v.dtype.kind == 'f' else v)
                            for k, v in sets[case['set']].items()})
        cf_vis, cf_wgt, cf_mask, vis_unit, wgt_unit = sc.closed_form(c)
        res = {}
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            for tag in ('f32', 'f64'):
                r = reference(ref, c, tag)
                assert r[0].dtype == sc.CDT[tag] and r[1].dtype == sc.RDT[tag], (case['name'], r[0].dtype, r[1].dtype)
                ev, ew = sc.worst(r[0], r[1], cf_vis, cf_wgt, vis_unit, wgt_unit, tag)
                assert ev <= sc.K / 2 and ew <= sc.K / 2, (case['name'], tag, ev, ew)
                worst[tag] = [max(worst[tag][0], ev), max(worst[tag][1], ew)]
                res[tag] = r
        out[f'k{j}_vis'], out[f'k{j}_wgt'] = res['f64'][0], res['f64'][1]
        if case['kind'] == 'sv':
            assert np.array_equal(res['f64'][2], cf_mask) and np.array_equal(res['f32'][2], cf_mask)
            out[f'k{j}_mask'] = res['f64'][2]
        print(f"{case['name']}: done", flush=True)
    for tag in worst:
        print(f"reference in {tag} against the fp64 closed form: vis {worst[tag][0]:.2f}, wgt {worst[tag][1]:.2f} "
              f"of the K = 1 bound (asserted <= {sc.K / 2:g})")
    save('stokes.npz', out)
