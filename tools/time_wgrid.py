#!/usr/bin/env python
"""
Times the visibility-space Hessian (operators/hessian.py::_hessian_impl -> operators/gridder.py -> csrc/wgrid.hip) on
one MI355X, on the two workloads of the table in DESIGN 4.10:

    512^2,  0.36 M unmasked visibilities, fp64, epsilon 1e-7, |w| <= 300 wavelengths    (W = 9, 34 of 35 planes used)
    2048^2, 3.6 M,                        fp32, epsilon 1e-4, |w| <= 1500 wavelengths   (W = 6, 127 of 128)

both with weights, a mask that keeps 70 % of the samples, and a beam.  Inputs are built on the device from a seed: a
field of 0.2 rad across (so that delta w = 1 / (4 max|nm1|) is 25 wavelengths at either size), 8 channels from 1.00 to
1.14 GHz, u and v uniform up to 96 % of the grid's half width at the top channel, w uniform, weights in [0.5, 1.5],
beam in [0.5, 1], x = randn.

The plan is warmed by two calls; then --calls (>= 7) calls are timed one by one, wall clock between two device
synchronisations.  Reported per size: min / median / max in ms, the support, the planes that hold visibilities, and
gridder.cache_stats['miss'] before and after the timed calls -- equal, so every timed call was a plan hit.  No profiler,
no counters, one process.  The last line of the output is one JSON record.

    python tools/time_wgrid.py [--calls 9] [--small] [--json FILE] [--reproducible]

--reproducible compares the two gridders instead ("The tile-owned gridder"): the default plan (k_grid, float
atomics) against the plan of reproducible=True (k_grid_tile) on the same arrays -- the two sizes above and a third set,
the first size with u and v drawn from a normal distribution of 4 % of the grid's half width, so that a few central
tiles hold most visibilities (the tile gridder walks a tile's list serially: its expected weak spot).  Timed per size,
the two modes alternated round by round, --calls rounds after two warm ones: the gridding step alone over every used
plane (device events around the launches of all planes, reported per plane), a whole vis2dirty (host clock between two
synchronisations), and the construction of a plan (order, and for the reproducible mode its target map); median, min
and max each.  The two modes' images are compared (relative l2), and two reproducible calls must agree bit for bit.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pfb_clean_amd import _dev  # noqa: E402
from pfb_clean_amd.operators import gridder  # noqa: E402
from pfb_clean_amd.operators.hessian import _hessian_impl  # noqa: E402

# (n, rows, dtype, epsilon, max |w| in wavelengths); rows x 8 channels x 0.7 unmasked
CONFIGS = [(512, 64000, torch.float64, 1e-7, 300.0), (2048, 640000, torch.float32, 1e-4, 1500.0)]
NCHAN, FIELD, KEEP = 8, 0.2, 0.7


def inputs(n, nrow, rdtype, wmax, dev, central=None):
    gen = torch.Generator(device=dev)
    gen.manual_seed(420)

    def uniform(shape, lo, hi, dtype=torch.float64):
        return lo + (hi - lo) * torch.rand(shape, dtype=dtype, device=dev, generator=gen)
    cell = FIELD / n
    freq = 1.0e9 * (1.0 + 0.02 * torch.arange(NCHAN, dtype=torch.float64, device=dev))
    lam = gridder.C_LIGHT / freq.max().item()
    def baseline(shape):
        if central is None:
            return uniform(shape, -1, 1) * 0.96
        return (central * torch.randn(shape, dtype=torch.float64, device=dev, generator=gen)).clamp_(-0.96, 0.96)
    uvw = torch.stack([baseline((nrow,)) * 0.5 / cell, baseline((nrow,)) * 0.5 / cell,
                       uniform((nrow,), -1, 1) * wmax], dim=1).mul_(lam).contiguous()
    wgt = uniform((nrow, NCHAN), 0.5, 1.5, rdtype)
    mask = (uniform((nrow, NCHAN), 0, 1) < KEEP).to(torch.uint8)
    beam = uniform((n, n), 0.5, 1.0, rdtype)
    x = torch.randn((n, n), dtype=rdtype, device=dev, generator=gen)
    torch.cuda.synchronize()
    return dict(x=x, uvw=uvw, weight=wgt, vis_mask=mask, freq=freq, beam=beam, cell=cell)


def time_config(n, nrow, rdtype, eps, wmax, dev, calls):
    a = inputs(n, nrow, rdtype, wmax, dev)

    def call():
        return _hessian_impl(a['x'], a['uvw'], a['weight'], a['vis_mask'], a['freq'], a['beam'], cell=a['cell'],
                             do_wgridding=True, epsilon=eps, double_accum=False)
    for _ in range(2):
        out = call()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    plan = gridder.plan_for(a['uvw'], a['freq'], a['vis_mask'], n, n, a['cell'], a['cell'], 0.0, 0.0, eps, True, rdtype)
    miss = gridder.cache_stats['miss']
    ms = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    used = sum(1 for _ in plan.plane_ranges())
    res = {'shape': [n, n], 'dtype': str(rdtype).split('.')[-1], 'epsilon': eps, 'wmax': wmax, 'support': plan.W,
           'unmasked': plan.nsorted, 'planes': plan.nplanes, 'planes_used': used, 'calls': calls,
           'min_ms': float(np.min(ms)), 'median_ms': float(np.median(ms)), 'max_ms': float(np.max(ms)),
           'per_plane_ms': float(np.median(ms)) / used, 'miss_before': miss, 'miss_after': gridder.cache_stats['miss']}
    del a, plan, out
    gridder.clear_plan_cache()
    torch.cuda.empty_cache()
    return res


def _stats(ms):
    return {'median': float(np.median(ms)), 'min': float(np.min(ms)), 'max': float(np.max(ms))}


def time_modes(tag, n, nrow, rdtype, eps, wmax, dev, calls, central=None):
    """The default and the reproducible gridder on one set of arrays, alternated."""
    a = inputs(n, nrow, rdtype, wmax, dev, central)
    cdtype = _dev.CPLX_OF[rdtype]
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    vis = torch.randn((nrow, NCHAN, 2), dtype=rdtype, device=dev, generator=gen)
    vis = torch.view_as_complex(vis).contiguous().to(cdtype)
    modes = (False, True)

    def build(rep):
        return gridder.WgridPlan(a['uvw'], a['freq'], a['vis_mask'], n, n, a['cell'], a['cell'], 0.0, 0.0, eps, True,
                                 rdtype, reproducible=rep)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    plans, build_ms = {}, {m: [] for m in modes}
    for r in range(4):          # the first round loads code objects and tables; three are kept
        for m in modes:
            ms, plan = wall(lambda: build(m))
            if r:
                build_ms[m].append(ms)
            if m in plans:
                plans[m].close()
            plans[m] = plan

    def grid_step(plan):
        """The gridding launches of every used plane, on the plan's own buffers."""
        g, val = plan._grid, plan._slots[1]
        for p, s0, s1 in plan.plane_ranges():
            if plan.reproducible:
                plan.run('pfb_wgrid_grid_tile', p, _dev.ptr(val), _dev.ptr(plan.coord), plan.nsorted, *plan._map_args,
                         _dev.ptr(g))
            else:
                plan.run('pfb_wgrid_grid', p, _dev.ptr(val), _dev.ptr(plan.coord), plan.nsorted, s0, s1, _dev.ptr(g))

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    images, step_ms, call_ms = {}, {m: [] for m in modes}, {m: [] for m in modes}
    for m in modes:
        images[m] = plans[m].vis2dirty(vis, a['weight'], False)          # fills val; the first warm call
    used = sum(1 for _ in plans[False].plane_ranges())
    assert used == sum(1 for _ in plans[True].plane_ranges())
    for r in range(calls + 2):
        for m in modes:
            step = events(lambda: grid_step(plans[m]))
            ms, img = wall(lambda: plans[m].vis2dirty(vis, a['weight'], False))
            if r >= 2:
                step_ms[m].append(step / used)
                call_ms[m].append(ms)
            if m:
                assert torch.equal(img, images[True]), 'two reproducible calls differ'
    diff = float((images[True].double() - images[False].double()).norm() / images[False].double().norm())
    tm = plans[True].tile_map
    per_target = (tm[1][1:] - tm[1][:-1])
    res = {'set': tag, 'shape': [n, n], 'dtype': str(rdtype).split('.')[-1], 'epsilon': eps, 'support': plans[True].W,
           'unmasked': plans[True].nsorted, 'planes_used': used, 'rounds': calls, 'targets': int(tm[0].numel()),
           'pairs': int(tm[2].numel()), 'max_pairs_per_target': int(per_target.max()),
           'rel_l2_between_modes': diff,
           'grid_step_per_plane_us': {('tile' if m else 'atomic'): {k: 1e3 * v for k, v in _stats(step_ms[m]).items()}
                                      for m in modes},
           'vis2dirty_ms': {('tile' if m else 'atomic'): _stats(call_ms[m]) for m in modes},
           'plan_build_ms': {('tile' if m else 'atomic'): _stats(build_ms[m]) for m in modes}}
    for plan in plans.values():
        plan.close()
    del a, plans, images, vis
    torch.cuda.empty_cache()
    return res


def main_modes(args, dev):
    sets = [('uniform',) + CONFIGS[0]] + ([] if args.small else [('uniform',) + CONFIGS[1]])
    sets.append(('central',) + CONFIGS[0] + (0.04,))
    res = []
    for cfg in sets:
        r = time_modes(*cfg[:6], dev, args.calls, *cfg[6:])
        res.append(r)
        for what, unit in (('grid_step_per_plane_us', 'us per plane'), ('vis2dirty_ms', 'ms'), ('plan_build_ms', 'ms')):
            row = '; '.join(f"{mode} {v['median']:.1f} ({v['min']:.1f} .. {v['max']:.1f})" for mode, v in r[what].items())
            print(f"{r['set']} {r['shape'][0]}^2 {r['dtype']} W {r['support']} {r['unmasked']} vis {r['planes_used']} "
                  f"planes: {what} [{unit}] {row}", file=sys.stderr, flush=True)
        print(f"    targets {r['targets']}, pairs {r['pairs']} (at most {r['max_pairs_per_target']} a target); the modes' "
              f"images differ by {r['rel_l2_between_modes']:.2e} (relative l2)", file=sys.stderr, flush=True)
    print(json.dumps({'wgrid_reproducible': res}))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump({'wgrid_reproducible': res}, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=9)
    ap.add_argument('--small', action='store_true', help='512^2 only')
    ap.add_argument('--json', default=None)
    ap.add_argument('--reproducible', action='store_true',
                    help='compare the default gridder and the tile-owned gridder of reproducible=True')
    args = ap.parse_args()
    if args.calls < 7:
        ap.error('--calls must be at least 7')
    dev = _dev.require_device()
    if args.reproducible:
        return main_modes(args, dev)
    res = []
    for cfg in (CONFIGS[:1] if args.small else CONFIGS):
        r = time_config(*cfg, dev, args.calls)
        res.append(r)
        print(f"{r['shape'][0]}^2 {r['dtype']} eps {r['epsilon']:g}: W {r['support']}, {r['unmasked']} visibilities, "
              f"{r['planes_used']} of {r['planes']} planes; _hessian_impl min / median / max "
              f"{r['min_ms']:.2f} / {r['median_ms']:.2f} / {r['max_ms']:.2f} ms over {r['calls']} calls; "
              f"cache_stats['miss'] {r['miss_before']} -> {r['miss_after']}", file=sys.stderr, flush=True)
    print(json.dumps({'wgrid_hessian': res}))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump({'wgrid_hessian': res}, f, indent=1)
    if any(r['miss_after'] != r['miss_before'] for r in res):
        sys.exit('a timed call built a plan')


if __name__ == '__main__':
    main()
