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

    python tools/time_wgrid.py [--calls 9] [--small] [--json FILE]
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


def inputs(n, nrow, rdtype, wmax, dev):
    gen = torch.Generator(device=dev)
    gen.manual_seed(420)

    def uniform(shape, lo, hi, dtype=torch.float64):
        return lo + (hi - lo) * torch.rand(shape, dtype=dtype, device=dev, generator=gen)
    cell = FIELD / n
    freq = 1.0e9 * (1.0 + 0.02 * torch.arange(NCHAN, dtype=torch.float64, device=dev))
    lam = gridder.C_LIGHT / freq.max().item()
    uvw = torch.stack([uniform((nrow,), -1, 1) * 0.96 * 0.5 / cell, uniform((nrow,), -1, 1) * 0.96 * 0.5 / cell,
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=9)
    ap.add_argument('--small', action='store_true', help='512^2 only')
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    if args.calls < 7:
        ap.error('--calls must be at least 7')
    dev = _dev.require_device()
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
