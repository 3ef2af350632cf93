#!/usr/bin/env python
"""
Times the band-coupled Hessian of the parametrised forward step (workers/fwdbwd.py:246-252, 327-334) on one MI355X: the
fused route (ParamHessian -> pfb_hessparam_apply, pfb_pcg_solve_param) beside the route that exists without it, the
closure composition `2 dhf(psf_convolve(df(v))) + sigmainv v` driven by the generic PCG (`_nofuse`).

Inputs are built on the device from a seed: psfhat from a Gaussian-tapered Poisson uv coverage, j = randn, x0 = 0.1 randn,
freq = linspace(1e9, 2e9, nband), sigma 0.8, lscale 0.5, sigmainv = std(j).

Reports, per configuration (4 x 2048^2 and 8 x 4096^2 float32, modes 'id' and 'exp'):
  solve   pcg(partial(hessian_psf, ...), j, tol=0, maxit=minit=--iters) fused and generic, alternating for --runs warm
          runs, repeated --repeats times: per repeat the median of the device-event times, over the repeats their range
          (the run-to-run spread a difference has to exceed); ms per iteration = solve / iters.
  apply   one ParamHessian apply beside one evaluation of the closure composition, timed the same way.
and prints one JSON line; the exit status is non-zero when a fused route is slower than the other by more than the
spread.

    python tools/time_hessparam.py [--runs 5] [--repeats 3] [--iters 20] [--small] [--json FILE]
"""
import argparse
import json
import os
import sys
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pfb_clean_amd import _dev  # noqa: E402
from pfb_clean_amd.operators.hessian import ParamHessian, hessian_psf  # noqa: E402
from pfb_clean_amd.operators.psf import psf_convolve_cube, clear_plan_cache  # noqa: E402
from pfb_clean_amd.opt.pcg import pcg, _as_hessian  # noqa: E402
from pfb_clean_amd.utils.misc import setup_parametrisation  # noqa: E402

CONFIGS = [(4, 2048), (8, 4096)]


def inputs(nband, n, dev):
    gen = torch.Generator(device=dev)
    gen.manual_seed(420)
    P = Q = 2 * n
    u = torch.fft.fftfreq(P, device=dev)[:, None]
    v = torch.fft.rfftfreq(Q, device=dev)[None, :]
    rate = (4 * torch.exp(-(u ** 2 + v ** 2) / (2 * 0.12 ** 2))).expand(nband, -1, -1)
    W = torch.poisson(rate, generator=gen)
    W = W / (nband * W.sum(dim=(1, 2), keepdim=True) * 2 / (P * Q))     # peak of the PSF ~ 1 / nband
    psfhat = W.to(torch.complex64).contiguous()
    j = torch.randn((nband, n, n), dtype=torch.float32, device=dev, generator=gen)
    x0 = 0.1 * torch.randn((nband, n, n), dtype=torch.float32, device=dev, generator=gen)
    torch.cuda.synchronize()
    return psfhat, j, x0


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(routes, runs, repeats):
    """{name: {'medians', 'median', 'min', 'max', 'range'}} of the device-event times of the routes run in turn."""
    for fn in routes.values():
        fn()
    torch.cuda.synchronize()
    med = {k: [] for k in routes}
    for _ in range(repeats):
        t = {k: [] for k in routes}
        for _ in range(runs):
            for k, fn in routes.items():
                t[k].append(event_ms(fn))
        for k in routes:
            med[k].append(float(np.median(t[k])))
    out = {}
    for k, m in med.items():
        m = np.array(m)
        out[k] = {'medians': m.tolist(), 'median': float(np.median(m)), 'min': float(m.min()), 'max': float(m.max()),
                  'range': float(m.max() - m.min())}
    return out


def not_slower(t, a, b):
    return bool(t[a]['median'] <= t[b]['median'] + max(t[a]['range'], t[b]['range']))


def time_config(nband, n, mode, dev, runs, repeats, iters):
    psfhat, j, x0 = inputs(nband, n, dev)
    sigmainv = float(j.std().item())
    _, _, dfunc, dhfunc = setup_parametrisation(mode, sigma=0.8, freq=np.linspace(1e9, 2e9, nband), lscale=0.5)
    conv = partial(psf_convolve_cube, None, None, None, psfhat, 2 * n)
    df, dhf = partial(dfunc, x0), partial(dhfunc, x0)
    A = partial(hessian_psf, conv, x0, sigmainv, df, dhf)
    G = partial(hessian_psf, conv, x0, sigmainv, df, dhf, _nofuse=True)
    H = _as_hessian(A, j)
    assert isinstance(H, ParamHessian) and _as_hessian(G, j) is None
    kw = dict(tol=0.0, maxit=iters, minit=iters, verbosity=0)
    # the two routes agree before they are timed
    xf, xg = pcg(A, j, **kw), pcg(G, j, **kw)
    out = torch.empty_like(j)
    af, ag = H(j, out=out), G(j)
    res = {'shape': [nband, n, n], 'dtype': 'float32', 'mode': mode, 'iters': iters, 'sigmainv': sigmainv,
           'solve_rel_diff': float((xf - xg).abs().max() / xg.abs().max()),
           'apply_rel_diff': float((af - ag).abs().max() / ag.abs().max())}
    del xf, xg, af, ag
    res['solve_ms'] = alternate({'fused': lambda: pcg(A, j, **kw), 'generic': lambda: pcg(G, j, **kw)}, runs, repeats)
    res['apply_ms'] = alternate({'fused': lambda: H(j, out=out), 'generic': lambda: G(j)}, 4 * runs, repeats)
    for k in ('fused', 'generic'):
        res['solve_ms'][k]['per_iteration'] = res['solve_ms'][k]['median'] / iters
    res['solve_fused_not_slower_beyond_spread'] = not_slower(res['solve_ms'], 'fused', 'generic')
    res['apply_fused_not_slower_beyond_spread'] = not_slower(res['apply_ms'], 'fused', 'generic')
    del psfhat, j, x0, out, H, A, G, conv, df, dhf
    clear_plan_cache()
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--small', action='store_true', help='4 x 2048^2 only')
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    dev = _dev.require_device()
    res = []
    for nband, n in (CONFIGS[:1] if args.small else CONFIGS):
        for mode in ('id', 'exp'):
            r = time_config(nband, n, mode, dev, args.runs, args.repeats, args.iters)
            res.append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
    print(json.dumps({'hessparam': res}))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump({'hessparam': res}, f, indent=1)
    slower = [(r['shape'], r['mode'], k) for r in res for k in ('solve', 'apply')
              if not r[k + '_fused_not_slower_beyond_spread']]
    if slower:
        sys.exit(f'fused route slower than the closure composition beyond the spread at {slower}')


if __name__ == '__main__':
    main()
