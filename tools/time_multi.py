#!/usr/bin/env python
"""
Times the four-product paths against four single-product calls on one MI355X:

  (a) stokes   utils.stokes.run with the basis list [0, 1, 2, 3] (one k_stokes_multi pass) against four calls of the
               unchanged single entry point on the same tensors: 2^18 rows x 64 channels x 4 correlations, a weight
               spectrum, a flag per correlation, 64 antennas in 64 time bins; Jones modes full4 and diag4; fp32, fp64.
  (b) gridder  a 4-plane vis2dirty and dirty2vis against four 2-D calls on ONE cached plan: 2^17 rows x 8 channels
               = 2^20 visibilities on a 2048^2 image of 0.2 rad, |w| <= 300 wavelengths, w-gridding, weights per plane;
               epsilon 1e-4 in fp32 and 1e-7 in fp64.

Inputs come from a seed.  After WARM warm-up rounds, REPS rounds alternate the stacked call and the four single calls;
each is timed by the host clock between two device synchronisations.  Reported: median (min - max) in ms of both, their
ratio, and whether the stacked call wins by more than the spread (its max below the four calls' min).  For (a) also the
bytes the algorithm needs, from the shapes.  No profiler, one process.  The last line of the output is one JSON record.

    python tools/time_multi.py [--reps 7] [--only stokes|gridder] [--json FILE]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pfb_clean_amd.operators import gridder  # noqa: E402
from pfb_clean_amd.utils import stokes  # noqa: E402

WARM = 2
NROW, NCHAN, NC, NANT, NTIME = 1 << 18, 64, 4, 64, 64
GRID_N, GRID_ROWS, GRID_CHAN, FIELD, WMAX = 2048, 1 << 17, 8, 0.2, 300.0


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    del out
    return time.perf_counter() - t


def compare(stacked, singles, reps):
    """The two ways, alternating: dict of median / min / max seconds each."""
    for _ in range(WARM):
        stacked(), singles()
    ts, tf = [], []
    for _ in range(reps):
        ts.append(clock(stacked))
        tf.append(clock(singles))
    ts.sort(), tf.sort()
    med = lambda t: t[len(t) // 2]        # noqa: E731
    return dict(stacked_s=med(ts), stacked_min_s=ts[0], stacked_max_s=ts[-1], four_s=med(tf), four_min_s=tf[0],
                four_max_s=tf[-1], ratio=med(tf) / med(ts), beyond_spread=ts[-1] < tf[0])


def show(name, r):
    print(f"{name:34s} stacked {r['stacked_s'] * 1e3:9.3f} ms ({r['stacked_min_s'] * 1e3:.3f} - {r['stacked_max_s'] * 1e3:.3f})"
          f"   four calls {r['four_s'] * 1e3:9.3f} ms ({r['four_min_s'] * 1e3:.3f} - {r['four_max_s'] * 1e3:.3f})"
          f"   x{r['ratio']:.2f}   beyond the spread: {r['beyond_spread']}", flush=True)


def time_stokes(reps):
    rows = []
    for cdt in (torch.complex64, torch.complex128):
        rdt = torch.float32 if cdt == torch.complex64 else torch.float64
        g = torch.Generator(device='cuda').manual_seed(9)

        def unit(shape):
            return torch.randn(shape, dtype=cdt, device='cuda', generator=g)
        data = unit((NROW, NCHAN, NC))
        weight = torch.rand((NROW, NCHAN, NC), dtype=rdt, device='cuda', generator=g) * 1.5 + 0.5
        flag = (torch.rand((NROW, NCHAN, NC), device='cuda', generator=g) < 0.02).to(torch.uint8)
        full = 0.2 * unit((NTIME, NANT, NCHAN, 1, 2, 2))
        diag = torch.polar(torch.rand((NTIME, NANT, NCHAN, 1, 2), dtype=rdt, device='cuda', generator=g) * 1.5 + 0.5,
                           torch.rand((NTIME, NANT, NCHAN, 1, 2), dtype=rdt, device='cuda', generator=g) * 6.2831853)
        full[..., 0, 0], full[..., 1, 1] = diag[..., 0], diag[..., 1]
        ant1 = torch.randint(0, NANT - 1, (NROW,), device='cuda', generator=g, dtype=torch.int32)
        ant2 = ant1 + 1 + torch.randint(0, NANT, (NROW,), device='cuda', generator=g, dtype=torch.int32) % (NANT - 1 - ant1)
        tbin_counts = torch.full((NTIME,), NROW // NTIME, dtype=torch.int64)
        tbin_idx = torch.arange(NTIME, dtype=torch.int64) * (NROW // NTIME)
        e = 4 if rdt == torch.float32 else 8
        nvis = NROW * NCHAN
        read = NC * 2 * e + NC * e + NC                    # correlations, weights, flags
        out = 2 * e + e                                    # vis, wgt of one product; the mask byte once
        for mode, jones in (('full4', full.contiguous()), ('diag4', diag.contiguous())):
            def run(basis):
                return stokes.run(data, weight, stokes.W_SPECTRUM, flag, None, True, jones, tbin_idx, tbin_counts, ant1,
                                  ant2, basis)
            r = compare(lambda: run([0, 1, 2, 3]), lambda: [run(b) for b in range(4)], reps)
            # the same numbers both ways, at the sizes timed
            st = run([0, 1, 2, 3])
            worst = 0.0
            for b in range(4):
                one = run(b)
                worst = max(worst, ((st[0][b] - one[0]).abs().max() / one[0].abs().max()).item(),
                            ((st[1][b] - one[1]).abs().max() / one[1].abs().max()).item())
                assert torch.equal(st[2], one[2])
            r.update(what='stokes', mode=mode, dtype=str(rdt), bytes_stacked=nvis * (read + 4 * out + 1),
                     bytes_four=4 * nvis * (read + out + 1), bytes_ratio=4 * (read + out + 1) / (read + 4 * out + 1),
                     stacked_bytes_per_s=nvis * (read + 4 * out + 1) / r['stacked_s'], worst_rel_difference=worst)
            rows.append(r)
            show(f"stokes {mode} {rdt}", r)
            print(f"    bytes {r['bytes_four'] / 1e9:.2f} GB -> {r['bytes_stacked'] / 1e9:.2f} GB (x{r['bytes_ratio']:.2f}), "
                  f"stacked {r['stacked_bytes_per_s'] / 1e12:.2f} TB/s, planes differ from the single calls by "
                  f"{worst:.1e} of the largest element", flush=True)
        del data, weight, flag, full, diag
        torch.cuda.empty_cache()
    return rows


def time_gridder(reps):
    rows = []
    n, cell = GRID_N, FIELD / GRID_N
    for rdt, eps in ((torch.float32, 1e-4), (torch.float64, 1e-7)):
        cdt = torch.complex64 if rdt == torch.float32 else torch.complex128
        gen = torch.Generator(device='cuda').manual_seed(420)

        def uniform(shape, lo, hi, dtype=torch.float64):
            return lo + (hi - lo) * torch.rand(shape, dtype=dtype, device='cuda', generator=gen)
        freq = 1.0e9 * (1.0 + 0.02 * torch.arange(GRID_CHAN, dtype=torch.float64, device='cuda'))
        lam = gridder.C_LIGHT / freq.max().item()
        uvw = torch.stack([uniform((GRID_ROWS,), -1, 1) * 0.96 * 0.5 / cell, uniform((GRID_ROWS,), -1, 1) * 0.96 * 0.5 / cell,
                           uniform((GRID_ROWS,), -1, 1) * WMAX], dim=1).mul_(lam).contiguous()
        vis = torch.randn((4, GRID_ROWS, GRID_CHAN), dtype=cdt, device='cuda', generator=gen)
        wgt = uniform((4, GRID_ROWS, GRID_CHAN), 0.5, 1.5, rdt)
        dirty = torch.randn((4, n, n), dtype=rdt, device='cuda', generator=gen)
        kw = dict(pixsize_x=cell, pixsize_y=cell, epsilon=eps, do_wgridding=True)
        gridder.clear_plan_cache()
        miss = gridder.cache_stats['miss']

        def v2d(v, w):
            return gridder.vis2dirty(uvw, freq, v, wgt=w, npix_x=n, npix_y=n, **kw)

        def d2v(d, w):
            return gridder.dirty2vis(uvw, freq, d, wgt=w, **kw)
        for name, fn, x in (('vis2dirty', v2d, vis), ('dirty2vis', d2v, dirty)):
            r = compare(lambda: fn(x, wgt), lambda: [fn(x[k], wgt[k]) for k in range(4)], reps)
            st = fn(x, wgt)
            worst = max((torch.linalg.norm(st[k] - fn(x[k], wgt[k])) / torch.linalg.norm(st[k])).item() for k in range(4))
            plan = gridder.plan_for(uvw, freq, None, n, n, cell, cell, 0.0, 0.0, eps, True, rdt)
            r.update(what=name, dtype=str(rdt), epsilon=eps, support=plan.W, planes=len(list(plan.plane_ranges())),
                     nvis=GRID_ROWS * GRID_CHAN, worst_rel_l2_difference=worst)
            rows.append(r)
            show(f"{name} {rdt} eps {eps:g} W {plan.W}", r)
            print(f"    {r['planes']} planes; stacked planes differ from the single calls by {worst:.1e} (rel l2)", flush=True)
        assert gridder.cache_stats['miss'] == miss + 1, "every call of a configuration must find the one plan"
        del vis, wgt, dirty
        gridder.clear_plan_cache()
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--only', choices=('stokes', 'gridder'))
    ap.add_argument('--json')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_multi.py needs the GPU")
    if args.reps < 5:
        sys.exit("at least five repetitions")
    rows = []
    if args.only != 'gridder':
        rows += time_stokes(args.reps)
    if args.only != 'stokes':
        rows += time_gridder(args.reps)
    record = dict(tool='time_multi', device=torch.cuda.get_device_name(0), reps=args.reps, rows=rows)
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(record, fh, indent=1)
    print(json.dumps(record))


if __name__ == '__main__':
    main()
