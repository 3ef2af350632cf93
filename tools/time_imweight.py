#!/usr/bin/env python
"""
Times the imaging-weight functions (utils/weighting.py -> csrc/imweight.hip) on one MI355X, the table of DESIGN 4.11:
compute_counts at k = 6 and k = 0 and _counts_to_weights at robust 0 and -3, in fp32 and fp64, for 2e6 rows x 8 channels
of unmasked visibilities on a 4096^2 grid, with u, v uniform over the grid and Gaussian (sigma = nx / 16 cells) around its
centre; and as a yardstick pfb_wgrid_grid on one plane at W = 6 (epsilon 1e-4, no w-gridding) with the same visibilities.
Inputs come from a seed.  Device events around each of 10 calls after 3 warm-up calls: median, min, max.  The atomic
adds' bytes (nvis k^2 sizeof(T)) are set against the chip-wide float-atomic rate of 1.3 TB/s.  No profiler, one process.

    python tools/time_imweight.py [OUTPUT_PREFIX]        writes OUTPUT_PREFIX.json and OUTPUT_PREFIX.md
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pfb_clean_amd import _dev  # noqa: E402
from pfb_clean_amd.operators import gridder  # noqa: E402
from pfb_clean_amd.utils import weighting  # noqa: E402

NROW, NCHAN, N = 2_000_000, 8, 4096
CELL = 2.0e-5
C = 299792458.0
ATOMIC_RATE = 1.3e12
OUT = sys.argv[1] if len(sys.argv) > 1 else 'imweight_timing'


def timed(fn, warm=3, reps=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def make_uvw(kind, rng):
    freq = 1.0e9 * (1.0 + 0.001 * np.arange(NCHAN))
    if kind == 'uniform':
        ug, vg = rng.uniform(16, N - 16, NROW), rng.uniform(16, N - 16, NROW)
    else:
        ug = np.clip(N / 2 + rng.standard_normal(NROW) * N / 16, 16, N - 16)
        vg = np.clip(N / 2 + rng.standard_normal(NROW) * N / 16, 16, N - 16)
    u_cell, umax, v_cell, vmax = weighting.uv_cells(N, N, CELL, CELL)
    nf = freq[0] / C
    uvw = np.stack([(ug * u_cell - umax) / nf, (vg * v_cell - vmax) / nf, np.zeros(NROW)], axis=1)
    return torch.from_numpy(uvw).cuda(), torch.from_numpy(freq).cuda()


def main():
    rng = np.random.default_rng(5)
    rows = []
    mask = torch.ones((NROW, NCHAN), dtype=torch.uint8, device='cuda')
    nvis = NROW * NCHAN
    for kind in ('uniform', 'gaussian'):
        uvw, freq = make_uvw(kind, rng)
        for dt, size in ((torch.float32, 4), (torch.float64, 8)):
            for k in (6, 0):
                f = lambda: weighting.compute_counts(uvw, freq, mask, N, N, CELL, CELL, dt, k=k)
                med, lo, hi = timed(f)
                counts = f()
                total = counts.sum(dtype=torch.float64).item()
                nbytes = nvis * max(k, 1) ** 2 * size
                rows.append(dict(what=f'compute_counts k={k}', uv=kind, dtype=str(dt), median_s=med, min_s=lo, max_s=hi,
                                 added_bytes=nbytes, bytes_per_s=nbytes / med, share=nbytes / med / ATOMIC_RATE,
                                 check=total, max_cell=counts.max().item()))
                print(rows[-1], flush=True)
            counts = weighting.compute_counts(uvw, freq, mask, N, N, CELL, CELL, dt, k=6)
            for robust in (0.0, -3.0):
                f = lambda: weighting._counts_to_weights(counts, uvw, freq, N, N, CELL, CELL, robust)
                med, lo, hi = timed(f)
                rows.append(dict(what=f'_counts_to_weights robust={robust:g}', uv=kind, dtype=str(dt), median_s=med,
                                 min_s=lo, max_s=hi, check=f().sum(dtype=torch.float64).item()))
                print(rows[-1], flush=True)
            # the yardstick: one plane of the w-gridder at W = 6 (epsilon 1e-4) on the same (4096, 4096) grid
            gridder.clear_plan_cache()
            plan = gridder.WgridPlan(uvw, freq, mask, N // 2, N // 2, CELL, CELL, 0.0, 0.0, 1e-4, False, dt)
            assert plan.W == 6 and plan.nplanes == 1 and plan.nsorted == nvis
            val = torch.ones(plan.nsorted, dtype=plan.cdtype, device='cuda')
            f = lambda: plan.run('pfb_wgrid_grid', 0, _dev.ptr(val), _dev.ptr(plan.coord), plan.nsorted, 0, plan.nsorted,
                                 _dev.ptr(plan._grid))
            med, lo, hi = timed(f)
            nbytes = nvis * 36 * 2 * size
            rows.append(dict(what='pfb_wgrid_grid W=6 (sorted)', uv=kind, dtype=str(dt), median_s=med, min_s=lo, max_s=hi,
                             added_bytes=nbytes, bytes_per_s=nbytes / med, share=nbytes / med / ATOMIC_RATE,
                             check=plan._grid.real.sum(dtype=torch.float64).item()))
            print(rows[-1], flush=True)
            del plan, val, counts
    with open(OUT + '.json', 'w') as fh:
        json.dump(rows, fh, indent=1)
    with open(OUT + '.md', 'w') as fh:
        fh.write('| call | uv | type | median ms (min - max) | added GB | GB/s | of 1.3 TB/s |\n|---|---|---|---|---|---|---|\n')
        for r in rows:
            b = r.get('added_bytes')
            fh.write(f"| {r['what']} | {r['uv']} | {r['dtype'].replace('torch.', '')} | {r['median_s'] * 1e3:.2f} "
                     f"({r['min_s'] * 1e3:.2f} - {r['max_s'] * 1e3:.2f}) | "
                     + (f"{b / 1e9:.2f} | {r['bytes_per_s'] / 1e9:.0f} | {r['share']:.2f} |\n" if b else '- | - | - |\n'))
    print(open(OUT + '.md').read())


if __name__ == '__main__':
    main()
