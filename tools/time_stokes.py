#!/usr/bin/env python
"""
Times the Stokes conversion (utils/stokes.py -> csrc/stokes.hip) on one MI355X, the table of DESIGN 4.12: one launch over
2^18 rows x 64 channels x 4 correlations in fp32 with FULL, DIAG and no Jones terms, a weight spectrum and a flag per
correlation, 64 antennas in 64 time bins of equal length.  Inputs come from a seed.  Device events around each of 20
calls after 5 warm-up calls: median, min, max.  A call is the streaming kernel and the one-workgroup sum of its partials.
Bytes are those the algorithm needs, from the shapes: per visibility the correlations, weights and flags in and vis, wgt,
mask out, plus the Jones terms once (they are re-read from the caches).  The inputs (0.9 GB) exceed the 256 MiB
Infinity Cache.  No profiler, one process.

    python tools/time_stokes.py [OUTPUT_PREFIX]        writes OUTPUT_PREFIX.json and OUTPUT_PREFIX.md

The record of DESIGN 4.12 is profiles/stokes_timing.json and profiles/stokes_timing.md, which adds the kernel times of a
rocprofv3 --kernel-trace run of this script.
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pfb_clean_amd.utils import stokes  # noqa: E402

NROW, NCHAN, NC, NANT, NTIME = 1 << 18, 64, 4, 64, 64
OUT = sys.argv[1] if len(sys.argv) > 1 else 'stokes_timing'


def timed(fn, warm=5, reps=20):
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


def main():
    g = torch.Generator(device='cuda').manual_seed(9)
    dev = 'cuda'

    def unit(shape):
        return torch.randn(shape, dtype=torch.complex64, device=dev, generator=g)
    data = unit((NROW, NCHAN, NC))
    weight = torch.rand((NROW, NCHAN, NC), device=dev, generator=g) * 1.5 + 0.5
    flag = (torch.rand((NROW, NCHAN, NC), device=dev, generator=g) < 0.02).to(torch.uint8)
    full = 0.2 * unit((NTIME, NANT, NCHAN, 1, 2, 2))
    diag = torch.polar(torch.rand((NTIME, NANT, NCHAN, 1, 2), device=dev, generator=g) * 1.5 + 0.5,
                       torch.rand((NTIME, NANT, NCHAN, 1, 2), device=dev, generator=g) * 6.2831853)
    full[..., 0, 0], full[..., 1, 1] = diag[..., 0], diag[..., 1]
    ant1 = torch.randint(0, NANT - 1, (NROW,), device=dev, generator=g, dtype=torch.int32)
    ant2 = (ant1 + 1 + torch.randint(0, NANT, (NROW,), device=dev, generator=g, dtype=torch.int32) % (NANT - 1 - ant1))
    tbin_counts = torch.full((NTIME,), NROW // NTIME, dtype=torch.int64)
    tbin_idx = torch.arange(NTIME, dtype=torch.int64) * (NROW // NTIME)
    nvis = NROW * NCHAN
    per_vis = NC * 8 + NC * 4 + NC + 8 + 4 + 1
    rows = []
    for name, jones in (('FULL', full.contiguous()), ('DIAG', diag.contiguous()), ('none', None)):
        def f():
            return stokes.run(data, weight, stokes.W_SPECTRUM, flag, None, True, jones, tbin_idx, tbin_counts, ant1, ant2,
                              0)
        med, lo, hi = timed(f)
        vis, wgt, mask, rec = f()
        nbytes = nvis * per_vis + (0 if jones is None else jones.numel() * 8)
        rows.append(dict(jones=name, median_s=med, min_s=lo, max_s=hi, bytes=nbytes, bytes_per_s=nbytes / med,
                         wsum=rec.item(), unmasked=int(mask.sum().item()), finite=bool(torch.isfinite(wgt).all().item())))
        print(rows[-1], flush=True)
    with open(OUT + '.json', 'w') as fh:
        json.dump(rows, fh, indent=1)
    with open(OUT + '.md', 'w') as fh:
        fh.write('| Jones | median ms (min - max) | GB in + out | TB/s |\n|---|---|---|---|\n')
        for r in rows:
            fh.write(f"| {r['jones']} | {r['median_s'] * 1e3:.3f} ({r['min_s'] * 1e3:.3f} - {r['max_s'] * 1e3:.3f}) | "
                     f"{r['bytes'] / 1e9:.3f} | {r['bytes_per_s'] / 1e12:.2f} |\n")
    print(open(OUT + '.md').read())


if __name__ == '__main__':
    main()
