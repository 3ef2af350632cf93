#!/usr/bin/env python
"""
Times channel averaging behind the Stokes pass (utils/stokes.py -> csrc/stokes.hip: k_stokes, then k_chan_average), the
table of DESIGN 4.16: 20 000 rows x 512 channels x 4 correlations with FULL Jones terms, a weight spectrum and a flag per
correlation, 32 antennas in 20 time bins, Stokes I, in fp32 and fp64: the pass alone, and the pass followed by the
averaging at chan_average 4 and 16.  Inputs come from a seed.  The fp32 inputs (0.5 GB) exceed the 256 MiB Infinity
Cache; the pass's fp32 outputs (0.13 GB) do not.

A repetition is a window of CALLS back-to-back calls between two device events after WARM warm-up calls, its figure the
window's time over CALLS; the versions alternate, five repetitions each.  The spread of a version is the range of its five
figures.  A call is every launch of its path: the streaming kernel(s) and the one-workgroup sums of the partials.
Two levels, a table each:
    device   the C entry points on buffers made once (pfb_stokes_vis, pfb_chan_average): the host only enqueues, so a
             window runs at the speed of the kernels;
    python   stokes.run(chan_average=n) as stokes_vis calls it: with every call's host work (the check and upload of the
             time bins, the index casts, the output allocations), which at this size is about as long as the fp32 kernel.
No profiler, one process.

    python tools/time_chanavg.py [OUTPUT_PREFIX]        writes OUTPUT_PREFIX.json and OUTPUT_PREFIX.md

DESIGN 4.16 also records the figures of the averaging fused into the pass, a kernel that was measured with this procedure
and not kept.
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pfb_clean_amd import _dev, _lib  # noqa: E402
from pfb_clean_amd.utils import stokes  # noqa: E402

NROW, NCHAN, NC, NANT, NTIME = 20000, 512, 4, 32, 20
WARM, CALLS, REPS = 10, 100, 5
AVERAGES = (1, 4, 16)
OUT = sys.argv[1] if len(sys.argv) > 1 else 'chanavg_timing'


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / CALLS


def main():
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = 'cuda'
    lib = _lib.load()
    rows = []
    for cdt in (torch.complex64, torch.complex128):
        rdt = torch.float32 if cdt == torch.complex64 else torch.float64
        g = torch.Generator(device=dev).manual_seed(9)
        data = torch.randn((NROW, NCHAN, NC), dtype=cdt, device=dev, generator=g)
        weight = torch.rand((NROW, NCHAN, NC), dtype=rdt, device=dev, generator=g) * 1.5 + 0.5
        flag = (torch.rand((NROW, NCHAN, NC), device=dev, generator=g) < 0.02).to(torch.uint8)
        jones = 0.2 * torch.randn((NTIME, NANT, NCHAN, 1, 2, 2), dtype=cdt, device=dev, generator=g)
        diag = torch.polar(torch.rand((NTIME, NANT, NCHAN, 1, 2), dtype=rdt, device=dev, generator=g) * 1.5 + 0.5,
                           torch.rand((NTIME, NANT, NCHAN, 1, 2), dtype=rdt, device=dev, generator=g) * 6.2831853)
        jones[..., 0, 0], jones[..., 1, 1] = diag[..., 0], diag[..., 1]
        jones = jones.contiguous()
        ant1 = torch.randint(0, NANT - 1, (NROW,), device=dev, generator=g, dtype=torch.int32)
        ant2 = (ant1 + 1 + torch.randint(0, NANT, (NROW,), device=dev, generator=g, dtype=torch.int32) % (NANT - 1 - ant1))
        tbin_counts = torch.full((NTIME,), NROW // NTIME, dtype=torch.int64)
        tbin_idx = torch.arange(NTIME, dtype=torch.int64) * (NROW // NTIME)
        esize = 4 if rdt == torch.float32 else 8
        nvis = NROW * NCHAN
        read = nvis * (NC * 2 * esize + NC * esize + NC) + jones.numel() * 2 * esize
        plain_out = nvis * (3 * esize + 1)
        # the device level: every buffer made once, the C entry points called as stokes.run calls them
        ti, tc = tbin_idx.to(dev), tbin_counts.to(dev)
        work, rec = _dev.scratch()[0], torch.zeros(1, dtype=torch.float64, device=dev)
        pvis = torch.empty((NROW, NCHAN), dtype=cdt, device=dev)
        pwgt = torch.empty((NROW, NCHAN), dtype=rdt, device=dev)
        pmask = torch.empty((NROW, NCHAN), dtype=torch.uint8, device=dev)
        avis, awgt, amask = torch.empty_like(pvis), torch.empty_like(pwgt), torch.empty_like(pmask)
        p, code = _dev.ptr, _dev.code(rdt)

        def device_call(n):
            _lib.check(lib.pfb_stokes_vis(code, stokes.FULL4, 0, p(data), None, 0, p(weight), stokes.W_SPECTRUM, p(flag), NC,
                                          None, 1, p(jones), 1, NTIME, NANT, p(ti), p(tc), 0, p(ant1), p(ant2), NROW, NCHAN,
                                          p(pvis), p(pwgt), p(pmask), p(rec), p(work), _dev.stream()))
            if n > 1:
                _lib.check(lib.pfb_chan_average(code, 1, p(pvis), p(pwgt), p(pmask), NROW, NCHAN, n, p(avis), p(awgt),
                                                p(amask), p(rec), p(work), _dev.stream()))

        def python_call(n):
            return stokes.run(data, weight, stokes.W_SPECTRUM, flag, None, True, jones, tbin_idx, tbin_counts, ant1, ant2, 0,
                              chan_average=n)
        for level, call in (('device', device_call), ('python', python_call)):
            fns = {n: (lambda n=n: call(n)) for n in AVERAGES}
            for fn in fns.values():
                for _ in range(WARM):
                    fn()
            torch.cuda.synchronize()
            ts = {n: [] for n in AVERAGES}
            for _ in range(REPS):
                for n, fn in fns.items():
                    ts[n].append(window(fn))
            for n in AVERAGES:
                t = sorted(ts[n])
                nbytes = read + plain_out + (0 if n == 1 else plain_out + plain_out // n)
                rows.append(dict(level=level, dtype=str(rdt).replace('torch.', ''), chan_average=n, seconds=t,
                                 median_s=t[REPS // 2], spread_s=t[-1] - t[0], bytes=nbytes,
                                 bytes_per_s=nbytes / t[REPS // 2]))
                print(rows[-1], flush=True)
        vis, wgt, mask, wsum = python_call(4)
        print(f"{rdt}: wsum {wsum.item()!r}, unmasked {int(mask.sum().item())}, finite "
              f"{bool(torch.isfinite(wgt).all().item())}", flush=True)
        del data, weight, flag, jones, pvis, pwgt, pmask, avis, awgt, amask
        torch.cuda.empty_cache()
    with open(OUT + '.json', 'w') as fh:
        json.dump(rows, fh, indent=1)
    with open(OUT + '.md', 'w') as fh:
        fh.write('| level | type | chan_average | ms per call (spread) | over the pass alone, ms | GB in + out | TB/s |\n'
                 '|---|---|---|---|---|---|---|\n')
        for r in rows:
            base = next(b for b in rows if (b['level'], b['dtype'], b['chan_average']) == (r['level'], r['dtype'], 1))
            fh.write(f"| {r['level']} | {r['dtype']} | {r['chan_average']} | {r['median_s'] * 1e3:.3f} "
                     f"({r['spread_s'] * 1e3:.3f}) | {(r['median_s'] - base['median_s']) * 1e3:.3f} | "
                     f"{r['bytes'] / 1e9:.3f} | {r['bytes_per_s'] / 1e12:.2f} |\n")
    print(open(OUT + '.md').read())


if __name__ == '__main__':
    main()
