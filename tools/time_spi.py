#!/usr/bin/env python
"""
Times the spectral-index fit on one MI355X against the route that exists without it.

Input: an (nband, N, N) fp32 cube of noisy power laws and a beam cube in [0.3, 1], built on the device; a seeded
fraction of the pixels (--fractions, default 1 % and 100 %) carries flux, the rest is 0 and falls to the threshold.

Reports, per fraction
  mask pass  pfb_spi_mask, median / min / max of --runs device-event times and TB/s of the two cubes it reads
  fit        pfb_spi_fit on the compacted components (tol = 1e-5), the same statistics, and components per second
  device     wall time of fit_spi on the device cubes, everything included (work buffer, count read, compaction,
             NaN maps, not-converged read)
  host       what a caller does today, on this machine's CPU: .cpu().numpy() of both cubes, then the numpy oracle
             of tests/spi_cases.py.  Above --host-comps components the oracle's fit runs on the first --host-comps
             of them and its time is scaled to all (stated in the output); its maps are checked against the device's
             on the components it did fit
and prints one JSON line.  There is no pass / fail threshold.  --shape NX NY takes the place of --n for a plane that is
not square (4097 x 4095: odd npix, the form of the mask pass for planes off the 16-byte grid); --mask-only stops after
the mask pass, which is what an A/B of two builds of the library (PFB_HIP_LIB) needs.

    python tools/time_spi.py [--n 4096 | --shape NX NY] [--nband 8] [--runs 10] [--fractions 0.01 1.0] [--mask-only]
                             [--json FILE]
"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from pfb_clean_amd import _dev, _lib  # noqa: E402
from pfb_clean_amd.utils import spi  # noqa: E402
import spi_cases as sc  # noqa: E402

THRESHOLD, PB_MIN = 2.0 ** -14, 0.25


def cubes(nband, shape, frac, freqs, ref_freq, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(420)
    alpha = torch.rand(shape, generator=g, device=dev, dtype=torch.float64) * 3.0 - 2.0
    I0 = 10.0 ** (torch.rand(shape, generator=g, device=dev, dtype=torch.float64) * 4.0 - 3.0)
    on = torch.rand(shape, generator=g, device=dev) < frac
    image = torch.empty((nband,) + shape, dtype=torch.float32, device=dev)
    beam = torch.empty((nband,) + shape, dtype=torch.float32, device=dev)
    for b in range(nband):
        beam[b] = torch.rand(shape, generator=g, device=dev) * 0.7 + 0.3
        noise = 1.0 + 0.05 * torch.randn(shape, generator=g, device=dev, dtype=torch.float64)
        image[b] = torch.where(on, I0 * beam[b] * (freqs[b] / ref_freq) ** alpha * noise, 0.0).to(torch.float32)
    torch.cuda.synchronize()
    return image, beam


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(t):
    t = np.array(t)
    return {'median': float(np.median(t)), 'min': float(t.min()), 'max': float(t.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--shape', type=int, nargs=2, default=None, metavar=('NX', 'NY'))
    ap.add_argument('--mask-only', action='store_true')
    ap.add_argument('--nband', type=int, default=8)
    ap.add_argument('--runs', type=int, default=10)
    ap.add_argument('--fractions', type=float, nargs='+', default=[0.01, 1.0])
    ap.add_argument('--host-comps', type=int, default=1 << 18)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    nband = args.nband
    nx, ny = args.shape or (args.n, args.n)
    npix = nx * ny
    dev = _dev.require_device()
    lib = _lib.load()
    freqs = np.linspace(0.9e9, 1.7e9, nband)
    weights = np.linspace(0.5, 2.0, nband)
    ref_freq = 1.3e9
    lnx, w, ref = spi._bands(freqs, weights, ref_freq)
    res = {'shape': [nband, nx, ny], 'dtype': 'float32', 'lib': _lib.LIB_PATH, 'runs': args.runs, 'cases': []}
    for frac in args.fractions:
        image, beam = cubes(nband, (nx, ny), frac, freqs, ref_freq, dev)
        code, nbytes = _dev.code(image.dtype), 2 * image.numel() * 4
        work = torch.empty(lib.pfb_spi_work_bytes(npix) // 8, dtype=torch.int64, device=dev)

        def run_mask():
            _lib.check(lib.pfb_spi_mask(code, image.data_ptr(), beam.data_ptr(), nband, npix, PB_MIN, THRESHOLD,
                                        work.data_ptr(), _dev.stream()))
        run_mask()
        ncomps = int(work[lib.pfb_comps_work_bytes(npix) // 8 - 1].item())
        if args.mask_only:
            torch.cuda.synchronize()
            tm = [event_ms(run_mask) for _ in range(args.runs)]
            res['cases'].append({'fraction': frac, 'ncomps': ncomps, 'GB_read': nbytes / 1e9,
                                 'mask_ms': dict(stats(tm), TBps_median=nbytes / float(np.median(tm)) / 1e9)})
            continue
        Ix = torch.empty(ncomps, dtype=torch.int64, device=dev)
        Iy = torch.empty(ncomps, dtype=torch.int64, device=dev)
        _lib.check(lib.pfb_comps_compact(npix, ny, work.data_ptr(), Ix.data_ptr(), Iy.data_ptr(), _dev.stream()))
        maps = torch.full((4, nx, ny), float('nan'), dtype=image.dtype, device=dev)
        notconv = torch.empty(1, dtype=torch.int64, device=dev)

        def run_fit():
            _lib.check(lib.pfb_spi_fit(code, image.data_ptr(), beam.data_ptr(), nband, npix, ny, Ix.data_ptr(),
                                       Iy.data_ptr(), ncomps, lnx.ctypes.data, w.ctypes.data, ref, PB_MIN, 1e-5, 100,
                                       maps.data_ptr(), notconv.data_ptr(), _dev.stream()))
        run_fit()
        torch.cuda.synchronize()
        tm = [event_ms(run_mask) for _ in range(args.runs)]
        tf = [event_ms(run_fit) for _ in range(args.runs)]
        case = {'fraction': frac, 'ncomps': ncomps, 'not_converged': int(notconv.item()),
                'mask_ms': dict(stats(tm), TBps_median=nbytes / float(np.median(tm)) / 1e9),
                'fit_ms': dict(stats(tf), Mcomps_per_s_median=ncomps / float(np.median(tf)) / 1e3)}
        del maps, Ix, Iy, work
        wall = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = spi.fit_spi(image, beam, freqs, weights, THRESHOLD, 1, PB_MIN, 0.0, ref_freq, io.StringIO())
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
        case['device_fit_spi_s'] = wall
        print(json.dumps(case), flush=True)

        t0 = time.perf_counter()
        himage, hbeam = image.cpu().numpy(), beam.cpu().numpy()
        t_copy = time.perf_counter() - t0
        t0 = time.perf_counter()
        cut = np.where(hbeam > PB_MIN, himage, 0)
        idx = np.argwhere(np.amin(cut, axis=0) > THRESHOLD)
        t_mask = time.perf_counter() - t0
        assert len(idx) == ncomps
        nfit = min(ncomps, args.host_comps)
        t0 = time.perf_counter()
        ix, iy = idx[:nfit, 0], idx[:nfit, 1]
        fit = sc.fit_components(cut[:, ix, iy].T.astype(np.float64), weights, freqs, ref_freq,
                                beam=hbeam[:, ix, iy].T.astype(np.float64))
        t_fit = time.perf_counter() - t0
        gmaps = np.stack([m.cpu().numpy()[ix, iy] for m in got])
        ok = np.isfinite(fit)
        dev_err = float(np.max(np.abs(gmaps[ok] - fit[ok]) / (1e-5 + 6e-8 * np.abs(fit[ok]))))
        case['host_path_s'] = {'copy': t_copy, 'cut_amin_argwhere': t_mask, 'fit_of': nfit, 'fit': t_fit,
                               'fit_scaled_to_all': t_fit * ncomps / max(nfit, 1),
                               'total': t_copy + t_mask + t_fit * ncomps / max(nfit, 1)}
        case['max_err_over_tol_plus_fp32_rounding'] = dev_err
        res['cases'].append(case)
        del image, beam, himage, hbeam, cut, got
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
