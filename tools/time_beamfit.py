#!/usr/bin/env python
"""
Times the clean-beam fit on one MI355X against the route that exists without it.

Input: an (nband, N, N) fp32 PSF-like cube built on the device (a Gaussian main lobe that differs from band to band,
8 % of a decaying ripple, 1e-3 of noise).

Reports
  max pass   pfb_beamfit_max beside pfb_any_nonzero, the parent commit's read-only pass over the same bytes: the two
             alternate for --runs warm runs, median / min / max of the device-event times and TB/s of the cube
  device     wall time of fitcleanbeam on the device cube (max pass, lobe pass, record read, L-BFGS-B per band)
  host       what a caller does today, on this machine's CPU: .cpu().numpy(), then per band max + any, the threshold
             and scipy.ndimage.label with a full 3 x 3 structure; its extents are checked against the device record
and prints one JSON line.

    python tools/time_beamfit.py [--n 8192] [--nband 8] [--runs 30] [--json FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.ndimage
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pfb_clean_amd import _dev, _lib  # noqa: E402
from pfb_clean_amd.utils import beamfit  # noqa: E402


def psf_cube(nband, n, dev):
    torch.manual_seed(420)
    ax = torch.arange(-n / 2, n / 2, device=dev, dtype=torch.float32)
    cube = torch.empty((nband, n, n), dtype=torch.float32, device=dev)
    k = 2 * np.sqrt(2 * np.log(2))
    for b in range(nband):
        emaj, emin, t = 14.0 + b, 7.0 + 0.5 * b, np.deg2rad(-(20.0 + 5 * b))
        u = np.cos(t) * ax[:, None] - np.sin(t) * ax[None, :]
        v = np.sin(t) * ax[:, None] + np.cos(t) * ax[None, :]
        r = torch.sqrt(ax[:, None] ** 2 + ax[None, :] ** 2)
        cube[b] = 0.92 * torch.exp(-k * (u * u / emin ** 2 + v * v / emaj ** 2)) \
            + 0.08 * torch.cos(0.9 * r / emin) * torch.exp(-r / (4 * emaj))
        cube[b] += 1e-3 * torch.randn((n, n), device=dev)
        del u, v, r
    torch.cuda.synchronize()
    return cube


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=8192)
    ap.add_argument('--nband', type=int, default=8)
    ap.add_argument('--runs', type=int, default=30)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    nband, n = args.nband, args.n
    dev = _dev.require_device()
    cube = psf_cube(nband, n, dev)
    lib = _lib.load()
    npix, code, nbytes = n * n, _dev.code(cube.dtype), cube.numel() * 4
    work = torch.empty(lib.pfb_beamfit_work_bytes(nband, npix) // 8, dtype=torch.float64, device=dev)
    ws, out = _dev.scratch()

    def run_max():
        _lib.check(lib.pfb_beamfit_max(code, cube.data_ptr(), nband, npix, work.data_ptr(), _dev.stream()))

    def run_any():
        _lib.check(lib.pfb_any_nonzero(code, cube.data_ptr(), cube.numel(), out.data_ptr(), ws.data_ptr(),
                                       _dev.stream()))

    for _ in range(3):
        run_max()
        run_any()
    torch.cuda.synchronize()
    tm, ta = [], []
    for _ in range(args.runs):
        tm.append(event_ms(run_max))
        ta.append(event_ms(run_any))
    res = {'shape': [nband, n, n], 'bytes': nbytes}
    for name, t in (('beamfit_max_ms', tm), ('any_nonzero_ms', ta)):
        t = np.array(t)
        res[name] = {'median': float(np.median(t)), 'min': float(t.min()), 'max': float(t.max()),
                     'TBps_median': nbytes / float(np.median(t)) / 1e9}
    rec = work[:nband * beamfit.RECORD].cpu().numpy().reshape(nband, beamfit.RECORD)
    assert np.array_equal(rec[:, 0], cube.amax(dim=(1, 2)).cpu().numpy().astype(np.float64)) and (rec[:, 1] == 1).all()
    print(json.dumps({k: res[k] for k in ('beamfit_max_ms', 'any_nonzero_ms')}), flush=True)

    fits = []
    for _ in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = beamfit.fitcleanbeam(cube)
        torch.cuda.synchronize()
        fits.append(time.perf_counter() - t0)
    recs, _ = beamfit.lobe_records(cube)
    res['fitcleanbeam_s'], res['fitcleanbeam_result'] = fits, np.array(got).tolist()
    res['records'] = recs[:, :len(beamfit.FIELDS)].tolist()
    print(json.dumps({'fitcleanbeam_s': fits, 'result': res['fitcleanbeam_result']}), flush=True)

    t0 = time.perf_counter()
    host = cube.cpu().numpy()
    t_copy = time.perf_counter() - t0
    t_max = t_thr = t_lab = 0.0
    ext = []
    for b in range(nband):
        t0 = time.perf_counter()
        mx, nz = host[b].max(), host[b].any()
        t1 = time.perf_counter()
        mask = np.where(host[b] / mx > 0.5, 1.0, 0)
        t2 = time.perf_counter()
        lab = scipy.ndimage.label(mask, structure=np.ones((3, 3)))[0]
        t3 = time.perf_counter()
        t_max, t_thr, t_lab = t_max + t1 - t0, t_thr + t2 - t1, t_lab + t3 - t2
        ii, jj = np.nonzero(lab == lab[n // 2, n // 2])
        ext.append([ii.min() - n / 2, ii.max() - n / 2, jj.min() - n / 2, jj.max() - n / 2])
    assert np.array_equal(np.array(ext, dtype=np.float64), recs[:, 3:7]), (ext, recs[:, 3:7])
    res['host_path_s'] = {'copy': t_copy, 'max_any': t_max, 'threshold': t_thr, 'label': t_lab,
                          'total': t_copy + t_max + t_thr + t_lab}
    print(json.dumps(res))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
