#!/usr/bin/env python
"""
Times the component-model fit on one MI355X against the route that exists without it.

Input: the benchmark's model (bench.synth_model: 25 Gaussians + 10 point pixels per band), N x N x nband, fp32,
device resident; Legendre basis with nbasisf = nband.

Reports the median over --runs warm runs of
  device   fit_image_cube on the device tensor (one read of the component count is its only synchronisation),
           and its stages on their own: mask (+ scan), compact, fit
  mask     as GB/s of the cube, beside the read rate tools/micro/hbm_stream reaches on the same box (run here when
           the binary has been built, or given with --stream-tbs)
  host     a device-to-host copy of the cube followed by the numpy statement of the fit
           (np.any / np.where / gather / normal equations / np.linalg.solve)
and prints one JSON line.  --shape NX NY takes the place of --n for a plane that is not square (4097 x 4095: odd npix,
the form of the mask pass for planes off the 16-byte grid); --mask-only times the mask pass alone (median, min and max
of --runs device-event times), which is what an A/B of two builds of the library (PFB_HIP_LIB) needs.

    python tools/time_comps.py [--n 4096 | --shape NX NY] [--nband 8] [--runs 20] [--host-runs 20] [--mask-only]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import synth_model  # noqa: E402
from pfb_clean_amd import _dev, _lib  # noqa: E402
from pfb_clean_amd.utils import comps  # noqa: E402


def median_ms(fn, runs, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(out)


def event_times(fn, runs, warm=3):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def event_ms(fn, runs, warm=3):
    return statistics.median(event_times(fn, runs, warm))


def stream_rate():
    exe = os.path.join(ROOT, 'tools', 'micro', 'hbm_stream')
    if not os.path.exists(exe):
        return None
    txt = subprocess.run([exe], capture_output=True, text=True, timeout=300).stdout
    m = re.search(r'^read\s+1R\+0W: best ([0-9.]+) TB/s', txt, re.M)
    return float(m.group(1)) if m else None


def host_fit(time_, freq, image, Xfit):
    mask = np.any(image, axis=(0, 1))
    Ix, Iy = np.where(mask)
    beta = image[:, :, Ix, Iy].reshape(Xfit.shape[0], Ix.size)
    return np.linalg.solve(Xfit.T.dot(Xfit), Xfit.T.dot(beta)), Ix, Iy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--shape', type=int, nargs=2, default=None, metavar=('NX', 'NY'))
    ap.add_argument('--mask-only', action='store_true')
    ap.add_argument('--nband', type=int, default=8)
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--host-runs', type=int, default=20)
    ap.add_argument('--stream-tbs', type=float, default=None)
    a = ap.parse_args()

    dev = _dev.require_device()
    lib = _lib.load()
    nband = a.nband
    nx, ny = a.shape or (a.n, a.n)
    cube = torch.stack([synth_model(b, nx, ny, torch.float32, dev) for b in range(nband)])[None].contiguous()
    time_, freq = np.array([3600.0]), 1e9 * (1.0 + 0.1 * np.arange(nband))
    nbytes = cube.numel() * cube.element_size()

    npix = nx * ny
    flat = cube.view(nband, npix)
    work = torch.empty(lib.pfb_comps_work_bytes(npix) // 8, dtype=torch.int64, device=dev)
    st = _dev.stream()

    def run_mask():
        _lib.check(lib.pfb_comps_mask(_lib.PFB_F32, _dev.ptr(flat), nband, npix, _dev.ptr(work), st))
    if a.mask_only:
        t = event_times(run_mask, a.runs)
        med = statistics.median(t)
        print(json.dumps({'shape': [nband, nx, ny], 'dtype': 'float32', 'lib': _lib.LIB_PATH, 'cube_MB': nbytes / 1e6,
                          'ncomps': int(work[-1].item()), 'runs': a.runs,
                          'mask_ms': {'median': med, 'min': min(t), 'max': max(t), 'TBps_median': nbytes / med / 1e9}}))
        return

    res = comps.fit_image_cube(time_, freq, cube, nbasisf=nband, method='Legendre')
    ncomps = res[1].numel()
    t_fit = median_ms(lambda: comps.fit_image_cube(time_, freq, cube, nbasisf=nband, method='Legendre'), a.runs)

    # the stages on their own
    Ix, Iy = torch.empty_like(res[1]), torch.empty_like(res[2])
    coeffs = torch.empty_like(res[0])
    Xfit = comps.fit_design(time_, freq, None, nband, 'Legendre')[0]
    sysd = torch.from_numpy(comps._fit_system(Xfit, None, 0)).to(dev)
    t_mask = event_ms(run_mask, a.runs)
    t_compact = event_ms(lambda: _lib.check(lib.pfb_comps_compact(npix, ny, _dev.ptr(work), _dev.ptr(Ix), _dev.ptr(Iy),
                                                                  st)), a.runs)
    t_solve = event_ms(lambda: _lib.check(lib.pfb_comps_fit(_lib.PFB_F32, _dev.ptr(flat), nband, npix, ny, _dev.ptr(Ix),
                                                            _dev.ptr(Iy), ncomps, _dev.ptr(sysd), nband,
                                                            _dev.ptr(coeffs), st)), a.runs)
    assert torch.equal(Ix, res[1]) and torch.equal(Iy, res[2])

    # the route without the feature: copy the cube out, fit in numpy
    t_d2h = median_ms(lambda: cube.cpu(), max(3, a.host_runs), warm=1)
    host = cube.cpu().numpy()
    hres = host_fit(time_, freq, host, Xfit)
    assert np.array_equal(hres[1], res[1].cpu().numpy()) and np.array_equal(hres[2], res[2].cpu().numpy())
    scale = np.abs(hres[0]).max()
    err = np.abs(hres[0] - res[0].cpu().numpy()).max() / scale
    t_numpy = median_ms(lambda: host_fit(time_, freq, host, Xfit), a.host_runs, warm=1)

    tbs = a.stream_tbs if a.stream_tbs is not None else stream_rate()
    out = {'shape': [nband, nx, ny], 'nband': nband, 'dtype': 'float32', 'ncomps': ncomps, 'cube_MB': nbytes / 1e6,
           'device_fit_ms': t_fit, 'mask_ms': t_mask, 'compact_ms': t_compact, 'fit_kernel_ms': t_solve,
           'mask_GBps': nbytes / 1e6 / t_mask, 'hbm_stream_read_GBps': None if tbs is None else 1e3 * tbs,
           'host_d2h_ms': t_d2h, 'host_numpy_ms': t_numpy, 'host_route_ms': t_d2h + t_numpy,
           'speedup': (t_d2h + t_numpy) / t_fit, 'coeffs_rel_diff_vs_numpy': err, 'runs': a.runs,
           'host_runs': a.host_runs}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
