#!/usr/bin/env python
"""
Times the major-cycle statistics and the mop mask on one MI355X against the routes that exist without them.

Inputs are built on the device from a seed: an (nband, N, N) residual of 0.3 + randn and a model of the same shape whose
support has density 0.1 (every component in one band).

Reports
  residual_stats   pfb_bandsum_stats with a model (band sum written, moments over the quiet pixels, max |sum|; the two
                   launches, no record read) beside the plain torch statements on the same tensors,
                       mfs = residual.sum(0); m = (model != 0).any(0); rms = mfs[~m].std(unbiased=False); rmax = mfs.abs().max()
                   which do not touch the code under test.  The two alternate for --runs warm runs, and that is repeated
                   --repeats times: per repeat the median of the device-event times, over the repeats their range (the
                   run-to-run spread that a difference has to exceed).  GB/s counts the bytes the fused pass has to
                   move: the residual and the model read once, one plane written.  The torch route's rms needs the
                   gather mfs[~m], whose size the host must learn: its time includes that synchronisation.
                   Shapes: 8 x 4096^2 float32 and 2 x 8192^2 float64.
  mop_mask         cycle.mop_mask(model, dirosion) on the device cube, wall time with a synchronise, beside today's
                   route on this machine's host CPU: .cpu().numpy(), np.any(axis=0), scipy.ndimage binary_dilation and
                   binary_erosion, and the mask copied back to the device.  The two results are compared.
and prints one JSON line; the exit status is non-zero when the fused pass is slower than the torch sequence by more than
the spread at either shape.

    python tools/time_cycle.py [--runs 20] [--repeats 5] [--dirosion 1] [--no-mop] [--json FILE]
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
from pfb_clean_amd.utils import cycle  # noqa: E402

SHAPES = [(8, 4096, torch.float32), (2, 8192, torch.float64)]


def cubes(nband, n, dtype, dev):
    gen = torch.Generator(device=dev)
    gen.manual_seed(420)
    residual = torch.randn((nband, n, n), dtype=dtype, device=dev, generator=gen) + 0.3
    model = torch.zeros((nband, n, n), dtype=dtype, device=dev)
    on = torch.rand((n, n), device=dev, generator=gen) < 0.1
    band = torch.randint(0, nband, (n, n), device=dev, generator=gen)
    for b in range(nband):
        model[b][on & (band == b)] = 1.5
    torch.cuda.synchronize()
    return residual, model


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def torch_stats(residual, model):
    mfs = residual.sum(0)
    m = (model != 0).any(0)
    rms = mfs[~m].std(unbiased=False)
    rmax = mfs.abs().max()
    return mfs, rms, rmax


def time_stats(nband, n, dtype, dev, runs, repeats):
    residual, model = cubes(nband, n, dtype, dev)
    lib = _lib.load()
    npix, code, esize = n * n, _dev.code(dtype), residual.element_size()
    work = torch.empty(lib.pfb_cycle_work_bytes(1) // 8, dtype=torch.float64, device=dev)
    out = torch.empty(cycle.RECORD, dtype=torch.float64, device=dev)
    mfs = torch.empty((n, n), dtype=dtype, device=dev)

    def fused():
        _lib.check(lib.pfb_bandsum_stats(code, residual.data_ptr(), nband, 1, npix, model.data_ptr(), nband,
                                         mfs.data_ptr(), work.data_ptr(), out.data_ptr(), _dev.stream()))

    def plain():
        torch_stats(residual, model)

    for _ in range(3):
        fused()
        plain()
    torch.cuda.synchronize()
    # the two routes agree before they are timed
    tm, trms, trmax = torch_stats(residual, model)
    count, _, m2, amax = out.tolist()
    rms = float(np.sqrt(m2 / count))
    tol = 1e-5 if dtype == torch.float32 else 1e-13          # torch's own band order is not numpy's
    assert torch.allclose(tm, mfs, rtol=tol, atol=tol) and abs(amax - trmax.item()) <= tol * amax, 'differs from torch'
    assert abs(rms - trms.item()) <= (1e-4 if dtype == torch.float32 else 1e-10) * rms, (rms, trms.item())
    nbytes = (2 * nband + 1) * npix * esize
    med = {'fused': [], 'torch': []}
    for _ in range(repeats):
        tf, tt = [], []
        for _ in range(runs):
            tf.append(event_ms(fused))
            tt.append(event_ms(plain))
        med['fused'].append(float(np.median(tf)))
        med['torch'].append(float(np.median(tt)))
    res = {'shape': [nband, n, n], 'dtype': str(dtype).split('.')[1], 'bytes_fused': nbytes, 'rms': rms, 'rmax': amax}
    for name, t in med.items():
        t = np.array(t)
        res[name + '_ms'] = {'medians': t.tolist(), 'median': float(np.median(t)), 'min': float(t.min()),
                             'max': float(t.max()), 'range': float(t.max() - t.min())}
    res['fused_GBps'] = nbytes / res['fused_ms']['median'] / 1e6
    res['fused_not_slower_beyond_spread'] = bool(
        res['fused_ms']['median'] <= res['torch_ms']['median'] + max(res['fused_ms']['range'], res['torch_ms']['range']))
    del residual, mfs
    return res, model


def time_mop(model, dirosion, repeats):
    dev_s, host = [], {'copy_out': [], 'any': [], 'closing': [], 'copy_in': []}
    struct = scipy.ndimage.generate_binary_structure(2, dirosion)
    cycle.mop_mask(model, dirosion)                          # warm-up: the code object is loaded outside the timed calls
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mask = cycle.mop_mask(model, dirosion)
        torch.cuda.synchronize()
        dev_s.append(time.perf_counter() - t0)
    for _ in range(min(repeats, 3)):
        t0 = time.perf_counter()
        m = model.cpu().numpy()
        t1 = time.perf_counter()
        sup = np.any(m, axis=0)
        t2 = time.perf_counter()
        closed = scipy.ndimage.binary_erosion(scipy.ndimage.binary_dilation(sup, structure=struct), structure=struct)
        t3 = time.perf_counter()
        back = torch.from_numpy(closed).to(model.device)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        for key, dt in zip(host, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            host[key].append(dt)
    assert torch.equal(back, mask), 'device and scipy masks differ'
    res = {'shape': list(model.shape), 'dirosion': dirosion, 'pixels_in_mask': int(mask.sum().item()),
           'device_s': {'all': dev_s, 'median': float(np.median(dev_s)), 'min': min(dev_s), 'max': max(dev_s)},
           'host_s': {k: float(np.median(v)) for k, v in host.items()}}
    res['host_s']['total'] = float(sum(res['host_s'].values()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--dirosion', type=int, default=1)
    ap.add_argument('--no-mop', action='store_true', help='time the statistics pass only')
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    dev = _dev.require_device()
    res = {'stats': [], 'mop_mask': []}
    for nband, n, dtype in SHAPES:
        r, model = time_stats(nband, n, dtype, dev, args.runs, args.repeats)
        res['stats'].append(r)
        print(json.dumps(r), flush=True)
        if not args.no_mop:
            m = time_mop(model, args.dirosion, args.repeats)
            res['mop_mask'].append(m)
            print(json.dumps(m), flush=True)
        del model
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(res, f, indent=1)
    slower = [r['shape'] for r in res['stats'] if not r['fused_not_slower_beyond_spread']]
    if slower:
        sys.exit(f'fused pass slower than the torch sequence beyond the spread at {slower}')


if __name__ == '__main__':
    main()
