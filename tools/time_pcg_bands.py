"""
Batched per-band PCG (pcg_fused_bands / pfb_pcg_solve_bands) against the band-by-band loop of pfb_pcg_solve it replaces
in pcg_psf, on seeded inputs; the two alternate within one run.  At 8 x 4096^2 the cube solve (pfb_pcg_solve over all
bands as one system) is timed as well, for the per-iteration cost of the same convolution launch group.

    python tools/time_pcg_bands.py [--reps 3] [--shapes 8x1024x1024:f32,8x4096x4096:f32,2x8192x8192:f64] [--out FILE]

One JSON line per (shape, setting): milliseconds per solve (median of --reps), per band-iteration and per iteration of
the batched launch group, iterations per band, and whether the two give the same iteration counts.  Up to 16 M elements
the batched solve is also timed with PFB_PCG_LOOKAHEAD=0 (no iteration run ahead of the host's look).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from pfb_clean_amd.operators.hessian import HessianPsf  # noqa: E402
from pfb_clean_amd.opt import pcg as P  # noqa: E402

SETTINGS = {'fixed50': dict(tol=0.0, maxit=50, minit=50), 'klean': dict(tol=1e-2, maxit=100, minit=1)}


def problem(nb, nx, ny, rdt, seed=2024):
    """A Gaussian PSF per band (slightly different widths), b = A(point sources) + noise."""
    dev = torch.device('cuda')
    g = torch.Generator(device=dev).manual_seed(seed)
    P_, Q = 2 * nx, 2 * ny
    u = torch.fft.fftfreq(P_, device=dev, dtype=torch.float64)[:, None]
    v = torch.fft.rfftfreq(Q, device=dev, dtype=torch.float64)[None, :]
    ctype = torch.complex64 if rdt == torch.float32 else torch.complex128
    psfhat = torch.stack([torch.exp(-(u ** 2 + v ** 2) / (2 * (0.08 + 0.01 * k) ** 2)) for k in range(nb)]).to(ctype)
    model = torch.zeros((nb, nx, ny), dtype=rdt, device=dev)
    idx = torch.randint(0, nx * ny, (nb, 64), generator=g, device=dev)
    model.view(nb, -1).scatter_(1, idx, torch.rand((nb, 64), generator=g, device=dev, dtype=rdt) + 0.5)
    sigmainv = 1e-3
    A = HessianPsf(psfhat, nx, ny, Q, sigmainv=sigmainv)
    b = A(model) + 1e-3 * torch.randn((nb, nx, ny), generator=g, device=dev, dtype=rdt)
    return A, b, sigmainv


def loop(A, b, sig, kw):
    iters = []
    for k in range(b.shape[0]):
        Ab = HessianPsf(A.plan, A.nx, A.ny, 0, sigmainv=sig, band0=k, nb=1)
        _, _, res = P.pcg_fused(Ab, b[k:k + 1], None, mdiv=sig, **kw)
        iters.append(res.iters)
    return iters


def batched(A, b, sig, kw):
    _, _, res = P.pcg_fused_bands(A, b, None, mdiv=sig, **kw)
    return [r.iters for r in res]


def batched_no_lookahead(A, b, sig, kw):
    os.environ['PFB_PCG_LOOKAHEAD'] = '0'
    try:
        return batched(A, b, sig, kw)
    finally:
        del os.environ['PFB_PCG_LOOKAHEAD']


def cube(A, b, sig, kw):
    _, _, res = P.pcg_fused(A, b, None, mdiv=sig, **kw)
    return [res.iters]


def timed(fn, *a):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(*a)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--shapes', default='8x1024x1024:f32,8x4096x4096:f32,2x8192x8192:f64,2x8192x8192:f32,'
                                        '2x6000x6000:f32')
    ap.add_argument('--settings', default='fixed50,klean')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = []
    for spec in args.shapes.split(','):
        dims, dt = spec.split(':')
        nb, nx, ny = (int(s) for s in dims.split('x'))
        rdt = torch.float32 if dt == 'f32' else torch.float64
        A, b, sig = problem(nb, nx, ny, rdt)
        for name in args.settings.split(','):
            kw = dict(SETTINGS[name], backtrack=True)
            legs = [('loop', loop), ('batched', batched)]
            if (nb, nx, ny, dt) == (8, 4096, 4096, 'f32'):
                legs.append(('cube', cube))
            if nb * nx * ny <= (16 << 20):       # where the batched solve runs one iteration ahead of its looks
                legs.append(('batched_no_lookahead', batched_no_lookahead))
            for _, fn in legs:                   # warm-up: plans, work buffers, code objects
                fn(A, b, sig, dict(kw, maxit=2, minit=2))
            ms = {k: [] for k, _ in legs}
            its = {}
            for _ in range(args.reps):
                for k, fn in legs:               # alternate
                    t, it = timed(fn, A, b, sig, kw)
                    ms[k].append(t)
                    its[k] = it
            med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
            row = dict(shape=spec, setting=name, ms=med, ms_all=ms, iters=its,
                       ms_per_launch_iter={k: med[k] / max(max(its[k]), 1) for k in med if k != 'loop'},
                       ms_per_band_iter={k: med[k] / max(sum(its[k]) if k != 'cube' else its[k][0] * nb, 1)
                                         for k in med},
                       speedup=med['loop'] / med['batched'], same_iters=its['loop'] == its['batched'])
            if 'cube' in med:
                row['batched_vs_cube_per_iter'] = row['ms_per_band_iter']['batched'] / row['ms_per_band_iter']['cube']
            print(json.dumps(row), flush=True)
            lines.append(row)
        del A, b
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, 'w') as f:
            for row in lines:
                f.write(json.dumps(row) + '\n')


if __name__ == '__main__':
    main()
