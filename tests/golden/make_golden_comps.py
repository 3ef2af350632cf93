#!/usr/bin/env python
"""
Golden vectors for the component model: runs the REFERENCE's own pfb/utils/misc.py (fit_image_cube,
eval_coeffs_to_cube, eval_coeffs_to_slice, lines 1084-1313) under the stub third-party modules of _refstubs.py and
stores inputs + reference outputs next to this file.

Run in the BUILD container only:   python tests/golden/make_golden_comps.py
(the reference tree is absent on the GPU box; the tests only read the .npz files.)

Files: comps_fit.npz (signatures, fit and edge cases), comps_eval.npz, comps_slice.npz, each below 1 MiB, written
with fixed zip timestamps: two runs give identical bytes.

Inputs.  Every image is rounded to and stored as float32 and the reference is run on its float64 upcast; the fp64
and the fp32 GPU runs both start from that one input and are compared with that one fp64 reference output.

Conditioning.  The reference solves the normal equations, so parity is only defined where that solve is stable.  Per
fit case `spread` is stored: the largest change of the reference's own coeffs, relative to max|coeffs|, when the image
is multiplied by 1 + 2.2e-16 randn (seeds 1, 2, 3).  Every stored case must have spread <= SPREAD_CAP; a case above
the cap is dropped, never the cap raised.  (Full-order 'poly' at 8 and 16 bands sits at 1e-7 .. 1e-6: not stored.)

`eval_scale` = max over planes and components of sum_p |E_p c_p|, the magnitude the rounding of an nparam-term
evaluation is relative to; E_p c_p is the reference's own evaluation with every other coefficient set to zero.

Seed: numpy.random.default_rng(420), the reference's own test seed.
"""
import inspect
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import _refstubs  # noqa: E402

_refstubs.install(ROOT)

import pfb.utils.misc as refmisc  # noqa: E402

SPREAD_CAP = 1e-11
MAX_BYTES = 1 << 20

# (ntime, nband, nx, ny, nbasist, nbasisf, method, weighted, sigmasq)
FIT_CASES = [
    (1, 4, 37, 29, None, 4, 'Legendre', True, 0),
    (1, 4, 37, 29, 1, 2, 'Legendre', True, 0),
    (1, 8, 64, 48, 1, 8, 'Legendre', False, 0),
    (1, 16, 33, 31, 1, 16, 'Legendre', True, 0),
    (1, 16, 33, 31, 1, 5, 'Legendre', False, 0),
    (1, 2, 37, 29, 1, 2, 'poly', False, 0),
    (1, 4, 37, 29, 1, 4, 'poly', True, 0),
    (1, 8, 37, 29, 1, 4, 'poly', True, 0),
    (3, 4, 20, 18, 2, 3, 'poly', False, 0),
    (3, 4, 20, 18, 2, 3, 'Legendre', False, 0),
    (1, 8, 9, 7, 1, 8, 'poly', False, 1e-6),
]
EVAL_OF = [0, 2, 7, 9]                # fit cases whose coefficients are rendered
# (nxo, nyo, cell ratio, (shift x, shift y) in input cells)
SLICE_CASES = [(40, 36, 1.0, (0, 0)), (30, 30, 1.0, (5, -3)), (80, 72, 1.0, (5, -3)), (64, 50, 0.7, (1.3, 0.4)),
               (25, 31, 1.9, (0, 0))]
SLICE_FITS = [(40, 36), (41, 35)]
CELL = 1.3e-3


def save(name, out):
    """np.savez_compressed with fixed member timestamps (bit-identical from run to run)."""
    path = os.path.join(HERE, name)
    with zipfile.ZipFile(path, 'w', compression=zipfile.ZIP_DEFLATED) as z:
        for key in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    size = os.path.getsize(path)
    assert size < MAX_BYTES, (name, size)
    print(f'{name}: {len(out)} arrays, {size} bytes')


def f32(a):
    return a.astype(np.float32)


def axes(ntime, nband):
    time = 3600.0 * (1 + np.arange(ntime))
    freq = np.linspace(0.856e9, 1.712e9, nband)
    return time, freq


def sparse_cube(rng, ntime, nband, nx, ny, frac=0.1):
    img = np.zeros((ntime, nband, nx, ny))
    on = rng.random((nx, ny)) < frac
    img[:, :, on] = rng.standard_normal((ntime, nband, int(on.sum())))
    return f32(img)


def fit(time, freq, img32, wgt, nbt, nbf, method, sigmasq, jitter=None):
    img = img32.astype(np.float64)
    if jitter is not None:
        img = img * (1.0 + 2.2e-16 * jitter.standard_normal(img.shape))
    return refmisc.fit_image_cube(time, freq, img, wgt, nbt, nbf, method, sigmasq)


def spread_of(ref, *args):
    worst = 0.0
    good = np.isfinite(ref)
    if not good.any():
        return worst
    for seed in (1, 2, 3):
        got = fit(*args, jitter=np.random.default_rng(seed))[0]
        worst = max(worst, np.abs(got - ref)[good].max() / np.abs(ref[good]).max())
    return worst


def eval_scale(time, freq, nx, ny, res):
    coeffs = res[0]
    tot = 0.0
    for p in range(coeffs.shape[0]):
        one = np.zeros_like(coeffs)
        one[p] = coeffs[p]
        tot = tot + np.abs(refmisc.eval_coeffs_to_cube(time, freq, nx, ny, one, *res[1:]))
    return np.nanmax(tot)


def put_fit(out, tag, time, freq, img32, wgt, nbt, nbf, method, sigmasq):
    args = (time, freq, img32, wgt, nbt, nbf, method, sigmasq)
    res = fit(*args)
    sp = spread_of(res[0], *args)
    print(f'  {tag} {img32.shape} nbasis=({nbt},{nbf}) {method} wgt={wgt is not None} sigmasq={sigmasq}: '
          f'ncomps {res[1].size} spread {sp:.2e}')
    assert sp <= SPREAD_CAP, (tag, sp)
    out[tag + '_time'], out[tag + '_freq'], out[tag + '_image'] = time, freq, img32
    if wgt is not None:
        out[tag + '_wgt'] = wgt
    out[tag + '_nbasis'] = np.array([-1 if nbt is None else nbt, -1 if nbf is None else nbf])
    out[tag + '_method'], out[tag + '_sigmasq'] = np.array(method), np.array(float(sigmasq))
    out[tag + '_coeffs'], out[tag + '_Ix'], out[tag + '_Iy'] = res[0], res[1], res[2]
    out[tag + '_strings'] = np.array([res[3], res[5], res[6]])
    out[tag + '_params'] = np.array(res[4])
    out[tag + '_spread'] = np.array(sp)
    nx, ny = img32.shape[2:]
    out[tag + '_eval_scale'] = np.array(eval_scale(time, freq, nx, ny, res)) if res[1].size else np.array(0.0)
    return res


def gen_fit(rng):
    out = {}
    for name, fn in [('fit_image_cube', refmisc.fit_image_cube), ('eval_coeffs_to_cube', refmisc.eval_coeffs_to_cube),
                     ('eval_coeffs_to_slice', refmisc.eval_coeffs_to_slice)]:
        out['sig_' + name] = np.array(list(inspect.signature(fn).parameters))
    fits = []
    for c, (ntime, nband, nx, ny, nbt, nbf, method, weighted, sigmasq) in enumerate(FIT_CASES):
        time, freq = axes(ntime, nband)
        img32 = sparse_cube(rng, ntime, nband, nx, ny)
        wgt = 0.5 + rng.random((ntime, nband)) if weighted else None
        fits.append((time, freq, nx, ny, put_fit(out, f'fit{c}', time, freq, img32, wgt, nbt, nbf, method, sigmasq)))
    out['nfit'] = np.array(len(FIT_CASES))

    # edge cases on 9 x 7 with 4 bands, Legendre, full order
    time, freq = axes(1, 4)
    zero = np.zeros((1, 4, 9, 7), dtype=np.float32)
    full = f32(1.0 + rng.random((1, 4, 9, 7)))
    mixed = zero.copy()
    mixed[0, :, 0, 0] = f32(rng.standard_normal(4))
    mixed[0, :, 2, 3] = -0.0
    mixed[0, :, 4, 4] = f32(rng.standard_normal(4))
    mixed[0, 1, 4, 4] = np.nan
    mixed[0, 3, 8, 6] = 0.75
    for tag, img32 in [('edge_zero', zero), ('edge_full', full), ('edge_mixed', mixed)]:
        res = put_fit(out, tag, time, freq, img32, None, None, None, 'Legendre', 0)
    assert res[1].tolist() == [0, 4, 8] and res[2].tolist() == [0, 4, 6]
    assert np.isnan(res[0][:, 1]).all() and np.isfinite(res[0][:, [0, 2]]).all()
    assert out['edge_zero_coeffs'].shape == (4, 0) and out['edge_full_Ix'].size == 63
    save('comps_fit.npz', out)
    return fits


def gen_eval(fits):
    out = {'eval_of': np.array(EVAL_OF)}
    for c in EVAL_OF:
        time, freq, nx, ny, res = fits[c]
        other = np.array([0.9e9, 1.2345e9, 1.6e9])
        for tag, fr in (('fitted', freq), ('other', other)):
            out[f'eval{c}_{tag}_freq'] = fr
            out[f'eval{c}_{tag}'] = refmisc.eval_coeffs_to_cube(time, fr, nx, ny, *res)
            out[f'eval{c}_{tag}_scale'] = np.array(eval_scale(time, fr, nx, ny, res))
    save('comps_eval.npz', out)


def gen_slice(rng):
    out = {'cases': np.array([(nxo, nyo, r, sx, sy) for (nxo, nyo, r, (sx, sy)) in SLICE_CASES]),
           'fits': np.array(SLICE_FITS), 'cell': np.array(CELL)}
    time, freq = axes(1, 4)
    for s, (nxi, nyi) in enumerate(SLICE_FITS):
        img32 = sparse_cube(rng, 1, 4, nxi, nyi)
        res = put_fit(out, f'sfit{s}', time, freq, img32, None, 1, 4, 'Legendre', 0)
        band = 1 + s
        out[f'sfit{s}_band'] = np.array(band)
        for k, (nxo, nyo, ratio, (sx, sy)) in enumerate(SLICE_CASES):
            got = refmisc.eval_coeffs_to_slice(time[0], freq[band], *res, nxi, nyi, CELL, CELL, 0.0, 0.0,
                                               nxo, nyo, ratio * CELL, ratio * CELL, sx * CELL, sy * CELL)
            assert got.shape == (nxo, nyo) and got.dtype == np.float64
            out[f'slice{s}_{k}'] = got
        out[f'sfit{s}_slice_scale'] = np.array(eval_scale(time, freq[band:band + 1], nxi, nyi, res))
    save('comps_slice.npz', out)


if __name__ == '__main__':
    rng = np.random.default_rng(420)
    gen_eval(gen_fit(rng))
    gen_slice(rng)
