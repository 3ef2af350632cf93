#!/usr/bin/env python
"""
Golden vectors for the restoring-beam functions: runs the REFERENCE's own pfb/utils/misc.py (Gaussian2D,
get_padding_info, convolve2gaussres) and pfb/utils/restoration.py (restore_image) under the stub third-party modules
of _refstubs.py (scipy.fft standing in for ducc0) and stores inputs + reference outputs next to this file.

Run in the BUILD container only:   python tests/golden/make_golden_restore.py
(the reference tree is absent on the GPU box; the tests only read the .npz files.)

Files.  No committed file may exceed 1 MiB, so the vectors are spread over restore.npz (signatures, padding table,
Gaussian2D), restore_image.npz and one restore_conv<c>.npz per convolve2gaussres shape (together below 4 MB).  The
archives are written with fixed zip timestamps: two runs give identical bytes.

Inputs.  Every input image is rounded to and stored as float32 and the reference is run on its float64 upcast; the
fp64 and the fp32 GPU runs both start from that one input and are compared with that one fp64 reference output.

Ratio branch (gausspari given).  The reference's multiplier gausskernhat / thiskernhat is noise over noise wherever
the initial kernel's spectrum has decayed to rounding level, so parity is only defined where the reference itself is
stable.  Per case `spread` is stored: the largest relative change of the reference's own output when every input of
its KERNEL r2c calls is multiplied by 1 + 2.2e-16 randn (seeds 1, 2, 3).  Every stored case must have
spread <= SPREAD_CAP; a case above the cap is dropped, never the cap raised.

Seed: numpy.random.default_rng(420), the reference's own test seed.
"""
import importlib.util
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

_spec = importlib.util.spec_from_file_location(
    'pfb_ref_restoration', os.path.join(os.path.dirname(os.path.dirname(refmisc.__file__)), 'utils', 'restoration.py'))
refrest = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(refrest)

SPREAD_CAP = 1e-11
MAX_BYTES = 1 << 20

# (nband, nx, ny, w): model branch gaussparf = (w, 0.6 w, 33 deg); reference grids 192x120, 192x360, 375x120, 96x96,
# 135x75 -- even, odd-P and odd-Q, each with a truncated kernel wider than the padding (wrap-around)
CONV_SHAPES = [(2, 128, 80, 15.), (1, 128, 220, 15.), (1, 250, 78, 9.), (2, 64, 64, 40.), (2, 90, 50, 30.)]
SMALL = (3, 4)                       # the two smallest shapes carry the extra model cases and all four ratio cases
RATIO_ALL = [(5., 2.0), (5., 2.5), (6., 2.0), (6., 2.5)]
RATIO_FEW = [(5., 2.0), (6., 2.5)]
PAD_N = [50, 78, 80, 90, 128, 220, 250, 1500, 2048, 4096, 6000]


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
    return size


def coords(nx, ny, cell=1.0):
    x = np.arange(-nx / 2, nx / 2) * cell
    y = np.arange(-ny / 2, ny / 2) * cell
    return np.meshgrid(x, y, indexing='ij')


def f32(a):
    return a.astype(np.float32)


def ratio_pars(F, f, nband):
    return (F, 0.8 * F, 33.0), tuple((f * (1 + 0.1 * b), f * (0.8 + 0.05 * b), 10.0 * b) for b in range(nband))


def spread_of(call, ref, scale=None):
    """Largest relative change of call()'s result over three seeded 1-ulp perturbations of the inputs of the kernel
    transforms: in convolve2gaussres the 1st r2c call transforms the target kernel, the 2nd the image, every later
    one an initial kernel (misc.py:212-227)."""
    real_r2c = refmisc.r2c
    worst = 0.0
    for seed in (1, 2, 3):
        jr = np.random.default_rng(seed)
        state = {'n': 0}

        def jitter(a, **kw):
            state['n'] += 1
            if state['n'] != 2:
                a = a * (1.0 + 2.2e-16 * jr.standard_normal(a.shape))
            return real_r2c(a, **kw)

        def counted(*a, **kw):
            state['n'] = 0
            return call(*a, **kw)
        refmisc.r2c = jitter
        try:
            got = counted()
        finally:
            refmisc.r2c = real_r2c
        worst = max(worst, np.abs(got - ref).max() / (np.abs(ref).max() if scale is None else scale))
    return worst


def gen_meta_gauss():
    out = {}
    for name, fn in [('Gaussian2D', refmisc.Gaussian2D), ('get_padding_info', refmisc.get_padding_info),
                     ('convolve2gaussres', refmisc.convolve2gaussres), ('restore_image', refrest.restore_image)]:
        out['sig_' + name] = np.array(list(inspect.signature(fn).parameters))
    out['pad_n'] = np.array(PAD_N)
    out['pad_lr'] = np.array([refmisc.get_padding_info(n, n, 0.5)[0][1] for n in PAD_N])
    out['pad_conv'] = np.array([[nx, ny] + list(p[1]) + list(p[2]) for (_, nx, ny, _) in CONV_SHAPES
                                for p in [refmisc.get_padding_info(nx, ny, 0.5)[0]]])
    # Gaussian2D: rows (nx, ny, emaj, emin, pa, normalise, nsigma, cell); GaussPar is in units of the cell
    rows = []
    for (nx, ny) in [(128, 80), (90, 51)]:
        for par in [(15., 9., 33.), (5., 5., 0.), (3., 2., -70.)]:
            for norm in (1, 0):
                for nsigma in (5, 2):
                    rows.append((nx, ny) + par + (norm, nsigma, 1.0))
    rows.append((128, 80, 15., 9., 33., 1, 5, 2.5e-4))
    out['gauss_cases'] = np.array(rows)
    for c, (nx, ny, emaj, emin, pa, norm, nsigma, cell) in enumerate(rows):
        xx, yy = coords(int(nx), int(ny), cell)
        out[f'gauss{c}'] = refmisc.Gaussian2D(xx, yy, (emaj * cell, emin * cell, pa), normalise=bool(norm),
                                              nsigma=int(nsigma))
    return save('restore.npz', out)


def gen_conv(rng):
    total = 0
    for c, (nband, nx, ny, w) in enumerate(CONV_SHAPES):
        out = {}
        xx, yy = coords(nx, ny)
        img32 = f32(rng.standard_normal((nband, nx, ny)))
        img = img32.astype(np.float64)
        gpf = (w, 0.6 * w, 33.0)
        out['image'] = img32
        out['model_par'] = np.array(gpf)
        out['model'] = refmisc.convolve2gaussres(img.copy(), xx, yy, gpf, 1)
        if c in SMALL:
            out['model_norm'] = refmisc.convolve2gaussres(img.copy(), xx, yy, gpf, 1, norm_kernel=True)
            out['model_pfrac25'] = refmisc.convolve2gaussres(img.copy(), xx, yy, gpf, 1, pfrac=0.25)
            pt = np.zeros((nband, nx, ny))
            pt[:, nx // 2, ny // 2] = 1.0
            out['model_point'] = refmisc.convolve2gaussres(pt, xx, yy, gpf, 1)
        tags = []
        for (F, f) in (RATIO_ALL if c in SMALL else RATIO_FEW):
            gf, gi = ratio_pars(F, f, nband)

            def call():
                return refmisc.convolve2gaussres(img.copy(), xx, yy, gf, 1, gausspari=gi, norm_kernel=True)
            ref = call()
            sp = spread_of(call, ref)
            print(f'  conv{c} {nband}x{nx}x{ny} F={F} f={f}: spread {sp:.2e}')
            assert sp <= SPREAD_CAP, (c, F, f, sp)
            tag = f'ratio_F{F:g}_f{f:g}'
            tags.append(tag)
            out[tag] = ref
            out[tag + '_par'] = np.array([gf] + list(gi))
            out[tag + '_spread'] = np.array(sp)
        out['ratio_tags'] = np.array(tags)
        total += save(f'restore_conv{c}.npz', out)
    return total


def gen_restore(rng):
    out = {}
    nband, nx, ny = 3, 96, 96
    model = np.zeros((nband, nx, ny))
    model[:, rng.integers(10, 86, 12), rng.integers(10, 86, 12)] = 1 + rng.random(12)
    model32 = f32(model)
    resid32 = f32(1e-2 * rng.standard_normal((nband, nx, ny)))
    gpf = tuple((8. + 0.5 * b, 6. + 0.25 * b, 20. + 5. * b) for b in range(nband))
    gpi = tuple((2.0 + 0.25 * b, 2.0 + 0.15 * b, 10. * b) for b in range(nband))
    out['model'], out['residual'] = model32, resid32
    out['gaussparf'], out['gausspari'] = np.array(gpf), np.array(gpi)
    muts = []
    for conv in (True, False):
        m = model32.astype(np.float64)
        res = refrest.restore_image(m, resid32.astype(np.float64), 1.0, 1.0, gpf, gpi, conv, 1, 0.5)
        out['image_conv' if conv else 'image_noconv'] = res
        muts.append(m)
    assert np.array_equal(muts[0], muts[1])
    out['model_mutated'] = muts[0]

    # rounding sensitivity of the residual step (the only ratio in restore_image)
    x = np.arange(-(nx // 2), nx // 2 + nx % 2) * 1.0
    xx, yy = np.meshgrid(x, x)

    def call():
        return refmisc.convolve2gaussres(resid32.astype(np.float64), xx, yy, gpf[0], 1, gausspari=gpi,
                                         norm_kernel=True, pfrac=0.5)
    # relative to max|restored image|, which the test's bound refers to
    sp = spread_of(call, call(), scale=np.abs(out['image_conv']).max())
    print(f'  restore_image residual step: spread {sp:.2e}')
    assert sp <= SPREAD_CAP, sp
    out['spread'] = np.array(sp)
    return save('restore_image.npz', out)


if __name__ == '__main__':
    rng = np.random.default_rng(420)
    total = gen_meta_gauss() + gen_conv(rng) + gen_restore(rng)
    print('total bytes', total)
