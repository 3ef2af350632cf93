#!/usr/bin/env python
"""
Golden vectors for the major-cycle statistics, the mop mask and the closing (pfb_clean_amd/utils/cycle.py): inputs and
what numpy / scipy.ndimage make of them, stored in cycle.npz next to this file.

Run in the BUILD container only:   python tests/golden/make_golden_cycle.py
(scipy.ndimage is the reference of the closing; the tests only read the .npz file.)

What the workers' loops do with these arrays, in this script's own words:
  band sum    residual_mfs = np.sum(residual, axis=0), in the cube's dtype
  statistics  rms = np.std(residual_mfs), or np.std over the pixels where np.any(model, axis=0) is False;
              rmax = np.abs(residual_mfs).max()
  mop mask    for dirosion != 0: struct = generate_binary_structure(2, dirosion), then one binary_dilation and one
              binary_erosion with it (scipy's defaults: one iteration, border_value=0); dirosion == 0 leaves the support

Two groups:
  st{k}   statistics cases, shapes STAT_SHAPES.  Stored once as float32 (`x32`, `model`); the float64 input is
          x64 = x32.astype(float64) / 3, an exactly rounded IEEE division that every machine repeats bit for bit and that
          fills the 53-bit mantissa (sums of float32 values would be exact in float64 and prove nothing about the
          order).  Outputs for both dtypes: the band sum, numpy's own std (a float32 for the float32 array) and max,
          with and without the model.
  cl{k}   closing cases: a bool mask and its closing for dirosion 0, 1, 2, 3, shapes CLOSE_SHAPES, patterns below.

Fixed zip timestamps: two runs give identical bytes.
"""
import io
import os
import zipfile

import numpy as np
import scipy.ndimage as ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_BYTES = 1 << 20

STAT_SHAPES = [(1, 1, 1), (3, 5, 7), (2, 33, 65), (8, 96, 130)]
CLOSE_SHAPES = [(1, 1), (1, 9), (9, 1), (7, 5), (64, 64), (65, 129), (130, 70)]
TILE_ROWS, TILE_COLS = 32, 64               # the closing kernel's output tile (MC_TH, MC_TW in csrc/cycle.hip)
DIROSIONS = (0, 1, 2, 3)


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


# ------------------------------------------------------------------------------------------------- statistics
def x64_of(x32):
    return x32.astype(np.float64) / 3.0


def gen_stats(out, rng):
    for k, (nband, nx, ny) in enumerate(STAT_SHAPES):
        x32 = (0.3 + rng.standard_normal((nband, nx, ny))).astype(np.float32)
        # a model of 3 bands whose support has density 0.1, every component in one band only
        on = rng.random((nx, ny)) < 0.1
        band = rng.integers(0, 3, size=(nx, ny))
        model = np.zeros((3, nx, ny), dtype=np.float32)
        for b in range(3):
            sel = on & (band == b)
            model[b][sel] = (0.5 + rng.random(int(sel.sum()))).astype(np.float32)
        assert np.array_equal(np.any(model, axis=0), on)
        out[f'st{k}_x32'], out[f'st{k}_model'] = x32, model
        for bits, x in ((32, x32), (64, x64_of(x32))):
            mfs = np.sum(x, axis=0)
            assert mfs.dtype == x.dtype
            quiet = mfs[~np.any(model, axis=0)]
            out[f'st{k}_mfs{bits}'] = mfs
            out[f'st{k}_std{bits}'] = np.std(mfs)
            out[f'st{k}_rmax{bits}'] = np.abs(mfs).max()
            out[f'st{k}_nquiet'] = np.array(quiet.size)
            with np.errstate(all='ignore'):
                out[f'st{k}_qstd{bits}'] = np.std(quiet) if quiet.size else np.array(np.nan, dtype=x.dtype)
            assert out[f'st{k}_std{bits}'].dtype == x.dtype
    out['nstat'] = np.array(len(STAT_SHAPES))


# ---------------------------------------------------------------------------------------------------- closing
def closing(mask, dirosion):
    if not dirosion:
        return mask.copy()
    struct = ndimage.generate_binary_structure(2, dirosion)
    return ndimage.binary_erosion(ndimage.binary_dilation(mask, structure=struct), structure=struct)


def patterns(nx, ny, rng):
    """[(name, mask)]: every pattern that fits the shape."""
    def pts(*ij):
        m = np.zeros((nx, ny), dtype=bool)
        for i, j in ij:
            if not (0 <= i < nx and 0 <= j < ny):
                return None
            m[i, j] = True
        return m

    ci, cj = nx // 2, ny // 2
    cand = []
    singles = {'corner00': (0, 0), 'corner01': (0, ny - 1), 'corner10': (nx - 1, 0), 'corner11': (nx - 1, ny - 1),
               'edge_top': (0, cj), 'edge_bottom': (nx - 1, cj), 'edge_left': (ci, 0), 'edge_right': (ci, ny - 1),
               'interior': (ci, cj)}
    for name, p in singles.items():
        cand.append((name, pts(p)))
    cand += [('gap1_rows', pts((ci - 1, cj), (ci + 1, cj))), ('gap2_rows', pts((ci - 1, cj), (ci + 2, cj))),
             ('gap3_rows', pts((ci - 1, cj), (ci + 3, cj))),
             ('gap1_cols', pts((ci, cj - 1), (ci, cj + 1))), ('gap2_cols', pts((ci, cj - 1), (ci, cj + 2))),
             ('gap3_cols', pts((ci, cj - 1), (ci, cj + 3))),
             ('diagonal', pts((ci, cj), (ci + 1, cj + 1))), ('antidiagonal', pts((ci, cj), (ci + 1, cj - 1))),
             ('diagonal_gap1', pts((ci - 1, cj - 1), (ci + 1, cj + 1)))]
    for d in (0.02, 0.2, 0.6):
        cand.append((f'random{d}', rng.random((nx, ny)) < d))
    # across the tile edges of the kernel: single pixels on either side, pairs whose gap IS the edge column / row, and a
    # dense patch over the tile corner
    c, r = TILE_COLS, TILE_ROWS
    cand += [('tile_cols', pts((3, c - 1), (7, c), (11, c + 1))), ('tile_cols_gap', pts((5, c - 1), (5, c + 1))),
             ('tile_cols_gap_left', pts((5, c - 2), (5, c))), ('tile_rows', pts((r - 1, 3), (r, 7), (r + 1, 11))),
             ('tile_rows_gap', pts((r - 1, 5), (r + 1, 5))), ('tile_rows_gap_up', pts((r - 2, 5), (r, 5)))]
    if nx > r + 4 and ny > c + 4:
        m = np.zeros((nx, ny), dtype=bool)
        m[r - 4:r + 4, c - 4:c + 4] = rng.random((8, 8)) < 0.5
        cand.append(('tile_corner_patch', m))
    cand += [('ones', np.ones((nx, ny), dtype=bool)), ('zeros', np.zeros((nx, ny), dtype=bool))]
    seen, res = [], []
    for name, m in cand:
        if m is None or any(np.array_equal(m, s) for s in seen):
            continue
        seen.append(m)
        res.append((name, m))
    return res


def gen_closings(out, rng):
    k = 0
    names, fills = [], {}
    for nx, ny in CLOSE_SHAPES:
        for name, mask in patterns(nx, ny, rng):
            out[f'cl{k}_mask'] = mask
            for d in DIROSIONS:
                res = closing(mask, d)
                assert res.dtype == bool and res.shape == mask.shape
                out[f'cl{k}_out{d}'] = res
                fills[(nx, ny, name, d)] = res
            names.append(f'{nx}x{ny}:{name}')
            k += 1
    out['nclose'], out['close_names'] = np.array(k), np.array(names)
    out['close_dirosions'], out['tile'] = np.array(DIROSIONS), np.array([TILE_ROWS, TILE_COLS])
    # what the cases are there to show
    f = lambda shape, name, d: fills[shape + (name, d)]
    assert not f((64, 64), 'corner00', 1).any() and not f((64, 64), 'edge_left', 2).any()       # border pixels vanish
    assert f((64, 64), 'interior', 1).sum() == 1
    # two pixels on a line: under the full 3 x 3 a gap of 1 or 2 fills (the dilated blocks touch) and a gap of 3 stays
    # open; under the cross nothing fills, the bridge pixel's own cross is not covered by the two dilated crosses
    for axis in ('rows', 'cols'):
        assert [int(f((64, 64), f'gap{g}_{axis}', 2).sum()) for g in (1, 2, 3)] == [3, 4, 2]
        assert [int(f((64, 64), f'gap{g}_{axis}', 1).sum()) for g in (1, 2, 3)] == [2, 2, 2]
    # a diagonal pair is closed under both structures (no 3 x 3 or cross around a third pixel is covered); the two
    # structures differ on the line pairs above and on the random masks; 2 and 3 are the same structure
    for d in (1, 2):
        assert np.array_equal(f((64, 64), 'diagonal', d), f((64, 64), 'diagonal', 0))
    assert not np.array_equal(f((64, 64), 'random0.2', 1), f((64, 64), 'random0.2', 2))
    assert np.array_equal(f((64, 64), 'random0.2', 2), f((64, 64), 'random0.2', 3))
    assert f((65, 129), 'tile_cols_gap', 2)[5, TILE_COLS] and f((130, 70), 'tile_rows_gap', 2)[TILE_ROWS, 5]
    ones = f((130, 70), 'ones', 2)
    assert not ones[0].any() and not ones[:, -1].any() and ones[1:-1, 1:-1].all()
    print(f'  {k} closing cases')


if __name__ == '__main__':
    out = {}
    rng = np.random.default_rng(421)
    gen_stats(out, rng)
    gen_closings(out, rng)
    save('cycle.npz', out)
