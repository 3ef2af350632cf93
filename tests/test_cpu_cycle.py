"""
Major-cycle statistics, mop mask and masked problem, the part that needs no GPU: the bindings, the host-only size
function, and the golden file (tests/golden/cycle.npz, written by tests/golden/make_golden_cycle.py) recomputed without
scipy: every stored closing as an OR of shifts of the zero-padded mask followed by an AND of shifts, every stored band
sum as a sequential sum over the bands.  Both must equal the file exactly.
"""
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'cycle.npz')
STAT_SHAPES = [(1, 1, 1), (3, 5, 7), (2, 33, 65), (8, 96, 130)]
CLOSE_SHAPES = [(1, 1), (1, 9), (9, 1), (7, 5), (64, 64), (65, 129), (130, 70)]
_cache = {}


def load():
    if not _cache:
        with np.load(GOLDEN, allow_pickle=False) as z:
            _cache.update({k: z[k] for k in z.files})
    return _cache


def x64_of(x32):
    """The float64 input of a statistics case, as the generator defines it."""
    return x32.astype(np.float64) / 3.0


def offsets(dirosion):
    """The true cells of generate_binary_structure(2, dirosion): |di| + |dj| <= max(dirosion, 1) inside the 3 x 3."""
    c = max(int(dirosion), 1)
    return [(di, dj) for di in (-1, 0, 1) for dj in (-1, 0, 1) if abs(di) + abs(dj) <= c]


def shifted(a, di, dj):
    """b[i, j] = a[i + di, j + dj], zero outside."""
    nx, ny = a.shape
    p = np.zeros((nx + 2, ny + 2), dtype=bool)
    p[1:-1, 1:-1] = a
    return p[1 + di:1 + di + nx, 1 + dj:1 + dj + ny]


def closing(mask, dirosion):
    """One dilation and one erosion with the outside of the image counting as 0 in both; dirosion 0: the mask."""
    if not dirosion:
        return mask.copy()
    offs = offsets(dirosion)
    dil = np.zeros_like(mask)
    for o in offs:
        dil |= shifted(mask, *o)
    ero = np.ones_like(mask)
    for o in offs:
        ero &= shifted(dil, *o)
    return ero


def test_bindings_declared():
    from pfb_clean_amd import _lib
    header = open(os.path.join(HERE, '..', 'include', 'pfb_hip.h')).read()
    for name in ('pfb_cycle_work_bytes', 'pfb_bandsum_stats', 'pfb_mask_close', 'pfb_masked_problem'):
        assert name in _lib.SIGNATURES and name + '(' in header
    from pfb_clean_amd.utils import cycle
    assert f'#define PFB_CYCLE_RECORD {cycle.RECORD}\n' in header
    assert _lib.load().pfb_abi_version() == 1


def test_work_bytes_in_and_out_of_range():
    from pfb_clean_amd import _lib
    from pfb_clean_amd.utils import cycle
    lib = _lib.load()
    one = lib.pfb_cycle_work_bytes(1)
    assert one > 0 and one % (8 * cycle.RECORD) == 0
    for nset in (2, 7, 65535):
        assert lib.pfb_cycle_work_bytes(nset) == nset * one
    for nset in (0, -1, 65536, 2 ** 31 - 1):
        assert lib.pfb_cycle_work_bytes(nset) == 0


def test_golden_shapes_and_counts():
    g = load()
    assert int(g['nstat']) == len(STAT_SHAPES)
    for k, shape in enumerate(STAT_SHAPES):
        assert g[f'st{k}_x32'].shape == shape and g[f'st{k}_x32'].dtype == np.float32
        assert g[f'st{k}_model'].shape == (3,) + shape[1:] and g[f'st{k}_model'].dtype == np.float32
        assert g[f'st{k}_mfs32'].dtype == np.float32 and g[f'st{k}_mfs64'].dtype == np.float64
        assert g[f'st{k}_std32'].dtype == np.float32 and g[f'st{k}_std64'].dtype == np.float64
    shapes = {g[f'cl{k}_mask'].shape for k in range(int(g['nclose']))}
    assert shapes == set(CLOSE_SHAPES)
    assert g['close_dirosions'].tolist() == [0, 1, 2, 3]
    names = [str(n).split(':')[1] for n in g['close_names']]
    for want in ('corner00', 'edge_left', 'interior', 'gap1_rows', 'gap2_cols', 'gap3_rows', 'diagonal', 'random0.02',
                 'random0.2', 'random0.6', 'tile_cols', 'tile_rows', 'tile_cols_gap', 'tile_rows_gap', 'ones', 'zeros'):
        assert want in names, want


@pytest.mark.parametrize('k', range(len(STAT_SHAPES)))
def test_band_sums_are_sequential_sums(k):
    g = load()
    x32, model = g[f'st{k}_x32'], g[f'st{k}_model']
    for bits, x in ((32, x32), (64, x64_of(x32))):
        s = x[0].copy()
        for b in range(1, x.shape[0]):
            s = s + x[b]
        assert s.dtype == x.dtype and np.array_equal(s, g[f'st{k}_mfs{bits}'])
        assert float(g[f'st{k}_rmax{bits}']) == float(np.abs(s).max())
        quiet = ~(model != 0).any(axis=0)
        assert int(g[f'st{k}_nquiet']) == int(quiet.sum())
        ref = np.std(s.astype(np.float64))
        assert abs(float(g[f'st{k}_std{bits}']) - ref) <= (1e-6 if bits == 32 else 1e-13) * max(ref, 1e-300) or ref == 0
        if quiet.any():
            qref = np.std(s[quiet].astype(np.float64))
            assert abs(float(g[f'st{k}_qstd{bits}']) - qref) <= (1e-6 if bits == 32 else 1e-13) * qref or qref == 0
        else:
            assert np.isnan(g[f'st{k}_qstd{bits}'])


@pytest.mark.parametrize('shape', CLOSE_SHAPES)
def test_closings_are_or_then_and_of_shifts(shape):
    g = load()
    seen = 0
    for k in range(int(g['nclose'])):
        mask = g[f'cl{k}_mask']
        if mask.shape != shape:
            continue
        assert mask.dtype == bool
        for d in g['close_dirosions']:
            assert np.array_equal(closing(mask, int(d)), g[f'cl{k}_out{int(d)}']), (str(g['close_names'][k]), int(d))
        seen += 1
    assert seen >= 2


def test_closing_properties_of_the_stored_cases():
    """What the GPU tests lean on: border pixels vanish, a closing contains nothing outside the dilation and keeps every
    interior pixel of the support, structures 2 and 3 agree."""
    g = load()
    for k in range(int(g['nclose'])):
        mask = g[f'cl{k}_mask']
        assert np.array_equal(g[f'cl{k}_out0'], mask)
        assert np.array_equal(g[f'cl{k}_out2'], g[f'cl{k}_out3'])
        for d in (1, 2):
            res = g[f'cl{k}_out{d}']
            assert not res[0].any() and not res[-1].any() and not res[:, 0].any() and not res[:, -1].any()
            inner = np.zeros_like(mask)
            inner[1:-1, 1:-1] = mask[1:-1, 1:-1]
            assert not (inner & ~res).any()
