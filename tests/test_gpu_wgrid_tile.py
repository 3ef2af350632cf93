"""
The tile-owned gridder (reproducible=True; csrc/wgrid.hip: pfb_wgrid_order_keys64, pfb_wgrid_order_coords,
pfb_wgrid_grid_tile[_multi]; DESIGN 4.10 "The tile-owned gridder") on the MI355X, through the C ABI and through Python,
against the numpy references of tests/wgrid_tile_cases.py (tests/test_cpu_wgrid_tile_cases.py proves them and the
table on the CPU).

Order   integers and fp64 coordinates, exact: the keys, idx against numpy's stable sort, coord bit for bit, the planes'
        offsets, and the map against the reference's CSR -- from the C ABI's keys and from a WgridPlan's own.
Kernel  per plane and product against wgrid_kernel_cases.ref_grid_plane: both types, every support 4 .. 12, 1 and 4
        products (2 and 3 at W = 7), on a grid of one tile, of two, with partial last tiles of 8 and 4 cells, first
        cells at N - 1 and in the last tile from below zero on both axes at once, a target that walks exactly one staging
        batch of 64 slots and one whose batches end between two segments and inside one, planes that hold nothing and
        slots exactly on the zero of the w weight.
        The bound is the project's, |got - ref| <= C U S with C = wgrid_kernel_cases.TOLERANCE_C['grid'] (8192 / 2048):
        every contribution is formed as k_grid forms it, product by product.  Where S is zero the result is exactly zero.
        Worst |got - ref| / (U S) recorded on the MI355X over the table (test_zz_report prints it):
            fp32  276.4  (W = 6 'batches', plane 0; every other kind of entry: 151.9, W = 10 'partial' plane 0)
            fp64  160.5  (W = 10 'partial', plane 0; the 'batches' entries: 99.3 at W = 7)
        The same figure shows for every product of an entry, whatever its values: it is the error of one kernel tap
        evaluated in the data type near the rim (test_gpu_wgrid_kernels.py describes it), not summation error.  The
        many-slot entries (139 slots in a target's list) stay under C like the others: no term grew, C stands.
Bits    two launches on a NaN-filled grid, and two plans built independently from the same arrays, give identical bits
        (np.array_equal on the integer views / torch.equal), end to end for vis2dirty, the stacked IQUV call, the Hessian
        and image_data_products with k = 0 counts; a default-mode call in between neither changes them nor finds their plan.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import wgrid_cases as wc
import wgrid_kernel_cases as kc
import wgrid_tile_cases as tc

pytestmark = pytest.mark.gpu
pmp = pytest.mark.parametrize

RDT = {'f32': torch.float32, 'f64': torch.float64}
CDT = {'f32': torch.complex64, 'f64': torch.complex128}
NAN = float('nan')
_worst = {}


@pytest.fixture(scope='module')
def lib():
    from pfb_clean_amd import _lib
    return _lib.load()


class Plan:
    """The native plan of a geometry record; `call` returns the status of pfb_wgrid_<name> on the current stream."""

    def __init__(self, lib, geom):
        from pfb_clean_amd import _lib
        self.lib, self.ok, self.h = lib, _lib.PFB_OK, C.c_void_p()
        code = _lib.PFB_F32 if geom['dtype'] == 'f32' else _lib.PFB_F64
        assert lib.pfb_wgrid_plan_create(code, geom['nx'], geom['ny'], geom['px'], geom['py'], geom['cx'], geom['cy'],
                                         geom['W'], geom['nplanes'], geom['w0'], geom['dw'], C.byref(self.h)) == self.ok

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.lib.pfb_wgrid_plan_destroy(self.h)

    def call(self, name, *args):
        args = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
        return getattr(self.lib, 'pfb_wgrid_' + name)(self.h, *args, torch.cuda.current_stream().cuda_stream)

    def run(self, name, *args):
        assert self.call(name, *args) == self.ok, self.lib.pfb_last_error()


def dev(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype).contiguous()


def host(t):
    a = t.cpu().numpy()
    return a.astype(np.complex128 if np.iscomplexobj(a) else np.float64)


def bits(t):
    return torch.view_as_real(t).cpu().numpy().view(np.int32 if t.dtype == torch.complex64 else np.int64)


def rounded(a, dtype):
    return a.astype(np.complex64 if dtype == 'f32' else np.complex128).astype(np.complex128)


def same_map(got, ref):
    """The five device arrays of a map against the reference's (tgt_tile, tgt_ptr, pair_start, pair_count, pair_p0)."""
    assert [t.dtype for t in got] == [torch.int32, torch.int64, torch.int64, torch.int32, torch.int32]
    for g, r in zip(got, ref[:5]):
        assert np.array_equal(g.cpu().numpy(), r)


# --------------------------------------------------------------------------------------------------------- order
@pmp('entry', tc.ORDER, ids=tc.ORDER_IDS)
def test_order_and_map_through_the_c_abi(lib, entry):
    from pfb_clean_amd.operators import gridder
    geom, uvw, freq, mask = kc.order_data(entry)
    nrow, nchan = entry['nrow'], entry['nchan']
    ref_idx, ref_coord, ref_off, ref_skeys = tc.ref_tile_order(geom, uvw, freq, mask)
    uvw_d, freq_d, mask_d = dev(uvw), dev(freq), dev(mask)
    with Plan(lib, geom) as plan:
        keys = torch.full((nrow * nchan,), -7, dtype=torch.int64, device='cuda')
        plan.run('order_keys64', uvw_d, freq_d, mask_d, nrow, nchan, keys)
        assert np.array_equal(keys.cpu().numpy(), tc.ref_keys64(geom, uvw, freq, mask))
        skeys, order = torch.sort(keys, stable=True)
        ns = ref_off[-1]
        assert ns >= 1 and np.array_equal(order[:ns].cpu().numpy(), ref_idx)          # numpy's stable sort, exactly
        idx = order[:ns].to(torch.int32)
        coord = torch.full((3, ns), NAN, dtype=torch.float64, device='cuda')
        plan.run('order_coords', uvw_d, freq_d, nrow, nchan, idx, ns, coord)
        assert np.array_equal(coord.cpu().numpy().view(np.int64), ref_coord.view(np.int64))          # bit for bit
    ukeys, counts = torch.unique_consecutive(skeys[:ns], return_counts=True)
    got = gridder.tile_map(ukeys, torch.cumsum(counts, 0) - counts, counts, geom['Nu'], geom['Nv'], geom['W'])
    same_map(got, tc.ref_tile_map(geom, *tc.segments(ref_skeys)))


@pmp('entry', tc.ORDER[1::2], ids=tc.ORDER_IDS[1::2])
def test_order_and_map_of_a_plan(entry):
    """A WgridPlan(reproducible=True) lays out its own planes: its order and map against the references on ITS geometry,
    and a second plan built from the same arrays holds the same bits."""
    from pfb_clean_amd.operators import gridder
    g0, uvw, freq, mask = kc.order_data(entry)
    mask2 = None if mask is None else mask.reshape(entry['nrow'], entry['nchan'])
    plans = [gridder.WgridPlan(uvw, freq, mask2, g0['nx'], g0['ny'], g0['px'], g0['py'], 0.0, 0.0, 1e-5, True,
                               torch.float64, reproducible=True) for _ in range(2)]
    p = plans[0]
    geom = kc.geometry('f64', g0['nx'], g0['ny'], p.W, nplanes=p.nplanes, w0=p.w0, dw=p.dw, px=g0['px'], py=g0['py'])
    idx, coord, plane_off, skeys = tc.ref_tile_order(geom, uvw, freq, mask)
    assert p.reproducible and p.nsorted == idx.size and p.plane_off == plane_off
    assert np.array_equal(p.idx.cpu().numpy(), idx)
    assert np.array_equal(p.coord.cpu().numpy().view(np.int64), coord.view(np.int64))
    same_map(p.tile_map, tc.ref_tile_map(geom, *tc.segments(skeys)))
    q = plans[1]
    assert torch.equal(p.idx, q.idx) and torch.equal(p.coord.view(torch.int64), q.coord.view(torch.int64))
    assert all(torch.equal(a, b) for a, b in zip(p.tile_map, q.tile_map))
    for plan in plans:
        plan.close()


# -------------------------------------------------------------------------------------------------------- kernel
def figure(got, ref, S):
    """max over elements and components of |got - ref| / S; exactly zero where S is zero."""
    worst = 0.0
    got, ref, S = (np.asarray(a, dtype=np.complex128) for a in (got, ref, S))
    assert np.isfinite(got.real).all() and np.isfinite(got.imag).all()
    for d, s in ((np.abs(got.real - ref.real), S.real), (np.abs(got.imag - ref.imag), S.imag)):
        on = s > 0
        assert not d[~on].any(), "a value with no contribution is not exactly zero"
        if on.any():
            worst = max(worst, float((d[on] / s[on]).max()))
    return worst


@pmp('entry', tc.TILE, ids=tc.TILE_IDS)
def test_grid_tile(lib, entry):
    geom, n = entry['geom'], entry['n']
    dtype, Nu, Nv = geom['dtype'], geom['Nu'], geom['Nv']
    coord, val, _, tmap = tc.tile_data(entry)
    val = rounded(val, dtype)
    val_d, coord_d = dev(val, CDT[dtype]), dev(coord)
    map_d = [dev(a) for a in tmap[:5]]
    sizes = (tmap[0].size, tmap[2].size)
    refs = {(plane, k): kc.ref_grid_plane(geom, coord, val[k], plane, 0, n) for plane in entry['planes']
            for k in range(tc.NPROD)}
    C_grid = kc.TOLERANCE_C['grid'][dtype]
    with Plan(lib, geom) as plan:
        for plane in entry['planes']:
            for nprod in entry['nprods']:
                runs = []
                for _ in range(2):
                    grid = torch.full((nprod, Nu, Nv), NAN, dtype=CDT[dtype], device='cuda')        # "grid = 0, then"
                    if nprod == 1:
                        plan.run('grid_tile', plane, val_d, coord_d, n, *map_d, *sizes, grid)
                    else:          # the stack's planes are n apart: the first nprod rows of val
                        plan.run('grid_tile_multi', nprod, plane, val_d, coord_d, n, *map_d, *sizes, grid)
                    runs.append(grid)
                assert np.array_equal(bits(runs[0]), bits(runs[1]))          # identical bits, not a tolerance
                got = host(runs[0])
                for k in range(nprod):
                    ref, S = refs[plane, k]
                    r = figure(got[k], ref, S) / kc.U[dtype]
                    what = (dtype, 'batches' if entry['kind'] == 'batches' else 'other')
                    _worst[what] = max(_worst.get(what, (0.0, '')), (r, f"{entry['id']} plane {plane}"))
                    print(f"{entry['id']} plane {plane} product {k} of {nprod}: |got - ref| / (U S) = {r:.3g}")
                    assert r <= C_grid, (entry['id'], plane, nprod, k, r)
                if plane >= geom['W'] + 2:          # no first plane in range: nothing but the launcher's zeros
                    assert not got.any()


def test_multi_equals_single_bit_for_bit(lib):
    """Product k of a stacked launch is the single launch on plane k of val: the same sums in the same order."""
    entry = tc.TILE[tc.TILE_IDS.index('W7-f64-partial')]
    geom, n = entry['geom'], entry['n']
    coord, val, _, tmap = tc.tile_data(entry)
    val_d, coord_d, map_d = dev(val), dev(coord), [dev(a) for a in tmap[:5]]
    sizes = (tmap[0].size, tmap[2].size)
    with Plan(lib, geom) as plan:
        stack = torch.full((4, geom['Nu'], geom['Nv']), NAN, dtype=torch.complex128, device='cuda')
        plan.run('grid_tile_multi', 4, 2, val_d, coord_d, n, *map_d, *sizes, stack)
        for k in range(4):
            one = torch.full((geom['Nu'], geom['Nv']), NAN, dtype=torch.complex128, device='cuda')
            plan.run('grid_tile', 2, val_d[k], coord_d, n, *map_d, *sizes, one)
            assert np.array_equal(bits(one), bits(stack[k]))


# ------------------------------------------------------------------------------------------------------ end to end
def kw(case):
    return dict(pixsize_x=case['px'], pixsize_y=case['py'], center_x=case['cx'], center_y=case['cy'],
                epsilon=case['eps'], do_wgridding=case['do_wgridding'], divide_by_n=case['divide_by_n'])


def case_named(name):
    return wc.CASES[wc.CASE_IDS.index(name)]


def tensors(case):
    return {k: (dev(case[k]) if case.get(k) is not None else None) for k in ('uvw', 'freq', 'vis', 'wgt', 'mask')}


def v2d(case, t, vis, wgt, **extra):
    from pfb_clean_amd.operators.gridder import vis2dirty
    return vis2dirty(t['uvw'], t['freq'], vis, wgt=wgt, mask=t['mask'], npix_x=case['nx'], npix_y=case['ny'],
                     **kw(case), **extra)


# fp64 at the case's epsilon; fp32 at gridder.EPS_MIN on the cases test_gpu_wgrid.py holds to that bound
E2E = ([(name, False) for name in ('32x24-eps1e-05', '48x16-eps1e-07', 'centre', 'seam', 'one-cell', 'no-wgrid')]
       + [(name, True) for name in ('32x24-eps1e-09', '48x16-eps1e-07', '16x64-eps1e-05', 'centre', 'one-cell')])


@pmp('name,single', E2E, ids=[f"{n}-{'f32-at-eps-min' if s else 'f64'}" for n, s in E2E])
def test_vis2dirty_reproducible(name, single):
    from pfb_clean_amd.operators import gridder
    case = case_named(name)
    if single:
        case = wc.as_f32(dict(case, eps=gridder.EPS_MIN[torch.float32]))
    t = tensors(case)
    gridder.clear_plan_cache()
    miss = gridder.cache_stats['miss']
    first = v2d(case, t, t['vis'], t['wgt'], reproducible=True)
    assert gridder.cache_stats['miss'] == miss + 1
    default = v2d(case, t, t['vis'], t['wgt'])                      # its own plan: it does not find the reproducible one
    assert gridder.cache_stats['miss'] == miss + 2
    again = v2d(case, t, t['vis'], t['wgt'], reproducible=True)
    assert gridder.cache_stats['miss'] == miss + 2 and torch.equal(first, again)
    gridder.clear_plan_cache()                                     # a plan built independently from the same arrays
    assert torch.equal(first, v2d(case, t, t['vis'], t['wgt'], reproducible=True))
    ref = wc.direct_vis2dirty(case, case['vis'])
    err, err_default = wc.rel_l2(host(first), ref), wc.rel_l2(host(default), ref)
    print(f"{name} {case['dtype']}: vis2dirty reproducible {err:.3e} default {err_default:.3e} (eps {case['eps']:g})")
    assert first.dtype == RDT[case['dtype']] and err <= case['eps'] and err_default <= case['eps']


@pmp('name', ['32x24-eps1e-05', 'centre'])
def test_stacked_iquv_reproducible(name):
    case = case_named(name)
    t = tensors(case)
    rng = np.random.default_rng(77)
    scale = rng.standard_normal(4) + 1j * rng.standard_normal(4)
    vis4 = np.stack([case['vis'] * s for s in scale])
    runs = [v2d(case, t, dev(vis4), t['wgt'], reproducible=True) for _ in range(2)]
    assert runs[0].shape == (4, case['nx'], case['ny']) and torch.equal(runs[0], runs[1])
    for k in range(4):
        assert wc.rel_l2(host(runs[0][k]), wc.direct_vis2dirty(case, vis4[k])) <= case['eps']
    # plane 0 of the stack under the plan that a 2-D call finds: the same sums
    assert torch.equal(runs[0][0], v2d(case, t, dev(vis4[0]), t['wgt'], reproducible=True))


@pmp('name', ['32x24-eps1e-05', '48x16-eps1e-07', 'centre', 'no-wgrid'])
def test_hessian_reproducible(name):
    from pfb_clean_amd.operators import gridder
    from pfb_clean_amd.operators.hessian import hessian
    c = dict(case_named(name), divide_by_n=False)
    c['py'] = c['px'] = min(c['px'], c['py'])
    rng = np.random.default_rng(21)
    beam, x = rng.uniform(0.5, 1.0, (c['nx'], c['ny'])), rng.standard_normal((c['nx'], c['ny']))
    t = tensors(c)
    opts = dict(x0=c['cx'], y0=c['cy'], cell=c['px'], do_wgridding=c['do_wgridding'], epsilon=c['eps'],
                double_accum=True, nthreads=4)
    xd, bd = dev(x), dev(beam)

    def H(**more):
        return hessian(xd, t['uvw'], t['wgt'], t['mask'], t['freq'], bd, dict(opts, **more))
    gridder.clear_plan_cache()
    miss = gridder.cache_stats['miss']
    first = H(reproducible=True)
    H()
    assert gridder.cache_stats['miss'] == miss + 2
    assert torch.equal(first, H(reproducible=True)) and gridder.cache_stats['miss'] == miss + 2
    err = wc.rel_l2(host(first), wc.direct_hessian(c, x, beam))
    print(f"{name}: reproducible hessian rel err {err:.3e} (eps {c['eps']:g})")
    assert err <= 2 * c['eps']


def test_compute_residual_follows():
    from pfb_clean_amd.operators.fft import psfhat_from_psf
    from pfb_clean_amd.operators.hessian import hessian_psf_slice

    class Var:
        def __init__(self, a):
            self.values, self.dtype, self.shape = a, a.dtype, a.shape

    class DS(dict):
        def __getattr__(self, k):
            try:
                return self[k]
            except KeyError:
                raise AttributeError(k)
    c = dict(case_named('32x24-eps1e-05'), divide_by_n=False)
    c['py'] = c['px'] = min(c['px'], c['py'])
    rng = np.random.default_rng(5)
    nx, ny = c['nx'], c['ny']
    psf = rng.standard_normal((2 * nx, 2 * ny))
    ds = DS(DIRTY=Var(rng.standard_normal((nx, ny))), PSF=Var(psf), PSFHAT=Var(psfhat_from_psf(psf)),
            BEAM=Var(rng.uniform(0.5, 1.0, (nx, ny))), WSUM=Var(np.array([1.0])), bandid=0, UVW=Var(c['uvw']),
            FREQ=Var(c['freq']),
            WEIGHT=Var(np.ones(c['vis'].shape) if c['wgt'] is None else c['wgt']),
            VIS_MASK=Var(np.ones(c['vis'].shape, np.uint8) if c['mask'] is None else c['mask']))
    ops = [hessian_psf_slice(ds, 1, 8, 1, 0.0, cell=c['px'], do_wgridding=True, epsilon=c['eps'], double_accum=True,
                             reproducible=r) for r in (True, True, False)]
    x = rng.standard_normal((nx, ny))
    res = [op.compute_residual(x) for op in ops]
    assert np.array_equal(res[0].view(np.int64), res[1].view(np.int64))
    assert wc.rel_l2(res[0], res[2]) <= 2 * c['eps']


def test_image_data_products_reproducible():
    from pfb_clean_amd.operators import gridder
    from pfb_clean_amd.utils import weighting
    c = case_named('32x24-eps1e-05')
    cell = min(c['px'], c['py'])
    nx, ny = c['nx'], c['ny']
    t = tensors(c)
    mask = t['mask'] if t['mask'] is not None else torch.ones(t['vis'].shape, dtype=torch.uint8, device='cuda')
    wgt = t['wgt'] if t['wgt'] is not None else torch.ones(t['vis'].shape, dtype=torch.float64, device='cuda')
    counts = weighting.compute_counts(t['uvw'], t['freq'], mask, nx, ny, cell, cell, torch.float64, k=0)
    model = dev(np.random.default_rng(3).standard_normal((nx, ny)))

    def products(**more):
        return gridder.image_data_products(t['uvw'], t['freq'], t['vis'], wgt, mask, counts, nx, ny, 2 * nx, 2 * ny, cell,
                                           cell, model=model, robustness=0.0, epsilon=c['eps'], do_wgridding=True,
                                           double_accum=True, **more)
    gridder.clear_plan_cache()
    first = products(reproducible=True)
    default = products()
    again = products(reproducible=True)
    for key in ('DIRTY', 'PSF', 'RESIDUAL'):
        assert torch.equal(first[key], again[key]), key
        assert wc.rel_l2(host(first[key]), host(default[key])) <= 2 * c['eps']


def test_masks_and_empty_plans():
    """Partial, all-but-one and all-zero masks through Python; the all-zero mask answers zeros without a launch."""
    from pfb_clean_amd.operators import gridder
    case = case_named('32x24-eps1e-05')
    rng = np.random.default_rng(9)
    nvis = case['vis'].size
    one = np.zeros(nvis, np.uint8)
    one[rng.integers(nvis)] = 1
    for mask in ((rng.uniform(size=nvis) < 0.6).astype(np.uint8), one, np.zeros(nvis, np.uint8)):
        c = dict(case, mask=mask.reshape(case['vis'].shape))
        t = tensors(c)
        got = [v2d(c, t, t['vis'], t['wgt'], reproducible=True) for _ in range(2)]
        assert torch.equal(got[0], got[1])
        if not mask.any():
            assert not got[0].any()
        else:
            assert wc.rel_l2(host(got[0]), wc.direct_vis2dirty(c, c['vis'])) <= c['eps']
    gridder.clear_plan_cache()


# -------------------------------------------------------------------------------------------------------- refusals
def test_refusals(lib):
    from pfb_clean_amd import _lib
    from pfb_clean_amd.operators import gridder
    case = case_named('32x24-eps1e-05')
    with pytest.raises(ValueError, match='degrid_only'):
        gridder.WgridPlan(case['uvw'], case['freq'], None, case['nx'], case['ny'], case['px'], case['py'], 0.0, 0.0,
                          case['eps'], True, torch.float64, degrid_only=True, reproducible=True)
    entry = tc.TILE[tc.TILE_IDS.index('W7-f64-two-tiles')]
    geom, n = entry['geom'], entry['n']
    coord, val, _, tmap = tc.tile_data(entry)
    val_d, coord_d = dev(val[0]), dev(coord)
    sizes = (tmap[0].size, tmap[2].size)
    grid = torch.full((geom['Nu'], geom['Nv']), 7.25, dtype=torch.complex128, device='cuda')

    def refused(name, what, *args):
        with Plan(lib, geom) as plan:          # a fresh plan: it has taken no map as read
            assert plan.call(name, *args) == _lib.PFB_ERR_INVALID
            msg = lib.pfb_last_error().decode()
            assert msg.startswith(f'wgrid_{name}:') and what in msg, msg
    past = [a.copy() for a in tmap[:5]]
    past[3][-1] += 1 + n - (past[2][-1] + past[3][-1])          # the last pair ends one slot past nsorted
    refused('grid_tile', 'outside the 300 slots', 0, val_d, coord_d, n, *[dev(a) for a in past], *sizes, grid)
    refused('grid_tile_multi', 'outside the 300 slots', 1, 0, val_d, coord_d, n, *[dev(a) for a in past], *sizes, grid)
    tiles = [a.copy() for a in tmap[:5]]
    tiles[0][-1] = 4                                             # 2 x 2 fine tiles
    refused('grid_tile', 'a target outside the 4 fine tiles', 0, val_d, coord_d, n, *[dev(a) for a in tiles], *sizes, grid)
    refused('grid_tile_multi', '5 products', 5, 0, val_d, coord_d, n, *[dev(a) for a in tmap[:5]], *sizes, grid)
    refused('grid_tile', 'plane 1 of 1', 1, val_d, coord_d, n, *[dev(a) for a in tmap[:5]], *sizes, grid)
    torch.cuda.synchronize()
    assert (grid == 7.25).all()                                  # a refused call writes nothing


def test_zz_report():
    """The worst figures of this run (run with -s to read them)."""
    for (dtype, kind), (r, where) in sorted(_worst.items()):
        print(f"recorded grid_tile {dtype} {kind:8s}: {r:10.3f} at {where}   C = {kc.TOLERANCE_C['grid'][dtype]:g}")
