"""
The w-gridder with a product axis on the MI355X: up to four planes (the Stokes products of one chunk) through
vis2dirty / dirty2vis under ONE plan and order (pfb_clean_amd.operators.gridder), and the pfb_wgrid_*_multi entry points
of csrc/wgrid.hip one by one through the C ABI.

Plane k of a stack is the case's (or table entry's) own data rolled by k rows and multiplied by a fixed factor --
FACT_C[k] for complex data, FACT_R[k] for real --, so that no two planes are equal or proportional; per-product weights
are the base weights rolled by k rows times 1 + k / 4.

Bounds: the single operators' own, per plane
  accuracy      |plane - direct sum|_2 / |direct sum|_2 <= epsilon, both directions, every case of wgrid_cases.CASES and
                the fp32 cases at gridder.EPS_MIN, for stacks of 2, 3, 4 planes with per-product weights, one shared
                weight plane and none.
  kernels       per element and component |got - ref| <= C U S with the C of wgrid_kernel_cases.TOLERANCE_C (4 x what the
                single kernels recorded): per plane the multi kernels perform the single kernels' operations, so the
                constants must hold.  Worst |got - ref| / (U S) over every table entry, plane and nprod = 1 .. 4,
                recorded on the MI355X (test_zz_report prints them):

                                    fp32 (C)            fp64 (C)
                    grid            1024.1  (8192)      451.1  (2048)
                    degrid           288.4  (1024)      116.2   (256)
                    prep               2.14   (16)       45.0   (256)
                    finish             1.99    (8)       37.2   (256)
                    image_forward      0.98    (4)        2.95   (16)
                    image_adjoint      1.80    (8)        2.88   (16)
                    image_correct      1.00    (4)        0      (1)

                The figures above the single kernels' (degrid 163 / 48.3, prep fp64 38.1, finish fp64 32.1) come from
                planes 1 .. 3, whose data the single tests do not see (rolled and scaled by FACT_C).  Plane 0 is the
                single tests' data and records the single kernels' own figures to every digit printed (degrid 162.956 /
                48.343, prep 2.143 / 38.142, finish 1.587 / 32.133, image_adjoint 1.801 / 2.445; grid 1024.0 / 449.9, its
                last digits moving with the order of the atomic adds): test_zz_report prints them as "(plane 0)".

  no leakage    a plane of zeros in gives a plane of EXACT zeros out while the others are not zero, gridding (atomics)
                and degridding; masked visibilities are exact zeros in every plane.
  adjointness   per plane, wgrid_cases.adjoint_mismatch at the criterion of test_gpu_wgrid.py:
                <= 100 max(the numpy model's mismatch, HALF_ULP).
  same plan     a 2-D call, a stacked call and a (1, nrow, nchan) call on the same arrays build one plan; the (1, ..)
                result equals the 2-D one to 1e-12 (the same sums in another order of the atomic adds).
  composition   stokes_vis(product='IQUV') straight into vis2dirty against the same call fed the closed form's vis and
                wgt: per pixel (2 K + nvis) eps S, S = sum_i wgt_i |vis_i| (1 + epsilon) of the plane -- a pixel is a sum
                over the visibilities of wgt_i vis_i times factors of modulus <= 1 up to the gridder's epsilon; K eps each
                from vis and wgt, nvis eps for nvis terms added in any order (divide_by_n=False, so no factor 1 / n).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import stokes_cases as sc
import wgrid_cases as wc
import wgrid_kernel_cases as kc
from wgrid_cases import CASES, CASE_IDS

pytestmark = pytest.mark.gpu
pmp = pytest.mark.parametrize

FACT_C = (1.0 + 0.0j, 0.5 - 1.25j, -1.5 + 0.75j, 0.25 + 2.0j)
FACT_R = (1.0, -1.75, 0.625, 2.5)
MAXP = 4
RDT = {'f32': torch.float32, 'f64': torch.float64}
CDT = {'f32': torch.complex64, 'f64': torch.complex128}
NP_R = {'f32': np.float32, 'f64': np.float64}
NP_C = {'f32': np.complex64, 'f64': np.complex128}
NAN = float('nan')
SENTINEL = 7.25
WMODES = ('per', 'shared', 'none')

_worst = {}


def case_named(name):
    return CASES[CASE_IDS.index(name)]


def dev(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype).contiguous()


def plane_of(a, k, fact):
    """Plane k of a stack made from `a`: rolled by k rows, times the k-th factor."""
    return np.roll(a, k, axis=0) * fact[k]


def weight_plane(w, k):
    return np.roll(w, k, axis=0) * (1.0 + 0.25 * k)


def kw(case):
    return dict(pixsize_x=case['px'], pixsize_y=case['py'], center_x=case['cx'], center_y=case['cy'],
                epsilon=case['eps'], do_wgridding=case['do_wgridding'], divide_by_n=case['divide_by_n'])


def v2d(case, vis, wgt, **extra):
    from pfb_clean_amd.operators.gridder import vis2dirty
    return vis2dirty(case['uvw'], case['freq'], vis, wgt=wgt, mask=case['mask'], npix_x=case['nx'], npix_y=case['ny'],
                     **kw(case), **extra)


def d2v(case, dirty, wgt):
    from pfb_clean_amd.operators.gridder import dirty2vis
    return dirty2vis(case['uvw'], case['freq'], dirty, wgt=wgt, mask=case['mask'], **kw(case))


def stack_data(case):
    """The four planes of a case in its data type: vis, dirty, and the weights of every mode (a list per plane, or
    None); the shared mode's plane is weights['shared'][0]."""
    rdt, cdt = NP_R[case['dtype']], NP_C[case['dtype']]
    base = case['wgt']
    if base is None:
        base = np.random.default_rng(case['seed'] + 77).uniform(0.5, 1.5, case['vis'].shape)
    base = base.astype(rdt)
    vis = [plane_of(case['vis'], k, FACT_C).astype(cdt) for k in range(MAXP)]
    dirty = [plane_of(case['dirty'], k, FACT_R).astype(rdt) for k in range(MAXP)]
    weights = {'per': [weight_plane(base, k).astype(rdt) for k in range(MAXP)], 'shared': [base] * MAXP,
               'none': [None] * MAXP}
    return vis, dirty, weights


def weight_arg(weights, mode, nprod):
    if mode == 'none':
        return None
    return weights['shared'][0] if mode == 'shared' else np.stack(weights['per'][:nprod])


# -------------------------------------------------------------------------------------------------------- accuracy
def accuracy(case):
    vis, dirty, weights = stack_data(case)
    rdt, cdt = NP_R[case['dtype']], NP_C[case['dtype']]
    empty = case['mask'] is not None and not case['mask'].any()
    refs = {}

    def ref(mode, k):
        if (mode, k) not in refs:
            refs[mode, k] = (wc.direct_vis2dirty(case, vis[k], wgt=weights[mode][k]),
                             wc.direct_dirty2vis(case, dirty[k], wgt=weights[mode][k]))
        return refs[mode, k]

    worst = 0.0
    for nprod in (2, 3, 4):
        for mode in WMODES:
            w = weight_arg(weights, mode, nprod)
            got_d = v2d(case, np.stack(vis[:nprod]), w)
            got_v = d2v(case, np.stack(dirty[:nprod]), w)
            assert got_d.dtype == rdt and got_d.shape == (nprod, case['nx'], case['ny'])
            assert got_v.dtype == cdt and got_v.shape == (nprod,) + case['vis'].shape
            if case['mask'] is not None:
                assert not got_v[:, case['mask'] == 0].any()
            if empty:
                assert not got_d.any() and not got_v.any()
                continue
            for k in range(nprod):
                want_d, want_v = ref(mode, k)
                e1 = wc.rel_l2(got_d[k].astype(np.float64), want_d)
                e2 = wc.rel_l2(got_v[k].astype(np.complex128), want_v)
                worst = max(worst, e1, e2)
                assert e1 <= case['eps'] and e2 <= case['eps'], (nprod, mode, k, e1, e2)
    print(f"{case['name']}: eps {case['eps']:g}, worst plane of every stack and weight mode {worst:.3e}")


@pmp('case', CASES, ids=CASE_IDS)
def test_accuracy_of_stacks_against_the_direct_sum(case):
    accuracy(case)


@pmp('name', ['32x24-eps1e-09', '48x16-eps1e-07', '16x64-eps1e-05', 'centre', 'one-cell'])
def test_fp32_stacks_at_the_lower_bound(name):
    """Single precision at the smallest epsilon it accepts, as test_gpu_wgrid.py::test_fp32_at_its_lower_bound."""
    from pfb_clean_amd.operators import gridder
    accuracy(wc.as_f32(dict(case_named(name), eps=gridder.EPS_MIN[torch.float32])))


# ------------------------------------------------------------------------------------------------------ no leakage
@pmp('name', ['32x24-eps1e-05', '32x24-f32-eps0.0001', 'centre'])
def test_a_plane_of_zeros_stays_zero(name):
    case = case_named(name)
    vis, dirty, weights = stack_data(case)
    w = weight_arg(weights, 'per', MAXP)
    for k in range(MAXP):
        vs, ds = np.stack(vis), np.stack(dirty)
        vs[k] = 0
        ds[k] = 0
        got_d, got_v = v2d(case, vs, w), d2v(case, ds, w)
        for j in range(MAXP):
            assert got_d[j].any() == (j != k) and got_v[j].any() == (j != k), (k, j)
        if case['mask'] is not None:
            assert (case['mask'] == 0).any() and not got_v[:, case['mask'] == 0].any()


# ----------------------------------------------------------------------------------------------------- adjointness
@pmp('name', ['32x24-eps1e-05', '16x64-eps1e-09', 'centre', 'seam', 'one-cell', 'no-wgrid'])
def test_adjointness_of_every_plane(name):
    case = case_named(name)
    model = wc.adjoint_mismatch(lambda v: wc.model_vis2dirty(case, v), lambda d: wc.model_dirty2vis(case, d), case)
    vis, dirty, _ = stack_data(case)
    wgt = case['wgt']                                     # one plane for every product, as the model has it

    def in_plane(stack, k, x):
        s = np.stack(stack)
        s[k] = x
        return s

    for k in range(MAXP):
        gpu = wc.adjoint_mismatch(lambda v: v2d(case, in_plane(vis, k, v), wgt)[k],
                                  lambda d: d2v(case, in_plane(dirty, k, d), wgt)[k], case)
        print(f"{name} plane {k}: adjoint mismatch model {model:.3e} gpu {gpu:.3e}")
        assert gpu <= 100 * max(model, wc.HALF_ULP)


# ------------------------------------------------------------------------------------------------------- same plan
def test_single_and_stacked_calls_share_one_plan():
    from pfb_clean_amd.operators import gridder
    case = case_named('48x16-eps1e-07')
    vis, dirty, weights = stack_data(case)
    gridder.clear_plan_cache()
    uvw, freq, mask = dev(case['uvw']), dev(case['freq']), dev(case['mask'])
    c = dict(case, uvw=uvw, freq=freq, mask=mask)
    start = gridder.cache_stats['miss']
    w = dev(weights['shared'][0])
    flat_d, flat_v = v2d(c, dev(vis[0]), w), d2v(c, dev(dirty[0]), w)
    assert gridder.cache_stats['miss'] == start + 1
    st_d, st_v = v2d(c, dev(np.stack(vis[:3])), w), d2v(c, dev(np.stack(dirty[:3])), w)
    one_d, one_v = v2d(c, dev(vis[0][None]), w), d2v(c, dev(dirty[0][None]), w)
    assert gridder.cache_stats['miss'] == start + 1
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in (st_d, st_v, one_d, one_v))
    assert one_d.shape == (1,) + flat_d.shape and one_v.shape == (1,) + flat_v.shape
    assert st_d.shape == (3,) + flat_d.shape and st_v.shape == (3,) + flat_v.shape
    for a, b in ((one_d[0], flat_d), (one_v[0], flat_v), (st_d[0], flat_d), (st_v[0], flat_v)):
        assert wc.rel_l2(a.cpu().numpy(), b.cpu().numpy()) <= 1e-12
    # a stack after a larger one, and the single call after both: the buffers of one do not disturb the other
    two_d = v2d(c, dev(np.stack(vis[:2])), w)
    assert wc.rel_l2(two_d.cpu().numpy(), st_d[:2].cpu().numpy()) <= 1e-12
    assert wc.rel_l2(v2d(c, dev(vis[0]), w).cpu().numpy(), flat_d.cpu().numpy()) <= 1e-12
    assert gridder.cache_stats['miss'] == start + 1


def test_all_masked_stack_gives_zeros_without_a_launch():
    case = case_named('mask-zero')
    vis, dirty, weights = stack_data(case)
    got_d, got_v = v2d(case, np.stack(vis[:3]), None), d2v(case, np.stack(dirty[:3]), weights['shared'][0])
    assert got_d.shape == (3, case['nx'], case['ny']) and not got_d.any()
    assert got_v.shape == (3,) + case['vis'].shape and not got_v.any()


# ------------------------------------------------------------------------------------------------- argument checks
def test_argument_checks_leave_the_plan_intact():
    case = case_named('32x24-eps1e-05')
    vis, dirty, weights = stack_data(case)
    w2 = np.stack(weights['per'][:2])
    good_d, good_v = v2d(case, np.stack(vis[:2]), w2), d2v(case, np.stack(dirty[:2]), w2)
    five_v, five_d = np.stack(vis + vis[:1]), np.stack(dirty + dirty[:1])
    w3 = np.stack(weights['per'][:3])
    bad = [lambda: v2d(case, five_v, None), lambda: d2v(case, five_d, None),                       # 5 planes
           lambda: v2d(case, np.stack(vis[:2]), w3), lambda: d2v(case, np.stack(dirty[:2]), w3),   # 3 weight planes for 2
           lambda: v2d(case, np.stack(vis[:2]), w2[:, :-1]),
           lambda: v2d(case, np.stack(vis[:2]).astype(np.complex64), w2),                          # mixed types
           lambda: d2v(case, np.stack(dirty[:2]).astype(np.float32), w2),
           lambda: v2d(case, np.stack(vis[:2])[None], None)]                                       # four dimensions
    for call in bad:
        with pytest.raises((ValueError, TypeError)):
            call()
        again_d, again_v = v2d(case, np.stack(vis[:2]), w2), d2v(case, np.stack(dirty[:2]), w2)
        assert wc.rel_l2(again_d, good_d) <= 1e-12 and np.array_equal(again_v, good_v)         # degridding: no atomics


# ----------------------------------------------------------------------------------------------------- composition
@pmp('tag', ('f32', 'f64'))
def test_stokes_vis_iquv_feeds_vis2dirty(tag):
    """Raw columns -> stokes_vis(product='IQUV') -> vis2dirty, tensors all the way, against the same stacked call fed
    the closed form's vis and wgt of every product (the module's docstring has the bound)."""
    from pfb_clean_amd.operators.gridder import vis2dirty
    from pfb_clean_amd.utils.stokes import stokes_vis
    c = case_named('32x24-eps1e-05')
    case = sc.case_named('sv-spectrum-minus-full')
    assert c['vis'].shape == case['ref_vis'].shape == sc.COMPOSE_SHAPE
    a = sv_args(case, tag, product='IQUV')
    t = {k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in a.items()}
    vis, wgt, mask, wsum = stokes_vis(**t)
    assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in (vis, wgt, mask, wsum))
    assert vis.shape == wgt.shape == (4,) + sc.COMPOSE_SHAPE and mask.shape == sc.COMPOSE_SHAPE

    def image(vis, wgt, mask):
        return vis2dirty(dev(c['uvw']), dev(c['freq']), vis, wgt=wgt, mask=mask, npix_x=c['nx'], npix_y=c['ny'],
                         pixsize_x=c['px'], pixsize_y=c['py'], center_x=c['cx'], center_y=c['cy'], epsilon=c['eps'],
                         do_wgridding=c['do_wgridding'], divide_by_n=False)

    forms = [sc.closed_form(dict(case, product=p)) for p in 'IQUV']
    live = forms[0][2] != 0
    assert np.array_equal(mask.cpu().numpy(), forms[0][2])
    got = image(vis, wgt, mask).cpu().numpy()
    want = image(dev(np.stack([f[0] for f in forms]).astype(sc.CDT[tag])),
                 dev(np.stack([f[1] for f in forms]).astype(sc.RDT[tag])), dev(forms[0][2])).cpu().numpy()
    assert got.shape == want.shape == (4, c['nx'], c['ny']) and got.dtype == want.dtype == sc.RDT[tag]
    nvis, figures = int(live.sum()), []
    for k, f in enumerate(forms):
        s = float((f[1] * np.abs(f[0]))[live].sum()) * (1 + c['eps'])
        assert want[k].any()
        figures.append(float(np.abs(got[k] - want[k]).max()) / ((2 * sc.K + nvis) * sc.EPS[tag] * s))
    print(f"composition {tag}: worst pixel over its bound, planes I Q U V: " + ', '.join(f'{v:.3g}' for v in figures))
    assert all(v <= 1 for v in figures), figures


def sv_args(case, tag, **over):
    """The arguments of stokes_vis for an 'sv' case; data, weights and Jones terms in the type under test."""
    s = case['set']
    cdt, rdt = sc.CDT[tag], sc.RDT[tag]
    j = sc.jones_arg(case)
    args = dict(data=sc.corr_arg(case, s['data']).astype(cdt), ant1=s['ant1'], ant2=s['ant2'], tbin_idx=s['tbin_idx'],
                tbin_counts=s['tbin_counts'], poltype=case['pol'], product=case['product'],
                jones=None if j is None else j.astype(cdt), precision={'f32': 'single', 'f64': 'double'}[tag])
    if case['op'] != 'none':
        args.update(data2=sc.corr_arg(case, s['data2']).astype(cdt), operator=case['op'])
    if case['wform'] == 'sigma':
        args['sigma'] = sc.corr_arg(case, s['sigma']).astype(rdt)
    elif case['wform'] != 'none':
        args['weight'] = sc.corr_arg(case, s['wrow' if case['wform'] == 'row' else 'weight']).astype(rdt)
    if case['use_flag']:
        args['flag'] = sc.corr_arg(case, s['flag3'])
    if case['use_frow']:
        args['frow'] = s['frow']
    args.update(over)
    return args


# ------------------------------------------------------------------------------------- the kernels, through the C ABI
@pytest.fixture(scope='module')
def lib():
    from pfb_clean_amd import _lib
    return _lib.load()


class Plan:
    """The native plan of a geometry record; `run` calls pfb_wgrid_<name> on the current stream and checks its status."""

    def __init__(self, lib, geom):
        from pfb_clean_amd import _lib
        self.lib, self.ok, self.h = lib, _lib.PFB_OK, C.c_void_p()
        code = _lib.PFB_F32 if geom['dtype'] == 'f32' else _lib.PFB_F64
        rc = lib.pfb_wgrid_plan_create(code, geom['nx'], geom['ny'], geom['px'], geom['py'], geom['cx'], geom['cy'],
                                       geom['W'], geom['nplanes'], geom['w0'], geom['dw'], C.byref(self.h))
        assert rc == self.ok

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.lib.pfb_wgrid_plan_destroy(self.h)

    def call(self, name, *args):
        args = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
        return getattr(self.lib, 'pfb_wgrid_' + name)(self.h, *args, torch.cuda.current_stream().cuda_stream)

    def run(self, name, *args):
        assert self.call(name, *args) == self.ok


def host(t):
    a = t.cpu().numpy()
    return a.astype(np.complex128 if np.iscomplexobj(a) else np.float64)


def full(shape, value, dtype):
    return torch.full(shape, value, dtype=dtype, device='cuda')


def rounded(a, dtype):
    """numpy complex128 / float64 values rounded to the data type (what the device is handed)."""
    if np.iscomplexobj(a):
        return a.astype(NP_C[dtype]).astype(np.complex128)
    return a.astype(NP_R[dtype]).astype(np.float64)


def figure(got, ref, S):
    """max over elements and components of |got - ref| / S; exact where S is zero."""
    worst = 0.0
    got, ref, S = (np.asarray(a, dtype=np.complex128) for a in (got, ref, S))
    assert np.isfinite(got.real).all() and np.isfinite(got.imag).all()
    for d, s in ((np.abs(got.real - ref.real), S.real), (np.abs(got.imag - ref.imag), S.imag)):
        on = s > 0
        assert not d[~on].any(), "a value with no contribution is not exactly zero"
        if on.any():
            worst = max(worst, float((d[on] / s[on]).max()))
    return worst


def check(name, dtype, got, ref, S, what='', k=None):
    r = figure(got, ref, S) / kc.U[dtype]
    _worst[name, dtype] = max(_worst.get((name, dtype), 0.0), r)
    if k == 0:                                            # plane 0 is the data of test_gpu_wgrid_kernels.py
        _worst[name + ' (plane 0)', dtype] = max(_worst.get((name + ' (plane 0)', dtype), 0.0), r)
    assert r <= kc.TOLERANCE_C[name][dtype], (name, dtype, what, r)


@pmp('entry', kc.FOOT, ids=kc.FOOT_IDS)
def test_grid_multi(lib, entry):
    geom, n, s0, s1 = entry['geom'], entry['n'], entry['s0'], entry['s1']
    dtype = geom['dtype']
    coord, val, _ = kc.foot_data(entry)
    vals = [rounded(plane_of(val, k, FACT_C), dtype) for k in range(MAXP)]
    poisoned = np.full((MAXP, n), NAN + 1j * NAN)
    for k in range(MAXP):
        poisoned[k, s0:s1] = vals[k][s0:s1]                         # nothing outside [s0, s1) may be read
    coord_d = dev(coord)
    with Plan(lib, geom) as plan:
        for plane in entry['planes']:
            fp = kc.footprint(geom, coord, plane, s0, s1)
            refs = [kc.ref_grid_plane(geom, coord, vals[k], plane, s0, s1, fp) for k in range(MAXP)]
            for nprod in range(1, MAXP + 1):
                grid = full((nprod, geom['Nu'], geom['Nv']), NAN, CDT[dtype])          # "every grid = 0, then"
                plan.run('grid_multi', nprod, plane, dev(poisoned[:nprod], CDT[dtype]), coord_d, n, s0, s1, grid)
                got = host(grid)
                for k in range(nprod):
                    check('grid', dtype, got[k], *refs[k], f"{entry['id']} plane {plane} product {k} of {nprod}", k)


@pmp('entry', kc.FOOT, ids=kc.FOOT_IDS)
def test_degrid_multi(lib, entry):
    geom, n, s0, s1 = entry['geom'], entry['n'], entry['s0'], entry['s1']
    dtype = geom['dtype']
    coord, _, grid = kc.foot_data(entry)
    grids = [rounded(plane_of(grid, k, FACT_C), dtype) for k in range(MAXP)]
    grids_d, coord_d = dev(np.stack(grids), CDT[dtype]), dev(coord)
    inside = np.zeros(n, bool)
    inside[s0:s1] = True
    with Plan(lib, geom) as plan:
        for plane in entry['planes']:
            fp = kc.footprint(geom, coord, plane, s0, s1)
            refs = [kc.ref_degrid_plane(geom, coord, grids[k], plane, s0, s1, fp) for k in range(MAXP)]
            reached = fp['ww'] != 0
            for nprod in range(1, MAXP + 1):
                acc = full((nprod, n), SENTINEL, CDT[dtype])
                plan.run('degrid_multi', nprod, plane, grids_d, coord_d, n, s0, s1, acc)
                got = acc.cpu().numpy().astype(np.complex128)
                for k in range(nprod):
                    ref, S = refs[k]
                    assert (got[k][~inside] == SENTINEL).all()
                    check('degrid', dtype, got[k][inside], SENTINEL + ref[inside], SENTINEL + S[inside],
                          f"{entry['id']} plane {plane} product {k} of {nprod}", k)
                    assert (got[k][inside][~reached] == SENTINEL).all()       # a slot that does not reach the plane


@pmp('entry', kc.SLOT, ids=kc.SLOT_IDS)
def test_slot_kernels_multi(lib, entry):
    d = kc.slot_data(entry)
    geom, dtype, idx, coord, nvis = d['geom'], entry['dtype'], d['idx'], d['coord'], d['nvis']
    ns = idx.size
    vis = [rounded(plane_of(d['vis'], k, FACT_C), dtype) for k in range(MAXP)]
    acc = [rounded(plane_of(d['acc'], k, FACT_C), dtype) for k in range(MAXP)]
    modes = ('none',) if d['wgt'] is None else ('per', 'shared')
    wgt = {'none': [None] * MAXP, 'shared': [None if d['wgt'] is None else rounded(d['wgt'], dtype)] * MAXP,
           'per': [None if d['wgt'] is None else rounded(weight_plane(d['wgt'], k), dtype) for k in range(MAXP)]}
    idx_d, coord_d = dev(idx), dev(coord)
    off = np.ones(nvis, bool)
    off[idx] = False
    with Plan(lib, geom) as plan:
        for mode in modes:
            for nprod in range(1, MAXP + 1):
                w = None if mode == 'none' else wgt['shared'][0] if mode == 'shared' else np.stack(wgt['per'][:nprod])
                w_d, shared = dev(w, RDT[dtype]), int(mode == 'shared')
                val = full((nprod, ns), NAN, CDT[dtype])
                plan.run('prep_multi', nprod, dev(np.stack(vis[:nprod]), CDT[dtype]), w_d, shared, idx_d, coord_d, ns,
                         nvis, val)
                out = full((nprod, nvis), NAN, CDT[dtype])                       # "vis = 0, then"
                plan.run('finish_multi', nprod, dev(np.stack(acc[:nprod]), CDT[dtype]), w_d, shared, idx_d, coord_d,
                         ns, out, nvis)
                got_val, got_out = host(val), host(out)
                for k in range(nprod):
                    what = f"{entry['id']} {mode} product {k} of {nprod}"
                    check('prep', dtype, got_val[k], *kc.ref_prep(geom, vis[k], wgt[mode][k], idx, coord), what, k)
                    assert not got_out[k][off].any()
                    check('finish', dtype, got_out[k], *kc.ref_finish(geom, acc[k], wgt[mode][k], idx, coord, nvis), what, k)


@pmp('entry', kc.IMAGE, ids=kc.IMAGE_IDS)
def test_image_kernels_multi(lib, entry):
    geom, plane = entry['geom'], entry['plane']
    dtype, nx, ny = geom['dtype'], geom['nx'], geom['ny']
    d = kc.image_data(entry)
    dirty = [rounded(plane_of(d['dirty'], k, FACT_R), dtype) for k in range(MAXP)]
    grid = [rounded(plane_of(d['grid'], k, FACT_C), dtype) for k in range(MAXP)]
    img = [rounded(plane_of(d['img'], k, FACT_C), dtype) for k in range(MAXP)]
    beam = None if d['beam'] is None else rounded(d['beam'], dtype)
    corr, nm1 = d['corr'], d['nm1']
    corr_d, nm1_d, beam_d = dev(corr), dev(nm1), dev(beam, RDT[dtype])
    window = np.zeros((geom['Nu'], geom['Nv']), bool)
    window[kc._window(geom)] = True
    with Plan(lib, geom) as plan:
        for nprod in range(1, MAXP + 1):
            out = full((nprod, geom['Nu'], geom['Nv']), NAN, CDT[dtype])            # "every grid = 0, then"
            plan.run('image_forward_multi', nprod, plane, dev(np.stack(dirty[:nprod]), RDT[dtype]), beam_d, corr_d,
                     nm1_d, out)
            acc = dev(np.stack(img[:nprod]), CDT[dtype])
            plan.run('image_adjoint_multi', nprod, plane, dev(np.stack(grid[:nprod]), CDT[dtype]), nm1_d, acc)
            res = full((nprod, nx, ny), NAN, RDT[dtype])
            plan.run('image_correct_multi', nprod, dev(np.stack(img[:nprod]), CDT[dtype]), corr_d, beam_d, res)
            got_f, got_a, got_c = host(out), host(acc), host(res)
            for k in range(nprod):
                what = f"{entry['id']} product {k} of {nprod}"
                assert not got_f[k][~window].any()                               # exact zeros outside the window
                check('image_forward', dtype, got_f[k], *kc.ref_image_forward(geom, dirty[k], beam, corr, nm1, plane), what, k)
                check('image_adjoint', dtype, got_a[k], *kc.ref_image_adjoint(geom, grid[k], nm1, plane, img[k]), what, k)
                check('image_correct', dtype, got_c[k], *kc.ref_image_correct(img[k], corr, beam), what, k)


def test_native_multi_entry_points_refuse(lib):
    """nprod outside 1 .. 4 is PFB_ERR_INVALID at every multi entry point, the pointers real all the same, and nothing
    is written; so is a null array."""
    from pfb_clean_amd import _lib
    INV = _lib.PFB_ERR_INVALID
    geom = kc.geometry('f64', 6, 8, 4)
    n, nvis = 5, 9
    cz = lambda *shape: full(shape, SENTINEL, torch.complex128)        # noqa: E731
    rz = lambda *shape: full(shape, SENTINEL, torch.float64)           # noqa: E731
    idx, coord = dev(np.arange(n, dtype=np.int32)), dev(np.zeros((3, n)))
    vis, val, grid, img, dirty, corr = cz(4, nvis), cz(4, n), cz(4, 12, 16), cz(4, 6, 8), rz(4, 6, 8), rz(6, 8)
    with Plan(lib, geom) as plan:
        for nprod in (0, 5, -1):
            calls = [('prep_multi', nprod, vis, None, 0, idx, coord, n, nvis, val),
                     ('finish_multi', nprod, val, None, 0, idx, coord, n, vis, nvis),
                     ('grid_multi', nprod, 0, val, coord, n, 0, n, grid),
                     ('degrid_multi', nprod, 0, grid, coord, n, 0, n, val),
                     ('image_forward_multi', nprod, 0, dirty, None, corr, None, grid),
                     ('image_adjoint_multi', nprod, 0, grid, None, img),
                     ('image_correct_multi', nprod, img, corr, None, dirty)]
            for name, *args in calls:
                assert plan.call(name, *args) == INV, (name, nprod)
        assert plan.call('grid_multi', 2, 0, None, coord, n, 0, n, grid) == INV
        assert plan.call('prep_multi', 2, vis, None, 0, idx, coord, n, n - 1, val) == INV       # nvis < nsorted
        torch.cuda.synchronize()
        for t in (vis, val, grid, img, dirty):
            assert (t == SENTINEL).all()


def test_zz_report():
    """The worst figures of this run (run with -s to read them)."""
    for (name, dtype), r in sorted(_worst.items()):
        print(f"recorded {name:24s} {dtype}: {r:10.3f}   C = {kc.TOLERANCE_C[name.split(' ')[0]][dtype]:g}")
