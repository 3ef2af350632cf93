"""
Several Stokes products in one pass on the MI355X (k_stokes_multi of csrc/stokes.hip through
pfb_clean_amd.utils.stokes.stokes_vis and pfb_clean_amd.utils.weighting.weight_data with a multi-letter `product`),
in fp32 and fp64.

Plane k of vis and wgt is held to what the single call of its letter is held to in test_gpu_stokes.py, at the same
per-element bounds (tests/stokes_cases.py: sc.worst <= sc.K): against the reference's golden output of that product's
case where tests/golden/stokes.npz has one (the sweep-, noj- and each sv- case's own product), else against
sc.closed_form of the case with that product (test_cpu_stokes_cases.py holds the closed form to the reference).  The mask
does not depend on the product and is exactly the golden's; wsum[k] is within sc.wsum_bound of math.fsum of plane k's
unflagged reference weights.  A swapped or repeated plane is far outside the bounds: the products of one input set
differ by the size of the data.
"""
import math

import numpy as np
import pytest
import torch

import stokes_cases as sc

pytestmark = pytest.mark.gpu

TAGS = ('f32', 'f64')
SETS, CASES = sc.load()
POLS = ('linear', 'circular')


def ids(cases):
    return [c['name'] for c in cases]


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def wd_args(case, tag, **over):
    """The arguments of weight_data for a 'wd' case, in the type under test."""
    s = case['set']
    args = dict(data=sc.corr_arg(case, s['data']).astype(sc.CDT[tag]),
                weight=sc.corr_arg(case, s['weight']).astype(sc.RDT[tag]), flag=s['flag'],
                jones=sc.jones_arg(case).astype(sc.CDT[tag]), tbin_idx=s['tbin_idx'], tbin_counts=s['tbin_counts'],
                ant1=s['ant1'], ant2=s['ant2'], pol=case['pol'], product=case['product'], nc=str(sc.ncorr(case['mode'])))
    args.update(over)
    return args


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


_forms = {}


def form(case, product=None):
    """sc.closed_form of the case with `product` (its own by default), computed once."""
    product = product or case['product']
    key = (case['name'], product)
    if key not in _forms:
        _forms[key] = sc.closed_form(dict(case, product=product))
    return _forms[key]


def reference(case, product):
    """(ref_vis, ref_wgt, vis_unit, wgt_unit) of `product` on the case's inputs: the golden of the case that differs in
    the product alone where the fixture holds it, else the closed form."""
    f = form(case, product)
    if product == case['product']:
        return case['ref_vis'], case['ref_wgt'], f[3], f[4]
    name = case['name'].rsplit('-', 1)[0] + '-' + product
    if case['name'].startswith(('sweep-', 'noj-')):
        twin = sc.case_named(name)
        assert twin['set'] is case['set'] and (twin['mode'], twin['pol']) == (case['mode'], case['pol'])
        return twin['ref_vis'], twin['ref_wgt'], f[3], f[4]
    return f[0], f[1], f[3], f[4]


def check_planes(case, letters, vis, wgt, tag, what=''):
    """Plane k of vis and wgt against the reference of letters[k] at the per-element bounds."""
    shape = case['set']['data'].shape[:2]
    assert vis.dtype == sc.CDT[tag] and wgt.dtype == sc.RDT[tag]
    assert vis.shape == wgt.shape == (len(letters),) + shape
    worst = (0.0, 0.0)
    for k, p in enumerate(letters):
        ref_vis, ref_wgt, vis_unit, wgt_unit = reference(case, p)
        ev, ew = sc.worst(vis[k], wgt[k], ref_vis, ref_wgt, vis_unit, wgt_unit, tag)
        assert ev <= sc.K and ew <= sc.K, (case['name'], what, p, ev, ew)
        worst = (max(worst[0], ev), max(worst[1], ew))
    print(f"{case['name']} {tag} {''.join(letters)} {what}: vis {worst[0]:.2f}, wgt {worst[1]:.2f} of the K = 1 bound")


def check_wsum(case, letters, wsum, tag):
    assert wsum.shape == (len(letters),) and wsum.dtype == sc.RDT[tag]
    live = form(case)[2] != 0
    for k, p in enumerate(letters):
        golden = reference(case, p)[1][live]
        assert abs(float(wsum[k]) - math.fsum(golden)) <= sc.wsum_bound(golden, tag), (case['name'], p)


def run_wd(case, tag, product, **over):
    from pfb_clean_amd.utils.weighting import weight_data
    out = weight_data(**wd_args(case, tag, product=product, **over))
    assert set(out) == {'vis', 'wgt'} and all(isinstance(v, np.ndarray) for v in out.values())
    return out['vis'], out['wgt']


# ---------------------------------------------------------------------------------------------------------- goldens
@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('pol', POLS)
@pytest.mark.parametrize('mode', sc.MODES)
def test_sweep_goldens_through_weight_data(mode, pol, tag):
    case = sc.case_named(f'sweep-{mode}-{pol}-I')
    check_planes(case, 'IQUV', *run_wd(case, tag, 'IQUV'), tag)


@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('pol', POLS)
@pytest.mark.parametrize('mode', ('noj4', 'noj2'))
def test_no_jones_goldens_through_stokes_vis(mode, pol, tag):
    from pfb_clean_amd.utils.stokes import stokes_vis
    case = sc.case_named(f'noj-{mode}-{pol}-I')
    vis, wgt, mask, wsum = stokes_vis(**sv_args(case, tag, product='IQUV'))
    assert all(isinstance(a, np.ndarray) for a in (vis, wgt, mask, wsum))
    check_planes(case, 'IQUV', vis, wgt, tag)
    assert mask.dtype == np.uint8 and mask.shape == case['ref_mask'].shape and np.array_equal(mask, case['ref_mask'])
    check_wsum(case, 'IQUV', wsum, tag)


# ---------------------------------------------------------------------------------------------------------- options
@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('case', sc.cases_of('sv', 'sv-'), ids=ids(sc.cases_of('sv', 'sv-')))
def test_every_option_with_four_products(case, tag):
    """Second column, weight forms, flags and row flags: the case's own product against its golden, the other three
    against the closed form."""
    from pfb_clean_amd.utils.stokes import stokes_vis
    vis, wgt, mask, wsum = stokes_vis(**sv_args(case, tag, product='IQUV'))
    check_planes(case, 'IQUV', vis, wgt, tag)
    assert mask.dtype == np.uint8 and np.array_equal(mask, case['ref_mask'])
    check_wsum(case, 'IQUV', wsum, tag)


# ------------------------------------------------------------------------------------------------------ shape edges
@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('case', sc.cases_of('wd', 'shape-'), ids=ids(sc.cases_of('wd', 'shape-')))
def test_shape_edges(case, tag):
    assert case['set']['data'].shape[:2] in sc.SHAPES
    check_planes(case, 'IQUV', *run_wd(case, tag, 'IQUV'), tag)


def test_every_shape_is_covered():
    assert {c['set']['data'].shape[:2] for c in sc.cases_of('wd', 'shape-')} == set(sc.SHAPES)


@pytest.mark.parametrize('tag', TAGS)
def test_more_row_groups_than_workgroups(tag):
    """129 channels: one row per workgroup; 4100 rows: more groups than the workgroups of the launch, which stride over
    them, four partial sums each.  Against the closed form in fp64."""
    from pfb_clean_amd.utils.stokes import stokes_vis
    rng = np.random.default_rng(77)
    nrow, nchan, nant, ntime = 4100, 129, 4, 3
    assert sc.rows_per_group(nchan) == 1

    def f32(a):
        return a.astype(np.complex64 if np.iscomplexobj(a) else np.float32)
    counts = np.array([1400, 1400, 1300])
    shape = (ntime, nchan, nant, 1, 2)
    jones = rng.uniform(0.5, 2.0, shape) * np.exp(2j * np.pi * rng.uniform(size=shape))
    jfull = np.zeros((ntime, nchan, nant, 1, 4), complex)
    jfull[..., 0], jfull[..., 3] = jones[..., 0], jones[..., 1]
    ant1 = rng.integers(0, nant - 1, nrow).astype(np.int32)
    s = dict(data=f32(rng.standard_normal((nrow, nchan, 4)) + 1j * rng.standard_normal((nrow, nchan, 4))).astype(complex),
             weight=f32(rng.uniform(0.5, 2.0, (nrow, nchan, 4))).astype(float),
             flag=np.zeros((nrow, nchan), bool), flag3=rng.uniform(size=(nrow, nchan, 4)) < 0.05, ant1=ant1,
             ant2=(ant1 + 1).astype(np.int32), tbin_idx=np.array([0, 1400, 2800]), tbin_counts=counts,
             jones=f32(jfull).astype(complex), layout='qcal')
    case = dict(name='groups', kind='sv', set=s, mode='diag4', pol='linear', product='I', wform='spectrum', op='none',
                use_flag=True, use_frow=False)
    vis, wgt, mask, wsum = stokes_vis(**sv_args(case, tag, product='IQUV'))
    assert vis.shape == wgt.shape == (4, nrow, nchan) and wsum.shape == (4,)
    for k, p in enumerate('IQUV'):
        ref_vis, ref_wgt, ref_mask, vis_unit, wgt_unit = sc.closed_form(dict(case, product=p))
        ev, ew = sc.worst(vis[k], wgt[k], ref_vis, ref_wgt, vis_unit, wgt_unit, tag)
        print(f"groups {tag} {p}: vis {ev:.2f}, wgt {ew:.2f} of the K = 1 bound")
        assert ev <= sc.K and ew <= sc.K and np.array_equal(mask, ref_mask)
        live = ref_wgt[ref_mask != 0]
        assert abs(float(wsum[k]) - math.fsum(live)) <= sc.wsum_bound(live, tag)


# ------------------------------------------------------------------------------------------------ order and subsets
@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('product', ['VI', 'QU', ('U', 'I', 'Q'), 'UVQI', ['V']], ids=str)
def test_planes_come_in_the_order_asked(product, tag):
    from pfb_clean_amd.utils.stokes import stokes_vis
    letters = tuple(product)
    for name in ('sweep-full4-linear-I', 'sweep-diag4-circular-I', 'sweep-diag2-linear-I'):
        case = sc.case_named(name)
        check_planes(case, letters, *run_wd(case, tag, product), tag)
    case = sc.case_named('noj-noj4-circular-I')
    vis, wgt, mask, wsum = stokes_vis(**sv_args(case, tag, product=product))
    check_planes(case, letters, vis, wgt, tag)
    check_wsum(case, letters, wsum, tag)
    assert np.array_equal(mask, case['ref_mask'])


def test_a_swapped_plane_is_far_outside():
    """What the order test can tell: plane k held against another letter's golden misses the bound by orders."""
    case = sc.case_named('sweep-full4-linear-I')
    vis, wgt = run_wd(case, 'f64', 'IQUV')
    for k, p in enumerate('IQUV'):
        other = 'IQUV'[(k + 1) % 4]
        ref_vis, ref_wgt, vis_unit, wgt_unit = reference(case, other)
        ev, ew = sc.worst(vis[k], wgt[k], ref_vis, ref_wgt, vis_unit, wgt_unit, 'f64')
        assert ev > 1e6 * sc.K, (p, other, ev)


def test_value_errors_and_single_letters():
    from pfb_clean_amd.utils.stokes import stokes_vis
    from pfb_clean_amd.utils.weighting import weight_data
    case = sc.case_named('sweep-full4-linear-I')
    sv = sc.case_named('sv-spectrum-minus-full')
    for bad in ('II', 'IX', '', 'IQUVI', ('I', 'I'), ('IQ', 'U'), ()):
        with pytest.raises(ValueError):
            weight_data(**wd_args(case, 'f64', product=bad))
        with pytest.raises(ValueError):
            stokes_vis(**sv_args(sv, 'f64', product=bad))
    # a single letter: the 2-D arrays of always
    out = weight_data(**wd_args(case, 'f64'))
    assert out['vis'].shape == out['wgt'].shape == case['ref_vis'].shape and out['vis'].ndim == 2
    vis, wgt, mask, wsum = stokes_vis(**sv_args(sv, 'f64'))
    assert vis.shape == wgt.shape == mask.shape == sv['ref_vis'].shape and wsum.shape == (1,)
    # and the same numbers as its plane of a stacked call, to the bound of both
    stack = weight_data(**wd_args(case, 'f64', product='QI'))
    check_planes(case, 'I', out['vis'][None], out['wgt'][None], 'f64')
    check_planes(case, 'QI', stack['vis'], stack['wgt'], 'f64')


# ------------------------------------------------------------------------------------------------- flags and data
@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('mode', sc.MODES)
def test_nan_and_inf_in_flagged_data_stay_out(mode, tag):
    case = sc.case_named(f'sweep-{mode}-linear-I')
    a = wd_args(case, tag)
    flag = a['flag'].astype(bool)
    assert flag.any()
    data, weight = a['data'].copy(), a['weight'].copy()
    rows, chans = np.nonzero(flag)
    for k, (r, c) in enumerate(zip(rows, chans)):
        data[r, c, k % data.shape[2]] = (np.nan, np.inf, complex(-np.inf, np.nan))[k % 3]
        weight[r, c, (k + 1) % data.shape[2]] = (np.inf, np.nan, -np.inf)[k % 3]
    vis, wgt = run_wd(case, tag, 'IQUV', data=data, weight=weight)
    assert np.isfinite(vis).all() and np.isfinite(wgt).all()
    assert not vis[:, flag].any() and not wgt[:, flag].any()
    check_planes(case, 'IQUV', vis, wgt, tag)


@pytest.mark.parametrize('tag', TAGS)
def test_everything_flagged(tag):
    from pfb_clean_amd.utils.stokes import stokes_vis
    case = sc.case_named('sv-spectrum-minus-full')
    shape = sc.corr_arg(case, case['set']['flag3']).shape
    for over in (dict(flag=np.ones(shape, bool)), dict(frow=np.ones(shape[0], bool))):
        vis, wgt, mask, wsum = stokes_vis(**sv_args(case, tag, product='IQUV', **over))
        assert vis.shape == (4,) + shape[:2] and not vis.any() and not wgt.any() and not mask.any()
        assert wsum.shape == (4,) and wsum.dtype == sc.RDT[tag] and not wsum.any()


def test_tensors_in_tensors_out():
    from pfb_clean_amd.utils.stokes import stokes_vis
    case = sc.case_named('sv-row-full')
    a = sv_args(case, 'f32', product='UQ')
    t = {k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in a.items()}
    got = stokes_vis(**t)
    assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in got)
    want = stokes_vis(**a)
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))          # no atomics: the same bits


# ------------------------------------------------------------------------------------------------------- the C ABI
def test_c_abi_refusals():
    """pfb_stokes_vis_multi itself: the smallest good call answers PFB_OK and stokes_vis's planes and sums; with one
    argument changed at a time it answers the status below before any launch -- the pointers real all the same -- and
    writes nothing."""
    import ctypes as C
    from pfb_clean_amd import _lib
    from pfb_clean_amd.utils import stokes as st
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    INV, UNS = _lib.PFB_ERR_INVALID, _lib.PFB_ERR_UNSUPPORTED
    nrow, nchan, nc, nprod = 2, 2, 2, 2
    data = dev(np.arange(1, 1 + 2 * nrow * nchan * nc, dtype=np.float64).view(np.complex128).reshape(nrow, nchan, nc))
    ti, tcnt = dev(np.array([0], dtype=np.int64)), dev(np.array([nrow], dtype=np.int64))
    a1, a2 = dev(np.array([0, 0], dtype=np.int32)), dev(np.array([1, 1], dtype=np.int32))
    vis = torch.empty((nprod, nrow, nchan), dtype=torch.complex128, device='cuda')
    wgt = torch.empty((nprod, nrow, nchan), dtype=torch.float64, device='cuda')
    mask = torch.empty((nrow, nchan), dtype=torch.uint8, device='cuda')
    wsum = torch.empty(nprod, dtype=torch.float64, device='cuda')
    work = torch.zeros(_lib.REDUCE_WS_DOUBLES, dtype=torch.float64, device='cuda')

    def ints(*v):
        return (C.c_int * len(v))(*v)
    names = ('dtype mode nprod basis data data2 subtract weight wform flag nflagcorr frow autocorr jones ndir ntime nant '
             'tbin_idx tbin_counts tbin_off ant1 ant2 nrow nchan vis wgt mask wsum work').split()
    good = dict(zip(names, [_lib.PFB_F64, st.NOJ2, nprod, ints(1, 0), data.data_ptr(), None, 0, None, st.W_NONE, None, 0,
                            None, 0, None, 1, 1, 2, ti.data_ptr(), tcnt.data_ptr(), 0, a1.data_ptr(), a2.data_ptr(), nrow,
                            nchan, vis.data_ptr(), wgt.data_ptr(), mask.data_ptr(), wsum.data_ptr(), work.data_ptr()]))
    assert len(good) == len(names) == 29

    def call(**over):
        return lib.pfb_stokes_vis_multi(*dict(good, **over).values(), stream)

    assert call() == _lib.PFB_OK
    want = st.stokes_vis(data, a1, a2, ti, tcnt, 'linear', 'QI', precision='double')
    assert torch.equal(vis, want[0]) and torch.equal(wgt, want[1]) and torch.equal(mask, want[2])
    assert torch.equal(wsum, want[3]) and float(wsum[1]) == nrow * nchan * float(want[1][1, 0, 0])
    # ... and its planes are the single entry point's, bit for bit
    for k, p in enumerate('QI'):
        one = st.stokes_vis(data, a1, a2, ti, tcnt, 'linear', p, precision='double')
        assert torch.equal(vis[k], one[0]) and torch.equal(wgt[k], one[1]) and float(wsum[k]) == float(one[3][0])

    vis.fill_(-7 - 7j), wgt.fill_(-7.0), mask.fill_(0xAB), wsum.fill_(-7.0)
    refused = [dict(nprod=0), dict(nprod=5), dict(nprod=-1), dict(basis=None), dict(basis=ints(0, 4)),
               dict(basis=ints(-1, 0)), dict(basis=ints(1, 1)), dict(nprod=3, basis=ints(2, 0, 2)),
               dict(dtype=2), dict(mode=-1), dict(mode=st.NOJ2 + 1), dict(wform=-1), dict(wform=st.W_ROW + 1),
               dict(nflagcorr=3)]
    refused += [{name: None} for name in ('data', 'tbin_idx', 'tbin_counts', 'ant1', 'ant2', 'vis', 'wgt', 'mask', 'wsum',
                                          'work')]
    refused += [dict(wform=st.W_SPECTRUM), dict(mode=st.DIAG2)]          # weight / jones null where they are read
    refused += [{name: good[name] + off} for name, off in (('data', 8), ('vis', 8), ('wgt', 4), ('wsum', 4), ('ant1', 2),
                                                          ('tbin_idx', 4))]
    refused += [dict(ntime=0), dict(nant=0), dict(ndir=0)]
    for over in refused:
        assert call(**over) == INV, over
    for over in (dict(nrow=0), dict(nchan=0)):
        assert call(**over) == UNS, over
    torch.cuda.synchronize()
    assert (vis == -7 - 7j).all() and (wgt == -7.0).all() and (mask == 0xAB).all() and (wsum == -7.0).all()
