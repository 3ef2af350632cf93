"""
Stokes visibilities and weights on the MI355X (csrc/stokes.hip through pfb_clean_amd.utils.weighting.weight_data and
pfb_clean_amd.utils.stokes.stokes_vis) against the reference's fp64 results of tests/golden/stokes.npz, in fp32 and fp64.

Bounds (tests/stokes_cases.py states them and where K = 16 comes from), per element:
    |vis - ref| <= K eps kp kq 1/2 sum_ab |B_ab| (|adj Gp| |V| |adj Gq|^T)_ab / |det Gp det Gq|
    |wgt - ref| <= K eps sum_ab w_ab ((|Gp| |B| |Gq|^T)_ab)^2
    mask        exactly the reference's (~flag).astype(uint8)
    wsum        within K eps sum wgt + the fp64 summation term of math.fsum of the golden weights
A flagged visibility and a row that no time bin covers are exact zeros.  The inputs are fp32 values, so that both types
see arithmetic error only.
"""
import math

import numpy as np
import pytest
import torch

import stokes_cases as sc
import wgrid_cases as wc

pytestmark = pytest.mark.gpu

TAGS = ('f32', 'f64')
SETS, CASES = sc.load()


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


_units = {}


def check(case, vis, wgt, tag):
    """vis and wgt against the case's golden outputs at the per-element bounds; returns the figures."""
    if case['name'] not in _units:
        _units[case['name']] = sc.closed_form(case)[3:]
    vis_unit, wgt_unit = _units[case['name']]
    assert vis.dtype == sc.CDT[tag] and wgt.dtype == sc.RDT[tag]
    assert vis.shape == case['ref_vis'].shape and wgt.shape == case['ref_wgt'].shape
    ev, ew = sc.worst(vis, wgt, case['ref_vis'], case['ref_wgt'], vis_unit, wgt_unit, tag)
    print(f"{case['name']} {tag}: vis {ev:.2f}, wgt {ew:.2f} of the K = 1 bound")
    assert ev <= sc.K and ew <= sc.K, (ev, ew)
    return ev, ew


def run_wd(case, tag, **over):
    from pfb_clean_amd.utils.weighting import weight_data
    out = weight_data(**wd_args(case, tag, **over))
    assert set(out) == {'vis', 'wgt'} and all(isinstance(v, np.ndarray) for v in out.values())
    return out['vis'], out['wgt']


# ------------------------------------------------------------------------------------------------- weight_data
@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('case', sc.cases_of('wd', 'sweep-'), ids=ids(sc.cases_of('wd', 'sweep-')))
def test_all_variants(case, tag):
    check(case, *run_wd(case, tag), tag)


@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('case', sc.cases_of('wd', 'shape-'), ids=ids(sc.cases_of('wd', 'shape-')))
def test_shape_edges(case, tag):
    check(case, *run_wd(case, tag), tag)


@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('case', sc.cases_of('wd', 'tbin-'), ids=ids(sc.cases_of('wd', 'tbin-')))
def test_time_bin_edges(case, tag):
    from pfb_clean_amd.utils.weighting import _weight_data
    s = case['set']
    keep = s['tbin_idx'].copy()
    vis, wgt = run_wd(case, tag)
    assert np.array_equal(s['tbin_idx'], keep)                      # the reference subtracts the minimum in place
    check(case, vis, wgt, tag)
    dead = sc.row_bins(vis.shape[0], s['tbin_idx'], s['tbin_counts']) < 0
    assert not vis[dead].any() and not wgt[dead].any()
    if case['name'] == 'tbin-gaps':
        assert dead[0] and dead[-1]
    # tensors in, tensors out, the bins as a device tensor: unchanged as well, and the same bits
    a = wd_args(case, tag)
    t = {k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in a.items()}
    tv, tw = _weight_data(*(t[k] for k in ('data', 'weight', 'flag', 'jones', 'tbin_idx', 'tbin_counts', 'ant1', 'ant2',
                                           'pol', 'product', 'nc')))
    assert isinstance(tv, torch.Tensor) and tv.is_cuda and isinstance(tw, torch.Tensor) and tw.is_cuda
    assert np.array_equal(t['tbin_idx'].cpu().numpy(), keep)
    assert np.array_equal(tv.cpu().numpy(), vis) and np.array_equal(tw.cpu().numpy(), wgt)


@pytest.mark.parametrize('tag', TAGS)
def test_more_row_groups_than_workgroups(tag):
    """129 channels: one row per workgroup; 4100 rows: more groups than the 4096 workgroups of the launch, which stride
    over them.  Against the closed form in fp64 (test_cpu_stokes_cases.py holds it to the reference)."""
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
    ref_vis, ref_wgt, ref_mask, vis_unit, wgt_unit = sc.closed_form(case)
    vis, wgt, mask, wsum = stokes_vis(**sv_args(case, tag))
    ev, ew = sc.worst(vis, wgt, ref_vis, ref_wgt, vis_unit, wgt_unit, tag)
    print(f"groups {tag}: vis {ev:.2f}, wgt {ew:.2f} of the K = 1 bound")
    assert ev <= sc.K and ew <= sc.K and np.array_equal(mask, ref_mask)
    assert abs(float(wsum[0]) - math.fsum(ref_wgt[ref_mask != 0])) <= sc.wsum_bound(ref_wgt[ref_mask != 0], tag)


def test_indices_past_two_to_the_31():
    """nrow nchan ncorr > 2^31, as on real chunks: (2^20 + 1) rows x 512 channels x 4 correlations of complex64 (17 GB)
    without Jones terms, weights or flags, Stokes I: vis = (v00 + v11) / 2 -- one add, one exact halving, the same bits
    as torch's -- wgt = 2, mask = 1 and their sum exactly, on every visibility up to the last."""
    from pfb_clean_amd.utils.stokes import stokes_vis
    nrow, nchan = (1 << 20) + 1, 512
    assert nrow * nchan * 4 > 1 << 31
    data = torch.view_as_complex(torch.randn((nrow, nchan, 4, 2), dtype=torch.float32, device='cuda'))
    ant1 = torch.zeros(nrow, dtype=torch.int32, device='cuda')
    vis, wgt, mask, wsum = stokes_vis(data, ant1, ant1 + 1, np.array([0]), np.array([nrow]), 'linear', 'I')
    assert torch.equal(vis, (data[..., 0] + data[..., 3]) * 0.5)
    assert bool((wgt == 2).all()) and bool((mask == 1).all())
    assert wsum.dtype == torch.float32 and float(wsum[0]) == 2.0 * nrow * nchan
    del data, vis, wgt, mask
    torch.cuda.empty_cache()


# --------------------------------------------------------------------------------------------- flags and data
@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('mode', sc.MODES)
def test_nan_and_inf_in_flagged_data_stay_out(mode, tag):
    case = sc.case_named(f'sweep-{mode}-linear-V' if mode != 'diag2' else 'sweep-diag2-linear-Q')
    a = wd_args(case, tag)
    flag = a['flag'].astype(bool)
    assert flag.any()
    data, weight = a['data'].copy(), a['weight'].copy()
    rows, chans = np.nonzero(flag)
    for k, (r, c) in enumerate(zip(rows, chans)):
        data[r, c, k % data.shape[2]] = (np.nan, np.inf, complex(-np.inf, np.nan))[k % 3]
        weight[r, c, (k + 1) % data.shape[2]] = (np.inf, np.nan, -np.inf)[k % 3]
    vis, wgt = run_wd(case, tag, data=data, weight=weight)
    assert np.isfinite(vis).all() and np.isfinite(wgt).all()
    assert not vis[flag].any() and not wgt[flag].any()
    check(case, vis, wgt, tag)


@pytest.mark.parametrize('tag', TAGS)
def test_everything_flagged(tag):
    from pfb_clean_amd.utils.stokes import stokes_vis
    case = sc.case_named('sv-spectrum-minus-full')
    shape = sc.corr_arg(case, case['set']['flag3']).shape
    for over in (dict(flag=np.ones(shape, bool)), dict(frow=np.ones(shape[0], bool))):
        vis, wgt, mask, wsum = stokes_vis(**sv_args(case, tag, **over))
        assert not vis.any() and not wgt.any() and not mask.any()
        assert wsum.shape == (1,) and wsum.dtype == sc.RDT[tag] and wsum[0] == 0
    a = wd_args(sc.case_named('sweep-full4-linear-I'), tag)
    from pfb_clean_amd.utils.weighting import weight_data
    out = weight_data(**dict(a, flag=np.ones(a['flag'].shape, bool)))
    assert not out['vis'].any() and not out['wgt'].any()


@pytest.mark.parametrize('tag', TAGS)
def test_autocorrelations_come_out_flagged(tag):
    from pfb_clean_amd.utils.stokes import stokes_vis
    case = sc.case_named('sv-plain')                        # no flag, no frow: the autocorrelations alone
    s = case['set']
    auto = s['ant1'] == s['ant2']
    assert auto.any() and not auto.all()
    vis, wgt, mask, wsum = stokes_vis(**sv_args(case, tag))
    assert not mask[auto].any() and mask[~auto].all()
    assert not vis[auto].any() and not wgt[auto].any() and wgt[~auto].all()
    # weight_data takes the flag as it is given, as the reference's does
    wd = sc.case_named('sweep-diag4-linear-I')
    a = wd_args(wd, tag, ant2=wd['set']['ant1'], flag=np.zeros(wd['set']['flag'].shape, bool))
    from pfb_clean_amd.utils.weighting import weight_data
    assert weight_data(**a)['wgt'].all()


# -------------------------------------------------------------------------------------------------- stokes_vis
@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('case', sc.cases_of('sv'), ids=ids(sc.cases_of('sv')))
def test_stokes_vis(case, tag):
    from pfb_clean_amd.utils.stokes import stokes_vis
    vis, wgt, mask, wsum = stokes_vis(**sv_args(case, tag))
    assert all(isinstance(a, np.ndarray) for a in (vis, wgt, mask, wsum))
    check(case, vis, wgt, tag)
    assert mask.dtype == np.uint8 and np.array_equal(mask, case['ref_mask'])
    golden = case['ref_wgt'][case['ref_mask'] != 0]
    assert wsum.shape == (1,) and wsum.dtype == sc.RDT[tag]
    err = abs(float(wsum[0]) - math.fsum(golden))
    print(f"{case['name']} {tag}: wsum off by {err:.3e}, bound {sc.wsum_bound(golden, tag):.3e}")
    assert err <= sc.wsum_bound(golden, tag)


@pytest.mark.parametrize('tag', TAGS)
def test_stokes_vis_casts_the_other_precision(tag):
    """Data, weights and Jones terms handed over in the other type are cast once each: the same bits as handing them
    over in the type of `precision` (the inputs are fp32 values)."""
    from pfb_clean_amd.utils.stokes import stokes_vis
    case = sc.case_named('sv-spectrum-minus-full')
    other = 'f64' if tag == 'f32' else 'f32'
    want = stokes_vis(**sv_args(case, tag))
    a = sv_args(case, other, precision=sv_args(case, tag)['precision'])
    got = stokes_vis(**a)
    assert all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got, want))


def test_value_errors():
    from pfb_clean_amd.utils.stokes import stokes_vis
    from pfb_clean_amd.utils.weighting import weight_data
    case = sc.case_named('sweep-full4-linear-I')
    a = wd_args(case, 'f64')
    # bins that descend, bins that overlap
    for idx, counts in (([40, 0, 60, 70], [20, 40, 10, 15]), ([0, 20, 40, 60], [25, 20, 20, 25])):
        with pytest.raises(ValueError, match='ascending'):
            weight_data(**dict(a, tbin_idx=np.array(idx), tbin_counts=np.array(counts)))
    # an unknown pol, product, nc; an nc that is not the data's
    for over in (dict(pol='elliptic'), dict(product='X'), dict(nc='3'), dict(nc=1), dict(nc='2')):
        with pytest.raises(ValueError):
            weight_data(**dict(a, **over))
    # FULL Jones terms with two correlations
    two = dict(a, data=np.ascontiguousarray(a['data'][..., [0, 3]]), weight=np.ascontiguousarray(a['weight'][..., [0, 3]]),
               nc='2')
    with pytest.raises(ValueError, match='2 x 2'):
        weight_data(**two)
    sv = sc.case_named('sv-spectrum-minus-full')
    b = sv_args(sv, 'f64')
    with pytest.raises(ValueError, match='2 x 2'):
        stokes_vis(**dict(b, data=np.ascontiguousarray(b['data'][..., [0, 3]]), data2=None,
                          weight=np.ascontiguousarray(b['weight'][..., [0, 3]]), flag=None))
    with pytest.raises(ValueError):
        stokes_vis(**dict(b, poltype='elliptic'))
    with pytest.raises(ValueError):
        stokes_vis(**dict(b, operator='*'))
    with pytest.raises(ValueError, match='ascending'):
        stokes_vis(**dict(b, tbin_idx=b['tbin_idx'][::-1].copy()))
    # integers for nc are as good as strings
    check(case, *(weight_data(**dict(a, nc=4))[k] for k in ('vis', 'wgt')), 'f64')


def test_c_abi_refusals():
    """pfb_stokes_vis itself: the smallest good call answers PFB_OK and stokes_vis's sum; with one argument changed at a
    time it answers the status below before any launch -- the pointers real all the same -- and writes nothing."""
    from pfb_clean_amd import _lib
    from pfb_clean_amd.utils import stokes as st
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    INV, UNS = _lib.PFB_ERR_INVALID, _lib.PFB_ERR_UNSUPPORTED
    nrow, nchan, nc = 2, 2, 2
    data = dev(np.arange(1, 1 + 2 * nrow * nchan * nc, dtype=np.float64).view(np.complex128).reshape(nrow, nchan, nc))
    ti, tcnt = dev(np.array([0], dtype=np.int64)), dev(np.array([nrow], dtype=np.int64))
    a1, a2 = dev(np.array([0, 0], dtype=np.int32)), dev(np.array([1, 1], dtype=np.int32))
    vis = torch.empty((nrow, nchan), dtype=torch.complex128, device='cuda')
    wgt = torch.empty((nrow, nchan), dtype=torch.float64, device='cuda')
    mask = torch.empty((nrow, nchan), dtype=torch.uint8, device='cuda')
    wsum = torch.empty(1, dtype=torch.float64, device='cuda')
    work = torch.zeros(_lib.REDUCE_WS_DOUBLES, dtype=torch.float64, device='cuda')
    names = ('dtype mode basis data data2 subtract weight wform flag nflagcorr frow autocorr jones ndir ntime nant '
             'tbin_idx tbin_counts tbin_off ant1 ant2 nrow nchan vis wgt mask wsum work').split()
    good = dict(zip(names, [_lib.PFB_F64, st.NOJ2, 0, data.data_ptr(), None, 0, None, st.W_NONE, None, 0, None, 0, None,
                            1, 1, 2, ti.data_ptr(), tcnt.data_ptr(), 0, a1.data_ptr(), a2.data_ptr(), nrow, nchan,
                            vis.data_ptr(), wgt.data_ptr(), mask.data_ptr(), wsum.data_ptr(), work.data_ptr()]))
    assert len(good) == len(names) == 28

    def call(**over):
        return lib.pfb_stokes_vis(*dict(good, **over).values(), stream)

    assert call() == _lib.PFB_OK
    want = st.stokes_vis(data, a1, a2, ti, tcnt, 'linear', 'I', precision='double')
    assert float(wsum[0]) == float(want[3][0]) == nrow * nchan * float(want[1][0, 0])       # 4 x the one wgt value
    assert torch.equal(vis, want[0]) and torch.equal(wgt, want[1]) and torch.equal(mask, want[2])

    vis.fill_(-7 - 7j), wgt.fill_(-7.0), mask.fill_(0xAB), wsum.fill_(-7.0)
    refused = [dict(dtype=2), dict(mode=-1), dict(mode=st.NOJ2 + 1), dict(basis=4), dict(wform=-1),
               dict(wform=st.W_ROW + 1), dict(nflagcorr=3)]
    refused += [{name: None} for name in ('data', 'tbin_idx', 'tbin_counts', 'ant1', 'ant2', 'vis', 'wgt', 'mask', 'wsum',
                                          'work')]
    refused += [dict(wform=st.W_SPECTRUM), dict(mode=st.DIAG2)]          # weight / jones null where they are read
    # the 16-byte vector loads of data, and every array's element
    refused += [{name: good[name] + off} for name, off in (('data', 8), ('vis', 8), ('wgt', 4), ('ant1', 2),
                                                          ('tbin_idx', 4))]
    refused += [dict(ntime=0), dict(nant=0), dict(ndir=0)]
    for over in refused:
        assert call(**over) == INV, over
    for over in (dict(nrow=0), dict(nchan=0)):
        assert call(**over) == UNS, over
    torch.cuda.synchronize()
    assert (vis == -7 - 7j).all() and (wgt == -7.0).all() and (mask == 0xAB).all() and (wsum == -7.0).all()


@pytest.mark.parametrize('tag', TAGS)
def test_a_singular_jones_matrix_is_not_an_error(tag):
    """IEEE inf / nan on the unflagged visibilities that read it, as in the reference; everything else as before."""
    case = sc.case_named('sweep-full4-linear-I')
    a = wd_args(case, tag)
    s = case['set']
    jones = a['jones'].copy()
    jones[1, 2, :, 0] = 0                                   # antenna 2 in time bin 1
    vis, wgt = run_wd(case, tag, jones=jones)
    hit = ((sc.row_bins(vis.shape[0], s['tbin_idx'], s['tbin_counts']) == 1) & ((s['ant1'] == 2) | (s['ant2'] == 2)))
    live = ~s['flag'].astype(bool)
    assert (hit[:, None] & live).any()
    assert not np.isfinite(vis[hit[:, None] & live]).any()
    good = ~hit[:, None] | ~live
    ref_vis, ref_wgt = np.where(good, case['ref_vis'], 0), np.where(good, case['ref_wgt'], 0)
    vis_unit, wgt_unit = sc.closed_form(case)[3:]
    ev, ew = sc.worst(np.where(good, vis, 0), np.where(good, wgt, 0), ref_vis, ref_wgt, np.where(good, vis_unit, 0),
                      np.where(good, wgt_unit, 0), tag)
    assert ev <= sc.K and ew <= sc.K


# ------------------------------------------------------------------------------------------------- composition
@pytest.mark.parametrize('tag', TAGS)
def test_stokes_vis_feeds_image_data_products(tag):
    """stokes_vis's tensors go straight into image_data_products at the smallest configuration of
    test_gpu_image_data_products.py, against the same call fed the golden vis, wgt and mask.  Both sides run the same
    kernels, so what separates them is the inputs' error and the order of the gridder's atomic adds:
        WEIGHT   natural weighting hands wgt through: the per-element wgt bound of stokes_vis itself;
        DIRTY    per pixel (2 K + nvis) eps S, S = sum_i wgt_i |vis_i|: a pixel is a sum over the visibilities of
                 wgt_i vis_i times factors of modulus <= 1 up to the gridder's epsilon (the (1 + epsilon) is in the
                 bound); K eps each from vis and wgt, nvis eps for nvis terms added in any order;
        PSF      the same with vis = 1: (K + nvis) eps sum_i wgt_i;
        PSFHAT   a sum over the PSF's pixels: npix times the PSF's bound;
        WSUM     K eps of the golden sum, and stokes_vis's own wsum at its bound.
    A wiring error -- a transposed axis, a stale mask, the wrong tensor -- is far outside all of them."""
    from pfb_clean_amd.operators.gridder import image_data_products
    from pfb_clean_amd.utils.stokes import stokes_vis
    c = wc.CASES[wc.CASE_IDS.index('32x24-eps1e-05')]
    case = sc.case_named('sv-spectrum-minus-full')
    assert c['vis'].shape == case['ref_vis'].shape == sc.COMPOSE_SHAPE
    a = sv_args(case, tag)
    t = {k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in a.items()}
    vis, wgt, mask, wsum = stokes_vis(**t)
    assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in (vis, wgt, mask, wsum))

    def products(vis, wgt, mask):
        return image_data_products(dev(c['uvw']), dev(c['freq']), vis, wgt, mask, None, c['nx'], c['ny'], 2 * c['nx'],
                                   2 * c['ny'], c['px'], c['py'], epsilon=c['eps'], do_wgridding=c['do_wgridding'],
                                   x0=c['cx'], y0=c['cy'])
    got = products(vis, wgt, mask)
    gv, gw = case['ref_vis'].astype(sc.CDT[tag]), case['ref_wgt'].astype(sc.RDT[tag])
    want = products(dev(gv), dev(gw), dev(case['ref_mask']))
    assert set(got) == set(want) == {'WEIGHT', 'WSUM', 'DIRTY', 'PSF', 'PSFHAT'}
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in got.values())
    got, want = ({k: v.cpu().numpy() for k, v in d.items()} for d in (got, want))
    eps, live = sc.EPS[tag], case['ref_mask'] != 0
    wgt_unit = sc.closed_form(case)[4]
    assert (np.abs(got['WEIGHT'].astype(np.float64) - case['ref_wgt']) <= sc.K * eps * wgt_unit)[live].all()
    nvis = int(live.sum())
    s_dirty = float((case['ref_wgt'] * np.abs(case['ref_vis']))[live].sum()) * (1 + c['eps'])
    s_psf = float(case['ref_wgt'][live].sum()) * (1 + c['eps'])
    figures = {}
    for key, bound in (('DIRTY', (2 * sc.K + nvis) * eps * s_dirty), ('PSF', (sc.K + nvis) * eps * s_psf),
                       ('PSFHAT', (sc.K + nvis) * eps * s_psf * want['PSF'].size)):
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape and want[key].any()
        figures[key] = float(np.abs(got[key] - want[key]).max()) / bound
    print(f"composition {tag}: worst difference over its bound " + ', '.join(f'{k} {v:.3g}' for k, v in figures.items()))
    assert all(v <= 1 for v in figures.values()), figures
    assert abs(float(got['WSUM'][0]) - float(want['WSUM'][0])) <= sc.K * eps * float(want['WSUM'][0])
    assert abs(float(got['WSUM'][0]) - float(wsum[0])) <= sc.wsum_bound(case['ref_wgt'][live], tag)
