"""
Band / time concatenation and beam resampling on the MI355X (pfb_clean_amd.utils.concat, .beam; csrc/visconcat.hip)
against what the reference's own source gives (tests/golden/concat.npz), case by case of tests/concat_cases.py and with
its bounds, whose derivations that module states:

  wgto       n_c u(T) ref                    viso   (n_c + 4) u(T) sum_i |vis_i| wgt_i mask_i / wgto per component
  masko, zeros where masko == 0, the non-finite pattern, UVW, FREQ, concatenated rows, attributes: equal
  wsum_i     relative (19 + max(0, ceil(log2(n / 128))) + 1) u(Tw)
  beam       that plus (nds + 2) u(Tb), on sum_i wsum_i |beam_i| / sum_i wsum_i
  eval_beam  16 u(fp64) sum_corners |w_c| |v_c|, plus u(fp32) |ref| with dtype=float32

concat_row's and concat_chan's expectations come from the reference's own lines run on eager stand-ins for xarray,
quartical's Blocker and dask.array (make_golden_concat.py defines them); nothing is restated in numpy there.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import concat_cases as cc
import wgrid_cases as wc
from concat_cases import OVERLAP_CASES, BEAM_SUM_CASES, BEAM_EVAL_CASES, CHAN_IN, CHAN_REF, ROW_IN, ROW_REF, TAGS

pytestmark = pytest.mark.gpu

TAG_LIST = list(TAGS)
CODE = {'f32': 0, 'f64': 1}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else t


def overlap_kwargs(src, conv=lambda a: a):
    kw = {}
    for i, s in enumerate(src):
        kw[f'vis{i}'], kw[f'wgt{i}'], kw[f'mask{i}'], kw[f'freq{i}'] = conv(s['vis']), conv(s['wgt']), conv(s['mask']), s['freq']
    return kw


def to_dataset(ds, conv=lambda a: a):
    """A case's dict as the package's VisDataset; conv moves the big arrays (to the device, or leaves them numpy)."""
    from pfb_clean_amd.utils.misc import VisDataset
    dims = {'VIS': ('row', 'chan'), 'WEIGHT': ('row', 'chan'), 'MASK': ('row', 'chan'), 'UVW': ('row', 'three'),
            'FREQ': ('chan',), 'BEAM': ('l_beam', 'm_beam')}
    return VisDataset({k: (d, conv(ds[k])) for k, d in dims.items()},
                      {k: ((k,), ds[k]) for k in ('chan', 'l_beam', 'm_beam')}, ds['attrs'])


def from_dataset(ds):
    out = {k: host(ds[k].values) for k in cc.VARS}
    out['attrs'] = dict(ds.attrs)
    return out


def ptrs(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def raw_sum_overlap(src, ufreq, tag, nrows=None, null=None, code=None):
    """pfb_vis_sum_overlap itself on the typed sources: (return code, viso, wgto, masko); the outputs start as a
    sentinel, so that a call that must not launch leaves them as they were."""
    from pfb_clean_amd import _lib
    cdt, rdt = TAGS[tag]
    vis, wgt, mask = ([dev(s[k]) for s in src] for k in ('vis', 'wgt', 'mask'))
    nrow, nco = src[0]['vis'].shape[0], ufreq.size
    cmap = dev(cc.channel_map(src, ufreq).astype(np.int32))
    viso = torch.full((nrow, nco), 7.0, dtype=getattr(torch, np.dtype(cdt).name), device='cuda')
    wgto = torch.full((nrow, nco), 7.0, dtype=getattr(torch, np.dtype(rdt).name), device='cuda')
    masko = torch.full((nrow, nco), 7, dtype=torch.uint8, device='cuda')
    nr = (C.c_size_t * len(src))(*(nrows or [s['vis'].shape[0] for s in src]))
    nch = (C.c_int * len(src))(*[s['vis'].shape[1] for s in src])
    rc = _lib.load().pfb_vis_sum_overlap(CODE[tag] if code is None else code, len(src), ptrs(vis), ptrs(wgt), ptrs(mask), nr,
                                         nch, cmap.data_ptr(), nrow, nco, None if null == 'viso' else viso.data_ptr(),
                                         wgto.data_ptr(), masko.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, viso.cpu().numpy(), wgto.cpu().numpy(), masko.cpu().numpy()


# ------------------------------------------------------------------------------------------------- sum_overlap
@pytest.mark.parametrize('tag', TAG_LIST)
@pytest.mark.parametrize('case', OVERLAP_CASES, ids=[c['name'] for c in OVERLAP_CASES])
def test_sum_overlap_kernel(case, tag):
    src = cc.typed_sources(case['src'], tag)
    rc, *got = raw_sum_overlap(src, case['ufreq'], tag)
    assert rc == 0
    cc.check_overlap(tuple(got), case['ref'][tag], src, case['ufreq'], tag, case['name'])


@pytest.mark.parametrize('tag', TAG_LIST)
@pytest.mark.parametrize('case', OVERLAP_CASES, ids=[c['name'] for c in OVERLAP_CASES])
def test_sum_overlap_function(case, tag):
    from pfb_clean_amd.utils.misc import sum_overlap
    src = cc.typed_sources(case['src'], tag)
    u = case['ufreq']
    out = sum_overlap(u, u[0], u[-1], **overlap_kwargs(src))
    assert set(out) == {'viso', 'wgto', 'masko'} and all(isinstance(v, np.ndarray) for v in out.values())
    cc.check_overlap((out['viso'], out['wgto'], out['masko']), case['ref'][tag], src, u, tag, case['name'])
    t = sum_overlap(u, u[0], u[-1], **overlap_kwargs(src, dev))
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in t.values())
    again = sum_overlap(u, u[0], u[-1], **overlap_kwargs(src, dev))
    for k in out:                                           # no atomics: the same bits from run to run, and as numpy in
        a = t[k].cpu().numpy()
        assert a.tobytes() == again[k].cpu().numpy().tobytes() == out[k].tobytes()


@pytest.mark.parametrize('tag', TAG_LIST)
@pytest.mark.parametrize('name', ['nine-interleaved', 'nine-full'])
def test_nine_sources_are_one_ordered_sum(name, tag):
    """Batches of 8 and then 1 give the bits of the statement's one sum over the 9 sources in dataset order."""
    case = cc.named(OVERLAP_CASES, name)
    assert len(case['src']) == cc.BATCH + 1
    src = cc.typed_sources(case['src'], tag)
    rc, viso, wgto, masko = raw_sum_overlap(src, case['ufreq'], tag)
    sv, sw, sm = cc.np_sum_overlap(src, case['ufreq'])
    assert rc == 0 and np.array_equal(masko, sm) and wgto.tobytes() == sw.tobytes()
    fin = np.isfinite(sv)
    assert np.array_equal(np.isfinite(viso), fin) and np.array_equal(viso[fin], sv[fin])


def test_sum_overlap_rejects_without_launching():
    from pfb_clean_amd import _lib
    case = cc.named(OVERLAP_CASES, 'partial')
    src = cc.typed_sources(case['src'], 'f64')
    for kw in (dict(null='viso'), dict(code=5), dict(nrows=[3, 4])):
        rc, viso, wgto, masko = raw_sum_overlap(src, case['ufreq'], 'f64', **kw)
        assert rc == _lib.PFB_ERR_INVALID, kw
        assert (viso == 7).all() and (wgto == 7).all() and (masko == 7).all()
    from pfb_clean_amd.utils.misc import sum_overlap
    kw = overlap_kwargs(src)
    kw['vis1'], kw['wgt1'], kw['mask1'] = (np.concatenate([kw[k], kw[k]]) for k in ('vis1', 'wgt1', 'mask1'))
    with pytest.raises(_lib.PfbHipError):
        sum_overlap(case['ufreq'], 0.0, 1.0, **kw)


# ---------------------------------------------------------------------------------------------------- sum_beam
@pytest.mark.parametrize('case', BEAM_SUM_CASES, ids=[c['name'] for c in BEAM_SUM_CASES])
def test_weight_sums_and_sum_beam(case):
    from pfb_clean_amd.utils.concat import weight_sums
    from pfb_clean_amd.utils.misc import _sum_beam
    for wtag, btag in cc.BEAM_TAGS:
        wgts = [w.astype(TAGS[wtag][1]) for w in case['wgt']]
        beams = [b.astype(TAGS[btag][1]) for b in case['beam']]
        rec = weight_sums([dev(w) for w in wgts])
        assert rec.is_cuda and rec.dtype == torch.float64
        for got, w in zip(rec.cpu().numpy(), wgts):
            ref = float(w.sum())                                # the reference's wgt.sum(), in the weights' type
            print(f"{case['name']} {wtag} n={w.size}: wsum rel err {abs(got - ref) / max(ref, 1e-300) / cc.U[wtag]:.2f} u")
            assert abs(got - ref) <= cc.wsum_bound(w.size, wtag) * ref
        kw = {}
        for i, (b, w) in enumerate(zip(beams, wgts)):
            kw[f'beam{i}'], kw[f'wgt{i}'] = b, w
        out = _sum_beam(9, 7, np.dtype(TAGS[btag][1]), **kw)
        assert set(out) == {'beam'} and isinstance(out['beam'], np.ndarray)
        cc.check_beam_sum(out['beam'], case['ref'][(wtag, btag)], beams, wgts, wtag, btag, case['name'])
        t = _sum_beam(9, 7, np.dtype(TAGS[btag][1]), **{k: dev(v) for k, v in kw.items()})['beam']
        assert t.is_cuda and t.cpu().numpy().tobytes() == out['beam'].tobytes()


def test_sum_beam_entry_points_reject():
    from pfb_clean_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    w, rec, work = dev(np.ones(4)), torch.full((2,), 7.0, dtype=torch.float64, device='cuda'), torch.zeros(8192, dtype=torch.float64, device='cuda')
    assert lib.pfb_vis_weight_sums(1, None, 4, rec.data_ptr(), work.data_ptr(), st) == _lib.PFB_ERR_INVALID
    assert lib.pfb_vis_weight_sums(3, w.data_ptr(), 4, rec.data_ptr(), work.data_ptr(), st) == _lib.PFB_ERR_INVALID
    beams, out = [dev(np.ones((2, 2)))], torch.full((2, 2), 7.0, dtype=torch.float64, device='cuda')
    assert lib.pfb_beam_combine(1, 1, ptrs(beams), None, 4, out.data_ptr(), st) == _lib.PFB_ERR_INVALID
    assert lib.pfb_beam_combine(2, 1, ptrs(beams), rec.data_ptr(), 4, out.data_ptr(), st) == _lib.PFB_ERR_INVALID
    assert lib.pfb_beam_combine(1, 1, (C.c_void_p * 1)(None), rec.data_ptr(), 4, out.data_ptr(), st) == _lib.PFB_ERR_INVALID
    g = dev(np.array([0.0, 1.0]))
    args = (beams[0].data_ptr(), 2, 2, g.data_ptr(), g.data_ptr(), g.data_ptr(), g.data_ptr(), 0, 2, 2)
    assert lib.pfb_beam_eval(1, *args, 1, None, st) == _lib.PFB_ERR_INVALID
    assert lib.pfb_beam_eval(1, *args, 4, out.data_ptr(), st) == _lib.PFB_ERR_INVALID
    assert lib.pfb_beam_eval(1, beams[0].data_ptr(), 1, 2, *args[3:], 1, out.data_ptr(), st) == _lib.PFB_ERR_INVALID
    torch.cuda.synchronize()
    assert (rec == 7).all() and (out == 7).all()


# --------------------------------------------------------------------------------------------------- eval_beam
@pytest.mark.parametrize('case', BEAM_EVAL_CASES, ids=[c['name'] for c in BEAM_EVAL_CASES])
def test_eval_beam(case):
    from pfb_clean_amd.utils.beam import _eval_beam, eval_beam
    for tag, (_, rdt) in TAGS.items():
        c = dict(case, beam=case['beam'].astype(rdt))
        got = _eval_beam(c['beam'], c['l_in'], c['m_in'], c['l_out'], c['m_out'])
        assert isinstance(got, np.ndarray)
        cc.check_beam_eval(got, case['ref'][tag], c, label=f"{case['name']} {tag}")
        t = eval_beam(dev(c['beam']), dev(c['l_in']), dev(c['m_in']), dev(c['l_out']), dev(c['m_out']))
        assert t.is_cuda and t.dtype == torch.float64 and t.cpu().numpy().tobytes() == got.tobytes()
        g32 = _eval_beam(c['beam'], c['l_in'], c['m_in'], c['l_out'], c['m_out'], dtype=np.float32)
        cc.check_beam_eval(g32, case['ref'][tag], c, dtype=np.float32, label=f"{case['name']} {tag} -> f32")


def test_eval_beam_nan_and_errors():
    from pfb_clean_amd.utils.beam import _eval_beam, _interp_beam_impl
    c = cc.named(BEAM_EVAL_CASES, '9x7-5x4')
    l_out = c['l_out'].copy()
    l_out[2] = np.nan
    got = _eval_beam(c['beam'], c['l_in'], c['m_in'], l_out, c['m_out'])
    assert np.isnan(got[2]).all() and np.array_equal(np.delete(got, 2, 0), np.delete(_eval_beam(
        c['beam'], c['l_in'], c['m_in'], c['l_out'], c['m_out']), 2, 0))
    with pytest.raises(ValueError, match='Only 1 or 2D coordinates supported for beam evaluation'):
        _eval_beam(c['beam'], c['l_in'], c['m_in'], np.zeros((2, 2, 2)), np.zeros((2, 2, 2)))
    bad = c['l_in'].copy()
    bad[3] = bad[5]
    with pytest.raises(ValueError):
        _eval_beam(c['beam'], bad, c['m_in'], c['l_out'], c['m_out'])
    ones = _interp_beam_impl(np.array([1.0e9]), 6, 4, 0.01, None)
    assert ones.is_cuda and ones.dtype == torch.float64 and tuple(ones.shape) == (6, 4) and bool((ones == 1).all())
    with pytest.raises(NotImplementedError):
        _interp_beam_impl(1.0e9, 6, 4, 0.01, 'kbl')


# ------------------------------------------------------------------------------------- concat_chan, concat_row
@pytest.mark.parametrize('tag', TAG_LIST)
@pytest.mark.parametrize('nband_out', [2, 3])
def test_concat_chan(nband_out, tag):
    from pfb_clean_amd.utils.misc import concat_chan
    typed = cc.typed_datasets(CHAN_IN, tag)
    ref, plan = CHAN_REF[(nband_out, tag)], cc.chan_plan(typed, nband_out)
    for conv in (lambda a: a, dev):
        got = concat_chan([to_dataset(ds, conv) for ds in typed], nband_out=nband_out)
        assert len(got) == len(ref)
        for k, (g, r, p) in enumerate(zip(got, ref, plan)):
            for name in ('VIS', 'WEIGHT', 'MASK', 'UVW', 'BEAM'):
                v = g[name].values
                assert (isinstance(v, torch.Tensor) and v.is_cuda) if conv is dev else isinstance(v, np.ndarray), name
            cc.check_chan_dataset(from_dataset(g), r, [typed[i] for i in p[-1]], tag, f'chan{nband_out}[{k}]')


def test_concat_early_returns_and_the_empty_bin():
    from pfb_clean_amd.utils.misc import concat_chan, concat_row
    xds = [to_dataset(ds) for ds in cc.typed_datasets(CHAN_IN, 'f64')]
    assert concat_chan(xds, nband_out=4) is xds
    one = xds[:1]
    assert concat_chan(one, nband_out=3) is one
    with pytest.raises(ValueError, match='band 0'):
        concat_chan(xds, nband_out=cc.NBAND_NONE)
    rows = [to_dataset(ds) for ds in cc.typed_datasets(ROW_IN, 'f64')][:2]
    assert concat_row(rows) is rows


@pytest.mark.parametrize('tag', TAG_LIST)
def test_concat_row(tag):
    from pfb_clean_amd.utils.misc import concat_row
    typed = cc.typed_datasets(ROW_IN, tag)
    ref, plan = ROW_REF[tag], cc.row_plan(typed)
    for conv in (lambda a: a, dev):
        got = concat_row([to_dataset(ds, conv) for ds in typed])
        assert len(got) == len(ref) == 2
        for k, (g, r, sel) in enumerate(zip(got, ref, plan)):
            for name in ('VIS', 'WEIGHT', 'MASK', 'UVW', 'BEAM'):
                v = g[name].values
                assert (isinstance(v, torch.Tensor) and v.is_cuda) if conv is dev else isinstance(v, np.ndarray), name
            cc.check_row_dataset(from_dataset(g), r, [typed[i] for i in sel], tag, f'row[{k}]')


# -------------------------------------------------------------------------------------------------- end to end
def test_merge_resample_and_image_on_the_device():
    """concat_chan -> image_geometry -> _eval_beam -> image_data_products with VIS, WEIGHT and MASK device tensors
    throughout; DIRTY against image_data_products of the golden merged arrays (both are within epsilon of the direct
    sum, the bound of test_gpu_image_data_products.py: 2 epsilon between them) and against the direct sum itself."""
    from pfb_clean_amd.operators.gridder import image_data_products
    from pfb_clean_amd.utils.beam import _eval_beam
    from pfb_clean_amd.utils.concat import image_geometry
    from pfb_clean_amd.utils.misc import concat_chan
    eps, nband_out = 1e-7, 2
    typed = cc.typed_datasets(CHAN_IN, 'f64')
    xds = concat_chan([to_dataset(ds, dev) for ds in typed], nband_out=nband_out)
    geo = image_geometry(xds, super_resolution_factor=2.0, nx=32, ny=24)
    uv_max = max(np.abs(ds['UVW'][:, :2]).max() for ds in CHAN_IN)
    assert geo['cell_N'] == 1.0 / (2 * uv_max * max(d['FREQ'].max() for d in CHAN_REF[(2, 'f64')]) / wc.C_LIGHT)
    assert geo['cell_rad'] == geo['cell_N'] / 2.0 and (geo['nx'], geo['ny'], geo['nx_psf'], geo['ny_psf']) == (32, 24, 64, 48)
    with pytest.raises(ValueError, match='Requested cell size too large'):
        image_geometry(xds, cell_size=2 * geo['cell_N'] * 180 * 3600 / np.pi, nx=32)
    cell = geo['cell_rad']
    l_out, m_out = (-(32 // 2) + np.arange(32)) * cell, (-(24 // 2) + np.arange(24)) * cell
    for ds, ref in zip(xds, CHAN_REF[(nband_out, 'f64')]):
        vis, wgt, mask = ds.VIS.values, ds.WEIGHT.values, ds.MASK.values
        assert vis.is_cuda and wgt.is_cuda and mask.is_cuda and ds.UVW.values.is_cuda and ds.BEAM.values.is_cuda
        beam = _eval_beam(ds.BEAM.values, ds.l_beam.values, ds.m_beam.values, dev(l_out), dev(m_out))
        assert beam.is_cuda and tuple(beam.shape) == (32, 24)
        c = dict(beam=ref['BEAM'], l_in=ref['l_beam'], m_in=ref['m_beam'], l_out=l_out, m_out=m_out)
        cc.check_beam_eval(beam.cpu().numpy(), cc.np_eval_beam(**c), c, label='end to end')
        kw = dict(robustness=None, epsilon=eps, do_wgridding=True, do_psf=False)
        out = image_data_products(ds.UVW.values, dev(ds.FREQ.values), vis, wgt, mask, None, 32, 24, 64, 48, cell, cell, **kw)
        assert all(v.is_cuda for v in out.values())
        gold = image_data_products(ref['UVW'], ref['FREQ'], ref['VIS'], ref['WEIGHT'], ref['MASK'], None, 32, 24, 64, 48,
                                   cell, cell, **kw)
        direct = wc.direct_vis2dirty(dict(uvw=ref['UVW'], freq=ref['FREQ'], mask=ref['MASK'], wgt=ref['WEIGHT'], nx=32,
                                          ny=24, px=cell, py=cell, cx=0.0, cy=0.0, do_wgridding=True, divide_by_n=False),
                                     ref['VIS'])
        dirty = out['DIRTY'].cpu().numpy()
        e_gold, e_direct = wc.rel_l2(dirty, gold['DIRTY']), wc.rel_l2(dirty, direct)
        print(f"band {ref['attrs']['bandid']} time {ref['attrs']['time_out']}: DIRTY vs golden arrays {e_gold:.3e}, "
              f"vs the direct sum {e_direct:.3e} (eps {eps:g})")
        assert e_gold <= 2 * eps and e_direct <= eps
