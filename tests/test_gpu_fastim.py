"""
fastim on the MI355X: pfb_imw_residual_weigh through the C ABI, single_stokes_image against the reference's results
(tests/golden/fastim.npz, made by tests/golden/make_golden_fastim.py), its stacked products and behaviour, and
stokes_image_cube against the single calls (pfb_clean_amd/utils/stokes2im.py).

Bounds:
  kernel        vis and wgt equal numpy's bit for bit: an element is one subtraction and a multiply by 0 or 1, a weight
                one fp64 product rounded once.  Each sum within n 2^-53 relative of math.fsum of the returned weights (n
                non-negative terms added in fp64 in any order).  Guards and planes beyond nprod unchanged; two runs agree
                bit for bit.
  'double'      out_dtype=float64, epsilon 1e-7.  Without a model |residual - golden|_2 <= epsilon |golden|_2 (the golden
                image is the direct sum: the criterion of test_gpu_image_data_products.py); with one,
                <= 2 epsilon (|R^H W vis| + |R^H W R model|), two gridder applications (the same file's precedent).
  'single'      epsilon at the fp32 EPS_MIN; per pixel |residual - golden| <= (2 K + nvis) eps S (1 + epsilon), K and eps
                those of stokes_cases, the bound of test_gpu_wgrid_multi.py's composition test, with S = sum over the
                unflagged visibilities of wgt (|vis| + |model vis|): the moduli of the terms a pixel adds.
  wsum          'double': within n 2^-53 relative of the golden weights' fp64 sum; 'single': within n 2^-24 relative of
                the golden value (the reference sums in fp32 there); n = nrow nchan.
  rms           |rms - golden| <= |residual - golden|_2 / sqrt(nx ny) (the triangle inequality for the std of a
                difference), and rms equals np.std of the returned image within npix 2^-52 relative (npix non-negative
                terms in any order, a mean and a root).
  float32       the default output lies, pixel by pixel, between the float32 casts of the float64 output of another run
                minus and plus the run-to-run spread of the gridder's atomic adds (1e-12 of the largest pixel in
                'double'): one correct rounding of the working image, since rounding is monotonic.
  same sums     results that differ only in the order of the gridder's atomic adds (and of the counts') agree to 1e-12
                relative, the criterion of test_gpu_wgrid_multi.py::test_single_and_stacked_calls_share_one_plan.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import fastim_cases as fc
import stokes_cases as sc

pytestmark = pytest.mark.gpu
pmp = pytest.mark.parametrize

NP_R = {'f32': np.float32, 'f64': np.float64}
NP_C = {'f32': np.complex64, 'f64': np.complex128}
GUARD = 64
SENT = 7.0            # exact in uint8 too
SAME = 1e-12


@pytest.fixture(scope='module')
def lib():
    from pfb_clean_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------- the kernel, through the C ABI
class Guarded:
    """`a` on the device between two guards of GUARD sentinels."""

    def __init__(self, a):
        self.n = a.size
        flat = np.full(a.size + 2 * GUARD, SENT, a.dtype)
        flat[GUARD:GUARD + a.size] = a.reshape(-1)
        self.buf = torch.from_numpy(flat).cuda()
        self.shape = a.shape

    def ptr(self):
        return self.buf.data_ptr() + GUARD * self.buf.element_size()

    def clone(self):
        g = object.__new__(Guarded)
        g.n, g.shape, g.buf = self.n, self.shape, self.buf.clone()
        return g

    def host(self):
        flat = self.buf.cpu().numpy()
        assert (flat[:GUARD] == SENT).all() and (flat[GUARD + self.n:] == SENT).all(), 'a guard was written'
        return flat[GUARD:GUARD + self.n].reshape(self.shape)


def kernel_data(n, tag):
    rng = np.random.default_rng(1000 + n)
    rdt, cdt = NP_R[tag], NP_C[tag]
    P = fc.MAX_PROD
    d = dict(vis=(rng.standard_normal((P, n)) + 1j * rng.standard_normal((P, n))).astype(cdt),
             model=(rng.standard_normal((P, n)) + 1j * rng.standard_normal((P, n))).astype(cdt),
             wgt=rng.uniform(0.5, 2.0, (P, n)).astype(rdt), imwgt=rng.uniform(0.0, 1.0, n),
             mask=(rng.uniform(size=n) < 0.8).astype(np.uint8))
    d['imwgt'][::7] = 0.0
    return d


def call(lib, tag, nprod, vis, model, model_of, mask, imwgt, n, wgt, rec, work):
    from pfb_clean_amd import _lib
    code = _lib.PFB_F32 if tag == 'f32' else _lib.PFB_F64
    nmodel = 0 if model is None else fc.MAX_PROD
    return lib.pfb_imw_residual_weigh(code, nprod, vis.ptr(), None if model is None else model.ptr(), nmodel,
                                      (C.c_int * len(model_of))(*model_of), mask.ptr(),
                                      None if imwgt is None else imwgt.ptr(), n, wgt.ptr(), rec.ptr(), work.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)


@pmp('tag', ('f32', 'f64'))
@pmp('n', fc.KERNEL_N)
def test_kernel_against_numpy(lib, n, tag):
    from pfb_clean_amd import _lib
    d = kernel_data(n, tag)
    base = {k: Guarded(v) for k, v in d.items()}
    zero_mask = Guarded(np.zeros(n, np.uint8))
    work = torch.empty(fc.WORK_DOUBLES, dtype=torch.float64, device='cuda')
    sums = {}                        # (plane, with imwgt) -> fsum over the mask of the expected (= returned) weights

    def expected_wgt(use_imwgt):
        w = d['wgt'].copy()
        if use_imwgt:
            w *= d['imwgt'][None, :]                             # numpy's in-place multiply: fp64 product, one rounding
        return w

    for nprod in range(1, fc.MAX_PROD + 1):
        runs = [(use_imwgt, m, False) for use_imwgt in (False, True) for m in fc.MODEL_MAPS[nprod]]
        runs.append((True, fc.MODEL_MAPS[nprod][-1], True))     # an all-zero mask
        for use_imwgt, model_of, zeroed in runs:
            mask_h = np.zeros(n, np.uint8) if zeroed else d['mask']
            want_vis, want_wgt = d['vis'].copy(), expected_wgt(use_imwgt)
            for p in range(nprod):
                if model_of[p] >= 0:
                    want_vis[p] = (d['vis'][p] - d['model'][model_of[p]]) * mask_h
            outs = []
            for _ in range(2):
                vis, wgt = base['vis'].clone(), base['wgt'].clone()
                rec = Guarded(np.full(fc.MAX_PROD, SENT))
                has_model = any(m >= 0 for m in model_of)
                rc = call(lib, tag, nprod, vis, base['model'] if has_model else None, model_of,
                          zero_mask if zeroed else base['mask'], base['imwgt'] if use_imwgt else None, n, wgt, rec, work)
                assert rc == _lib.PFB_OK
                outs.append((vis, wgt, rec))
            what = (n, tag, nprod, use_imwgt, model_of, zeroed)
            for a, b in zip(*outs):                                                     # two runs, the same bits
                assert torch.equal(a.buf.view(torch.uint8), b.buf.view(torch.uint8)), what
            got_vis, got_wgt, got_rec = (t.host() for t in outs[0])
            assert got_vis.dtype == want_vis.dtype and np.array_equal(got_vis, want_vis), what
            assert got_wgt.dtype == want_wgt.dtype and np.array_equal(got_wgt[:nprod], want_wgt[:nprod]), what
            assert np.array_equal(got_wgt[nprod:], d['wgt'][nprod:]), what             # planes beyond nprod: untouched
            assert (got_rec[nprod:] == SENT).all(), what
            for p in range(nprod):
                if zeroed:
                    assert got_rec[p] == 0.0, what
                    continue
                if (p, use_imwgt) not in sums:
                    sums[p, use_imwgt] = math.fsum(got_wgt[p][mask_h != 0].astype(np.float64).tolist())
                total = sums[p, use_imwgt]
                print(f'{what} plane {p}: sum {got_rec[p]!r} fsum {total!r}')
                assert abs(got_rec[p] - total) <= n * 2.0 ** -53 * total, what
    for k in ('model', 'imwgt', 'mask'):                         # the inputs and their guards are as they were
        assert np.array_equal(base[k].host(), d[k])


def test_kernel_refuses_and_an_empty_call_launches_nothing(lib):
    from pfb_clean_amd import _lib
    n = 17
    d = kernel_data(n, 'f64')
    g = {k: Guarded(v) for k, v in d.items()}
    rec = Guarded(np.full(fc.MAX_PROD, SENT))
    work = torch.empty(fc.WORK_DOUBLES, dtype=torch.float64, device='cuda')
    INV = _lib.PFB_ERR_INVALID
    for nprod in (0, 5, -1):
        assert call(lib, 'f64', nprod, g['vis'], g['model'], [0, 1, 2, 3], g['mask'], g['imwgt'], n, g['wgt'], rec, work) == INV
    assert call(lib, 'f64', 2, g['vis'], g['model'], [0, 4], g['mask'], g['imwgt'], n, g['wgt'], rec, work) == INV
    assert call(lib, 'f64', 2, g['vis'], None, [0, -1], g['mask'], g['imwgt'], n, g['wgt'], rec, work) == INV   # no planes
    assert lib.pfb_imw_residual_weigh(7, 1, g['vis'].ptr(), None, 0, (C.c_int * 1)(-1), g['mask'].ptr(), None, n,
                                      g['wgt'].ptr(), rec.ptr(), work.data_ptr(), None) == INV
    torch.cuda.synchronize()
    assert np.array_equal(g['vis'].host(), d['vis']) and np.array_equal(g['wgt'].host(), d['wgt'])
    assert (rec.host() == SENT).all()
    assert call(lib, 'f64', 3, g['vis'], g['model'], [0, 1, 2], g['mask'], g['imwgt'], 0, g['wgt'], rec, work) == _lib.PFB_OK
    assert np.array_equal(g['vis'].host(), d['vis']) and np.array_equal(g['wgt'].host(), d['wgt'])
    assert rec.host().tolist() == [0.0, 0.0, 0.0, SENT]


# ------------------------------------------------------------------------------ single_stokes_image against the golden
_runs = {}


def run(name, tag):
    """single_stokes_image on a golden case with out_dtype=float64, once per session: (residual, attrs)."""
    from pfb_clean_amd.utils.stokes2im import single_stokes_image
    if (name, tag) not in _runs:
        _runs[name, tag] = single_stokes_image(**fc.call_kwargs(fc.case_named(name), tag), out_dtype=np.float64)
    return _runs[name, tag]


@pmp('name', fc.CASE_IDS)
def test_double_against_the_reference(name):
    case, g = fc.case_named(name), fc.golden(name, 'double')
    res, attrs = run(name, 'double')
    assert isinstance(res, np.ndarray) and res.dtype == np.float64 and res.shape == (case['nx'], case['ny'])
    eps = fc.EPS['double']
    err = np.linalg.norm(res - g['residual'])
    if case['mds'] is None:
        bound = eps * np.linalg.norm(g['residual'])
    else:
        bound = 2 * eps * (g['norm_data'] + g['norm_model'])
    n = case['nrow'] * case['nchan']
    print(f"{name} double: |residual - golden| {err:.3e} bound {bound:.3e}; wsum {attrs['wsum']!r} golden {g['wsum']!r}; "
          f"rms {attrs['rms']!r} golden {g['rms']!r}")
    assert err <= bound
    assert isinstance(attrs['wsum'], float) and isinstance(attrs['rms'], float)
    assert abs(attrs['wsum'] - g['wsum']) <= n * 2.0 ** -53 * g['wsum']
    check_rms(res, attrs, g)


@pmp('name', fc.CASE_IDS)
def test_single_against_the_reference(name):
    from pfb_clean_amd.operators import gridder
    case, g = fc.case_named(name), fc.golden(name, 'single')
    assert fc.EPS['single'] == gridder.EPS_MIN[torch.float32]
    res, attrs = run(name, 'single')
    assert res.dtype == np.float64 and res.shape == (case['nx'], case['ny'])
    nvis = int(fc.live_mask(case).sum())
    bound = (2 * sc.K + nvis) * sc.EPS['f32'] * float(g['S']) * (1 + fc.EPS['single'])
    err = float(np.abs(res - g['residual']).max())
    n = case['nrow'] * case['nchan']
    print(f"{name} single: worst pixel {err:.3e} bound {bound:.3e}; wsum {attrs['wsum']!r} golden {g['wsum']!r}")
    assert err <= bound
    assert abs(attrs['wsum'] - g['wsum']) <= n * 2.0 ** -24 * g['wsum']
    check_rms(res, attrs, g)


def check_rms(res, attrs, g):
    npix = res.size
    assert abs(attrs['rms'] - g['rms']) <= np.linalg.norm(res - g['residual']) / math.sqrt(npix)
    assert abs(attrs['rms'] - np.std(res)) <= npix * 2.0 ** -52 * np.std(res)


@pmp('tag', fc.TAGS)
def test_default_output_is_float32_and_the_attributes_are_the_reference_s(tag):
    from pfb_clean_amd.utils.stokes2im import single_stokes_image
    case = fc.case_named('model-two-bins')
    res64, _ = run(case['name'], tag)
    res, attrs = single_stokes_image(**fc.call_kwargs(case, tag))
    # The float64 image of ANOTHER run cast once: the gridder adds with atomics, so two runs agree to d = SAME (fp64
    # sums) or 1e-5 (fp32 sums, the criterion of the tensors test below) of the largest pixel, not bit for bit.  Rounding
    # is monotonic: one correct cast of a value within d of res64 lies between the casts of res64 - d and res64 + d.
    d = (SAME if tag == 'double' else 1e-5) * np.abs(res64).max()
    lo, hi = (res64 - d).astype(np.float32), (res64 + d).astype(np.float32)
    assert res.dtype == np.float32 and ((lo <= res) & (res <= hi)).all()
    if tag == 'double':
        assert (res != res64).any()                              # and the cast rounded something
    assert set(attrs) == {'ra', 'dec', 'x0', 'y0', 'cell_rad', 'fieldid', 'ddid', 'scanid', 'freq_out', 'freq_min',
                          'freq_max', 'bandid', 'time_out', 'time_min', 'time_max', 'timeid', 'product', 'utc', 'wsum',
                          'rms'}
    assert (attrs['fieldid'], attrs['ddid'], attrs['scanid'], attrs['bandid'], attrs['timeid']) == (0, 1, 2, 3, 4)
    assert (attrs['ra'], attrs['dec'], attrs['x0'], attrs['y0']) == (0.3, -0.5, 0.0, 0.0)
    assert attrs['freq_out'] == np.mean(case['freq']) and attrs['freq_min'] == case['freq'].min()
    assert attrs['time_out'] == np.mean(case['utime']) and attrs['product'] == 'I' and attrs['cell_rad'] == case['cell']
    assert attrs['utc'] == '2014-02-24 23:06:40'                 # 4.9e9 s - 3506716800 s after 1970-01-01


# ------------------------------------------------------------------------------------------------- stacked products
def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel())


def test_iquv_against_four_single_letter_calls():
    from pfb_clean_amd.utils.stokes2im import single_stokes_image
    case = fc.case_named('jones-sigma-minus')
    kw = lambda product: fc.call_kwargs(case, 'double', opts=fc.opts(case, 'double', product=product))    # noqa: E731
    res, attrs = single_stokes_image(**kw('IQUV'), out_dtype=np.float64)
    assert res.shape == (4, case['nx'], case['ny']) and attrs['product'] == 'IQUV'
    assert isinstance(attrs['wsum'], list) and isinstance(attrs['rms'], list) and len(attrs['wsum']) == len(attrs['rms']) == 4
    for k, letter in enumerate('IQUV'):
        one, a = single_stokes_image(**kw(letter), out_dtype=np.float64)
        assert one.shape == res.shape[1:] and one.any()
        assert rel(res[k], one) <= SAME, letter
        assert abs(attrs['wsum'][k] - a['wsum']) <= SAME * a['wsum'] and abs(attrs['rms'][k] - a['rms']) <= SAME * a['rms']
    assert len({round(r, 6) for r in attrs['rms']}) == 4        # the planes are four different images
    # another order, fewer planes
    two, a2 = single_stokes_image(**kw('VQ'), out_dtype=np.float64)
    assert rel(two[0], res[3]) <= SAME and rel(two[1], res[1]) <= SAME
    assert abs(a2['wsum'][0] - attrs['wsum'][3]) <= SAME * attrs['wsum'][3]


def test_a_model_for_one_letter_leaves_the_other_planes():
    from pfb_clean_amd.utils.stokes2im import single_stokes_image
    case = fc.case_named('model-two-bins')
    o = fc.opts(case, 'double', product='IQUV')
    plain, ap = single_stokes_image(**fc.call_kwargs(case, 'double', opts=o, mds=None), out_dtype=np.float64)
    with_i, ai = single_stokes_image(**fc.call_kwargs(case, 'double', opts=o, mds={'I': case['mds']}), out_dtype=np.float64)
    for k in (1, 2, 3):
        assert rel(with_i[k], plain[k]) <= SAME
    assert rel(with_i[0], plain[0]) > 1e-3                       # the model was subtracted from I
    assert rel(with_i[0], run(case['name'], 'double')[0]) <= SAME
    assert all(abs(a - b) <= SAME * b for a, b in zip(ai['wsum'], ap['wsum']))
    with pytest.raises(ValueError):
        single_stokes_image(**fc.call_kwargs(case, 'double', opts=o))            # a bare model for four letters
    with pytest.raises(ValueError):
        single_stokes_image(**fc.call_kwargs(case, 'double', mds={'Q': case['mds']}))


# ------------------------------------------------------------------------------------------------- behaviour checks
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if isinstance(a, np.ndarray) else a


def test_filter_extreme_counts_equals_the_hand_chained_calls():
    from pfb_clean_amd.operators.gridder import vis2dirty
    from pfb_clean_amd.utils import weighting
    from pfb_clean_amd.utils.stokes import stokes_vis
    from pfb_clean_amd.utils.stokes2im import single_stokes_image
    case = fc.case_named('row-weights')
    o = fc.opts(case, 'double', filter_extreme_counts=True, filter_level=10.0)
    res, attrs = single_stokes_image(**fc.call_kwargs(case, 'double', opts=o), out_dtype=np.float64)
    nx, ny, cell = case['nx'], case['ny'], case['cell']
    vis, wgt, mask, _ = stokes_vis(case['data'], case['ant1'], case['ant2'], case['tbin_idx'], case['tbin_counts'],
                                   case['poltype'], case['product'], weight=case['weight'], precision='double')
    counts = weighting.compute_counts(case['uvw'], case['freq'], mask, nx, ny, cell, cell, np.float64, ngrid=o.nvthreads)
    filtered = weighting.filter_extreme_counts(counts, nbox=o.filter_nbox, nlevel=o.filter_level)
    assert not np.array_equal(filtered, counts)
    w = wgt * weighting.counts_to_weights(filtered, case['uvw'], case['freq'], nx, ny, cell, cell, o.robustness)
    want = vis2dirty(case['uvw'], case['freq'], vis, wgt=w, mask=mask, npix_x=nx, npix_y=ny, pixsize_x=cell,
                     pixsize_y=cell, epsilon=o.epsilon, do_wgridding=True, divide_by_n=False,
                     double_precision_accumulation=True)
    assert rel(res, want) <= SAME
    total = math.fsum(w[mask != 0].tolist())
    assert abs(attrs['wsum'] - total) <= SAME * total


def test_what_the_reference_cannot_run_is_refused():
    from pfb_clean_amd.utils.stokes2im import single_stokes_image
    case = fc.case_named('model-two-bins')
    for over in (dict(l2reweight_dof=5), dict(target='J0408-6545'), dict(target='04:08:20,-65:45:09')):
        with pytest.raises(NotImplementedError):
            single_stokes_image(**fc.call_kwargs(case, 'double', opts=fc.opts(case, 'double', **over)))


@pmp('product', ('Q', 'IQ'))
def test_an_all_flagged_chunk_gives_zeros(product):
    from pfb_clean_amd.utils.stokes2im import single_stokes_image
    case = fc.case_named('jones-sigma-minus')
    res, attrs = single_stokes_image(**fc.call_kwargs(case, 'single', frow=np.ones(case['nrow'], bool),
                                                      opts=fc.opts(case, 'single', product=product)))
    lead = () if len(product) == 1 else (len(product),)
    assert res.shape == lead + (case['nx'], case['ny']) and res.dtype == np.float32 and not res.any()
    assert attrs['wsum'] == (0.0 if not lead else [0.0] * len(product))
    assert attrs['rms'] == (0.0 if not lead else [0.0] * len(product))


@pmp('name', ('jones-sigma-minus', 'model-two-bins'))
def test_the_caller_s_arrays_are_unchanged_and_tensors_give_tensors(name):
    from pfb_clean_amd.utils.stokes2im import single_stokes_image
    case = fc.case_named(name)
    kw = fc.call_kwargs(case, 'single')
    kw['tbin_idx'] = kw['tbin_idx'] + 500                        # counted from the minimum
    tens = {k: dev(v) for k, v in kw.items()}
    keep = {k: v.clone() for k, v in tens.items() if isinstance(v, torch.Tensor)}
    res, attrs = single_stokes_image(**tens)
    assert isinstance(res, torch.Tensor) and res.is_cuda and res.dtype == torch.float32
    for k, v in keep.items():
        assert torch.equal(tens[k], v), k
    host, _ = single_stokes_image(**kw)
    for k in fc.COLUMNS:
        if isinstance(case[k], np.ndarray) and k != 'tbin_idx':
            assert np.array_equal(kw[k], case[k]), k
    assert np.array_equal(kw['tbin_idx'], case['tbin_idx'] + 500)
    assert rel(res.cpu().numpy(), run(name, 'single')[0]) <= 1e-5           # fp32 sums in another order
    assert rel(host, res.cpu().numpy()) <= 1e-5


def test_fbin_idx_counts_from_its_minimum():
    from pfb_clean_amd.utils.stokes2im import single_stokes_image
    case = fc.case_named('model-two-bins')
    res, attrs = single_stokes_image(**fc.call_kwargs(case, 'double', fbin_idx=case['fbin_idx'] + 1000),
                                     out_dtype=np.float64)
    want, wa = run(case['name'], 'double')
    assert rel(res, want) <= SAME and abs(attrs['rms'] - wa['rms']) <= SAME * wa['rms']


# --------------------------------------------------------------------------------------------------------- the cube
def cube_args(c, opts, convert=lambda a: a):
    cols = {k: (convert(c[k]) if isinstance(c[k], np.ndarray) else c[k])
            for k in ('data', 'ant1', 'ant2', 'uvw', 'freq', 'utime', 'frow', 'flag', 'weight', 'jones')}
    return dict(cols, time_mapping=c['time_mapping'], row_mapping=c['row_mapping'], freq_mapping=c['freq_mapping'],
                opts=opts, nx=c['nx'], ny=c['ny'], cell_rad=c['cell'], poltype=c['poltype'], mds=c['mds'],
                channels_per_grid_image=c['cpgi'], channels_per_degrid_image=c['cpdi'])


@pmp('product', ('I', 'IV'))
def test_cube_equals_the_single_calls(product):
    from pfb_clean_amd.operators import gridder
    from pfb_clean_amd.utils.stokes2im import single_stokes_image, stokes_image_cube
    c = fc.cube_dataset()
    o = fc.opts(c, 'double', product=product)
    mds = c['mds'] if product == 'I' else {'I': c['mds']}
    c = dict(c, mds=mds)
    lead = () if product == 'I' else (len(product),)
    # ---- tensors in: tensors out, no plan enters the cache, one set of tables for the one geometry
    gridder.clear_plan_cache()
    before = dict(gridder.cache_stats)
    res, wsum, rms = stokes_image_cube(**cube_args(c, o, dev), out_dtype=torch.float64)
    assert gridder.cache_stats['miss'] == before['miss']
    assert gridder.cache_stats['tables'] - before['tables'] <= 1            # the model's grid is the image's
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in (res, wsum, rms))
    assert res.shape == (3, 2) + lead + (c['nx'], c['ny']) and res.dtype == torch.float64
    assert wsum.shape == rms.shape == (3, 2) + lead and wsum.dtype == torch.float64
    res, wsum, rms = res.cpu().numpy(), wsum.cpu().numpy(), rms.cpu().numpy()
    # ---- the six single calls on the sliced columns
    tb, tc = c['tbin_idx'], c['tbin_counts']
    for ti in range(3):
        It = slice(2 * ti, 2 * ti + 2)
        Irow = slice(int(tb[2 * ti]), int(tb[2 * ti + 1] + tc[2 * ti + 1]))
        for fi in range(2):
            Inu = slice(2 * fi, 2 * fi + 2)
            one, attrs = single_stokes_image(
                data=c['data'][Irow, Inu], ant1=c['ant1'][Irow], ant2=c['ant2'][Irow], uvw=c['uvw'][Irow],
                frow=c['frow'][Irow], flag=c['flag'][Irow, Inu], weight=c['weight'][Irow, Inu], mds=mds,
                jones=c['jones'][It, Inu], opts=o, nx=c['nx'], ny=c['ny'], freq=c['freq'][Inu], cell_rad=c['cell'],
                utime=c['utime'][It], tbin_idx=tb[It], tbin_counts=tc[It], fbin_idx=np.arange(2 * fi, 2 * fi + 2),
                fbin_counts=np.ones(2, np.int64), radec=c['radec'], antpos=c['antpos'], poltype=c['poltype'],
                out_dtype=np.float64)
            assert one.any() and rel(res[ti, fi], one) <= SAME, (ti, fi)
            assert np.allclose(wsum[ti, fi], attrs['wsum'], rtol=SAME, atol=0)
            assert np.allclose(rms[ti, fi], attrs['rms'], rtol=SAME, atol=0)
    # ---- numpy in gives numpy out, float32 by default
    host = stokes_image_cube(**cube_args(c, o))
    assert all(isinstance(a, np.ndarray) for a in host) and host[0].dtype == np.float32 and host[1].dtype == np.float64
    assert rel(host[0], res) <= 1e-6 and rel(host[1], wsum) <= SAME
