"""
The predict step on the MI355X: pfb_wgrid_finish_block and pfb_vis_restore_corrs through the C ABI, and
gridder.im2vis / comps2vis / loc2psf_vis and misc.restore_corrs on top of them, against tests/degrid_cases.py and
tests/golden/degrid.npz (tests/test_cpu_degrid.py proves those on the CPU).

finish_block    every combination of nsorted 1 / 255 / 256 / 257, nchan_blk 1 / 3, ncorr 1 / 2 / 4, row0 0 / 5, chan0 0 / 2
                (nchan_out > chan0 + nchan_blk), centre phase, output type (the plan's, or complex64 under an fp64 plan),
                accumulate, and an order that skips visibilities.  The output is pre-filled (a constant sentinel, or random
                old values where the kernel adds); every cell outside (block rows x block channels x {0, ncorr - 1}) and
                every skipped visibility inside keeps its bits.  A written cell stays, per component, within
                    C U_T S  +  U_O |v| (narrowed)  +  U_O (|old| + |v| + the former two) (accumulate)
                with C = TOLERANCE_C['finish'] of wgrid_kernel_cases.py, S its sum of absolute values
                (degrid_cases.ref_finish_block).  Without a centre phase nothing is uncertain and the bits are asserted:
                (O) acc, or fl_O(old + (O) acc) -- which is what tells "cast, then add" from "add, then cast".
                Recorded on the MI355X, max |got - ref| / (U_T S) over the same-type overwrite entries, against that C:
                    fp32 1.59 (C = 8)        fp64 34.0 (C = 256)        -- below C: the constants stand
restore_corrs   bit for bit, ncorr 1 / 2 / 4, both types, 255 / 256 / 257 visibilities.
im2vis          a band's channels are dirty2vis(uvw, freq[ind], image[i]) bit for bit; uncovered channels exactly zero.
accuracy        the project's rule, rel_l2 <= epsilon per block against the direct sum (degrid_cases.ACCURACY: fp64 at
                1e-5, 1e-7, 1e-9, fp32 at 1e-3 and EPS_MIN), and against degrid.npz -- the reference's own run -- at the same
                bound.  fp32 runs see the inputs rounded to fp32 (the model is given the same).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import degrid_cases as dc
import wgrid_cases as wc
import wgrid_kernel_cases as kc

pytestmark = pytest.mark.gpu
pmp = pytest.mark.parametrize

RDT = {'f32': torch.float32, 'f64': torch.float64}
CDT = {'f32': torch.complex64, 'f64': torch.complex128}
NP_R = {'f32': np.float32, 'f64': np.float64}
SENTINEL = 7.25 - 3.5j

_worst = {}


@pytest.fixture(scope='module')
def lib():
    from pfb_clean_amd import _lib
    return _lib.load()


@pytest.fixture(scope='module')
def npz(golden):
    return golden('degrid')


@pytest.fixture(scope='module')
def gridder():
    from pfb_clean_amd.operators import gridder
    return gridder


class Plan:
    """The native plan of a geometry record of wgrid_kernel_cases."""

    def __init__(self, lib, geom):
        from pfb_clean_amd import _lib
        self.lib, self.h = lib, C.c_void_p()
        self.code = {'f32': _lib.PFB_F32, 'f64': _lib.PFB_F64}
        rc = lib.pfb_wgrid_plan_create(self.code[geom['dtype']], geom['nx'], geom['ny'], geom['px'], geom['py'],
                                       geom['cx'], geom['cy'], geom['W'], geom['nplanes'], geom['w0'], geom['dw'],
                                       C.byref(self.h))
        assert rc == 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.lib.pfb_wgrid_plan_destroy(self.h)

    def finish_block(self, acc, idx, coord, nchan_blk, out, out_tag, row0, chan0, accumulate):
        return self.lib.pfb_wgrid_finish_block(self.h, acc.data_ptr(), idx.data_ptr(), coord.data_ptr(), acc.numel(),
                                               nchan_blk, out.data_ptr(), self.code[out_tag], row0, out.shape[1], chan0,
                                               out.shape[2], int(accumulate), torch.cuda.current_stream().cuda_stream)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype).contiguous()


# ------------------------------------------------------------------------------------------------- finish_block
TYPES = (('f32', 'f32'), ('f64', 'f64'), ('f64', 'f32'))


@pmp('nsorted', (1, 255, 256, 257))
@pmp('dtype,out_tag', TYPES, ids=['f32', 'f64', 'f64-to-c64'])
def test_finish_block(lib, dtype, out_tag, nsorted):
    seed = 0
    for nchan_blk in (1, 3):
        for centre in (False, True):
            for skip in (False, True):
                seed += 1
                geom, acc, idx, coord, nrow_blk = dc.finish_data(nsorted, nchan_blk, dtype, centre, skip, 7000 + seed)
                acc = acc.astype(dc.NP_C[dtype])
                acc_d, idx_d, coord_d = dev(acc), dev(idx), dev(coord)
                with Plan(lib, geom) as plan:
                    for ncorr in (1, 2, 4):
                        for row0 in (0, 5):
                            for chan0 in (0, 2):
                                for accumulate in (False, True):
                                    _finish_one(plan, geom, acc, idx, coord, acc_d, idx_d, coord_d, nchan_blk, nrow_blk,
                                                out_tag, ncorr, row0, chan0, centre, accumulate, seed)


def _finish_one(plan, geom, acc, idx, coord, acc_d, idx_d, coord_d, nchan_blk, nrow_blk, out_tag, ncorr, row0, chan0,
                centre, accumulate, seed):
    dtype = geom['dtype']
    shape = (row0 + nrow_blk + 1, chan0 + nchan_blk + 1, ncorr)
    what = (f"{dtype}->{out_tag} ns {acc.size} nchan_blk {nchan_blk} ncorr {ncorr} row0 {row0} chan0 {chan0} centre {centre} "
            f"accumulate {accumulate}")
    if accumulate:
        rng = np.random.default_rng(seed + 100 * ncorr + row0 + chan0)
        out0 = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dc.NP_C[out_tag])
    else:
        out0 = np.full(shape, SENTINEL, dc.NP_C[out_tag])
    out_d = dev(out0)
    assert plan.finish_block(acc_d, idx_d, coord_d, nchan_blk, out_d, out_tag, row0, chan0, accumulate) == 0, what
    got = out_d.cpu().numpy()
    ref, B, written = dc.ref_finish_block(geom, acc, idx, coord, nchan_blk, out0, out_tag, row0, chan0, accumulate)
    assert written.sum() == acc.size * min(ncorr, 2)
    assert np.array_equal(got[~written].view(NP_R[out_tag]), out0[~written].view(NP_R[out_tag])), what   # untouched bits
    over = dc.excess(got, ref, B)
    assert over <= 1.0, (what, over)
    if not centre:                    # nothing uncertain: cast, then store or add in the output's type
        cell = dc.cells_of(idx, nchan_blk, row0, shape[1], chan0, ncorr)
        want = out0.reshape(-1).copy()
        for k in ((0,) if ncorr == 1 else (0, ncorr - 1)):
            cast = acc.astype(dc.NP_C[out_tag])
            want[cell + k] = want[cell + k] + cast if accumulate else cast
        assert np.array_equal(got.reshape(-1).view(NP_R[out_tag]), want.view(NP_R[out_tag])), what
    if out_tag == dtype and not accumulate:
        v, S = kc.ref_finish(geom, acc, None, np.arange(acc.size), coord, acc.size)
        cell = dc.cells_of(idx, nchan_blk, row0, shape[1], chan0, ncorr)
        g = got.reshape(-1)[cell].astype(np.complex128)
        fig = 0.0
        for d, s in ((np.abs(g.real - v.real), S.real), (np.abs(g.imag - v.imag), S.imag)):
            fig = max(fig, float((d[s > 0] / s[s > 0]).max()) / kc.U[dtype])
        _worst[dtype] = max(_worst.get(dtype, 0.0), fig)


def test_finish_block_figures():
    """Prints what test_finish_block recorded (run the file as a whole)."""
    for dtype in ('f32', 'f64'):
        if dtype in _worst:
            print(f"finish_block {dtype}: max |got - ref| / (U S) = {_worst[dtype]:.3g} "
                  f"(C = {kc.TOLERANCE_C['finish'][dtype]:g})")
            assert _worst[dtype] <= kc.TOLERANCE_C['finish'][dtype]


def test_finish_block_refuses(lib):
    geom, acc, idx, coord, nrow_blk = dc.finish_data(8, 2, 'f32', False, False, 1)
    acc_d, idx_d, coord_d = dev(acc.astype(np.complex64)), dev(idx), dev(coord)
    out = torch.zeros((nrow_blk, 4, 2), dtype=torch.complex128, device='cuda')
    with Plan(lib, geom) as plan:
        assert plan.finish_block(acc_d, idx_d, coord_d, 2, out, 'f64', 0, 0, False) == -1      # widening
        out32 = torch.zeros((nrow_blk, 4, 5), dtype=torch.complex64, device='cuda')
        assert plan.finish_block(acc_d, idx_d, coord_d, 2, out32, 'f32', 0, 0, False) == -1    # ncorr 5
        out32 = torch.zeros((nrow_blk, 4, 2), dtype=torch.complex64, device='cuda')
        assert plan.finish_block(acc_d, idx_d, coord_d, 2, out32, 'f32', 0, 3, False) == -1    # chan0 + nchan_blk > nchan_out
        assert plan.finish_block(acc_d, idx_d, coord_d, 0, out32, 'f32', 0, 0, False) == -1
        assert plan.finish_block(acc_d, idx_d, coord_d, 2, out32, 'f32', 0, 2, False) == 0
    assert not out.any().item() and not out32[:, :2].any().item() and out32[:, 2:].all().item()


# ------------------------------------------------------------------------------------------------ restore_corrs
@pmp('nvis', (255, 256, 257))
@pmp('dtype', ('f32', 'f64'))
@pmp('ncorr', (1, 2, 4))
def test_restore_corrs(lib, ncorr, dtype, nvis):
    from pfb_clean_amd.utils import misc
    rng = np.random.default_rng(nvis + ncorr)
    vis = (rng.standard_normal((nvis, 1)) + 1j * rng.standard_normal((nvis, 1))).astype(dc.NP_C[dtype])
    want = dc.ref_restore_corrs(vis, ncorr)
    got = misc.restore_corrs(vis, ncorr)
    assert isinstance(got, np.ndarray) and got.dtype == vis.dtype and got.shape == (nvis, 1, ncorr)
    assert np.array_equal(got.view(NP_R[dtype]), want.view(NP_R[dtype]))
    # the C ABI on a pre-filled output: every element is written
    vd = dev(vis.reshape(85, -1) if nvis == 255 else vis)
    out = torch.full((nvis * ncorr,), SENTINEL, dtype=CDT[dtype], device='cuda')
    from pfb_clean_amd import _lib
    code = _lib.PFB_F32 if dtype == 'f32' else _lib.PFB_F64
    assert lib.pfb_vis_restore_corrs(code, vd.data_ptr(), nvis, ncorr, out.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream) == 0
    assert np.array_equal(out.cpu().numpy().view(NP_R[dtype]), want.reshape(-1).view(NP_R[dtype]))
    gt = misc._restore_corrs(vd, ncorr)
    assert gt.is_cuda and tuple(gt.shape) == tuple(vd.shape) + (ncorr,) and torch.equal(gt.reshape(-1), out)
    assert lib.pfb_vis_restore_corrs(code, vd.data_ptr(), nvis, 5, out.data_ptr(), None) == -1
    with pytest.raises(ValueError):
        misc.restore_corrs(vis, 0)


# ------------------------------------------------------------------------------------------------------- im2vis
def _kw(c, **over):
    kw = dict(x0=c['cx'], y0=c['cy'], epsilon=c['eps'], do_wgridding=c['do_wgridding'], divide_by_n=c['divide_by_n'])
    kw.update(over)
    return kw


@pmp('centre', (False, True))
@pmp('dtype', ('f32', 'f64'))
def test_im2vis_is_dirty2vis_per_band(gridder, dtype, centre):
    c = dc.ACCURACY[0]
    eps = 1e-5
    x0, y0 = (0.05, -0.08) if centre else (0.0, 0.0)
    cube = c['cube'][:2].astype(NP_R[dtype])
    idx, cnts = np.array([11, 14]), np.array([2, 2])              # channels 0 1 | 3 4 of six: 2 and 5 uncovered
    got = gridder.im2vis(c['uvw'], c['freq'], cube, c['px'], c['py'], idx, cnts, x0=x0, y0=y0, epsilon=eps,
                         do_wgridding=True, divide_by_n=False)
    assert isinstance(got, np.ndarray) and got.dtype == dc.NP_C[dtype] and got.shape == (c['uvw'].shape[0], 6)
    assert not got[:, 2].any() and not got[:, 5].any()
    for i, a in enumerate((0, 3)):
        band = gridder.dirty2vis(c['uvw'], np.ascontiguousarray(c['freq'][a:a + 2]), cube[i], pixsize_x=c['px'],
                                 pixsize_y=c['py'], center_x=x0, center_y=y0, epsilon=eps, do_wgridding=True,
                                 divide_by_n=False)
        assert band.dtype == got.dtype and np.array_equal(got[:, a:a + 2].view(NP_R[dtype]), band.view(NP_R[dtype]))
    # tensors in, a tensor out, the same bits; the private name is the same function
    gt = gridder._im2vis_impl(dev(c['uvw']), dev(c['freq']), dev(cube), c['px'], c['py'], idx, cnts, x0, y0, eps, False,
                              True, False, 4)
    assert gt.is_cuda and np.array_equal(gt.cpu().numpy().view(NP_R[dtype]), got.view(NP_R[dtype]))


# ----------------------------------------------------------------------------------------------------- accuracy
def _comps2vis(gridder, c, dtype=None, **over):
    dtype = dtype or c['dtype']
    kw = _kw(c, ncorr_out=c.get('ncorr_out', 4))
    kw.update(over)
    return gridder.comps2vis(c['uvw'], c['utime'], c['freq'], *dc.bins(c), c['comps'].astype(NP_R[dtype]), c['Ix'], c['Iy'],
                             dc.modelf, dc.tfunc, dc.ffunc, c['nx'], c['ny'], c['px'], c['py'], **kw)


def _layout_ok(got, ncorr):
    assert got.ndim == 3 and got.shape[2] == ncorr
    assert not got[:, :, 1:-1].any() and np.array_equal(got[:, :, 0], got[:, :, -1]) and got[:, :, 0].all()


@pmp('c', dc.ACCURACY, ids=dc.ACCURACY_IDS)
def test_accuracy_against_the_direct_sum(gridder, c):
    dtype, ncorr = c['dtype'], c['ncorr_out']
    got = _comps2vis(gridder, c)
    assert isinstance(got, np.ndarray) and got.dtype == dc.NP_C[dtype]
    _layout_ok(got, ncorr)
    ref = dc.model_comps2vis(c, 1, comps=c['comps'].astype(NP_R[dtype]))[:, :, 0]
    errs = dc.block_errors(c, got[:, :, 0].astype(np.complex128), ref)
    cube = c['cube'].astype(NP_R[dtype])
    im = gridder.im2vis(c['uvw'], c['freq'], cube, c['px'], c['py'], c['fbin_idx'], c['fbin_cnts'], **_kw(c))
    cube_errs = dc.band_errors(c, im.astype(np.complex128), dc.model_im2vis(c, cube.astype(np.float64)))
    print(f"{c['name']}: worst block {max(errs) / c['eps']:.3f} epsilon (comps2vis), {max(cube_errs) / c['eps']:.3f} "
          f"epsilon (im2vis)")
    assert len(errs) == 6 and max(errs) <= c['eps'] and max(cube_errs) <= c['eps']


@pmp('dtype', ('f64', 'f32'))
@pmp('c', dc.GOLDEN, ids=dc.GOLDEN_IDS)
def test_against_the_reference_run(gridder, npz, c, dtype):
    eps = c['eps'] if dtype == 'f64' else 1e-5
    ncorr = dc.GOLDEN_NCORR[c['name']]
    ref = npz[c['name'] + '_comps2vis']
    got = _comps2vis(gridder, c, dtype, ncorr_out=ncorr, epsilon=eps)
    assert got.shape == ref.shape and got.dtype == dc.NP_C[dtype]
    _layout_ok(got, ncorr)
    errs = dc.block_errors(c, got[:, :, 0].astype(np.complex128), ref[:, :, 0])
    im = gridder.im2vis(c['uvw'], c['freq'], c['cube'].astype(NP_R[dtype]), c['px'], c['py'], c['fbin_idx'],
                        c['fbin_cnts'], **_kw(c, epsilon=eps))
    cube_errs = dc.band_errors(c, im.astype(np.complex128), npz[c['name'] + '_im2vis'])
    print(f"{c['name']} {dtype}: worst block {max(errs) / eps:.3f} epsilon (comps2vis), {max(cube_errs) / eps:.3f} "
          f"epsilon (im2vis) against the reference's run")
    assert max(errs) <= eps and max(cube_errs) <= eps


@pmp('c', [dc.GOLDEN[0], dc.ACCURACY[1], dc.ACCURACY[7]], ids=['g-mapping', dc.ACCURACY_IDS[1], dc.ACCURACY_IDS[7]])
def test_time_bins_in_one_call_are_the_single_bin_calls(gridder, c):
    whole = _comps2vis(gridder, c, ncorr_out=2)
    rdt = NP_R[c['dtype']]
    for t in range(c['tbin_idx'].size):
        one, r0, r1 = dc.time_bin_case(c, t)
        part = _comps2vis(gridder, one, ncorr_out=2)
        assert part.shape == (r1 - r0,) + whole.shape[1:]
        assert np.array_equal(part.view(rdt), whole[r0:r1].view(rdt))


def test_tensors_in_give_the_same_bits_and_an_empty_model_gives_zeros(gridder):
    c = dc.GOLDEN[1]
    want = _comps2vis(gridder, c, ncorr_out=2)
    t = lambda a: dev(a)                                                                             # noqa: E731
    got = gridder._comps2vis_impl(t(c['uvw']), t(c['utime']), t(c['freq']), *(t(b) for b in dc.bins(c)), t(c['comps']),
                                  t(c['Ix']), t(c['Iy']), dc.modelf, dc.tfunc, dc.ffunc, c['nx'], c['ny'], c['px'], c['py'],
                                  c['cx'], c['cy'], c['eps'], 1, c['do_wgridding'], c['divide_by_n'], 2)
    assert got.is_cuda and np.array_equal(got.cpu().numpy().view(np.float64), want.view(np.float64))
    none = gridder.comps2vis(c['uvw'], c['utime'], c['freq'], *dc.bins(c), c['comps'][:, :0], c['Ix'][:0], c['Iy'][:0],
                             dc.modelf, dc.tfunc, dc.ffunc, c['nx'], c['ny'], c['px'], c['py'], **_kw(c))
    assert none.shape == want.shape[:2] + (4,) and none.dtype == np.complex128 and not none.any()


# -------------------------------------------------------------------------------------------------- worker tail
def test_out_and_accumulate(gridder):
    c = dc.ACCURACY[6]                                    # fp32
    new = _comps2vis(gridder, c)
    rng = np.random.default_rng(5)
    old = (rng.standard_normal(new.shape) + 1j * rng.standard_normal(new.shape)).astype(np.complex64)
    out = dev(old)
    ret = _comps2vis(gridder, c, out=out, accumulate=True)
    assert ret is out
    got, want = out.cpu().numpy().astype(np.complex128), old.astype(np.complex128) + new
    for g, w in ((got.real, want.real), (got.imag, want.imag)):
        assert (np.abs(g - w) <= kc.U['f32'] * np.abs(w)).all()
    assert np.array_equal(out.cpu().numpy()[:, :, 1:-1], old[:, :, 1:-1])          # the middle correlations: untouched
    # without accumulate `out` is zeroed first: whatever it held, the fresh result's bits
    ret = _comps2vis(gridder, c, out=out)
    assert ret is out and np.array_equal(out.cpu().numpy().view(np.float32), new.view(np.float32))


def test_out_dtype_narrows_in_the_kernel(gridder):
    c = dc.ACCURACY[1]                                    # fp64
    wide = _comps2vis(gridder, c)
    narrow = _comps2vis(gridder, c, out_dtype=np.complex64)
    assert wide.dtype == np.complex128 and narrow.dtype == np.complex64 and narrow.shape == wide.shape
    for g, w in ((narrow.real.astype(np.float64), wide.real), (narrow.imag.astype(np.float64), wide.imag)):
        assert (np.abs(g - w) <= kc.U['f32'] * np.abs(w)).all()
    print("narrowed == astype(complex64) bit for bit:", np.array_equal(narrow, wide.astype(np.complex64)))
    # the worker's tail: vis (complex64) += model column of an fp64 model
    out = torch.ones(wide.shape, dtype=torch.complex64, device='cuda')
    _comps2vis(gridder, c, out=out, accumulate=True)
    want = 1.0 + wide
    got = out.cpu().numpy().astype(np.complex128)
    tol = 2 * kc.U['f32'] * (1.0 + np.abs(wide.real) + np.abs(wide.imag))
    assert (np.abs(got.real - want.real) <= tol).all() and (np.abs(got.imag - want.imag) <= tol).all()


# -------------------------------------------------------------------------------------------------------- plans
def test_predict_leaves_the_plan_cache_alone(gridder):
    c = wc.CASES[0]
    gridder.clear_plan_cache()
    kw = dict(npix_x=c['nx'], npix_y=c['ny'], pixsize_x=c['px'], pixsize_y=c['py'], do_wgridding=True)
    vis = c['vis'].astype(np.complex128)
    epsilons = [10.0 ** -(3 + 0.5 * k) for k in range(8)]         # eight plans: the cache is full
    for eps in epsilons:
        gridder.vis2dirty(c['uvw'], c['freq'], vis, epsilon=eps, **kw)
    before = dict(gridder.cache_stats)
    p = dc.ACCURACY[1]                                    # made for the 16 x 64 image
    nchan = 10
    freq = 1.0e9 * (1.0 + 0.01 * np.arange(nchan))
    cube = np.random.default_rng(3).standard_normal((nchan, 16, 64))
    got = gridder.im2vis(p['uvw'], freq, cube, 0.03, 0.008, np.arange(nchan), np.ones(nchan, np.int64), epsilon=1e-6)
    assert got.shape == (p['uvw'].shape[0], nchan) and got.all()
    assert gridder.cache_stats['miss'] == before['miss'] and gridder.cache_stats['tables'] == before['tables'] + 1
    for eps in epsilons:
        gridder.vis2dirty(c['uvw'], c['freq'], vis, epsilon=eps, **kw)
    assert gridder.cache_stats['miss'] == before['miss']
    gridder.clear_plan_cache()


# ------------------------------------------------------------------------------------------------- loc2psf_vis
def test_loc2psf_vis(gridder, npz):
    L = dc.LOC2PSF
    c = dc.GOLDEN[dc.GOLDEN_IDS.index(L['case'])]
    shape = (c['uvw'].shape[0], c['freq'].size)
    for precision, cdt in (('single', np.complex64), ('double', np.complex128)):
        ones = gridder.loc2psf_vis(c['uvw'], c['freq'], L['cell'], precision=precision)
        assert ones.dtype == cdt and np.array_equal(ones, np.ones(shape, cdt))
        for wg in (True, False):
            got = gridder.loc2psf_vis(c['uvw'], c['freq'], L['cell'], x0=L['x0'], y0=L['y0'], do_wgridding=wg,
                                      precision=precision)
            ref = npz[f"loc2psf_centre_{'wg' if wg else 'nowg'}"]
            err = wc.rel_l2(got.astype(np.complex128), ref)
            print(f"loc2psf_vis {precision} do_wgridding {wg}: rel_l2 {err:.3e}")
            assert got.dtype == cdt and got.shape == shape
            assert err <= 1e-7 + (kc.U['f32'] if precision == 'single' else 0.0)


# ------------------------------------------------------------------------------------------------------- errors
def test_errors(gridder):
    c = dc.GOLDEN[1]
    im = lambda **kw: gridder.im2vis(c['uvw'], c['freq'], c['cube'], c['px'], c['py'],                  # noqa: E731
                                     kw.pop('idx', c['fbin_idx']), kw.pop('cnts', c['fbin_cnts']), **_kw(c, **kw))
    with pytest.raises(NotImplementedError):
        im(flip_v=True)
    with pytest.raises(ValueError):
        im(cnts=np.array([2, 1, 4]))                     # reaches channel 7 of 6
    with pytest.raises(ValueError):
        im(cnts=np.array([2, -1, 3]))

    def call(**kw):
        z = dict(c, **{k: kw.pop(k) for k in list(kw) if k in c})
        args = dict(modelf=dc.modelf)
        args.update({k: kw.pop(k) for k in list(kw) if k in ('modelf',)})
        return gridder.comps2vis(z['uvw'], z['utime'], z['freq'], *dc.bins(z), z['comps'], z['Ix'], z['Iy'], args['modelf'],
                                 dc.tfunc, dc.ffunc, z['nx'], z['ny'], z['px'], z['py'], **_kw(z, **kw))
    out = torch.full(c['uvw'].shape[:1] + (c['freq'].size, 4), SENTINEL, dtype=torch.complex128, device='cuda')
    bad = [dict(tbin_cnts=np.array([3, 3])),                                 # beyond utime
           dict(utime=c['utime'][:-1]),
           dict(rbin_cnts=c['rbin_cnts'] + np.eye(1, c['rbin_cnts'].size, c['rbin_cnts'].size - 1, dtype=np.int64)[0]),
           dict(uvw=c['uvw'][:-1]),                                          # rows beyond uvw
           dict(fbin_cnts=np.array([2, 1, 4])),                              # beyond freq
           dict(freq=c['freq'][:-1]),
           dict(tbin_cnts=np.array([3, -2])), dict(fbin_cnts=np.array([2, -1, 3])),
           dict(rbin_cnts=-c['rbin_cnts']),
           dict(ncorr_out=0), dict(ncorr_out=5),
           dict(Ix=c['Ix'] + c['nx']), dict(Iy=-1 - c['Iy']),
           dict(modelf=dc.modelf_affine), dict(modelf=dc.modelf_quadratic)]
    for kw in bad:
        with pytest.raises(ValueError):
            call(out=out, **kw)
    assert (out == SENTINEL).all().item()                # each was refused before anything was written
    with pytest.raises(ValueError):                      # the kernel narrows, it does not widen
        gridder.comps2vis(c['uvw'], c['utime'], c['freq'], *dc.bins(c), c['comps'].astype(np.float32), c['Ix'], c['Iy'],
                          dc.modelf, dc.tfunc, dc.ffunc, c['nx'], c['ny'], c['px'], c['py'], epsilon=1e-4, out=out)
    assert (out == SENTINEL).all().item()
    ok = call(out=out)
    assert ok is out and _layout_ok(out.cpu().numpy(), 4) is None
