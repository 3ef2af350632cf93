"""
The kernels of csrc/wgrid.hip one by one on the MI355X, through the C ABI, against the numpy fp64 references of
tests/wgrid_kernel_cases.py (tests/test_cpu_wgrid_kernel_cases.py proves the references and the tables on the CPU):
every support 4 .. 12 in both types -- the fp32 footprint kernels of W >= 8 are public ABI that gridder.EPS_MIN keeps
Python away from --, grids as narrow as the footprint, slot counts around a block of 256 lanes, slot ranges inside the
order, planes where the w weight is exactly zero, images of npix % 256 != 0, and sort-key tiles of 16, 32 and 64 cells
with a partial last tile.

Bounds
  order          integers and fp64 coordinates: exact.  keys and histogram equal the reference; idx is a permutation of
                 the unmasked visibilities with non-decreasing keys; coord holds the coordinates of idx bit for bit.
  every other    per element and component |got - ref| <= C U S: U the unit roundoff of the data type (2^-24, 2^-53), S
  entry point    the reference's sum over absolute values (wgrid_kernel_cases), C = TOLERANCE_C[entry point][type].
                 Where S is zero the result is exactly zero.  Inputs are rounded to the data type BEFORE the reference
                 sees them.  pfb_wgrid_degrid adds to acc and pfb_wgrid_image_adjoint to img: |target| is part of S.
  adjointness    fp64, sum_cells grid(val) G against sum_slots val degrid(G) (the weights are real: bilinear, no
                 conjugate), to U (C_grid sum S_grid |G| + C_degrid sum |val| S_degrid).

C was not guessed: the suite ran once with C = inf, recording max |got - ref| / (U S) per entry point and type
(check() below still records and test_zz_report prints the table), and C is 4 x the worst figure rounded up to a power
of two.  Recorded on the MI355X (worst over every table entry):

                    fp32 figure -> C        fp64 figure -> C
    grid            1024.0 -> 8192           449.9 -> 2048     (W = 8, 34 x 26, the last plane, both types: a cell that
                                                                only one edge tap of a slot at the rim of the w kernel
                                                                reaches; every other entry: 457 / 322)
    degrid           163   -> 1024            48.3 ->  256     (W = 5 plane 0; W = 12 last plane)
    prep               2.14 ->  16            38.1 ->  256     (fp64: the centre phase, 2 pi x 3 turns of argument)
    finish             1.59 ->   8            32.1 ->  256
    weight             0.99 ->   4             0   ->    1
    image_forward      0.97 ->   4             2.95 ->  16
    image_adjoint      1.80 ->   8             2.45 ->  16
    image_correct      0.99 ->   4             0   ->    1

  The footprint kernels' figures are not summation error: phi(x) = exp(2.3 W (sqrt(1 - x^2) - 1)) evaluated in the data
  type has the relative error 2.3 W U / sqrt(1 - x^2) near |x| = 1, unbounded at the rim where phi itself is
  exp(-2.3 W); a cell or slot whose only contribution is such a tap shows all of it.  The fp32 kernels of W >= 8, which
  Python never launches, measure like the others: grid 1024 (W = 8) and 257 - 364 at W = 9 .. 12, degrid 49 - 153.

tests/test_cpu_wgrid_kernel_cases.py holds C against five defects (>= 16 C each).

Not reachable or not detectable
  - the dropped last footprint row in fp32 at W > 8 in pfb_wgrid_degrid (the tap is of the order of U; the fp64 build of
    the same template is held to the bound, and pfb_wgrid_grid shows it in cells that only a last row reaches);
  - the order of the slots within one key (the arrival order of the lanes; any permutation is right);
  - a grid of exactly W cells at W = 5, 6, 9, 10 and of W + 1 at 5 and 9: nx must be even, the narrowest grid is
    4 ceil(W / 4) cells.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import wgrid_cases as wc
import wgrid_kernel_cases as kc

pytestmark = pytest.mark.gpu
pmp = pytest.mark.parametrize

RDT = {'f32': torch.float32, 'f64': torch.float64}
CDT = {'f32': torch.complex64, 'f64': torch.complex128}
NAN = float('nan')
SENTINEL = 7.25

_worst = {}


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

    def run(self, name, *args):
        args = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
        assert getattr(self.lib, 'pfb_wgrid_' + name)(self.h, *args, torch.cuda.current_stream().cuda_stream) == self.ok


def dev(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype).contiguous()


def host(t):
    """A device tensor as fp64 / complex128 numpy."""
    a = t.cpu().numpy()
    return a.astype(np.complex128 if np.iscomplexobj(a) else np.float64)


def full(shape, value, dtype):
    return torch.full(shape, value, dtype=dtype, device='cuda')


def figure(got, ref, S):
    """max over elements and components of |got - ref| / S (in units of 1, not of U); exact where S is zero."""
    worst = 0.0
    got, ref, S = (np.asarray(a, dtype=np.complex128) for a in (got, ref, S))
    assert np.isfinite(got.real).all() and np.isfinite(got.imag).all()
    for d, s in ((np.abs(got.real - ref.real), S.real), (np.abs(got.imag - ref.imag), S.imag)):
        on = s > 0
        assert not d[~on].any(), "a value with no contribution is not exactly zero"
        if on.any():
            worst = max(worst, float((d[on] / s[on]).max()))
    return worst


def check(name, dtype, got, ref, S, what=''):
    r = figure(got, ref, S) / kc.U[dtype]
    _worst[name, dtype] = max(_worst.get((name, dtype), 0.0), r)
    print(f"{name} {dtype} {what}: |got - ref| / (U S) = {r:.3g} (C = {kc.TOLERANCE_C[name][dtype]:g})")
    assert r <= kc.TOLERANCE_C[name][dtype], (name, dtype, what, r)


# --------------------------------------------------------------------------------------------------------- order
@pmp('entry', kc.ORDER, ids=kc.ORDER_IDS)
def test_order(lib, entry):
    geom, uvw, freq, mask = kc.order_data(entry)
    nrow, nchan = entry['nrow'], entry['nchan']
    nvis = nrow * nchan
    ref_keys, ref_hist = kc.ref_keys(geom, uvw, freq, mask)
    ref_idx, ref_coord, ref_off = kc.ref_order(geom, uvw, freq, mask)
    with Plan(lib, geom) as plan:
        nkeys, np0, tile = C.c_int(), C.c_int(), C.c_int()
        assert lib.pfb_wgrid_plan_info(plan.h, C.byref(nkeys), C.byref(np0), C.byref(tile)) == plan.ok
        assert (nkeys.value, np0.value, tile.value) == (geom['nkeys'], geom['np0'], geom['tile'])
        nbytes = lib.pfb_wgrid_work_bytes(plan.h)
        assert nbytes == 8 * geom['nkeys']
        work = full((nbytes,), 0xA5, torch.uint8)                 # the launcher clears it
        keys = full((nvis,), -7, torch.int32)
        uvw_d, freq_d, mask_d = dev(uvw), dev(freq), dev(mask)
        plan.run('order_count', uvw_d, freq_d, mask_d, nrow, nchan, keys, work)
        counts = work[:4 * geom['nkeys']].view(torch.int32)
        got_keys = keys.cpu().numpy()
        assert np.array_equal(got_keys, ref_keys) and np.array_equal(counts.cpu().numpy(), ref_hist)
        live = got_keys >= 0
        assert got_keys[live].max() < geom['nkeys'] and (got_keys[~live] == -1).all()
        # the caller's scan, as gridder.WgridPlan._build_order does it
        offsets = torch.zeros(geom['nkeys'] + 1, dtype=torch.int64, device='cuda')
        offsets[1:] = torch.cumsum(counts, 0, dtype=torch.int64)
        plane_off = offsets[::geom['nkeys'] // geom['np0']].cpu().tolist()
        assert plane_off == list(ref_off) and len(plane_off) == geom['np0'] + 1
        nsorted = plane_off[-1]
        assert nsorted == live.sum() >= 1
        idx = full((nsorted,), -1, torch.int32)
        coord = full((3, nsorted), NAN, torch.float64)
        plan.run('order_fill', uvw_d, freq_d, nrow, nchan, keys, offsets, work, nsorted, idx, coord)
        got_idx, got_coord = idx.cpu().numpy(), coord.cpu().numpy()
    assert np.array_equal(np.sort(got_idx), np.flatnonzero(live))
    assert (np.diff(ref_keys[got_idx]) >= 0).all()
    want = np.stack([c[got_idx] for c in kc.vis_coords(geom, uvw, freq)])
    assert np.array_equal(got_coord.view(np.int64), want.view(np.int64))          # bit for bit
    # the same multiset of slots per key as the reference's stable sort
    assert np.array_equal(ref_keys[got_idx], ref_keys[ref_idx])


# ----------------------------------------------------------------------------------------------- footprint kernels
def rounded(a, dtype):
    """numpy complex128 / float64 values rounded to the data type (what the device is handed)."""
    if np.iscomplexobj(a):
        return a.astype(np.complex64 if dtype == 'f32' else np.complex128).astype(np.complex128)
    return a.astype(np.float32 if dtype == 'f32' else np.float64).astype(np.float64)


@pmp('entry', kc.FOOT, ids=kc.FOOT_IDS)
def test_grid(lib, entry):
    geom, n, s0, s1 = entry['geom'], entry['n'], entry['s0'], entry['s1']
    dtype = geom['dtype']
    coord, val, _ = kc.foot_data(entry)
    val = rounded(val, dtype)
    poisoned = np.full(n, NAN + 1j * NAN)
    poisoned[s0:s1] = val[s0:s1]                                   # nothing outside [s0, s1) may be read
    val_d, coord_d = dev(poisoned, CDT[dtype]), dev(coord)
    with Plan(lib, geom) as plan:
        for plane in entry['planes']:
            ref, S = kc.ref_grid_plane(geom, coord, val, plane, s0, s1)
            runs = []
            for _ in range(2):
                grid = full((geom['Nu'], geom['Nv']), NAN, CDT[dtype])        # "grid = 0, then"
                plan.run('grid', plane, val_d, coord_d, n, s0, s1, grid)
                runs.append(host(grid))
                assert not np.isnan(runs[-1].view(np.float64)).any()
            check('grid', dtype, runs[0], ref, S, f"{entry['id']} plane {plane}")
            check('grid', dtype, runs[1], runs[0], S, f"{entry['id']} plane {plane}, second run")


@pmp('entry', kc.FOOT, ids=kc.FOOT_IDS)
def test_degrid(lib, entry):
    geom, n, s0, s1 = entry['geom'], entry['n'], entry['s0'], entry['s1']
    dtype = geom['dtype']
    coord, _, grid = kc.foot_data(entry)
    grid = rounded(grid, dtype)
    grid_d, coord_d = dev(grid, CDT[dtype]), dev(coord)
    inside = np.zeros(n, bool)
    inside[s0:s1] = True
    with Plan(lib, geom) as plan:
        for plane in entry['planes']:
            ref, S = kc.ref_degrid_plane(geom, coord, grid, plane, s0, s1)
            runs = []
            for _ in range(2):
                acc = full((n,), SENTINEL, CDT[dtype])
                plan.run('degrid', plane, grid_d, coord_d, n, s0, s1, acc)
                runs.append(acc.cpu().numpy())
            assert np.array_equal(runs[0].view(runs[0].real.dtype), runs[1].view(runs[1].real.dtype))   # no atomics
            got = runs[0].astype(np.complex128)
            assert (got[~inside] == SENTINEL).all() and not got[~inside].imag.any()
            # acc += sum: the target is part of the scale
            check('degrid', dtype, got[inside], SENTINEL + ref[inside], SENTINEL + S[inside], f"{entry['id']} plane {plane}")
            reached = kc.footprint(geom, coord, plane, s0, s1)['ww'] != 0
            assert (got[inside][~reached] == SENTINEL).all()          # a slot that does not reach the plane is skipped


@pmp('entry', [e for e in kc.FOOT if e['geom']['dtype'] == 'f64'],
     ids=[e['id'] for e in kc.FOOT if e['geom']['dtype'] == 'f64'])
def test_grid_and_degrid_are_adjoint(lib, entry):
    geom, n, s0, s1 = entry['geom'], entry['n'], entry['s0'], entry['s1']
    coord, val, G = kc.foot_data(entry)
    val[:s0] = 0.0
    val[s1:] = 0.0
    val_d, G_d, coord_d = dev(val), dev(G), dev(coord)
    Cg, Cd = kc.TOLERANCE_C['grid']['f64'], kc.TOLERANCE_C['degrid']['f64']
    mod = lambda S: S.real + S.imag        # noqa: E731
    with Plan(lib, geom) as plan:
        for plane in entry['planes']:
            grid = full((geom['Nu'], geom['Nv']), NAN, torch.complex128)
            acc = torch.zeros(n, dtype=torch.complex128, device='cuda')
            plan.run('grid', plane, val_d, coord_d, n, s0, s1, grid)
            plan.run('degrid', plane, G_d, coord_d, n, s0, s1, acc)
            lhs, rhs = (host(grid) * G).sum(), (val * host(acc)).sum()
            Sg = kc.ref_grid_plane(geom, coord, val, plane, s0, s1)[1]
            Sd = kc.ref_degrid_plane(geom, coord, G, plane, s0, s1)[1]
            scale = (mod(Sg) * np.abs(G)).sum(), (np.abs(val) * mod(Sd)).sum()
            r = abs(lhs - rhs) / (kc.U['f64'] * sum(scale))
            print(f"{entry['id']} plane {plane}: |<grid val, G> - <val, degrid G>| / (U sum S) = {r:.3g}")
            assert abs(lhs - rhs) <= kc.U['f64'] * (Cg * scale[0] + Cd * scale[1])


# ---------------------------------------------------------------------------------------------------- slot kernels
@pmp('entry', kc.SLOT, ids=kc.SLOT_IDS)
def test_slot_kernels(lib, entry):
    d = kc.slot_data(entry)
    geom, dtype, idx, coord, nvis = d['geom'], entry['dtype'], d['idx'], d['coord'], d['nvis']
    ns = idx.size
    vis, acc = rounded(d['vis'], dtype), rounded(d['acc'], dtype)
    wgt = None if d['wgt'] is None else rounded(d['wgt'], dtype)
    vis_d, acc_d, wgt_d = dev(vis, CDT[dtype]), dev(acc, CDT[dtype]), dev(wgt, RDT[dtype])
    idx_d, coord_d = dev(idx), dev(coord)
    with Plan(lib, geom) as plan:
        val = full((ns,), NAN, CDT[dtype])
        plan.run('prep', vis_d, wgt_d, idx_d, coord_d, ns, val)
        check('prep', dtype, host(val), *kc.ref_prep(geom, vis, wgt, idx, coord), entry['id'])
        out = full((nvis,), NAN, CDT[dtype])                                    # "vis = 0, then"
        plan.run('finish', acc_d, wgt_d, idx_d, coord_d, ns, out, nvis)
        got = host(out)
        off = np.ones(nvis, bool)
        off[idx] = False
        assert off.sum() == nvis - ns > 0 and not got[off].any()
        check('finish', dtype, got, *kc.ref_finish(geom, acc, wgt, idx, coord, nvis), entry['id'])
        val = full((ns,), NAN, CDT[dtype])
        plan.run('weight', acc_d, wgt_d, idx_d, ns, val)
        check('weight', dtype, host(val), *kc.ref_weight(acc, wgt, idx), entry['id'])


# --------------------------------------------------------------------------------------------------- image kernels
@pmp('entry', kc.IMAGE, ids=kc.IMAGE_IDS)
def test_image_kernels(lib, entry):
    geom, plane = entry['geom'], entry['plane']
    dtype, nx, ny = geom['dtype'], geom['nx'], geom['ny']
    d = kc.image_data(entry)
    dirty, grid, img = rounded(d['dirty'], dtype), rounded(d['grid'], dtype), rounded(d['img'], dtype)
    beam = None if d['beam'] is None else rounded(d['beam'], dtype)
    corr, nm1 = d['corr'], d['nm1']
    corr_d, nm1_d, beam_d = dev(corr), dev(nm1), dev(beam, RDT[dtype])
    with Plan(lib, geom) as plan:
        out = full((geom['Nu'], geom['Nv']), NAN, CDT[dtype])                   # "grid = 0, then"
        plan.run('image_forward', plane, dev(dirty, RDT[dtype]), beam_d, corr_d, nm1_d, out)
        ref, S = kc.ref_image_forward(geom, dirty, beam, corr, nm1, plane)
        got = host(out)
        window = np.zeros(got.shape, bool)
        window[kc._window(geom)] = True
        assert window.sum() == nx * ny and not got[~window].any()               # exact zeros outside the window
        check('image_forward', dtype, got, ref, S, entry['id'])
        acc = dev(img, CDT[dtype])
        plan.run('image_adjoint', plane, dev(grid, CDT[dtype]), nm1_d, acc)
        check('image_adjoint', dtype, host(acc), *kc.ref_image_adjoint(geom, grid, nm1, plane, img), entry['id'])
        res = full((nx, ny), NAN, RDT[dtype])
        plan.run('image_correct', dev(img, CDT[dtype]), corr_d, beam_d, res)
        check('image_correct', dtype, host(res), *kc.ref_image_correct(img, corr, beam), entry['id'])


# ------------------------------------------------------------------------------- end to end, fp32 at the first rung
def test_fp32_at_the_smallest_support():
    """Single precision at epsilon = 1e-2 (W = 4, the first rung of the support dispatch) against the direct sum."""
    from pfb_clean_amd.operators.gridder import vis2dirty, dirty2vis
    case = wc.as_f32(wc.CASES[wc.CASE_IDS.index('34x26-eps0.01')])
    assert wc.support(case['eps']) == 4
    kw = dict(pixsize_x=case['px'], pixsize_y=case['py'], center_x=case['cx'], center_y=case['cy'], epsilon=case['eps'],
              do_wgridding=case['do_wgridding'], divide_by_n=case['divide_by_n'])
    got_d = vis2dirty(case['uvw'], case['freq'], case['vis'], wgt=case['wgt'], mask=case['mask'], npix_x=case['nx'],
                      npix_y=case['ny'], **kw)
    got_v = dirty2vis(case['uvw'], case['freq'], case['dirty'], wgt=case['wgt'], mask=case['mask'], **kw)
    assert got_d.dtype == np.float32 and got_v.dtype == np.complex64 and not got_v[case['mask'] == 0].any()
    e1 = wc.rel_l2(got_d.astype(np.float64), wc.direct_vis2dirty(case, case['vis']))
    e2 = wc.rel_l2(got_v.astype(np.complex128), wc.direct_dirty2vis(case, case['dirty']))
    print(f"fp32 eps 1e-2: vis2dirty {e1:.3e} dirty2vis {e2:.3e}")
    assert e1 <= case['eps'] and e2 <= case['eps']


def test_zz_report():
    """The figures C is derived from, as this run recorded them (run with -s to read them)."""
    for (name, dtype), r in sorted(_worst.items()):
        print(f"recorded {name:14s} {dtype}: {r:10.3f}   C = {kc.TOLERANCE_C[name][dtype]:g}")
