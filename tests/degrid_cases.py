"""
The predict step's contract: the case table of test_cpu_degrid.py / test_gpu_degrid.py, a numpy model of the
block mapping of comps2vis and im2vis, and fp64 references of the two kernels it adds.

blocks / render / model_comps2vis / model_im2vis
                      the mapping written from the reference's statements (pfb/operators/gridder.py:258-294, 492-548):
                      every index array shifted by its minimum, time bin -> rows, band -> channels, the component model
                      rendered at (tfunc(mean utime), ffunc(mean freq)) and degridded on the block uvw[indr], freq[indf].
                      `degrid` is wgrid_cases.direct_dirty2vis (the exact sum: THE reference of every accuracy test) or
                      wgrid_cases.model_dirty2vis (the recipe in numpy, which shows on the CPU that it meets epsilon on
                      every block).
ref_finish_block      pfb_wgrid_finish_block in fp64 with the per-component bound it is held to.
finish_block_like     the kernel's arithmetic imitated in numpy in the kernel's types, with seeded defects: what
                      test_cpu_degrid.py holds the bound against.
ref_restore_corrs     pfb_vis_restore_corrs (exact).
GOLDEN / ACCURACY     the tables.  tests/golden/make_golden_degrid.py runs the reference on GOLDEN.
"""
import numpy as np

import wgrid_cases as wc
import wgrid_kernel_cases as kc

T0, F0 = 4.0e9, 1.0e9


# ------------------------------------------------------------------------------------------- the worker's callables
def tfunc(t):
    return t / T0


def ffunc(f):
    return f / F0 - 1.0


def modelf(t, f, c0, c1, c2):
    """Linear in c0, c1, c2; with arrays for them it gives an array, as the reference calls it."""
    return c0 + c1 * f + c2 * t * f


def modelf_affine(t, f, c0, c1, c2):
    return 1.0 + c0 + c1 * f + c2 * t * f


def modelf_quadratic(t, f, c0, c1, c2):
    return c0 * c0 + c1 * f + c2 * t * f


# ------------------------------------------------------------------------------------------------------ cases
def make_predict(name, image, eps, seed, tcnts=(2, 1), rows=(3, 9), fcnts=(2, 1, 3), offsets=(0, 0, 0), ncomps=5,
                 dtype='f64', **kw):
    """A wgrid_cases case (uvw, freq, geometry, epsilon, flags) with the bins of a predict call on top: len(tcnts) time
    bins of tcnts[t] unique times, each unique time with rows[0] .. rows[1] rows, len(fcnts) bands of fcnts[b] channels;
    offsets = the minima of (tbin_idx, rbin_idx, fbin_idx).  ncomps components at distinct pixels, three parameters."""
    rng = np.random.default_rng(seed + 77)
    nutime = int(sum(tcnts))
    rcnts = rng.integers(rows[0], rows[1] + 1, nutime).astype(np.int64)
    nrow, nchan = int(rcnts.sum()), int(sum(fcnts))
    c = wc.make_case(name, image, eps, seed, nrow=nrow, nchan=nchan, dtype=dtype, **kw)
    start = lambda cnt: np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)        # noqa: E731
    c['utime'] = 4.0e9 + 8.0 * np.arange(nutime)
    c['tbin_idx'], c['tbin_cnts'] = start(tcnts) + offsets[0], np.asarray(tcnts, np.int64)
    c['rbin_idx'], c['rbin_cnts'] = start(rcnts) + offsets[1], rcnts
    c['fbin_idx'], c['fbin_cnts'] = start(fcnts) + offsets[2], np.asarray(fcnts, np.int64)
    nx, ny = c['nx'], c['ny']
    pix = rng.choice(nx * ny, size=ncomps, replace=False)
    c['Ix'], c['Iy'] = (pix // ny).astype(np.int64), (pix % ny).astype(np.int64)
    c['comps'] = rng.standard_normal((3, ncomps)) * np.array([[1.0], [0.5], [0.25]])
    c['cube'] = rng.standard_normal((len(fcnts), nx, ny))
    return c


def bins(c):
    return (c['rbin_idx'], c['rbin_cnts'], c['tbin_idx'], c['tbin_cnts'], c['fbin_idx'], c['fbin_cnts'])


def blocks(c):
    """[(t, b, r0, r1, c0, c1, tout, fout)] of a case, by the reference's statements."""
    rbin_idx2 = c['rbin_idx'] - c['rbin_idx'].min()
    tbin_idx2 = c['tbin_idx'] - c['tbin_idx'].min()
    fbin_idx2 = c['fbin_idx'] - c['fbin_idx'].min()
    out = []
    for t in range(c['tbin_idx'].size):
        indt = slice(tbin_idx2[t], tbin_idx2[t] + c['tbin_cnts'][t])
        r0, r1 = rbin_idx2[indt][0], rbin_idx2[indt][-1] + c['rbin_cnts'][indt][-1]
        for b in range(c['fbin_idx'].size):
            c0, c1 = fbin_idx2[b], fbin_idx2[b] + c['fbin_cnts'][b]
            out.append((t, b, int(r0), int(r1), int(c0), int(c1), tfunc(np.mean(c['utime'][indt])),
                        ffunc(np.mean(c['freq'][c0:c1]))))
    return out


def block_case(c, r0, r1, c0, c1):
    """The wgrid_cases case of one block: its rows and channels, no weights, no mask."""
    return dict(c, uvw=c['uvw'][r0:r1], freq=c['freq'][c0:c1], wgt=None, mask=None)


def time_bin_case(c, t):
    """The call the reference's worker makes: time bin t alone, with its rows and unique times (the bins keep their
    values: the callee shifts them by their minima)."""
    tbin_idx2 = c['tbin_idx'] - c['tbin_idx'].min()
    rbin_idx2 = c['rbin_idx'] - c['rbin_idx'].min()
    indt = slice(tbin_idx2[t], tbin_idx2[t] + c['tbin_cnts'][t])
    r0, r1 = rbin_idx2[indt][0], rbin_idx2[indt][-1] + c['rbin_cnts'][indt][-1]
    one = dict(c, uvw=np.ascontiguousarray(c['uvw'][r0:r1]), utime=c['utime'][indt], rbin_idx=c['rbin_idx'][indt],
               rbin_cnts=c['rbin_cnts'][indt], tbin_idx=c['tbin_idx'][t:t + 1], tbin_cnts=c['tbin_cnts'][t:t + 1])
    return one, int(r0), int(r1)


def render(c, tout, fout, comps=None):
    image = np.zeros((c['nx'], c['ny']))
    image[c['Ix'], c['Iy']] = modelf(tout, fout, *(c['comps'] if comps is None else comps).astype(np.float64))
    return image


def model_comps2vis(c, ncorr_out, degrid=wc.direct_dirty2vis, comps=None):
    """vis (nrow, nchan, ncorr_out) complex128; `comps` replaces the case's (the same rounded to fp32, say)."""
    vis = np.zeros((c['uvw'].shape[0], c['freq'].size, ncorr_out), complex)
    for t, b, r0, r1, c0, c1, tout, fout in blocks(c):
        if r1 > r0 and c1 > c0:
            vis[r0:r1, c0:c1, 0] = degrid(block_case(c, r0, r1, c0, c1), render(c, tout, fout, comps))
    if ncorr_out > 1:
        vis[:, :, -1] = vis[:, :, 0]
    return vis


def model_im2vis(c, cube, degrid=wc.direct_dirty2vis):
    nrow = c['uvw'].shape[0]
    vis = np.zeros((nrow, c['freq'].size), complex)
    f2 = c['fbin_idx'] - c['fbin_idx'].min()
    for i in range(cube.shape[0]):
        c0, c1 = int(f2[i]), int(f2[i] + c['fbin_cnts'][i])
        if c1 > c0:
            vis[:, c0:c1] = degrid(block_case(c, 0, nrow, c0, c1), cube[i])
    return vis


def block_errors(c, got, ref):
    """rel_l2 of every (time bin, band) block of a (nrow, nchan) result against the reference."""
    return [wc.rel_l2(got[r0:r1, c0:c1], ref[r0:r1, c0:c1]) for _, _, r0, r1, c0, c1, _, _ in blocks(c)
            if r1 > r0 and c1 > c0]


def band_errors(c, got, ref):
    f2 = c['fbin_idx'] - c['fbin_idx'].min()
    return [wc.rel_l2(got[:, a:a + n], ref[:, a:a + n]) for a, n in zip(f2, c['fbin_cnts']) if n]


# the reference's run, stored in tests/golden/degrid.npz: the mapping with non-zero minima and uneven counts (1, 3, 2) on
# the three images, centre, the two flags
GOLDEN = [
    make_predict('g-mapping', '6x8', 1e-7, 900, tcnts=(1, 3, 2), rows=(1, 3), fcnts=(1, 3, 2), offsets=(5, 100, 7),
                 wmax=20.0, divide_by_n=False),
    make_predict('g-32x24', '32x24', 1e-7, 901, tcnts=(3, 2), fcnts=(2, 1, 3), offsets=(5, 100, 7), wmax=20.0,
                 divide_by_n=False),
    make_predict('g-16x64-centre-n', '16x64', 1e-5, 902, tcnts=(2, 2), fcnts=(1, 2, 2), wmax=60.0, cx=-0.1, cy=0.03,
                 divide_by_n=True),
    make_predict('g-32x24-no-wgrid', '32x24', 1e-7, 903, tcnts=(2, 3), fcnts=(3, 1, 2), offsets=(0, 40, 2), wmax=20.0,
                 do_wgridding=False, divide_by_n=False),
]
GOLDEN_NCORR = {'g-mapping': 4, 'g-32x24': 2, 'g-16x64-centre-n': 1, 'g-32x24-no-wgrid': 4}
GOLDEN_IDS = [c['name'] for c in GOLDEN]
LOC2PSF = dict(case='g-mapping', cell=0.005, x0=0.02, y0=-0.03)          # the delta of loc2psf_vis on g-mapping's uvw, freq


# the accuracy cases of the GPU tests: 2 time bins x 3 bands; fp64 at 1e-5, 1e-7, 1e-9, fp32 at 1e-3 and EPS_MIN (1e-5);
# ncorr_out 1, 2, 4, both flags both ways, a centre, the three images; nrow <= 300, nchan <= 6
# The seeds are chosen on the CPU: with few components the recipe's own error depends on where they fall (the kernel
# correction is at its worst on the image's rim), and at 1e-9 it takes 0.47 .. 0.64 epsilon over five seed decades tried;
# this one keeps every block of every case below RECIPE_MARGIN (test_cpu_degrid.py asserts it)
def _accuracy(seed0=990):
    table = []
    spec = [('32x24', 1e-5, 'f64', 4, True, False, 0.0, 0.0, 20.0), ('16x64', 1e-7, 'f64', 2, True, True, 0.0, 0.0, 60.0),
            ('6x8', 1e-9, 'f64', 1, True, False, 0.0, 0.0, 20.0), ('32x24', 1e-7, 'f64', 4, False, False, 0.0, 0.0, 20.0),
            ('16x64', 1e-5, 'f64', 2, False, True, -0.1, 0.03, 20.0), ('32x24', 1e-9, 'f64', 1, True, True, 0.05, -0.08, 60.0),
            ('32x24', 1e-3, 'f32', 4, True, False, 0.0, 0.0, 20.0), ('16x64', 1e-5, 'f32', 2, True, True, 0.0, 0.0, 20.0),
            ('6x8', 1e-5, 'f32', 1, False, False, 0.05, 0.04, 20.0), ('32x24', 1e-3, 'f32', 2, True, True, 0.05, -0.08, 60.0)]
    for k, (image, eps, dtype, ncorr, wg, by_n, cx, cy, wmax) in enumerate(spec):
        name = f"{image}-{dtype}-eps{eps:g}-nc{ncorr}{'' if wg else '-nowg'}{'-n' if by_n else ''}{'-centre' if cx else ''}"
        c = make_predict(name, image, eps, seed0 + k, tcnts=(3, 2), rows=(20, 40), fcnts=(2, 1, 3),
                         offsets=(k % 2 * 3, k % 3 * 50, k % 2 * 7), dtype=dtype, wmax=wmax, do_wgridding=wg,
                         divide_by_n=by_n, cx=cx, cy=cy)
        c['ncorr_out'] = ncorr
        table.append(c)
    return table


ACCURACY = _accuracy()
ACCURACY_IDS = [c['name'] for c in ACCURACY]
RECIPE_MARGIN = 0.6           # the numpy recipe stays below this fraction of epsilon on every block of every case


# ------------------------------------------------------------------------------------------ the two kernels, fp64
NP_C = {'f32': np.complex64, 'f64': np.complex128}


def cells_of(idx, nchan_blk, row0, nchan_out, chan0, ncorr):
    """Flat indices into (nrow_out, nchan_out, ncorr) of correlation 0 of every slot."""
    idx = np.asarray(idx, np.int64)
    r, c = idx // nchan_blk, idx % nchan_blk
    return ((row0 + r) * nchan_out + chan0 + c) * ncorr


def ref_finish_block(geom, acc, idx, coord, nchan_blk, out0, out_tag, row0, chan0, accumulate, C=None):
    """(out, B, written): the contract of pfb_wgrid_finish_block in fp64 on out0 (nrow_out, nchan_out, ncorr), what each
    cell may differ by per component (B complex: its real part bounds the real part), and the mask of written cells.
    B = C U_T S, the rounding of the phase product of wgrid_kernel_cases.ref_finish (the same arithmetic: one phase
    factor), + U_O |v| where the output type is narrower than the plan's (one rounding), + U_O (|old| + |v| + the former
    two) with accumulate (one rounding of the sum).  B is zero where nothing is written: those cells keep their bits."""
    tdt = geom['dtype']
    C = kc.TOLERANCE_C['finish'][tdt] if C is None else C
    nrow_out, nchan_out, ncorr = out0.shape
    v, S = kc.ref_finish(geom, acc, None, np.arange(acc.size), coord, acc.size)        # per slot
    bound = C * kc.U[tdt] * S
    absv = np.abs(v.real) + 1j * np.abs(v.imag)
    if out_tag != tdt:
        bound = bound + kc.U[out_tag] * absv
    out = out0.astype(np.complex128).reshape(-1).copy()
    B = np.zeros(out.size, complex)
    written = np.zeros(out.size, bool)
    base = cells_of(idx, nchan_blk, row0, nchan_out, chan0, ncorr)
    for k in ((0,) if ncorr == 1 else (0, ncorr - 1)):
        cell = base + k
        old = out[cell]
        if accumulate:
            B[cell] = bound + kc.U[out_tag] * (np.abs(old.real) + 1j * np.abs(old.imag) + absv + bound)
            out[cell] = old + v
        else:
            B[cell] = bound
            out[cell] = v
        written[cell] = True
    return out.reshape(out0.shape), B.reshape(out0.shape), written.reshape(out0.shape)


DEFECTS = ('row0_dropped', 'chan0_dropped', 'last_corr_at_1', 'mod_nchan_out', 'accumulate_overwrites')


def finish_block_like(geom, acc, idx, coord, nchan_blk, out0, out_tag, row0, chan0, accumulate, defect=None):
    """What the kernel computes, imitated in numpy in its types: the phase product rounded to the plan's type, cast to
    the output's type, stored or added there.  `defect` seeds one of DEFECTS, or 'add_before_cast'."""
    tdt = geom['dtype']
    nrow_out, nchan_out, ncorr = out0.shape
    v = kc.ref_finish(geom, acc, None, np.arange(acc.size), coord, acc.size)[0].astype(NP_C[tdt])
    idx = np.asarray(idx, np.int64)
    r = idx // nchan_blk
    c = idx % (nchan_out if defect == 'mod_nchan_out' else nchan_blk)
    base = (((0 if defect == 'row0_dropped' else row0) + r) * nchan_out + (0 if defect == 'chan0_dropped' else chan0)
            + c) * ncorr
    out = out0.astype(NP_C[out_tag]).reshape(-1).copy()
    last = 1 if defect == 'last_corr_at_1' else ncorr - 1
    for k in ((0,) if ncorr == 1 else (0, last)):
        cell = base + k
        if accumulate and defect == 'add_before_cast':
            out[cell] = (out[cell].astype(NP_C[tdt]) + v).astype(NP_C[out_tag])
        elif accumulate and defect != 'accumulate_overwrites':
            out[cell] = out[cell] + v.astype(NP_C[out_tag])
        else:
            out[cell] = v.astype(NP_C[out_tag])
    return out.reshape(out0.shape)


def excess(got, ref, B):
    """max over cells and components of |got - ref| / B; inf where a cell with B = 0 differs from ref in any bit."""
    got, ref = np.asarray(got, np.complex128), np.asarray(ref, np.complex128)
    worst = 0.0
    for d, b in ((np.abs(got.real - ref.real), B.real), (np.abs(got.imag - ref.imag), B.imag)):
        if d[b == 0].any():
            return np.inf
        on = b > 0
        if on.any():
            worst = max(worst, float((d[on] / b[on]).max()))
    return worst


def ref_restore_corrs(vis, ncorr):
    out = np.zeros(vis.shape + (ncorr,), vis.dtype)
    out[..., 0] = vis
    out[..., ncorr - 1] = vis
    return out


def finish_data(nsorted, nchan_blk, dtype, centre, skip, seed):
    """geom, acc, idx, coord of a finish_block entry: nsorted slots of a block with nchan_blk channels.  With `skip` the
    order leaves visibilities out (a masked plan: every third of the block's is absent); idx is a permutation."""
    cx, cy = (0.05, -0.08) if centre else (0.0, 0.0)
    geom = kc.geometry(dtype, 34, 26, 6, nplanes=10, w0=-4.0, dw=1.5, cx=cx, cy=cy)
    rng = np.random.default_rng(seed)
    nvis = nsorted + (nsorted + 1) // 2 if skip else nsorted
    nvis = -(-nvis // nchan_blk) * nchan_blk                       # whole rows
    if not skip and nvis != nsorted:
        skip = True                                                # nsorted no multiple of nchan_blk: the last row is partial
    live = np.sort(rng.choice(nvis, size=nsorted, replace=False)) if skip else np.arange(nvis)
    idx = rng.permutation(live).astype(np.int32)
    # inside the grid, as an order's coordinates are: the phase's argument stays within the few turns that
    # TOLERANCE_C['finish'] was recorded at
    coord = np.stack([rng.uniform(-0.5, 0.5, nsorted) * geom['Nu'], rng.uniform(-0.5, 0.5, nsorted) * geom['Nv'],
                      rng.uniform(0.0, 9.0, nsorted)])
    acc = rng.standard_normal(nsorted) + 1j * rng.standard_normal(nsorted)
    return geom, acc, idx, coord, nvis // nchan_blk
