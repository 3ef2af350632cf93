"""
The kernels of csrc/wgrid.hip one by one: a plain numpy fp64 reference per entry point, written from the contract in
include/pfb_hip.h ("w-gridder"), and the geometry tables of test_cpu_wgrid_kernel_cases.py / test_gpu_wgrid_kernels.py.

geometry(...)          the record pfb_wgrid_plan_create derives: grid, tile rule, first planes, keys.
ref_keys / ref_order   the sort key of every visibility (-1 where masked) with its histogram, and the order a stable sort
                       of the keys gives (the device's order within one key is the arrival order: any permutation).
footprint / ref_grid_plane / ref_degrid_plane
                       one plane of gridding and of degridding over the slots [s0, s1), with the w weight
                       phi((plane - pg) / h) and its exact zero.
ref_prep / ref_finish / ref_weight, ref_image_forward / ref_image_adjoint / ref_image_correct
                       the slot and image kernels.
Every ref_* returns (value, S): S is the same sum over absolute values -- the reference applied to |Re| and |Im| of its
data, with |factor| for every real factor, |Re| + |Im| on both components where a phase turns the value (_turned), and
with |target| added where the entry point accumulates onto its target.  It is
what a rounding bound multiplies: the GPU tests assert |got - ref| <= C[entry][type] * U[type] * S per element and per
component (S of a complex value is complex: its real part scales the real part).

TOLERANCE_C            the constants C, measured on the MI355X (test_gpu_wgrid_kernels.py has the figures).
FOOT / ORDER / IMAGE / SLOT   the tables; tests/test_cpu_wgrid_kernel_cases.py proves each entry has its property.

The grid can be as narrow as the footprint only where that leaves nx even: 2 nx = 4 ceil(W / 4), which is W itself at
W = 4, 8, 12, W + 1 at 7 and 11, and W + 2 or W + 3 at 5, 6, 9, 10.
"""
import numpy as np

from wgrid_cases import C_LIGHT, phi

U = {'f32': 2.0 ** -24, 'f64': 2.0 ** -53}
WG_BLOCK = 256
WG_MAX_TILES = 4096

# C[entry point][type]: 4 x the worst |got - ref| / (U S) recorded on the MI355X over every table entry, rounded up to a
# power of two (the recorded figures: docstring of test_gpu_wgrid_kernels.py).  The two fp64 entries that
# recorded 0 -- one real product, which numpy rounds the same way -- get 1: one rounding
TOLERANCE_C = {
    'grid': {'f32': 8192.0, 'f64': 2048.0},
    'degrid': {'f32': 1024.0, 'f64': 256.0},
    'prep': {'f32': 16.0, 'f64': 256.0},
    'finish': {'f32': 8.0, 'f64': 256.0},
    'weight': {'f32': 4.0, 'f64': 1.0},
    'image_forward': {'f32': 4.0, 'f64': 16.0},
    'image_adjoint': {'f32': 8.0, 'f64': 16.0},
    'image_correct': {'f32': 4.0, 'f64': 1.0},
}


# ---------------------------------------------------------------------------------------------------- the record
def geometry(dtype, nx, ny, W, nplanes=1, w0=0.0, dw=1.0, px=0.012, py=0.03, cx=0.0, cy=0.0):
    """What pfb_wgrid_plan_create keeps and derives (the tile edge doubles from 16 until at most 4096 tiles remain)."""
    assert nx % 2 == 0 and ny % 2 == 0 and 2 * nx >= W and 2 * ny >= W and (nplanes == 1 or nplanes > W)
    Nu, Nv = 2 * nx, 2 * ny
    tile = 16
    while ((Nu + tile - 1) // tile) * ((Nv + tile - 1) // tile) > WG_MAX_TILES:
        tile *= 2
    ntu, ntv = (Nu + tile - 1) // tile, (Nv + tile - 1) // tile
    np0 = nplanes - W + 1 if nplanes > 1 else 1
    return dict(dtype=dtype, nx=nx, ny=ny, Nu=Nu, Nv=Nv, W=W, h=0.5 * W, nplanes=nplanes, np0=np0, tile=tile, ntu=ntu,
                ntv=ntv, nkeys=np0 * ntu * ntv, px=px, py=py, cx=cx, cy=cy, w0=w0, dw=dw if nplanes > 1 else 1.0,
                wk=nplanes > 1)


def plane_w(geom, plane):
    return geom['w0'] + plane * (geom['dw'] if geom['wk'] else 0.0)


def first(g, h):
    return np.ceil(g - h)


def wrap(a0, N):
    m = a0 - N * np.floor(a0 / N)
    return np.clip(m.astype(np.int64), 0, N - 1)


# ----------------------------------------------------------------------------------------------------- the order
def vis_coords(geom, uvw, freq):
    """(ug, vg, pg) of visibility t = r nchan + k, by the expressions of the device: mul, div, mul (sub, div)."""
    nchan = freq.size
    r = np.arange(uvw.shape[0] * nchan) // nchan
    f = freq[np.arange(uvw.shape[0] * nchan) % nchan]
    su, sv = geom['px'] * geom['Nu'], geom['py'] * geom['Nv']
    ug = uvw[r, 0] * f / C_LIGHT * su
    vg = uvw[r, 1] * f / C_LIGHT * sv
    pg = (uvw[r, 2] * f / C_LIGHT - geom['w0']) / geom['dw'] if geom['wk'] else np.zeros_like(ug)
    return ug, vg, pg


def ref_keys(geom, uvw, freq, mask):
    """keys (nvis,) int32, -1 where masked, and their histogram (nkeys,)."""
    ug, vg, pg = vis_coords(geom, uvw, freq)
    h = geom['h']
    a, b = wrap(first(ug, h), geom['Nu']), wrap(first(vg, h), geom['Nv'])
    p0 = np.zeros(ug.size, np.int64)
    if geom['wk']:
        p = first(pg, h)
        top = geom['np0'] - 1
        p0 = np.where(p > 0.0, np.where(p < top, p, top), 0).astype(np.int64)          # the clamp, both sides
    keys = p0 * (geom['ntu'] * geom['ntv']) + (a // geom['tile']) * geom['ntv'] + b // geom['tile']
    if mask is not None:
        keys = np.where(mask.reshape(-1) != 0, keys, -1)
    hist = np.bincount(keys[keys >= 0], minlength=geom['nkeys'])
    return keys.astype(np.int32), hist


def ref_order(geom, uvw, freq, mask):
    """(idx, coord (3, nsorted), plane_off (np0 + 1)) of the stable sort by key."""
    keys, hist = ref_keys(geom, uvw, freq, mask)
    live = np.flatnonzero(keys >= 0)
    idx = live[np.argsort(keys[live], kind='stable')].astype(np.int32)
    coord = np.stack([c[idx] for c in vis_coords(geom, uvw, freq)]) if idx.size else np.zeros((3, 0))
    offsets = np.concatenate([[0], np.cumsum(hist)])
    return idx, coord, offsets[::geom['nkeys'] // geom['np0']]


def plane_ranges(geom, plane_off):
    """(plane, s0, s1) as gridder.WgridPlan.plane_ranges reads them off the offsets."""
    W, np0 = geom['W'], geom['np0']
    for p in range(geom['nplanes']):
        s0, s1 = plane_off[max(0, p - W + 1)], plane_off[min(p, np0 - 1) + 1]
        if s1 > s0:
            yield p, int(s0), int(s1)


# ------------------------------------------------------------------------------------------- the footprint kernels
def footprint(geom, coord, plane, s0, s1):
    """Of the slots [s0, s1) on `plane`: w weight (n,), row and column kernel values (n, W), rows and columns (n, W)."""
    W, h = geom['W'], geom['h']
    ug, vg, pg = coord[0, s0:s1], coord[1, s0:s1], coord[2, s0:s1]
    ww = phi((plane - pg) / h, W) if geom['wk'] else np.ones_like(ug)
    a0, b0 = first(ug, h), first(vg, h)
    k = np.arange(W)
    fu = phi((a0[:, None] + k - ug[:, None]) / h, W)
    fv = phi((b0[:, None] + k - vg[:, None]) / h, W)
    rows = (wrap(a0, geom['Nu'])[:, None] + k) % geom['Nu']
    cols = (wrap(b0, geom['Nv'])[:, None] + k) % geom['Nv']
    return dict(ww=ww, fu=fu, fv=fv, rows=rows, cols=cols)


def _absc(z):
    return np.abs(z.real) + 1j * np.abs(z.imag)


def ref_grid_plane(geom, coord, val, plane, s0, s1, fp=None):
    """grid (Nu, Nv) = the slots [s0, s1) of val spread on `plane`; nothing outside the range is read."""
    fp = footprint(geom, coord, plane, s0, s1) if fp is None else fp
    out = []
    for v in (val[s0:s1].astype(np.complex128), _absc(val[s0:s1].astype(np.complex128))):
        grid = np.zeros((geom['Nu'], geom['Nv']), complex)
        contrib = (v * fp['ww'])[:, None, None] * fp['fu'][:, :, None] * fp['fv'][:, None, :]
        np.add.at(grid, (fp['rows'][:, :, None], fp['cols'][:, None, :]), contrib)
        out.append(grid)
    return out[0], out[1]


def ref_degrid_plane(geom, coord, grid, plane, s0, s1, fp=None):
    """The footprint sums of the slots [s0, s1) on `plane` as (ns,) complex, zero outside the range."""
    fp = footprint(geom, coord, plane, s0, s1) if fp is None else fp
    out = []
    for g in (grid.astype(np.complex128), _absc(grid.astype(np.complex128))):
        foot = g[fp['rows'][:, :, None], fp['cols'][:, None, :]]
        acc = np.zeros(coord.shape[1], complex)
        acc[s0:s1] = fp['ww'] * np.einsum('vab,va,vb->v', foot, fp['fu'], fp['fv'])
        out.append(acc)
    return out[0], out[1]


# ------------------------------------------------------------------------------------------------ the slot kernels
def centre_turns(geom, coord):
    return coord[0] * (geom['cx'] / (geom['px'] * geom['Nu'])) + coord[1] * (geom['cy'] / (geom['py'] * geom['Nv']))


def _turned(a):
    """The scale of a times a phase exp(i t): an error of t moves Re by |Im a| |dt| and Im by |Re a| |dt| wherever the
    phase points, so both components scale with |Re a| + |Im a| (a componentwise product of absolute values would
    vanish where cos t does and bound nothing)."""
    m = np.abs(a.real) + np.abs(a.imag)
    return m + 1j * m


def _centre(geom, coord, sign):
    """The centre phase of every slot, or None where the kernel applies none (centre (0, 0))."""
    on = geom['cx'] != 0.0 or geom['cy'] != 0.0
    return np.exp(sign * 2j * np.pi * centre_turns(geom, coord)) if on else None


def ref_prep(geom, vis, wgt, idx, coord):
    """val[s] = wgt vis exp(+2 pi i (u cx + v cy)) of visibility idx[s]."""
    v = vis.reshape(-1).astype(np.complex128)[idx]
    if wgt is not None:
        v = v * wgt.reshape(-1).astype(np.float64)[idx]
    ph = _centre(geom, coord, +1)
    return (v, _absc(v)) if ph is None else (v * ph, _turned(v))


def ref_finish(geom, acc, wgt, idx, coord, nvis):
    """vis (nvis,) = 0, then vis[idx[s]] = wgt acc[s] exp(-2 pi i (u cx + v cy))."""
    a = acc.astype(np.complex128)
    ph = _centre(geom, coord, -1)
    w = 1.0 if wgt is None else wgt.reshape(-1).astype(np.float64)[idx]
    vis, S = np.zeros(nvis, complex), np.zeros(nvis, complex)
    vis[idx] = (a if ph is None else a * ph) * w
    S[idx] = (_absc(a) if ph is None else _turned(a)) * w
    return vis, S


def ref_weight(acc, wgt, idx):
    a = acc.astype(np.complex128)
    w = 1.0 if wgt is None else wgt.reshape(-1).astype(np.float64)[idx]
    return a * w, _absc(a) * np.abs(w)


# ----------------------------------------------------------------------------------------------- the image kernels
def _window(geom):
    gi = (np.arange(geom['nx']) - geom['nx'] // 2) % geom['Nu']
    gj = (np.arange(geom['ny']) - geom['ny'] // 2) % geom['Nv']
    return np.ix_(gi, gj)


def ref_image_forward(geom, dirty, beam, corr, nm1, plane):
    """grid (Nu, Nv) = 0, then its centred window = dirty corr [beam] exp(+2 pi i w_p nm1)."""
    d = dirty.astype(np.float64) * corr * (1.0 if beam is None else beam.astype(np.float64))
    grid, S = np.zeros((geom['Nu'], geom['Nv']), complex), np.zeros((geom['Nu'], geom['Nv']), complex)
    grid[_window(geom)] = d if nm1 is None else d * np.exp(2j * np.pi * plane_w(geom, plane) * nm1)
    S[_window(geom)] = np.abs(d) if nm1 is None else _turned(d + 0j)
    return grid, S


def ref_image_adjoint(geom, grid, nm1, plane, img0):
    """img0 + window(grid) exp(-2 pi i w_p nm1)."""
    g = grid.astype(np.complex128)[_window(geom)]
    i0 = img0.astype(np.complex128)
    if nm1 is None:
        return i0 + g, _absc(i0) + _absc(g)
    return i0 + g * np.exp(-2j * np.pi * plane_w(geom, plane) * nm1), _absc(i0) + _turned(g)


def ref_image_correct(img, corr, beam):
    d = img.astype(np.complex128).real * corr * (1.0 if beam is None else beam.astype(np.float64))
    return d, np.abs(d)


# ------------------------------------------------------------------------------------------------------ the tables
DTYPES = ('f32', 'f64')
SUPPORTS = tuple(range(4, 13))


def narrow(W):
    """The smallest even nx whose grid 2 nx holds the footprint."""
    return 2 * ((W + 3) // 4)


def slots_per_block(W):
    return WG_BLOCK // (2 * W)


INTERIOR = (37, 250)          # first and last slot of the interior range [s0, s1) of the 300-slot entries


def foot_coords(geom, n, seed):
    """coord (3, n): the slots rotate through -- inside the grid; on the seam (exactly +- N/2) and a quarter cell inside;
    two to five grids beyond Nyquist on either sign; wild (about +- 1e6 cells); around cell 0, where the footprint's
    indices wrap, on one axis and on both.  All finite.  With a w kernel the plane
    coordinates lie within h - 0.1 of the middle plane nplanes // 2, so every slot has weight there, and the first
    slots sit exactly h away from plane 0 or from the last plane: an exact zero of the weight."""
    rng = np.random.default_rng(seed)
    out = np.zeros((3, n))
    for ax, N in ((0, geom['Nu']), (1, geom['Nv'])):
        g = rng.uniform(-0.5 * N, 0.5 * N, n)
        s = np.arange(n) + 2 * ax                # the two axes are out of step: a seam slot on u lies inside on v
        sign = np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0)
        g = np.where(s % 8 == 1, rng.uniform(-1.0, 1.0, n), g)            # around cell 0: the index wraps on this axis
        g = np.where(s % 8 == 3, sign * 0.5 * N, g)
        g = np.where(s % 8 == 5, sign * (0.5 * N - 0.25), g)
        g = np.where(s % 8 == 6, g + sign * N * rng.integers(2, 6, n), g)
        g = np.where(s % 8 == 7, g + sign * (1.0e6 + N * rng.integers(0, 50, n)), g)
        out[ax] = np.where(np.arange(n) % 8 == 0, rng.uniform(-1.0, 1.0, n), g)        # ... and on both axes at once
    if geom['wk']:
        h, pm = geom['h'], geom['nplanes'] // 2
        pg = rng.uniform(pm - h + 0.1, pm + h - 0.1, n)
        pg[0] = h                                   # phi(-1) at plane 0: exactly 0
        if n > 1:
            pg[1] = geom['nplanes'] - 1 - h          # phi(+1) at the last plane
        if n > 2:
            pg[2] = float(pm)                        # on a plane
        for s, d in zip(INTERIOR, (0.3, -0.4)):      # the ends of the interior range carry weight on the middle plane
            if n > s:
                pg[s] = pm + d
        out[2] = pg
    return out


def _foot_table():
    table = []
    for W in SUPPORTS:
        nb, m = slots_per_block(W), narrow(W)
        np3 = W + 3
        shapes = [('narrow-u', m, 8, 1, nb, 0, nb, (0,)),
                  ('narrow-v', 8, m, 1, nb + 1, 0, nb + 1, (0,)),
                  ('narrow-uv-one', m, m, 1, 1, 0, 1, (0,)),
                  ('34x26-planes', 34, 26, np3, 300, 0, 300, (0, np3 // 2, np3 - 1)),
                  ('34x26-interior', 34, 26, np3, 300, INTERIOR[0], INTERIOR[1] + 1, (0, np3 // 2, np3 - 1))]
        for dtype in DTYPES:
            for k, (tag, nx, ny, nplanes, n, s0, s1, planes) in enumerate(shapes):
                geom = geometry(dtype, nx, ny, W, nplanes=nplanes, w0=-3.0, dw=0.8)
                table.append(dict(id=f'W{W}-{dtype}-{tag}', geom=geom, n=n, s0=s0, s1=s1, planes=planes,
                                  seed=1000 + 10 * W + k))
    return table


FOOT = _foot_table()
FOOT_IDS = [e['id'] for e in FOOT]


def foot_data(entry):
    """coord, val (n,), grid (Nu, Nv) of a footprint entry, fp64 / complex128 (the tests cast to the entry's type)."""
    geom, n = entry['geom'], entry['n']
    rng = np.random.default_rng(entry['seed'] + 5)
    coord = foot_coords(geom, n, entry['seed'])
    val = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    grid = rng.standard_normal((geom['Nu'], geom['Nv'])) + 1j * rng.standard_normal((geom['Nu'], geom['Nv']))
    return coord, val, grid


# ---- order only
ORDER_W, ORDER_NPLANES, ORDER_W0, ORDER_DW = 7, 12, -5.0, 0.75
ORDER_IMAGES = (('512x512', 512, 512, 16), ('520x512', 520, 512, 32), ('2050x130', 2050, 130, 32),
                ('2050x1030', 2050, 1030, 64), ('34x26', 34, 26, 16))
ORDER_SHAPES = ((1, 1), (255, 1), (256, 1), (257, 1), (513, 1), (1, 3), (85, 3), (171, 3))
ORDER_MASKS = ('none', 'partial', 'all-but-one')


def _order_table():
    table = []
    for gi, (name, nx, ny, tile) in enumerate(ORDER_IMAGES):
        for si, (nrow, nchan) in enumerate(ORDER_SHAPES):
            table.append(dict(id=f'{name}-{nrow}x{nchan}-{ORDER_MASKS[(gi + si) % 3]}', nx=nx, ny=ny, tile=tile,
                              nrow=nrow, nchan=nchan, mask=ORDER_MASKS[(gi + si) % 3], seed=2000 + 10 * gi + si))
    return table


ORDER = _order_table()
ORDER_IDS = [e['id'] for e in ORDER]


def order_data(entry):
    """(geom, uvw, freq, mask) of an order entry.  Rows rotate through: anywhere in the grid; the last tile of u (and of
    v) from a negative coordinate; the footprint's first cell at N - 1; the first tile.  w runs from three planes below
    w0 to three beyond the last plane."""
    geom = geometry('f64', entry['nx'], entry['ny'], ORDER_W, nplanes=ORDER_NPLANES, w0=ORDER_W0, dw=ORDER_DW,
                    px=1e-3, py=1e-3)
    rng = np.random.default_rng(entry['seed'])
    nrow, nchan, h = entry['nrow'], entry['nchan'], geom['h']
    r = np.arange(nrow)
    cells = []
    for N in (geom['Nu'], geom['Nv']):
        g = rng.uniform(-0.5 * N, 0.5 * N, nrow)
        g = np.where(r % 4 == 1, -0.5 - 0.01 * (r % 7), g)            # first cell N - ceil(h) ..: the last tile
        g = np.where(r % 4 == 2, h - 1.75, g)                         # first cell -1 -> N - 1
        g = np.where(r % 4 == 3, h + 0.01 * (r % 5), g)               # first cell 0 or 1
        cells.append(g)
    pg = rng.uniform(-3.0, ORDER_NPLANES + 3.0, nrow)
    freq = 1.0e9 * (1.0 + 0.004 * np.arange(nchan))
    lam = C_LIGHT / freq[0]
    uvw = np.stack([cells[0] / (geom['px'] * geom['Nu']), cells[1] / (geom['py'] * geom['Nv']),
                    ORDER_W0 + pg * ORDER_DW], axis=1) * lam
    nvis = nrow * nchan
    if entry['mask'] == 'none':
        mask = None
    elif entry['mask'] == 'partial':
        mask = (rng.uniform(size=nvis) < 0.6).astype(np.uint8)
        mask[rng.integers(nvis)] = 1
    else:
        mask = np.zeros(nvis, np.uint8)
        mask[rng.integers(nvis)] = 1
    return geom, np.ascontiguousarray(uvw), freq, mask


# ---- image kernels: W = 4 so that (2, 2) has a plan; (beam, nm1, nplanes, plane)
IMAGE_SIZES = ((2, 2), (6, 8), (10, 6), (18, 22), (34, 26))
IMAGE_VARIANTS = (('beam-nm1-oneplane', True, True, 1, 0), ('nm1-plane0', False, True, 8, 0),
                  ('beam-nm1-plane5', True, True, 8, 5), ('plain', False, False, 1, 0))


def _image_table():
    table = []
    for i, (nx, ny) in enumerate(IMAGE_SIZES):
        for dtype in DTYPES:
            for j, (tag, beam, nm1, nplanes, plane) in enumerate(IMAGE_VARIANTS):
                table.append(dict(id=f'{nx}x{ny}-{dtype}-{tag}', beam=beam, nm1=nm1, plane=plane, seed=3000 + 10 * i + j,
                                  geom=geometry(dtype, nx, ny, 4, nplanes=nplanes, w0=-7.5, dw=2.25)))
    return table


IMAGE = _image_table()
IMAGE_IDS = [e['id'] for e in IMAGE]


def image_data(entry):
    """dirty, beam, corr, nm1 (nx, ny) real, and grid (Nu, Nv), img (nx, ny) complex of an image entry."""
    geom = entry['geom']
    nx, ny = geom['nx'], geom['ny']
    rng = np.random.default_rng(entry['seed'])
    cplx = lambda shape: rng.standard_normal(shape) + 1j * rng.standard_normal(shape)        # noqa: E731
    return dict(dirty=rng.standard_normal((nx, ny)), beam=rng.uniform(0.5, 1.0, (nx, ny)) if entry['beam'] else None,
                corr=rng.uniform(1.0, 3.0, (nx, ny)), nm1=-rng.uniform(0.0, 0.02, (nx, ny)) if entry['nm1'] else None,
                grid=cplx((geom['Nu'], geom['Nv'])), img=cplx((nx, ny)))


# ---- slot kernels: (wgt, centre) on the order of a small geometry, fewer slots than visibilities
SLOT = [dict(id=f'{dtype}-{"wgt" if wgt else "nowgt"}-{"centre" if centre else "nocentre"}', dtype=dtype, wgt=wgt,
             centre=centre, seed=4000 + k)
        for k, (dtype, wgt, centre) in enumerate((d, w, c) for d in DTYPES for w in (True, False) for c in (True, False))]
SLOT_IDS = [e['id'] for e in SLOT]


def slot_data(entry):
    """257 rows x 3 channels inside the 34 x 26 image's grid, a partial mask: geom, the reference order, and data."""
    cx, cy = (0.05, -0.08) if entry['centre'] else (0.0, 0.0)
    geom = geometry(entry['dtype'], 34, 26, 6, nplanes=10, w0=-4.0, dw=1.5, cx=cx, cy=cy)
    rng = np.random.default_rng(entry['seed'])
    nrow, nchan = 257, 3
    freq = 1.0e9 * (1.0 + 0.02 * np.arange(nchan))
    lam = C_LIGHT / freq.max()
    uvw = np.stack([rng.uniform(-0.5, 0.5, nrow) / geom['px'], rng.uniform(-0.5, 0.5, nrow) / geom['py'],
                    rng.uniform(-1.0, 4.0, nrow)], axis=1) * lam
    mask = (rng.uniform(size=nrow * nchan) < 0.7).astype(np.uint8)
    idx, coord, plane_off = ref_order(geom, uvw, freq, mask)
    cplx = lambda n: rng.standard_normal(n) + 1j * rng.standard_normal(n)        # noqa: E731
    return dict(geom=geom, uvw=uvw, freq=freq, mask=mask, idx=idx, coord=coord, nvis=nrow * nchan,
                vis=cplx(nrow * nchan), acc=cplx(idx.size), wgt=rng.uniform(0.5, 1.5, nrow * nchan) if entry['wgt'] else None)
