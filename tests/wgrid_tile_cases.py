"""
The tile-owned gridder of csrc/wgrid.hip (pfb_wgrid_order_keys64 / _order_coords / _grid_tile): numpy
references for its order and its target map, an emulation of the kernel's sums, and the table of
test_cpu_wgrid_tile_cases.py / test_gpu_wgrid_tile.py.  Built on wgrid_kernel_cases (geometry, vis_coords, first, wrap,
ref_grid_plane), which states the footprint once.

coord_keys / ref_keys64      the 64-bit key (p0 nfu + a / 16) nfv + b / 16 of a slot or visibility, MASKED where masked.
ref_tile_order               (idx, coord, plane_off, sorted keys) of the STABLE sort of the keys.
segments                     the non-empty runs (key, start, count) of sorted keys.
axis_feeds / ref_tile_map    the target rule, written as the sentence states it -- tile t is fed by first cells a with
                             (r - a) mod N < W for a cell r of t -- with plain loops, and the CSR it gives.  rule='wrong'
                             is "the tile and its next neighbour on either axis, no dedup": what the table must catch.
emulate_grid_plane           the kernel in numpy fp64: per target the pairs with plane - W + 1 <= p0 <= plane in list
                             order, per slot the cells of the footprint inside the tile.  Also returns, per target, the
                             counts of the pairs it walked (the staging batches are cut from their concatenation).
TILE                         the kernel table: coord is given directly (a slot may sit exactly on a zero of the w weight)
                             and ordered by its keys.
ORDER                        the order table: wgrid_kernel_cases.order_data on small grids.
"""
import numpy as np

import wgrid_kernel_cases as kc

FINE = 16                     # WG_FINE of csrc/wgrid.hip
BATCH = 64                    # WG_BATCH
MASKED = np.int64(2 ** 63 - 1)


def fine_tiles(geom):
    return -(-geom['Nu'] // FINE), -(-geom['Nv'] // FINE)


# ----------------------------------------------------------------------------------------------------- the order
def coord_keys(geom, coord):
    """The key of every column of coord (3, n), with a, b, p0 as kc.ref_keys forms them."""
    h = geom['h']
    nfu, nfv = fine_tiles(geom)
    a, b = kc.wrap(kc.first(coord[0], h), geom['Nu']), kc.wrap(kc.first(coord[1], h), geom['Nv'])
    p0 = np.zeros(coord.shape[1], np.int64)
    if geom['wk']:
        p = kc.first(coord[2], h)
        top = geom['np0'] - 1
        p0 = np.where(p > 0.0, np.where(p < top, p, top), 0).astype(np.int64)
    return (p0 * nfu + a // FINE) * nfv + b // FINE


def ref_keys64(geom, uvw, freq, mask):
    keys = coord_keys(geom, np.stack(kc.vis_coords(geom, uvw, freq)))
    return keys if mask is None else np.where(mask.reshape(-1) != 0, keys, MASKED)


def plane_offsets(geom, skeys):
    nfu, nfv = fine_tiles(geom)
    return np.searchsorted(skeys, np.arange(geom['np0'] + 1, dtype=np.int64) * (nfu * nfv)).tolist()


def ref_tile_order(geom, uvw, freq, mask):
    """(idx int32, coord (3, nsorted), plane_off (np0 + 1), the live sorted keys)."""
    keys = ref_keys64(geom, uvw, freq, mask)
    order = np.argsort(keys, kind='stable')
    skeys = keys[order]
    plane_off = plane_offsets(geom, skeys)
    ns = plane_off[-1]
    assert ns == int((keys != MASKED).sum())
    idx = order[:ns].astype(np.int32)
    coord = np.stack([c[idx] for c in kc.vis_coords(geom, uvw, freq)]) if ns else np.zeros((3, 0))
    return idx, coord, plane_off, skeys[:ns]


def segments(skeys):
    ukeys, starts, counts = np.unique(skeys, return_index=True, return_counts=True)
    return ukeys.astype(np.int64), starts.astype(np.int64), counts.astype(np.int64)


# ------------------------------------------------------------------------------------------------ the target map
def axis_feeds(N, W, rule='general'):
    """feeds[f]: the target tiles of an axis of N cells that source tile f feeds, in the order the rule names them."""
    nt = -(-N // FINE)
    if rule == 'wrong':
        return [[f, (f + 1) % nt] for f in range(nt)]
    feeds = []
    for f in range(nt):
        firsts = range(FINE * f, min(FINE * f + FINE, N))
        feeds.append([t for t in range(nt)
                      if any((r - a) % N < W for r in range(FINE * t, min(FINE * t + FINE, N)) for a in firsts)])
    return feeds


def ref_tile_map(geom, ukeys, starts, counts, rule='general'):
    """(tgt_tile, tgt_ptr, pair_start, pair_count, pair_p0, pair_src): per target the pairs sorted by (p0, source)."""
    nfu, nfv = fine_tiles(geom)
    fu_feeds, fv_feeds = axis_feeds(geom['Nu'], geom['W'], rule), axis_feeds(geom['Nv'], geom['W'], rule)
    lists = {}
    for key, start, count in zip(ukeys.tolist(), starts.tolist(), counts.tolist()):
        p0, src = divmod(key, nfu * nfv)
        for tu in fu_feeds[src // nfv]:
            for tv in fv_feeds[src % nfv]:
                lists.setdefault(tu * nfv + tv, []).append((p0, src, start, count))
    tgt_tile = np.array(sorted(lists), np.int32)
    pairs = [p for t in tgt_tile.tolist() for p in sorted(lists[t])]
    tgt_ptr = np.concatenate([[0], np.cumsum([len(lists[t]) for t in tgt_tile.tolist()])]).astype(np.int64)
    col = lambda k, dt: np.array([p[k] for p in pairs], dt)        # noqa: E731
    return tgt_tile, tgt_ptr, col(2, np.int64), col(3, np.int32), col(0, np.int32), col(1, np.int64)


def emulate_grid_plane(geom, coord, val, plane, tmap):
    """(grid (Nu, Nv) complex, walked): the tile gridder's sums in fp64, and per target the counts of the pairs in range."""
    Nu, Nv, W = geom['Nu'], geom['Nv'], geom['W']
    nfv = fine_tiles(geom)[1]
    tgt_tile, tgt_ptr, pstart, pcount, pp0 = tmap[:5]
    fp = kc.footprint(geom, coord, plane, 0, coord.shape[1])
    grid = np.zeros((Nu, Nv), complex)
    walked = {}
    for t, tile in enumerate(tgt_tile.tolist()):
        r0, c0 = (tile // nfv) * FINE, (tile % nfv) * FINE
        for p in range(tgt_ptr[t], tgt_ptr[t + 1]):
            if not plane - W + 1 <= pp0[p] <= plane:
                continue
            walked.setdefault(tile, []).append(int(pcount[p]))
            for s in range(pstart[p], pstart[p] + pcount[p]):
                if fp['ww'][s] == 0:
                    continue
                rows, cols = fp['rows'][s], fp['cols'][s]
                ir = (rows >= r0) & (rows < r0 + FINE)
                ic = (cols >= c0) & (cols < c0 + FINE)
                grid[np.ix_(rows[ir], cols[ic])] += fp['fu'][s][ir][:, None] * (val[s] * fp['ww'][s] * fp['fv'][s][ic])
    return grid, walked


# ------------------------------------------------------------------------------------------------------ the tables
# the slots of the 'batches' entries, per source tile (fu, fv) of the 64 x 64 grid (4 tiles an axis): target (1, 1) walks
# 30 + 34 + 5 + 70 slots -- a batch ends between two segments (64) and inside one (128) --, target (3, 3) exactly 64
BATCH_SOURCES = ((0, 0, 30), (0, 1, 34), (1, 0, 5), (1, 1, 70), (3, 3, 64), (2, 0, 50))
NPROD = 4


def _cross(N, h):
    """A coordinate whose footprint starts in the last cell of the tile before the last one, reached from below zero."""
    nt = -(-N // FINE)
    return h + (FINE * (nt - 1) - 1 - N) - 0.5


def tile_coords(entry):
    """coord (3, n) of a table entry, in generation order (tile_data orders it)."""
    geom, n = entry['geom'], entry['n']
    rng = np.random.default_rng(entry['seed'])
    h = geom['h']
    out = np.zeros((3, n))
    if entry['kind'] == 'batches':
        at = 0
        for fu, fv, count in BATCH_SOURCES:
            out[0, at:at + count] = h + FINE * fu + rng.uniform(-0.9, 14.9, count)
            out[1, at:at + count] = h + FINE * fv + rng.uniform(-0.9, 14.9, count)
            at += count
        assert at == n
        return out[:, rng.permutation(n)]
    s = np.arange(n)
    for ax, N in ((0, geom['Nu']), (1, geom['Nv'])):
        g = rng.uniform(-0.5 * N, 0.5 * N, n)
        sign = np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0)
        g = np.where(s % 6 == 1, h - 1.75 - 0.2 * rng.uniform(size=n), g)          # first cell -1 -> N - 1, both axes
        g = np.where(s % 6 == 2, h - 2.5 - 0.01 * (s % 7), g)                      # first cell -2: the last tile, from below zero
        g = np.where(s % 6 == 3, _cross(N, h), g)                 # into the last tile, through it and on into tile 0
        if ax == 1:
            g = np.where(s % 6 == 4, rng.uniform(-1.0, 1.0, n), g)                 # around cell 0 on one axis
        g = np.where(s % 6 == 5, g + sign * N * rng.integers(2, 6, n), g)          # grids beyond Nyquist
        out[ax] = g
    if geom['wk']:
        pg = rng.uniform(h - 0.9, h + 2.0, n)        # first planes 0, 1, 2: planes beyond W + 1 hold nothing
        pg[0], pg[1] = h, h + 1.0                    # exactly h below planes 0 and 1: the weight's zero
        out[2] = pg
    return out


def _tile_table():
    table = []
    for W in kc.SUPPORTS:
        shapes = [('one-tile', 'mixed', 8, 8, 1, 250, (0,)),
                  ('two-tiles', 'mixed', 16, 16, 1, 300, (0,)),
                  ('partial', 'mixed', 20, 18, W + 6, 400, (0, 1, 2, W + 1, W + 2, W + 5)),
                  ('batches', 'batches', 32, 32, 1, sum(c for _, _, c in BATCH_SOURCES), (0,))]
        for dtype in kc.DTYPES:
            for k, (tag, kind, nx, ny, nplanes, n, planes) in enumerate(shapes):
                table.append(dict(id=f'W{W}-{dtype}-{tag}', tag=tag, kind=kind, n=n, planes=planes,
                                  nprods=(1, 2, 3, 4) if W == 7 else (1, 4), seed=5000 + 10 * W + k,
                                  geom=kc.geometry(dtype, nx, ny, W, nplanes=nplanes, w0=-3.0, dw=0.8)))
    return table


TILE = _tile_table()
TILE_IDS = [e['id'] for e in TILE]

_data = {}


def tile_data(entry):
    """(coord (3, n) in key order, val (NPROD, n) complex, plane_off, tmap) of a table entry; computed once per seed
    and geometry (the two types of a support share it) and never written."""
    key = entry['id'].replace(entry['geom']['dtype'], '')
    if key not in _data:
        geom, n = entry['geom'], entry['n']
        coord = tile_coords(entry)
        keys = coord_keys(geom, coord)
        order = np.argsort(keys, kind='stable')
        coord, skeys = np.ascontiguousarray(coord[:, order]), keys[order]
        rng = np.random.default_rng(entry['seed'] + 5)
        val = rng.standard_normal((NPROD, n)) + 1j * rng.standard_normal((NPROD, n))
        for a in (coord, val):
            a.setflags(write=False)
        _data[key] = coord, val, plane_offsets(geom, skeys), ref_tile_map(geom, *segments(skeys))
    return _data[key]


# ---- the order: kc.order_data's rows (anywhere; the last tile from a negative coordinate; first cell N - 1; the first
# tile; w from below the first plane to beyond the last) on grids of one tile, two tiles and partial last tiles
ORDER_IMAGES = ((8, 8), (16, 16), (20, 18), (34, 26))
ORDER_SHAPES = ((257, 1), (171, 3))


def _order_table():
    table = []
    for gi, (nx, ny) in enumerate(ORDER_IMAGES):
        for si, (nrow, nchan) in enumerate(ORDER_SHAPES):
            mask = kc.ORDER_MASKS[(gi + si) % 3]
            table.append(dict(id=f'{nx}x{ny}-{nrow}x{nchan}-{mask}', nx=nx, ny=ny, nrow=nrow, nchan=nchan, mask=mask,
                              seed=6000 + 10 * gi + si))
    return table


ORDER = _order_table()
ORDER_IDS = [e['id'] for e in ORDER]
