"""
The w-gridder on MI355X -- ducc0.wgridder.experimental.vis2dirty / dirty2vis as pfb/operators/hessian.py:62-106 calls
them, with ducc0's names and defaults.  The operators are the direct Fourier sums stated in include/pfb_hip.h
("w-gridder"); they are evaluated by w-stacking on a twice oversampled grid with the kernel
exp(2.3 W (sqrt(1 - x^2) - 1)) of W = ceil(log10(1/epsilon)) + 2 cells:

    vis2dirty   per w plane: grid (pfb_wgrid_grid), unnormalised inverse c2c, window and w phase
                (pfb_wgrid_image_adjoint); at the end the kernel correction with 1/n (pfb_wgrid_image_correct)
    dirty2vis   the adjoint, step by step: pfb_wgrid_image_forward, forward c2c, pfb_wgrid_degrid

The c2c transform of a plane is torch.fft (the precedent of operators/fft.py); everything else is csrc/wgrid.hip.

Beyond ducc0: vis (nprod, nrow, nchan) / dirty (nprod, nx, ny), nprod <= 4 -- the Stokes products of one chunk, e.g. of
utils.stokes.stokes_vis(product='IQUV') -- go through both operators in ONE call under one plan and order
(pfb_wgrid_*_multi: what depends on the coordinates alone is computed once for all planes).

A WgridPlan holds what one (uvw, freq, mask) set and one image geometry share between calls: support, planes, the
correction tables and the visibilities' sorted order.  Plans live in a PlanCache: a major cycle that presents the same
arrays again builds nothing.  numpy in gives numpy out, tensors in give tensors out; there is no CPU path.

image_data_products (pfb/operators/gridder.py:551-740) composes these with utils/weighting.py into the grid worker's
products: WEIGHT, WSUM, DIRTY, PSF, PSFHAT and RESIDUAL of one band.

The predict step (pfb/operators/gridder.py:258-548) degrids on BLOCKS of rows and channels: im2vis a cube's
bands into their channels, comps2vis the component model of every (time bin, band) into a (row, chan, corr) model column
(pfb_wgrid_finish_block lands the sorted slots there), loc2psf_vis the PSF's visibilities.  A block's plan takes nm1 and
the correction tables from the GeomTables of its geometry, which are built once, and never enters the plan cache.
"""
import ctypes as C
import math
import threading

import numpy as np
import torch

from .. import _dev, _lib
from .._plan import NativePlan, PlanCache, array_key
from ..utils import weighting
from ..utils.comps import _render
from .fft import psfhat_from_psf

C_LIGHT = 299792458.0
EPS_MAX = 1e-2
MAX_PROD = 4            # planes of a stacked call (WG_MAX_PROD of csrc/wgrid.hip): the Stokes products
# lower bounds of epsilon: fp64 by the support range of the kernels (W <= 12); fp32 measured: the lowest decade tried
# (1e-3, 1e-4, 1e-5) at which every case of tests/wgrid_cases.py stays under epsilon / 3 on the MI355X
EPS_MIN = {torch.float64: 1e-10, torch.float32: 1e-5}
_QUAD_NODES = 128
FINE_TILE = 16          # the tile edge of the reproducible mode (WG_FINE of csrc/wgrid.hip): a workgroup's cells


def support_for(epsilon):
    """W = ceil(log10(1 / epsilon)) + 2 (a whole decade is not pushed up by the rounding of the logarithm)."""
    return int(math.ceil(-math.log10(epsilon) - 1e-9)) + 2


def check_epsilon(epsilon, rdtype):
    eps = float(epsilon)
    lo = EPS_MIN[rdtype]
    if not (lo * (1 - 1e-12) <= eps <= EPS_MAX * (1 + 1e-12)):
        raise ValueError(f"epsilon {eps:g} outside the supported range [{lo:g}, {EPS_MAX:g}] for {rdtype}")
    return eps


def _quadrature(W):
    """(x, f) of the correction integral below: the Gauss-Legendre nodes in theta as x = sin(theta) -- a node's
    frequency in t is 2 pi h x -- and phi(x) cos(theta) times the node's weight."""
    th, wq = np.polynomial.legendre.leggauss(_QUAD_NODES)
    th, wq = th * (np.pi / 2), wq * (np.pi / 2)
    return np.sin(th), np.exp(2.3 * W * (np.cos(th) - 1.0)) * np.cos(th) * wq


def kernel_correction(W, t):
    """c(t) = h int_-1^1 phi(x) cos(2 pi h t x) dx, h = W / 2, phi(x) = exp(2.3 W (sqrt(1 - x^2) - 1)): Gauss-Legendre
    in theta, x = sin(theta), where the integrand is smooth up to the ends.  fp64 on the host."""
    t = np.asarray(t, dtype=np.float64)
    h = 0.5 * W
    x, f = _quadrature(W)
    return h * (np.cos(2 * np.pi * h * t[..., None] * x) * f).sum(-1)


def _kernel_correction_dev(W, t):
    """kernel_correction on a device fp64 tensor, node by node: the (nx, ny) table of the w axis is summed where it
    will live instead of as an (nx, ny, nodes) array on the host."""
    h = 0.5 * W
    x, f = _quadrature(W)
    acc = torch.zeros_like(t)
    for a, fq in zip(2 * np.pi * h * x, f):
        acc.add_(torch.cos(t * float(a)), alpha=float(fq))
    return acc.mul_(h)


def image_lmn(nx, ny, pixsize_x, pixsize_y, center_x, center_y):
    """(l, m, nm1) of the pixel grid: l (nx, 1), m (1, ny), nm1 (nx, ny)."""
    l = ((np.arange(nx) - nx // 2) * pixsize_x + center_x)[:, None]
    m = ((np.arange(ny) - ny // 2) * pixsize_y + center_y)[None, :]
    r2 = l * l + m * m
    if r2.max() >= 1.0:
        raise ValueError("the image reaches beyond the horizon (l^2 + m^2 >= 1)")
    return l, m, -r2 / (1.0 + np.sqrt(1.0 - r2))


def plane_layout(wmin, wmax, max_nm1, W, epsilon, do_wgridding):
    """(nplanes, w0, dw): planes at w0 + p dw.  One plane -- no w kernel -- without w-gridding (at w = 0) and where the
    w term cannot matter: the phase it leaves, pi max|nm1| (wmax - wmin), is below epsilon / 100 (at the mid w)."""
    if not do_wgridding:
        return 1, 0.0, 1.0
    if math.pi * max_nm1 * (wmax - wmin) <= 0.01 * epsilon:
        return 1, 0.5 * (wmin + wmax), 1.0
    dw = 1.0 / (4.0 * max_nm1)
    # a visibility at plane coordinate g = (w - w0) / dw touches planes ceil(g - h) .. + W - 1, g in [h, h + range / dw];
    # one plane to spare for the rounding of g at wmax
    return int(math.ceil((wmax - wmin) / dw)) + W + 1, wmin - 0.5 * W * dw, dw


class GeomTables:
    """What every plan on one image geometry, support and do_wgridding shares, whatever its visibilities: nm1, and the
    kernel correction 1 / (c_u c_v) with and without 1 / c_w(dw nm1) -- dw = 1 / (4 max|nm1|) is the geometry's too.
    fp64 device tables, each formed on first use; use through tables_for."""

    def __init__(self, nx, ny, pixsize_x, pixsize_y, center_x, center_y, W, do_wgridding, dev):
        self.W, self.do_wgridding = W, bool(do_wgridding)
        if self.do_wgridding:
            nm1 = image_lmn(nx, ny, pixsize_x, pixsize_y, center_x, center_y)[2]
        else:
            nm1 = np.zeros((nx, ny))            # without w-gridding nm1 := 0 and n := 1
        self.max_nm1 = float(np.abs(nm1).max())
        tu = (np.arange(nx) - nx // 2) / (2.0 * nx)
        tv = (np.arange(ny) - ny // 2) / (2.0 * ny)
        cuv = kernel_correction(W, tu)[:, None] * kernel_correction(W, tv)[None, :]
        self.nm1 = torch.from_numpy(np.ascontiguousarray(nm1)).to(dev) if self.do_wgridding else None
        self._corr = {(False, False): (1.0 / torch.from_numpy(cuv).to(dev)).contiguous()}
        self._lock = threading.Lock()

    def corr(self, wkernel, divide_by_n):
        """1 / (c_u c_v [c_w]) [/ n]: c_w for a plan of more than one plane."""
        wkernel, by_n = bool(wkernel), bool(divide_by_n) and self.do_wgridding          # without w-gridding n := 1
        with self._lock:
            if (True, False) not in self._corr and wkernel:
                dw = 1.0 / (4.0 * self.max_nm1)            # plane_layout's, whatever the w range
                cw = _kernel_correction_dev(self.W, dw * self.nm1)
                self._corr[True, False] = (self._corr[False, False] / cw).contiguous()
            if (wkernel, by_n) not in self._corr:
                self._corr[wkernel, True] = (self._corr[wkernel, False] / (1.0 + self.nm1)).contiguous()
            return self._corr[wkernel, by_n]


_tables = PlanCache(8)


def tables_for(nx, ny, pixsize_x, pixsize_y, center_x, center_y, W, do_wgridding, dev):
    """The cached GeomTables of a geometry; cache_stats['tables'] counts the constructions."""
    key = (int(nx), int(ny), float(pixsize_x), float(pixsize_y), float(center_x), float(center_y), int(W),
           bool(do_wgridding), str(dev))

    def make():
        cache_stats['tables'] += 1
        return GeomTables(int(nx), int(ny), pixsize_x, pixsize_y, center_x, center_y, int(W), do_wgridding, dev)
    return _tables.get(key, make)


def _axis_targets(N, W):
    """(ntiles, K) int64, -1 padded: the fine tiles of an axis of N cells that a footprint of W cells can reach when its
    first cell lies in tile f -- tile t is fed by first cells a with (r - a) mod N < W for a cell r of t --, each once.
    K is 2 on an ordinary axis, 1 where one tile is the axis (it is its own neighbour) and 3 where a partial last tile is
    narrower than W - 1 cells (a footprint crosses it and wraps into tile 0)."""
    nt = -(-N // FINE_TILE)
    a = np.arange(N)
    reach = ((a[:, None] + np.arange(W)) % N) // FINE_TILE
    codes = np.unique((a // FINE_TILE)[:, None] * nt + reach)
    src, tgt = codes // nt, codes % nt
    cnt = np.bincount(src, minlength=nt)
    table = np.full((nt, int(cnt.max())), -1, np.int64)
    table[src, np.arange(codes.size) - (np.cumsum(cnt) - cnt)[src]] = tgt
    return table


def tile_map(ukeys, starts, counts, Nu, Nv, W):
    """The target map of the tile-owned gridder from the non-empty segments (key, start, count) of a reproducible order,
    key = (p0 nfu + fu) nfv + fv ascending: (tgt_tile int32 (nT), tgt_ptr int64 (nT + 1), pair_start int64, pair_count
    int32, pair_p0 int32), a CSR over the fine tiles that receive anything.  A segment is listed under every tile its
    footprints can reach (_axis_targets on either axis); inside a target the pairs ascend by (p0, source tile) -- the
    segments' own order, kept by a stable sort on the target alone.  Device tensors in and out; no dense per-key table."""
    dev = ukeys.device
    nfu, nfv = -(-Nu // FINE_TILE), -(-Nv // FINE_TILE)
    src = ukeys % (nfu * nfv)
    tu = torch.from_numpy(_axis_targets(Nu, W)).to(dev)[src // nfv]          # (nseg, Ku)
    tv = torch.from_numpy(_axis_targets(Nv, W)).to(dev)[src % nfv]           # (nseg, Kv)
    tgt = tu[:, :, None] * nfv + tv[:, None, :]
    valid = (tu >= 0)[:, :, None] & (tv >= 0)[:, None, :]
    seg = torch.arange(ukeys.numel(), device=dev)[:, None, None].expand_as(tgt)[valid]          # segment-major
    tgt, by_target = torch.sort(tgt[valid], stable=True)
    seg = seg[by_target]
    tgt_tile, per_target = torch.unique_consecutive(tgt, return_counts=True)
    tgt_ptr = torch.zeros(tgt_tile.numel() + 1, dtype=torch.int64, device=dev)
    tgt_ptr[1:] = torch.cumsum(per_target, 0)
    return (tgt_tile.to(torch.int32), tgt_ptr, starts[seg].contiguous(), counts[seg].to(torch.int32),
            (ukeys // (nfu * nfv))[seg].to(torch.int32))


class WgridPlan(NativePlan):
    """One (uvw, freq, mask) set on one image geometry: the native geometry record, the sorted order (idx, coord, the
    planes' slot ranges), nm1 and the correction tables (the geometry's GeomTables), and the per-call buffers (one grid,
    val / acc, the complex image; and their stacks of up to MAX_PROD planes once a stacked call has come).  Use through vis2dirty / dirty2vis / hessian, which hold `lock`.  `degrid_only`: a
    block plan of the predict step, which holds the grid and one slot vector and has dirty2vis_into only.

    `reproducible`: the plan grids without atomics (pfb_wgrid_grid_tile, DESIGN 4.10 "The tile-owned gridder"): its own
    order -- keys on fine tiles of 16 x 16 cells, ascending visibility inside a key -- and the target map of that order
    (`tile_map`).  Every result of such a plan is identical bit for bit from run to run and from plan to plan on the
    same arrays; everything but the gridding step is the default plan's code on the other order."""
    _destroy = 'pfb_wgrid_plan_destroy'

    def __init__(self, uvw, freq, mask, nx, ny, pixsize_x, pixsize_y, center_x, center_y, epsilon, do_wgridding, rdtype,
                 degrid_only=False, reproducible=False):
        super().__init__()
        if degrid_only and reproducible:
            raise ValueError("reproducible: a block plan of the predict step (degrid_only) never grids")
        self.reproducible = bool(reproducible)
        dev = _dev.require_device()
        nx, ny = int(nx), int(ny)
        if nx < 2 or ny < 2 or nx % 2 or ny % 2:
            raise ValueError(f"npix_x, npix_y must be even (got {nx}, {ny})")
        self.rdtype, self.cdtype = rdtype, _dev.CPLX_OF[rdtype]
        self.epsilon = check_epsilon(epsilon, rdtype)
        self.W = W = support_for(self.epsilon)
        self.nx, self.ny = nx, ny
        self.do_wgridding = bool(do_wgridding)
        self.uvw, self.freq = _dev.uvw_freq(uvw, freq)
        self.nrow, self.nchan = int(self.uvw.shape[0]), int(self.freq.shape[0])
        self.nvis = self.nrow * self.nchan
        self.mask = None if mask is None else _dev.byte_mask(mask, (self.nrow, self.nchan))
        self.tables = tables_for(nx, ny, pixsize_x, pixsize_y, center_x, center_y, W, self.do_wgridding, dev)
        self.nm1 = self.tables.nm1
        # ---- the w range of the unmasked visibilities -> planes
        self.nsorted = 0
        self._stack = None              # the buffers of stacked calls (_buffers)
        w = self.uvw[:, 2:3] * self.freq[None, :] / C_LIGHT
        if self.mask is not None:
            w = w[self.mask != 0]
        if self.nvis == 0 or w.numel() == 0:
            return                      # nothing to grid: every call answers zeros without a launch
        wmin, wmax = w.min().item(), w.max().item()
        del w
        if not (math.isfinite(wmin) and math.isfinite(wmax)):
            raise ValueError("uvw / freq hold a non-finite value")
        self.nplanes, self.w0, self.dw = plane_layout(wmin, wmax, self.tables.max_nm1, W, self.epsilon,
                                                      self.do_wgridding)
        _lib.check(self._lib.pfb_wgrid_plan_create(_dev.code(rdtype), nx, ny, float(pixsize_x), float(pixsize_y),
                                                   float(center_x), float(center_y), W, self.nplanes, self.w0, self.dw,
                                                   C.byref(self._h)))
        nkeys, np0, tile = C.c_int(), C.c_int(), C.c_int()
        _lib.check(self._lib.pfb_wgrid_plan_info(self._h, C.byref(nkeys), C.byref(np0), C.byref(tile)))
        self.nkeys, self.np0, self.tile = nkeys.value, np0.value, tile.value
        if self.reproducible:
            self._build_tile_order(dev)
        else:
            self._build_order(dev)
        self._grid = torch.empty((2 * nx, 2 * ny), dtype=self.cdtype, device=dev)
        self._slots = torch.empty((1 if degrid_only else 2, self.nsorted), dtype=self.cdtype, device=dev)
        self._img = None if degrid_only else torch.empty((nx, ny), dtype=self.cdtype, device=dev)

    def _build_order(self, dev):
        """Counting sort by (first plane, uv tile): histogram kernel, torch.cumsum, placement kernel.  One number -- the
        count of unmasked visibilities -- and the planes' offsets cross to the host."""
        work = torch.empty(self._lib.pfb_wgrid_work_bytes(self._h), dtype=torch.uint8, device=dev)
        keys = torch.empty(self.nvis, dtype=torch.int32, device=dev)
        self.run('pfb_wgrid_order_count', _dev.ptr(self.uvw), _dev.ptr(self.freq), _dev.ptr(self.mask), self.nrow,
                 self.nchan, _dev.ptr(keys), _dev.ptr(work))
        counts = work[:4 * self.nkeys].view(torch.int32)
        offsets = torch.zeros(self.nkeys + 1, dtype=torch.int64, device=dev)
        offsets[1:] = torch.cumsum(counts, 0, dtype=torch.int64)
        self.plane_off = offsets[::self.nkeys // self.np0].cpu().tolist()        # np0 + 1 entries
        self.nsorted = self.plane_off[-1]
        self.idx = torch.empty(self.nsorted, dtype=torch.int32, device=dev)
        self.coord = torch.empty((3, self.nsorted), dtype=torch.float64, device=dev)
        self.run('pfb_wgrid_order_fill', _dev.ptr(self.uvw), _dev.ptr(self.freq), self.nrow, self.nchan, _dev.ptr(keys),
                 _dev.ptr(offsets), _dev.ptr(work), self.nsorted, _dev.ptr(self.idx), _dev.ptr(self.coord))

    def _build_tile_order(self, dev):
        """The order of the reproducible mode: 64-bit keys (first plane, fine tile) from the key kernel, a STABLE
        torch.sort -- ascending visibility inside a key, where the counting sort's cursor leaves the arrival order --,
        the coordinates of that order, and the target map of its segments.  The planes' offsets cross to the host."""
        ntiles = (-(-2 * self.nx // FINE_TILE)) * (-(-2 * self.ny // FINE_TILE))
        keys = torch.empty(self.nvis, dtype=torch.int64, device=dev)
        self.run('pfb_wgrid_order_keys64', _dev.ptr(self.uvw), _dev.ptr(self.freq), _dev.ptr(self.mask), self.nrow,
                 self.nchan, _dev.ptr(keys))
        keys, order = torch.sort(keys, stable=True)
        firsts = torch.arange(self.np0 + 1, dtype=torch.int64, device=dev) * ntiles          # below the mask's sentinel
        self.plane_off = torch.searchsorted(keys, firsts).cpu().tolist()        # np0 + 1 entries
        self.nsorted = self.plane_off[-1]
        self.idx = order[:self.nsorted].to(torch.int32)
        self.coord = torch.empty((3, self.nsorted), dtype=torch.float64, device=dev)
        self.run('pfb_wgrid_order_coords', _dev.ptr(self.uvw), _dev.ptr(self.freq), self.nrow, self.nchan,
                 _dev.ptr(self.idx), self.nsorted, _dev.ptr(self.coord))
        ukeys, counts = torch.unique_consecutive(keys[:self.nsorted], return_counts=True)
        self.tile_map = tile_map(ukeys, torch.cumsum(counts, 0) - counts, counts, 2 * self.nx, 2 * self.ny, self.W)
        self._map_args = tuple(_dev.ptr(t) for t in self.tile_map) + (self.tile_map[0].numel(),
                                                                      self.tile_map[2].numel())

    # ------------------------------------------------------------------------------------------------ pieces
    def corr(self, divide_by_n):
        """1 / (c_u c_v c_w) [/ n] as a device fp64 table: with c_w where the plan has more than one plane."""
        return self.tables.corr(self.nplanes > 1, divide_by_n)

    def plane_ranges(self):
        """(plane, s0, s1) of every plane that has slots: first planes p - W + 1 .. p."""
        off = self.plane_off
        for p in range(self.nplanes):
            s0, s1 = off[max(0, p - self.W + 1)], off[min(p, self.np0 - 1) + 1]
            if s1 > s0:
                yield p, s0, s1

    def _check(self, name, t, dtype, shape):
        if t is None:
            return
        if t.dtype != dtype or tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} must be {dtype} of shape {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")

    # A stacked call carries `nprod` planes (Stokes products) through every step under the plan's one order; nprod None
    # is the single operator, on the plan's own buffers and through the single entry points.
    def _buffers(self, nprod):
        """(grid, slots (2, ..), img) of a call: the plan's own, or the first nprod planes of its stacks -- grid
        (nprod, 2 nx, 2 ny), two slot stacks (nprod, nsorted), the complex images (nprod, nx, ny) --, which are allocated
        on the first stacked call, grown by a call with more planes, and kept."""
        if nprod is None:
            return self._grid, self._slots, self._img
        if self._stack is None or self._stack[0].shape[0] < nprod:
            dev = self.idx.device
            self._stack = (torch.empty((nprod, 2 * self.nx, 2 * self.ny), dtype=self.cdtype, device=dev),
                           torch.empty((2, nprod, self.nsorted), dtype=self.cdtype, device=dev),
                           torch.empty((nprod, self.nx, self.ny), dtype=self.cdtype, device=dev))
        if self._stack[0].shape[0] == nprod:
            return self._stack
        # fewer planes than the stacks hold: every plane has to follow its predecessor, so the slots are re-cut
        g, slots, img = self._stack
        return g[:nprod], slots.view(-1)[:2 * nprod * self.nsorted].view(2, nprod, self.nsorted), img[:nprod]

    def _step(self, name, nprod, *args):
        """pfb_wgrid_<name>, or pfb_wgrid_<name>_multi with nprod in front of its arguments."""
        if nprod is None:
            self.run('pfb_wgrid_' + name, *args)
        else:
            self.run('pfb_wgrid_' + name + '_multi', nprod, *args)

    def _degrid_all(self, x, beam, divide_by_n, nprod=None):
        """acc (the first slot vector, or stack) = the footprint sums of every slot over all planes, from image x."""
        g, slots, _ = self._buffers(nprod)
        acc = slots[0]
        acc.zero_()
        corr = self.corr(divide_by_n)
        for p, s0, s1 in self.plane_ranges():
            self._step('image_forward', nprod, p, _dev.ptr(x), _dev.ptr(beam), _dev.ptr(corr), _dev.ptr(self.nm1),
                       _dev.ptr(g))
            gh = torch.fft.fft2(g).contiguous()       # a fresh tensor: `out=` costs a copy of the grid per transform
            self._step('degrid', nprod, p, _dev.ptr(gh), _dev.ptr(self.coord), self.nsorted, s0, s1, _dev.ptr(acc))
        return acc

    def _grid_all(self, val, beam, divide_by_n, nprod=None):
        """The (nx, ny) real image, or the (nprod, nx, ny) images, of the slot values `val`, corrected."""
        g, _, img = self._buffers(nprod)
        img.zero_()
        for p, s0, s1 in self.plane_ranges():
            if self.reproducible:
                self._step('grid_tile', nprod, p, _dev.ptr(val), _dev.ptr(self.coord), self.nsorted, *self._map_args,
                           _dev.ptr(g))
            else:
                self._step('grid', nprod, p, _dev.ptr(val), _dev.ptr(self.coord), self.nsorted, s0, s1, _dev.ptr(g))
            gh = torch.fft.ifft2(g, norm='forward').contiguous()
            self._step('image_adjoint', nprod, p, _dev.ptr(gh), _dev.ptr(self.nm1), _dev.ptr(img))
        out = torch.empty(img.shape, dtype=self.rdtype, device=val.device)
        self._step('image_correct', nprod, _dev.ptr(img), _dev.ptr(self.corr(divide_by_n)), _dev.ptr(beam),
                   _dev.ptr(out))
        return out

    def _stacked(self, name, x, plane_shape, dtype, wgt):
        """What a call is: (None, wgt, 0) for a 2-D x -- checked as always --, else (nprod, wgt, shared) for x
        (nprod, *plane_shape) with 1 <= nprod <= 4 and wgt None, (nprod, nrow, nchan), or (nrow, nchan) shared by every
        plane."""
        vshape = (self.nrow, self.nchan)
        if x.ndim != 3:
            self._check(name, x, dtype, plane_shape)
            self._check('wgt', wgt, self.rdtype, vshape)
            return None, wgt, 0
        nprod = int(x.shape[0])
        if not 1 <= nprod <= MAX_PROD:
            raise ValueError(f"{name} stacks {nprod} planes: 1 to {MAX_PROD} products share a call")
        self._check(name, x, dtype, (nprod,) + tuple(plane_shape))
        shared = wgt is not None and wgt.ndim == 2
        self._check('wgt', wgt, self.rdtype, vshape if shared else (nprod,) + vshape)
        return nprod, (None if wgt is None else wgt.contiguous()), int(shared)

    # ---------------------------------------------------------------------------------------------- operators
    def vis2dirty(self, vis, wgt=None, divide_by_n=True):
        """dirty (nx, ny) of vis (nrow, nchan), or (nprod, nx, ny) of a stack vis (nprod, nrow, nchan), nprod <= 4, with
        wgt None, one (nrow, nchan) plane for every product, or (nprod, nrow, nchan)."""
        nprod, wgt, shared = self._stacked('vis', vis, (self.nrow, self.nchan), self.cdtype, wgt)
        if self.nsorted == 0:
            return torch.zeros(vis.shape[:-2] + (self.nx, self.ny), dtype=self.rdtype, device=vis.device)
        vis = vis if nprod is None else vis.contiguous()
        with self.lock:
            val = self._buffers(nprod)[1][1]
            if nprod is None:
                self.run('pfb_wgrid_prep', _dev.ptr(vis), _dev.ptr(wgt), _dev.ptr(self.idx), _dev.ptr(self.coord),
                         self.nsorted, _dev.ptr(val))
            else:
                self.run('pfb_wgrid_prep_multi', nprod, _dev.ptr(vis), _dev.ptr(wgt), shared,
                         _dev.ptr(self.idx), _dev.ptr(self.coord), self.nsorted, self.nvis, _dev.ptr(val))
            return self._grid_all(val, None, divide_by_n, nprod)

    def dirty2vis(self, dirty, wgt=None, divide_by_n=True):
        """vis (nrow, nchan) of dirty (nx, ny), or (nprod, nrow, nchan) of a stack dirty (nprod, nx, ny); wgt as in
        vis2dirty."""
        nprod, wgt, shared = self._stacked('dirty', dirty, (self.nx, self.ny), self.rdtype, wgt)
        vshape = dirty.shape[:-2] + (self.nrow, self.nchan)
        if self.nsorted == 0:
            return torch.zeros(vshape, dtype=self.cdtype, device=dirty.device)
        vis = torch.empty(vshape, dtype=self.cdtype, device=dirty.device)
        dirty = dirty if nprod is None else dirty.contiguous()
        with self.lock:
            acc = self._degrid_all(dirty, None, divide_by_n, nprod)
            if nprod is None:
                self.run('pfb_wgrid_finish', _dev.ptr(acc), _dev.ptr(wgt), _dev.ptr(self.idx), _dev.ptr(self.coord),
                         self.nsorted, _dev.ptr(vis), self.nvis)
            else:
                self.run('pfb_wgrid_finish_multi', nprod, _dev.ptr(acc), _dev.ptr(wgt), shared, _dev.ptr(self.idx),
                         _dev.ptr(self.coord), self.nsorted, _dev.ptr(vis), self.nvis)
        return vis

    def dirty2vis_into(self, dirty, out, row0, chan0, accumulate=False, divide_by_n=True):
        """dirty2vis of this plan's rows and channels -- a block without mask or weights -- landed in the caller's `out`
        (nrow_out, nchan_out, ncorr) at rows row0 .., channels chan0 .., correlations 0 and ncorr - 1, assigned or (with
        `accumulate`) added; no other cell of `out` is touched.  `out` is of the plan's complex type, or complex64
        under an fp64 plan: narrowed in the kernel, cast first and then added."""
        self._check('dirty', dirty, self.rdtype, (self.nx, self.ny))
        if self.mask is not None:
            raise ValueError("a block plan has no mask")
        if (out.ndim != 3 or not out.is_contiguous() or out.dtype not in (self.cdtype, torch.complex64)
                or not 1 <= out.shape[2] <= 4):
            raise ValueError(f"out must be a contiguous (nrow, nchan, 1 .. 4) tensor of {self.cdtype} or complex64: "
                             f"{out.dtype} {tuple(out.shape)}")
        row0, chan0 = int(row0), int(chan0)
        if row0 < 0 or chan0 < 0 or row0 + self.nrow > out.shape[0] or chan0 + self.nchan > out.shape[1]:
            raise ValueError(f"block rows {row0} .. + {self.nrow}, channels {chan0} .. + {self.nchan} outside out "
                             f"{tuple(out.shape)}")
        if self.nsorted == 0:
            return
        with self.lock:
            acc = self._degrid_all(dirty, None, divide_by_n)
            self.run('pfb_wgrid_finish_block', _dev.ptr(acc), _dev.ptr(self.idx), _dev.ptr(self.coord), self.nsorted,
                     self.nchan, _dev.ptr(out), _dev.code(_dev.REAL_OF[out.dtype]), row0, int(out.shape[1]), chan0,
                     int(out.shape[2]), int(bool(accumulate)))

    def hessian(self, x, wgt=None, beam=None):
        """beam * vis2dirty(wgt * dirty2vis(beam * x)), divide_by_n=False both ways (hessian.py:62-106): the
        visibilities stay in sorted slots between the two halves and the beam rides in the image-side kernels."""
        self._check('x', x, self.rdtype, (self.nx, self.ny))
        self._check('weight', wgt, self.rdtype, (self.nrow, self.nchan))
        self._check('beam', beam, self.rdtype, (self.nx, self.ny))
        if self.nsorted == 0:
            return torch.zeros_like(x)
        with self.lock:
            acc = self._degrid_all(x, beam, False)
            val = self._slots[1]
            self.run('pfb_wgrid_weight', _dev.ptr(acc), _dev.ptr(wgt), _dev.ptr(self.idx), self.nsorted, _dev.ptr(val))
            return self._grid_all(val, beam, False)


# ------------------------------------------------------------------------------------------------------ plan cache
_cache = PlanCache(8)
# plans of the cache built (each builds one order) and GeomTables built: the tests count these
cache_stats = {'miss': 0, 'tables': 0}


def plan_for(uvw, freq, mask, nx, ny, pixsize_x, pixsize_y, center_x, center_y, epsilon, do_wgridding, rdtype,
             reproducible=False):
    """The cached plan of these arrays on this geometry; `reproducible` is part of the key, so a default call never finds
    a reproducible plan or the reverse.  The arrays are keyed by _plan.array_key (numpy: address, layout
    and a strided content sample; tensors: data_ptr and version counter); the entry keeps the arrays alive, so that
    their memory cannot come back as DIFFERENT data under the same key (clear_plan_cache() releases plans and
    references)."""
    key = (array_key(uvw), array_key(freq), array_key(mask), int(nx), int(ny), float(pixsize_x), float(pixsize_y),
           float(center_x), float(center_y), float(epsilon), bool(do_wgridding), str(rdtype), bool(reproducible))

    def make():
        cache_stats['miss'] += 1
        return (WgridPlan(uvw, freq, mask, nx, ny, pixsize_x, pixsize_y, center_x, center_y, epsilon, do_wgridding,
                          rdtype, reproducible=reproducible), (uvw, freq, mask))
    return _cache.get(key, make)[0]


def clear_plan_cache():
    _cache.clear()
    _tables.clear()


# ---------------------------------------------------------------------------------------------------- ducc0's API
def _check_flags(do_wgridding, epsilon, pixsize_x, pixsize_y):
    if do_wgridding is None or epsilon is None or pixsize_x is None or pixsize_y is None:
        raise TypeError("pixsize_x, pixsize_y, epsilon and do_wgridding are required")


def vis2dirty(uvw, freq, vis, wgt=None, mask=None, npix_x=None, npix_y=None, pixsize_x=None, pixsize_y=None,
              center_x=0.0, center_y=0.0, epsilon=None, do_wgridding=None, divide_by_n=True,
              double_precision_accumulation=False, nthreads=1, reproducible=False):
    """ducc0.wgridder.experimental.vis2dirty: dirty (npix_x, npix_y) in the real type of vis.  `nthreads` is accepted
    and ignored.  double_precision_accumulation with complex64 input runs the fp64 kernels on the data cast up.

    Beyond ducc0: vis (nprod, nrow, nchan), nprod <= 4 -- the Stokes products of utils.stokes.stokes_vis(product='IQUV')
    -- gives dirty (nprod, npix_x, npix_y) under ONE plan and order, the one a 2-D call on the same arrays finds in the
    cache; wgt is None, (nrow, nchan) for every plane, or (nprod, nrow, nchan).

    reproducible=True grids without atomics, under a plan of its own: the result is identical bit for bit from run to
    run for the same arrays in the same row order (another order of the same visibilities is another sum order)."""
    _check_flags(do_wgridding, epsilon, pixsize_x, pixsize_y)
    if npix_x is None or npix_y is None:
        raise TypeError("npix_x and npix_y are required")
    vd = _dev.to_dev(vis)
    if vd.dtype not in _dev.REAL_OF:
        raise TypeError(f"vis must be complex64 or complex128, got {vd.dtype}")
    rdt_in = _dev.REAL_OF[vd.dtype]
    wd = _dev.to_dev(wgt)
    if wd is not None and wd.dtype != rdt_in:
        raise TypeError(f"wgt must be {rdt_in} for {vd.dtype} visibilities, got {wd.dtype}")
    rdt = torch.float64 if double_precision_accumulation else rdt_in
    if rdt != rdt_in:
        vd, wd = vd.to(torch.complex128), (None if wd is None else wd.to(torch.float64))
    plan = plan_for(uvw, freq, mask, npix_x, npix_y, pixsize_x, pixsize_y, center_x, center_y, epsilon, do_wgridding,
                    rdt, reproducible)
    out = plan.vis2dirty(vd, wd, divide_by_n)
    return _dev.host_like(out.to(rdt_in), vis)


def dirty2vis(uvw, freq, dirty, wgt=None, mask=None, pixsize_x=None, pixsize_y=None, center_x=0.0, center_y=0.0,
              epsilon=None, do_wgridding=None, divide_by_n=True, nthreads=1):
    """ducc0.wgridder.experimental.dirty2vis: vis (nrow, nchan) in the complex type of dirty, 0 where mask == 0.
    Beyond ducc0: dirty (nprod, nx, ny), nprod <= 4, gives vis (nprod, nrow, nchan); wgt as in vis2dirty."""
    _check_flags(do_wgridding, epsilon, pixsize_x, pixsize_y)
    dd = _dev.to_dev(dirty)
    if dd.dtype not in _dev.CPLX_OF or dd.ndim not in (2, 3):
        raise TypeError(f"dirty must be a float32 or float64 image (nx, ny) or a stack (nprod, nx, ny) of them, got "
                        f"{dd.dtype} {tuple(dd.shape)}")
    wd = _dev.to_dev(wgt)
    if wd is not None and wd.dtype != dd.dtype:
        raise TypeError(f"wgt must be {dd.dtype} like dirty, got {wd.dtype}")
    nx, ny = dd.shape[-2:]
    plan = plan_for(uvw, freq, mask, nx, ny, pixsize_x, pixsize_y, center_x, center_y, epsilon, do_wgridding, dd.dtype)
    return _dev.host_like(plan.dirty2vis(dd, wd, divide_by_n), dirty)


# --------------------------------------------------------------------------- the grid worker's products, in one go
def image_data_products(uvw, freq, vis, wgt, mask, counts, nx, ny, nx_psf, ny_psf, cellx, celly, model=None,
                        robustness=None, x0=0.0, y0=0.0, nthreads=1, epsilon=1e-7, do_wgridding=True, double_accum=True,
                        l2reweight_dof=None, do_dirty=True, do_psf=True, do_weight=True, reproducible=False):
    """pfb/operators/gridder.py:551-740: the image-space data products of one band in one go, with the reference's
    keys -- WEIGHT (if do_weight), WSUM (1,), DIRTY, PSF and PSFHAT (if do_psf), RESIDUAL (if a model is given) -- and its
    statements in its order: model visibilities, the l2 reweight, the imaging weights of `robustness` from `counts`
    multiplied into wgt, the dirty image, the PSF on (nx_psf, ny_psf) (from unit visibilities, or for a centre
    (x0, y0) != 0 from the degridded 128 x 128 delta), its transform, the residual image.  divide_by_n=False throughout.

    One plan of the cache per geometry: the (nx, ny) plan serves model, dirty and residual, the (nx_psf, ny_psf) plan the
    PSF (and a 128 x 128 one the delta).  They work in float64 when double_accum is set and in the type of vis otherwise.
    The model is degridded WITH the mask -- which the plan carries -- since residual_vis is multiplied by it anyway.
    reproducible=True takes the plans that grid without atomics: DIRTY, PSF, PSFHAT and RESIDUAL are then identical bit
    for bit from run to run, given weights that are (counts of compute_counts with k = 0 are; with k > 0 they are
    accumulated with float atomics and vary in their last bits).

    Differences from the reference: the caller's wgt is never written (the reference's `wgt *= imwgt` writes into it);
    no weights at all (wgt None, no robustness, no l2 reweight, or an l2 reweight with an all-zero mask and no
    robustness) is a ValueError here and a TypeError on `None[...]` there.  `nthreads` and `do_dirty` are accepted and
    ignored (the reference ignores do_dirty too).  numpy in gives numpy out; with tensors in, the l2 reweight's
    sum of the mask is the one number that is read on the host."""
    if model is None and l2reweight_dof:
        raise ValueError('Requested l2 reweight but no model passed in. '
                         'Perhaps transfer model from somewhere?')
    if robustness is not None and counts is None:
        raise ValueError('counts are None but robustness specified. '
                         'This is probably a bug!')
    vd = _dev.to_dev(vis)
    if vd.dtype not in _dev.REAL_OF or vd.ndim != 2:
        raise TypeError(f"vis must be a (nrow, nchan) complex64 or complex128 array, got {vd.dtype} {tuple(vd.shape)}")
    cdt_in, rdt_in = vd.dtype, _dev.REAL_OF[vd.dtype]
    rdt = torch.float64 if double_accum else rdt_in
    cdt = _dev.CPLX_OF[rdt]
    md = _dev.byte_mask(mask, vd.shape)
    wd = _dev.to_dev(wgt)
    if wd is not None and (wd.dtype != rdt_in or wd.shape != vd.shape):
        raise TypeError(f"wgt must be {rdt_in} of the shape of vis, got {wd.dtype} {tuple(wd.shape)}")
    nx, ny = int(nx), int(ny)

    def plan(npx, npy):
        return plan_for(uvw, freq, mask, npx, npy, cellx, celly, x0, y0, epsilon, do_wgridding, rdt, reproducible)

    def image(p, v, w):
        return p.vis2dirty(v.to(cdt), None if w is None else w.to(rdt), False).to(rdt_in)

    def degrid(p, img):
        return p.dirty2vis(img.to(rdt), None, False).to(cdt_in)

    out = {}
    imwgt = None
    if robustness is not None:
        imwgt = weighting._counts_to_weights(_dev.to_dev(counts, rdt_in), _dev.to_dev(uvw), _dev.to_dev(freq), nx, ny,
                                             cellx, celly, robustness)
    residual_vis = wsum = None
    if model is not None:
        xd = _dev.to_dev(model)
        if xd.dtype not in _dev.CPLX_OF or tuple(xd.shape) != (nx, ny):
            raise TypeError(f"model must be a float32 or float64 image of shape {(nx, ny)}")
        model_vis = degrid(plan(nx, ny), xd)            # no weights in this direction
        residual_vis, wl2, wsum = weighting._l2_reweight_dev(vd, model_vis, md, l2reweight_dof, imwgt)
        if l2reweight_dof:
            wd, imwgt = wl2, (None if wl2 is not None else imwgt)         # the product was formed in the kernel
    if imwgt is not None:
        wd = imwgt if wd is None else wd * imwgt
    if wd is None:
        raise ValueError('no weights: wgt is None and neither robustness nor an l2 reweight gives any')
    if do_weight:
        out['WEIGHT'] = wd
    out['WSUM'] = wsum if wsum is not None else weighting.masked_sum(wd, md)
    out['DIRTY'] = image(plan(nx, ny), vd, wd)
    if do_psf:
        if x0 or y0:
            delta = torch.zeros((128, 128), dtype=rdt, device=vd.device)
            delta[64, 64] = 1.0
            psf_vis = degrid(plan(128, 128), delta)
        else:
            psf_vis = torch.ones(vd.shape, dtype=cdt_in, device=vd.device)
        out['PSF'] = image(plan(int(nx_psf), int(ny_psf)), psf_vis, wd)
        out['PSFHAT'] = psfhat_from_psf(out['PSF'])
    if model is not None:
        out['RESIDUAL'] = image(plan(nx, ny), residual_vis, wd)
    return {key: _dev.host_like(t, vis) for key, t in out.items()}


# ------------------------------------------------------------------------- the predict step: degridding on blocks
def _degrid_blocks(uvw_d, freq_d, blocks, images, out, cellx, celly, x0, y0, epsilon, do_wgridding, divide_by_n,
                   accumulate):
    """images[k] degridded on blocks[k] = (r0, r1, c0, c1) of the device arrays uvw_d, freq_d into out (nrow, nchan,
    ncorr).
    A block's plan -- on uvw[r0:r1], freq[c0:c1], no mask -- is not put into the plan cache, so that a predict call
    evicts nothing that plan_for holds; it takes its tables from the geometry's GeomTables and is closed after use."""
    for (r0, r1, c0, c1), img in zip(blocks, images):
        plan = WgridPlan(uvw_d[r0:r1], freq_d[c0:c1], None, img.shape[0], img.shape[1], cellx, celly, x0, y0, epsilon,
                         do_wgridding, img.dtype, degrid_only=True)
        try:
            plan.dirty2vis_into(img, out, r0, c0, accumulate, divide_by_n)
        finally:
            plan.close()


def _host_ints(a, name):
    """A bin array as int64 numpy (a device tensor comes to the host: bins are tiny)."""
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    if a.ndim != 1 or a.dtype.kind not in 'iu':
        raise ValueError(f"{name} must be a 1-D integer array, got {a.dtype} {a.shape}")
    return a.astype(np.int64)


def _outside(a, n):
    """Does the index array hold an entry outside [0, n)?  numpy is looked at on the host, a tensor where it lives."""
    if len(a) == 0:
        return False
    return bool(a.min() < 0) or bool(a.max() >= n)


def _host_floats(a):
    return (a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).astype(np.float64)


def _bins(idx, cnts, size, name):
    """(start, stop) of every bin, idx shifted by its minimum as the reference shifts it; ValueError for a negative
    count or a bin that reaches outside [0, size)."""
    idx, cnts = _host_ints(idx, name + '_idx'), _host_ints(cnts, name + '_cnts')
    if idx.size == 0 or idx.shape != cnts.shape:
        raise ValueError(f"{name}_idx and {name}_cnts must be non-empty and of one length")
    if (cnts < 0).any():
        raise ValueError(f"{name}_cnts holds a negative count")
    start = idx - idx.min()
    stop = start + cnts
    if stop.max() > size:
        raise ValueError(f"a bin of {name}_idx reaches {int(stop.max())}, beyond the {size} entries it indexes")
    return start, stop


def _im2vis_impl(uvw, freq, image, cellx, celly, freq_bin_idx, freq_bin_counts, x0=0, y0=0, epsilon=1e-7, flip_v=False,
                 do_wgridding=True, divide_by_n=False, nthreads=1):
    """pfb/operators/gridder.py:258-294: band i of the (nband, nx, ny) cube degridded into the channels
    freq_bin_idx[i] - freq_bin_idx.min() .. + freq_bin_counts[i] of a (nrow, nchan) array of result_type(image,
    complex64); channels that no band covers are zero.  A band's channels are what dirty2vis(uvw, freq[ind], image[i])
    gives, bit for bit.  flip_v is not implemented (the w-gridder here has no flip); `nthreads` is accepted and
    ignored."""
    if flip_v:
        raise NotImplementedError("flip_v: the w-gridder has no flip")
    xd = _dev.to_dev(image)
    if xd.dtype not in _dev.CPLX_OF or xd.ndim != 3:
        raise TypeError(f"image must be a (nband, nx, ny) float32 or float64 cube, got {xd.dtype} {tuple(xd.shape)}")
    ud, fd = _dev.uvw_freq(uvw, freq)
    nrow, nchan = int(ud.shape[0]), int(fd.shape[0])
    start, stop = _bins(freq_bin_idx, freq_bin_counts, nchan, 'freq_bin')
    if start.size != xd.shape[0]:
        raise ValueError(f"{start.size} frequency bins for {xd.shape[0]} bands")
    check_epsilon(epsilon, xd.dtype)
    vis = torch.zeros((nrow, nchan, 1), dtype=_dev.CPLX_OF[xd.dtype], device=xd.device)
    live = [i for i in range(start.size) if stop[i] > start[i] and nrow]
    _degrid_blocks(ud, fd, [(0, nrow, int(start[i]), int(stop[i])) for i in live], [xd[i] for i in live], vis, cellx,
                   celly, x0, y0, epsilon, do_wgridding, divide_by_n, False)
    return _dev.host_like(vis.view(nrow, nchan), image)


def _basis_rows(modelf, touts, fouts, nparam):
    """E (len(touts) * len(fouts), nparam): the factor of parameter p at (tout, fout) is modelf(tout, fout, *e_p) -- one
    scalar call per unit vector.  modelf must be linear in its parameters: checked once, at the first (tout, fout), on a
    fixed parameter vector (1.25, -1.625, 2, ..: no entry 0 or 1, where a power of a parameter is the parameter, and a
    sum other than 1, which a constant term would survive), to 1e-12 relative."""
    unit = np.eye(nparam)
    E = np.empty((len(touts), len(fouts), nparam))
    for i, t in enumerate(touts):
        for j, f in enumerate(fouts):
            E[i, j] = [float(modelf(t, f, *unit[p])) for p in range(nparam)]
    if E.size:
        probe = np.array([(-1.0) ** p * (1.25 + 0.375 * p) for p in range(nparam)])
        got, want = float(modelf(touts[0], fouts[0], *probe)), float(E[0, 0] @ probe)
        if not abs(got - want) <= 1e-12 * np.abs(E[0, 0] * probe).sum():
            raise ValueError("modelf is not linear in its parameters: the component model cannot be rendered from its "
                             f"factors (modelf gives {got!r}, the factors {want!r})")
    return E.reshape(len(touts) * len(fouts), nparam)


def _comps2vis_impl(uvw, utime, freq, rbin_idx, rbin_cnts, tbin_idx, tbin_cnts, fbin_idx, fbin_cnts, comps, Ix, Iy,
                    modelf, tfunc, ffunc, nx, ny, cellx, celly, x0=0, y0=0, epsilon=1e-7, nthreads=1, do_wgridding=True,
                    divide_by_n=False, ncorr_out=4, *, out=None, accumulate=False, out_dtype=None):
    """pfb/operators/gridder.py:492-548, the predict step of the degrid worker: the component model (comps (nparam,
    ncomps) at pixels Ix, Iy; modelf, tfunc, ffunc the callables the worker lambdifies) rendered per time bin and band and
    degridded into vis (nrow, nchan, ncorr_out), correlations 0 and -1, of result_type(comps, complex64).

    Time bin t takes the unique times indt = tbin_idx[t] .. + tbin_cnts[t] and the rows indr = rbin_idx[indt][0] ..
    rbin_idx[indt][-1] + rbin_cnts[indt][-1], band b the channels indf = fbin_idx[b] .. + fbin_cnts[b], every index array
    shifted by its minimum; the image of (t, b) is the model at (tfunc(mean(utime[indt])), ffunc(mean(freq[indf]))).  It
    is rendered by the component kernel from the factors modelf(tout, fout, *e_p) -- modelf must be linear in its
    parameters (ValueError otherwise) --, one launch per time bin for all its bands, in the type of comps.

    One deliberate reading of the reference: it hands dirty2vis the WHOLE uvw, not uvw[indr], which runs only where indr
    covers every row -- one time bin per call, as its worker calls it; two time bins in one call raise a broadcast
    ValueError there.  Here a block degrids uvw[indr]: the same wherever the reference runs, and a call with several time
    bins equals the concatenation of the single-bin calls, bit for bit.

    Keyword-only, for the worker's tail: `out` a contiguous (nrow, nchan, ncorr_out) device tensor to write into (zeroed
    first unless `accumulate`: then the model is ADDED, vis += model column); `out_dtype` complex64 narrows an fp64
    model in the kernel (the worker's astype(complex64): cast first, then store or add).  A bin outside utime, uvw or
    freq, a negative count, ncorr_out outside 1 .. 4 and a component outside (nx, ny) are ValueErrors before any launch.
    Empty bins are skipped.  `nthreads` is accepted and ignored.  numpy in gives numpy out."""
    nx, ny, ncorr_out = int(nx), int(ny), int(ncorr_out)
    if not 1 <= ncorr_out <= 4:
        raise ValueError(f"ncorr_out must be 1 .. 4, got {ncorr_out}")
    ud, fd = _dev.uvw_freq(uvw, freq)
    nrow, nchan = int(ud.shape[0]), int(fd.shape[0])
    ut, fh = _host_floats(utime), _host_floats(freq)
    t0, t1 = _bins(tbin_idx, tbin_cnts, ut.size, 'tbin')
    f0, f1 = _bins(fbin_idx, fbin_cnts, nchan, 'fbin')
    rbin_idx, rbin_cnts = _host_ints(rbin_idx, 'rbin_idx'), _host_ints(rbin_cnts, 'rbin_cnts')
    if rbin_idx.shape != rbin_cnts.shape or rbin_idx.size < t1.max():
        raise ValueError(f"a time bin reaches {int(t1.max())}, beyond the {rbin_idx.size} entries of rbin_idx / "
                         "rbin_cnts")
    if (rbin_cnts < 0).any():
        raise ValueError("rbin_cnts holds a negative count")
    rbin_idx2 = rbin_idx - rbin_idx.min()
    cd = _dev.to_dev(comps)
    if cd.dtype not in _dev.CPLX_OF or cd.ndim != 2:
        raise TypeError(f"comps must be a (nparam, ncomps) float32 or float64 array, got {cd.dtype} {tuple(cd.shape)}")
    rdt = cd.dtype
    check_epsilon(epsilon, rdt)
    if _outside(Ix, nx) or _outside(Iy, ny):
        raise ValueError(f"Ix / Iy hold a pixel outside the ({nx}, {ny}) image")
    ixd, iyd = _dev.to_dev(Ix, torch.int64), _dev.to_dev(Iy, torch.int64)
    # ---- the blocks: rows of every live time bin, channels of every live band
    tlive = [t for t in range(t0.size) if t1[t] > t0[t]]
    blive = [b for b in range(f0.size) if f1[b] > f0[b]]
    rows = []
    for t in tlive:
        r0, r1 = int(rbin_idx2[t0[t]]), int(rbin_idx2[t1[t] - 1] + rbin_cnts[t1[t] - 1])
        if r0 > r1 or r1 > nrow:
            raise ValueError(f"time bin {t} maps to rows {r0} .. {r1}, outside the {nrow} rows of uvw")
        rows.append((r0, r1))
    # ---- the output
    cdt = _dev.CPLX_OF[rdt]
    if out is not None:
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.is_contiguous()
                and tuple(out.shape) == (nrow, nchan, ncorr_out) and out.dtype in _dev.REAL_OF):
            raise ValueError(f"out must be a contiguous complex device tensor of shape {(nrow, nchan, ncorr_out)}")
        odt = out.dtype
        if out_dtype is not None and _cplx_dtype(out_dtype) != odt:
            raise ValueError(f"out is {odt} but out_dtype asks for {out_dtype}")
    else:
        odt = cdt if out_dtype is None else _cplx_dtype(out_dtype)
    if odt == torch.complex128 and rdt == torch.float32:
        raise ValueError("a complex128 model column from float32 comps: the kernel narrows, it does not widen")
    touts = [tfunc(np.mean(ut[t0[t]:t1[t]])) for t in tlive]
    fouts = [ffunc(np.mean(fh[f0[b]:f1[b]])) for b in blive]
    E = _basis_rows(modelf, touts, fouts, int(cd.shape[0]))
    # ---- launches
    if out is None:
        vis = torch.zeros((nrow, nchan, ncorr_out), dtype=odt, device=cd.device)
    else:
        vis = out if accumulate else out.zero_()
    nb = len(blive)
    for k, (r0, r1) in enumerate(rows):
        if r1 == r0 or nb == 0 or cd.shape[1] == 0:          # nothing to degrid, or a model without components
            continue
        images = _render(E[k * nb:(k + 1) * nb], nx, ny, cd, ixd, iyd, rdt)
        _degrid_blocks(ud, fd, [(r0, r1, int(f0[b]), int(f1[b])) for b in blive], images, vis, cellx, celly, x0, y0,
                       epsilon, do_wgridding, divide_by_n, accumulate)
    return vis if out is not None else _dev.host_like(vis, uvw)


def _cplx_dtype(dtype):
    if isinstance(dtype, torch.dtype):
        t = dtype
    else:
        t = _dev._NP2T.get(np.dtype(dtype))
    if t not in _dev.REAL_OF:
        raise ValueError(f"out_dtype must be complex64 or complex128, got {dtype}")
    return t


def _loc2psf_vis_impl(uvw, freq, cell, x0=0, y0=0, do_wgridding=True, epsilon=1e-7, nthreads=1, precision='single',
                      divide_by_n=False, convention='CASA'):
    """pfb/operators/gridder.py:298-341: the visibilities of a unit source at the phase centre, (nrow, nchan) complex64
    ('single') or complex128: ones, or for a centre (x0, y0) != 0 the degridded 128 x 128 delta at epsilon 1e-7, the
    reference's fixed value whatever `epsilon`.  That accuracy is below the fp32 kernels' range, so 'single' degrids in
    fp64 and narrows in the landing kernel.  `nthreads` and `convention` are accepted and ignored."""
    ud, fd = _dev.uvw_freq(uvw, freq)
    nrow, nchan = int(ud.shape[0]), int(fd.shape[0])
    cdt = torch.complex64 if precision == 'single' else torch.complex128
    if not (x0 or y0):
        return _dev.host_like(torch.ones((nrow, nchan), dtype=cdt, device=ud.device), uvw)
    delta = torch.zeros((128, 128), dtype=torch.float64, device=ud.device)
    delta[64, 64] = 1.0
    vis = torch.zeros((nrow, nchan, 1), dtype=cdt, device=ud.device)
    if nrow and nchan:
        _degrid_blocks(ud, fd, [(0, nrow, 0, nchan)], [delta], vis, cell, cell, x0, y0, 1e-7, do_wgridding, divide_by_n,
                       False)
    return _dev.host_like(vis.view(nrow, nchan), uvw)


im2vis, comps2vis, loc2psf_vis = _im2vis_impl, _comps2vis_impl, _loc2psf_vis_impl
