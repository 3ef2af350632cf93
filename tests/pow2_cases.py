"""
Case table of the power-of-two convolution kernels (tests/test_cpu_pow2_cases.py, tests/test_gpu_pow2_edges.py): the
three passes of csrc/fftconv_pow2.hip -- forward rows, columns, inverse rows -- in their plain, persistent and two-level
forms, and the PSFHAT producer that runs on the same kernels.

The first half mirrors the library's launch bookkeeping as plain functions of (number format, length, CU count): which
kernel serves a pass, its tile, its grid, the trips of a workgroup and the bands it visits.  Every function names the
constexpr or function of the source it mirrors.  The second half is the case table: every case names the pass it is
aimed at, its class (format, nx, ny), its band count AS A FUNCTION OF THE CU COUNT, the call variants it runs and the
PROPERTY IT EXISTS FOR, a predicate over the mirror.  The predicates are asserted on the CPU at 256 CUs and at 304, so a
case cannot silently stop exercising its edge when a tile, a grid rule or a threshold changes.

Sizes: images (nband, nx, ny) on the (2 nx, 2 ny) PSF grid the fast path requires.  H = nx is the length of a column
transform, L = ny / 2 that of a row transform (real rows run as packed complex transforms).

Groups:
  a  class sweep: every column class 64 .. 8192 at ny = 128 and every row class L = 64 .. 8192 (fp64: 4096) at nx = 64, two
     bands, every call variant with and without beam
  b  column trips of the persistent (H = 2048, 4096) and the two-level (H = 8192) kernel at ny = 128: a second trip with
     inactive slots, a balanced grid below the cap with and without inactive slots, band boundaries inside a workgroup's
     trips; whole and on the band sub-ranges (1, n - 1) and (n - 1, 1)
  c  row trips of the persistent forward and inverse kernels at nx = 64 (XCD pairing on) and nx = 96 (pairing off
     wherever a tile has fewer than 8 rows): fewer tiles than workgroups, one full trip, a second trip of a few tiles (the rotated map's tail and its
     repeat branch), three trips across band boundaries
  d  the non-temporal PSF instantiations of the column kernels: the smallest band count whose PSF share reaches 200 MiB
  e  the PSFHAT producer (pfb_psfconv_set_psf with psfhat_out) for every column and every row class

Device footprint (x, out, operands, T, psf_l, partials at 256 CUs): 128 MB hold the class sweep and the producer but for
their largest classes; the trip cases cannot be that small (the persistent grids are one workgroup per CU, so a full trip
is 256 tiles whatever the image) and are held to 512 MB like the non-temporal ones, the three-trip row cases (513 tiles
and more) to 768 MB.  Every case of the table is run.  tests/test_cpu_pow2_cases.py asserts the three caps.

Plain Python, numpy and scipy: no GPU and no torch.  The references are float64 through oracle.fftconv.
"""
import numpy as np

from oracle import fftconv as ofc

F32, F64 = 'float32', 'float64'
DTYPES = (F32, F64)
RSZ = {F32: 4, F64: 8}                  # bytes of one real value
CSZ = {F32: 8, F64: 16}                 # bytes of one complex value
NVB = {F32: 2, F64: 1}                  # FastCfg<T>::NVB: complex values of one 16-byte block
LDS_MAX = 160 * 1024                    # LDS_MAX
LDS_BUDGET = 152 * 1024                 # LDS_BUDGET
POW2 = (64, 128, 256, 512, 1024, 2048, 4096, 8192)      # for_pow2_size
ROW_TILE_MAX = 32                       # ROW_TILE_MAX
INV_ROT = 3                             # INV_ROT
PSF_NT_BYTES = 200 << 20                # launch_col: psf_nt
ECOLX = 8                               # ECOLX
MB = 1e6
CAP_BYTES = 128 * MB                    # device footprint of a case at 256 CUs; where a class cannot have its property
CAP_BYTES_BIG = 512 * MB                # below it (test_cpu_pow2_cases.py pins which), this one;
CAP_BYTES_THREE = 768 * MB              # the three-trip row cases: 513 tiles and more at 256 CUs
NTHREADS = 8                            # of the float64 references


# ------------------------------------------------------------------------------------------- mirror: transforms
def odd_part(n):
    """fft_pow2.hpp odd_part"""
    while n > 1 and n % 2 == 0:
        n //= 2
    return n


def rmax_of(E):
    """fft_pow2.hpp rmax_of"""
    return min(E & -E, 16)


def pass_radix(N, E, P):
    """fft_pow2.hpp pass_radix"""
    N2 = N // odd_part(N)
    return min(rmax_of(E), N2 // P) if P < N2 else odd_part(N)


def ptw_total(N, E):
    """fft_pow2.hpp ptw_total = ptw_offset(N, E, N)"""
    off, p = 0, pass_radix(N, E, 1)
    while p < N:
        off += 4 * p
        p *= pass_radix(N, E, p)
    return off


def fft_xpad(P, R, c, CB):
    """fft_pow2.hpp fft_xpad"""
    slots = 128 // CB
    return c + c // slots if P == 1 else c if P >= slots else c + (c // (P * R)) * P


def fft_lds_elems(N, E, CB):
    """fft_pow2.hpp fft_lds_elems"""
    RM = rmax_of(E)
    if odd_part(N) == 1:
        return N + N // min(RM, 128 // CB)
    need, P = N + (N >> 4) + 1, 1
    while P * pass_radix(N, E, P) < N:
        need = max(need, fft_xpad(P, pass_radix(N, E, P), N - 1, CB) + 1)
        P *= pass_radix(N, E, P)
    return (need + 1) & ~1


class RegFft:
    """fft_pow2.hpp RegFft<T, N, E>: TPB, LDS_ELEMS, PTWC"""
    def __init__(self, dtype, N, E):
        self.TPB, self.LDS_ELEMS, self.PTWC = N // E, fft_lds_elems(N, E, CSZ[dtype]), ptw_total(N, E) // 4
        self.PTWP = (self.PTWC + 1) & ~1


def fast_nblocks(L, nvb):
    """fast_nblocks: 16-byte column blocks of the even and the odd bins"""
    return (L + nvb) // nvb + L // nvb


# ------------------------------------------------------------------------------------------- mirror: columns
def mix_col_len(nx):
    """mix_col_len"""
    return odd_part(nx) in (3, 5) and 96 <= nx <= 6144


def col_two_level(nx):
    """col_two_level"""
    return odd_part(nx) == 1 and nx >= 8192


def ecol(dtype, H):
    """ecol<T, H>"""
    if odd_part(H) > 1:
        return 12 if H % 3 == 0 else 10                 # mix_col_e
    if H >= 8192 and dtype == F64:
        return 16
    return 4 if 64 <= H <= 1024 else 8                  # COL_E4_MAXH, FastCfg<T>::ECOL


def col_groups(H, E):
    """col_groups<H, E>"""
    return 1 if H // E >= 256 else 256 // (H // E)


def col_resident(threads):
    """col_resident"""
    return max(1, (8 * 64) // threads)


def balanced_grid(need, maxgrid):
    """balanced_grid"""
    if need <= maxgrid:
        return need
    trips = -(-need // maxgrid)
    return -(-need // trips)


class ColCfg:
    """ColCfg<T, H> with ColX<T, H, ECOLX> and ColCfg::shape(): KIND, DB and the serving kernel's gc, threads, lds,
    wg_per_cu"""
    def __init__(self, dtype, H):
        cs, nvb = CSZ[dtype], NVB[dtype]
        self.E1 = ecol(dtype, H)
        f1 = RegFft(dtype, H, self.E1)
        self.GC1 = col_groups(H, self.E1)
        self.NT1 = self.GC1 * f1.TPB
        self.XB1 = cs * self.GC1 * nvb * f1.LDS_ELEMS
        self.TAB1 = cs * f1.PTWP
        self.KIND = ('plain' if odd_part(H) > 1 else 'twolevel' if col_two_level(H)
                     else 'persistent' if H >= 2048 and self.XB1 + self.TAB1 <= LDS_MAX else 'plain')
        self.DB = self.KIND == 'persistent' and col_resident(self.NT1) == 1 and 2 * self.XB1 + self.TAB1 <= LDS_MAX
        if self.KIND == 'twolevel':
            fx = RegFft(dtype, H // 2, ECOLX)
            gc = col_groups(H // 2, ECOLX)
            nt = gc * fx.TPB
            lds = cs * (fx.PTWP + fx.TPB + gc * nvb * fx.LDS_ELEMS + nt * ECOLX * nvb)          # ColX::LDS
            wg = min(col_resident(nt), max(1, LDS_MAX // lds))
            self.gc, self.threads, self.lds, self.wg_per_cu = gc, nt, lds, wg
        elif self.KIND == 'persistent':
            self.gc, self.threads, self.lds, self.wg_per_cu = (self.GC1, self.NT1, (2 if self.DB else 1) * self.XB1 + self.TAB1,
                                                                col_resident(self.NT1))
        else:
            self.gc, self.threads, self.lds, self.wg_per_cu = self.GC1, self.NT1, self.XB1, 0


def psf_elems_per_band(dtype, nx, ny):
    """pfb_psfconv_plan_create: psf_elems_per_band = nvb P VB on a fast plan"""
    return fast_nblocks(ny // 2, NVB[dtype]) * 2 * nx * NVB[dtype]


def T_elems_per_band(dtype, nx, ny):
    """pfb_psfconv_plan_create: T_elems_per_band"""
    return fast_nblocks(ny // 2, NVB[dtype]) * nx * NVB[dtype]


def psf_nt(dtype, nx, ny, nb):
    """launch_col: psf_nt, the launch's share of the PSF spectrum against 200 MiB"""
    return CSZ[dtype] * psf_elems_per_band(dtype, nx, ny) * nb >= PSF_NT_BYTES


class ColLaunch:
    """launch_col<T, H> on bands [band0, band0 + nb) and the item loop of k_col_pow2p / k_col_pow2x: grid, trips
    (niter), the inactive slots of the last trip and the bands a workgroup visits (descending: band_first)."""
    def __init__(self, dtype, nx, ny, band0, nb, ncu):
        c = self.cfg = ColCfg(dtype, nx)
        self.dtype, self.nx, self.kind, self.band0, self.nb = dtype, nx, c.KIND, band0, nb
        self.nblk = fast_nblocks(ny // 2, NVB[dtype])
        self.nt = False
        if c.KIND == 'plain':
            self.grid, self.trips, self.inactive, self.maxgrid = (-(-self.nblk // c.gc)) * nb, 1, 0, None
            return
        self.nt = psf_nt(dtype, nx, ny, nb)
        self.band_first = band0 + nb - 1
        self.nitems = self.nblk * nb
        need = -(-self.nitems // c.gc)
        self.maxgrid = ncu * c.wg_per_cu
        self.grid = balanced_grid(need, self.maxgrid) if c.KIND == 'persistent' else min(need, self.maxgrid)
        self.stride = self.grid * c.gc
        self.trips = -(-self.nitems // self.stride)                 # niter
        self.inactive = self.trips * self.stride - self.nitems

    def kernel(self):
        if self.kind == 'plain':
            return ('col', self.dtype, self.nx)
        return ('colp' if self.kind == 'persistent' else 'colx', self.dtype, self.nx, self.nt)

    def bands_of(self, w, g=0):
        """per trip the band of workgroup w's group g, None for an inactive trip (item_of, col_of)"""
        out = []
        for it in range(self.trips):
            item = w * self.cfg.gc + g + it * self.stride
            out.append(self.band_first - item // self.nblk if item < self.nitems else None)
        return out

    def crosses_band(self):
        """a workgroup whose active trips lie in more than one band"""
        return self.kind != 'plain' and any(len({b for b in self.bands_of(w) if b is not None}) > 1 for w in range(self.grid))

    def boundary_between_trips(self):
        """the band boundary of the item order falls between the slots of one trip for some band: workgroup w and w + 1
        work in different bands in the same trip"""
        return self.kind != 'plain' and any(self.bands_of(w)[it] != self.bands_of(w + 1)[it] and None not in
                                            (self.bands_of(w)[it], self.bands_of(w + 1)[it])
                                            for it in range(self.trips) for w in range(self.grid - 1))


# ------------------------------------------------------------------------------------------- mirror: rows
def row_lengths(dtype):
    """pow2_supported: ny up to 16384 (fp32), 8192 (fp64)"""
    return POW2 if dtype == F32 else POW2[:-1]


class RowCfg:
    """RowCfg<T, L, INVK>: E, TPB, WAVE, GMAX (power-of-two L)"""
    def __init__(self, dtype, L, inv):
        emax = ((16 if L == 4096 else 8) if inv else 16) if dtype == F32 else 8
        self.E = 8 if L // 64 < 8 else min(L // 64, emax)
        self.TPB = L // self.E
        self.WAVE = self.TPB <= 64
        self.GMAX = 4 if inv else 8


def row_groups(dtype, L, E, GMAX):
    """row_groups<T, L, E, GMAX>: rows per workgroup of the plain row kernels"""
    TPB = L // E
    G = max(256 // TPB, GMAX)
    stride = fft_lds_elems(L, E, CSZ[dtype]) + 4
    while G > 1 and (G * TPB > 1024 or G * stride * CSZ[dtype] + 384 > LDS_BUDGET):
        G //= 2
    return G


class FwdP:
    """FwdP<T, L>: the persistent forward row kernel's tile and whether it serves the class (OK)"""
    def __init__(self, dtype, L):
        cs, nvb = CSZ[dtype], NVB[dtype]
        self.BIG = L >= 4096
        self.E = 16 if L >= 2048 else 8
        f = RegFft(dtype, L, self.E)
        self.TPR = L // self.E
        self.NT = 1024
        self.G = self.NT // self.TPR
        self.BSTEP = self.NT // self.G
        self.NTM = nvb * self.BSTEP if self.BIG else L
        self.LDS = cs * (f.PTWP + self.NTM + self.G * (f.LDS_ELEMS + 4))
        self.KR = (32 * nvb * self.BSTEP) // (2 * L)
        self.OK = (self.E == 16 and self.LDS <= LDS_MAX and not (self.BIG and dtype == F64) and
                   (not self.BIG or (32 * self.TPR == 2 * L and self.KR * 2 * L == 32 * nvb * self.BSTEP
                                     and self.NTM >= self.TPR)))
        self.SH = 8 // self.G                              # FwdP::tile_row: SH


def inv_pe(dtype, L):
    """InvPE<T, L>::E"""
    return 16 if dtype == F64 and L >= 4096 else RowCfg(dtype, L, True).E


class InvP:
    """InvP<T, L, InvPE<T, L>::E>: the persistent inverse row kernel's tile and whether it serves the class (OK);
    PER_BAND: inv_pb_ok; SH as in k_row_inv_pow2p"""
    def __init__(self, dtype, L):
        cs, nvb = CSZ[dtype], NVB[dtype]
        E = self.E = inv_pe(dtype, L)
        c = RowCfg(dtype, L, True)
        f = RegFft(dtype, L, E)
        self.PARK = dtype == F32 and E < 16
        self.G = (1024 if dtype == F32 else 512) // f.TPB
        self.NT = self.G * f.TPB
        self.SMT = E >= 16
        self.NTM = f.TPB if self.SMT else L
        self.LDS = 384 + cs * (f.PTWP + self.NTM + self.G * (f.LDS_ELEMS + 4) + (self.G * L if self.PARK else 0))
        size_ok = (self.NT == 1024 and 4 <= self.G <= 16) if dtype == F32 else (self.NT == 512 and self.G in (2, 4) and L >= 1024)
        self.OK = (odd_part(L) == 1 and self.LDS <= LDS_MAX and not c.WAVE and (not self.SMT or 32 * f.TPB == 2 * L) and size_ok)
        self.PER_BAND = self.OK and odd_part(L) == 1 and not (dtype == F32 and self.SMT)
        self.SH = max(1, 128 // (self.G * cs * nvb)) if self.G else 1


def pairing(SH, tiles_per_band):
    """xcd_line_pair (FwdP::tile_row, xcd_row_group) and k_row_inv_pow2p `pairing`: the XCD piece pairing is on"""
    return SH > 1 and tiles_per_band % (8 * SH) == 0


def tile_row(rg, tiles_per_band, SH, G):
    """FwdP::tile_row / the `tile` lambda of k_row_inv_pow2p (xcd_paired): tile rg of a band -> its first image row"""
    if pairing(SH, tiles_per_band):
        q, rem = divmod(rg, 8 * SH)
        rg = SH * (q * 8 + (rem & 7)) + (rem >> 3)
    return rg * G


class RowFwd:
    """RowFwdK<T, L> and launch_row_fwd: kernel, rows per tile, grid, the tiles a workgroup walks (static map: tile =
    workgroup + trip x grid)."""
    def __init__(self, dtype, L, nx=None, nb=None, ncu=None):
        fp = FwdP(dtype, L)
        self.dtype, self.L, self.PERSISTENT = dtype, L, fp.OK
        if fp.OK:
            self.E, self.G, self.SH, self.wg_per_cu = fp.E, fp.G, fp.SH, 1     # one resident workgroup per CU
        else:
            c = RowCfg(dtype, L, False)
            self.E, self.G, self.wg_per_cu = c.E, row_groups(dtype, L, c.E, c.GMAX), 0
            self.SH = 8 // self.G                           # xcd_row_group<G>
        if nx is not None:
            self.tiles_per_band = nx // self.G
            self.ntiles = self.tiles_per_band * nb
            self.cap = ncu * self.wg_per_cu if fp.OK else self.ntiles
            self.grid = min(self.ntiles, self.cap)
            self.pairing = pairing(self.SH, self.tiles_per_band)

    def kernel(self, beam):
        return ('fwdq', self.dtype, self.L, bool(beam)) if self.PERSISTENT else ('fwd', self.dtype, self.L)

    def reachable(self):
        """RowFwdK::reachable"""
        return {self.kernel(False), self.kernel(True)}

    def tiles_of(self, b):
        return list(range(b, self.ntiles, self.grid)) if self.PERSISTENT else [b]

    def repeats(self, b):
        """k_row_fwd_pow2q: 'last tile: harmless repeat' -- every workgroup ends on it"""
        return self.PERSISTENT


def inv_tiles(grid, ntiles, b):
    """k_row_inv_pow2p: the tiles workgroup b of `grid` walks -- trip s takes tile (b + s INV_ROT) mod grid + s grid, and
    the first candidate past the end is the repeat that ends the loop"""
    if b >= ntiles:
        return []
    out, s = [b], 1
    while True:
        cand = (b + s * INV_ROT) % grid + s * grid
        if cand >= ntiles:
            return out
        out.append(cand)
        s += 1


class RowInv:
    """RowInvK<T, L> and launch_row_inv: which kernel a call variant reaches and the launches it makes."""
    def __init__(self, dtype, L):
        ip = self.ip = InvP(dtype, L)
        c = RowCfg(dtype, L, True)
        self.dtype, self.L, self.PERSISTENT, self.PER_BAND = dtype, L, ip.OK, ip.PER_BAND
        self.E, self.EP = c.E, ip.E
        self.G_plain = row_groups(dtype, L, c.E, c.GMAX)                    # rows_per_wg
        self.SH_plain = 8 // self.G_plain
        self.G = ip.G if ip.OK else self.G_plain
        self.SH = ip.SH if ip.OK else self.SH_plain

    def plain(self):
        return ('inv', self.dtype, self.L)

    def reachable(self):
        """RowInvK::reachable"""
        out = {self.plain()}
        if self.PERSISTENT:
            for beam in (False, True):
                out |= {('invp', self.dtype, self.L, m, beam, False) for m in (0, 1, 2)}
                if self.PER_BAND:
                    out.add(('invp', self.dtype, self.L, 2, beam, True))
        return out

    def launches(self, nx, nband, nb, ncu, entry, dw, dw2, beam):
        """[(kernel, grid, bands of the launch, tiles_per_band)] of one call (launch_row_inv)"""
        if self.PERSISTENT and dw in (None, 'x'):
            ip = self.ip
            mode = 0 if dw is None else 1 if dw2 is None else 2
            tpb = nx // ip.G
            ntiles, cap = tpb * nb, ncu                                      # one resident workgroup per CU
            grid = min(ntiles, cap)
            if entry == 'bands' and dw:
                if self.PER_BAND and dw2:
                    if grid * nb > nx * nband:
                        grid = nx * nband // nb                              # the partials hold nx x nband slots
                    return [(('invp', self.dtype, self.L, 2, beam, True), grid, nb, tpb)]
                return [(('invp', self.dtype, self.L, mode, beam, False), min(tpb, cap), 1, tpb)] * nb
            return [(('invp', self.dtype, self.L, mode, beam, False), grid, nb, tpb)]
        tpb = nx // self.G_plain
        return [(self.plain(), tpb * nb, nb, tpb)]


def pow2_supported(dtype, nx, ny):
    """pow2_supported on the (2 nx, 2 ny) grid, power-of-two rows"""
    col_ok = (odd_part(nx) == 1 and 64 <= nx <= 8192) or mix_col_len(nx)
    row_ok = odd_part(ny) == 1 and 128 <= ny <= (16384 if dtype == F32 else 8192)
    return col_ok and row_ok and nx % ROW_TILE_MAX == 0


# ------------------------------------------------------------------------------------------- call variants
# name -> (entry point, dot_with, dot_with2).  'x': the image itself (the persistent inverse kernel's modes 1 and 2),
# 'w' / 'w2': independent arrays (the plain inverse kernel with its fused sums, whatever the class)
CALLS = {'none': ('apply', None, None), 'dot-x': ('dots', 'x', None), 'dot-x-w': ('dots', 'x', 'w'),
         'dot-w': ('dots', 'w', None), 'dot-w-w2': ('dots', 'w', 'w2'), 'bands-x': ('bands', 'x', None),
         'bands-x-w': ('bands', 'x', 'w'), 'bands-w-w2': ('bands', 'w', 'w2')}
ALL_CALLS = tuple(CALLS)
# with beam: out = beam conv(beam x) / wsum + sigmainv x; without: the bare convolution
BEAM_ARGS = {False: (0.0, 0.0), True: (1.3, 0.7)}           # (wsum, sigmainv); wsum 0: none


def variants(calls, beams=(False, True)):
    return tuple((c, b) for b in beams for c in calls)


# ------------------------------------------------------------------------------------------- cases
class Case:
    def __init__(self, group, name, target, dtype, nx, ny, nband, variants, prop, subranges=False, why=''):
        self.group, self.name, self.target, self.dtype, self.nx, self.ny = group, name, target, dtype, nx, ny
        self._nband, self.variants, self.prop, self.subranges, self.why = nband, tuple(variants), prop, subranges, why

    @property
    def id(self):
        return f"{self.group}-{self.name}-{'f32' if self.dtype == F32 else 'f64'}"

    @property
    def L(self):
        return self.ny // 2

    def nband(self, ncu):
        return self._nband(ncu) if callable(self._nband) else self._nband

    def holds(self, ncu):
        return bool(self.prop(self, ncu))

    def ranges(self, ncu):
        """(band0, nb) of the launches: the whole cube and, where asked for, the two sub-ranges"""
        n = self.nband(ncu)
        return [(0, n)] + ([(1, n - 1), (n - 1, 1)] if self.subranges and n >= 2 else [])

    def col(self, ncu, rng=None):
        band0, nb = rng or (0, self.nband(ncu))
        return ColLaunch(self.dtype, self.nx, self.ny, band0, nb, ncu)

    def fwd(self, ncu, rng=None):
        return RowFwd(self.dtype, self.L, self.nx, (rng or (0, self.nband(ncu)))[1], ncu)

    def inv(self):
        return RowInv(self.dtype, self.L)

    def inv_launches(self, ncu, variant, rng=None):
        (call, beam), nb = variant, (rng or (0, self.nband(ncu)))[1]
        return self.inv().launches(self.nx, self.nband(ncu), nb, ncu, *CALLS[call], beam)

    def kernels(self, ncu):
        """every kernel instantiation the case launches at this CU count"""
        out = set()
        if self.target == 'producer':
            return out
        for rng in self.ranges(ncu):
            out.add(self.col(ncu, rng).kernel())
            for v in self.variants:
                out.add(self.fwd(ncu, rng).kernel(v[1]))
                out |= {k for k, _, _, _ in self.inv_launches(ncu, v, rng)}
        return out

    def operands(self):
        """the operand arrays beside x and out that the variants read"""
        names = set()
        for call, beam in self.variants:
            names |= {n for n in CALLS[call][1:] if n not in (None, 'x')}
            if beam:
                names.add('beam')
        return sorted(names)

    def footprint(self, ncu=256):
        """device bytes: x, out, the operands, T, psf_l and the partials (the caller's psfhat is released once it is
        installed and compared; the producer's PSF, its psfhat_out and its four-slot scratch count instead)"""
        n, d = self.nband(ncu), self.dtype
        img = RSZ[d] * n * self.nx * self.ny
        plan = CSZ[d] * n * (T_elems_per_band(d, self.nx, self.ny) + psf_elems_per_band(d, self.nx, self.ny)) + 24 * self.nx * n
        if self.target == 'producer':
            P, Q = 2 * self.nx, 2 * self.ny
            return (plan + RSZ[d] * n * P * Q + CSZ[d] * n * P * (self.ny + 1) + 4 * CSZ[d] * T_elems_per_band(d, self.nx, self.ny)
                    + 2 * img)
        return plan + img * (2 + len(self.operands()))

    def cap(self):
        return CAP_BYTES_THREE if self.group == 'c' and '-three' in self.name else CAP_BYTES_BIG

    def __repr__(self):
        return f"Case({self.id}: {self.target} {self.dtype} {self.nx} x {self.ny})"


def smallest_nb(pred, lo=1, hi=200):
    """the smallest band count in [lo, hi] with the property"""
    for n in range(lo, hi + 1):
        if pred(n):
            return n
    raise ValueError("no band count has the property")


# ---- what the table expects of the library (checked against the mirror, which is checked against the source)
COL_KIND = {64: 'plain', 96: 'plain', 128: 'plain', 256: 'plain', 512: 'plain', 1024: 'plain', 2048: 'persistent',
            4096: 'persistent', 8192: 'twolevel'}
FWD_PERSISTENT = {(F32, 2048), (F32, 4096)}
INV_PERSISTENT = {(d, L) for d in DTYPES for L in (1024, 2048, 4096)}
INV_PER_BAND = INV_PERSISTENT - {(F32, 4096)}
TRIP_COLS = (2048, 4096, 8192)


# ---- predicates
def p_sweep(case, ncu):
    """the class is served by the kernels the table expects, on a fast plan"""
    d, L = case.dtype, case.L
    return (pow2_supported(d, case.nx, case.ny) and case.col(ncu).kind == COL_KIND[case.nx]
            and case.fwd(ncu).PERSISTENT == ((d, L) in FWD_PERSISTENT) and case.inv().PERSISTENT == ((d, L) in INV_PERSISTENT)
            and case.inv().PER_BAND == ((d, L) in INV_PER_BAND) and not case.col(ncu).nt)


def col_edge(edge, dtype, nx, ny, nb, ncu):
    """the column trip edges of group b"""
    c = ColLaunch(dtype, nx, ny, 0, nb, ncu)
    if c.kind == 'plain' or c.nt:
        return False
    if edge == 'remainder':             # two-level, unbalanced: a full grid and a second trip of less than a band's items
        return c.kind == 'twolevel' and c.grid == c.maxgrid and c.trips == 2 and 0 < c.nitems - c.stride < c.nblk
    if edge == 'three':                 # two-level: three trips, the last one partly inactive
        return c.kind == 'twolevel' and c.trips == 3 and c.inactive > 0 and c.crosses_band()
    if edge == 'balanced-full':         # persistent: a balanced grid strictly below the cap, no inactive slot
        return c.kind == 'persistent' and c.trips >= 2 and c.grid < c.maxgrid and c.inactive == 0 and c.crosses_band()
    if edge == 'balanced-inactive':     # persistent: the same with an inactive last trip
        return c.kind == 'persistent' and c.trips >= 2 and c.grid < c.maxgrid and c.inactive > 0 and c.crosses_band()
    if edge == 'three-p':               # persistent: three trips, a workgroup in three bands
        return (c.kind == 'persistent' and c.trips == 3 and c.grid < c.maxgrid
                and any(len(set(c.bands_of(w)) - {None}) == 3 for w in range(c.grid)))
    raise KeyError(edge)


def p_col(edge):
    def prop(case, ncu):
        n = case.nband(ncu)
        sub = ColLaunch(case.dtype, case.nx, case.ny, 1, n - 1, ncu)
        # whole: the edge; sub-range (1, n - 1): band0 > 0 and still more than one trip or a band boundary inside a trip
        # (a case of two bands has one-band sub-ranges: the three-trip case of its class is the one with such a sub-range)
        return (col_edge(edge, case.dtype, case.nx, case.ny, n, ncu) and case.subranges and n >= 2
                and (n == 2 or sub.trips >= 2 or sub.boundary_between_trips()) and sub.band_first == n - 1)
    return prop


def row_edge(edge, target, dtype, L, nx, nb, ncu):
    """the row trip edges of group c, for the persistent forward ('fwd') or inverse ('inv') kernel"""
    if target == 'fwd':
        k = RowFwd(dtype, L, nx, nb, ncu)
        if not k.PERSISTENT:
            return False
        ntiles, cap, tpb = k.ntiles, k.cap, k.tiles_per_band
        walks = [k.tiles_of(b) for b in range(k.grid)]
    else:
        k = RowInv(dtype, L)
        if not k.PERSISTENT:
            return False
        tpb = nx // k.G
        ntiles, cap = tpb * nb, ncu
        walks = [inv_tiles(min(ntiles, cap), ntiles, b) for b in range(min(ntiles, cap))]
    assert sorted(t for w in walks for t in w) == list(range(ntiles)), "the tile map is a bijection"
    bands = [{t // tpb for t in w} for w in walks]
    if edge == 'part':                  # fewer tiles than workgroups, two bands: the grid is the tile count
        return nb == 2 and ntiles + tpb <= cap and all(len(w) == 1 for w in walks) and len(walks) == ntiles
    if edge == 'full':                  # one trip, as full as whole bands allow (ntiles = grid where tpb divides the cap)
        return ntiles <= cap < ntiles + tpb and all(len(w) == 1 for w in walks)
    if edge == 'tail':                  # a second trip of fewer tiles than workgroups: some repeat, some go on
        r = ntiles - cap
        two = [b for b, w in enumerate(walks) if len(w) == 2]
        wrapped = target == 'fwd' or (any(b >= cap - INV_ROT for b in two) and len(two) == r)
        return 0 < r <= tpb and len(two) == r and wrapped and any(len(w) == 1 for w in walks)
    if edge == 'three':                 # three trips, the third partial, a workgroup in three bands
        return (2 * cap < ntiles < 3 * cap and any(len(w) == 3 for w in walks) and any(len(w) == 2 for w in walks)
                and any(len(b) == 3 for b in bands))
    raise KeyError(edge)


def p_row(edge, want_pairing):
    def prop(case, ncu):
        k = case.fwd(ncu) if case.target == 'fwd' else case.inv()
        tpb = case.nx // k.G
        on = pairing(k.SH, tpb)
        return (row_edge(edge, case.target, case.dtype, case.L, case.nx, case.nband(ncu), ncu)
                and on == (want_pairing and k.SH > 1) and (want_pairing or k.SH == 1 or not on))
    return prop


def p_nt(case, ncu):
    """the launch reads the PSF with non-temporal loads and one band fewer would not"""
    n = case.nband(ncu)
    return (case.col(ncu).nt and not psf_nt(case.dtype, case.nx, case.ny, n - 1) and case.col(ncu).kind != 'plain'
            and case.col(ncu).trips >= 2)


def p_producer(case, ncu):
    return pow2_supported(case.dtype, case.nx, case.ny) and case.col(ncu).kind == COL_KIND[case.nx]


# ---- the table
ROW_EDGES = ('part', 'full', 'tail', 'three')
COL_EDGES = {'persistent': ('balanced-full', 'balanced-inactive', 'three-p'), 'twolevel': ('remainder', 'three')}
PERSISTENT_CALLS = ('none', 'dot-x', 'dot-x-w', 'bands-x', 'bands-x-w')


def _cases():
    out = []

    def add(*a, **k):
        out.append(Case(*a, **k))

    for d in DTYPES:
        # a. class sweep
        for H in POW2:
            add('a', f'col{H}', 'sweep', d, H, 128, 2, variants(ALL_CALLS), p_sweep)
        for L in row_lengths(d)[1:]:                      # (L = 64 is the partner of every column case)
            add('a', f'row{L}', 'sweep', d, 64, 2 * L, 2, variants(ALL_CALLS), p_sweep)
        # b. column trips: the smallest band count with the edge, whole and on two sub-ranges
        for H in TRIP_COLS:
            for edge in COL_EDGES[COL_KIND[H]]:
                nb = (lambda ncu, e=edge, dd=d, h=H: smallest_nb(lambda n: col_edge(e, dd, h, 128, n, ncu), 2))
                add('b', f'col{H}-{edge}', 'col', d, H, 128, nb, (('none', False), ('dot-x-w', True)), p_col(edge), subranges=True)
        # c. row trips of the persistent row kernels
        for target, classes in (('fwd', sorted(L for dd, L in FWD_PERSISTENT if dd == d)),
                                ('inv', sorted(L for dd, L in INV_PERSISTENT if dd == d))):
            for L in classes:
                for nx in (64, 96):
                    for edge in ROW_EDGES:
                        nb = (lambda ncu, e=edge, t=target, dd=d, ll=L, n=nx:
                              smallest_nb(lambda k: row_edge(e, t, dd, ll, n, k, ncu), 1))
                        calls = PERSISTENT_CALLS if target == 'inv' else ('none',)
                        # (the one-trip cases with and without beam,
                        # the inverse kernel's larger cases with either: a reference each; the forward kernel has one call)
                        beams = ((False, True) if target == 'fwd' or edge in ('part', 'full') else
                                 (nx == 64,) if edge == 'tail' else (nx != 64,))
                        add('c', f'{target}{L}-nx{nx}-{edge}', target, d, nx, 2 * L, nb, variants(calls, beams),
                            p_row(edge, nx == 64), subranges=edge == 'three')
        # d. non-temporal PSF reads
        for H in TRIP_COLS:
            nb = (lambda ncu, dd=d, h=H: smallest_nb(lambda n: psf_nt(dd, h, 128, n), 2))
            add('d', f'nt{H}', 'col', d, H, 128, nb, (('none', False),), p_nt)
        # e. the producer
        for H in POW2:
            add('e', f'col{H}', 'producer', d, H, 128, 2, (('none', False),), p_producer)
        for L in row_lengths(d)[1:]:
            add('e', f'row{L}', 'producer', d, 64, 2 * L, 2, (('none', False),), p_producer)
    return out


CASES = _cases()


def fits(case, ncu=256):
    return case.footprint(ncu) <= case.cap()


RUN_CASES = CASES                       # every case is run; the CPU module asserts that each fits its cap


def by_id(cid):
    return next(c for c in CASES if c.id == cid)


def run_params(groups):
    """the cases of `groups`, sorted by image size so that cases of one size follow each other (see store)"""
    return sorted((c for c in RUN_CASES if c.group in groups), key=lambda c: (c.nx, c.ny))


# ------------------------------------------------------------------------------------------- inputs and references
INPUT_KINDS = ('noise', 'impulse')
IMPULSE_COLS = lambda ny: (0, 1, ny // 2, ny - 1)           # noqa: E731


def f32_exact(a):
    """Round to float32 / complex64 and back: both number formats then see the same values."""
    a = np.asarray(a)
    return a.astype(np.complex64).astype(np.complex128) if np.iscomplexobj(a) else a.astype(np.float32).astype(np.float64)


def tile_rows(case, ncu=256):
    """rows per tile of the kernel the case is aimed at (the inverse kernel's where it is aimed at none)"""
    return case.fwd(ncu).G if case.target == 'fwd' else case.inv().G


def impulse_rows(nx, G):
    """first and last row of the first, a middle and the last tile"""
    tiles = nx // G
    return list(dict.fromkeys(t * G + r for t in (0, tiles // 2, tiles - 1) for r in (0, G - 1)))


def impulse_tile(case, ncu=256):
    return min(tile_rows(case, ncu), case.nx)


def impulse_position(nx, ny, G, b):
    """band b -> (row, column): a different tile-edge row in each band, the columns 0, 1, ny / 2, ny - 1 in turn"""
    rows, cols = impulse_rows(nx, G), IMPULSE_COLS(ny)
    return rows[b % len(rows)], cols[(b + b // len(rows)) % 4]


def impulse_positions(case, ncu):
    return [impulse_position(case.nx, case.ny, impulse_tile(case, ncu), b) for b in range(case.nband(ncu))]


def _rng(nx, ny, b, salt):
    """the generator of band b of the images of (nx, ny): a band holds the same values whatever case asks for it"""
    return np.random.default_rng([9000, nx, ny, b, salt])


class _Store:
    """The arrays of one image size, band by band.  Band b depends on (nx, ny, b) alone, so a case of n bands reads the
    first n of what a larger case of the same size has made, references included: each band's PSF, images and float64
    references are computed once per module run, not once per case."""
    def __init__(self, nx, ny):
        self.nx, self.ny, self.a = nx, ny, {}

    def get(self, name, n, make):
        """bands [0, n) of `name`; make(b0, b1) computes the missing bands [b0, b1)"""
        have = self.a.get(name)
        k = 0 if have is None else have.shape[0]
        if k < n:
            new = np.ascontiguousarray(make(k, n))
            have = new if have is None else np.concatenate([have, new])
            have.setflags(write=False)
            self.a[name] = have
        return self.a[name][:n]

    def psf(self, b0, b1):
        out = np.stack([_rng(self.nx, self.ny, b, 0).standard_normal((2 * self.nx, 2 * self.ny), dtype=np.float32)
                        for b in range(b0, b1)]).astype(np.float64)
        out[:, self.nx, self.ny] += 5.0
        return f32_exact(out)

    def ph(self, n):
        return self.get('ph', n, lambda b0, b1: f32_exact(ofc.psfhat_from_psf(self.psf(b0, b1), nthreads=NTHREADS)))

    def noise(self, name, n):
        salt = {'x': 1, 'w': 2, 'w2': 3}[name]
        return self.get(name, n, lambda b0, b1: np.stack([_rng(self.nx, self.ny, b, salt).standard_normal(
            (self.nx, self.ny), dtype=np.float32) for b in range(b0, b1)]).astype(np.float64))

    def beam(self, n):
        return self.get('beam', n, lambda b0, b1: (0.5 + np.stack([_rng(self.nx, self.ny, b, 4).random(
            (self.nx, self.ny), dtype=np.float32) for b in range(b0, b1)])).astype(np.float32).astype(np.float64))

    def impulse(self, G, n):
        def make(b0, b1):
            x = np.zeros((b1 - b0, self.nx, self.ny))
            for b in range(b0, b1):
                i, j = impulse_position(self.nx, self.ny, G, b)
                x[b - b0, i, j] = 1.0
            return x
        return self.get(('impulse', G), n, make)

    def x(self, kind, G, n):
        return self.noise('x', n) if kind == 'noise' else self.impulse(G, n)

    def ref(self, kind, G, beam_on, n):
        def make(b0, b1):
            wsum, sigmainv = BEAM_ARGS[beam_on]
            ph, x = self.ph(b1)[b0:], self.x(kind, G, b1)[b0:]
            beam = self.beam(b1)[b0:] if beam_on else None
            return ofc.hessian_psf_cube(*ofc.make_scratch(ph, 2 * self.ny, x.shape, np.float64), beam, ph, 2 * self.ny, x,
                                        nthreads=NTHREADS, sigmainv=sigmainv, wsum=wsum if wsum > 0 else None)
        return self.get(('ref', kind, G if kind == 'impulse' else 0, beam_on), n, make)


_store = []


def store(case):
    """the store of the case's image size; one size is kept at a time (run the cases sorted by size)"""
    if not _store or (_store[0].nx, _store[0].ny) != (case.nx, case.ny):
        _store[:] = [_Store(case.nx, case.ny)]
    return _store[0]


def make_psf(case, ncu):
    """(nband, 2 nx, 2 ny): noise with a raised centre, exact in float32"""
    return store(case).psf(0, case.nband(ncu))


def inputs(case, kind, ncu):
    """{ph, x, w, w2, beam}: the spectrum of the PSF by the oracle (rounded to complex64: what the plan is given), the
    image of `kind` and the operands the case's variants read, all float64 holding float32 values."""
    st, n = store(case), case.nband(ncu)
    out = dict(ph=st.ph(n), x=st.x(kind, impulse_tile(case, ncu), n))
    for name in case.operands():
        out[name] = st.beam(n) if name == 'beam' else st.noise(name, n)
    return out


def reference(case, kind, beam_on, ncu):
    """out = [beam] conv([beam] x) [/ wsum] + sigmainv x by oracle.fftconv.hessian_psf_cube, float64"""
    return store(case).ref(kind, impulse_tile(case, ncu), beam_on, case.nband(ncu))


def impulse_answer(case, ncu, beam_on):
    """The same by hand: an impulse at (i0, j0) of band b reads the PSF around its centre,
    conv[b, i, j] = psf[b, nx + i - i0, ny + j - j0] (oracle.fftconv.direct_circular_convolution)."""
    v = inputs(case, 'impulse', ncu)
    psf = np.fft.irfft2(v['ph'], s=(2 * case.nx, 2 * case.ny))          # of the ROUNDED spectrum, origin at index 0
    wsum, sigmainv = BEAM_ARGS[beam_on]
    out = np.empty(v['x'].shape)
    ii, jj = np.arange(case.nx)[:, None], np.arange(case.ny)[None, :]
    for b, (i0, j0) in enumerate(impulse_positions(case, ncu)):
        y = psf[b, (ii - i0) % (2 * case.nx), (jj - j0) % (2 * case.ny)]
        if beam_on:
            y = y * v['beam'][b, i0, j0] * v['beam'][b]
        out[b] = y / (wsum if wsum > 0 else 1.0) + sigmainv * v['x'][b]
    return out
