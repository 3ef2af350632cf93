"""
The case table of tests/test_gpu_pow2_edges.py (tests/pow2_cases.py), checked on the CPU:

  * the mirror of the launch bookkeeping reproduces the constants of csrc/fftconv_pow2.hip and the grids its comments
    quote.  The constants are the tables COL, ROW and FWDP_LDS below, and test_tables_are_the_source_constants ties them
    to the .hip file: it writes a translation unit that includes the file and holds one static_assert per table entry
    against the source's own constexprs, and has hipcc check it (host side, syntax only).  A change of a tile, of
    elements per thread or of an LDS size there fails that test until table and mirror follow;
  * every case has the property it exists for at 256 CUs and at 304: the band-count rule follows the CU count;
  * the coverage matrices built from the table have no empty cell:
      columns      {persistent, two-level} x {fp32, fp64} x {single trip, second trip, inactive slot, band crossing, band
                   sub-range with band0 > 0 in more than one trip}
      forward rows {persistent kernel, with and without beam} x {pairing on, off} x {fewer tiles than workgroups, full trip,
                   tail, three trips}
      inverse rows {persistent kernel by mode and per-band form} x {pairing on, off} x {fewer tiles than workgroups, full trip, tail,
                   three trips}, every (mode, beam, per-band) instantiation with pairing on and off, the plain kernel of
                   every class by dot variant
    and every instantiation ColKernels::serving, RowFwdK::reachable and RowInvK::reachable enumerate is launched by a case;
  * the device footprint of every case at 256 CUs (x, out, operands, T, psf_l, partials);
  * the references equal the oracle's on both inputs, and the impulse references equal the PSF read by hand.

Footprints.  128 MB hold every case of the class sweep and the producer but the six largest classes listed in
OVER_128MB: two bands of an 8192-point fp64 column class take 135 MB in T, psf_l, x and out alone.  No trip case of the
row kernels fits 128 MB: the persistent row grids are one workgroup per CU, a 64-row band of the shortest persistent
class (1024-point rows) is 8 tiles and 5 MB in T, psf_l, x and out, so that even one full trip of 256 tiles is 166 MB.
These cases, the column trips and the non-temporal cases (200 MiB of PSF by definition) are held to 512 MB, the three-trip
row cases (more than two tiles per CU: 513 tiles and more) to 768 MB; the largest is 693 MB.  Every case is run.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import fftconv as ofc

import pow2_cases as pc

pmp = pytest.mark.parametrize
F32, F64 = pc.F32, pc.F64
CUS = (256, 304)
ids = [c.id for c in pc.CASES]

# the source's constexprs (test_tables_are_the_source_constants):
# (format, H) -> ColCfg::E1, KIND, DB and shape(): gc, threads, lds, wg_per_cu
COL = {(F32, 64): (4, 'plain', False, 16, 256, 20480, 0), (F32, 96): (12, 'plain', False, 32, 256, 59392, 0),
       (F32, 128): (4, 'plain', False, 8, 256, 20480, 0), (F32, 256): (4, 'plain', False, 4, 256, 20480, 0),
       (F32, 512): (4, 'plain', False, 2, 256, 20480, 0), (F32, 1024): (4, 'plain', False, 1, 256, 20480, 0),
       (F32, 2048): (8, 'persistent', False, 1, 256, 41536, 2), (F32, 4096): (8, 'persistent', True, 1, 512, 152128, 1),
       (F32, 8192): (8, 'twolevel', False, 1, 512, 148032, 1),
       (F64, 64): (4, 'plain', False, 16, 256, 20480, 0), (F64, 96): (12, 'plain', False, 32, 256, 59392, 0),
       (F64, 128): (4, 'plain', False, 8, 256, 20480, 0), (F64, 256): (4, 'plain', False, 4, 256, 20480, 0),
       (F64, 512): (4, 'plain', False, 2, 256, 20480, 0), (F64, 1024): (4, 'plain', False, 1, 256, 20480, 0),
       (F64, 2048): (8, 'persistent', False, 1, 256, 46208, 2), (F64, 4096): (8, 'persistent', True, 1, 512, 156800, 1),
       (F64, 8192): (16, 'twolevel', False, 1, 512, 156800, 1)}
# (format, L) -> RowFwdK: PERSISTENT, E, rows per tile | RowInvK: PERSISTENT, PER_BAND, E, EP, rows per tile of the plain and
# of the persistent kernel (InvP::G: meaningful where PERSISTENT), InvP::LDS
ROW = {(F32, 64): ((False, 8, 32), (False, False, 8, 8, 32, 128, 144320)),
       (F32, 128): ((False, 8, 16), (False, False, 8, 8, 16, 64, 143296)),
       (F32, 256): ((False, 8, 8), (False, False, 8, 8, 8, 32, 143296)),
       (F32, 512): ((False, 8, 8), (False, False, 8, 8, 4, 16, 144832)),
       (F32, 1024): ((False, 16, 8), (True, True, 8, 8, 4, 8, 152768)),
       (F32, 2048): ((True, 16, 8), (True, True, 8, 8, 4, 4, 160832)),
       (F32, 4096): ((True, 16, 4), (True, False, 16, 16, 4, 4, 144000)),
       (F32, 8192): ((False, 16, 2), (False, False, 8, 8, 1, 1, 242656)),
       (F64, 64): ((False, 8, 32), (False, False, 8, 8, 32, 64, 79360)),
       (F64, 128): ((False, 8, 16), (False, False, 8, 8, 16, 32, 79360)),
       (F64, 256): ((False, 8, 8), (False, False, 8, 8, 8, 16, 80384)),
       (F64, 512): ((False, 8, 8), (False, False, 8, 8, 4, 8, 83968)),
       (F64, 1024): ((False, 8, 8), (True, True, 8, 8, 4, 4, 100096)),
       (F64, 2048): ((False, 8, 4), (True, True, 8, 8, 4, 2, 116352)),
       (F64, 4096): ((False, 8, 2), (True, True, 8, 16, 2, 2, 156416))}
FWDP_LDS = {(F32, 2048): 158080, (F32, 4096): 145664}

OVER_128MB = {'a-col8192-f64', 'e-col4096-f64', 'e-col8192-f32', 'e-col8192-f64', 'e-row8192-f32', 'e-row4096-f64'}


# ------------------------------------------------------------------------------------------------- the mirror
def test_mirror_reproduces_the_source_constants():
    for (d, H), want in COL.items():
        c = pc.ColCfg(d, H)
        assert (c.E1, c.KIND, c.DB, c.gc, c.threads, c.lds, c.wg_per_cu) == want, (d, H)
        assert c.KIND == pc.COL_KIND[H] and c.lds <= pc.LDS_MAX
    for (d, L), (fw, iw) in ROW.items():
        f, i = pc.RowFwd(d, L), pc.RowInv(d, L)
        assert (f.PERSISTENT, f.E, f.G) == fw, (d, L)
        assert (i.PERSISTENT, i.PER_BAND, i.E, i.EP, i.G_plain, i.ip.G, i.ip.LDS) == iw, (d, L)
        assert f.PERSISTENT == ((d, L) in pc.FWD_PERSISTENT) and i.PERSISTENT == ((d, L) in pc.INV_PERSISTENT)
        assert i.PER_BAND == ((d, L) in pc.INV_PER_BAND)
        assert pc.ROW_TILE_MAX % f.G == 0 and pc.ROW_TILE_MAX % i.G_plain == 0
        if f.PERSISTENT:
            assert pc.FwdP(d, L).LDS == FWDP_LDS[(d, L)]
    assert set(ROW) == {(d, L) for d in pc.DTYPES for L in pc.row_lengths(d)}
    assert pc.fast_nblocks(64, 2) == 65 and pc.fast_nblocks(64, 1) == 129 and pc.fast_nblocks(2048, 2) == 2049


def test_tables_are_the_source_constants(tmp_path):
    """COL, ROW and FWDP_LDS against csrc/fftconv_pow2.hip itself: one static_assert per entry, compiled on the host side."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc: the tables cannot be compiled against csrc/fftconv_pow2.hip')
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'pfb_clean_amd', 'csrc')
    ty = {F32: 'float', F64: 'double'}
    kind = {'plain': 'Plain', 'persistent': 'Persistent', 'twolevel': 'TwoLevel'}
    b = {False: 'false', True: 'true'}
    tu = ['#define PFB_POW2_PART 1', '#include "fftconv_pow2.hip"', 'namespace pfb {',
          'template <typename T, int L, bool INVK> constexpr int plain_rows() {',
          '    return row_groups<T, L, RowCfg<T, L, INVK>::E, RowCfg<T, L, INVK>::GMAX>(); }',
          'template <typename T, int L> constexpr int fwd_rows() {',
          '    if constexpr (RowFwdK<T, L>::PERSISTENT) return FwdP<T, L>::G; else return plain_rows<T, L, false>(); }']
    for (d, H), (e1, k, db, gc, nt, lds, wg) in COL.items():
        c = f'ColCfg<{ty[d]}, {H}>'
        tu.append(f'static_assert({c}::E1 == {e1} && {c}::KIND == ColKind::{kind[k]} && {c}::DB == {b[db]} && '
                  f'{c}::shape().gc == {gc} && {c}::shape().threads == {nt} && {c}::shape().lds == {lds} && '
                  f'{c}::shape().wg_per_cu == {wg}, "COL {d} {H}");')
    for (d, L), ((fp, fe, fg), (ip, ipb, ie, iep, ig, ipg, ilds)) in ROW.items():
        a, f, i = f'{ty[d]}, {L}', f'RowFwdK<{ty[d]}, {L}>', f'RowInvK<{ty[d]}, {L}>'
        tu.append(f'static_assert({f}::PERSISTENT == {b[fp]} && {f}::E == {fe} && fwd_rows<{a}>() == {fg}, "ROW fwd {d} {L}");')
        tu.append(f'static_assert({i}::PERSISTENT == {b[ip]} && {i}::PER_BAND == {b[ipb]} && {i}::E == {ie} && {i}::EP == {iep} && '
                  f'plain_rows<{a}, true>() == {ig} && {i}::IP::G == {ipg} && {i}::IP::LDS == {ilds}, "ROW inv {d} {L}");')
    for (d, L), lds in FWDP_LDS.items():
        tu.append(f'static_assert(FwdP<{ty[d]}, {L}>::OK && FwdP<{ty[d]}, {L}>::LDS == {lds}, "FWDP_LDS {d} {L}");')
    src = tmp_path / 'pow2_tables.hip'
    src.write_text('\n'.join(tu + ['}', '']))
    r = subprocess.run([hipcc, '-std=c++17', '--offload-arch=gfx950', '--offload-host-only', '-fsyntax-only', '-I', csrc, str(src)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]


def test_mirror_reproduces_the_grids_the_source_quotes():
    """balanced_grid's comment: 253 instead of 256 workgroups at 8 x 4096^2 fp32, 342 instead of 512 at 1 x 2048^2, 228 at
    1 x 4096^2; the two-level kernel keeps the full grid."""
    assert pc.ColLaunch(F32, 4096, 4096, 0, 8, 256).grid == 253
    assert pc.ColLaunch(F32, 2048, 2048, 0, 1, 256).grid == 342
    assert pc.ColLaunch(F32, 4096, 4096, 0, 1, 256).grid == 228
    assert pc.ColLaunch(F32, 8192, 8192, 0, 2, 256).grid == 256
    assert pc.balanced_grid(256, 256) == 256 and pc.balanced_grid(257, 256) == 129 and pc.balanced_grid(7, 256) == 7
    # the examples of the issue this table answers: (2048, 256) with 2 bands is 258 items on up to 512 workgroups,
    # (8192, 128) is 130 items on 256: one trip each
    c = pc.ColLaunch(F32, 2048, 256, 0, 2, 256)
    assert (c.nitems, c.maxgrid, c.trips) == (258, 512, 1)
    c = pc.ColLaunch(F32, 8192, 128, 0, 2, 256)
    assert (c.nitems, c.maxgrid, c.trips) == (130, 256, 1)
    # the non-temporal threshold: 268 MB per 4096^2 fp32 band
    assert pc.psf_nt(F32, 4096, 4096, 1) and not pc.psf_nt(F32, 2048, 2048, 2) and pc.psf_nt(F32, 2048, 2048, 4)
    assert pc.CSZ[F32] * pc.psf_elems_per_band(F32, 4096, 4096) == 8 * 2049 * 8192 * 2


def test_tile_maps_by_hand():
    # descending bands: 2 bands of 129 blocks on 129 workgroups, band0 = 3: trip 0 in band 4, trip 1 in band 3
    c = pc.ColLaunch(F64, 4096, 128, 3, 2, 256)
    assert (c.grid, c.trips, c.inactive) == (129, 2, 0) and c.bands_of(0) == [4, 3] and c.bands_of(128) == [4, 3]
    c = pc.ColLaunch(F64, 4096, 128, 0, 3, 256)
    assert (c.grid, c.trips, c.inactive) == (194, 2, 1) and c.bands_of(193) == [1, None] and c.bands_of(100) == [2, 0]
    # the rotated map: 10 tiles on 4 workgroups.  Trip 1 takes (b + 3) mod 4 + 4, trip 2 (b + 6) mod 4 + 8
    assert [pc.inv_tiles(4, 10, b) for b in range(4)] == [[0, 7], [1, 4], [2, 5, 8], [3, 6, 9]]
    assert pc.inv_tiles(8, 5, 6) == [] and pc.inv_tiles(5, 5, 4) == [4]
    # the pairing: 16 tiles of 4 rows (SH = 2): tiles b and b + 8 take the two halves of an 8-row line
    assert [pc.tile_row(r, 16, 2, 4) for r in (0, 8, 1, 9, 7, 15)] == [0, 4, 8, 12, 56, 60]
    assert sorted(pc.tile_row(r, 32, 4, 2) for r in range(32)) == list(range(0, 64, 2))
    assert [pc.tile_row(r, 24, 2, 4) for r in (0, 8, 23)] == [0, 32, 92] and not pc.pairing(2, 24) and not pc.pairing(1, 16)


# ------------------------------------------------------------------------------------------------- the table
def test_table_is_well_formed():
    assert len(set(ids)) == len(ids)
    assert {c.group for c in pc.CASES} == set('abcde')
    for c in pc.CASES:
        assert c.target in ('sweep', 'col', 'fwd', 'inv', 'producer') and c.dtype in pc.DTYPES, c
        assert pc.pow2_supported(c.dtype, c.nx, c.ny), c
        assert c.nx in (64, 96) or c.ny == 128, "the partner axis is the smallest"
        assert all(call in pc.CALLS and beam in (False, True) for call, beam in c.variants) and c.variants, c
        for ncu in CUS:
            assert 1 <= c.nband(ncu) <= 80, c
    assert pc.RUN_CASES == pc.CASES, "every case is run"


@pmp('ncu', CUS)
@pmp('case', pc.CASES, ids=ids)
def test_case_has_its_property(case, ncu):
    assert case.holds(ncu), (case, ncu, case.nband(ncu))


def test_band_counts_follow_the_cu_count():
    moved = [c.id for c in pc.CASES if c.group in 'bc' and c.nband(256) != c.nband(304)]
    assert len(moved) >= 40, moved
    for c in pc.CASES:
        if c.group == 'd':                  # the threshold is in bytes: the same band count whatever the chip
            assert c.nband(256) == c.nband(304)


def test_footprints():
    for c in pc.RUN_CASES:
        fp = c.footprint(256)
        three = c.group == 'c' and '-three' in c.name
        assert c.cap() == (pc.CAP_BYTES_THREE if three else pc.CAP_BYTES_BIG) and fp <= c.cap(), (c, fp)
        if c.group in 'ae':
            assert (fp > pc.CAP_BYTES) == (c.id in OVER_128MB), (c, fp)
    assert (pc.CAP_BYTES, pc.CAP_BYTES_BIG, pc.CAP_BYTES_THREE) == (128e6, 512e6, 768e6)
    # group c cannot be smaller: one full trip of the shortest persistent row class, without any operand
    c = pc.by_id('c-inv1024-nx64-full-f32')
    bare = (pc.CSZ[F32] * (pc.T_elems_per_band(F32, 64, 2048) + pc.psf_elems_per_band(F32, 64, 2048)) + 2 * 4 * 64 * 2048) * c.nband(256)
    assert c.nband(256) == 32 and bare > pc.CAP_BYTES


# ------------------------------------------------------------------------------------------------- coverage matrices
def _col_cells(ncu=256):
    cells = {}
    for c in pc.RUN_CASES:
        if c.target == 'producer':
            continue
        for band0, nb in c.ranges(ncu):
            k = c.col(ncu, (band0, nb))
            if k.kind == 'plain':
                cells.setdefault(('plain', c.dtype, c.nx, 'single'), c.id)
                continue
            feats = ['single'] if k.trips == 1 else ['second-trip']
            if k.inactive:
                feats.append('inactive')
            if k.crosses_band():
                feats.append('band-crossing')
            if band0 > 0 and k.trips >= 2:
                feats.append('sub-range')
            if k.kind == 'persistent' and k.trips >= 2 and k.grid < k.maxgrid:
                feats.append('balanced-below-cap' + ('-inactive' if k.inactive else '-full'))
            for f in feats:
                cells.setdefault((k.kind, c.dtype, c.nx, f, k.nt), c.id)
    return cells


def test_column_matrix_is_complete():
    cells = _col_cells()
    for d in pc.DTYPES:
        for H in pc.POW2[:5]:
            assert ('plain', d, H, 'single') in cells
        for H in pc.TRIP_COLS:
            kind = pc.COL_KIND[H]
            feats = ['single', 'second-trip', 'inactive', 'band-crossing', 'sub-range']
            if kind == 'persistent':
                feats += ['balanced-below-cap-full', 'balanced-below-cap-inactive']
            for f in feats:
                assert (kind, d, H, f, False) in cells, (kind, d, H, f)
            assert (kind, d, H, 'second-trip', True) in cells, "the non-temporal instantiation"


def _row_edge_of(ntiles, cap, tpb, walks):
    n = max(len(w) for w in walks)
    if ntiles < cap and ntiles + tpb <= cap:
        return 'part'
    if ntiles <= cap:
        return 'full'
    return {2: 'tail', 3: 'three'}.get(n, 'more') if ntiles % cap else 'even'


def _fwd_cells(ncu=256):
    cells = {}
    for c in pc.RUN_CASES:
        if c.target == 'producer':
            continue
        for rng in c.ranges(ncu):
            k = c.fwd(ncu, rng)
            for _, beam in c.variants:
                if not k.PERSISTENT:
                    cells.setdefault((k.kernel(beam), k.pairing), c.id)
                    continue
                edge = _row_edge_of(k.ntiles, k.cap, k.tiles_per_band, [k.tiles_of(b) for b in range(k.grid)])
                cells.setdefault((k.kernel(beam), k.pairing, edge), c.id)
    return cells


def test_forward_row_matrix_is_complete():
    cells = _fwd_cells()
    for d, L in sorted(pc.FWD_PERSISTENT):
        sh = pc.RowFwd(d, L).SH
        for beam in (False, True):
            for pair in ((True, False) if sh > 1 else (False,)):
                for edge in ('part', 'full', 'tail', 'three'):
                    assert (('fwdq', d, L, beam), pair, edge) in cells, (d, L, beam, pair, edge)
    # the plain kernel of every other class
    for d in pc.DTYPES:
        for L in pc.row_lengths(d):
            if (d, L) not in pc.FWD_PERSISTENT:
                assert any(k[0] == ('fwd', d, L) for k in cells), (d, L)


def _inv_cells(ncu=256):
    cells = {}
    for c in pc.RUN_CASES:
        if c.target == 'producer':
            continue
        for rng in c.ranges(ncu):
            for v in c.variants:
                for kern, grid, nbl, tpb in c.inv_launches(ncu, v, rng):
                    if kern[0] == 'inv':
                        cells.setdefault((kern, v[0], v[1]), c.id)
                        continue
                    ntiles = tpb * nbl
                    on = pc.pairing(c.inv().SH, tpb)
                    edge = _row_edge_of(ntiles, ncu, tpb, [pc.inv_tiles(grid, ntiles, b) for b in range(grid)])
                    _, d, L, mode, beam, pb = kern
                    cells.setdefault(('edge', d, L, mode, pb, on, edge), c.id)
                    cells.setdefault(('inst', kern, on), c.id)
                    cells.setdefault(('beam', d, L, beam, edge), c.id)
                    if grid < min(ntiles, ncu):
                        cells.setdefault(('clamped', d, L, beam), c.id)
    return cells


def test_inverse_row_matrix_is_complete():
    cells = _inv_cells()
    for d, L in sorted(pc.INV_PERSISTENT):
        k = pc.RowInv(d, L)
        pairs = (True, False) if k.SH > 1 else (False,)
        edges = ['part', 'full', 'tail', 'three']
        forms = [(0, False), (1, False), (2, False)] + ([(2, True)] if k.PER_BAND else [])
        for on in pairs:
            for mode, pb in forms:
                for edge in edges:
                    if pb and edge != 'part' and on is False and k.SH == 1:
                        continue
                    # the per-band kernel's grid is cut to the partials' nx slots when a launch has all the plan's bands:
                    # its trip edges are those of that grid, see the test below
                    if pb and edge in ('full', 'tail', 'three'):
                        continue
                    assert ('edge', d, L, mode, pb, on, edge) in cells, (d, L, mode, pb, on, edge)
                for beam in (False, True):
                    assert ('inst', ('invp', d, L, mode, beam, pb), on) in cells, (d, L, mode, beam, pb, on)
        for beam in (False, True):
            for edge in edges:
                assert ('beam', d, L, beam, edge) in cells, (d, L, beam, edge)
            if k.PER_BAND:
                assert ('clamped', d, L, beam) in cells, "per-band launch with its grid cut to the partials"
    # the plain kernel with its fused sums, in EVERY class (the persistent ones included), with and without beam
    for d in pc.DTYPES:
        for L in pc.row_lengths(d):
            for call in ('dot-w', 'dot-w-w2', 'bands-w-w2'):
                for beam in (False, True):
                    assert (('inv', d, L), call, beam) in cells, (d, L, call, beam)
            if (d, L) not in pc.INV_PERSISTENT:
                for call in pc.ALL_CALLS:
                    assert (('inv', d, L), call, False) in cells and (('inv', d, L), call, True) in cells


def test_per_band_kernel_runs_many_trips_on_a_clamped_grid():
    """k_row_inv_pow2p<.., PB>: one launch over all bands with partials [3][nb][grid], grid cut to nx nband / nb.  With
    all the plan's bands that is nx workgroups whatever the chip: the larger cases run it over three trips and more, with
    band boundaries in every workgroup's walk."""
    seen = set()
    for c in pc.run_params('c'):
        if c.target != 'inv' or not c.inv().PER_BAND or ('bands-x-w', c.variants[0][1]) not in c.variants:
            continue
        (kern, grid, nbl, tpb), = c.inv_launches(256, ('bands-x-w', c.variants[0][1]))
        assert kern[5] and grid <= c.nx * c.nband(256) // nbl
        walks = [pc.inv_tiles(grid, tpb * nbl, b) for b in range(grid)]
        assert sorted(t for w in walks for t in w) == list(range(tpb * nbl))
        if max(len(w) for w in walks) >= 3 and any(len({t // tpb for t in w}) >= 3 for w in walks):
            seen.add((c.dtype, c.L, c.nx))
    for d, L in pc.INV_PER_BAND:
        assert (d, L, 64) in seen and (d, L, 96) in seen, (d, L)


def test_every_reachable_instantiation_is_launched():
    launched = set()
    for c in pc.RUN_CASES:
        launched |= c.kernels(256)
    want = set()
    for d in pc.DTYPES:
        for H in pc.POW2:                                       # ColKernels::serving, and the plain kernel where KIND is Plain
            kind = pc.COL_KIND[H]
            want |= ({('col', d, H)} if kind == 'plain' else
                     {('colp' if kind == 'persistent' else 'colx', d, H, nt) for nt in (False, True)})
        want.add(('col', d, 96))
        for L in pc.row_lengths(d):
            want |= pc.RowFwd(d, L).reachable() | pc.RowInv(d, L).reachable()
    assert not want - launched, sorted(want - launched, key=str)
    assert len(want) == 2 * (6 + 6 + 1) + (8 + 2) + 7 + (8 + 7) + 5 * 6 + 8 + 6, "the count by hand"


# ------------------------------------------------------------------------------------------------- inputs, references
def test_impulses_sit_on_tile_edges():
    for c in pc.RUN_CASES:
        G = min(pc.tile_rows(c), c.nx)
        pos = pc.impulse_positions(c, 256)
        assert len(pos) == c.nband(256)
        rows = [i for i, _ in pos]
        assert all(i % G in (0, G - 1) and 0 <= i < c.nx for i in rows), c
        assert {j for _, j in pos} <= set(pc.IMPULSE_COLS(c.ny))
        n = min(len(pos), len(set(pc.impulse_rows(c.nx, G))))
        assert len(set(rows[:n])) == n, "a different row in each band"
        if len(pos) >= 24:
            assert {j for _, j in pos} == set(pc.IMPULSE_COLS(c.ny)) and len(set(pos)) == min(len(pos), 4 * n)
        tiles = {i // G for i in rows}
        assert 0 in tiles and (c.nx // G - 1 in tiles or len(pos) < 5)


SMALL = [c for c in pc.RUN_CASES if c.footprint(256) <= 24 * pc.MB and c.target != 'producer'] + [pc.by_id('b-col2048-balanced-full-f32')]


@pmp('case', SMALL, ids=lambda c: c.id)
def test_references_are_the_oracles(case):
    ncu = 256
    for beam in sorted({b for _, b in case.variants}):
        wsum, sigmainv = pc.BEAM_ARGS[beam]
        for kind in pc.INPUT_KINDS:
            v = pc.inputs(case, kind, ncu)
            ref = pc.reference(case, kind, beam, ncu)
            assert ref.shape == v['x'].shape == (case.nband(ncu), case.nx, case.ny)
            for name in ('ph', 'x') + tuple(case.operands()):
                assert np.array_equal(v[name], pc.f32_exact(v[name])), name
            Q = 2 * case.ny
            bx = v['x'] * v['beam'] if beam else v['x']
            want = ofc.psf_convolve_cube(*ofc.make_scratch(v['ph'], Q, bx.shape, np.float64), v['ph'], Q, bx).copy()
            if beam:
                want *= v['beam']
            want = want / (wsum if wsum > 0 else 1.0) + sigmainv * v['x']
            assert np.abs(ref - want).max() <= 1e-12 * np.abs(want).max(), (kind, beam)
            if kind == 'impulse':
                hand = pc.impulse_answer(case, ncu, beam)
                assert np.abs(ref - hand).max() <= 1e-12 * np.abs(hand).max(), beam
                assert v['x'].sum() == case.nband(ncu) and np.count_nonzero(v['x']) == case.nband(ncu)


@pmp('case', [c for c in pc.RUN_CASES if c.target == 'producer' and c.footprint(256) <= 24 * pc.MB], ids=lambda c: c.id)
def test_producer_inputs(case):
    psf = pc.make_psf(case, 256)
    assert psf.shape == (2, 2 * case.nx, 2 * case.ny) and np.array_equal(psf, pc.f32_exact(psf))
    assert np.all(psf[:, case.nx, case.ny] > 1.0), "the raised centre"
    ph = ofc.psfhat_from_psf(psf)
    assert np.abs(pc.inputs(case, 'noise', 256)['ph'] - ph).max() <= 1e-6 * np.abs(ph).max()
