"""
The psi / psi^H kernels of csrc/wavelet.hip (k_dwt_l1_fused, k_dwt_batched, k_idwt_batched2, k_idwt_finest_fused2,
k_transpose) at every tile, level and alignment edge, against the CPU oracle in float64.

tests/psi_cases.py holds the cases and the property each exists for; tests/test_cpu_psi_cases.py proves on the CPU that
every case has its property and that the references are sound.  Groups: (a) tile remainders C % TA in {0, 1, TA - 1},
(b) images smaller than a tile, (c) nlevel == dwt_max_level down to levels of 1, 2 and 4 coefficients, (d) batched grids
larger than one basis needs (the early exits of the level kernels), (e) the AL = true / false staging of coarse inputs
and the vector / scalar stores, (f) launch grids below, at and past a multiple of 64 workgroups (xcd_tile), (g) odd image
sizes, (h) dictionaries of 'self' alone, 'self' twice, one wavelet twice, a single basis, FMAX = 18 around 'self'.

Every case, in float32 and float64:
  1. psi.dot into an array of 7.25: cells the oracle never writes keep 7.25 exactly, the others match the oracle;
  2. psi.hdot of coefficients that are random EVERYWHERE (margin cells hold noise that must not leak) into an array of NaN:
     no NaN left, the image matches the oracle;
  3. float64: |<dot x, c>_written - <x, hdot c>| <= 1e-12 |dot x| |c| with c zeroed outside the written cells, which does
     not involve the oracle;
  4. a one-band plan run on one band gives, bit for bit, that band of the multi-band results;
  5. groups (a) and (e): the same calls with image pointers one element past a 16-byte boundary (level 0 of psi.dot staged
     by the AL = false branch in float64 too, the image of psi.hdot stored by the scalar branch) give the same bits: only
     the loads and stores differ between the branches, not the arithmetic.
Tolerances are those of tests/test_gpu_psi_pd.py, relative to max |reference|: 1e-12 (float64), 2e-5 (float32), for the
deepest cases too.

Odd sizes: the reference is the oracle on the image zero-padded to even sizes (psi_cases.oracle_dot / oracle_hdot); the
'self' plane is written on [0:ny, 0:nx] only, the image of hdot is the oracle's cropped.  A level count beyond
dwt_max_level is refused with ValueError, by Psi as by the oracle; the three such cases of the table are pinned as
refusals.

Not reachable, hence not tested: the plain (non-register-blocked) tail of dwt_tile below its `if constexpr`.  With the
shipped TA (32 / 16) every filter length satisfies (2 TA + F - 2) / 2 <= 64, so both number formats always take
dwt_tile_fast.
"""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from oracle import daubechies as odb        # noqa: E402  (checker only)
from oracle import wavelets as owv          # noqa: E402

import psi_cases as pc                      # noqa: E402

pmp = pytest.mark.parametrize
TOL = {pc.F32: 2e-5, pc.F64: 1e-12}
TDT = {pc.F32: torch.float32, pc.F64: torch.float64}
SENTINEL = 7.25


@pytest.fixture(scope='module')
def amd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from pfb_clean_amd.operators.psi import Psi
    from pfb_clean_amd import wavelets

    class NS:
        pass
    ns = NS()
    ns.Psi, ns.wavelets = Psi, wavelets
    return ns


def maxerr(a, b):
    return np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max()


def one_past(t, fill=None):
    """A contiguous device tensor with t's shape, dtype and values (`fill` instead, when given) that starts one element
    into a larger buffer, so that its pointer is not 16-byte aligned."""
    v = torch.empty(t.numel() + 1, dtype=t.dtype, device='cuda')[1:].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    if fill is None:
        v.copy_(t)
    else:
        v.fill_(fill)
    return v


def run_dot(psi, xd, shape):
    alpha = torch.full(shape, SENTINEL, dtype=xd.dtype, device='cuda')
    assert psi.dot(xd, alpha) is alpha
    return alpha


def run_hdot(psi, cd, shape):
    xo = torch.full(shape, float('nan'), dtype=cd.dtype, device='cuda')
    assert psi.hdot(cd, xo) is xo
    return xo


@pmp('dtype', pc.DTYPES)
@pmp('case', pc.RUN_CASES, ids=[c.id for c in pc.RUN_CASES])
def test_psi_edge_case(amd, case, dtype):
    x, a_ref, c, xo_ref = pc.reference(case)
    tol, tdt = TOL[dtype], TDT[dtype]
    written = ~np.isnan(a_ref)
    a_scale, x_scale = np.abs(a_ref[written]).max(), np.abs(xo_ref).max()
    bases = list(case.bases)
    psi = amd.Psi(case.nband, case.nx, case.ny, bases, case.nlevel, 1, dtype=tdt)
    assert (psi.Nymax, psi.Nxmax) == case.plane() == a_ref.shape[2:]
    xd = torch.tensor(x, dtype=tdt).cuda()                       # exact in float32: both formats see the same values
    cd = torch.tensor(c, dtype=tdt).cuda()
    # 1. dot
    alpha = run_dot(psi, xd, a_ref.shape)
    a = alpha.cpu().numpy()
    untouched = bool(np.all(a[~written] == SENTINEL))
    ea = maxerr(a[written], a_ref[written]) / a_scale
    # 2. hdot
    xo = run_hdot(psi, cd, xo_ref.shape).cpu().numpy()
    nan_left = int(np.isnan(xo).sum())
    ex = maxerr(xo, xo_ref) / x_scale if not nan_left else np.inf
    print(f"psi edges {case.id} {dtype}: dot {ea:.2e} hdot {ex:.2e} (tol {tol:.0e})")
    assert untouched, "psi.dot wrote a cell the oracle never writes"
    assert not np.isnan(a).any() and ea < tol
    assert nan_left == 0, "psi.hdot left pixels unwritten"
    assert ex < tol
    # 3. adjointness, float64
    if dtype == pc.F64:
        wd = torch.tensor(written).cuda()
        cw = torch.where(wd, cd, torch.zeros_like(cd))
        y = run_hdot(psi, cw, xo_ref.shape)
        aw = torch.where(wd, alpha, torch.zeros_like(alpha))
        lhs, rhs = torch.sum(aw * cw).item(), torch.sum(xd * y).item()
        bound = 1e-12 * torch.linalg.vector_norm(aw).item() * torch.linalg.vector_norm(cw).item()
        print(f"psi edges {case.id} adjoint: |lhs - rhs| {abs(lhs - rhs):.2e} bound {bound:.2e}")
        assert abs(lhs - rhs) <= bound
    # 4. one band alone, bit for bit
    b = case.nband - 1
    one = amd.Psi(1, case.nx, case.ny, bases, case.nlevel, 1, dtype=tdt)
    a1 = run_dot(one, xd[b:b + 1].clone(), (1,) + a_ref.shape[1:]).cpu().numpy()
    assert np.array_equal(a1[0], a[b])
    x1 = run_hdot(one, cd[b:b + 1].clone(), (1,) + xo_ref.shape[1:]).cpu().numpy()
    assert np.array_equal(x1[0], xo[b])
    one.close()
    # 5. unaligned image pointers, bit for bit
    if case.group in 'ae':
        a5 = run_dot(psi, one_past(xd), a_ref.shape).cpu().numpy()
        assert np.array_equal(a5, a)
        xo5 = one_past(xd, fill=float('nan'))
        assert psi.hdot(cd, xo5) is xo5
        assert np.array_equal(xo5.cpu().numpy(), xo)
    psi.close()


@pmp('case', pc.REFUSED_CASES, ids=[c.id for c in pc.REFUSED_CASES])
def test_level_count_beyond_dwt_max_level_is_refused(amd, case):
    """db5 at 2 levels needs 36 pixels: (33, 64), (64, 33) and (31, 45) are refused like the same request at the next
    even size, as the reference (psi.py:44-46) and the oracle refuse it."""
    assert any(case.nlevel > odb.dwt_max_level(min(case.nx, case.ny) + 1, w) for w in case.wavelets)
    with pytest.raises(ValueError):
        amd.Psi(case.nband, case.nx, case.ny, list(case.bases), case.nlevel, 1)
    with pytest.raises(ValueError):
        owv.Psi(case.nband, case.nx + case.nx % 2, case.ny + case.ny % 2, list(case.bases), case.nlevel, 1)


@pmp('dtype', pc.DTYPES)
@pmp('cid', pc.STANDALONE)
def test_standalone_dwt2d_idwt2d_edge_case(amd, cid, dtype):
    """pfb_clean_amd.wavelets.dwt2d / idwt2d with the reference's argument lists (as
    test_standalone_dwt2d_idwt2d_with_the_reference_argument_lists calls them) on band 0 of one tiny, one deepest and one
    tile-remainder case: the same checks as above, on device tensors."""
    case = pc.by_id(cid)
    wv = amd.wavelets
    x, a_ref, c, _ = pc.reference(case)
    tol, tdt = TOL[dtype], TDT[dtype]
    nx, ny, nlevel = case.nx, case.ny, case.nlevel
    dec_lo, dec_hi, rec_lo, rec_hi = wv.filter_bank(case.bases[0])
    sx, sy, spx, spy, ix, iy, ntx, nty = wv.level_sizes(nx, ny, dec_lo.size, nlevel)
    bk = case.bk(case.bases[0])
    assert (nty, ntx) == case.plane() and list(sx) == bk.sx and list(spy) == bk.spy and ix == bk.ix and iy == bk.iy
    a0, c0 = a_ref[0, 0], c[0, 0]
    written = ~np.isnan(a0)
    xo_ref = np.zeros((nx, ny))
    owv.idwt2d(c0, xo_ref, bk, *odb.filter_bank(case.bases[0])[2:])
    xd, cd = torch.tensor(x[0], dtype=tdt).cuda(), torch.tensor(c0, dtype=tdt).cuda()
    alpha = torch.full((nty, ntx), SENTINEL, dtype=tdt, device='cuda')
    assert wv.dwt2d(xd, alpha, None, None, ix, iy, sx, sy, dec_lo, dec_hi, nlevel) is alpha
    a = alpha.cpu().numpy()
    assert np.all(a[~written] == SENTINEL)
    ea = maxerr(a[written], a0[written]) / np.abs(a0[written]).max()
    xo = torch.full((nx, ny), float('nan'), dtype=tdt, device='cuda')
    before = cd.clone()
    assert wv.idwt2d(cd, xo, None, None, None, ix, iy, sx, sy, spx, spy, rec_lo, rec_hi, nlevel) is xo
    assert torch.equal(cd, before)
    xh = xo.cpu().numpy()
    assert not np.isnan(xh).any()
    ex = maxerr(xh, xo_ref) / np.abs(xo_ref).max()
    print(f"standalone {cid} {dtype}: dwt2d {ea:.2e} idwt2d {ex:.2e}")
    assert ea < tol and ex < tol
    if dtype == pc.F64:
        wd = torch.tensor(written).cuda()
        cw = torch.where(wd, cd, torch.zeros_like(cd))
        y = torch.full((nx, ny), float('nan'), dtype=tdt, device='cuda')
        wv.idwt2d(cw, y, None, None, None, ix, iy, sx, sy, spx, spy, rec_lo, rec_hi, nlevel)
        aw = torch.where(wd, alpha, torch.zeros_like(alpha))
        lhs, rhs = torch.sum(aw * cw).item(), torch.sum(xd * y).item()
        assert abs(lhs - rhs) <= 1e-12 * torch.linalg.vector_norm(aw).item() * torch.linalg.vector_norm(cw).item()
