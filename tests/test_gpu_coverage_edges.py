"""
The coverage FFT paths at every radix, pass order and LDS boundary: the Stockham FFT in LDS (csrc/fft_generic.hpp), its
global-memory form (csrc/fft_long.hpp) and the stage entries of csrc/fftconv.hip, through the three ways they are
reached -- pfb_psfhat_from_psf ('producer'), pfb_psfhat_regrid ('regrid') and the apply entries on a coverage plan
('apply') -- against float64 references, in float32 and float64.

tests/coverage_cases.py holds the cases and the property each exists for; tests/test_cpu_coverage_cases.py proves on the
CPU that every case has its property, that the table covers {radix} x {LDS, global} x {rows, columns} x {forward,
inverse} x {format} x {first, later pass}, and that the references agree with the oracle.

Every case runs on seeded white noise and on a unit impulse (see the *_input functions of coverage_cases).  Every output
lives inside a larger tensor: 64 elements of 7.25 on either side, NaN inside.  After the call the inside is finite (no
element left unwritten), the margins are untouched and the inputs equal their copies bit for bit.

Tolerances, relative to max |reference| (the impulse spectra have |reference| = 1: absolute):
  spectra       1e-12 (float64), 2e-6 (float32)      as test_native_psfhat_producer
  convolutions  1e-12 (float64), 1e-5 (float32)      TOL_CONV of the convolution tests
  inner products of the kernel's own output, |got - sum| <= TOL_DOT * (|w| |out|, |w2| |out|, |out|^2) with TOL_DOT =
                1e-12 (float64), 1e-9 (float32)      as test_gpu_pcg_bands.py: the sums are fp64 whatever the format
  inner products against those of the oracle's output: the same plus what the convolution's own bound allows, by
                Cauchy-Schwarz |<w, out - ref>| <= |w| d and | |out|^2 - |ref|^2 | <= (2 |ref| + d) d with
                d = sqrt(N) TOL_CONV max |ref| (N values in the band range).

`apply`: a plan of pfb_psfconv_plan_create with PFB_FORCE_GENERIC set, so that no size takes the power-of-two kernels.
Per input the variants of VARIANTS (beam, wsum, sigmainv, dot_with = x or an independent w, dot_with2, the three entry
points); on three-band plans the band ranges (1, 1) and (1, 2), bit-equal to those bands of the whole launch; and the call
without inner products bit-equal to the same call with them (k_long_finish runs one workgroup a row only where a row's
sums are wanted; the samples do not depend on the launch grid).
"""
import ctypes
import time

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import coverage_cases as cc                 # noqa: E402

pmp = pytest.mark.parametrize
F32, F64 = cc.F32, cc.F64
TOL_SPEC = {F32: 2e-6, F64: 1e-12}
TOL_CONV = {F32: 1e-5, F64: 1e-12}
TOL_DOT = {F32: 1e-9, F64: 1e-12}
RDT = {F32: torch.float32, F64: torch.float64}
CDT = {F32: torch.complex64, F64: torch.complex128}
MARGIN = 64
SENTINEL = 7.25


@pytest.fixture(scope='module')
def amd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from pfb_clean_amd import _lib, _dev

    class NS:
        pass
    ns = NS()
    ns.lib, ns._lib, ns.dev = _lib.load(), _lib, _dev
    return ns


@pytest.fixture(scope='module')
def log():
    """Worst error per (what, group, format) and the wall time per test; printed when the module is done."""
    rec = {'worst': {}, 'times': {}, 't0': time.perf_counter()}
    yield rec
    print("\ncoverage edges: worst error relative to its tolerance's scale, per check, group and format")
    for key in sorted(rec['worst']):
        err, cid = rec['worst'][key]
        print(f"  {key[0]:<18} ({key[1]}) {key[2]}: {err:.3e}   [{cid}]")
    if rec['times']:
        slow = max(rec['times'], key=rec['times'].get)
        print(f"coverage edges: {len(rec['times'])} tests, module wall time {time.perf_counter() - rec['t0']:.1f} s, "
              f"slowest {slow} {rec['times'][slow]:.2f} s")


def note(log, what, case, dtype, err):
    key = (what, case.group, dtype)
    if key not in log['worst'] or err > log['worst'][key][0]:
        log['worst'][key] = (err, case.id)


def guarded(shape, tdt):
    """(whole buffer, view of `shape` inside it): the view holds NaN, the MARGIN elements on either side SENTINEL."""
    n = int(np.prod(shape))
    fill = complex(SENTINEL, -SENTINEL) if tdt.is_complex else SENTINEL
    buf = torch.full((n + 2 * MARGIN,), fill, dtype=tdt, device='cuda')
    inner = buf[MARGIN:MARGIN + n]
    inner.fill_(complex(float('nan'), float('nan')) if tdt.is_complex else float('nan'))
    return buf, inner.view(shape)


def check_guard(buf, inner, what):
    n = inner.numel()
    real = (lambda t: torch.view_as_real(t)) if buf.dtype.is_complex else (lambda t: t)
    lo, hi = real(buf[:MARGIN]), real(buf[MARGIN + n:])
    assert torch.all(lo.abs() == SENTINEL) and torch.all(hi.abs() == SENTINEL), f"{what}: wrote outside its array"
    bad = int((~torch.isfinite(real(inner))).sum())
    assert bad == 0, f"{what}: {bad} values left unwritten or not finite"


def relerr(got, ref):
    return np.abs(np.asarray(got).astype(ref.dtype) - ref).max() / np.abs(ref).max()


def ids_of(params):
    return [f"{c.id}-{d}" for c, d in params]


class Timer:
    def __init__(self, log, name):
        self.log, self.name = log, name

    def __enter__(self):
        self.t = time.perf_counter()

    def __exit__(self, *a):
        self.log['times'][self.name] = time.perf_counter() - self.t


# --------------------------------------------------------------------------------------------------------- producer
@pmp('case,dtype', cc.run_params('producer'), ids=ids_of(cc.run_params('producer')))
def test_producer(amd, log, case, dtype):
    lib, _dev = amd.lib, amd.dev
    P, Q = case.dims
    with Timer(log, f"producer {case.id} {dtype}"):
        for kind in cc.INPUT_KINDS:
            psf, ref = cc.producer_input(case, kind)
            src = torch.tensor(psf, dtype=RDT[dtype]).cuda()
            keep = src.clone()
            buf, out = guarded(ref.shape, CDT[dtype])
            rc = lib.pfb_psfhat_from_psf(_dev.code(RDT[dtype]), _dev.ptr(src), case.nband, P, Q, _dev.ptr(out), _dev.stream())
            assert rc == amd._lib.PFB_OK, lib.pfb_last_error()
            torch.cuda.synchronize()
            check_guard(buf, out, f"{case.id} {kind}")
            assert torch.equal(src, keep), "the input changed"
            err = relerr(out.cpu().numpy(), ref)
            print(f"coverage producer {case.id} {dtype} {kind}: {err:.2e} (tol {TOL_SPEC[dtype]:.0e})")
            note(log, 'producer', case, dtype, err)
            assert err < TOL_SPEC[dtype], (case, kind, err)


# --------------------------------------------------------------------------------------------------------- regrid
@pmp('case,dtype', cc.run_params('regrid'), ids=ids_of(cc.run_params('regrid')))
def test_regrid(amd, log, case, dtype):
    """pfb_psfhat_regrid in the format asked for, called directly, against the reference spectrum on the new grid."""
    lib, _dev = amd.lib, amd.dev
    nx, ny, P, Q, P2, Q2 = case.dims
    with Timer(log, f"regrid {case.id} {dtype}"):
        for kind in cc.INPUT_KINDS:
            ph, ref = cc.regrid_input(case, kind)
            src = torch.tensor(ph, dtype=CDT[dtype]).cuda()
            keep = src.clone()
            buf, out = guarded(ref.shape, CDT[dtype])
            rc = lib.pfb_psfhat_regrid(_dev.code(RDT[dtype]), _dev.ptr(src), case.nband, nx, ny, P, Q, P2, Q2, _dev.ptr(out),
                                       _dev.stream())
            assert rc == amd._lib.PFB_OK, lib.pfb_last_error()
            torch.cuda.synchronize()
            check_guard(buf, out, f"{case.id} {kind}")
            assert torch.equal(src, keep), "the input changed"
            err = relerr(out.cpu().numpy(), ref)
            print(f"coverage regrid {case.id} {dtype} {kind}: {err:.2e} (tol {TOL_SPEC[dtype]:.0e})")
            note(log, 'regrid', case, dtype, err)
            assert err < TOL_SPEC[dtype], (case, kind, err)


# --------------------------------------------------------------------------------------------------------- apply
# name, entry point, beam, wsum (0: none), sigmainv, dot_with, dot_with2
VARIANTS = (('plain', 'apply', False, 0.0, 0.0, None, None),
            ('plain-dots', 'dots', False, 0.0, 0.0, 'x', None),
            ('apply-dot-x', 'apply', True, 1.3, 0.7, 'x', None),
            ('dots-w-w2', 'dots', True, 1.3, 0.7, 'w', 'w2'),
            ('bands-x-w', 'bands', False, 0.0, 0.7, 'x', 'w'),
            ('bands-w', 'bands', True, 2.0, 0.0, 'w', None))
_apply_refs = {}


def apply_reference(case, kind, variant):
    name, _, beam_on, wsum, sigmainv, _, _ = variant
    key = (case.id, kind, name)
    if key not in _apply_refs:
        ph, x, w, w2, beam = cc.apply_input(case, kind)
        ref = cc.oracle_hessian(ph, case.dims[3], x, beam if beam_on else None, wsum if wsum > 0 else None, sigmainv)
        ref.setflags(write=False)
        _apply_refs[key] = ref
    return _apply_refs[key]


def run_apply(amd, plan, variant, dev_in, band0, nb):
    """One call on bands [band0, band0 + nb): (out, dots or None) as numpy, guards and inputs checked."""
    lib, _dev = amd.lib, amd.dev
    name, entry, beam_on, wsum, sigmainv, dw, dw2 = variant
    sl = slice(band0, band0 + nb)
    arg = {k: (v[sl] if k != 'ph' else v) for k, v in dev_in.items()}
    assert all(t.is_contiguous() for t in arg.values())
    keep = {k: v.clone() for k, v in arg.items()}
    obuf, out = guarded(arg['x'].shape, arg['x'].dtype)
    ndots = {'apply': 1, 'dots': 3, 'bands': 3 * nb}[entry] if dw else 0
    dbuf, dots = guarded((max(ndots, 1),), torch.float64)
    beam = _dev.ptr(arg['beam']) if beam_on else None
    pw, pw2 = (_dev.ptr(arg[dw]) if dw else None), (_dev.ptr(arg[dw2]) if dw2 else None)
    pd = _dev.ptr(dots) if dw else None
    head = (plan, band0, nb, _dev.ptr(arg['x']), beam, wsum, sigmainv, _dev.ptr(out), pw)
    if entry == 'apply':
        rc = lib.pfb_psfconv_apply(*head, pd, _dev.stream())
    elif entry == 'dots':
        rc = lib.pfb_psfconv_apply_dots(*head, pw2, pd, _dev.stream())
    else:
        rc = lib.pfb_psfconv_apply_dots_bands(*head, pw2, pd, _dev.stream())
    assert rc == amd._lib.PFB_OK, lib.pfb_last_error()
    torch.cuda.synchronize()
    check_guard(obuf, out, f"{name} out")
    if dw:
        check_guard(dbuf, dots, f"{name} dots")
    else:
        assert torch.all(torch.isnan(dots)) and torch.all(dbuf[:MARGIN] == SENTINEL)
    for k in arg:
        assert torch.equal(arg[k], keep[k]), f"{name}: the input {k} changed"
    return out.cpu().numpy(), (dots.cpu().numpy() if dw else None)


def check_dots(case, dtype, log, variant, got, out, ref, host, sl, refmax):
    """got: the entry's sums; out: its own output, ref: the oracle's, both on bands sl; refmax: max |ref| of the whole cube,
    the scale of the convolution's tolerance."""
    name, entry, _, _, _, dw, dw2 = variant
    o = out.astype(np.float64)
    wv, w2v = host[dw][sl], (host[dw2][sl] if dw2 else None)
    groups = [(b, slice(b, b + 1)) for b in range(o.shape[0])] if entry == 'bands' else [(0, slice(None))]
    for k, g in groups:
        own, want = cc.dots(wv[g], w2v[g] if dw2 else None, o[g]), cc.dots(wv[g], w2v[g] if dw2 else None, ref[g])
        no, nr, nw = np.linalg.norm(o[g]), np.linalg.norm(ref[g]), np.linalg.norm(wv[g])
        nw2 = np.linalg.norm(w2v[g]) if dw2 else 0.0
        d = np.sqrt(o[g].size) * TOL_CONV[dtype] * refmax
        scale = [nw * no, nw2 * no, no * no]
        slack = [nw * d, nw2 * d, (2 * nr + d) * d]
        for q in range(1 if entry == 'apply' else 3):
            v = got[3 * k + q] if entry == 'bands' else got[q]
            if q == 1 and not dw2:
                assert v == 0.0, (name, k, v)
                continue
            e_own = abs(v - own[q]) / max(scale[q], 1e-300)
            note(log, 'dots-own', case, dtype, e_own)
            assert e_own <= TOL_DOT[dtype], (name, k, q, v, own[q])
            bound = TOL_DOT[dtype] * scale[q] + slack[q]
            note(log, 'dots-oracle/bound', case, dtype, abs(v - want[q]) / max(bound, 1e-300))
            assert abs(v - want[q]) <= bound, (name, k, q, v, want[q], bound)


@pmp('case,dtype', cc.run_params('apply'), ids=ids_of(cc.run_params('apply')))
def test_apply(amd, log, monkeypatch, case, dtype):
    lib, _lib, _dev = amd.lib, amd._lib, amd.dev
    monkeypatch.setenv('PFB_FORCE_GENERIC', '1')
    nx, ny, P, Q = case.dims
    nband = case.nband
    plan = ctypes.c_void_p()
    _lib.check(lib.pfb_psfconv_plan_create(nx, ny, P, Q, nband, _dev.code(RDT[dtype]), ctypes.byref(plan)))
    try:
        fast = ctypes.c_int(-1)
        _lib.check(lib.pfb_psfconv_plan_info(plan, ctypes.byref(fast), None, None))
        assert fast.value == 0, "not a coverage plan"
        with Timer(log, f"apply {case.id} {dtype}"):
            for kind in cc.INPUT_KINDS:
                names = ('ph', 'x', 'w', 'w2', 'beam')
                host = dict(zip(names, cc.apply_input(case, kind)))
                dev_in = {k: torch.tensor(host[k], dtype=(CDT if k == 'ph' else RDT)[dtype]).cuda() for k in names}
                ph_keep = dev_in['ph'].clone()
                _lib.check(lib.pfb_psfconv_set_psfhat(plan, _dev.ptr(dev_in['ph']), _dev.stream()))
                torch.cuda.synchronize()
                outs = {}
                for variant in VARIANTS:
                    name = variant[0]
                    ref = apply_reference(case, kind, variant)
                    out, got = run_apply(amd, plan, variant, dev_in, 0, nband)
                    outs[name] = out
                    err = relerr(out, ref)
                    print(f"coverage apply {case.id} {dtype} {kind} {name}: {err:.2e} (tol {TOL_CONV[dtype]:.0e})")
                    note(log, 'apply', case, dtype, err)
                    assert err < TOL_CONV[dtype], (case, kind, name, err)
                    if got is not None:
                        check_dots(case, dtype, log, variant, got, out, ref, host, slice(0, nband), np.abs(ref).max())
                    if nband == 3 and name in ('plain', 'dots-w-w2', 'bands-x-w'):
                        for band0, nb in ((1, 1), (1, 2)):
                            sl = slice(band0, band0 + nb)
                            sub, sgot = run_apply(amd, plan, variant, dev_in, band0, nb)
                            assert np.array_equal(sub, out[sl]), (case, kind, name, band0, nb)
                            if sgot is not None:
                                check_dots(case, dtype, log, variant, sgot, sub, ref[sl], host, sl, np.abs(ref).max())
                assert np.array_equal(outs['plain'], outs['plain-dots']), "the samples depend on whether sums are asked for"
                assert torch.equal(dev_in['ph'], ph_keep)
    finally:
        lib.pfb_psfconv_plan_destroy(plan)
