"""
The power-of-two convolution kernels (csrc/fftconv_pow2.hip) at trip, tile and band edges: plain, persistent and two-level
column kernels, plain and persistent row kernels in every mode, and the PSFHAT producer on the fast path, against float64
references through oracle.fftconv, in float32 and float64.

tests/pow2_cases.py holds the cases and the property each exists for; tests/test_cpu_pow2_cases.py proves on the CPU that
every case has its property and that the table leaves no cell of its coverage matrices empty.  This module reads the CU
count from the device, asserts the case's property AT THAT COUNT, and builds its plan directly with
pfb_psfconv_plan_create, so that the class named runs and nothing is embedded; fast_path is asserted through
pfb_psfconv_plan_info.

Every case runs on seeded white noise and on unit impulses, one per band on a tile-edge row (pow2_cases.impulse_positions).
For every call:

  guards      the output and the sums live inside larger buffers, NaN inside, 64 sentinels on either side; afterwards the
              inside is finite and the margins are intact; x, beam, w, w2 and the caller's psfhat equal their copies bit
              for bit
  point-wise  max |got - ref| / max |ref| PER BAND against TOL_CONV (1e-5 float32, 1e-12 float64), the producer's
              spectrum against TOL_SPEC (2e-6, 1e-12)
  sums        against float64 sums of the kernel's own output, |got - own| <= TOL_DOT (|w| |out|, |w2| |out|, |out|^2)
              with TOL_DOT = 1e-9 (float32), 1e-12 (float64) as in test_gpu_pcg_bands.py; the per-band sums add up to the
              whole-cube sums within the same bound
  bit for bit the same call twice gives the same output and the same sums (the persistent kernels keep prefetches in
              flight across barriers: a race shows as a difference); a band sub-range equals those bands of the whole
              launch (not in group d: the non-temporal choice depends on the band count)

A call with dot_with2 but no dot_with -- the one way into the plain inverse kernel that launch_row_inv provides for
beside an independent dot_with -- is refused by the entry points (PFB_ERR_INVALID) and leaves the output untouched;
test_dot_with2_alone_is_refused pins that.

Measured at the commit that added this module (MI355X, 256 CUs), worst band of any case, in max norm: convolutions
1.1e-6 (float32, three trips of the 4096-point rows) and 1.2e-15 (float64), the producer's spectrum 6.4e-7 and 5.6e-16,
the sums 1.4e-15 and 4.4e-16 of their scale: no class needs more than about a tenth of
TOL_CONV, a third of TOL_SPEC.  145 tests in 42 s, none above 2.0 s.  Most of that is the float64 references, which
pow2_cases.store computes once per image size and band: the cases are run sorted by size.
"""
import ctypes
import time

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from oracle import fftconv as ofc           # noqa: E402
import pow2_cases as pc                     # noqa: E402

pmp = pytest.mark.parametrize
F32, F64 = pc.F32, pc.F64
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
    ns.ncu = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    return ns


@pytest.fixture(scope='module')
def log():
    """Worst error per (what, group, format) and the wall time per test; printed when the module is done."""
    rec = {'worst': {}, 'times': {}, 't0': time.perf_counter()}
    yield rec
    print("\npow2 edges: worst error relative to its tolerance's scale, per check, group and format")
    for key in sorted(rec['worst']):
        err, cid = rec['worst'][key]
        print(f"  {key[0]:<18} ({key[1]}) {key[2]}: {err:.3e}   [{cid}]")
    if rec['times']:
        print("pow2 edges: wall time per test, references included")
        for name, t in rec['times'].items():
            print(f"  {name:<44} {t:6.2f} s")
        slow = max(rec['times'], key=rec['times'].get)
        print(f"pow2 edges: {len(rec['times'])} tests, module wall time {time.perf_counter() - rec['t0']:.1f} s, "
              f"sum of tests {sum(rec['times'].values()):.1f} s, slowest {slow} {rec['times'][slow]:.2f} s")


def note(log, what, case, err):
    key = (what, case.group, case.dtype)
    if key not in log['worst'] or err > log['worst'][key][0]:
        log['worst'][key] = (err, case.id)


class Timer:
    def __init__(self, log, name):
        self.log, self.name = log, name

    def __enter__(self):
        self.t = time.perf_counter()

    def __exit__(self, *a):
        self.log['times'][self.name] = time.perf_counter() - self.t


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


def band_errors(got, ref):
    """max |got - ref| / max |ref| per band, on the device in float64 (complex128 for spectra)"""
    d = (got.to(ref.dtype) - ref).abs().flatten(1).amax(dim=1)
    return (d / ref.abs().flatten(1).amax(dim=1)).cpu().numpy()


class Plan:
    def __init__(self, amd, case, nband):
        self.amd, self.h = amd, ctypes.c_void_p()
        amd._lib.check(amd.lib.pfb_psfconv_plan_create(case.nx, case.ny, 2 * case.nx, 2 * case.ny, nband,
                                                       amd.dev.code(RDT[case.dtype]), ctypes.byref(self.h)))

    def __enter__(self):
        fast = ctypes.c_int(-1)
        self.amd._lib.check(self.amd.lib.pfb_psfconv_plan_info(self.h, ctypes.byref(fast), None, None))
        assert fast.value == 1, "not a fast-path plan"
        return self.h

    def __exit__(self, *a):
        self.amd.lib.pfb_psfconv_plan_destroy(self.h)


def install_psfhat(amd, plan, ph, dtype):
    """pfb_psfconv_set_psfhat from a device copy of `ph`, which must come back unchanged"""
    dev = torch.tensor(ph, dtype=CDT[dtype]).cuda()
    keep = dev.clone()
    amd._lib.check(amd.lib.pfb_psfconv_set_psfhat(plan, amd.dev.ptr(dev), amd.dev.stream()))
    torch.cuda.synchronize()
    assert torch.equal(dev, keep), "set_psfhat changed the caller's psfhat"


def run_apply(amd, plan, variant, dev_in, keep, band0, nb):
    """One call on bands [band0, band0 + nb): (out, sums or None) on the device, guards and inputs checked."""
    lib, _dev = amd.lib, amd.dev
    (call, beam_on), (entry, dw, dw2) = variant, pc.CALLS[variant[0]]
    wsum, sigmainv = pc.BEAM_ARGS[beam_on]
    sl = slice(band0, band0 + nb)
    arg = {k: v[sl] for k, v in dev_in.items()}
    assert all(t.is_contiguous() for t in arg.values())
    obuf, out = guarded(arg['x'].shape, arg['x'].dtype)
    ndots = {'apply': 1, 'dots': 3, 'bands': 3 * nb}[entry] if dw else 0
    dbuf, sums = guarded((max(ndots, 1),), torch.float64)
    beam = _dev.ptr(arg['beam']) if beam_on else None
    pw, pw2 = (_dev.ptr(arg[dw]) if dw else None), (_dev.ptr(arg[dw2]) if dw2 else None)
    pd = _dev.ptr(sums) if dw else None
    head = (plan, band0, nb, _dev.ptr(arg['x']), beam, wsum, sigmainv, _dev.ptr(out), pw)
    if entry == 'apply':
        rc = lib.pfb_psfconv_apply(*head, pd, _dev.stream())
    elif entry == 'dots':
        rc = lib.pfb_psfconv_apply_dots(*head, pw2, pd, _dev.stream())
    else:
        rc = lib.pfb_psfconv_apply_dots_bands(*head, pw2, pd, _dev.stream())
    assert rc == amd._lib.PFB_OK, lib.pfb_last_error()
    torch.cuda.synchronize()
    what = f"{call}{'+beam' if beam_on else ''} bands [{band0}, {band0 + nb})"
    check_guard(obuf, out, what + " out")
    if dw:
        check_guard(dbuf, sums, what + " sums")
    else:
        assert torch.all(torch.isnan(sums)) and torch.all(dbuf[:MARGIN] == SENTINEL)
    for k in dev_in:
        assert torch.equal(dev_in[k], keep[k]), f"{what}: the input {k} changed"
    return out, (sums if dw else None)


def own_sums(variant, dev_in, out, sl):
    """float64 sums of the kernel's own output and their scales: per band [nb, 3] each"""
    _, dw, dw2 = pc.CALLS[variant[0]]
    o = out.double().flatten(1)
    w = dev_in[dw][sl].double().flatten(1)
    w2 = dev_in[dw2][sl].double().flatten(1) if dw2 else torch.zeros_like(o)
    own = torch.stack([(w * o).sum(1), (w2 * o).sum(1), (o * o).sum(1)], dim=1)
    sq = torch.stack([(w * w).sum(1), (w2 * w2).sum(1), (o * o).sum(1)], dim=1)
    return own.cpu().numpy(), sq.cpu().numpy()


def check_sums(case, log, variant, got, dev_in, out, sl):
    """got: the entry's sums (device).  Returns the whole-range sums (3,) for the per-band / whole-cube comparison."""
    entry, dw, dw2 = pc.CALLS[variant[0]]
    own, sq = own_sums(variant, dev_in, out, sl)
    got = got.cpu().numpy()
    tol = TOL_DOT[case.dtype]
    if entry == 'bands':
        got = got.reshape(-1, 3)
        scale = np.sqrt(sq * sq[:, 2:3])                    # |w| |out|, |w2| |out|, |out|^2 per band
        want = own
    else:
        tot = sq.sum(0)
        scale, want, got = np.sqrt(tot * tot[2])[None], own.sum(0)[None], got[None]
    if not dw2:
        assert np.all(got[:, 1] == 0.0), (variant, got[:, 1])
    err = np.abs(got - want) / np.maximum(scale, 1e-300)
    if not dw2:
        err[:, 1] = 0.0
    note(log, 'sums-own', case, err.max() / tol)
    assert err.max() <= tol, (case, variant, err, got, want)
    tot = sq.sum(0)
    return got.sum(0), np.sqrt(tot * tot[2])


# ------------------------------------------------------------------------------------------------------------ apply
APPLY = pc.run_params('abcd')


@pmp('case', APPLY, ids=[c.id for c in APPLY])
def test_apply(amd, log, case):
    ncu, d = amd.ncu, case.dtype
    assert case.holds(ncu), f"{case} has lost its property at {ncu} CUs"
    n = case.nband(ncu)
    with Timer(log, f"apply {case.id}"), Plan(amd, case, n) as plan:
        base = pc.inputs(case, 'noise', ncu)
        install_psfhat(amd, plan, base['ph'], d)
        ops = {k: torch.tensor(base[k], dtype=RDT[d]).cuda() for k in case.operands()}
        for kind in pc.INPUT_KINDS:
            host = pc.inputs(case, kind, ncu)
            dev_in = dict(ops, x=torch.tensor(host['x'], dtype=RDT[d]).cuda())
            keep = {k: v.clone() for k, v in dev_in.items()}
            totals, refs = {}, {}
            for variant in case.variants:
                call, beam_on = variant
                if beam_on not in refs:
                    refs.clear()
                    refs[beam_on] = torch.tensor(pc.reference(case, kind, beam_on, ncu)).cuda()
                ref = refs[beam_on]
                out, sums = run_apply(amd, plan, variant, dev_in, keep, 0, n)
                errs = band_errors(out, ref)
                print(f"pow2 apply {case.id} {kind} {call}{'+beam' if beam_on else ''}: worst band {errs.max():.2e} "
                      f"(tol {TOL_CONV[d]:.0e})")
                note(log, 'apply', case, errs.max() / TOL_CONV[d])
                assert errs.max() < TOL_CONV[d], (case, kind, variant, errs)
                if sums is not None:
                    totals[variant] = check_sums(case, log, variant, sums, dev_in, out, slice(0, n))
                if case.group == 'd':
                    continue
                # the same call again: bit for bit
                out2, sums2 = run_apply(amd, plan, variant, dev_in, keep, 0, n)
                assert torch.equal(out, out2), (case, kind, variant, "two runs differ")
                assert sums is None or torch.equal(sums, sums2), (case, kind, variant, "the sums of two runs differ")
                del out2
                for band0, nb in case.ranges(ncu)[1:]:
                    sl = slice(band0, band0 + nb)
                    sub, ssum = run_apply(amd, plan, variant, dev_in, keep, band0, nb)
                    assert torch.equal(sub, out[sl]), (case, kind, variant, band0, nb, "sub-range differs from the whole launch")
                    if ssum is not None:
                        check_sums(case, log, variant, ssum, dev_in, sub, sl)
                    del sub
            # per-band sums add up to the whole-cube sums
            for beam_on in (False, True):
                for whole, bands in (('dot-x', 'bands-x'), ('dot-x-w', 'bands-x-w'), ('dot-w-w2', 'bands-w-w2')):
                    if (whole, beam_on) in totals and (bands, beam_on) in totals:
                        (a, scale), (b, _) = totals[(whole, beam_on)], totals[(bands, beam_on)]
                        err = (np.abs(a - b) / np.maximum(scale, 1e-300)).max()
                        note(log, 'sums-bands-whole', case, err / TOL_DOT[d])
                        assert err <= TOL_DOT[d], (case, kind, whole, bands, a, b)


def test_dot_with2_alone_is_refused(amd):
    """dot_with2 without dot_with: every entry point refuses it before anything is launched."""
    case = pc.by_id('a-row1024-f32')
    with Plan(amd, case, 2) as plan:
        host = pc.inputs(case, 'noise', amd.ncu)
        install_psfhat(amd, plan, host['ph'], case.dtype)
        x, w = (torch.tensor(host[k], dtype=torch.float32).cuda() for k in ('x', 'w'))
        obuf, out = guarded(x.shape, x.dtype)
        dbuf, sums = guarded((6,), torch.float64)
        p = amd.dev.ptr
        for fn in (amd.lib.pfb_psfconv_apply_dots, amd.lib.pfb_psfconv_apply_dots_bands):
            rc = fn(plan, 0, 2, p(x), None, 0.0, 0.0, p(out), None, p(w), p(sums), amd.dev.stream())
            assert rc == amd._lib.PFB_ERR_INVALID
        torch.cuda.synchronize()
        assert torch.all(torch.isnan(out)) and torch.all(torch.isnan(sums))
        assert torch.all(obuf[:MARGIN] == SENTINEL) and torch.all(dbuf[:MARGIN] == SENTINEL)


# ------------------------------------------------------------------------------------------------------------ producer
PRODUCER = pc.run_params('e')


@pmp('case', PRODUCER, ids=[c.id for c in PRODUCER])
def test_producer(amd, log, case):
    """pfb_psfconv_set_psf with psfhat_out against oracle.fftconv.psfhat_from_psf, and the plan it leaves against a plan
    given the oracle's spectrum: both convolve like the oracle."""
    lib, _lib, _dev, d = amd.lib, amd._lib, amd.dev, case.dtype
    nx, ny, n = case.nx, case.ny, case.nband(amd.ncu)
    assert case.holds(amd.ncu)
    with Timer(log, f"producer {case.id}"), Plan(amd, case, n) as plan:
        psf = pc.make_psf(case, amd.ncu)
        ref_hat = ofc.psfhat_from_psf(psf, nthreads=pc.NTHREADS)
        src = torch.tensor(psf, dtype=RDT[d]).cuda()
        keep = src.clone()
        buf, hat = guarded(ref_hat.shape, CDT[d])
        rc = lib.pfb_psfconv_set_psf(plan, _dev.ptr(src), _dev.ptr(hat), _dev.stream())
        assert rc == _lib.PFB_OK, lib.pfb_last_error()
        torch.cuda.synchronize()
        check_guard(buf, hat, f"{case.id} psfhat_out")
        assert torch.equal(src, keep), "the PSF changed"
        errs = band_errors(hat, torch.tensor(ref_hat).cuda())
        print(f"pow2 producer {case.id}: worst band {errs.max():.2e} (tol {TOL_SPEC[d]:.0e})")
        note(log, 'producer', case, errs.max() / TOL_SPEC[d])
        assert errs.max() < TOL_SPEC[d], (case, errs)
        del src, keep, buf, hat
        # the plan set_psf left, and a second one given the oracle's spectrum, on noise and on the impulses
        for kind in pc.INPUT_KINDS:
            xh = pc.inputs(case, kind, amd.ncu)['x']
            Q = 2 * ny
            ref = torch.tensor(ofc.psf_convolve_cube(*ofc.make_scratch(ref_hat, Q, xh.shape, np.float64), ref_hat, Q, xh,
                                                     nthreads=pc.NTHREADS)).cuda()
            dev_in = {'x': torch.tensor(xh, dtype=RDT[d]).cuda()}
            keepx = {'x': dev_in['x'].clone()}
            out, _ = run_apply(amd, plan, ('none', False), dev_in, keepx, 0, n)
            errs = band_errors(out, ref)
            note(log, 'producer-apply', case, errs.max() / TOL_CONV[d])
            assert errs.max() < TOL_CONV[d], (case, kind, errs)
            with Plan(amd, case, n) as plan2:
                install_psfhat(amd, plan2, ref_hat, d)
                out2, _ = run_apply(amd, plan2, ('none', False), dev_in, keepx, 0, n)
                errs2 = band_errors(out2, ref)
                assert errs2.max() < TOL_CONV[d], (case, kind, errs2)
                between = band_errors(out, out2.double())
                print(f"pow2 producer {case.id} {kind}: apply {errs.max():.2e}, with the oracle's spectrum {errs2.max():.2e}, "
                      f"between the two {between.max():.2e} (tol {TOL_CONV[d]:.0e})")
                note(log, 'producer-vs-oracle-plan', case, between.max() / TOL_CONV[d])
                assert between.max() < TOL_CONV[d], (case, kind, between)
