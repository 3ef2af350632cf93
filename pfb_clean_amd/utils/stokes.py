"""
Stokes visibilities and weights from correlations and Jones terms on MI355X -- what the reference's init and fastim
workers do between reading a chunk and the `vis, wgt, mask` that the grid worker consumes (pfb/utils/stokes.py,
pfb/utils/weighting.py:281-350, pfb/utils/stokes2im.py:98-195; csrc/stokes.hip).

    stokes_basis   the 2 x 2 basis matrix B of (pol, product)
    stokes_vis     vis, wgt, mask, wsum from the raw columns of a chunk, one kernel: of one product, or of up to four
                   ('IQUV') as leading planes from one pass over the columns; chan_average=n then averages bins of n
                   channels on the device
    average_channels   that averaging of vis, wgt, mask that exist (a dataset an earlier run converted)
    average_freq   the averaged channels' frequencies and widths, on the host

The reference generates its per-visibility functions with sympy; they have the closed form

    vis = 1/2 tr(B^H Gp^-1 V Gq^-H)            wgt = sum_ab w_ab |(Gp B Gq^H)_ab|^2

with Gp, Gq the Jones matrices of the row's antennas at its time bin and channel (direction 0), V the 2 x 2 matrix of
the row's correlations and w their weights (the weights cancel out of vis).  With two correlations V = diag(v0, v1),
w01 = w10 = 1: U, V linear and Q, U circular give vis = 0 with a non-zero wgt, as in the reference.

numpy in gives numpy out, tensors in give tensors out; there is no CPU path.

Where this differs from the reference, by definition:
  * tbin_idx is never modified (the reference subtracts its minimum in place; here it is subtracted on read);
  * the time bins must be ascending and must not overlap, anything else is a ValueError.  tbin_idx and tbin_counts are
    index metadata of ntime entries: they are read on the host for that check, whatever kind of array they are;
  * an unknown pol, product or number of correlations, and a full 2 x 2 Jones term with 2 correlations, are a
    ValueError (the reference fails with NameError / IndexError);
  * a singular Jones matrix on an unflagged visibility gives IEEE inf / nan as in the reference; it is not an error;
  * a row with an antenna index outside the Jones term's antenna axis gets zeros (the reference: IndexError).
"""
import ctypes as C

import numpy as np
import torch

from .. import _dev, _lib

# (pol, product) -> index of the basis matrix in BASIS_MATRICES (PFB's basis codes)
BASIS_INDEX = {('linear', 'I'): 0, ('linear', 'Q'): 1, ('linear', 'U'): 2, ('linear', 'V'): 3,
               ('circular', 'I'): 0, ('circular', 'V'): 1, ('circular', 'Q'): 2, ('circular', 'U'): 3}
BASIS_MATRICES = (((1, 0), (0, 1)), ((1, 0), (0, -1)), ((0, 1), (1, 0)), ((0, 1j), (-1j, 0)))
# PFB_STOKES_* of include/pfb_hip.h
DIAG4, DIAG2, FULL4, NOJ4, NOJ2 = range(5)
W_NONE, W_SIGMA, W_SPECTRUM, W_ROW = range(4)
_PRECISION = {'single': torch.complex64, 'double': torch.complex128}


def basis_index(pol, product):
    try:
        return BASIS_INDEX[(str(pol), str(product))]
    except KeyError:
        raise ValueError(f"unknown polarisation type / product ({pol!r}, {product!r}): pol is 'linear' or 'circular', "
                         "product one of 'I', 'Q', 'U', 'V'") from None


def product_letters(product):
    """`product` as its letters: None for ONE product given as a one-letter string (the 2-D results of always), else
    the tuple of letters of a stacked call -- a string of 2 to 4 letters ('IQUV', 'QU', 'VI') or a sequence of one-letter
    strings (('U', 'I', 'Q'); a sequence of one letter is a stack of one plane) --, in the order asked.  No letters, more
    than four and a repeated letter are a ValueError; what a letter means is basis_index's to say."""
    if isinstance(product, str):
        if len(product) == 1:
            return None
        letters = tuple(product)
    else:
        try:
            letters = tuple(product)
        except TypeError:
            raise ValueError(f"product must be a string of letters from 'IQUV' or a sequence of them, got {product!r}") from None
        if not all(isinstance(p, str) and len(p) == 1 for p in letters):
            raise ValueError(f"a sequence of products holds one letter each, got {product!r}")
    if not 1 <= len(letters) <= 4:
        raise ValueError(f"1 to 4 products in one call, got {product!r}")
    if len(set(letters)) != len(letters):
        raise ValueError(f"a product is asked for twice in {product!r}")
    return letters


def basis_list(pol, product):
    """The basis index of a single product, or the list of them -- one per plane, in the order asked -- of a stacked
    one (product_letters)."""
    letters = product_letters(product)
    if letters is None:
        return basis_index(pol, product)
    return [basis_index(pol, p) for p in letters]


def stokes_basis(pol, product):
    """The basis matrix B of (pol, product) as a (2, 2) complex128 numpy array:
        [[1, 0], [0, 1]]  I          [[1, 0], [0, -1]]  Q linear, V circular
        [[0, 1], [1, 0]]  U linear, Q circular          [[0, i], [-i, 0]]  V linear, U circular"""
    return np.array(BASIS_MATRICES[basis_index(pol, product)], dtype=np.complex128)


def ncorr_of(nc):
    """'2' / '4' or the integers; everything else: ValueError."""
    try:
        n = int(str(nc))
    except ValueError:
        n = None
    if n not in (2, 4):
        raise ValueError(f"the product is available from 2 or 4 correlations, got nc={nc!r}")
    return n


def _aligned(t, nbytes):
    """t itself where the kernel's vector loads can read it, else a copy (a fresh allocation is aligned)."""
    return t if t is None or t.data_ptr() % min(nbytes, 16) == 0 else t.clone()


def _time_bins(tbin_idx, tbin_counts, dev):
    """(tbin_idx, tbin_counts) as int64 device tensors -- copies, the caller's arrays stay as they are -- and the
    minimum of tbin_idx, after the host's check that the bins ascend without overlap."""
    host = []
    for a in (tbin_idx, tbin_counts):
        a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        if a.dtype.kind not in 'iu':
            raise ValueError("tbin_idx and tbin_counts must be integer arrays")
        host.append(a.astype(np.int64))
    ti, tc = host
    if ti.ndim != 1 or ti.shape != tc.shape or ti.size == 0:
        raise ValueError("tbin_idx and tbin_counts must be one-dimensional, of one length >= 1")
    if (tc < 0).any() or (ti[1:] < ti[:-1] + tc[:-1]).any():
        raise ValueError("the time bins must be ascending and must not overlap")
    return torch.from_numpy(ti).to(dev), torch.from_numpy(tc).to(dev), int(ti[0])


def check_chan_average(n):
    """chan_average as an int >= 1; anything else: ValueError."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
        raise ValueError(f"chan_average must be an integer >= 1, got {n!r}")
    if n > 0x7fffffff:
        raise ValueError(f"chan_average {n} does not fit an int; one bin takes chan_average >= nchan")
    return int(n)


def _average_dev(vis, wgt, mask, n):
    """pfb_chan_average on device tensors of their final types: vis, wgt ([nprod,] nrow, nchan), mask (nrow, nchan) ->
    vis, wgt ([nprod,] nrow, nchan_out), mask (nrow, nchan_out) and the fp64 sums, one per plane."""
    lead = tuple(vis.shape[:-2])
    nrow, nchan = (int(k) for k in vis.shape[-2:])
    nout = -(-nchan // n)
    nprod = lead[0] if lead else 1
    viso = torch.empty(lead + (nrow, nout), dtype=vis.dtype, device=vis.device)
    wgto = torch.empty(lead + (nrow, nout), dtype=wgt.dtype, device=vis.device)
    masko = torch.empty((nrow, nout), dtype=torch.uint8, device=vis.device)
    rec = torch.zeros(nprod, dtype=torch.float64, device=vis.device)
    if nrow * nchan:
        _lib.check(_lib.load().pfb_chan_average(
            _dev.code(wgt.dtype), nprod, _dev.ptr(vis), _dev.ptr(wgt), _dev.ptr(mask), nrow, nchan, n, _dev.ptr(viso),
            _dev.ptr(wgto), _dev.ptr(masko), _dev.ptr(rec), _dev.ptr(_dev.scratch()[0]), _dev.stream()))
    return viso, wgto, masko, rec


def run(data, weight, wform, flag, frow, autocorr, jones, tbin_idx, tbin_counts, ant1, ant2, basis, data2=None,
        subtract=False, chan_average=1):
    """The one launch.  Device tensors of their final types in: data, data2 complex (nrow, nchan, 2 | 4); weight real per
    wform; flag uint8 (nrow, nchan) or (nrow, nchan, ncorr) or None; frow uint8 (nrow,) or None; jones
    (ntime, nant, nchan, ndir, 2[, 2]) or None.  `basis` is a basis index -- vis, wgt, mask (nrow, nchan) and the fp64
    one-element sum of the unflagged wgt -- or a list of nprod distinct ones (basis_list): vis, wgt (nprod, nrow, nchan),
    the planes in the list's order, mask (nrow, nchan) and nprod sums, from one pass over the inputs.  All on the device;
    nothing is read back.  chan_average = n > 1: the same with ceil(nchan / n) channels, the weighted means of DESIGN
    4.16, by pfb_chan_average behind the pass; n = 1 is the call of always."""
    n = check_chan_average(chan_average)
    if data.ndim != 3 or data.dtype not in _dev.REAL_OF:
        raise TypeError("data must be complex64 or complex128 of shape (nrow, nchan, ncorr)")
    rdt = _dev.REAL_OF[data.dtype]
    nrow, nchan, nc = (int(n) for n in data.shape)
    ncorr_of(nc)
    esize = 4 if rdt == torch.float32 else 8
    dev = data.device
    ti, tc, off = _time_bins(tbin_idx, tbin_counts, dev)
    if jones is None:
        mode, ndir, nant = (NOJ4 if nc == 4 else NOJ2), 1, 1 << 30
    else:
        if jones.ndim not in (5, 6):
            raise ValueError("Jones term has incorrect number of dimensions")
        if jones.ndim == 6 and nc == 2:
            raise ValueError("a full 2 x 2 Jones term needs 4 correlations, the data have 2")
        if jones.dtype != data.dtype:
            raise TypeError(f"jones must be {data.dtype}, got {jones.dtype}")
        if (tuple(jones.shape[4:]) != ((2,) if jones.ndim == 5 else (2, 2)) or jones.shape[0] != ti.numel()
                or jones.shape[2] != nchan or jones.shape[1] < 1 or jones.shape[3] < 1):
            raise ValueError(f"jones must be (ntime={ti.numel()}, nant, nchan={nchan}, ndir, 2[, 2]), got "
                             f"{tuple(jones.shape)}")
        mode = FULL4 if jones.ndim == 6 else DIAG4 if nc == 4 else DIAG2
        nant, ndir = int(jones.shape[1]), int(jones.shape[3])
        jones = _aligned(jones, 2 * esize * (4 if mode == FULL4 else 2))
    if data2 is not None and (data2.dtype != data.dtype or data2.shape != data.shape):
        raise TypeError("data2 must have the type and shape of data")
    if wform != W_NONE:
        want = (nrow, nc) if wform == W_ROW else (nrow, nchan, nc)
        if weight.dtype != rdt or tuple(weight.shape) != want:
            raise TypeError(f"the weights must be {rdt} of shape {want}, got {weight.dtype} {tuple(weight.shape)}")
    nfc = 0 if flag is None else 1 if flag.ndim == 2 else nc
    a1, a2 = (_dev.to_dev(a).to(torch.int32) for a in (ant1, ant2))
    if tuple(a1.shape) != (nrow,) or tuple(a2.shape) != (nrow,):
        raise ValueError(f"ant1 and ant2 must have shape ({nrow},)")
    # one product: (nrow, nchan) through pfb_stokes_vis; a list of them: a leading axis through pfb_stokes_vis_multi
    stacked = isinstance(basis, (list, tuple))
    lead = (len(basis),) if stacked else ()
    vis = torch.empty(lead + (nrow, nchan), dtype=data.dtype, device=dev)
    wgt = torch.empty(lead + (nrow, nchan), dtype=rdt, device=dev)
    mask = torch.empty((nrow, nchan), dtype=torch.uint8, device=dev)
    rec = torch.zeros(len(basis) if stacked else 1, dtype=torch.float64, device=dev)
    if nrow * nchan:
        data, data2 = _aligned(data, 2 * esize * nc), _aligned(data2, 2 * esize * nc)
        weight = None if wform == W_NONE else _aligned(weight, esize * nc)
        flag = _aligned(flag, nfc) if nfc > 1 else flag
        lib = _lib.load()
        if stacked:
            entry, which = lib.pfb_stokes_vis_multi, (len(basis), (C.c_int * len(basis))(*basis))
        else:
            entry, which = lib.pfb_stokes_vis, (basis,)
        _lib.check(entry(
            _dev.code(rdt), mode, *which, _dev.ptr(data), _dev.ptr(data2), int(bool(subtract)), _dev.ptr(weight), wform,
            _dev.ptr(flag), nfc, _dev.ptr(frow), int(bool(autocorr)), _dev.ptr(jones), ndir, ti.numel(), nant,
            _dev.ptr(ti), _dev.ptr(tc), off, _dev.ptr(a1), _dev.ptr(a2), nrow, nchan, _dev.ptr(vis), _dev.ptr(wgt),
            _dev.ptr(mask), _dev.ptr(rec), _dev.ptr(_dev.scratch()[0]), _dev.stream()))
    if n > 1:
        return _average_dev(vis, wgt, mask, n)
    return vis, wgt, mask, rec


def stokes_vis(data, ant1, ant2, tbin_idx, tbin_counts, poltype, product, data2=None, operator=None, sigma=None,
               weight=None, flag=None, frow=None, jones=None, precision='single', chan_average=1):
    """stokes2im.py:98-195 (and stokes2vis.py:76-160, 233-240) as one kernel: (vis, wgt, mask, wsum).

    data (nrow, nchan, ncorr) complex, ncorr 2 or 4; data2 with operator '+' or '-' is added or subtracted;
    the weights are sigma -> 1 / sigma^2, else weight (nrow, nchan, ncorr), or (nrow, ncorr) broadcast over channels,
    else ones; the flag is any(flag, 2) | frow[:, None] | (ant1 == ant2)[:, None], flag (nrow, nchan, ncorr) and frow
    (nrow,) each optional.  jones is None or in QuartiCal's layout (ntime, nchan, nant, ndir, 2 or 4): 2 is the diagonal,
    4 the full matrix.  The channel and antenna axes are swapped by ONE permuting copy (then the reference's reshape to
    (..., 2, 2), a view), not by strides: along a row the kernel then reads Jones terms that are contiguous in the
    channel, and the Jones terms are smaller than the data by about half the number of antennas.  Only direction 0 is
    read.  Data, weights or Jones terms in the other precision are cast with one .to() each, as the reference casts them.

    vis (nrow, nchan) complex and wgt (nrow, nchan) real of `precision`; mask = (~flag) as uint8; wsum the sum of wgt
    over unflagged visibilities, accumulated in fp64, as a one-element array of wgt's type.  Flagged visibilities and
    rows that no time bin covers get vis = wgt = 0, whatever their data hold.  Differences from the reference: see the
    module.

    Several products in one pass (the reference has none: its fastim worker refuses anything but one letter): `product`
    a string of 2 to 4 distinct letters ('IQUV', 'QU', 'VI') or a sequence of letters gives vis and wgt
    (nprod, nrow, nchan), the planes in the order asked, mask (nrow, nchan) -- it does not depend on the product -- and
    wsum (nprod,).  Every input is read once.  A repeated or unknown letter is a ValueError.

    chan_average = n > 1 (stokes2vis.py:174-203) averages bins of n channels behind the pass, on the device: vis, wgt,
    mask come out with ceil(nchan / n) channels -- the last bin may be short, n > nchan gives one -- as wgt = the sum of
    the bin's live wgt, vis = their weighted mean (exactly 0 where that sum is 0), mask = any of the bin's; wsum is the
    sum of the averaged wgt over the averaged mask.  average_freq gives the bins' frequencies.  n = 1 is the call of
    always, the same bits."""
    check_chan_average(chan_average)
    if str(precision).lower() not in _PRECISION:
        raise ValueError(f"precision must be 'single' or 'double', got {precision!r}")
    cdt = _PRECISION[str(precision).lower()]
    rdt = _dev.REAL_OF[cdt]
    basis = basis_list(poltype, product)
    dd = _dev.to_dev(data)
    if dd.ndim != 3 or not dd.is_complex():
        raise TypeError("data must be complex of shape (nrow, nchan, ncorr)")
    nrow, nchan, nc = (int(n) for n in dd.shape)
    ncorr_of(nc)
    dd = dd.to(cdt)
    d2 = None
    if data2 is not None:
        if operator not in ('+', '-'):
            raise ValueError(f"operator must be '+' or '-' with a second data column, got {operator!r}")
        d2 = _dev.to_dev(data2).to(cdt)
    if sigma is not None:
        wd, wform = _dev.to_dev(sigma).to(rdt), W_SIGMA
    elif weight is not None:
        wd = _dev.to_dev(weight).to(rdt)
        wform = W_ROW if wd.ndim == 2 else W_SPECTRUM
    else:
        wd, wform = None, W_NONE
    fd = None if flag is None else _dev.byte_mask(flag, (nrow, nchan, nc), 'flag')
    fr = None if frow is None else _dev.byte_mask(frow, (nrow,), 'frow')
    jd = None
    if jones is not None:
        jd = _dev.to_dev(jones)
        if jd.ndim != 5 or jd.shape[-1] not in (2, 4):
            raise ValueError(f"jones must be (ntime, nchan, nant, ndir, 2 or 4), got {tuple(jd.shape)}")
        jd = jd.to(cdt).swapaxes(1, 2).contiguous()
        if jd.shape[-1] == 4:
            jd = jd.reshape(*jd.shape[:4], 2, 2)
    vis, wgt, mask, rec = run(dd, wd, wform, fd, fr, True, jd, tbin_idx, tbin_counts, ant1, ant2, basis, data2=d2,
                              subtract=operator == '-', chan_average=chan_average)
    return tuple(_dev.host_like(t, data) for t in (vis, wgt, mask, rec.to(rdt)))


def average_channels(vis, wgt, mask, n):
    """Bins of n channels of vis, wgt (nrow, nchan), or (nprod <= 4, nrow, nchan) with the one mask (nrow, nchan), as
    stokes_vis(..., chan_average=n) forms them: (vis, wgt, mask, wsum) with ceil(nchan / n) channels,
        wgt_out = sum of wgt over the bin's samples with mask != 0, in channel order
        vis_out = sum of wgt vis over them / wgt_out, exactly 0 where wgt_out == 0
        mask_out = any(mask) as 0 / 1 bytes
    and wsum the fp64 sum of wgt_out over mask_out != 0, one per plane, in wgt's type.  What a masked sample holds is
    never read into a sum.  vis complex64 or complex128, wgt its real type; the products wgt vis are formed in that type,
    the sums in fp64, in a fixed order: the same bits every run.  numpy in gives numpy out, tensors in give tensors
    out."""
    n = check_chan_average(n)
    vd, wd = _dev.to_dev(vis), _dev.to_dev(wgt)
    if vd.dtype not in _dev.REAL_OF or vd.ndim not in (2, 3):
        raise TypeError("vis must be complex64 or complex128 of shape (nrow, nchan) or (nprod, nrow, nchan)")
    if wd.dtype != _dev.REAL_OF[vd.dtype] or wd.shape != vd.shape:
        raise TypeError(f"wgt must be {_dev.REAL_OF[vd.dtype]} of vis' shape {tuple(vd.shape)}, got {wd.dtype} "
                        f"{tuple(wd.shape)}")
    if vd.ndim == 3 and not 1 <= vd.shape[0] <= 4:
        raise ValueError(f"1 to 4 product planes in one call, got {vd.shape[0]}")
    md = _dev.byte_mask(mask, tuple(vd.shape[-2:]))
    viso, wgto, masko, rec = _average_dev(vd, wd, md, n)
    return tuple(_dev.host_like(t, vis) for t in (viso, wgto, masko, rec.to(wd.dtype)))


def average_freq(freq, chan_width, n):
    """(freq_out, chan_width_out) of the bins of n channels, float64 numpy arrays of ceil(nchan / n) entries: the mean of
    a bin's frequencies and the sum of its widths.  Metadata of nchan entries: formed on the host in fp64."""
    n = check_chan_average(n)
    host = []
    for a in (freq, chan_width):
        a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        host.append(a.astype(np.float64))
    f, w = host
    if f.ndim != 1 or f.shape != w.shape:
        raise ValueError("freq and chan_width must be one-dimensional, of one length")
    starts = np.arange(0, f.size, n)
    if f.size == 0:
        return f.copy(), w.copy()
    counts = np.minimum(starts + n, f.size) - starts
    return np.add.reduceat(f, starts) / counts, np.add.reduceat(w, starts)
