"""
Channel averaging on the MI355X (csrc/stokes.hip: k_chan_average and k_chan_average_lane behind
stokes_vis(..., chan_average=n) and average_channels) against the fp64 oracle of tests/chanavg_cases.py, in
fp32 and fp64.

Bounds, per element (chanavg_cases.py states them): for stokes_vis(chan_average=n)
    |wgt - W| <= eps [K sum Wu_i + (m - 1) W]
    |vis - R| <= eps [(K sum (w_i U_i + Wu_i |v_i|) + m S) / W + |R| ((K sum Wu_i + (m - 1) W) / W + 2)]
and the same with K = 0 for average_channels on inputs that are exact in the type; an element whose bound is zero is
exact; mask exactly the oracle's; wsum within stokes_cases.wsum_bound.  Every figure is printed before it is asserted.
"""
import numpy as np
import pytest
import torch

import chanavg_cases as ca
import stokes_cases as sc

pytestmark = pytest.mark.gpu

TAGS = ('f32', 'f64')


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check(c, got, tag, ref=None, label='oracle'):
    """(vis, wgt, mask, wsum) against the case's oracle (or `ref`, a dict in its form) at the bounds."""
    o = ca.oracle(c) if ref is None else ref
    vis, wgt, mask, wsum = got
    assert all(isinstance(a, np.ndarray) for a in got)
    assert vis.dtype == sc.CDT[tag] and wgt.dtype == sc.RDT[tag] and mask.dtype == np.uint8 and wsum.dtype == sc.RDT[tag]
    assert vis.shape == o['vis'].shape and wgt.shape == o['wgt'].shape and mask.shape == o['mask'].shape
    ev, ew = ca.worst(vis, o['vis'], o['vis_unit'], tag), ca.worst(wgt, o['wgt'], o['wgt_unit'], tag)
    print(f"{c['name']} {tag} vs {label}: vis {ev:.3f}, wgt {ew:.3f} of the bound")
    assert np.isfinite(vis).all() and np.isfinite(wgt).all()
    assert ev <= 1 and ew <= 1, (ev, ew)
    assert np.array_equal(mask, o['mask'])
    planes = list(zip(wsum, o['wgt'])) if o['wgt'].ndim == 3 else [(wsum[0], o['wgt'])]
    assert wsum.shape == (len(planes),)
    for k, (ws, rw) in enumerate(planes):
        err, bound = ca.wsum_check(ws, rw, o['mask'], tag)
        print(f"    wsum[{k}] off by {err:.3e}, bound {bound:.3e}")
        assert err <= bound
    return ev, ew


def run(c, tag, **over):
    from pfb_clean_amd.utils.stokes import stokes_vis
    return stokes_vis(**ca.sv_args(c, tag, **over), chan_average=c['n'])


# ---------------------------------------------------------------------------------- stokes_vis(chan_average=n)
@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('c', ca.shape_cases(), ids=ca.ids(ca.shape_cases()))
def test_shapes(c, tag):
    check(c, run(c, tag), tag)


@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('c', ca.sweep_cases(), ids=ca.ids(ca.sweep_cases()))
def test_every_mode_and_basis(c, tag):
    check(c, run(c, tag), tag)


@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('c', ca.stack_cases(), ids=ca.ids(ca.stack_cases()))
def test_stacked_products(c, tag):
    got = run(c, tag)
    assert got[0].shape[0] == len(c['product']) and got[2].ndim == 2
    check(c, got, tag)


@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('c', ca.form_cases(), ids=ca.ids(ca.form_cases()))
def test_weight_forms_columns_and_frow(c, tag):
    check(c, run(c, tag), tag)


@pytest.mark.parametrize('tag', TAGS)
def test_tensors_in_give_tensors_out(tag):
    from pfb_clean_amd.utils.stokes import stokes_vis
    c = ca.shape_cases()[11]
    assert c['shape'] == (2, 300, 7)
    a = ca.sv_args(c, tag)
    t = {k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in a.items()}
    got = stokes_vis(**t, chan_average=c['n'])
    assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in got)
    want = run(c, tag)
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))


@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('c', [ca.shape_cases()[1], ca.stack_cases()[2]], ids=['one', 'stacked'])
def test_n_one_is_bit_identical_to_the_plain_call(c, tag):
    from pfb_clean_amd.utils.stokes import stokes_vis
    a = ca.sv_args(c, tag)
    want = stokes_vis(**a)
    got = stokes_vis(**a, chan_average=1)
    assert all(g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('c', [ca.shape_cases()[7], ca.stack_cases()[3], ca.stack_cases()[4]], ids=['rows', 'one-row', 'wide'])
def test_the_call_is_the_pass_then_average_channels(c, tag):
    """stokes_vis(chan_average=n) gives the bits of stokes_vis followed by average_channels."""
    from pfb_clean_amd.utils.stokes import average_channels, stokes_vis
    vis, wgt, mask, _ = stokes_vis(**ca.sv_args(c, tag))
    want = average_channels(vis, wgt, mask, c['n'])
    assert all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(run(c, tag), want))


def test_indices_past_two_to_the_31():
    """(2^20 + 1) rows x 512 channels x 4 correlations of complex64 (17 GB), no Jones terms, weights or flags, Stokes I,
    n = 4: every sample has wgt = 2, so wgt_out = 8 and wsum = 8 nrow 128 exactly, mask = 1, and vis_out is the plain
    mean of four samples: against torch's within 16 eps max|v| (four products and three additions each side)."""
    from pfb_clean_amd.utils.stokes import stokes_vis
    nrow, nchan, n = (1 << 20) + 1, 512, 4
    assert nrow * nchan * 4 > 1 << 31
    data = torch.view_as_complex(torch.randn((nrow, nchan, 4, 2), dtype=torch.float32, device='cuda'))
    ant1 = torch.zeros(nrow, dtype=torch.int32, device='cuda')
    vis, wgt, mask, wsum = stokes_vis(data, ant1, ant1 + 1, np.array([0]), np.array([nrow]), 'linear', 'I', chan_average=n)
    assert vis.shape == wgt.shape == mask.shape == (nrow, nchan // n)
    assert bool((wgt == 8).all()) and bool((mask == 1).all())
    assert float(wsum[0]) == 8.0 * nrow * (nchan // n)
    want = ((data[..., 0] + data[..., 3]) * 0.5).reshape(nrow, nchan // n, n).mean(dim=2)
    del data
    err = float((vis - want).abs().max())
    top = float(want.abs().max())
    print(f"past 2^31: worst |vis - torch's mean| {err:.3e}, 16 eps max|v| = {16 * sc.EPS['f32'] * top:.3e}")
    assert err <= 16 * sc.EPS['f32'] * top
    assert bool((vis[-1] != 0).all())
    del vis, wgt, mask, want
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------- average_channels
@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('c', ca.shape_cases() + ca.stack_cases()[:2], ids=ca.ids(ca.shape_cases() + ca.stack_cases()[:2]))
def test_average_channels_at_the_tight_bound(c, tag):
    """Inputs that are exact in the type: K = 0.  Twice: the same bits."""
    from pfb_clean_amd.utils.stokes import average_channels
    vis, wgt, mask = ca.exact_inputs(c, tag)
    ref = ca.tight(vis, wgt, mask, c['n'])
    got = average_channels(vis, wgt, mask, c['n'])
    check(c, got, tag, ref=ref, label='the fp64 average of its inputs, K = 0')
    again = average_channels(vis, wgt, mask, c['n'])
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    # tensors in, tensors out; a bool mask
    t = average_channels(dev(vis), dev(wgt), dev(mask != 0), c['n'])
    assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in t)
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(t, got))


@pytest.mark.parametrize('tag', TAGS)
def test_average_channels_never_reads_what_the_mask_hides(tag):
    from pfb_clean_amd.utils.stokes import average_channels
    c = ca.shape_cases()[4]
    vis, wgt, mask = ca.exact_inputs(c, tag)
    want = average_channels(vis, wgt, mask, c['n'])
    vis, wgt = vis.copy(), wgt.copy()
    hidden = mask == 0
    assert hidden.any()
    vis[hidden], wgt[hidden] = complex(np.nan, np.inf), -np.inf
    got = average_channels(vis, wgt, mask, c['n'])
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    # n = 1 keeps the live samples within the rounding of w v / w and zeroes the hidden ones
    one = average_channels(vis, wgt, mask, 1)
    assert np.array_equal(one[2], mask) and not one[0][hidden].any() and not one[1][hidden].any()
    assert np.array_equal(one[1][~hidden], wgt[~hidden])
    assert (np.abs(one[0] - np.where(hidden, 0, vis))[~hidden] <= 3 * sc.EPS[tag] * np.abs(vis[~hidden])).all()


# ----------------------------------------------------------------------------------------------------- refusals
def test_value_errors():
    from pfb_clean_amd.utils.stokes import average_channels, stokes_vis
    c = ca.shape_cases()[1]
    a = ca.sv_args(c, 'f32')
    for bad in (0, -3, 2.0, '2', None, True, 1 << 31):
        with pytest.raises(ValueError, match='chan_average'):
            stokes_vis(**a, chan_average=bad)
        with pytest.raises(ValueError, match='chan_average'):
            average_channels(np.zeros((2, 4), np.complex64), np.zeros((2, 4), np.float32), np.ones((2, 4), np.uint8), bad)
    vis, wgt, mask = np.zeros((2, 4), np.complex64), np.zeros((2, 4), np.float32), np.ones((2, 4), np.uint8)
    with pytest.raises(TypeError):
        average_channels(vis, wgt.astype(np.float64), mask, 2)
    with pytest.raises(TypeError):
        average_channels(vis.real.copy(), wgt, mask, 2)
    with pytest.raises(TypeError):
        average_channels(vis, wgt[:, :3].copy(), mask, 2)
    with pytest.raises(ValueError):
        average_channels(vis, wgt, mask[:1], 2)
    with pytest.raises(ValueError):
        average_channels(np.zeros((5, 2, 4), np.complex64), np.zeros((5, 2, 4), np.float32), mask, 2)
    with pytest.raises(ValueError):
        average_channels(vis, wgt, mask.astype(np.int32), 2)


def test_c_abi_refusals():
    """pfb_chan_average itself: the smallest good call answers PFB_OK and what the Python layer gives; with one argument
    changed at a time it answers the status below before any launch -- the pointers real all the same -- and writes
    nothing."""
    from pfb_clean_amd import _lib
    from pfb_clean_amd.utils import stokes as st
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    INV, UNS = _lib.PFB_ERR_INVALID, _lib.PFB_ERR_UNSUPPORTED
    nrow, nchan, n = 2, 3, 2
    src_v = dev(np.arange(1, 1 + 2 * nrow * nchan, dtype=np.float64).view(np.complex128).reshape(nrow, nchan))
    src_w = dev(np.array([[1.0, 2.0, 4.0], [0.5, 0.25, 8.0]]))
    src_m = dev(np.array([[1, 1, 1], [0, 1, 1]], dtype=np.uint8))
    vis = torch.empty((nrow, 2), dtype=torch.complex128, device='cuda')
    wgt = torch.empty((nrow, 2), dtype=torch.float64, device='cuda')
    mask = torch.empty((nrow, 2), dtype=torch.uint8, device='cuda')
    wsum = torch.empty(1, dtype=torch.float64, device='cuda')
    work = torch.zeros(_lib.REDUCE_WS_DOUBLES, dtype=torch.float64, device='cuda')
    names = 'dtype nprod vis wgt mask nrow nchan chan_average viso wgto masko wsum work'.split()
    good = dict(zip(names, [_lib.PFB_F64, 1, src_v.data_ptr(), src_w.data_ptr(), src_m.data_ptr(), nrow, nchan, n,
                            vis.data_ptr(), wgt.data_ptr(), mask.data_ptr(), wsum.data_ptr(), work.data_ptr()]))
    assert len(good) == len(names) == 13

    def call(**over):
        return lib.pfb_chan_average(*dict(good, **over).values(), stream)

    assert call() == _lib.PFB_OK
    want = st.average_channels(src_v, src_w, src_m, n)
    assert torch.equal(vis, want[0]) and torch.equal(wgt, want[1]) and torch.equal(mask, want[2])
    assert wgt.cpu().tolist() == [[3.0, 4.0], [0.25, 8.0]] and mask.cpu().tolist() == [[1, 1], [1, 1]]
    assert float(wsum[0]) == float(want[3][0]) == 15.25
    assert vis.cpu().tolist() == [[(1 * (1 + 2j) + 2 * (3 + 4j)) / 3, 5 + 6j], [9 + 10j, 11 + 12j]]

    vis.fill_(-7 - 7j), wgt.fill_(-7.0), mask.fill_(0xAB), wsum.fill_(-7.0)
    refused = [dict(chan_average=0), dict(chan_average=-2), dict(nprod=0), dict(nprod=5), dict(dtype=3)]
    refused += [{name: None} for name in ('vis', 'wgt', 'mask', 'viso', 'wgto', 'masko', 'wsum', 'work')]
    refused += [{name: good[name] + off} for name, off in (('vis', 8), ('wgt', 4), ('viso', 8), ('wgto', 4), ('wsum', 4))]
    for over in refused:
        assert call(**over) == INV, over
    for over in (dict(nrow=0), dict(nchan=0), dict(nrow=1 << 31)):
        assert call(**over) == UNS, over
    torch.cuda.synchronize()
    assert (vis == -7 - 7j).all() and (wgt == -7.0).all() and (mask == 0xAB).all() and (wsum == -7.0).all()
