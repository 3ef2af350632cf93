"""
The embed chooser over the three length families of the fast convolution path (operators/psf.py::_embed_grid): per axis
the smallest length among the powers of two and the OFFERED 3 2^k / 5 2^k lengths (MIX_OFFERED).  No GPU: the chooser is plain Python.

Offered are the lengths that measured faster per plan.apply than the power-of-two grid the problem had before, by more
than the run-to-run spread (profiles/mixed_conv_sweep.md, MI355X): fp32 ROWS of 5120 and 6144 pixels on power-of-two
columns (8192 x 6144 0.90, 8192 x 5120 0.89, 4096 x 6144 0.91 of the time on 8192 / 4096 x 8192).  No column length is
offered: 5120 x 8192 took 1.08 x the time of 8192^2 and 6144 x 4096 1.15 x that of 8192 x 4096 (the plain column kernel
loses to the persistent ones), 3072^2 fp32 1.09 x the time of 4096^2, 1536^2 fp64 1.02 x that of 2048^2; the shorter
lengths and the other fp64 lengths were not timed.  So with the shipped chooser (6000, 6000) -> (8192, 6144),
(5040, 3000) -> (8192, 4096), an image of 96 x 192 or 160 x 320 is embedded in a power of two as before, (80, 160) ->
(128, 256), and the 4/3 n bound holds on fp32 rows of 4097 .. 6144 pixels only.  The chooser LOGIC over all three families -- the values a
fully offered chooser gives, (5040, 3000) -> (5120, 3072), (96, 192) -> None, (80, 160) -> (96, 160), at most 4/3 n
from 128 on -- is tested with every class the library takes offered (`full`).
"""
import pytest
import torch

from pfb_clean_amd.operators import psf
from pfb_clean_amd.operators.psf import _embed_grid

F32, F64 = torch.float32, torch.float64


@pytest.fixture
def full(monkeypatch):
    """Every class the library takes is offered."""
    monkeypatch.setattr(psf, 'MIX_OFFERED', {ax: {dt: tuple(psf._mix_lengths(*rng)) for dt, rng in per.items()}
                                             for ax, per in psf.MIX_ALL.items()})


def grid2x(nx, ny, rdt=F32):
    return _embed_grid(nx, ny, 2 * nx, 2 * ny, rdt)


def in_family(n):
    while n % 2 == 0:
        n //= 2
    return n in (1, 3, 5)


# ------------------------------------------------------------------------------------------------ the shipped chooser
@pytest.mark.parametrize('nx,ny,rdt,want', [
    (6000, 6000, F32, (8192, 6144)),     # rows 6144, columns the next power of two: 0.90 of the time on 8192^2
    (5040, 5040, F32, (8192, 5120)),
    (4100, 6000, F32, (8192, 6144)),
    (4000, 6000, F32, (4096, 6144)),
    (4096, 6144, F32, None),             # offered and exact: nothing to embed
    (4100, 7200, F32, (8192, 8192)),     # 5120 x 8192 measured 8 % slower than 8192^2
    (6000, 4000, F32, (8192, 4096)),     # 6144 x 4096 measured 15 % slower than 8192 x 4096
    (5040, 3000, F32, (8192, 4096)),     # 3072 is not offered: 3072^2 measured 9 % slower than 4096^2
    (3000, 3000, F32, (4096, 4096)),
    (3072, 3072, F32, (4096, 4096)),     # a class of its own, embedded as before
    (1500, 1500, F64, (2048, 2048)),     # 1536^2 fp64 measured 2 % slower than 2048^2
    (6000, 6000, F64, (8192, 8192)),     # fp64 5120 / 6144: not timed
    (6144, 6144, F32, (8192, 6144)),     # a class of its own; its column length is not offered
    (96, 192, F32, (128, 256)),          # the short classes: not timed
    (160, 320, F32, (256, 512)),
    (80, 160, F32, (128, 256)),
])
def test_shipped_chooser_values(nx, ny, rdt, want):
    assert grid2x(nx, ny, rdt) == want


@pytest.mark.parametrize('rdt', [F32, F64])
def test_shipped_chooser_lengths(rdt):
    """Each axis on its own: the chosen length holds n and is a power of two or an offered length; on fp32 ROWS of
    4097 .. 6144 pixels -- where the offered lengths lie -- it is at most 5/4 n, elsewhere the next power of two, as
    before."""
    for n in range(1, 8193):
        gx = _embed_grid(n, 1024, 12000, 2048, rdt)          # nx_psf > LINE_MAX: the 3 x pixel rule does not apply
        gy = _embed_grid(1024, n, 12000, 2 * n + 2 * (n % 2), rdt)
        for got, lo, rows in ((gx[0], 64, False), (gy[1], 128, True)):
            pow2 = max(lo, 1 << (n - 1).bit_length())
            if rows and rdt == F32 and 4096 < n <= 6144:
                assert got == (5120 if n <= 5120 else 6144) and 4 * got <= 5 * n + 4
            else:
                assert got == pow2, (n, got)


# -------------------------------------------------------------------------- the chooser with every class offered
@pytest.mark.parametrize('nx,ny,want', [
    (6000, 6000, (6144, 6144)),
    (5040, 3000, (5120, 3072)),
    (4100, 7200, (5120, 8192)),
    (96, 192, None),               # a class of its own on both axes: nothing to embed
    (160, 320, None),
    (80, 160, (96, 160)),          # nx = 80 is no class (the row tiles of 32 rows do not divide it); ny = 160 is
])
def test_chooser_values(full, nx, ny, want):
    assert grid2x(nx, ny) == want


def test_fp64_rows_stop_at_the_fp64_limit(full):
    assert grid2x(7000, 7000, F64) == (8192, 8192)          # not 10240: fp64 rows end at 8192 pixels
    assert grid2x(7000, 9000, F64) is None
    assert grid2x(7000, 9000, F32) == (8192, 10240)


@pytest.mark.parametrize('rdt', [F32, F64])
@pytest.mark.parametrize('problem,want', [
    ((100, 120, 200, 240), (128, 128)),
    ((100, 120, 150, 180), (128, 128)),
    ((250, 78, 500, 156), (256, 128)),
    ((64, 64, 128, 128), (64, 128)),
    ((48, 40, 96, 80), None),            # the coverage kernels: embedding costs more than 3 x the pixels
    ((24, 20, 48, 40), None),
    ((33, 31, 66, 62), None),
    ((33, 31, 66, 64), None),
    ((9000, 24, 18000, 48), None),       # beyond the fast path: the long-line path
])
def test_pinned_plans_keep_their_grid(problem, want, rdt, monkeypatch):
    assert _embed_grid(*problem, rdt) == want
    monkeypatch.setattr(psf, 'MIX_OFFERED', {ax: {dt: tuple(psf._mix_lengths(*rng)) for dt, rng in per.items()}
                                             for ax, per in psf.MIX_ALL.items()})
    assert _embed_grid(*problem, rdt) == want


def test_switches_and_odd_psf_rows(monkeypatch):
    assert _embed_grid(100, 150, 200, 301, F64) is None
    for var in ('PFB_NO_EMBED', 'PFB_FORCE_GENERIC'):
        monkeypatch.setenv(var, '1')
        assert grid2x(6000, 6000) is None
        monkeypatch.delenv(var)
    assert grid2x(6000, 6000) == (8192, 6144)


@pytest.mark.parametrize('rdt', [F32, F64])
def test_every_length_is_held_by_a_family_member_at_most_a_third_longer(full, rdt):
    """Each axis on its own (the other one a power of two): for n = 1 .. 8192 the chosen length holds n, is 2^k, 3 2^k or
    5 2^k, and from n = 128 on is at most 4/3 n (four lengths per octave: 4, 5, 6, 8)."""
    for n in range(1, 8193):
        # nx_psf = 12000 > LINE_MAX: the 3 x pixel rule against the coverage kernels does not apply
        gx = _embed_grid(n, 1024, 12000, 2048, rdt)
        gy = _embed_grid(1024, n, 12000, 2 * n + 2 * (n % 2), rdt)
        for got, other in ((gx[0], gx[1]), (gy[1], gy[0])):
            assert other == 1024
            assert got >= n and in_family(got), (n, got)
            if n >= 128:
                assert 3 * got <= 4 * n, (n, got)
        assert gx[0] >= 64 and gy[1] >= 128
