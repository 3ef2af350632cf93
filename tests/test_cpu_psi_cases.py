"""
The case table of tests/test_gpu_psi_edges.py (tests/psi_cases.py), checked on the CPU:

  * every case has the property it exists for (its predicate over the bookkeeping and the mirrored tile constants), per
    number format where the property is per format, and the XCD cases cover every kernel family, format and grid kind;
  * the bookkeeping of an odd size equals that of the size rounded up -- what the odd-size reference rests on;
  * the references of psi_cases are oracle.wavelets.Psi's own results wherever that can run, and the oracle round trip
    hdot(dot(x)) == nbasis * x holds to 1e-12 on every even-sized case: the oracle handles the tiny and the deepest shapes
    before anything is blamed on the GPU.
"""
import numpy as np
import pytest

from oracle import wavelets as owv

import psi_cases as pc

pmp = pytest.mark.parametrize
ids = [c.id for c in pc.CASES]


def test_table_is_well_formed():
    assert len(set(ids)) == len(ids)
    assert {c.group for c in pc.CASES} == set('abcdefgh')
    for c in pc.CASES:
        assert max(c.nx, c.ny) <= 272 and 1 <= c.nband <= 5 and 1 <= c.nlevel <= pc.MAXLEV, c
    assert all(pc.by_id(i) in pc.RUN_CASES for i in pc.STANDALONE)
    # the refused ones are exactly the 2-level db5 cases below 36 pixels, and each has a 2-level stand-in that runs
    assert sorted(c.id for c in pc.REFUSED_CASES) == ['g-31x45-L2', 'g-33x64-L2', 'g-64x33-L2']
    for c in pc.REFUSED_CASES:
        assert not pc.by_id(c.id.replace('-L2', '-db3-L2')).refused


@pmp('case', pc.CASES, ids=ids)
def test_case_has_its_property(case):
    holds = {d: case.holds(d) for d in pc.DTYPES}
    if case.need == 'both':
        assert all(holds.values()), (case, holds)
    elif case.need == 'any':
        assert any(holds.values()), (case, holds)
    else:
        assert holds[case.need], (case, holds)


def test_xcd_cases_cover_every_family_format_and_kind():
    seen = set()
    for c in pc.CASES:
        if c.group != 'f':
            continue
        for (d, fam, lev), (total, kind) in c.prop.expect.items():
            g = pc.family_grid(c, d, fam, lev)
            assert g[0] * g[1] * g[2] == total and pc.grid_kind(g) == kind, (c, d, fam, lev, g)
            if kind == 'tail':
                assert total > 64 and total % 64 and g[0] % 8
            seen.add((d, fam, kind))
    want = {(d, fam, kind) for d in pc.DTYPES for fam in pc.FAMILIES for kind in ('lt64', 'mult64', 'tail')}
    assert want <= seen, sorted(want - seen)


def test_tile_remainder_cases_cover_every_remainder():
    """Group (a) reaches C % TA = 0, 1 and TA - 1, and C < TA, on both axes in both formats."""
    for d in pc.DTYPES:
        for axis in ('sx', 'sy'):
            rem = {getattr(c.bk(c.wavelets[0]), axis)[0] % pc.TA[d] for c in pc.CASES if c.group == 'a'}
            assert {0, 1, pc.TA[d] - 1} <= rem, (d, axis, rem)
            assert any(getattr(c.bk(c.wavelets[0]), axis)[0] < pc.TA[d] for c in pc.CASES if c.group == 'a')


def test_deep_cases_reach_the_smallest_levels():
    cs = {c for cc in pc.CASES if cc.group == 'c' for c in cc.bk(cc.wavelets[0]).sx + cc.bk(cc.wavelets[0]).sy}
    assert {1, 2, 4} <= cs


def test_odd_size_bookkeeping_equals_that_of_the_next_even_size():
    for F in range(2, 20, 2):
        for nlevel in (1, 2, 3):
            for n in range(1, 200, 2):
                a, b = owv.Bookkeeping(n, n, F, nlevel), owv.Bookkeeping(n + 1, n + 1, F, nlevel)
                assert (a.sx, a.Ntotx, a.ix, a.spx[1:]) == (b.sx, b.Ntotx, b.ix, b.spx[1:]), (F, nlevel, n)
                assert (a.sy, a.Ntoty, a.iy, a.spy[1:]) == (b.sy, b.Ntoty, b.iy, b.spy[1:]), (F, nlevel, n)
                assert a.spx[0] == n + 1            # the finest synthesis writes n + 1 pixels, of which n are kept


@pmp('case', pc.REFUSED_CASES, ids=[c.id for c in pc.REFUSED_CASES])
def test_oracle_refuses_the_level_count_too(case):
    for n in (min(case.nx, case.ny), min(case.nx, case.ny) + 1):
        with pytest.raises(ValueError):
            owv.Psi(case.nband, n, n, list(case.bases), case.nlevel, 1)


@pmp('case', pc.RUN_CASES, ids=[c.id for c in pc.RUN_CASES])
def test_reference_and_oracle_round_trip(case):
    x, a_ref, c, xo_ref = pc.reference(case)
    assert a_ref.shape == (case.nband, len(case.bases)) + case.plane()
    written = ~np.isnan(a_ref)
    assert written.any() and np.array_equal(written, np.broadcast_to(written[:1], written.shape))
    if case.wavelets and not case.odd:
        # the references are oracle.wavelets.Psi's own numbers
        po = owv.Psi(case.nband, case.nx, case.ny, list(case.bases), case.nlevel, 1)
        assert (po.Nymax, po.Nxmax) == case.plane()
        a = np.full(a_ref.shape, np.nan)
        po.dot(x, a)
        assert np.array_equal(a, a_ref, equal_nan=True)
        xo = np.full(xo_ref.shape, np.nan)
        po.hdot(c, xo)
        assert np.array_equal(xo, xo_ref)
    # round trip, odd sizes included (zero extension: the padded round trip reproduces the image); margins hold 1e3 and
    # are never read
    back = pc.oracle_hdot(case, np.where(written, a_ref, 1e3))
    assert np.abs(back - len(case.bases) * x).max() < 1e-12
    # adjointness of the references themselves (odd sizes included): <dot x, c>_written == <x, hdot c_written>
    cw = np.where(written, c, 0.0)
    lhs = np.sum(np.where(written, a_ref, 0.0) * cw)
    rhs = np.sum(x * pc.oracle_hdot(case, cw))
    assert abs(lhs - rhs) <= 1e-12 * np.linalg.norm(a_ref[written]) * np.linalg.norm(cw)
