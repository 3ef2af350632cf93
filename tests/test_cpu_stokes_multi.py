"""
The product argument of utils.stokes (no GPU): which `product` values mean one product and which a stack, the basis
list a stacked call hands to pfb_stokes_vis_multi, and the values that are refused.
"""
import pytest

from pfb_clean_amd.utils import stokes as st

LETTERS = 'IQUV'


def test_a_single_letter_is_one_product():
    for pol in ('linear', 'circular'):
        for p in LETTERS:
            assert st.product_letters(p) is None
            assert st.basis_list(pol, p) == st.BASIS_INDEX[(pol, p)] == st.basis_index(pol, p)
            assert isinstance(st.basis_list(pol, p), int)


def test_basis_lists_of_both_polarisations():
    assert st.basis_list('linear', 'IQUV') == [0, 1, 2, 3]
    assert st.basis_list('circular', 'IQUV') == [0, 2, 3, 1]
    assert st.basis_list('circular', 'VQ') == [1, 2]


@pytest.mark.parametrize('product', ['IQUV', 'QU', 'VI', 'UVQI', ('U', 'I', 'Q'), ['V', 'I'], ['Q'], ('I',), 'VUQ'],
                         ids=str)
def test_the_order_asked_is_kept(product):
    letters = tuple(product)
    assert st.product_letters(product) == letters
    for pol in ('linear', 'circular'):
        got = st.basis_list(pol, product)
        assert isinstance(got, list) and got == [st.BASIS_INDEX[(pol, p)] for p in letters]
        assert len(set(got)) == len(got) and all(0 <= b <= 3 for b in got)


@pytest.mark.parametrize('product', ['II', 'IX', '', 'IQUVI', 'QUQ', ('I', 'I'), ('IQ', 'U'), (), ['I', 'Q', 'U', 'V', 'I'],
                                     'iq', 5, None, ('I', 3)], ids=repr)
def test_value_errors(product):
    with pytest.raises(ValueError):
        st.basis_list('linear', product)


def test_an_unknown_polarisation_is_refused_for_stacks_too():
    with pytest.raises(ValueError):
        st.basis_list('elliptic', 'IQ')
    with pytest.raises(ValueError):
        st.basis_list('elliptic', 'I')


def test_the_native_signature_is_declared():
    """_lib declares every new entry point; the multi Stokes entry takes (nprod, basis) where the single takes basis."""
    from pfb_clean_amd import _lib
    single, multi = _lib.SIGNATURES['pfb_stokes_vis'][1], _lib.SIGNATURES['pfb_stokes_vis_multi'][1]
    assert len(multi) == len(single) + 1 and multi[:2] == single[:2] and multi[4:] == single[3:]
    for name in ('prep', 'finish', 'grid', 'degrid', 'image_forward', 'image_adjoint', 'image_correct'):
        assert f'pfb_wgrid_{name}_multi' in _lib.SIGNATURES
