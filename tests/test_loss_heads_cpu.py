"""The head tables of the discriminator / generator loss terms (miscc.losses.d_term_heads, g_term_heads) and the
store-or-accumulate bookkeeping of ops.DHeadsFn.backward (ops._row_modes): pure host code, no device."""
import pytest


def test_head_tables_are_the_reference_terms():
    """row0, rows, cond_row0, target, weight, segment -- written out as they stood in discriminator_loss and _g_term before
    the tables became functions: errD = (real + cond_real)/2 + (fake + cond_fake + cond_wrong)/3 (losses.py:141-158)"""
    from miscc.losses import d_term_heads, g_term_heads
    n = 3
    assert tuple(tuple(h) for h in d_term_heads(n, True)) == (
        (0, n, 0, 1., .5, 1), (n, n, 0, 0., 1. / 3, 3), (0, n - 1, 1, 0., 1. / 3, 4),
        (0, n, None, 1., .5, 0), (n, n, None, 0., 1. / 3, 2))
    assert tuple(tuple(h) for h in d_term_heads(n, False)) == (
        (0, n, 0, 1., 1., 0), (n, n, 0, 0., .5, 1), (0, n - 1, 1, 0., .5, 2))
    assert tuple(tuple(h) for h in g_term_heads(n, True)) == ((0, n, 0, 1., 1., 1), (0, n, None, 1., 1., 0))
    assert tuple(tuple(h) for h in g_term_heads(n, False)) == ((0, n, 0, 1., 1., 0),)
    h = d_term_heads(n, True)[2]
    assert (h.row0, h.rows, h.cond_row0, h.target, h.weight, h.segment) == (0, 2, 1, 0., 1. / 3, 4)


def test_row_modes_of_the_discriminator_tables():
    from miscc.losses import d_term_heads
    from sbagan.ops import _row_modes
    n = 3
    # every head writes at its own place in the issue order (conditional heads in groups of one)
    assert _row_modes(d_term_heads(n, True), 2 * n) == ([0, 1, 3, 4, 2], {0: 0, 1: 0, 3: 1, 4: 1, 2: 1})
    assert _row_modes(d_term_heads(n, False), 2 * n) == ([0, 1, 2], {0: 0, 1: 0, 2: 1})
    # the three conditional heads as one group write behind the last of them (one data-gradient launch): the
    # unconditional heads, issued before that, then store
    assert _row_modes(d_term_heads(n, True), 2 * n, [[0, 1, 2]]) == ([0, 1, 3, 4, 2], {3: 0, 4: 0, 0: 1, 1: 1, 2: 1})
    assert _row_modes(d_term_heads(n, False), 2 * n, [[0, 1, 2]]) == ([0, 1, 2], {0: 0, 1: 0, 2: 1})
    # plain tuples are accepted
    assert _row_modes(((0, 4, None, 1., 1., 0),), 4) == ([0], {0: 0})


def test_row_modes_refuses_bad_tables():
    from sbagan.ops import Head, _row_modes
    with pytest.raises(AssertionError, match='partially overlapping head rows'):
        _row_modes((Head(0, 3, None, 1., 1., 0), Head(2, 3, None, 1., 1., 1)), 5)
    with pytest.raises(AssertionError, match='rows without a head'):
        _row_modes((Head(0, 3, None, 1., 1., 0),), 4)
    with pytest.raises(AssertionError, match='rows without a head'):
        _row_modes((Head(0, 2, None, 1., 1., 0), Head(3, 1, None, 1., 1., 1)), 4)


def test_discriminator_loss_refuses_real_and_fake_of_different_shape():
    """(the reference fails on them as well, at COND_DNET(fake_features, conditions); no trunk pass is made)"""
    import torch
    from miscc.losses import discriminator_loss
    real, fake = torch.zeros(3, 3, 8, 8), torch.zeros(2, 3, 8, 8)
    with pytest.raises(ValueError) as e:
        discriminator_loss(None, real, fake, torch.zeros(3, 4), None, None)
    assert '(3, 3, 8, 8)' in str(e.value) and '(2, 3, 8, 8)' in str(e.value)
