"""CPU checks of the attention-map overlays (sbagan/visualize.py): the expand operator against scipy, the declared and
bound entry points, the command-line flag in all four entry points, the top-k order, the wrappers' refusal of CPU
tensors."""

import numpy as np
import pytest
import torch

import vis_ref


@pytest.mark.parametrize('a,up', [(1, 16), (3, 2), (5, 4), (17, 16), (64, 2), (64, 4), (128, 2)])
def test_expand_operator_against_scipy(a, up):
    """M x M^T equals zoom + gaussian_filter within 1e-12; (5, 4) and (1, 16) reflect more than once (80 > V)"""
    from sbagan.visualize import expand_operator
    M = expand_operator(a, up)
    assert M.shape == (a * up, a) and M.dtype == np.float64
    assert M.min() >= 0.0 and np.abs(M.sum(1) - 1.0).max() < 1e-12
    x = np.random.RandomState(a * 100 + up).randn(a, a)
    err = np.abs(M @ x @ M.T - vis_ref.expand(x, up)).max()
    print('a %d up %d: max |M x M^T - scipy| = %.3e' % (a, up, err))
    assert err <= 1e-12
    assert expand_operator(a, up) is M and not M.flags.writeable          # cached, read-only


def test_expand_operator_up_1_is_the_identity():
    from sbagan.visualize import expand_operator
    for up in (0, 1):
        assert np.array_equal(expand_operator(7, up), np.eye(7))


def test_header_declares_and_lib_binds_both_entry_points():
    from sbagan import _lib
    for name, nargs in (('sba_vis_expand', 11), ('sba_vis_compose', 20)):
        assert name in _lib.DECLS and _lib.DECLS[name].ret == 'int', name
        assert len(_lib.DECLS[name].params) == nargs == len(_lib.SIGNATURES[name])
        assert getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name]


def test_flag_parses_in_all_four_entry_points_and_defaults_to_off():
    import main
    import main_bert
    import pretrain_DAMSM
    import pretrain_DAMSM_bert
    for mod in (main, main_bert, pretrain_DAMSM, pretrain_DAMSM_bert):
        assert mod.parse_args([]).attention_maps is False, mod.__name__
        assert mod.parse_args(['--attention_maps']).attention_maps is True, mod.__name__
    import trainer
    import trainer_bert
    assert trainer.condGANTrainer.attention_maps is False and trainer_bert.condGANTrainer.attention_maps is False


def test_topk_order_with_ties_at_zero():
    from sbagan.visualize import topk_order
    conf = np.array([0.0, 0.3, 0.0, 0.3, 0.0, 0.1, 0.0])
    assert topk_order(conf).tolist() == [3, 1, 5, 6, 4]                   # ties: the higher index first
    assert topk_order(np.zeros(3)).tolist() == [2, 1, 0]
    assert topk_order(conf).tolist() == np.argsort(conf, kind='stable')[::-1][:5].tolist()
    assert vis_ref.topk(np.zeros((3, 4, 4)), np.zeros((3, 2, 2)), 2, 3)[1].tolist() == [2, 1, 0]


def test_word_colours_are_distinct():
    from sbagan.visualize import word_colours
    cols = word_colours(20)
    assert len(set(cols)) == 20 and all(0 <= v <= 255 for c in cols for v in c) and (0, 0, 0) not in cols


def test_wrappers_refuse_cpu_tensors():
    from sbagan import ops
    with pytest.raises(RuntimeError):
        ops.vis_expand(torch.zeros(2, 4, 4))
    with pytest.raises(RuntimeError):
        ops.vis_compose(4, 50, np.zeros((1, 1, 1, 4), np.int32), np.zeros((1, 1, 1, 2), np.float32),
                        np.zeros((1, 1), np.uint32), torch.zeros(1, 4, 4))

