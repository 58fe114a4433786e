"""Precision / recall / density / coverage on the host: the numpy reference (tests/prdc_ref.py) on hand-checked points,
prdc_from_counts against it, the result fields, the command-line flag, the operators' refusal of CPU tensors and the
header / binding agreement.  (The kernels are tested on the GPU in tests/test_prdc_gpu.py.)"""
import ctypes
import json

import numpy as np
import pytest
import torch

import prdc_ref


def on_a_line(xs, D=64, axis=7):
    """points at the positions xs along one axis of a D-dimensional space, every other coordinate 0.5"""
    P = np.full((len(xs), D), 0.5, dtype=np.float32)
    P[:, axis] = xs
    return P


def test_reference_on_hand_checked_points():
    """real at 0, 1, 3 and generated at 0.5, 10 on a line, k = 1.
    Squared radii: real 1, 1, 4 (3's nearest other point is 1); generated 90.25 both (each other's only neighbour).
    0.5 lies in the balls of 0 and 1 (0.25 <= 1) and not of 3 (6.25 > 4); 10 in none: precision 1/2, density 2 / (1 * 2).
    0 lies in the ball of 0.5 only (100 > 90.25), 1 and 3 in both: recall 1.
    The own balls of 0 and 1 hold 0.5, the one of 3 holds nothing (6.25 > 4): coverage 2/3."""
    R, F = on_a_line([0.0, 1.0, 3.0]), on_a_line([0.5, 10.0])
    assert np.array_equal(prdc_ref.dist2(R, F), [[0.25, 100.0], [0.25, 81.0], [6.25, 49.0]])
    assert np.array_equal(prdc_ref.knn_radius(R, 1), [1.0, 1.0, 4.0])
    assert np.array_equal(prdc_ref.knn_radius(R, 2), [9.0, 4.0, 9.0])
    assert np.array_equal(prdc_ref.knn_radius(F, 1), [90.25, 90.25])
    fake_in_real, real_in_fake, real_own = prdc_ref.counts(R, F, 1)
    assert fake_in_real.tolist() == [2, 0] and real_in_fake.tolist() == [1, 2, 2] and real_own.tolist() == [1, 1, 0]
    assert prdc_ref.prdc(R, F, 1) == {'precision': 0.5, 'recall': 1.0, 'density': 1.0, 'coverage': 2.0 / 3.0}


def test_reference_ties_count_and_self_is_excluded_by_index():
    X = on_a_line([0.0, 0.0, 5.0])
    # the twins are each other's neighbour at distance 0; the third point's radius is not 0, as it would be with itself
    assert np.array_equal(prdc_ref.knn_radius(X, 1), [0.0, 0.0, 25.0])
    # a distance equal to the radius is inside the ball
    in_b, in_own = prdc_ref.ball_counts(on_a_line([2.0]), on_a_line([0.0, 4.0, 5.0]), radius_a=[4.0],
                                        radius_b=[4.0, 3.9, 9.0])
    assert in_b.tolist() == [2] and in_own.tolist() == [2]
    in_b, in_own = prdc_ref.ball_counts(X, X, radius_b=[0.0, 0.0, 0.0])
    assert in_own is None and in_b.tolist() == [2, 2, 1]


def test_prdc_from_counts_against_the_reference():
    from sbagan.prdc import FIELDS, prdc_from_counts
    assert sorted(FIELDS) == ['coverage', 'density', 'dtype', 'k', 'n_fake', 'n_real', 'precision', 'recall']
    rng = np.random.RandomState(3)
    for nr, nf, k in ((40, 30, 1), (60, 80, 5), (9, 9, 8)):
        R = rng.randn(nr, 64).astype(np.float32)
        F = (0.9 * rng.randn(nf, 64) + 0.15).astype(np.float32)
        counts = prdc_ref.counts(R, F, k)
        res = prdc_from_counts(*counts, k=k, dtype='bfloat16')
        want = prdc_ref.prdc(R, F, k)
        assert sorted(res) == sorted(FIELDS)
        for key, value in want.items():
            assert res[key] == value, key
        assert (res['k'], res['n_real'], res['n_fake'], res['dtype']) == (k, nr, nf, 'bfloat16')
        assert json.loads(json.dumps(res)) == res               # plain Python numbers and strings only
        # int32 device counts give the same figures
        assert prdc_from_counts(*(c.astype(np.int32) for c in counts), k=k, dtype='bfloat16') == res
    res = prdc_from_counts([2, 0], [1, 2, 2], [1, 1, 0], 1)
    assert (res['precision'], res['recall'], res['density'], res['coverage']) == (0.5, 1.0, 1.0, 2.0 / 3.0)
    with pytest.raises(ValueError):
        prdc_from_counts([1, 2], [1, 2, 3], [1, 2], 1)          # real_in_fake and real_own differ in length
    with pytest.raises(ValueError):
        prdc_from_counts([], [1], [1], 1)
    with pytest.raises(ValueError):
        prdc_from_counts([1], [1], [1], 0)


def test_prdc_class_arguments_and_too_few_rows():
    from sbagan.prdc import PRDC
    for bad in (dict(D=100), dict(k=0), dict(k=9), dict(k=2.0), dict(capacity=0)):
        with pytest.raises(ValueError):
            PRDC(None, **bad)
    ev = PRDC(None, D=64, k=3, dtype='float32')
    assert ev.count('real') == 0 and ev.count('fake') == 0 and ev.dtype == 'float32'
    with pytest.raises(RuntimeError, match='real side holds 0 rows'):
        ev.result()
    with pytest.raises(ValueError):
        ev.count('both')
    with pytest.raises(RuntimeError):                           # CPU rows are refused
        ev.update_features('real', torch.zeros(4, 64))
    with pytest.raises(ValueError):
        ev.update_features('real', torch.zeros(4, 32))


def test_prdc_flag_in_all_four_entry_points(capsys):
    import main
    import main_bert
    import pretrain_DAMSM
    import pretrain_DAMSM_bert
    for mod in (main, main_bert, pretrain_DAMSM, pretrain_DAMSM_bert):
        assert mod.parse_args([]).prdc == 0
        for k in range(0, 9):
            assert mod.parse_args(['--prdc', str(k)]).prdc == k
        for bad in ('9', '-1', 'five'):
            with pytest.raises(SystemExit):
                mod.parse_args(['--prdc', bad])
    capsys.readouterr()
    from trainer import condGANTrainer
    import trainer_bert
    for cls in (condGANTrainer, trainer_bert.condGANTrainer):
        assert cls.prdc == 0 and cls.prdc_result is None


def test_prdc_operators_refuse_cpu_tensors():
    from sbagan import ops
    x, r = torch.zeros(8, 64), torch.zeros(8, dtype=torch.float64)
    with pytest.raises(RuntimeError):
        ops.prdc_knn_radius(x, 2)
    with pytest.raises(RuntimeError):
        ops.prdc_ball_counts(x, x, radius_a=r)
    with pytest.raises(RuntimeError):
        ops.prdc_ball_counts(x, x, radius_b=r, splits=2)
    with pytest.raises(TypeError):
        ops.prdc_knn_radius([[0.0] * 64] * 8, 2)


def test_header_declares_what_the_binding_binds():
    from sbagan import _lib
    decls = {name: (d.ret, ['%s %s' % (ctext, arg) for ctext, arg, _ in d.params])
             for name, d in _lib.DECLS.items() if name.startswith('sba_prdc_')}
    assert sorted(decls) == ['sba_prdc_ball_counts', 'sba_prdc_knn_radius', 'sba_prdc_workspace_bytes']
    for name in ('sba_prdc_knn_radius', 'sba_prdc_ball_counts'):
        ret, args = decls[name]
        sig = _lib.SIGNATURES[name]
        assert ret == 'int' and len(sig) == len(args)
        for ctype, arg in zip(sig, args):                       # pointers to pointers, ints to ints, int64_t to int64
            want = ctypes.c_void_p if '*' in arg else ctypes.c_int64 if 'int64_t' in arg else ctypes.c_int
            assert ctype is want, (name, arg)
        assert getattr(_lib.lib, name).restype is ctypes.c_int
    ret, args = decls['sba_prdc_workspace_bytes']
    size = _lib.lib.sba_prdc_workspace_bytes
    assert ret == 'int64_t' and size.restype is ctypes.c_int64 and list(size.argtypes) == [ctypes.c_int] * len(args)
    # the size needs no device: nothing for one part, 8 f64 per row and part otherwise, parts capped at the tiles
    assert size(100, 100, 1) == 0 and size(100, 100, 2) == 2 * 100 * 64 and size(100, 100, 7) == 2 * 100 * 64
    assert size(3000, 3000, 0) == 11 * 3000 * 64 and size(30000, 30000, 0) == 2 * 30000 * 64
    assert size(0, 5, 1) == -1 and size(5, 5, 33) == -1
