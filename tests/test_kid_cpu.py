"""Kernel Inception Distance on the host: the numpy reference (tests/kid_ref.py) on the hand-checked case, kid_from_sums
against it, the result fields, the command-line flags, the subset draws, the operator's refusal of CPU tensors and
out-of-range indices, and the header / binding agreement.  (The kernel is tested on the GPU in tests/test_kid_gpu.py.)"""
import ctypes
import json
import random

import numpy as np
import pytest
import torch

import kid_ref


def test_reference_on_the_hand_checked_case():
    """D = 64, a = 8 e0, X = {a, 0}, Y = {a, 2a}: k(a, 0) = 1, k(a, a) = (64 / 64 + 1)^3 = 8, k(a, 2a) = 27, k(2a, 2a) =
    125 and k(0, .) = 1.  Sxx = k(a, 0) + k(0, a) = 2; Syy = 2 k(a, 2a) = 54; Sxy = 8 + 27 + 1 + 1 = 37;
    mmd2 = 2 / 2 + 54 / 2 - 2 * 37 / 4 = 9.5."""
    a = np.zeros(64, dtype=np.float32)
    a[0] = 8.0
    X, Y = np.stack([a, 0 * a]), np.stack([a, 2 * a])
    assert kid_ref.kernel_sum(X, X, exclude_diag=True) == 2.0
    assert kid_ref.kernel_sum(Y, Y, exclude_diag=True) == 54.0
    assert kid_ref.kernel_sum(Y, Y) == 54.0 + 8.0 + 125.0          # with the diagonal: k(a, a) and k(2a, 2a) join
    assert kid_ref.kernel_sum(X, Y) == 37.0
    assert kid_ref.mmd2(X, Y) == 9.5
    from sbagan.kid import kid_from_sums
    res = kid_from_sums([2.0], [54.0], [37.0], 2, D=64)
    assert res['kid'] == 9.5 and res['kid_std'] == 0.0 and res['gamma'] == 1.0 / 64


def test_reference_excludes_by_position_and_masks_bad_indices():
    rng = np.random.RandomState(0)
    X = rng.randint(-3, 4, size=(5, 64)).astype(np.float32)
    # the same row at two positions of a subset: the two positions still pair with each other
    twice = kid_ref.kernel_sum(X, X, [1, 1], [1, 1], exclude_diag=True)
    assert twice == 2.0 * kid_ref.kernel_sum(X[1:2], X[1:2])
    # a row number outside [0, n) is left out with all of its pairs
    assert kid_ref.kernel_sum(X, X, [0, -1, 2, 5], [3, 4]) == kid_ref.kernel_sum(X, X, [0, 2], [3, 4])
    assert kid_ref.kernel_sum(X, X, [0, 5, 2], [0, 1, -1], exclude_diag=True) == (
        kid_ref.kernel_sum(X[[0]], X[[1]]) + kid_ref.kernel_sum(X[[2]], X[[0, 1]]))
    sums = kid_ref.kernel_sums(X, X, [[0, 1], [2, 3]], None)
    assert sums.shape == (2,) and sums[1] == kid_ref.kernel_sum(X[[2, 3]], X)


def test_kid_from_sums_against_the_reference():
    from sbagan.kid import FIELDS, draw_subsets, kid_from_sums
    assert sorted(FIELDS) == ['coef0', 'degree', 'dtype', 'gamma', 'kid', 'kid_std', 'n_fake', 'n_real', 'seed',
                              'subset_size', 'subsets']
    rng = np.random.RandomState(3)
    for nr, nf, m, S, D in ((40, 30, 12, 5, 64), (25, 60, 25, 3, 128), (9, 9, 2, 7, 64)):
        R = np.abs(rng.randn(nr, D)).astype(np.float32)
        F = np.abs(0.9 * rng.randn(nf, D) + 0.2).astype(np.float32)
        ir, jf = draw_subsets(nr, nf, m, S, seed=5)
        sxx = kid_ref.kernel_sums(R, R, ir, ir, exclude_diag=True)
        syy = kid_ref.kernel_sums(F, F, jf, jf, exclude_diag=True)
        sxy = kid_ref.kernel_sums(R, F, ir, jf)
        res = kid_from_sums(sxx, syy, sxy, m, n_real=nr, n_fake=nf, D=D, dtype='bfloat16', seed=5)
        want = kid_ref.kid(R, F, ir, jf)
        assert sorted(res) == sorted(FIELDS)
        # the same formula on the same sums; the mean and the deviation of S numbers may round differently
        assert abs(res['kid'] - want['kid']) <= 1e-12 * abs(want['kid'])
        assert abs(res['kid_std'] - want['kid_std']) <= 1e-9 * abs(want['kid']) + 1e-12 * want['kid_std']
        assert (res['subsets'], res['subset_size'], res['n_real'], res['n_fake']) == (S, m, nr, nf)
        assert (res['degree'], res['coef0'], res['gamma'], res['dtype'], res['seed']) == (3, 1.0, 1.0 / D, 'bfloat16', 5)
        assert json.loads(json.dumps(res)) == res               # plain Python numbers and strings only
        for key in ('kid', 'kid_std', 'coef0', 'gamma'):
            assert type(res[key]) is float
        for key in ('subsets', 'subset_size', 'n_real', 'n_fake', 'degree', 'seed'):
            assert type(res[key]) is int
    with pytest.raises(ValueError):
        kid_from_sums([1.0, 2.0], [1.0], [1.0, 2.0], 4)
    with pytest.raises(ValueError):
        kid_from_sums([], [], [], 4)
    with pytest.raises(ValueError):
        kid_from_sums([1.0], [1.0], [1.0], 1)


def test_kid_class_arguments_and_too_few_rows():
    from sbagan.kid import KID
    for bad in (dict(D=100), dict(subsets=0), dict(subsets=1025), dict(subsets=2.0), dict(subset_size=1),
                dict(subset_size=True), dict(capacity=0)):
        with pytest.raises(ValueError):
            KID(None, **bad)
    ev = KID(None, D=64, subsets=3, subset_size=10, dtype='float32')
    assert ev.count('real') == 0 and ev.count('fake') == 0 and ev.dtype == 'float32' and ev.seed == 100
    with pytest.raises(RuntimeError, match='real side holds 0 rows'):
        ev.result()
    with pytest.raises(ValueError):
        ev.count('both')
    with pytest.raises(RuntimeError):                           # CPU rows are refused
        ev.update_features('real', torch.zeros(4, 64))
    with pytest.raises(ValueError):
        ev.update_features('real', torch.zeros(4, 32))


def test_kid_flags_in_all_four_entry_points(capsys):
    import main
    import main_bert
    import pretrain_DAMSM
    import pretrain_DAMSM_bert
    for mod in (main, main_bert, pretrain_DAMSM, pretrain_DAMSM_bert):
        args = mod.parse_args([])
        assert args.kid is False and args.kid_subsets == 100 and args.kid_subset_size == 1000
        args = mod.parse_args(['--kid', '--kid_subsets', '1024', '--kid_subset_size', '2'])
        assert args.kid is True and args.kid_subsets == 1024 and args.kid_subset_size == 2
        assert mod.parse_args(['--kid_subsets', '1']).kid_subsets == 1
        for flag, bad in (('--kid_subsets', '0'), ('--kid_subsets', '1025'), ('--kid_subsets', 'many'),
                          ('--kid_subset_size', '1'), ('--kid_subset_size', '-5'), ('--kid_subset_size', '1e3')):
            with pytest.raises(SystemExit):
                mod.parse_args([flag, bad])
    capsys.readouterr()
    from trainer import condGANTrainer
    import trainer_bert
    for cls in (condGANTrainer, trainer_bert.condGANTrainer):
        assert cls.kid is False and cls.kid_subsets == 100 and cls.kid_subset_size == 1000 and cls.kid_seed == 100
        assert cls.kid_result is None and cls.kid_evaluator is None


def test_subset_draws_are_reproducible_without_replacement_and_private():
    from sbagan.kid import KID, draw_subsets
    random.seed(7)
    np.random.seed(7)
    torch.manual_seed(7)
    before = (random.getstate(), np.random.get_state(), torch.get_rng_state())
    ir, jf = draw_subsets(50, 33, 20, 6, seed=100)
    ir2, jf2 = draw_subsets(50, 33, 20, 6, seed=100)
    ir3, _ = draw_subsets(50, 33, 20, 6, seed=101)
    after = (random.getstate(), np.random.get_state(), torch.get_rng_state())
    assert before[0] == after[0] and torch.equal(before[2], after[2])
    assert before[1][0] == after[1][0] and np.array_equal(before[1][1], after[1][1]) and before[1][2:] == after[1][2:]
    assert ir.dtype == np.int32 and jf.dtype == np.int32 and ir.shape == (6, 20) and jf.shape == (6, 20)
    assert np.array_equal(ir, ir2) and np.array_equal(jf, jf2) and not np.array_equal(ir, ir3)
    for idx, n in ((ir, 50), (jf, 33)):
        assert idx.min() >= 0 and idx.max() < n
        for row in idx:
            assert len(set(row.tolist())) == 20                 # without replacement within a subset
    assert not np.array_equal(ir[0], ir[1])
    # the documented order: a private RandomState(seed), the real side's subsets first, then the generated side's
    rng = np.random.RandomState(100)
    want_r = np.stack([rng.choice(50, 20, replace=False) for _ in range(6)])
    want_f = np.stack([rng.choice(33, 20, replace=False) for _ in range(6)])
    assert np.array_equal(ir, want_r) and np.array_equal(jf, want_f)
    # m = n: every subset is a permutation of all rows
    full, _ = draw_subsets(9, 9, 9, 2, seed=1)
    assert sorted(full[0].tolist()) == list(range(9))


def test_kid_operator_refuses_cpu_tensors_and_bad_indices():
    from sbagan import ops
    x = torch.zeros(8, 64)
    with pytest.raises(RuntimeError):
        ops.kid_kernel_sums(x, x)
    with pytest.raises(RuntimeError):
        ops.kid_kernel_sums(x, x, np.zeros((1, 4), dtype=np.int32), np.zeros((1, 4), dtype=np.int32), exclude_diag=True)
    with pytest.raises(TypeError):
        ops.kid_kernel_sums([[0.0] * 64] * 8, x)
    # the index check itself runs on the host, before any upload
    ok = ops._kid_indices('t', np.array([[0, 7], [3, 3]], dtype=np.int64), 'idx', 8)
    assert ok.dtype == np.int32 and ok.flags['C_CONTIGUOUS'] and ok.tolist() == [[0, 7], [3, 3]]
    assert ops._kid_indices('t', torch.tensor([[1, 2]], dtype=torch.int32), 'idx', 8).tolist() == [[1, 2]]
    for bad in ([[0, 8]], [[-1, 2]], [[2 ** 31]]):
        with pytest.raises(ValueError, match='outside'):
            ops._kid_indices('t', np.array(bad, dtype=np.int64), 'idx', 8)
    with pytest.raises(TypeError):
        ops._kid_indices('t', np.array([[0.0, 1.0]]), 'idx', 8)
    with pytest.raises(ValueError):
        ops._kid_indices('t', np.array([0, 1], dtype=np.int32), 'idx', 8)           # 1-D
    with pytest.raises(ValueError):
        ops._kid_indices('t', np.zeros((2, 0), dtype=np.int32), 'idx', 8)           # no positions


def test_header_declares_what_the_binding_binds():
    from sbagan import _lib
    decls = {name: (d.ret, ['%s %s' % (ctext, arg) for ctext, arg, _ in d.params])
             for name, d in _lib.DECLS.items() if name.startswith('sba_kid_')}
    assert sorted(decls) == ['sba_kid_kernel_sums', 'sba_kid_workspace_bytes']
    ret, args = decls['sba_kid_kernel_sums']
    sig = _lib.SIGNATURES['sba_kid_kernel_sums']
    assert ret == 'int' and len(sig) == len(args) == 18
    for ctype, arg in zip(sig, args):                           # pointers to pointers, ints to ints, int64_t to int64
        want = ctypes.c_void_p if '*' in arg else ctypes.c_int64 if 'int64_t' in arg else ctypes.c_int
        assert ctype is want, arg
    assert _lib.lib.sba_kid_kernel_sums.restype is ctypes.c_int
    ret, args = decls['sba_kid_workspace_bytes']
    size = _lib.lib.sba_kid_workspace_bytes
    assert ret == 'int64_t' and size.restype is ctypes.c_int64 and list(size.argtypes) == [ctypes.c_int] * len(args)


def test_workspace_size_needs_no_device():
    """one f64 per (subset, block of 64 A positions, column split); nothing when that is a single partial per subset"""
    from sbagan import _lib
    size = _lib.lib.sba_kid_workspace_bytes
    assert size(64, 64, 1, 0) == 0 and size(64, 64, 5, 1) == 0 and size(2, 2, 1024, 32) == 0
    assert size(65, 64, 1, 1) == 2 * 8 and size(65, 64, 3, 1) == 3 * 2 * 8
    assert size(130, 130, 3, 2) == 3 * 3 * 2 * 8
    assert size(130, 130, 3, 32) == 3 * 3 * 3 * 8                  # splits are capped at the three B tiles
    # the library's choice aims at 512 workgroups: 16 blocks x 100 subsets need no split, one subset gets all 16 tiles
    assert size(1000, 1000, 100, 0) == 100 * 16 * 8
    assert size(1000, 1000, 1, 0) == 16 * 16 * 8
    for bad in ((0, 5, 1, 0), (5, 0, 1, 0), (5, 5, 0, 0), (5, 5, 1025, 0), (5, 5, 1, -1), (5, 5, 1, 33)):
        assert size(*bad) == -1, bad
