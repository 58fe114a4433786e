"""Nearest training images on the host: the numpy reference (tests/nearest_ref.py) against brute force, the host
arithmetic of sbagan.nearest.nearest_from_lists on hand-made lists, the cache of the training rows and its key, the three
command-line flags, the gaps of the real-valued fixtures the GPU test relies on, and the header / binding agreement.
(The kernel is tested on the GPU in tests/test_nearest_gpu.py.)"""
import ctypes
import json

import numpy as np
import pytest
import torch

import nearest_ref

INF = float('inf')


# ------------------------------------------------------------------ the reference
def test_reference_against_brute_force():
    rng = np.random.RandomState(1)
    for na, nb, D, k in ((5, 7, 4, 8), (9, 20, 3, 3), (1, 1, 2, 1)):
        A, B = rng.randint(-2, 3, (na, D)).astype(np.float32), rng.randint(-2, 3, (nb, D)).astype(np.float32)
        d2, idx = nearest_ref.topk(A, B, k)
        assert d2.shape == (na, k) and idx.shape == (na, k) and idx.dtype == np.int64
        for i in range(na):
            # brute force: pick the minimum of what is left, k times; argmin takes the first of equals
            left = [float(((A[i].astype(np.float64) - B[j].astype(np.float64)) ** 2).sum()) for j in range(nb)]
            for m in range(k):
                if m >= nb:
                    assert d2[i, m] == INF and idx[i, m] == -1
                    continue
                j = int(np.argmin(left))
                assert (d2[i, m], idx[i, m]) == (left[j], j)
                left[j] = INF
    # ties are certain on such values, and go to the smaller row number
    d2, idx = nearest_ref.topk(np.zeros((1, 4), np.float32), np.ones((3, 4), np.float32), 2)
    assert d2.tolist() == [[4.0, 4.0]] and idx.tolist() == [[0, 1]]


def test_reference_never_lists_a_nan_or_an_infinite_distance():
    d2 = np.array([[3.0, np.nan, 1.0, INF], [np.nan, np.nan, np.nan, np.nan]])
    got_d, got_j = nearest_ref.topk_of(d2, 3)
    assert got_j.tolist() == [[2, 0, -1], [-1, -1, -1]]
    assert got_d.tolist() == [[1.0, 3.0, INF], [INF, INF, INF]]


# ------------------------------------------------------------------ nearest_from_lists
def test_fields_and_plain_numbers():
    from sbagan.nearest import FIELDS, nearest_from_lists
    res = nearest_from_lists([[1.0, 2.0]], [[0, 1]], [4.0], [1], [1.0, 1.0], dtype='bfloat16')
    assert sorted(res) == sorted(FIELDS)
    assert json.loads(json.dumps(res)) == res
    assert (res['k'], res['n_train'], res['n_real'], res['n_fake'], res['n_nan'], res['dtype']) == (2, 2, 1, 1, 0, 'bfloat16')
    assert res['nn_dist_fake'] == {'median': 1.0, 'mean': 1.0} and res['nn_dist_real'] == {'median': 2.0, 'mean': 2.0}
    assert res['nn_ratio'] == 0.5
    assert res['suspects'] == [{'row': 0, 'key': 0, 'd2': [1.0, 2.0], 'train_rows': [0, 1], 'train_keys': [0, 1]}]


def test_authenticity_is_strict_and_a_missing_neighbour_counts_against():
    from sbagan.nearest import nearest_from_lists
    r2 = [4.0, 9.0, np.nan]
    #                 == r_T: not authentic | above: authentic | no neighbour | nearest row's own radius is a NaN
    fd = [[4.0], [4.0 + 2.0 ** -50], [INF], [100.0]]
    fi = [[0], [0], [-1], [2]]
    res = nearest_from_lists(fd, fi, [9.0, 9.5], [1, 1], r2)
    assert res['authenticity'] == 0.25 and res['authenticity_real'] == 0.5
    assert res['n_nan'] == 1 and res['n_fake'] == 4
    # the row without a neighbour is in no distance figure and is no copy
    assert res['nn_dist_fake']['median'] == 2.0 and res['copy_fraction'] == 0.5     # threshold 9: 4, 4 + eps
    want = nearest_ref.statistics(fd, fi, [9.0, 9.5], [1, 1], r2)
    for key, value in want.items():
        assert res[key] == value, key
    # nothing has a neighbour: no figure, nothing authentic, no suspect
    res = nearest_from_lists([[INF]], [[-1]], [INF], [-1], [1.0])
    assert res['authenticity'] == 0.0 and res['authenticity_real'] == 0.0 and res['n_nan'] == 2
    assert res['nn_dist_fake'] == {'median': None, 'mean': None} and res['nn_ratio'] is None
    assert res['copy_fraction'] == 0.0 and res['copy_threshold'] is None and res['train_hit_max'] == 0
    assert res['suspects'] == [] and json.loads(json.dumps(res)) == res


@pytest.mark.parametrize('n_real,place', [(1, 1), (99, 1), (100, 1), (101, 2)])
def test_copy_threshold_is_the_ceil_of_one_percent(n_real, place):
    from sbagan.nearest import nearest_from_lists
    rd = np.arange(n_real, 0, -1, dtype=np.float64)             # n_real .. 1: the place-th smallest is `place`
    fd = [[0.5], [1.0], [1.5], [2.0], [2.5]]
    res = nearest_from_lists(fd, [[0]] * 5, rd, [0] * n_real, [0.0])
    assert res['copy_threshold'] == float(place)
    assert res['copy_fraction'] == (2 if place == 1 else 4) / 5.0       # `<=`: the value equal to T counts
    assert res['copy_fraction'] == nearest_ref.statistics(fd, [[0]] * 5, rd, [0] * n_real, [0.0])['copy_fraction']


def test_train_hits():
    from sbagan.nearest import nearest_from_lists
    fi = [[3], [3], [1], [3], [-1], [0]]
    fd = [[1.0], [1.0], [1.0], [1.0], [INF], [1.0]]
    res = nearest_from_lists(fd, fi, [1.0], [0], [1.0] * 4)
    assert res['train_hit_max'] == 3 and res['train_hit_distinct'] == 3 / 4.0     # min(6 generated, 4 training)
    res = nearest_from_lists(fd[:2], fi[:2], [1.0], [0], [1.0] * 4)
    assert res['train_hit_max'] == 2 and res['train_hit_distinct'] == 1 / 2.0     # min(2 generated, 4 training)


def test_suspects_in_order_of_distance_then_row_number():
    from sbagan.nearest import nearest_from_lists
    fd = [[2.0, 3.0], [1.0, INF], [2.0, 2.0], [INF, INF], [1.0, 5.0]]
    fi = [[0, 1], [2, -1], [1, 0], [-1, -1], [0, 2]]
    fake_keys, train_keys = ['g%d' % g for g in range(5)], ['t0', 't1', 't2']
    res = nearest_from_lists(fd, fi, [1.0], [0], [1.0] * 3, fake_keys, train_keys, show=4)
    assert [s['row'] for s in res['suspects']] == [1, 4, 0, 2] == nearest_ref.suspect_rows(fd, fi, 4)
    assert res['suspects'][0] == {'row': 1, 'key': 'g1', 'd2': [1.0], 'train_rows': [2], 'train_keys': ['t2']}
    assert res['suspects'][3] == {'row': 2, 'key': 'g2', 'd2': [2.0, 2.0], 'train_rows': [1, 0],
                                  'train_keys': ['t1', 't0']}
    # more asked for than rows with a neighbour: the row without one is never a suspect
    res = nearest_from_lists(fd, fi, [1.0], [0], [1.0] * 3, fake_keys, train_keys, show=16)
    assert [s['row'] for s in res['suspects']] == [1, 4, 0, 2]
    assert nearest_from_lists(fd, fi, [1.0], [0], [1.0] * 3, show=0)['suspects'] == []


def test_statistics_against_the_reference_on_random_sets():
    from sbagan.nearest import nearest_from_lists
    rng = np.random.RandomState(4)
    T = rng.randn(40, 8).astype(np.float32)
    R = rng.randn(25, 8).astype(np.float32)
    F = np.concatenate([T[:6] + 0.01 * rng.randn(6, 8).astype(np.float32), rng.randn(20, 8).astype(np.float32)])
    fd, fi = nearest_ref.topk(F, T, 3)
    rd, ri = nearest_ref.topk(R, T, 1)
    r2 = nearest_ref.knn_radius(T, 1)
    res = nearest_from_lists(fd, fi, rd, ri, r2, show=5)
    want = nearest_ref.statistics(fd, fi, rd, ri, r2)
    for key, value in want.items():
        assert res[key] == value, key
    assert 0.0 < res['authenticity'] < 1.0 and res['copy_fraction'] >= 6 / 26.0
    assert [s['row'] for s in res['suspects']] == nearest_ref.suspect_rows(fd, fi, 5)
    # int32 row numbers and one-column real lists, as the device hands them over, give the same result
    assert nearest_from_lists(fd, fi.astype(np.int32), rd[:, 0], ri[:, 0].astype(np.int32), r2, show=5) == res


def test_refusals_of_the_host_arithmetic():
    from sbagan.nearest import nearest_from_lists
    ok = dict(fake_d2=[[1.0]], fake_idx=[[0]], real_d2=[1.0], real_idx=[0], train_r2=[1.0])
    for bad in (dict(fake_idx=[[0, 0]]), dict(fake_idx=[[1]]), dict(real_idx=[-2]), dict(fake_idx=[[0.5]]),
                dict(real_d2=[[1.0, 2.0]], real_idx=[[0, 0]]), dict(train_r2=[]), dict(show=-1),
                dict(fake_keys=['a', 'b']), dict(train_keys=[]), dict(fake_d2=np.zeros((0, 1)), fake_idx=np.zeros((0, 1), int))):
        with pytest.raises(ValueError):
            nearest_from_lists(**dict(ok, **bad))


# ------------------------------------------------------------------ the evaluator's arguments, the cache and its key
def test_nearest_class_arguments_and_too_few_rows():
    from sbagan.nearest import Nearest
    for bad in (dict(D=100), dict(k=0), dict(k=9), dict(k=2.0), dict(capacity=0), dict(show=-1), dict(show=1.5)):
        with pytest.raises(ValueError):
            Nearest(None, **bad)
    ev = Nearest(None, D=64, k=3, dtype='float32')
    assert [ev.count(s) for s in ('train', 'real', 'fake')] == [0, 0, 0] and ev.dtype == 'float32'
    with pytest.raises(RuntimeError, match='train side holds 0 rows'):
        ev.result()
    with pytest.raises(ValueError):
        ev.count('both')
    with pytest.raises(RuntimeError):                           # CPU rows are refused
        ev.update_features('train', torch.zeros(4, 64))
    with pytest.raises(ValueError):
        ev.update_features('real', torch.zeros(4, 32))


def test_feature_rows_keep_their_two_sides_by_default():
    from sbagan.feature_rows import SIDES, FeatureRows
    assert SIDES == ('real', 'fake')
    with pytest.raises(ValueError, match="side must be 'real' or 'fake'"):
        FeatureRows('PRDC', 64).count('train')
    assert FeatureRows('Nearest', 64, sides=('train', 'real', 'fake')).count('train') == 0


def test_cache_key_refusals(tmp_path):
    """the round trip of the file needs a device (tests/test_nearest_gpu.py); what is refused does not"""
    from sbagan.nearest import Nearest, stats_key
    key = stats_key('enc/image_encoder200.pth', 'bfloat16', 'train', 256)
    assert key == 'encoder=enc/image_encoder200.pth|dtype=bfloat16|split=train|side=256'
    path = str(tmp_path / 'train.npz')
    rows, names = np.zeros((3, 64), np.float32), np.asarray(['a', 'b', 'c'])
    np.savez(path, rows=rows, keys=names, key=np.str_(key))
    for other in (stats_key('enc/image_encoder100.pth', 'bfloat16', 'train', 256),
                  stats_key('enc/image_encoder200.pth', 'float32', 'train', 256),
                  stats_key('enc/image_encoder200.pth', 'bfloat16', 'test', 256),
                  stats_key('enc/image_encoder200.pth', 'bfloat16', 'train', 128)):
        with pytest.raises(ValueError, match='holds training rows for'):
            Nearest(None, D=64, key=other).load_train(path, 'cpu')
    for bad in (dict(rows=rows.astype(np.float64)), dict(rows=rows[:, :32]), dict(keys=names[:2]), dict(rows=rows[:0], keys=names[:0])):
        np.savez(path, **dict(dict(rows=rows, keys=names, key=np.str_(key)), **bad))
        with pytest.raises(ValueError, match='does not hold'):
            Nearest(None, D=64, key=key).load_train(path, 'cpu')


# ------------------------------------------------------------------ the command line
def test_nearest_flags_in_all_four_entry_points(capsys):
    import main
    import main_bert
    import pretrain_DAMSM
    import pretrain_DAMSM_bert
    for mod in (main, main_bert, pretrain_DAMSM, pretrain_DAMSM_bert):
        args = mod.parse_args([])
        assert (args.nearest, args.nearest_stats, args.nearest_show) == (0, None, 16)
        for k in range(0, 9):
            assert mod.parse_args(['--nearest', str(k)]).nearest == k
        for bad in ('9', '-1', 'five'):
            with pytest.raises(SystemExit):
                mod.parse_args(['--nearest', bad])
        args = mod.parse_args(['--nearest', '3', '--nearest_stats', 'rows.npz', '--nearest_show', '0'])
        assert (args.nearest, args.nearest_stats, args.nearest_show) == (3, 'rows.npz', 0)
        assert mod.parse_args(['--nearest_show', '40']).nearest_show == 40
        for bad in ('-1', 'all'):
            with pytest.raises(SystemExit):
                mod.parse_args(['--nearest_show', bad])
    capsys.readouterr()
    from trainer import condGANTrainer
    import trainer_bert
    for cls in (condGANTrainer, trainer_bert.condGANTrainer):
        assert cls.nearest == 0 and cls.nearest_result is None and cls.nearest_show == 16 and cls.nearest_stats is None


# ------------------------------------------------------------------ what the GPU test relies on
@pytest.mark.parametrize('case', nearest_ref.REAL)
def test_real_fixtures_keep_their_neighbour_gaps(case):
    na, nb, D, k = case[:4]
    A, B, ref = nearest_ref.real_case(*case)
    assert A.shape == (na, D) and B.shape == (nb, D) and A.dtype == np.float32 and not A.flags.writeable
    gap, bound = nearest_ref.smallest_gap(ref, k), nearest_ref.d2_bound_rel(D)
    print('smallest relative gap %.3g against the bound %.3g' % (gap, bound))
    assert gap > 10.0 * bound
    assert (ref['top_idx'] >= 0).all() and np.isfinite(ref['top_d2']).all()
    assert (np.diff(ref['top_d2'], axis=1) > 0).all()


def test_operator_refuses_cpu_tensors():
    from sbagan import ops
    assert ops.KNN_MAX_K == 8
    x = torch.zeros(8, 64)
    with pytest.raises(RuntimeError):
        ops.knn_topk(x, x, 2)
    with pytest.raises(TypeError):
        ops.knn_topk([[0.0] * 64] * 8, x, 2)


def test_header_declares_what_the_binding_binds():
    from sbagan import _lib
    decls = {name: (d.ret, ['%s %s' % (ctext, arg) for ctext, arg, _ in d.params])
             for name, d in _lib.DECLS.items() if name.startswith('sba_knn_')}
    assert sorted(decls) == ['sba_knn_topk', 'sba_knn_workspace_bytes']
    ret, args = decls['sba_knn_topk']
    sig = _lib.SIGNATURES['sba_knn_topk']
    assert ret == 'int' and len(sig) == len(args)
    for ctype, arg in zip(sig, args):
        want = ctypes.c_void_p if '*' in arg else ctypes.c_int64 if 'int64_t' in arg else ctypes.c_int
        assert ctype is want, arg
    ret, args = decls['sba_knn_workspace_bytes']
    size = _lib.lib.sba_knn_workspace_bytes
    assert ret == 'int64_t' and size.restype is ctypes.c_int64 and list(size.argtypes) == [ctypes.c_int] * len(args)
    # the size needs no device: nothing for one part, k (f64 + int32) per row and part otherwise, parts capped at the tiles
    assert size(100, 100, 5, 1) == 0 and size(100, 100, 5, 2) == 2 * 100 * 5 * 12 and size(100, 100, 5, 7) == 2 * 100 * 5 * 12
    assert size(2933, 8855, 8, 0) == 12 * 2933 * 8 * 12             # 46 row blocks: 12 parts reach 512 workgroups
    assert size(0, 5, 1, 1) == -1 and size(5, 5, 0, 1) == -1 and size(5, 5, 9, 1) == -1 and size(5, 5, 1, 33) == -1
