"""Nearest training images on the GPU: the float64 distance-and-selection kernel through ops.knn_topk and the C ABI --
exactly equal to the numpy reference (tests/nearest_ref.py) on integer-valued features, within the derived bound
(distances) and exactly (row numbers) on real-valued ones -- invariance under the column split, the bitwise link to
ops.prdc_knn_radius, rows that hold a NaN, a padded row stride, the refusals, the Nearest class with a stub feature
callable, and sampling() with --nearest through both entry points."""
import json
import math
import os

import numpy as np
import pytest
import torch

import nearest_ref
import sampling_harness as sh

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = 8                       # guard words on either side of an output
INF = float('inf')


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def dev(x):
    return torch.tensor(np.asarray(x), device=DEV)


def host(t):
    return t.cpu().numpy()


def topk(a, b, k, splits=0):
    from sbagan import ops
    d2, idx = ops.knn_topk(dev(a), dev(b), k, splits=splits)
    assert d2.dtype == torch.float64 and idx.dtype == torch.int32
    assert tuple(d2.shape) == (a.shape[0], k) == tuple(idx.shape) and d2.is_contiguous() and idx.is_contiguous()
    return host(d2), host(idx)


def guarded(na, k):
    """(d2 buffer, idx buffer) with GUARD words of a pattern around the [na][k] outputs, the outputs filled with it too"""
    d = torch.full((na * k + 2 * GUARD,), -7.0, dtype=torch.float64, device=DEV)
    j = torch.full((na * k + 2 * GUARD,), -7, dtype=torch.int32, device=DEV)
    return d, j


def c_topk(a, b, k, splits, d, j, ws=None, ws_bytes=0, lda=None, ldb=None, D=None):
    """sba_knn_topk on the inner part of guarded buffers; returns the status"""
    from sbagan import _lib
    return _lib.lib.sba_knn_topk(a.data_ptr(), a.shape[0], lda or a.stride(0), b.data_ptr(), b.shape[0], ldb or b.stride(0),
                                 D or a.shape[1], k, splits, d.data_ptr() + 8 * GUARD, j.data_ptr() + 4 * GUARD,
                                 ws.data_ptr() if ws is not None else None, ws_bytes,
                                 torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------ exactness on integer-valued features
# (1, 1): the smallest call; 64: the tile edge; 63 x 65 and 65 x 130: one below / above it, a second row block, a column
# tile of 1 and of 2 rows; 130 x 63: three row blocks on one column tile; 5 x 7 at k = 8: fewer rows than places.
EXACT = [(1, 1, 64, 1), (64, 64, 64, 1), (63, 65, 64, 8), (65, 130, 128, 5), (130, 63, 192, 3), (5, 7, 64, 8)]


@pytest.mark.parametrize('na,nb,D,k', EXACT)
def test_integer_features_are_exact(na, nb, D, k):
    from sbagan import _lib
    A, B = nearest_ref.int_features(na, D, 1000 * D + 10 * na + k), nearest_ref.int_features(nb, D, 77 * D + nb + k)
    B[nb - 1] = A[0]                                            # a distance of exactly 0
    if nb > 2:
        B[0] = B[2] = A[na - 1]                                 # twins at 0 from the last row: a tie at the head of its list
    want_d, want_j = nearest_ref.topk(A, B, k)
    assert want_d[0, 0] == 0.0
    if nb > 2:                                                  # the tie goes to the smaller row number
        assert want_d[na - 1, 0] == 0.0 and want_j[na - 1, 0] == 0 and (k == 1 or want_j[na - 1, 1] == 2)
    assert (want_j[:, min(nb, k):] == -1).all() and (want_j[:, :min(nb, k)] >= 0).all()
    a, b = dev(A), dev(B)
    for splits in (1, 2):
        d, j = guarded(na, k)
        size = _lib.lib.sba_knn_workspace_bytes(na, nb, k, splits)
        ws = torch.zeros(size // 8 + 1, dtype=torch.float64, device=DEV) if size else None
        assert c_topk(a, b, k, splits, d, j, ws, size) == 0
        d, j = host(d), host(j)
        assert np.array_equal(bits(d[GUARD:-GUARD].reshape(na, k)), bits(want_d))
        assert np.array_equal(j[GUARD:-GUARD].reshape(na, k), want_j)
        for buf in (d, j):
            assert (buf[:GUARD] == -7).all() and (buf[-GUARD:] == -7).all()
    got_d, got_j = topk(A, B, k)
    assert np.array_equal(bits(got_d), bits(want_d)) and np.array_equal(got_j, want_j)


# ------------------------------------------------------------------ real-valued features against float64 numpy
@pytest.mark.parametrize('case', nearest_ref.REAL)
def test_real_features_within_the_bound_and_row_numbers_equal(case):
    na, nb, D, k = case[:4]
    A, B, ref = nearest_ref.real_case(*case)
    bound = nearest_ref.d2_bound_rel(D)
    got_d, got_j = topk(A, B, k)
    # the order of the first k stands when consecutive neighbours lie further apart than both can move
    gap = nearest_ref.smallest_gap(ref, k)
    print('smallest relative gap %.3g against the bound %.3g' % (gap, bound))
    assert gap > 10.0 * bound
    assert (got_j >= 0).all()
    tol = bound * (ref['n_a'][:, None] + ref['n_b'][got_j])
    err = np.abs(got_d - np.take_along_axis(ref['d2'], got_j.astype(np.int64), axis=1))
    print('distance error / bound %.3g' % (err / tol).max())
    assert (err <= tol).all()
    assert np.array_equal(got_j, ref['top_idx'])                # every row, none left out
    assert (np.abs(got_d - ref['top_d2']) <= tol).all()


# ------------------------------------------------------------------ split invariance, determinism
def test_splits_and_repeated_launches_are_bit_identical():
    A, B, ref = nearest_ref.real_case(*nearest_ref.REAL[2])     # nb = 200: four column tiles
    runs = [topk(A, B, 3, splits) for splits in (1, 2, 5, 32, 1, 1, 0)]     # (5 and 32 are capped at the four tiles)
    assert np.array_equal(runs[0][1], ref['top_idx'])
    for d, j in runs[1:]:
        assert np.array_equal(bits(d), bits(runs[0][0])) and np.array_equal(j, runs[0][1])
    # ties everywhere, fewer listable rows than places in one split: the key decides alike
    X, Y = nearest_ref.int_features(70, 64, 5) // 4, nearest_ref.int_features(133, 64, 6) // 4
    runs = [topk(X, Y, 8, splits) for splits in (1, 2, 3, 32)]
    want_d, want_j = nearest_ref.topk(X, Y, 8)
    assert (np.diff(want_d, axis=1) == 0).any()
    for d, j in runs:
        assert np.array_equal(bits(d), bits(want_d)) and np.array_equal(j, want_j)


# ------------------------------------------------------------------ the link to PRDC
@pytest.mark.parametrize('k', [1, 5, 7])
def test_lists_without_self_give_the_prdc_radius_bit_for_bit(k):
    from sbagan import ops
    rng = np.random.RandomState(11)
    X = rng.randn(130, 128).astype(np.float32)
    X[100] = X[3]                                               # twins in different row blocks
    x = dev(X)
    d, j = ops.knn_topk(x, x, k + 1)
    d, j = host(d), host(j)
    radius = host(ops.prdc_knn_radius(x, k))
    for i in range(130):
        others = d[i][j[i] != i]                                # (self sits in the list: d2(i, i) is 0 or a rounding error)
        assert others.shape[0] >= k
        assert bits(others[k - 1]) == bits(radius[i]), i
    # a twin is as far away as the row itself, bit for bit (0, or the same rounding error of |x|^2 against x . x): the two
    # lead both lists, the smaller row number first
    for i in (3, 100):
        assert bits(d[i, 0]) == bits(d[i, 1]) and d[i, 1] < 1e-9 and j[i, :2].tolist() == [3, 100]
    # on integer-valued rows that distance is exactly 0
    Y = nearest_ref.int_features(130, 128, 12)
    Y[100] = Y[3]
    d, j = ops.knn_topk(dev(Y), dev(Y), k + 1)
    d, j = host(d), host(j)
    for i in (3, 100):
        assert d[i, 0] == 0.0 and d[i, 1] == 0.0 and j[i, :2].tolist() == [3, 100]
    assert np.array_equal(j[:, 0], np.where(np.arange(130) == 100, 3, np.arange(130))) and (d[:, 0] == 0.0).all()
    radius = host(ops.prdc_knn_radius(dev(Y), k))
    want = nearest_ref.knn_radius(Y, k)
    assert np.array_equal(bits(radius), bits(want)) and (k > 1 or (radius[3] == 0.0 and radius[100] == 0.0))


# ------------------------------------------------------------------ NaN rows, padded rows
def test_a_row_holding_a_nan_is_never_listed():
    A, B = (np.array(v) for v in nearest_ref.real_case(*nearest_ref.REAL[0])[:2])
    clean_d, clean_j = topk(A, B, 8)
    A[66, 13] = np.nan                                          # in A: that query has no neighbour at all
    d, j = topk(A, B, 8)
    assert (d[66] == INF).all() and (j[66] == -1).all()
    keep = np.arange(70) != 66
    assert np.array_equal(bits(d[keep]), bits(clean_d[keep])) and np.array_equal(j[keep], clean_j[keep])
    A[66, 13] = 0.0
    victim = int(clean_j[0, 0])                                 # in B: the row that was row 0's nearest
    B[victim, 70 % 64] = np.nan
    for splits in (1, 3):
        d, j = topk(A, B, 8, splits)
        assert (j != victim).all() and (j >= 0).all() and np.isfinite(d).all()
        Bc = np.delete(B, victim, axis=0)
        want_d, want_j = nearest_ref.topk(A, Bc, 8)
        want_j = want_j + (want_j >= victim)                    # row numbers of the full set
        assert np.array_equal(j, want_j)
    # B of nothing but NaN rows: every list is the padding
    d, j = topk(A[:5], np.full((3, 64), np.nan, np.float32), 2)
    assert (d == INF).all() and (j == -1).all()


def test_row_stride_larger_than_the_width():
    from sbagan import ops
    X, Y = nearest_ref.int_features(65, 192, 7), nearest_ref.int_features(21, 192, 8)
    wide_x = torch.full((65, 200), 1e30, device=DEV)            # ld = 200: the 8 extra columns must never be read
    wide_y = torch.full((21, 196), 1e30, device=DEV)
    wide_x[:, :192] = dev(X)
    wide_y[:, :192] = dev(Y)
    want_d, want_j = nearest_ref.topk(X, Y, 4)
    for splits in (1, 2):
        d, j = ops.knn_topk(wide_x[:, :192], wide_y[:, :192], 4, splits=splits)
        assert np.array_equal(bits(host(d)), bits(want_d)) and np.array_equal(host(j), want_j)


# ------------------------------------------------------------------ refusals, all before any launch
def test_wrapper_refusals():
    from sbagan import ops
    x = torch.ones(8, 64, device=DEV)
    with pytest.raises(ValueError):
        ops.knn_topk(torch.ones(8, 100, device=DEV), torch.ones(8, 100, device=DEV), 2)    # D = 100
    with pytest.raises(ValueError):
        ops.knn_topk(x, torch.ones(8, 128, device=DEV), 2)                          # widths differ
    with pytest.raises(ValueError):
        ops.knn_topk(x, x, 0)
    with pytest.raises(ValueError):
        ops.knn_topk(x, x, 9)
    with pytest.raises(ValueError):
        ops.knn_topk(x, x, True)
    with pytest.raises(ValueError):
        ops.knn_topk(x, x, 2, splits=33)
    with pytest.raises(ValueError):
        ops.knn_topk(x, x, 2, splits=-1)
    with pytest.raises(TypeError):
        ops.knn_topk(x.double(), x, 2)
    with pytest.raises(TypeError):
        ops.knn_topk(x, x.double(), 2)
    with pytest.raises(RuntimeError):
        ops.knn_topk(x.cpu(), x, 2)
    with pytest.raises(RuntimeError):
        ops.knn_topk(x, x.cpu(), 2)
    with pytest.raises(ValueError):
        ops.knn_topk(torch.ones(8, 64, 1, device=DEV), x, 2)                        # 3-D
    with pytest.raises(ValueError):
        ops.knn_topk(x, torch.ones(64, 8, device=DEV).t(), 2)                       # column stride != 1
    with pytest.raises(ValueError):
        ops.knn_topk(torch.ones(8, 66, device=DEV)[:, :64], x, 2)                   # row stride 66
    with pytest.raises(ValueError):
        ops.knn_topk(x, torch.ones(8, 68, device=DEV)[:, 1:65], 2)                  # misaligned
    with pytest.raises(ValueError):
        ops.knn_topk(x[:0], x, 2)                                                   # no query row
    d2, idx = ops.knn_topk(x, x[:1], 8)                                             # fewer rows than places is no error
    assert (host(idx)[:, 0] == 0).all() and (host(idx)[:, 1:] == -1).all() and (host(d2)[:, 1:] == INF).all()


def test_c_abi_refusals():
    from sbagan import _lib
    E_ARG = -1
    x = torch.ones(200, 128, device=DEV)
    d, j = guarded(200, 8)
    size = _lib.lib.sba_knn_workspace_bytes
    assert size(200, 200, 5, 1) == 0 and size(200, 200, 5, 2) == 2 * 200 * 5 * 12 and size(200, 200, 5, 32) == 4 * 200 * 5 * 12
    assert size(0, 200, 5, 1) == -1 and size(200, 0, 5, 1) == -1 and size(200, 200, 0, 1) == -1
    assert size(200, 200, 9, 1) == -1 and size(200, 200, 5, 33) == -1 and size(200, 200, 5, -1) == -1
    ws = torch.zeros(4 * 200 * 8 * 12 // 8, dtype=torch.float64, device=DEV)
    full = ws.numel() * 8
    lib, st = _lib.lib.sba_knn_topk, torch.cuda.current_stream().cuda_stream
    X, Dp, Jp, W = x.data_ptr(), d.data_ptr() + 8 * GUARD, j.data_ptr() + 4 * GUARD, ws.data_ptr()

    def call(a=X, na=200, lda=128, b=X, nb=200, ldb=128, D=128, k=5, splits=1, d2=Dp, idx=Jp, w=W, nbytes=full):
        return lib(a, na, lda, b, nb, ldb, D, k, splits, d2, idx, w, nbytes, st)
    assert call(k=0) == E_ARG and call(k=9) == E_ARG
    assert call(D=96, lda=96, ldb=96) == E_ARG                                      # D % 64
    assert call(D=0) == E_ARG
    assert call(a=X + 4, na=100) == E_ARG and call(b=X + 4, nb=100) == E_ARG        # misaligned rows
    assert call(d2=Dp + 4) == E_ARG and call(idx=Jp + 2) == E_ARG                   # misaligned outputs
    assert call(a=None) == E_ARG and call(b=None) == E_ARG and call(d2=None) == E_ARG and call(idx=None) == E_ARG
    assert call(na=0) == E_ARG and call(nb=0) == E_ARG
    assert call(na=100, lda=64) == E_ARG and call(nb=100, ldb=130) == E_ARG         # ld < D, ld % 4
    assert call(splits=2, w=None) == E_ARG                                          # two parts need a workspace
    assert call(splits=2, nbytes=size(200, 200, 5, 2) - 1) == E_ARG                 # ... of the full size
    assert call(splits=2, w=W + 4) == E_ARG
    assert call(splits=33) == E_ARG and call(splits=-1) == E_ARG
    torch.cuda.synchronize()
    assert (host(d) == -7.0).all() and (host(j) == -7).all() and (host(ws) == 0).all()
    assert call(splits=2) == 0 and call(w=None, nbytes=0) == 0                       # (and what is accepted runs)
    torch.cuda.synchronize()
    assert (host(d)[GUARD:GUARD + 1000] == 0.0).all() and (host(d)[GUARD + 1000:] == -7.0).all()


# ------------------------------------------------------------------ the Nearest class with a stub feature callable
def _feed(ev, side, x, keys=None):
    """rows of x in batches of 20, 20, 7, 1, 20, ... rows"""
    lo, b = 0, 0
    while lo < x.shape[0]:
        rows = min((20, 20, 7, 1)[b % 4], x.shape[0] - lo)
        ev.update(side, x[lo:lo + rows], None if keys is None else keys[lo:lo + rows])
        lo, b = lo + rows, b + 1


def _stub_sets():
    """integer-valued, so a copy of a row lies at exactly 0 from it and every figure equals the reference's"""
    return nearest_ref.int_features(90, 64, 21), nearest_ref.int_features(40, 64, 22), nearest_ref.int_features(50, 64, 23)


def _stub_evaluator(T, R, F, k=3, show=4):
    from sbagan.nearest import Nearest
    ev = Nearest(lambda x: x, D=64, k=k, show=show, dtype='float32', capacity=16)      # (grows several times a side)
    _feed(ev, 'train', dev(T), ['t%d' % i for i in range(T.shape[0])])
    _feed(ev, 'real', dev(R))
    _feed(ev, 'fake', dev(F), ['g%d' % i for i in range(F.shape[0])])
    return ev


def test_nearest_class_against_the_reference():
    from sbagan.nearest import FIELDS
    T, R, F = _stub_sets()
    ev = _stub_evaluator(T, R, F)
    assert [ev.count(s) for s in ('train', 'real', 'fake')] == [90, 40, 50]
    assert np.array_equal(host(ev.rows('train')), T) and np.array_equal(host(ev.rows('fake')), F)
    res = ev.result()
    print({k: v for k, v in res.items() if k != 'suspects'})
    assert sorted(res) == sorted(FIELDS) and json.loads(json.dumps(res)) == res
    fd, fi = nearest_ref.topk(F, T, 3)
    rd, ri = nearest_ref.topk(R, T, 1)
    want = nearest_ref.statistics(fd, fi, rd, ri, nearest_ref.knn_radius(T, 1))
    for key, value in want.items():                # every distance is exact on these sets: so is every figure
        assert res[key] == value, key
    assert 0.0 < res['authenticity'] < 1.0 and 0.0 < res['authenticity_real'] < 1.0
    assert (res['k'], res['n_train'], res['n_real'], res['n_fake'], res['dtype']) == (3, 90, 40, 50, 'float32')
    rows = nearest_ref.suspect_rows(fd, fi, 4)
    assert [s['row'] for s in res['suspects']] == rows and [s['key'] for s in res['suspects']] == ['g%d' % g for g in rows]
    for s in res['suspects']:
        assert s['train_rows'] == fi[s['row']].tolist() and s['train_keys'] == ['t%d' % j for j in s['train_rows']]
    with pytest.raises(TypeError):
        ev.update('fake', dev(F).double())
    with pytest.raises(ValueError):
        ev.update('both', dev(F))
    with pytest.raises(ValueError):
        ev.update('fake', dev(F[:3]), ['one'])


def test_nearest_class_on_copies_on_the_real_rows_and_on_a_collapse():
    T, R, F = _stub_sets()
    # generated rows that are copies of training rows
    res = _stub_evaluator(T, R, T[5:45].copy()).result()
    assert res['authenticity'] == 0.0 and res['copy_fraction'] == 1.0
    assert res['nn_dist_fake'] == {'median': 0.0, 'mean': 0.0} and res['nn_ratio'] == 0.0
    assert res['train_hit_distinct'] == 1.0 and res['train_hit_max'] == 1
    assert [s['train_rows'][0] for s in res['suspects']] == [5, 6, 7, 8] and res['suspects'][0]['d2'][0] == 0.0
    assert 0.0 < res['authenticity_real'] <= 1.0
    # generated rows equal to the real rows: every generated-side figure equals its real-side counterpart
    res = _stub_evaluator(T, R, R.copy()).result()
    assert res['authenticity'] == res['authenticity_real'] and res['nn_dist_fake'] == res['nn_dist_real']
    rd, _ = nearest_ref.topk(R, T, 1)
    assert res['nn_ratio'] == 1.0 and res['copy_fraction'] == np.count_nonzero(rd == rd.min()) / 40.0
    # a collapsed generator: every generated row is one training row
    res = _stub_evaluator(T, R, np.repeat(T[17:18], 23, axis=0)).result()
    assert res['train_hit_max'] == 23 and res['train_hit_distinct'] == 1.0 / 23 and res['authenticity'] == 0.0


def test_cache_round_trip(tmp_path):
    from sbagan.nearest import Nearest
    T, R, F = _stub_sets()
    ev = _stub_evaluator(T, R, F)
    ev.key = 'encoder=e|dtype=float32|split=train|side=128'
    path = str(tmp_path / 'train.npz')
    ev.save_train(path)
    again = Nearest(lambda x: x, D=64, k=3, show=4, key=ev.key, dtype='float32')
    assert not again.is_loaded()
    again.load_train(path, DEV)
    assert again.is_loaded() and again.keys['train'] == ev.keys['train']
    assert np.array_equal(host(again.rows('train')), T)
    _feed(again, 'real', dev(R))
    _feed(again, 'fake', dev(F), ['g%d' % i for i in range(50)])
    assert again.result() == ev.result()
    with pytest.raises(ValueError, match='holds training rows for'):
        Nearest(lambda x: x, D=64, key='another').load_train(path, DEV)
    with pytest.raises(RuntimeError, match='already holds rows'):
        again.load_train(path, DEV)


# ------------------------------------------------------------------ the entry points
@pytest.fixture
def random_encoders(monkeypatch):
    """the entry points have no switch for randomly initialised encoders: both trainers get it through the base class"""
    import trainer
    init = trainer.condGANTrainer.__init__

    def init_random(self, *a, **kw):
        kw['allow_random_encoders'] = True
        init(self, *a, **kw)
    monkeypatch.setattr(trainer.condGANTrainer, '__init__', init_random)


def _check_json(files, k, show, n_train=4, n_images=6):
    from sbagan.nearest import FIELDS
    res = json.loads(files['nearest.json'].decode())
    print('nearest.json:', res)
    assert sorted(res) == sorted(FIELDS)
    assert (res['k'], res['n_train'], res['n_real'], res['n_fake'], res['n_nan'], res['dtype']) == \
        (k, n_train, n_images, n_images, 0, 'bfloat16')
    for key in ('authenticity', 'authenticity_real', 'copy_fraction', 'train_hit_distinct'):
        assert 0.0 <= res[key] <= 1.0
    assert 1 <= res['train_hit_max'] <= n_images and math.isfinite(res['nn_ratio']) and res['nn_ratio'] > 0.0
    assert len(res['suspects']) == min(show if show else 0, n_images)
    for s in res['suspects']:
        assert s['key'].startswith('cls/t') and len(s['d2']) == k and s['d2'] == sorted(s['d2'])
        assert all(name.startswith('cls/a') for name in s['train_keys']) and len(set(s['train_keys'])) == k
    return res


def _rnn_generator(tmp_path):
    from test_host_cpu import _make_dataset
    sh.toy_cfg()
    import model
    from miscc.utils import weights_init
    root = str(tmp_path / 'toy')
    _make_dataset(root, n_test=6)
    torch.manual_seed(1)
    netG = model.G_NET()
    netG.apply(weights_init)
    torch.save(netG.state_dict(), str(tmp_path / 'netG.pth'))
    return root


def test_main_without_and_with_the_flag_and_with_the_cache(tmp_path, random_encoders):
    import io

    import main
    from miscc.config import reset_cfg
    from PIL import Image
    root = _rnn_generator(tmp_path)
    stats = str(tmp_path / 'train.npz')
    files0, states0, calls0 = sh.run_main(main, tmp_path, 'without', [], root)
    files1, states1, calls1 = sh.run_main(main, tmp_path, 'with', ['--nearest', '3', '--nearest_show', '2',
                                                                   '--nearest_stats', stats], root)
    assert calls0 == 0 and len(files0) == 6 and all(k.endswith('_s-1.png') for k in files0)
    # the same image files, byte for byte, with nearest.json and nearest.png beside them
    assert sorted(files1) == sorted(list(files0) + ['nearest.json', 'nearest.png'])
    assert {k: v for k, v in files1.items() if k in files0} == files0
    # the flag consumes none of the randomness the data path and the noise draw from
    assert sh.same_states(states1, states0)
    assert calls1 == 3 + 3 + 2                      # one trunk forward per generated, per real and per training batch
    res1 = _check_json(files1, 3, 2)
    sheet = Image.open(io.BytesIO(files1['nearest.png']))
    assert sheet.size == (4 * 128, 2 * 128) and sheet.mode == 'RGB'
    # each row: the generated image as it was written, then its training images through the centre-crop path
    from sbagan.retrieval import _CenterCrops
    import datasets
    crops = _CenterCrops(datasets.TextDataset(root, 'train', base_size=64), 128, int(128 * 76 / 64))
    for r, s in enumerate(res1['suspects']):
        tiles = [Image.open(io.BytesIO(files1['single/%s_s-1.png' % s['key']])).convert('RGB')]
        tiles += [crops.window(j) for j in s['train_rows']]
        for c, tile in enumerate(tiles):
            assert tile.size == (128, 128)          # (the toy images are 128 px: the tiles are the images themselves)
            assert np.array_equal(np.asarray(sheet.crop((128 * c, 128 * r, 128 * c + 128, 128 * r + 128))),
                                  np.asarray(tile))
    # a missing --nearest_stats file was written; a second run reads it: no training pass, the same JSON
    assert os.path.exists(stats)
    files2, states2, calls2 = sh.run_main(main, tmp_path, 'cached', ['--nearest', '3', '--nearest_show', '2',
                                                                     '--nearest_stats', stats], root)
    assert calls2 == 3 + 3
    assert json.loads(files2['nearest.json'].decode()) == res1 and files2['nearest.png'] == files1['nearest.png']
    assert {k: v for k, v in files2.items() if k in files0} == files0 and sh.same_states(states2, states0)
    # --nearest_show 0: no picture and no suspects; a file written under another key is refused
    files3, _, _ = sh.run_main(main, tmp_path, 'bare', ['--nearest', '1', '--nearest_show', '0'], root)
    assert sorted(files3) == sorted(list(files0) + ['nearest.json'])
    _check_json(files3, 1, 0)
    from sbagan import ops
    try:
        with pytest.raises(ValueError, match='holds training rows for'):
            sh.run_main(main, tmp_path, 'refused', ['--nearest', '3', '--nearest_stats', stats], root, dtype=torch.float32)
    finally:
        ops.set_compute_dtype(torch.bfloat16)
    reset_cfg()


def test_main_with_fid_and_prdc_shares_the_forwards(tmp_path, random_encoders):
    import main
    from miscc.config import reset_cfg
    root = _rnn_generator(tmp_path)
    files0, states0, calls0 = sh.run_main(main, tmp_path, 'two', ['--fid', '--prdc', '2'], root)
    files1, states1, calls1 = sh.run_main(main, tmp_path, 'three', ['--fid', '--prdc', '2', '--nearest', '2'], root)
    assert calls0 == 3 + 3
    assert calls1 == 3 + 3 + 2                      # each batch goes through the trunk ONCE for all three evaluators
    assert sorted(files1) == sorted(list(files0) + ['nearest.json', 'nearest.png'])
    assert sh.images({k: v for k, v in files1.items() if k != 'nearest.png'}) == sh.images(files0)
    for name in ('fid.json', 'prdc.json'):
        assert json.loads(files1[name].decode()) == json.loads(files0[name].decode())
    assert sh.same_states(states1, states0)
    _check_json(files1, 2, 16)
    reset_cfg()


def test_main_bert_with_the_flag(tmp_path, random_encoders):
    import main_bert
    import model_bert
    from miscc.config import reset_cfg
    from miscc.utils import weights_init
    from test_bert_entry_gpu import _bert_dir
    from test_host_cpu import _make_dataset
    sh.toy_cfg()
    root = str(tmp_path / 'toy')
    _make_dataset(root, n_test=6)
    bert_dir = _bert_dir(tmp_path)
    torch.manual_seed(1)
    netG = model_bert.G_NET()
    netG.apply(weights_init)
    torch.save(netG.state_dict(), str(tmp_path / 'netG.pth'))
    files, _, calls = sh.run_main(main_bert, tmp_path, 'bert', ['--nearest', '2', '--nearest_show', '3'], root, bert_dir)
    assert len(files) == 8 and calls == 3 + 3 + 2
    _check_json(files, 2, 3)
    reset_cfg()
