"""FID on the GPU: the float64 moment kernels through ops.fid_accumulate / ops.fid_finalize -- bit for bit against numpy
on integer-valued features (every f64 sum is then exact), within the derived summation bounds on real-valued ones --
determinism, the refusals, the FID class with a stub feature callable, and sampling() with --fid through both trainers."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import sampling_harness as sh

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
U = 2.0 ** -53                  # unit roundoff of float64
TILE = 64
SENTINEL = -12345.5


def upper_tiles(D):
    """[D][D] bool: the entries inside the 64 x 64 tiles with tile row <= tile column"""
    t = np.arange(D) // TILE
    return t[:, None] <= t[None, :]


def fresh(D, sentinel=True):
    """zeroed sum and gram on the device; the tiles below the diagonal pre-filled with a sentinel"""
    gram = np.zeros((D, D))
    if sentinel:
        gram[~upper_tiles(D)] = SENTINEL
    return torch.zeros(D, dtype=torch.float64, device=DEV), torch.from_numpy(gram).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def check_exact(X, s, g):
    """sum and the upper tiles of gram equal numpy's float64 results bit for bit; the other tiles hold the sentinel"""
    D = X.shape[1]
    X64 = X.astype(np.float64)
    s, g, up = s.cpu().numpy(), g.cpu().numpy(), upper_tiles(D)
    assert np.array_equal(bits(s), bits(X64.sum(0)))
    assert np.array_equal(bits(g)[up], bits(X64.T @ X64)[up])
    assert (g[~up] == SENTINEL).all()


def int_features(n, D, seed):
    """integer values in [-8, 8], not symmetric in any way, every one of them present"""
    return np.random.RandomState(seed).randint(-8, 9, size=(n, D)).astype(np.float32)


# ------------------------------------------------------------------ exactness
# D = 64: one diagonal tile; 128: the first off-diagonal tile; 192: the triangular tile decode; 2048: the full grid.
# n = 1, 3: less than one MFMA step; 4, 5: one step and one row more; 21: a partial chunk; 64: two full chunks
EXACT = [(D, n) for D in (64, 128, 192) for n in (1, 3, 4, 5, 21, 64)] + [(2048, 20)]


@pytest.mark.parametrize('D,n', EXACT)
def test_integer_features_are_exact(D, n):
    from sbagan import ops
    X = int_features(n, D, 1000 * D + n)
    s, g = fresh(D)
    ops.fid_accumulate(torch.from_numpy(X).to(DEV), s, g)
    check_exact(X, s, g)


def test_row_stride_larger_than_the_width():
    from sbagan import ops
    X = int_features(21, 192, 7)
    wide = torch.full((21, 200), 99.0, device=DEV)         # ldx = 200: the 8 extra columns must never be read
    wide[:, :192] = torch.from_numpy(X).to(DEV)
    s, g = fresh(192)
    ops.fid_accumulate(wide[:, :192], s, g)
    check_exact(X, s, g)


def test_two_calls_accumulate_into_the_same_buffers():
    from sbagan import ops
    X = int_features(64 + 21, 192, 8)
    s, g = fresh(192)
    ops.fid_accumulate(torch.from_numpy(X[:64]).to(DEV), s, g)
    ops.fid_accumulate(torch.from_numpy(X[64:]).to(DEV), s, g)
    check_exact(X, s, g)


def test_asymmetric_operands_land_in_their_own_rows_and_columns():
    """x[k][i] = 1 for one column i, x[k][j] = j + 1: gram[i][j] = n (j + 1) in row i only -- catches a transposed or
    row-permuted accumulator write, which a symmetric random product can hide in the diagonal tiles"""
    from sbagan import ops
    D, n, i = 128, 4, 37
    X = np.zeros((n, D), dtype=np.float32)
    X[:, i] = 1.0
    X[:, 70:] = np.arange(71, D + 1, dtype=np.float32)
    s, g = fresh(D)
    ops.fid_accumulate(torch.from_numpy(X).to(DEV), s, g)
    check_exact(X, s, g)
    g = g.cpu().numpy()
    assert g[i, 100] == n * 101.0 and g[i, i] == n and g[36, 100] == 0.0 and g[38, 100] == 0.0


# ------------------------------------------------------------------ real-valued features against float64 numpy
# Bounds (derived, not measured): the f32 products are exact in f64; each entry is a sum of n terms, n f64 additions with
# relative error U each, so |error| <= n U sum|terms| to first order -- doubled for the numpy reference's own error.
REAL = [(64, 5), (128, 33), (192, 300), (2048, 20)]


def reference(X):
    """float64 numpy moments of the f32 rows X and the bounds on the kernels' distance from them"""
    n = X.shape[0]
    X64 = X.astype(np.float64)
    A, a = np.abs(X64).T @ np.abs(X64), np.abs(X64).sum(0)
    ref = {'sum': X64.sum(0), 'gram': X64.T @ X64, 'sigma': np.cov(X64, rowvar=False), 'mu': X64.mean(0),
           'sum_tol': 2 * n * U * a, 'gram_tol': 2 * n * U * A,
           'sigma_tol': 4 * n * U * (A + np.outer(a, a) / n) / (n - 1)}
    # mu = sum / n: the sum's bound over n, and one rounding of the division on either side
    ref['mu_tol'] = ref['sum_tol'] / n + 2 * U * np.abs(ref['mu'])
    for v in ref.values():
        v.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def real_case(D, n, seed=0):
    """(X f32 [n][D], reference(X)): positive-skewed features of uneven scale, computed once per shape"""
    rng = np.random.RandomState(100 * D + n + seed)
    X = (np.abs(rng.randn(n, D)) * rng.uniform(0.1, 3.0, D) - 0.2).astype(np.float32)
    X.setflags(write=False)
    return X, reference(X)


def check_stats(n_ref, ref, n, mu, sigma):
    assert n == n_ref
    assert (np.abs(mu - ref['mu']) <= ref['mu_tol']).all()
    assert (np.abs(sigma - ref['sigma']) <= ref['sigma_tol']).all()
    assert np.array_equal(bits(sigma), bits(sigma.T))


@pytest.mark.parametrize('D,n', REAL)
def test_real_features_within_the_summation_bounds(D, n):
    from sbagan import ops
    X, ref = real_case(D, n)
    s, g = fresh(D)
    ops.fid_accumulate(torch.tensor(X, device=DEV), s, g)
    up = upper_tiles(D)
    sh, gh = s.cpu().numpy(), g.cpu().numpy()
    es, eg = np.abs(sh - ref['sum']), np.abs(gh - ref['gram'])
    print('D %d n %d: sum error / bound %.3g, gram error / bound %.3g'
          % (D, n, (es / ref['sum_tol']).max(), (eg[up] / ref['gram_tol'][up]).max()))
    assert (es <= ref['sum_tol']).all()
    assert (eg[up] <= ref['gram_tol'][up]).all()
    assert (gh[~up] == SENTINEL).all()

    # finalize reads the upper triangle only: the sentinel tiles (and NaNs below the diagonal of the diagonal tiles)
    # must not reach sigma
    g[torch.from_numpy(np.tril(np.ones((D, D), dtype=bool), -1)).to(DEV)] = float('nan')
    mu, sigma, trace = ops.fid_finalize(s, g, n)
    mu, sigma, trace = mu.cpu().numpy(), sigma.cpu().numpy(), float(trace.cpu().numpy()[0])
    esig = np.abs(sigma - ref['sigma'])
    print('    sigma error / bound %.3g, trace error %.3g' % ((esig / ref['sigma_tol']).max(),
                                                             abs(trace - np.trace(ref['sigma']))))
    check_stats(n, ref, n, mu, sigma)
    assert abs(trace - np.trace(ref['sigma'])) <= D * np.diag(ref['sigma_tol']).max()


def test_two_launches_are_bit_identical():
    from sbagan import ops
    X, _ = real_case(192, 300)
    x = torch.tensor(X, device=DEV)
    outs = []
    for _ in range(2):
        s, g = fresh(192)
        ops.fid_accumulate(x[:171], s, g)
        ops.fid_accumulate(x[171:], s, g)
        outs.append([t.cpu().numpy() for t in (s, g) + ops.fid_finalize(s, g, 300)])
    for a, b in zip(*outs):
        assert np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------ refusals, all before any launch
def test_wrapper_refusals():
    from sbagan import ops
    s, g = fresh(64)
    x = torch.ones(4, 64, device=DEV)
    s100 = torch.zeros(100, dtype=torch.float64, device=DEV)
    g100 = torch.zeros(100, 100, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError):
        ops.fid_accumulate(torch.ones(4, 100, device=DEV), s100, g100)          # D = 100
    with pytest.raises(ValueError):
        ops.fid_accumulate(x[:0], s, g)                                         # n = 0
    with pytest.raises(TypeError):
        ops.fid_accumulate(x.double(), s, g)                                    # f64 features
    with pytest.raises(RuntimeError):
        ops.fid_accumulate(x.cpu(), s, g)                                       # CPU features
    with pytest.raises(ValueError):
        ops.fid_accumulate(torch.ones(4, 128, device=DEV), s, g)                # width != D
    with pytest.raises(ValueError):
        ops.fid_accumulate(torch.ones(64, 4, device=DEV).t(), s, g)             # column stride != 1
    with pytest.raises(ValueError):
        ops.fid_accumulate(torch.ones(4, 65, device=DEV)[:, 1:], s, g)          # misaligned, row stride 65
    with pytest.raises(TypeError):
        ops.fid_accumulate(x, s.float(), g)
    with pytest.raises(ValueError):
        ops.fid_accumulate(x, s, g[:, :32])
    with pytest.raises(ValueError):
        ops.fid_finalize(s, g, 1)                                               # no covariance of one row
    with pytest.raises(ValueError):
        ops.fid_finalize(s100, g100, 4)
    torch.cuda.synchronize()
    assert (s.cpu().numpy() == 0).all() and (g.cpu().numpy()[upper_tiles(64)] == 0).all()


def test_c_abi_refusals():
    from sbagan import _lib
    E_ARG = -1
    s, g = fresh(128)
    x = torch.ones(8, 128, device=DEV)
    out = torch.zeros(128 * 128 + 128 + 1, dtype=torch.float64, device=DEV)
    mu, sigma, trace = out.data_ptr(), out.data_ptr() + 8 * 128, out.data_ptr() + 8 * (128 + 128 * 128)
    st = torch.cuda.current_stream().cuda_stream
    acc, fin = _lib.lib.sba_fid_accumulate, _lib.lib.sba_fid_finalize
    assert acc(x.data_ptr() + 4, 4, 128, 128, s.data_ptr(), g.data_ptr(), st) == E_ARG      # misaligned x
    assert acc(x.data_ptr(), 4, 128, 128, s.data_ptr() + 4, g.data_ptr(), st) == E_ARG      # misaligned sum
    assert acc(x.data_ptr(), 4, 100, 128, s.data_ptr(), g.data_ptr(), st) == E_ARG          # D % 64
    assert acc(x.data_ptr(), 0, 128, 128, s.data_ptr(), g.data_ptr(), st) == E_ARG          # n < 1
    assert acc(x.data_ptr(), 4, 128, 64, s.data_ptr(), g.data_ptr(), st) == E_ARG           # ldx < D
    assert acc(None, 4, 128, 128, s.data_ptr(), g.data_ptr(), st) == E_ARG
    assert fin(s.data_ptr(), g.data_ptr(), 1, 128, mu, sigma, trace, st) == E_ARG           # n < 2
    assert fin(s.data_ptr(), g.data_ptr(), 4, 100, mu, sigma, trace, st) == E_ARG
    torch.cuda.synchronize()
    assert (s.cpu().numpy() == 0).all() and (g.cpu().numpy()[upper_tiles(128)] == 0).all()
    assert (out.cpu().numpy() == 0).all()


# ------------------------------------------------------------------ the FID class with a stub feature callable
def _feed(ev, side, x):
    """rows of x in batches of 20, 20, 7, 1, 20, ... rows"""
    lo, k = 0, 0
    while lo < x.shape[0]:
        b = min((20, 20, 7, 1)[k % 4], x.shape[0] - lo)
        ev.update(side, x[lo:lo + b])
        lo, k = lo + b, k + 1


def test_fid_class_with_stub_features():
    from sbagan.fid import FID, fid_from_stats
    D, n = 128, 300
    (Xr, ref_r), (Xf, ref_f) = real_case(D, n), real_case(D, n, seed=1)
    calls = []

    def features(images):           # the stub "trunk": the images are the feature rows
        calls.append(images.shape[0])
        return images

    ev = FID(features, D=D, chunk=16, dtype='float32')       # 16-row flushes split every 20-row batch
    _feed(ev, 'real', torch.tensor(Xr, device=DEV))
    _feed(ev, 'fake', torch.tensor(Xf, device=DEV))
    assert sum(calls) == 2 * n and set(calls) == {20, 7, 1, 12}
    check_stats(n, ref_r, *ev.stats('real'))
    check_stats(n, ref_f, *ev.stats('fake'))
    res = ev.result()
    want = fid_from_stats(ref_r['mu'], ref_r['sigma'], ref_f['mu'], ref_f['sigma'])
    scale = np.trace(ref_r['sigma']) + np.trace(ref_f['sigma'])
    print('fid %.12g, from the numpy moments %.12g, difference %.3g of the traces'
          % (res['fid'], want, abs(res['fid'] - want) / scale))
    assert abs(res['fid'] - want) <= 1e-9 * scale
    assert res['n_real'] == n and res['n_fake'] == n and res['dtype'] == 'float32'
    assert res['trace_real'] == pytest.approx(np.trace(ref_r['sigma']), abs=D * np.diag(ref_r['sigma_tol']).max())
    assert res['mean_term'] == pytest.approx(((ref_r['mu'] - ref_f['mu']) ** 2).sum(), rel=1e-12)

    same = FID(features, D=D, chunk=16)
    _feed(same, 'real', torch.tensor(Xr, device=DEV))
    same.update('fake', torch.tensor(Xr, device=DEV))        # one 300-row batch: other flush boundaries, same rows
    res = same.result()
    print('the same features on both sides: fid %.3g at tr S = %.4g' % (res['fid'], res['trace_real']))
    assert abs(res['fid']) <= 1e-9 * np.trace(ref_r['sigma'])
    with pytest.raises(TypeError):
        same.update('fake', torch.tensor(Xr, device=DEV).double())
    with pytest.raises(ValueError):
        same.update('fake', torch.zeros(3, 64, device=DEV))


# ------------------------------------------------------------------ sampling() with the flag
def _check_result(algo, files, n_images):
    res = json.loads(files['fid.json'].decode())
    print('fid.json:', res)
    assert res == algo.fid_result
    assert sorted(res) == ['dtype', 'fid', 'mean_term', 'n_fake', 'n_real', 'trace_fake', 'trace_real']
    assert res['n_real'] == n_images and res['n_fake'] == n_images and res['dtype'] == 'bfloat16'
    for k in ('fid', 'mean_term', 'trace_real', 'trace_fake'):
        assert math.isfinite(res[k])
    assert res['mean_term'] >= 0.0 and res['trace_real'] >= 0.0 and res['trace_fake'] >= 0.0
    return res


def test_sampling_without_with_and_with_cached_real_statistics(tmp_path):
    from miscc.config import reset_cfg
    make, loader, ds, ckpts = sh.setup(tmp_path, ('without', 'with', 'cached'))
    stats = str(tmp_path / 'real.npz')
    algo0, files0, states0, calls0 = sh.sample(make, loader, ds, ckpts[0])
    algo1, files1, states1, calls1 = sh.sample(make, loader, ds, ckpts[1], fid=True, fid_stats=stats)
    assert algo0.fid_result is None and calls0 == 0 and len(files0) == 6 and all(k.endswith('.png') for k in files0)
    # the same image files, byte for byte, and fid.json beside them
    assert sorted(files1) == sorted(list(files0) + ['fid.json']) and sh.images(files1) == files0
    # the flag consumes none of the randomness the data path and the noise draw from
    assert sh.same_states(states1, states0)
    res1 = _check_result(algo1, files1, 6)
    assert calls1 == 3 + 3                          # one trunk forward per generated and per real batch
    assert os.path.exists(stats)                    # a missing --fid_stats file is written after the run
    # a second run reads the real side from that file: no real-side forward, the same trace_real bit for bit
    algo2, files2, states2, calls2 = sh.sample(make, loader, ds, ckpts[2], fid=True, fid_stats=stats)
    res2 = _check_result(algo2, files2, 6)
    assert calls2 == 3
    assert res2['trace_real'] == res1['trace_real'] and res2['n_real'] == 6
    assert sh.images(files2) == files0 and sh.same_states(states2, states0)
    # a file written under another key is refused
    from sbagan import ops
    ops.set_compute_dtype(torch.float32)
    try:
        with pytest.raises(ValueError, match='holds statistics for'):
            sh.sample(make, loader, ds, ckpts[2], fid=True, fid_stats=stats)
    finally:
        ops.set_compute_dtype(torch.bfloat16)
    reset_cfg()


def test_sampling_with_r_precision_shares_the_generated_forward(tmp_path):
    from miscc.config import reset_cfg
    make, loader, ds, ckpts = sh.setup(tmp_path, ('rp', 'both'))
    algo0, files0, states0, calls0 = sh.sample(make, loader, ds, ckpts[0], r_precision=4)
    algo1, files1, states1, calls1 = sh.sample(make, loader, ds, ckpts[1], fid=True, r_precision=4)
    assert calls0 == 3
    assert calls1 == 3 + 3                          # the generated batch goes through the trunk ONCE
    assert sorted(files1) == sorted(list(files0) + ['fid.json']) and sh.images(files1) == sh.images(files0)
    assert json.loads(files1['r_precision.json'].decode()) == json.loads(files0['r_precision.json'].decode())
    assert sh.same_states(states1, states0)
    _check_result(algo1, files1, 6)
    reset_cfg()


def test_sampling_with_fid_through_the_bert_trainer(tmp_path):
    from miscc.config import reset_cfg
    make, loader, ds, (ckpt,) = sh.setup(tmp_path, ('out',), bert=True)
    algo, files, _, calls = sh.sample(make, loader, ds, ckpt, fid=True)
    assert len(files) == 7 and calls == 6
    _check_result(algo, files, 6)
    reset_cfg()
