"""Kernel Inception Distance on the GPU: the float64 kernel-sum kernel through ops.kid_kernel_sums and through the raw C
ABI -- exactly equal to the numpy reference (tests/kid_ref.py) on integer-valued features, within a derived bound on
real-valued ones -- reproducibility, the column splits, null index vectors, padded and offset row buffers, indices out
of range, the refusals, the KID class with a stub feature callable, and sampling() with --kid through both trainers."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import kid_ref
import sampling_harness as sh

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
U = 2.0 ** -53                  # unit roundoff of float64
E_ARG = -1
SENTINEL = -7.0


def dev(x):
    return torch.tensor(np.asarray(x), device=DEV)


def host(t):
    return t.cpu().numpy()


def ops_sums(a, b, ia=None, ib=None, exclude_diag=False, splits=0):
    from sbagan import ops
    s = ops.kid_kernel_sums(a, b, ia, ib, exclude_diag=exclude_diag, splits=splits)
    want = 1 if ia is None and ib is None else len(ia if ia is not None else ib)
    assert s.dtype == torch.float64 and tuple(s.shape) == (want,) and s.device == a.device
    return s


def raw_sums(a, b, ia, ib, ma, mb, subsets, exclude_diag=0, splits=0):
    """the C entry point itself: (return code, sums [subsets] pre-filled with SENTINEL); ia / ib: int32 device tensors
    or None"""
    from sbagan import _lib
    nbytes = _lib.lib.sba_kid_workspace_bytes(ma, mb, subsets, splits)
    assert nbytes >= 0
    ws = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=DEV)
    sums = torch.full((subsets,), SENTINEL, dtype=torch.float64, device=DEV)
    rc = _lib.lib.sba_kid_kernel_sums(a.data_ptr(), a.shape[0], a.stride(0), None if ia is None else ia.data_ptr(), ma,
                                      b.data_ptr(), b.shape[0], b.stride(0), None if ib is None else ib.data_ptr(), mb,
                                      a.shape[1], subsets, exclude_diag, splits, sums.data_ptr(), ws.data_ptr(), nbytes,
                                      torch.cuda.current_stream().cuda_stream)
    return rc, sums


def subsets_of(n, m, S, seed):
    """[S][m] int32: rows without replacement within a subset; n is little more than m, so the subsets share rows
    (certainly once 2 m > n)"""
    rng = np.random.RandomState(seed)
    return np.stack([rng.choice(n, m, replace=False) for _ in range(S)]).astype(np.int32)


def sum_bound_rel(D, P):
    """|S - S_ref| <= 2 (3 D + P + 8) U S_ref for a sum of P positive terms: each term's dot product takes D
    accumulations, the cube triples its relative error, P additions follow, and the reference is allowed the same"""
    return 2.0 * (3 * D + P + 8) * U


# ------------------------------------------------------------------ exactness on integer-valued features
# Values in -3 .. 3 at D = 64, 128 and in {0, 1} at D = 2048: g / D has at most 11 fractional bits and |t| <= 10, so
# t^3 and every partial sum of at most 130^2 of them are exactly representable: any summation order gives the same bits.
# m = 2: the fewest rows; 63, 64, 65: below, on and above the tile edge; 130: three row blocks and three column tiles.
EXACT = [(D, m, S) for D in (64, 128, 2048) for m in (2, 63, 64, 65, 130) for S in (1, 3)]
OTHER = {2: 65, 63: 130, 64: 65, 65: 130, 130: 63}


def int_features(n, D, seed):
    rng = np.random.RandomState(seed)
    return (rng.randint(0, 2, size=(n, D)) if D == 2048 else rng.randint(-3, 4, size=(n, D))).astype(np.float32)


@pytest.mark.parametrize('D,m,S', EXACT)
def test_integer_features_are_exact(D, m, S):
    mb = OTHER[m]
    na, nb = m + 7, mb + 5                                      # gathered from buffers of n > m rows
    A, B = int_features(na, D, 1000 * D + 10 * m + S), int_features(nb, D, 77 * D + m + S)
    ia, ja, ib = subsets_of(na, m, S, m), subsets_of(na, m, S, m + 1), subsets_of(nb, mb, S, m + 2)
    a, b = dev(A), dev(B)
    want_xx = torch.tensor(kid_ref.kernel_sums(A, A, ia, ja, exclude_diag=True))
    want_full = torch.tensor(kid_ref.kernel_sums(A, A, ia, ja))
    want_xy = torch.tensor(kid_ref.kernel_sums(A, B, ia, ib))
    assert (want_xx != want_full).all()                         # the diagonal matters in these cases
    ia_d, ja_d, ib_d = dev(ia), dev(ja), dev(ib)
    for splits in (0, 1, 2, 3):
        assert torch.equal(ops_sums(a, a, ia, ja, True, splits).cpu(), want_xx), splits
        assert torch.equal(ops_sums(a, a, ia, ja, False, splits).cpu(), want_full), splits
        assert torch.equal(ops_sums(a, b, ia, ib, False, splits).cpu(), want_xy), splits
        for got, want in ((raw_sums(a, a, ia_d, ja_d, m, m, S, 1, splits), want_xx),
                          (raw_sums(a, b, ia_d, ib_d, m, mb, S, 0, splits), want_xy)):
            assert got[0] == 0 and torch.equal(got[1].cpu(), want), splits


# ------------------------------------------------------------------ real-valued features against float64 numpy
REAL = [(192, 65, 2), (2048, 130, 1)]


@functools.lru_cache(maxsize=None)
def real_case(D, m, S):
    """(X, Y, ix, iy, reference sums): non-negative rows, as the pooled trunk's are; computed once per case"""
    rng = np.random.RandomState(D + m)
    X = (np.abs(rng.randn(m + 9, D)) * 0.4).astype(np.float32)
    Y = (np.abs(rng.randn(m + 4, D)) * 0.4).astype(np.float32)
    ix, iy = subsets_of(m + 9, m, S, 1), subsets_of(m + 4, m, S, 2)
    ref = {'xx': kid_ref.kernel_sums(X, X, ix, ix, exclude_diag=True),
           'yy': kid_ref.kernel_sums(Y, Y, iy, iy, exclude_diag=True), 'xy': kid_ref.kernel_sums(X, Y, ix, iy)}
    for v in (X, Y, ix, iy) + tuple(ref.values()):
        v.setflags(write=False)
    return X, Y, ix, iy, ref


def _three_terms(X, Y, ix, iy, splits=0):
    x, y = dev(X), dev(Y)
    return {'xx': host(ops_sums(x, x, ix, ix, True, splits)), 'yy': host(ops_sums(y, y, iy, iy, True, splits)),
            'xy': host(ops_sums(x, y, ix, iy, False, splits))}


@pytest.mark.parametrize('D,m,S', REAL)
def test_real_features_within_the_derived_bound(D, m, S):
    X, Y, ix, iy, ref = real_case(D, m, S)
    got = _three_terms(X, Y, ix, iy)
    bound = sum_bound_rel(D, m * m)
    for term in ('xx', 'yy', 'xy'):
        assert (ref[term] > 0).all()
        err = np.abs(got[term] - ref[term]) / ref[term]
        print('%s: relative error %.3g, bound %.3g' % (term, err.max(), bound))
        assert (err <= bound).all()


def test_launches_repeat_bit_for_bit_and_splits_agree_within_the_bound():
    D, m, S = REAL[0]
    X, Y, ix, iy, ref = real_case(D, m, S)
    bound = sum_bound_rel(D, m * m)
    first = _three_terms(X, Y, ix, iy, splits=2)
    again = _three_terms(X, Y, ix, iy, splits=2)
    for term in first:
        assert np.array_equal(first[term].view(np.int64), again[term].view(np.int64))
    for splits in (0, 1, 3, 32):                                # (32 is capped at the two tiles there are)
        other = _three_terms(X, Y, ix, iy, splits=splits)
        for term in first:
            assert (np.abs(other[term] - first[term]) <= bound * ref[term]).all(), (splits, term)


# ------------------------------------------------------------------ layout and indexing
def test_null_index_vectors_are_the_rows_in_order():
    A, B = np.abs(int_features(70, 64, 1)), np.abs(int_features(130, 64, 2))
    A, B = A * np.float32(0.37), B * np.float32(0.61)           # not exact any more: the ORDER of the sums must agree
    a, b = dev(A), dev(B)
    ar_a, ar_b = np.arange(70, dtype=np.int32)[None], np.arange(130, dtype=np.int64)[None]
    for splits in (0, 1, 2):
        for x, y, ix, iy, excl in ((a, b, ar_a, ar_b, False), (a, a, ar_a, ar_a, True)):
            explicit = ops_sums(x, y, ix, iy, excl, splits)
            assert torch.equal(ops_sums(x, y, None, None, excl, splits), explicit)
            assert torch.equal(ops_sums(x, y, ix, None, excl, splits), explicit)
            assert torch.equal(ops_sums(x, y, None, iy, excl, splits), explicit)
    # one side null, the other with three subsets: the null side is every row for each of them
    ia = subsets_of(70, 40, 3, 5)
    got = ops_sums(a, b, ia, None)
    assert torch.equal(got, ops_sums(a, b, ia, np.repeat(ar_b, 3, axis=0)))
    want = kid_ref.kernel_sums(A, B, ia, None)                  # (non-negative rows: every term is positive)
    assert (np.abs(host(got) - want) <= sum_bound_rel(64, 40 * 130) * want).all()


def test_row_stride_larger_than_the_width_and_a_buffer_at_an_offset():
    A, B = int_features(72, 128, 7), int_features(21, 128, 8)
    ia, ib = subsets_of(72, 65, 2, 1), subsets_of(21, 20, 2, 2)
    want = torch.tensor(kid_ref.kernel_sums(A, B, ia, ib))
    wide_a = torch.full((72, 136), 1e30, device=DEV)            # ld = 136: the 8 extra columns must never be read
    wide_b = torch.full((30, 132), 1e30, device=DEV)
    wide_a[:, :128] = dev(A)
    wide_b[4:25, 4:] = dev(B)                                   # rows 4 .. 24, columns 4 .. 131: offset both ways
    view_a, view_b = wide_a[:, :128], wide_b[4:25, 4:]
    assert view_b.data_ptr() % 16 == 0 and view_b.data_ptr() != wide_b.data_ptr()
    for splits in (1, 2):
        assert torch.equal(ops_sums(view_a, view_b, ia, ib, False, splits).cpu(), want)
    want_xx = torch.tensor(kid_ref.kernel_sums(A, A, ia, ia, exclude_diag=True))
    assert torch.equal(ops_sums(view_a, view_a, ia, ia, True).cpu(), want_xx)


def test_the_same_rows_as_both_operands_equal_a_separate_copy():
    X, _, ix, _, _ = real_case(*REAL[0])
    x = dev(X)
    assert torch.equal(ops_sums(x, x, ix, ix, True), ops_sums(x, x.clone(), ix, ix, True))
    assert torch.equal(ops_sums(x, x, None, None, True), ops_sums(x, x.clone(), None, None, True))


# ------------------------------------------------------------------ bounds
def test_indices_out_of_range_and_positions_past_the_end_read_nothing():
    """The rows lie in the middle of a tensor whose other rows are NaN; the index vectors hold -1, n and other row
    numbers just outside [0, n), and m = 70 leaves 58 positions past the end in the last tile (of subset 0 they are
    the first positions of subset 1 in memory).  All of those are zero rows left out of the sum: the sums equal the
    reference and are finite.  Through the C entry point: the wrapper refuses such indices."""
    n, m, S, D = 80, 70, 2, 64
    A, B = int_features(n, D, 3), int_features(n, D, 4)
    big_a = torch.full((n + 24, D), float('nan'), device=DEV)
    big_b = torch.full((n + 24, D), float('nan'), device=DEV)
    big_a[12:12 + n] = dev(A)
    big_b[12:12 + n] = dev(B)
    a, b = big_a[12:12 + n], big_b[12:12 + n]
    ia, ib = subsets_of(n, m, S, 1), subsets_of(n, m, S, 2)
    for idx in (ia, ib):
        idx[0, 0], idx[0, 5], idx[0, 63], idx[0, 64], idx[0, 69] = -1, n, -12, n + 11, n + 1
        idx[1, 1], idx[1, 68] = n + 3, -2
    ib[0, 5], ib[0, 6] = ib[0, 6], n                           # not the same bad positions on both sides
    for splits in (0, 1, 2):
        for excl, x, y, ix, iy, X, Y in ((0, a, b, ia, ib, A, B), (1, a, a, ia, ib, A, A), (1, b, b, ib, ib, B, B)):
            want = kid_ref.kernel_sums(X, Y, ix, iy, exclude_diag=bool(excl))
            rc, got = raw_sums(x, y, dev(ix), dev(iy), m, m, S, excl, splits)
            got = host(got)
            assert rc == 0 and np.isfinite(got).all() and np.array_equal(got, want), (splits, excl)
    # null index vectors with m > n: the positions n .. m - 1 name rows past the end of the set
    rc, got = raw_sums(a, b, None, None, n + 10, n + 7, 1, 0, 0)
    assert rc == 0 and host(got)[0] == kid_ref.kernel_sum(A, B)


# ------------------------------------------------------------------ refusals, all before any launch
def test_wrapper_refusals():
    from sbagan import ops
    x = torch.ones(8, 64, device=DEV)
    i4 = np.zeros((2, 4), dtype=np.int32)
    with pytest.raises(ValueError):
        ops.kid_kernel_sums(torch.ones(8, 100, device=DEV), torch.ones(8, 100, device=DEV))     # D = 100
    with pytest.raises(ValueError):
        ops.kid_kernel_sums(x, torch.ones(8, 128, device=DEV))                      # widths differ
    with pytest.raises(TypeError):
        ops.kid_kernel_sums(x, x.double())
    with pytest.raises(RuntimeError):
        ops.kid_kernel_sums(x, x.cpu())
    with pytest.raises(ValueError):
        ops.kid_kernel_sums(torch.ones(8, 64, 1, device=DEV), x)                    # 3-D
    with pytest.raises(ValueError):
        ops.kid_kernel_sums(torch.ones(64, 8, device=DEV).t(), x)                   # column stride != 1
    with pytest.raises(ValueError):
        ops.kid_kernel_sums(torch.ones(8, 66, device=DEV)[:, :64], x)               # row stride 66
    with pytest.raises(ValueError):
        ops.kid_kernel_sums(torch.ones(8, 68, device=DEV)[:, 1:65], x)              # misaligned
    for splits in (33, -1, 1.0, True):
        with pytest.raises(ValueError):
            ops.kid_kernel_sums(x, x, splits=splits)
    with pytest.raises(ValueError):
        ops.kid_kernel_sums(x, x[:5], exclude_diag=True)                            # ma != mb
    with pytest.raises(ValueError):
        ops.kid_kernel_sums(x, x, i4, np.zeros((2, 5), dtype=np.int32), exclude_diag=True)
    with pytest.raises(ValueError):
        ops.kid_kernel_sums(x, x, i4, np.zeros((3, 4), dtype=np.int32))             # subset counts differ
    with pytest.raises(ValueError):
        ops.kid_kernel_sums(x, x, np.zeros((1025, 2), dtype=np.int32))              # too many subsets
    for bad in (8, -1):
        idx = i4.copy()
        idx[1, 2] = bad
        with pytest.raises(ValueError, match='outside'):
            ops.kid_kernel_sums(x, x, idx, i4)
        with pytest.raises(ValueError, match='outside'):
            ops.kid_kernel_sums(x, x[:5], i4, np.where(idx == 8, 5, idx))           # checked against ITS row count
    with pytest.raises(TypeError):
        ops.kid_kernel_sums(x, x, i4.astype(np.float32))
    with pytest.raises(ValueError):
        ops.kid_kernel_sums(x, x, i4[0])                                            # 1-D
    with pytest.raises(ValueError):
        ops.kid_kernel_sums(x, x, torch.zeros(2, 4, dtype=torch.int32, device=DEV))     # indices come from the host


def test_c_abi_refusals():
    from sbagan import _lib
    fn, size = _lib.lib.sba_kid_kernel_sums, _lib.lib.sba_kid_workspace_bytes
    x = torch.ones(200, 128, device=DEV)
    idx = torch.zeros(3 * 200, dtype=torch.int32, device=DEV)
    sums = torch.full((1024,), SENTINEL, dtype=torch.float64, device=DEV)
    ws = torch.zeros(4096, dtype=torch.float64, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    X, I, O, W, full = x.data_ptr(), idx.data_ptr(), sums.data_ptr(), ws.data_ptr(), ws.numel() * 8
    assert size(200, 200, 3, 2) == 3 * 4 * 2 * 8 <= full

    def call(a=X, na=200, lda=128, ia=I, ma=200, b=X, nb=200, ldb=128, ib=I, mb=200, D=128, subsets=3, excl=0, splits=2,
             out=O, w=W, wbytes=full):
        return fn(a, na, lda, ia, ma, b, nb, ldb, ib, mb, D, subsets, excl, splits, out, w, wbytes, st)
    bad = [dict(a=None), dict(b=None), dict(out=None), dict(a=X + 4), dict(b=X + 8), dict(out=O + 4),
           dict(ia=I + 2), dict(ib=I + 1),
           dict(D=100), dict(D=0), dict(D=32), dict(D=192),                         # D % 64, D < 64, D > ld
           dict(lda=64), dict(ldb=130), dict(lda=130),                              # ld < D, ld % 4
           dict(na=0), dict(nb=0), dict(ma=0), dict(mb=0), dict(ma=-3),
           dict(subsets=0), dict(subsets=1025), dict(splits=-1), dict(splits=33),
           dict(excl=1, mb=199),                                                    # the diagonal needs ma == mb
           dict(w=None), dict(w=W + 4), dict(wbytes=size(200, 200, 3, 2) - 1), dict(wbytes=0)]
    for kw in bad:
        assert call(**kw) == E_ARG, kw
    torch.cuda.synchronize()
    assert (host(sums) == SENTINEL).all() and (host(ws) == 0).all()
    assert call() == 0 and call(excl=1) == 0 and call(ia=None, ib=None) == 0        # and the good call is taken
    assert call(ma=64, mb=64, splits=1, w=None, wbytes=0) == 0                      # one partial a subset: no workspace
    torch.cuda.synchronize()
    assert (host(sums)[:3] != SENTINEL).all() and (host(sums)[3:] == SENTINEL).all()


# ------------------------------------------------------------------ the KID class with a stub feature callable
def kid_tolerance(sxx, syy, sxy, m, D):
    """per subset: the three sums' bounds divided by their normalisers and added"""
    b = sum_bound_rel(D, m * m)
    return b * (np.abs(sxx) / (m * (m - 1.0)) + np.abs(syy) / (m * (m - 1.0)) + 2.0 * np.abs(sxy) / (float(m) * m))


def reference_result(R, F, ir, jf):
    """({'kid', 'kid_std'}, tolerance of kid, tolerance of kid_std) on the given subsets: the mean moves by at most the
    mean of the per-subset tolerances, the population deviation by at most their largest"""
    m, D = ir.shape[1], R.shape[1]
    tol = kid_tolerance(kid_ref.kernel_sums(R, R, ir, ir, exclude_diag=True),
                        kid_ref.kernel_sums(F, F, jf, jf, exclude_diag=True), kid_ref.kernel_sums(R, F, ir, jf), m, D)
    return kid_ref.kid(R, F, ir, jf), tol.mean(), tol.max()


def _feed(ev, side, x, update_features=False):
    import test_prdc_gpu as tp
    tp._feed(ev, side, x, update_features)                      # batches of 20, 20, 7, 1, 20, ... rows


def _check_against_reference(res, R, F, ir, jf):
    want, tol_kid, tol_std = reference_result(R, F, ir, jf)
    print('kid %.9g (reference %.9g, tolerance %.3g)  kid_std %.9g (reference %.9g, tolerance %.3g)'
          % (res['kid'], want['kid'], tol_kid, res['kid_std'], want['kid_std'], tol_std))
    assert math.isfinite(res['kid']) and math.isfinite(res['kid_std'])
    assert abs(res['kid'] - want['kid']) <= tol_kid and abs(res['kid_std'] - want['kid_std']) <= tol_std


def test_kid_class_with_stub_features():
    from sbagan.kid import FIELDS, KID, draw_subsets
    from sbagan.prdc import PRDC
    rng = np.random.RandomState(11)
    nr, nf, D = 150, 97, 128
    R = (np.abs(rng.randn(nr, D)) * 0.4).astype(np.float32)
    F = (np.abs(0.9 * rng.randn(nf, D) + 0.3) * 0.4).astype(np.float32)
    calls = []

    def features(images):           # the stub "trunk": the images are the feature rows
        calls.append(images.shape[0])
        return images

    ev = KID(features, D=D, subsets=5, subset_size=70, seed=9, dtype='float32', capacity=16)    # four growths a side
    _feed(ev, 'real', dev(R))
    _feed(ev, 'fake', dev(F), update_features=True)
    assert sum(calls) == nr and ev.count('real') == nr and ev.count('fake') == nf
    assert np.array_equal(host(ev.rows('real')), R) and np.array_equal(host(ev.rows('fake')), F)
    res = ev.result()
    print(res)
    assert sorted(res) == sorted(FIELDS) and json.loads(json.dumps(res)) == res
    assert (res['subsets'], res['subset_size'], res['n_real'], res['n_fake']) == (5, 70, nr, nf)
    assert (res['degree'], res['coef0'], res['gamma'], res['dtype'], res['seed']) == (3, 1.0, 1.0 / D, 'float32', 9)
    ir, jf = draw_subsets(nr, nf, 70, 5, 9)
    _check_against_reference(res, R, F, ir, jf)
    assert res['kid'] > 0.0 and res['kid_std'] > 0.0            # the two sides differ, and so do the subsets
    assert ev.result() == res                                   # the draws start from the seed every time

    # a subset size above a side's row count is clamped to that side
    big = KID(features, D=D, subsets=3, subset_size=1000, seed=9, dtype='float32')
    big.update_features('real', dev(R))
    big.update_features('fake', dev(F))
    res_big = big.result()
    assert res_big['subset_size'] == nf
    _check_against_reference(res_big, R, F, *draw_subsets(nr, nf, nf, 3, 9))

    # rows=<a PRDC>: one buffer, the same result
    prdc = PRDC(features, D=D, k=3, dtype='float32', capacity=16)
    shared = KID(features, D=D, subsets=5, subset_size=70, seed=9, dtype='float32', rows=prdc)
    _feed(prdc, 'real', dev(R), update_features=True)
    _feed(prdc, 'fake', dev(F), update_features=True)
    for side in ('real', 'fake'):
        assert shared.count(side) == prdc.count(side)
        assert shared.rows(side).data_ptr() == prdc.rows(side).data_ptr()
    assert shared.result() == res
    with pytest.raises(RuntimeError):
        shared.update_features('real', dev(R))
    with pytest.raises(ValueError):
        KID(features, D=64, rows=prdc)

    with pytest.raises(TypeError):
        ev.update('fake', dev(F).double())
    with pytest.raises(ValueError):
        ev.update('fake', torch.zeros(3, 64, device=DEV))
    with pytest.raises(ValueError):
        ev.update('both', dev(F))
    few = KID(features, D=D, subsets=2)
    few.update('real', dev(R))
    with pytest.raises(RuntimeError, match='fake side holds 0 rows'):
        few.result()
    few.update('fake', dev(F[:1]))
    with pytest.raises(RuntimeError, match='fake side holds 1 rows'):
        few.result()
    few.update('fake', dev(F[1:2]))                             # two rows: the fewest a subset can have
    assert few.result()['subset_size'] == 2


# ------------------------------------------------------------------ sampling() with the flag
SUBSETS, SUBSET_SIZE = 4, 5         # of the 6 toy images a side: the subsets differ, so kid_std is not trivially 0


def _sample(make, loader, ds, ckpt, **attrs):
    """sampling_harness.sample with the subset settings of these tests"""
    return sh.sample(make, loader, ds, ckpt, kid_subsets=SUBSETS, kid_subset_size=SUBSET_SIZE, **attrs)


def _check_result(algo, files, n_images):
    from sbagan.kid import FIELDS, draw_subsets
    res = json.loads(files['kid.json'].decode())
    print('kid.json:', res)
    assert res == algo.kid_result and sorted(res) == sorted(FIELDS)
    assert (res['n_real'], res['n_fake']) == (n_images, n_images)
    assert (res['subsets'], res['subset_size']) == (SUBSETS, SUBSET_SIZE)
    assert (res['dtype'], res['seed'], res['degree'], res['coef0'], res['gamma']) == ('bfloat16', 100, 3, 1.0, 1.0 / 2048)
    ev = algo.kid_evaluator
    R, F = host(ev.rows('real')), host(ev.rows('fake'))
    assert R.shape == (n_images, 2048) and F.shape == (n_images, 2048) and R.dtype == np.float32
    _check_against_reference(res, R, F, *draw_subsets(n_images, n_images, SUBSET_SIZE, SUBSETS, 100))
    return res


def test_sampling_without_and_with_the_flag(tmp_path):
    from miscc.config import reset_cfg
    make, loader, ds, ckpts = sh.setup(tmp_path, ('without', 'with'))
    algo0, files0, states0, calls0 = _sample(make, loader, ds, ckpts[0])
    algo1, files1, states1, calls1 = _sample(make, loader, ds, ckpts[1], kid=True)
    assert algo0.kid_result is None and calls0 == 0 and len(files0) == 6 and all(k.endswith('.png') for k in files0)
    # the same image files, byte for byte, and kid.json beside them
    assert sorted(files1) == sorted(list(files0) + ['kid.json']) and sh.images(files1) == files0
    # the flag consumes none of the randomness the data path and the noise draw from
    assert sh.same_states(states1, states0)
    _check_result(algo1, files1, 6)
    assert calls1 == 3 + 3                          # one trunk forward per generated and per real batch
    reset_cfg()


def test_sampling_with_every_evaluator_shares_the_forwards_and_the_rows(tmp_path):
    from miscc.config import reset_cfg
    make, loader, ds, ckpts = sh.setup(tmp_path, ('three', 'four', 'cached'))
    stats = str(tmp_path / 'real.npz')
    algo0, files0, states0, calls0 = _sample(make, loader, ds, ckpts[0], prdc=3, fid=True, fid_stats=stats, r_precision=4)
    algo1, files1, states1, calls1 = _sample(make, loader, ds, ckpts[1], kid=True, prdc=3, fid=True, r_precision=4)
    assert calls0 == 3 + 3 and os.path.exists(stats)
    assert calls1 == 3 + 3                          # each batch goes through the trunk ONCE for all four evaluators
    assert sorted(files1) == sorted(list(files0) + ['kid.json']) and sh.images(files1) == sh.images(files0)
    for name in ('fid.json', 'prdc.json', 'r_precision.json'):
        assert json.loads(files1[name].decode()) == json.loads(files0[name].decode())
    assert sh.same_states(states1, states0)
    res1 = _check_result(algo1, files1, 6)
    for side in ('real', 'fake'):                   # with --prdc the rows are stored once
        assert algo1.kid_evaluator.rows(side).data_ptr() == algo1.prdc_evaluator.rows(side).data_ptr()
    # cached real FID statistics: FID skips its real pass, the real batches are encoded for KID alone
    algo2, files2, states2, calls2 = _sample(make, loader, ds, ckpts[2], kid=True, fid=True, fid_stats=stats, r_precision=4)
    assert calls2 == 3 + 3
    assert _check_result(algo2, files2, 6) == res1
    assert json.loads(files2['fid.json'].decode()) == json.loads(files0['fid.json'].decode())
    assert sh.images(files2) == sh.images(files0) and sh.same_states(states2, states0)
    reset_cfg()


def test_sampling_with_kid_through_the_bert_trainer(tmp_path):
    from miscc.config import reset_cfg
    make, loader, ds, (ckpt,) = sh.setup(tmp_path, ('out',), bert=True)
    algo, files, _, calls = _sample(make, loader, ds, ckpt, kid=True)
    assert len(files) == 7 and calls == 6
    _check_result(algo, files, 6)
    reset_cfg()
