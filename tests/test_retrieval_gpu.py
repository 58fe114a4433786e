"""Image-caption retrieval on the GPU: the float64 score-and-rank kernels through ops.retrieval_own_best /
ops.retrieval_counts -- exactly equal to the numpy reference (tests/retrieval_ref.py) on integer-valued features, within
the derived bound (best) and exactly (counts) on real-valued ones -- the bitwise properties of the score (column split,
repeated launches, either set as the query side), ties, NaN and infinite rows, a padded row stride, the refusals of the
wrapper and of the C ABI, the Retrieval class with stub codes, and --retrieval / --retrieval_only through
pretrain_DAMSM.main and pretrain_DAMSM_bert.main on a toy directory."""
import functools
import glob
import json
import os
import random
import re

import numpy as np
import pytest
import torch

import retrieval_ref as ref

pytestmark = pytest.mark.gpu

from test_host_cpu import _make_dataset  # noqa: E402

DEV = 'cuda:0'
GUARD = 16                      # elements around every output of a refused call, checked untouched


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_f64(a, b):
    """bit-equal where both are numbers, NaN where either is"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a[~nan]), bits(b[~nan]))


def dev(x):
    return None if x is None else torch.tensor(np.asarray(x), device=DEV)


def keys(v):
    return None if v is None else torch.tensor(np.asarray(v, dtype=np.int32), device=DEV)


def gpu_best(A, B, ka, kb, splits=0, eps=ref.EPS):
    from sbagan import ops
    best = ops.retrieval_own_best(dev(A), dev(B), keys(ka), keys(kb), eps, splits)
    assert best.dtype == torch.float64 and tuple(best.shape) == (A.shape[0],)
    return best.cpu().numpy()


def gpu_counts(A, B, ka, kb, best, ca=None, cb=None, splits=0, eps=ref.EPS):
    from sbagan import ops
    above, masked = ops.retrieval_counts(dev(A), dev(B), keys(ka), keys(kb), dev(np.asarray(best, dtype=np.float64)),
                                         keys(ca), keys(cb), eps, splits)
    for t in (above, masked):
        assert t is None or (t.dtype == torch.int32 and tuple(t.shape) == (A.shape[0],))
    return above.cpu().numpy(), None if masked is None else masked.cpu().numpy()


# ------------------------------------------------------------------ exactness on integer-valued features
# Small integers: dot products, squared norms and the product of two norms are integers far below 2^53, exact in any
# order; square root and division are correctly rounded on both sides.  na, nb: 1; 63, 64, 65: one below, on and one
# above the tile edge; 130, 200: three and four tiles, the last a partial one.  D = 64: two staged chunks, 256: eight.
SHAPES = [(1, 1), (1, 130), (63, 65), (64, 64), (65, 200), (130, 1)]


@functools.lru_cache(maxsize=None)
def int_case(D, na, nb):
    """rows, keys, classes and what the reference makes of them.  key_b[j] = j % (na + 1): a query owns the rows j = i,
    i + na + 1, ... -- none, one or several, in different tiles and splits once nb > 64 -- and the key na belongs to no
    query; every 11th query from the 4th has a key of no row at all (best = -inf, every row counts), and the last query
    shares the key of the first.  The last B row repeats the first: exact ties among the candidates."""
    rng = np.random.RandomState(1000 * D + 10 * na + nb)
    A = rng.randint(-8, 9, size=(na, D)).astype(np.float32)
    B = rng.randint(-8, 9, size=(nb, D)).astype(np.float32)
    if nb > 1:
        B[nb - 1] = B[0]
    ka = np.arange(na, dtype=np.int32)
    ka[3::11] = -5
    if na > 1:
        ka[na - 1] = ka[0]
    kb = (np.arange(nb) % (na + 1)).astype(np.int32)
    ca, cb = (np.arange(na) % 3).astype(np.int32), ((np.arange(nb) // 2) % 3).astype(np.int32)
    S = ref.scores(A, B)
    best = ref.own_best(S, ka, kb)
    above, masked = ref.counts(S, ka, kb, best, ca, cb)
    for v in (A, B, ka, kb, ca, cb, S, best, above, masked):
        v.setflags(write=False)
    return A, B, ka, kb, ca, cb, best, above, masked


def test_the_integer_cases_cover_the_key_patterns():
    own = {}
    for na, nb in SHAPES:
        _, _, ka, kb, _, _, best, above, _ = int_case(64, na, nb)
        n_own = (kb[None, :] == ka[:, None]).sum(1)
        own[(na, nb)] = set(np.minimum(n_own, 2).tolist())
        assert np.array_equal(np.isneginf(best), n_own == 0)
        assert (above[n_own == 0] == nb).all()
    assert own[(1, 1)] == {1} and own[(64, 64)] >= {0, 1} and own[(130, 1)] == {0, 1}
    assert own[(1, 130)] == {2} and own[(65, 200)] == {0, 2} and own[(63, 65)] == {0, 1, 2}
    _, _, ka, kb, _, _, _, _, _ = int_case(64, 65, 200)
    mine = np.flatnonzero(kb == ka[1])
    assert mine.tolist() == [1, 67, 133, 199] and len(set(mine // 64)) == 4  # four tiles: every part of splits = 2, 3


@pytest.mark.parametrize('splits', [0, 1, 2, 3])
@pytest.mark.parametrize('na,nb', SHAPES)
@pytest.mark.parametrize('D', [64, 256])
def test_integer_features_are_exact(D, na, nb, splits):
    A, B, ka, kb, ca, cb, best, above, masked = int_case(D, na, nb)
    got = gpu_best(A, B, ka, kb, splits)
    assert np.array_equal(bits(got), bits(best))
    a, m = gpu_counts(A, B, ka, kb, got, ca, cb, splits)
    assert np.array_equal(a, above) and np.array_equal(m, masked)


# ------------------------------------------------------------------ real-valued features against float64
# retrieval_ref.score_bound(D) = (D + D / 8 + 12) U bounds |s_kernel - s_reference| (derived in test_retrieval_cpu.py);
# the own best is a maximum of such scores and moves by no more.  A count is EQUAL to the reference's wherever no
# candidate's score lies within twice the bound of the query's threshold, which the test asserts first on the reference
# alone.  (ni, captions per image, D, images per class): the seeds were chosen on the CPU so that this holds.
REAL = [(70, 3, 64, 4), (65, 2, 256, 5)]
SEED = {70: 0, 65: 1}


@functools.lru_cache(maxsize=None)
def real_case(ni, per, D, group):
    """normalised Gaussian rows, each caption its image's row at weight 1 / sqrt(D) plus noise: the own score lies about
    one standard deviation of the other scores above them, so the ranks range from 0 far upwards"""
    rng = np.random.RandomState(SEED[ni])
    X = rng.randn(ni, D)
    owner = np.arange(ni * per) // per
    Y = X[owner] / np.sqrt(D) + rng.randn(ni * per, D)
    X, Y = (v / np.linalg.norm(v, axis=1, keepdims=True) for v in (X, Y))
    X, Y = X.astype(np.float32), Y.astype(np.float32)
    cls = (np.arange(ni) // group).astype(np.int64)
    r = ref.all_ranks(X, Y, owner, cls, exact=True)
    for v in list(r.values()) + [X, Y, owner, cls]:
        v.setflags(write=False)
    return X, Y, owner, cls, r


def min_gap(r, owner):
    """the smallest distance of a candidate's score from its query's threshold, own pairs left out, both directions"""
    S = r['scores']
    notown = owner[None, :] != np.arange(S.shape[0])[:, None]
    gi = np.abs(S - r['best'][:, None])[notown].min()
    gt = np.abs(S - r['thr'][None, :])[notown].min()
    return min(gi, gt)


@pytest.mark.parametrize('ni,per,D,group', REAL)
def test_real_features_best_within_the_bound_and_counts_equal(ni, per, D, group):
    X, Y, owner, cls, r = real_case(ni, per, D, group)
    bound = ref.score_bound(D)
    gap = min_gap(r, owner)
    print('D = %d: bound %.3e, smallest gap to a threshold %.3e' % (D, bound, gap))
    assert gap > 2 * bound
    assert r['i2t_instance'].max() > ni // 2 and r['i2t_instance'].min() == 0       # the ranks spread
    assert (r['i2t_class_masked'] != r['i2t_instance']).any()
    ki, kt, ci, ct = np.arange(ni), owner, cls, cls[owner]
    for splits in (0, 2):
        best = gpu_best(X, Y, ki, kt, splits)
        err = np.abs(best - r['best']).max()
        print('  splits %d: |best - reference| <= %.3e (%.3f of the bound)' % (splits, err, err / bound))
        assert err <= bound
        a, m = gpu_counts(X, Y, ki, kt, best, ci, ct, splits)
        assert np.array_equal(a, r['i2t_instance']) and np.array_equal(m, r['i2t_class_masked'])
        thr = gpu_best(Y, X, kt, ki, splits)
        assert np.abs(thr - r['thr']).max() <= bound
        a, m = gpu_counts(Y, X, kt, ki, thr, ct, ci, splits)
        assert np.array_equal(a, r['t2i_instance']) and np.array_equal(m, r['t2i_class_masked'])


# ------------------------------------------------------------------ bitwise properties of the score
def test_scores_have_the_same_bits_for_every_split_launch_and_side():
    X, Y, owner, cls, r = real_case(*REAL[0])
    ni, nt = X.shape[0], Y.shape[0]
    ki, kt = np.arange(ni), owner
    best = gpu_best(X, Y, ki, kt, 1)
    thr = gpu_best(Y, X, kt, ki, 1)
    for splits in (0, 1, 2, 3, 4, 32):
        for _ in range(2):
            assert np.array_equal(bits(gpu_best(X, Y, ki, kt, splits)), bits(best)), splits
            assert np.array_equal(bits(gpu_best(Y, X, kt, ki, splits)), bits(thr)), splits
    # images as the query side against captions as the query side: thr[t] IS s(owner[t], t), and best[i] the largest of
    # its captions' -- the same bits, not merely close
    assert np.array_equal(bits(best), bits(np.array([thr[owner == i].max() for i in range(ni)])))
    # every single score, through the threshold: with the one key pattern "row j of B belongs to query (j - k) mod ni"
    # best[i] is s(i, (i + k) mod nt); both sides must agree on it for every k tried
    Yk = Y[:ni]
    for k in (0, 1, 17, 69):
        kb = ((np.arange(ni) - k) % ni).astype(np.int32)            # row j is owned by query j - k
        fwd = gpu_best(X, Yk, np.arange(ni), kb)                     # fwd[i] = s(x_i, y_{i + k})
        rev = gpu_best(Yk, X, kb, np.arange(ni))                     # rev[j] = s(y_j, x_{j - k})
        assert np.array_equal(bits(fwd), bits(rev[(np.arange(ni) + k) % ni])), k
    # the counts are the same for every split as well
    want = gpu_counts(X, Y, ki, kt, best, cls, cls[owner], 1)
    for splits in (0, 2, 3, 32):
        got = gpu_counts(X, Y, ki, kt, best, cls, cls[owner], splits)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_a_duplicate_of_an_own_caption_under_another_key_is_a_tie_that_counts():
    rng = np.random.RandomState(11)
    X = rng.randint(-8, 9, size=(5, 64)).astype(np.float32)
    Y = rng.randint(-8, 9, size=(10, 64)).astype(np.float32)
    owner, cls = np.arange(10) // 2, np.arange(5)
    Y[0] = Y[1] = 3 * X[0]                  # image 0's captions point its way: score 1, its best
    base = ref.all_ranks(X, Y, owner, cls)
    assert base['i2t_instance'][0] == 0
    Y[7] = Y[0]                             # the same row again, as a caption of image 3
    r = ref.all_ranks(X, Y, owner, cls)
    assert r['i2t_instance'][0] == 1 and r['best'][0] == 1.0
    best = gpu_best(X, Y, np.arange(5), owner)
    assert np.array_equal(bits(best), bits(r['best']))
    a, m = gpu_counts(X, Y, np.arange(5), owner, best, cls, cls[owner])
    assert np.array_equal(a, r['i2t_instance']) and np.array_equal(m, r['i2t_class_masked']) and a[0] == 1
    thr = gpu_best(Y, X, owner, np.arange(5))
    assert np.array_equal(bits(thr), bits(r['thr']))
    a, _ = gpu_counts(Y, X, owner, np.arange(5), thr, cls[owner], cls)
    assert np.array_equal(a, r['t2i_instance']) and a[7] >= 1      # image 0 beats image 3 on the copied caption


def test_nan_and_infinite_rows():
    rng = np.random.RandomState(12)
    X = rng.randint(-8, 9, size=(70, 64)).astype(np.float32)
    Y = rng.randint(-8, 9, size=(140, 64)).astype(np.float32)
    owner, cls = np.arange(140) // 2, np.arange(70) // 3
    X[5, 7] = np.nan
    X[66, 0] = np.inf
    X[67, 63] = -np.inf
    Y[3, 1] = np.nan                        # one of image 1's captions
    Y[100, 5] = np.inf                      # one of image 50's
    Y[139] = 0                              # a zero row scores 0, exactly
    r = ref.all_ranks(X, Y, owner, cls)
    assert np.isnan(r['best'][[1, 5, 50, 66, 67]]).all() and np.isnan(r['best']).sum() == 5
    assert (r['i2t_instance'][[1, 5, 50, 66, 67]] == 138).all()          # a NaN threshold: every candidate counts
    assert r['i2t_instance'][0] >= 2                                      # the NaN captions count against everyone
    assert (r['t2i_instance'][[3, 100]] == 69).all() and r['scores'][0, 139] == 0.0
    for splits in (1, 3):
        best = gpu_best(X, Y, np.arange(70), owner, splits)
        assert same_f64(best, r['best'])
        a, m = gpu_counts(X, Y, np.arange(70), owner, best, cls, cls[owner], splits)
        assert np.array_equal(a, r['i2t_instance']) and np.array_equal(m, r['i2t_class_masked'])
        thr = gpu_best(Y, X, owner, np.arange(70), splits)
        assert same_f64(thr, r['thr'])
        a, m = gpu_counts(Y, X, owner, np.arange(70), thr, cls[owner], cls, splits)
        assert np.array_equal(a, r['t2i_instance']) and np.array_equal(m, r['t2i_class_masked'])
    # thresholds of -inf, +inf and NaN given from outside
    thr = np.array([-np.inf, np.inf, np.nan] + [0.0] * 67)
    a, _ = gpu_counts(X, Y, np.arange(70), owner, thr)
    want, _ = ref.counts(r['scores'], np.arange(70), owner, thr)
    assert np.array_equal(a, want) and a[0] == 138 and a[2] == 138
    assert a[1] == np.isnan(np.delete(r['scores'][1], [2, 3])).sum() >= 1  # nothing but a NaN is "not below +inf"


def test_a_row_stride_larger_than_the_width_and_no_class_vectors():
    from sbagan import ops
    A, B, ka, kb, ca, cb, best, above, masked = int_case(64, 65, 200)
    wide_a = torch.full((65, 64 + 8), float('nan'), device=DEV)
    wide_b = torch.full((200, 64 + 64), float('nan'), device=DEV)
    wide_a[:, :64] = dev(A)
    wide_b[:, :64] = dev(B)
    a, b = wide_a[:, :64], wide_b[:, :64]
    assert a.stride(0) == 72 and b.stride(0) == 128
    for splits in (0, 1, 3):
        got = ops.retrieval_own_best(a, b, keys(ka), keys(kb), splits=splits)
        assert np.array_equal(bits(got.cpu().numpy()), bits(best))
        ab, m = ops.retrieval_counts(a, b, keys(ka), keys(kb), got, keys(ca), keys(cb), splits=splits)
        assert np.array_equal(ab.cpu().numpy(), above) and np.array_equal(m.cpu().numpy(), masked)
        ab, m = ops.retrieval_counts(a, b, keys(ka), keys(kb), got, splits=splits)
        assert m is None and np.array_equal(ab.cpu().numpy(), above)


def test_eps_is_the_floor_of_the_denominator():
    A = np.zeros((2, 64), dtype=np.float32)
    B = np.zeros((2, 64), dtype=np.float32)
    A[0, 0], A[1, 0], B[0, 0], B[1, 0] = 2.0 ** -20, 1.0, 2.0 ** -20, 2.0 ** -21     # |a||b| = 2^-40 < eps for (0, 0)
    k = np.arange(2)
    for eps in (1e-8, 0.5):
        want = ref.own_best(ref.scores(A, B, eps), k, k)
        assert np.array_equal(bits(gpu_best(A, B, k, k, eps=eps)), bits(want))
    assert ref.scores(A, B)[0, 0] == 2.0 ** -40 / 1e-8


# ------------------------------------------------------------------ refusals
def test_the_wrapper_refuses_before_any_launch(monkeypatch):
    from sbagan import _lib, ops
    A, B, ka, kb, ca, cb, best, _, _ = int_case(64, 65, 200)
    a, b, ka, kb, ca, cb, best = dev(A), dev(B), keys(ka), keys(kb), keys(ca), keys(cb), dev(best)

    def no_call(name, *args):
        raise AssertionError('a refusal reached %s' % name)
    monkeypatch.setattr(ops, 'call', no_call)
    monkeypatch.setattr(_lib, 'call', no_call)
    bad_best = [
        (TypeError, dict(a=a.double())), (TypeError, dict(a=A)), (TypeError, dict(key_a=ka.long())),
        (ValueError, dict(a=a[:, :63])), (ValueError, dict(a=dev(np.zeros((65, 96), np.float32)))),
        (ValueError, dict(b=dev(np.zeros((200, 128), np.float32)))), (ValueError, dict(a=a.t().contiguous().t())),
        (ValueError, dict(a=torch.zeros(65 * 64 + 1, device=DEV)[1:].view(65, 64))), (RuntimeError, dict(b=b.cpu())),
        (ValueError, dict(key_a=ka[:64])), (ValueError, dict(key_b=kb[::2])), (RuntimeError, dict(key_b=kb.cpu())),
        (ValueError, dict(splits=-1)), (ValueError, dict(splits=33)), (ValueError, dict(splits=1.0)),
        (ValueError, dict(eps=0.0)), (ValueError, dict(eps=float('nan'))), (ValueError, dict(a=a[:0])),
    ]
    for exc, change in bad_best:
        kw = dict(a=a, b=b, key_a=ka, key_b=kb)
        kw.update(change)
        with pytest.raises(exc):
            ops.retrieval_own_best(**kw)
    bad_counts = [
        (TypeError, dict(best=best.float())), (ValueError, dict(best=best[:64])), (ValueError, dict(cls_a=ca)),
        (ValueError, dict(cls_b=cb)), (TypeError, dict(cls_a=ca.long(), cls_b=cb)),
        (ValueError, dict(cls_a=ca, cls_b=cb[:199])), (ValueError, dict(splits=33)), (TypeError, dict(best=None)),
    ]
    for exc, change in bad_counts:
        kw = dict(a=a, b=b, key_a=ka, key_b=kb, best=best)
        kw.update(change)
        with pytest.raises(exc):
            ops.retrieval_counts(**kw)


def test_the_c_abi_refuses_with_every_output_untouched():
    """null pointers, D 0 / 63 / 65, misaligned rows, ld < D, splits -1 / 33, a workspace too small, eps 0, the class
    arguments in part: SBA_E_ARG, and not one element of best, the counts or the workspace is written"""
    from sbagan import _lib
    lib = _lib.lib
    na, nb, D = 65, 200, 64
    A, B, ka, kb, ca, cb, best, _, _ = int_case(D, na, nb)
    a, b, ka, kb, ca, cb = dev(A), dev(B), keys(ka), keys(kb), keys(ca), keys(cb)
    wide = torch.zeros(na * D + 4, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    out_d = torch.full((na + 2 * GUARD,), -7.5, dtype=torch.float64, device=DEV)
    out_i = torch.full((2, na + 2 * GUARD), -77, dtype=torch.int32, device=DEV)
    thr = dev(best)
    need = lib.sba_retrieval_workspace_bytes(na, nb, 3)
    assert need == 3 * na * 8
    ws = torch.full((need // 8 + 2 * GUARD,), -7.5, dtype=torch.float64, device=DEV)
    pa, pb, pka, pkb, pca, pcb = (t.data_ptr() for t in (a, b, ka, kb, ca, cb))
    po, pw = out_d[GUARD:].data_ptr(), ws[GUARD:].data_ptr()
    p0, p1, pt = out_i[0, GUARD:].data_ptr(), out_i[1, GUARD:].data_ptr(), thr.data_ptr()
    ok = dict(a=pa, na=na, lda=D, b=pb, nb=nb, ldb=D, D=D, key_a=pka, key_b=pkb, eps=1e-8, splits=3, best=po, ws=pw,
              ws_bytes=need)
    changes = [dict(a=None), dict(b=None), dict(key_a=None), dict(key_b=None), dict(best=None), dict(ws=None),
               dict(D=0), dict(D=63), dict(D=65), dict(a=wide.data_ptr() + 4), dict(b=pb + 8), dict(lda=60), dict(ldb=63),
               dict(lda=66), dict(splits=-1), dict(splits=33), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(eps=0.0),
               dict(eps=-1.0), dict(na=0), dict(nb=0), dict(best=po + 4), dict(ws=pw + 4), dict(key_a=pka + 2)]
    for ch in changes:
        kw = dict(ok)
        kw.update(ch)
        rc = lib.sba_retrieval_own_best(kw['a'], kw['na'], kw['lda'], kw['b'], kw['nb'], kw['ldb'], kw['D'], kw['key_a'],
                                        kw['key_b'], kw['eps'], kw['splits'], kw['best'], kw['ws'], kw['ws_bytes'], st)
        assert rc == -1, ch
    okc = dict(ok, cls_a=pca, cls_b=pcb, best=pt, above=p0, above_masked=p1)
    changes_c = [c for c in changes if 'best' not in c] + [
        dict(best=None), dict(best=pt + 4), dict(above=None), dict(above=p0 + 2), dict(cls_a=None), dict(cls_b=None),
        dict(above_masked=None), dict(cls_a=None, cls_b=None), dict(cls_a=None, above_masked=None),
        dict(cls_a=pca + 2), dict(above_masked=p1 + 1)]
    for ch in changes_c:
        kw = dict(okc)
        kw.update(ch)
        rc = lib.sba_retrieval_counts(kw['a'], kw['na'], kw['lda'], kw['b'], kw['nb'], kw['ldb'], kw['D'], kw['key_a'],
                                      kw['key_b'], kw['cls_a'], kw['cls_b'], kw['best'], kw['eps'], kw['splits'],
                                      kw['above'], kw['above_masked'], kw['ws'], kw['ws_bytes'], st)
        assert rc == -1, ch
    torch.cuda.synchronize()
    assert bool((out_d == -7.5).all()) and bool((out_i == -77).all()) and bool((ws == -7.5).all())
    # and the accepted call writes exactly its outputs: na elements each, the guards stay
    assert lib.sba_retrieval_own_best(pa, na, D, pb, nb, D, D, pka, pkb, 1e-8, 3, po, pw, need, st) == 0
    assert lib.sba_retrieval_counts(pa, na, D, pb, nb, D, D, pka, pkb, pca, pcb, po, 1e-8, 3, p0, p1, pw, need, st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(out_d[GUARD:GUARD + na].cpu().numpy()), bits(best))
    for t, fill in ((out_d, -7.5), (out_i[0], -77), (out_i[1], -77), (ws, -7.5)):
        assert bool((t[:GUARD] == fill).all()) and bool((t[-GUARD:] == fill).all())
    assert bool((out_i[:, GUARD:GUARD + na] >= 0).all())


# ------------------------------------------------------------------ the Retrieval class with stub codes
def test_retrieval_class_against_the_reference():
    from sbagan import retrieval
    X, Y, owner, cls, r = real_case(*REAL[0])
    ev = retrieval.Retrieval(dev(X), dev(Y), owner, cls)
    ranks = ev.ranks()
    assert sorted(ranks) == sorted(retrieval.RANKS)
    for name in retrieval.RANKS:
        assert ranks[name].dtype == np.int32 and np.array_equal(ranks[name], r[name]), name
    res = ev.result()
    for name in retrieval.RANKS:
        assert res[name] == ref.figures(r[name]), name
        assert sorted(res[name]) == sorted(retrieval.FIGURES)
    assert res['n_images'] == 70 and res['n_captions'] == 210 and res['captions_per_image'] == 3.0
    assert res['eps'] == 1e-8 and res['dtype'] in ('float32', 'bfloat16')
    assert res['i2t_class_masked']['r_at_1'] >= res['i2t_instance']['r_at_1']
    json.dumps(res)
    # an uneven number of captions per image, in any order
    perm = np.random.RandomState(2).permutation(210)[:150]
    keep = np.concatenate([perm, np.setdiff1d(np.arange(0, 210, 3), perm)])     # every image keeps its first caption
    ev = retrieval.Retrieval(dev(X), dev(Y[keep]), owner[keep], cls)
    r2 = ref.all_ranks(X, Y[keep], owner[keep], cls, exact=True)
    assert min_gap(r2, owner[keep]) > 2 * ref.score_bound(64)
    for name in retrieval.RANKS:
        assert np.array_equal(ev.ranks()[name], r2[name]), name


# ------------------------------------------------------------------ the entry points on a toy directory
CROP, BATCH, WORDS_NUM = 128, 4, 8


def _yml(path, root, net_e='', epochs=1):
    import yaml
    with open(path, 'w') as f:
        f.write(yaml.safe_dump({
            'CONFIG_NAME': 'DAMSM', 'DATASET_NAME': 'toy', 'DATA_DIR': root, 'GPU_ID': 0, 'WORKERS': 0,
            'TREE': {'BRANCH_NUM': 1, 'BASE_SIZE': CROP},
            'TRAIN': {'FLAG': True, 'NET_E': net_e, 'BATCH_SIZE': BATCH, 'MAX_EPOCH': epochs, 'SNAPSHOT_INTERVAL': 1,
                      'ENCODER_LR': 0.002, 'RNN_GRAD_CLIP': 0.25,
                      'SMOOTH': {'GAMMA1': 4.0, 'GAMMA2': 5.0, 'GAMMA3': 10.0}},
            'TEXT': {'EMBEDDING_DIM': 256, 'CAPTIONS_PER_IMAGE': 2, 'WORDS_NUM': WORDS_NUM}}))
    return path


def _toy_cfg():
    from miscc.config import cfg, reset_cfg
    reset_cfg()
    cfg.TREE.BRANCH_NUM, cfg.TREE.BASE_SIZE = 1, CROP
    cfg.TEXT.CAPTIONS_PER_IMAGE, cfg.TEXT.WORDS_NUM, cfg.TEXT.EMBEDDING_DIM = 2, WORDS_NUM, 256
    cfg.TRAIN.BATCH_SIZE = BATCH
    return cfg


def _stdout(text):
    """what a run printed, without the timing of the interval lines"""
    return [re.sub(r'ms/batch\s*[0-9.]+', 'ms/batch', l) for l in text.splitlines()]


def run_main(toy, capsys, monkeypatch, flags, key=None, net_e='', make_step=None, max_steps=None, epochs=2):
    """one pretrain_DAMSM.main run in the deterministic f32 mode from one seed (cached by `key`): two epochs of one
    batch, so the second evaluation meets weights and running statistics that an update has moved since the first"""
    key = key or ' '.join(flags)
    if key in toy['runs']:
        return toy['runs'][key]
    import pretrain_DAMSM
    from miscc.config import reset_cfg
    from sbagan import ops
    reset_cfg()
    ops.set_compute_dtype(torch.float32)
    ops.set_deterministic(True)
    try:
        work = toy['tmp'].mktemp('run')
        (work / 'cwd').mkdir()
        monkeypatch.chdir(work / 'cwd')             # the entry point writes to ../output/<name>
        yml = _yml(str(work / 'toy.yml'), toy['root'], net_e, epochs)
        capsys.readouterr()
        out = pretrain_DAMSM.main(['--cfg', yml, '--gpu', '0', '--manualSeed', '7'] + list(flags), max_steps=max_steps,
                                  make_step=make_step)
        torch.cuda.synchronize()
        out = os.path.abspath(out)                  # (it is relative to this run's directory)
        text = capsys.readouterr().out
        rng = (np.random.get_state(), torch.random.get_rng_state(), torch.cuda.get_rng_state(0), random.getstate())
    finally:
        ops.set_deterministic(False)
        reset_cfg()
    top = out if os.path.basename(out) != 'Model' else os.path.dirname(out)
    res = {'dir': top, 'text': text, 'lines': _stdout(text),
           'files': {os.path.relpath(p, top): torch.load(p, map_location='cpu')
                     for p in sorted(glob.glob(os.path.join(top, '**', '*.pth'), recursive=True))},
           'jsonl': None, 'json': None,
           'rng_after': rng}
    path = os.path.join(top, 'Model', 'retrieval.jsonl')
    if os.path.isfile(path):
        with open(path) as f:
            res['jsonl'] = [json.loads(l) for l in f.read().splitlines()]
    path = os.path.join(top, 'retrieval.json')
    if os.path.isfile(path):
        with open(path) as f:
            res['json'] = json.load(f)
    toy['runs'][key] = res
    return res


@pytest.fixture(scope='module')
def toy(tmp_path_factory):
    import datasets
    root = str(tmp_path_factory.mktemp('retrieval') / 'toy')
    _make_dataset(root, n_train=4, n_test=4, per_image=2)
    _toy_cfg()
    datasets.TextDataset(root, 'train', base_size=CROP)         # writes captions.pickle, so every run prints alike
    from miscc.config import reset_cfg
    reset_cfg()
    return {'root': root, 'tmp': tmp_path_factory, 'runs': {}}


def _figures(record):
    from sbagan.retrieval import RANKS
    return {k: record[k] for k in RANKS + ('n_images', 'n_captions', 'captions_per_image', 'eps', 'dtype')}


@pytest.fixture()
def det_f32():
    """_load_pair switches to the mode the cached runs were made in; this puts the default back"""
    from miscc.config import reset_cfg
    from sbagan import ops
    yield
    ops.set_deterministic(False)
    reset_cfg()


def _load_pair(toy, model_dir_top, epoch=0):
    """the saved pair of an epoch in eval mode, and the validation split"""
    import datasets
    import pretrain_DAMSM
    from sbagan import ops
    ops.set_compute_dtype(torch.float32)
    ops.set_deterministic(True)
    cfg = _toy_cfg()
    cfg.DATA_DIR = toy['root']
    cfg.TRAIN.NET_E = os.path.join(model_dir_top, 'Model', 'text_encoder%d.pth' % epoch)
    ds = datasets.TextDataset(toy['root'], 'test', base_size=CROP)
    text_encoder, image_encoder, _, start = pretrain_DAMSM.build_models(ds.n_words, BATCH)
    assert start == epoch + 1
    return ds, text_encoder.eval(), image_encoder.eval()


def _own_codes(ds, text_encoder, image_encoder):
    """the codes of the validation split computed by the test: centre crops by PIL through a HIP trunk of the test's own,
    all captions in one length-sorted batch through the loaded module (the word subset of an over-long caption drawn as
    the evaluation seeds it)"""
    import datasets
    from sbagan.inception_hip import InceptionHIP
    imgs = []
    for i in range(len(ds)):
        img = datasets.load_image(ds.image_path(i), ds.image_box(i), int(CROP * 76 / 64))
        W, H = img.size
        x1, y1 = (W - CROP) // 2, (H - CROP) // 2
        imgs.append(ds.norm(img.crop((x1, y1, x1 + CROP, y1 + CROP))))
    state = np.random.get_state()
    np.random.seed(0)
    caps, lens = zip(*(ds.get_caption(t) for t in range(len(ds) * ds.embeddings_num)))
    np.random.set_state(state)
    caps, lens = np.stack(caps).reshape(len(lens), -1), np.asarray(lens, dtype=np.int64)
    order = np.argsort(-lens, kind='stable')
    with torch.no_grad():
        _, x = InceptionHIP(image_encoder)(torch.stack(imgs).to(DEV))
        c, n = torch.from_numpy(caps[order]).to(DEV), torch.from_numpy(lens[order]).to(DEV)
        _, y = text_encoder(c, n, text_encoder.init_hidden(len(lens)))
    y = y.float()[torch.from_numpy(np.argsort(order)).to(DEV)]
    return x.float().cpu().numpy(), y.cpu().numpy()


def test_pretraining_with_retrieval_writes_the_ranks_of_the_saved_pair(toy, capsys, monkeypatch, det_f32):
    from sbagan.retrieval import RANKS
    a = run_main(toy, capsys, monkeypatch, ['--retrieval', '1'])
    assert sorted(a['files']) == ['Model/image_encoder0.pth', 'Model/image_encoder1.pth', 'Model/text_encoder0.pth',
                                  'Model/text_encoder1.pth']
    assert [r['epoch'] for r in a['jsonl']] == [0, 1] and [r['lr'] for r in a['jsonl']] == [0.002, 0.002 * 0.98]
    lines = [l for l in a['lines'] if '| retrieval ' in l]
    assert len(lines) == 2 and lines[0].startswith('| end epoch   0 | retrieval i2t ') and 'class-masked' in lines[0]
    assert lines[1].startswith('| end epoch   1 | retrieval i2t ')
    valid = [i for i, l in enumerate(a['lines']) if 'valid loss' in l]
    assert [a['lines'].index(l) for l in lines] == [i + 1 for i in valid]
    for epoch, rec in enumerate(a['jsonl']):
        assert rec['n_images'] == 4 and rec['n_captions'] == 8 and rec['captions_per_image'] == 2.0
        assert rec['dtype'] == 'float32' and rec['eps'] == 1e-8
        ds, text_encoder, image_encoder = _load_pair(toy, a['dir'], epoch)
        x, y = _own_codes(ds, text_encoder, image_encoder)
        owner, cls = np.arange(8) // 2, np.asarray(ds.class_id)[:4]
        r = ref.all_ranks(x, y, owner, cls, exact=True)
        print('toy split, epoch %d: smallest gap to a threshold %.3e, bound %.3e'
              % (epoch, min_gap(r, owner), ref.score_bound(256)))
        assert min_gap(r, owner) > 2 * ref.score_bound(256)
        for name in RANKS:
            assert rec[name] == ref.figures(r[name]), (epoch, name)


def test_the_flag_leaves_the_training_as_it_is(toy, capsys, monkeypatch):
    """the deterministic f32 run with and without --retrieval: equal checkpoints, equal stdout but for the one line, and
    the global generators of numpy and torch left where the run without the flag leaves them"""
    a = run_main(toy, capsys, monkeypatch, ['--retrieval', '1'])
    b = run_main(toy, capsys, monkeypatch, [])
    assert b['jsonl'] is None and not os.path.exists(os.path.join(b['dir'], 'Model', 'retrieval.jsonl'))
    assert sorted(a['files']) == sorted(b['files'])
    for name in a['files']:
        bad = [k for k in a['files'][name] if not torch.equal(a['files'][name][k], b['files'][name][k])]
        assert not bad, (name, bad[:5])
    assert [l for l in a['lines'] if '| retrieval ' not in l] == b['lines']
    assert len(a['lines']) == len(b['lines']) + 2
    (na, ta, ca, pa), (nb, tb, cb, pb) = a['rng_after'], b['rng_after']
    assert torch.equal(ta, tb) and torch.equal(ca, cb) and pa == pb
    assert na[0] == nb[0] and np.array_equal(na[1], nb[1]) and na[2:] == nb[2:]


def test_device_data_gives_the_host_path_codes_bit_for_bit(toy, capsys, monkeypatch, det_f32):
    from sbagan import device_data, retrieval
    a = run_main(toy, capsys, monkeypatch, ['--retrieval', '1'])
    ds, text_encoder, image_encoder = _load_pair(toy, a['dir'])
    resize = int(CROP * 76 / 64)
    cache = device_data.DeviceImageCache(ds, resize, torch.device(DEV), max_bytes=1 << 30)
    image_encoder.train()                       # the mode is put back, and the running statistics stay
    before = {k: v.clone() for k, v in image_encoder.state_dict().items()}
    state = torch.random.get_rng_state()
    for batch in (4, 3):                        # 3: a short last batch
        host = retrieval.encode_images(ds, image_encoder, batch, CROP, resize)
        devc = retrieval.encode_images(ds, image_encoder, batch, CROP, resize, cache=cache)
        assert tuple(host.shape) == (4, 256) and host.dtype == torch.float32
        assert torch.equal(host, devc)
    assert image_encoder.training and torch.equal(torch.random.get_rng_state(), state)
    after = image_encoder.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    image_encoder.eval()
    # the loader's new method against the PIL crop itself
    loader = device_data.DeviceBatchLoader(ds, cache, BATCH, CROP, 1, 0)
    got = loader.center_batch([2, 0])
    want = torch.stack([retrieval._CenterCrops(ds, CROP, resize)[i] for i in (2, 0)])
    assert torch.equal(got.cpu(), want) and loader.last_draws is None
    res = retrieval.evaluate_split(ds, image_encoder, text_encoder, BATCH, CROP, resize, cache=cache).result()
    assert _figures(res) == _figures(a['jsonl'][0])
    assert not text_encoder.training and not image_encoder.training
    # and through the entry point: the flag combination runs and writes its line
    d = run_main(toy, capsys, monkeypatch, ['--retrieval', '1', '--device_data', '--device_data_gb', '1'])
    assert len(d['jsonl']) == 2 and d['jsonl'][0]['n_captions'] == 8


def test_retrieval_only(toy, capsys, monkeypatch):
    a = run_main(toy, capsys, monkeypatch, ['--retrieval', '1'])
    net_e = os.path.join(a['dir'], 'Model', 'text_encoder1.pth')
    o = run_main(toy, capsys, monkeypatch, ['--retrieval_only'], net_e=net_e)
    assert o['files'] == {} and o['jsonl'] is None
    assert _figures(o['json']) == _figures(a['jsonl'][1]) and o['json']['net_e'] == net_e
    lines = [l for l in o['lines'] if '| retrieval ' in l]
    assert len(lines) == 1 and lines[0].startswith('| end epoch   1 |') and lines[0] == \
        [l for l in a['lines'] if '| retrieval ' in l][1]
    assert not any(l.startswith('| epoch') or 'valid loss' in l for l in o['lines'])
    with pytest.raises(RuntimeError, match='--retrieval_only'):
        run_main(toy, capsys, monkeypatch, ['--retrieval_only'], key='refused')


def test_bert_entry_point_with_retrieval(toy, tmp_path, capsys, monkeypatch):
    import pretrain_DAMSM_bert
    from miscc.config import reset_cfg
    from sbagan import ops
    from test_bert_entry_gpu import _bert_dir
    bert_dir = _bert_dir(tmp_path)
    reset_cfg()
    ops.set_compute_dtype(torch.bfloat16)
    try:
        (tmp_path / 'w' / 'cwd').mkdir(parents=True)
        monkeypatch.chdir(tmp_path / 'w' / 'cwd')
        yml = _yml(str(tmp_path / 'toy.yml'), toy['root'])
        model_dir = pretrain_DAMSM_bert.main(['--cfg', yml, '--gpu', '0', '--manualSeed', '7', '--bert_dir', bert_dir,
                                              '--retrieval', '1'], max_steps=1)
        text = capsys.readouterr().out
    finally:
        reset_cfg()
    with open(os.path.join(model_dir, 'retrieval.jsonl')) as f:
        recs = [json.loads(l) for l in f.read().splitlines()]
    assert len(recs) == 1 and recs[0]['n_images'] == 4 and recs[0]['n_captions'] == 8 and recs[0]['dtype'] == 'bfloat16'
    assert 0.0 <= recs[0]['t2i_instance']['r_at_1'] <= recs[0]['t2i_instance']['r_at_5'] <= 1.0
    assert 1.0 <= recs[0]['i2t_instance']['median_rank'] <= 7.0
    assert text.count('| retrieval ') == 1


def test_replayed_pretraining_with_retrieval_is_its_eager_twin(toy, capsys, monkeypatch):
    from sbagan.damsm import DAMSMSlotStep
    flags = ['--retrieval', '1', '--replay', '--device_data', '--device_data_gb', '1']
    runs = []
    for eager in (False, True):
        steps = []

        def make(*a, **kw):
            steps.append(DAMSMSlotStep(*a, eager=eager, **kw))
            return steps[-1]
        r = run_main(toy, capsys, monkeypatch, flags, key='replay eager=%s' % eager, make_step=make)
        r.setdefault('recorded', steps[0].recording is not None)
        runs.append(r)
    a, b = runs
    assert a['recorded'] and not b['recorded'] and 'could not be recorded' not in a['text']
    assert len(a['files']) == 4 and sorted(a['files']) == sorted(b['files'])
    for name in a['files']:
        bad = [k for k in a['files'][name] if not torch.equal(a['files'][name][k], b['files'][name][k])]
        assert not bad, (name, bad[:5])
    assert [r['epoch'] for r in a['jsonl']] == [0, 1] and a['jsonl'] == b['jsonl']
    # (the validation line is left out: the step's own trunk folds its BatchNorm statistics when a python-side training
    # forward has marked them moved, which the replayed launches do not -- as without --retrieval)
    def kept(r):
        return [l for l in r['lines'] if 'valid loss' not in l]
    assert kept(a) == kept(b) and sum('| retrieval ' in l for l in kept(a)) == 2
