"""A numpy float64 reference of the retrieval definitions (sbagan/retrieval.py): the cosine scores, the own
best, the four rank vectors and the figures.  Everything is a full matrix here; nothing is shared with the code under
test."""
import math

import numpy as np

EPS = 1e-8
U = 2.0 ** -53                  # unit roundoff of float64


def score_bound(D):
    """|s_kernel - s_reference(exact=True)| <= (D + D / 8 + 12) U for rows whose norm product is above eps^2; derived in
    tests/test_retrieval_cpu.py and DESIGN.md 7l"""
    return (D + D / 8.0 + 12.0) * U


def scores(X, Y, eps=EPS, exact=False):
    """s [n][m] f64 = x_i . y_j / max(sqrt(|x_i|^2 |y_j|^2), eps) of f32 rows.  exact: dot products and squared norms
    by math.fsum (the products of widened f32 values are exact in f64, so each is the correctly rounded sum); otherwise
    numpy's own summation order, which is exact too wherever every partial sum is an integer below 2^53."""
    X, Y = np.asarray(X, dtype=np.float32).astype(np.float64), np.asarray(Y, dtype=np.float32).astype(np.float64)
    with np.errstate(all='ignore'):
        if exact:
            g = np.array([[math.fsum(x * y) for y in Y] for x in X], dtype=np.float64).reshape(len(X), len(Y))
            nx, ny = (np.array([math.fsum(v * v) for v in M], dtype=np.float64) for M in (X, Y))
        else:
            g = np.array([[np.sum(x * y) for y in Y] for x in X], dtype=np.float64).reshape(len(X), len(Y))
            nx, ny = (X * X).sum(1), (Y * Y).sum(1)
        # fmax, as the kernel's: a NaN norm product gives way to eps (the score is NaN then anyway: g is)
        return g / np.fmax(np.sqrt(nx[:, None] * ny[None, :]), eps)


def own_best(S, key_a, key_b):
    """best [n]: the largest score of a row over the columns of its own key; -inf without one, NaN with a NaN among them"""
    key_a, key_b = np.asarray(key_a), np.asarray(key_b)
    out = np.full(S.shape[0], -np.inf)
    for i in range(S.shape[0]):
        own = S[i, key_b == key_a[i]]
        if own.size:
            out[i] = np.nan if np.isnan(own).any() else own.max()
    return out


def counts(S, key_a, key_b, thr, cls_a=None, cls_b=None):
    """(above, above_masked) int32 [n]: the columns of another key that are NOT below the row's threshold -- a tie and a
    NaN on either side count -- and those of them of another class too (None without the classes)"""
    key_a, key_b = np.asarray(key_a), np.asarray(key_b)
    with np.errstate(invalid='ignore'):
        hit = ~(S < np.asarray(thr)[:, None]) & (key_b[None, :] != key_a[:, None])
    above = hit.sum(1).astype(np.int32)
    if cls_a is None:
        return above, None
    other = np.asarray(cls_b)[None, :] != np.asarray(cls_a)[:, None]
    return above, (hit & other).sum(1).astype(np.int32)


def all_ranks(X, Y, owner, image_class, eps=EPS, exact=False):
    """the four rank vectors of images X [ni] and captions Y [nt], plus 'best' [ni] and 'thr' [nt]"""
    owner, image_class = np.asarray(owner), np.asarray(image_class)
    S = scores(X, Y, eps, exact)
    key_i = np.arange(S.shape[0])
    best = own_best(S, key_i, owner)
    thr = S[owner, np.arange(S.shape[1])]
    i_all, i_mask = counts(S, key_i, owner, best, image_class, image_class[owner])
    t_all, t_mask = counts(S.T, owner, key_i, thr, image_class[owner], image_class)
    return {'i2t_instance': i_all, 'i2t_class_masked': i_mask, 't2i_instance': t_all, 't2i_class_masked': t_mask,
            'best': best, 'thr': thr, 'scores': S}


def figures(ranks):
    """R@1 / R@5 / R@10 (rank < k) and the median and mean of rank + 1, in plain python"""
    r = sorted(int(v) for v in np.asarray(ranks).reshape(-1))
    n = len(r)
    out = {'r_at_%d' % k: sum(1 for v in r if v < k) / float(n) for k in (1, 5, 10)}
    out['median_rank'] = float(r[n // 2] + 1) if n % 2 else (r[n // 2 - 1] + r[n // 2]) / 2.0 + 1.0
    out['mean_rank'] = sum(r) / float(n) + 1.0
    return out
