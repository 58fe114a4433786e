"""Float64 numpy reference of the nearest-training-image evaluation (sbagan/nearest.py, csrc/knn.hip), written from the
definitions: squared distances as direct differences ((a - b) ** 2).sum(), never the Gram form; the neighbours of a row
in ascending order of the key (d2, j), a NaN or infinite d2 never listed, the tail padded with +inf / -1; the statistics
from their definitions, row by row."""
import math

import numpy as np

from prdc_ref import dist2, knn_radius  # noqa: F401  (the distance and the self-excluding radius are PRDC's)


def topk_of(d2, k):
    """(d2 [na][k] float64, idx [na][k] int64) from a distance matrix [na][nb]"""
    d2 = np.asarray(d2, dtype=np.float64)
    na, nb = d2.shape
    out_d, out_j = np.full((na, k), np.inf), np.full((na, k), -1, dtype=np.int64)
    for i in range(na):
        listable = [(d2[i, j], j) for j in range(nb) if d2[i, j] < np.inf]      # (a NaN compares false)
        for m, (d, j) in enumerate(sorted(listable)[:k]):
            out_d[i, m], out_j[i, m] = d, j
    return out_d, out_j


def topk(a, b, k):
    """the k rows of b nearest to each row of a, ties to the smaller row number"""
    with np.errstate(invalid='ignore'):
        return topk_of(dist2(a, b), k)


def statistics(fake_d2, fake_idx, real_d2, real_idx, train_r2):
    """the scalar figures of sbagan.nearest.nearest_from_lists, one row at a time"""
    fd, fi = np.asarray(fake_d2, dtype=np.float64), np.asarray(fake_idx)
    rd, ri = np.asarray(real_d2, dtype=np.float64).reshape(-1), np.asarray(real_idx).reshape(-1)
    nf, nr, nt = fd.shape[0], rd.shape[0], len(train_r2)

    def side(d, t):
        authentic, dist = 0, []
        for x in range(len(d)):
            if t[x] < 0:
                continue
            dist.append(math.sqrt(d[x]))
            if d[x] > train_r2[t[x]]:
                authentic += 1
        return authentic / float(len(d)), dist

    auth_f, dist_f = side(fd[:, 0], fi[:, 0])
    auth_r, dist_r = side(rd, ri)
    finite_r = sorted(rd[x] if ri[x] >= 0 else np.inf for x in range(nr))
    threshold = finite_r[-(-nr // 100) - 1]
    copies = sum(1 for g in range(nf) if fi[g, 0] >= 0 and fd[g, 0] <= threshold)
    hits = {}
    for g in range(nf):
        if fi[g, 0] >= 0:
            hits[int(fi[g, 0])] = hits.get(int(fi[g, 0]), 0) + 1
    out = {'authenticity': auth_f, 'authenticity_real': auth_r, 'copy_fraction': copies / float(nf),
           'copy_threshold': float(threshold) if threshold < np.inf else None,
           'train_hit_distinct': len(hits) / float(min(nf, nt)), 'train_hit_max': max(hits.values()) if hits else 0,
           'n_nan': sum(1 for g in range(nf) if fi[g, 0] < 0) + sum(1 for x in range(nr) if ri[x] < 0)}
    for name, dist in (('nn_dist_fake', dist_f), ('nn_dist_real', dist_r)):
        out[name] = {'median': float(np.median(dist)), 'mean': float(np.mean(dist))} if dist else \
            {'median': None, 'mean': None}
    mf, mr = out['nn_dist_fake']['median'], out['nn_dist_real']['median']
    out['nn_ratio'] = mf / mr if (mf is not None and mr) else None
    return out


def suspect_rows(fake_d2, fake_idx, show):
    """the generated rows with the smallest d2 to their nearest training row, ties to the smaller row number"""
    fd, fi = np.asarray(fake_d2, dtype=np.float64), np.asarray(fake_idx)
    ranked = sorted((fd[g, 0], g) for g in range(fd.shape[0]) if fi[g, 0] >= 0)
    return [g for _, g in ranked[:show]]


# ------------------------------------------------------------------ fixtures the CPU and the GPU tests share
U = 2.0 ** -53                  # unit roundoff of float64
# (na, nb, D, k, shift, seed), built as test_prdc_gpu.real_case builds its sets: B is randn, A is 0.9 randn + shift
REAL = [(70, 150, 64, 8, 0.15, 0), (130, 97, 192, 5, 0.08, 7), (65, 200, 128, 3, 0.2, 3)]
_CASES = {}


def d2_bound_rel(D):
    """the bound tests/test_prdc_gpu.py derives on |d2_kernel - d2_reference| for this formula and these summation
    orders, relative to |a|^2 + |b|^2"""
    return (4 * D + 9) * U


def real_case(na, nb, D, k, shift, seed):
    """(A, B, reference): the fixtures and what numpy knows about them, computed once per case and read-only"""
    case = (na, nb, D, k, shift, seed)
    if case not in _CASES:
        rng = np.random.RandomState(seed)
        B = rng.randn(nb, D)
        A = 0.9 * rng.randn(na, D) + shift
        A, B = A.astype(np.float32), B.astype(np.float32)
        d2 = dist2(A, B)
        ref = {'d2': d2, 'n_a': (A.astype(np.float64) ** 2).sum(1), 'n_b': (B.astype(np.float64) ** 2).sum(1)}
        ref['top_d2'], ref['top_idx'] = topk_of(d2, k)
        for v in (A, B) + tuple(ref.values()):
            v.setflags(write=False)
        _CASES[case] = (A, B, ref)
    return _CASES[case]


def smallest_gap(ref, k):
    """the smallest difference between consecutive neighbours among the first k + 1 of any row, relative to
    |a|^2 + max |b|^2: both values of a pair move by at most the bound at their own norms, so the order of the first k
    stands when this exceeds two bounds"""
    first = np.sort(ref['d2'], axis=1)[:, :k + 1]
    return float(((first[:, 1:] - first[:, :-1]) / (ref['n_a'][:, None] + ref['n_b'].max())).min())


def int_features(n, D, seed):
    """integer values in [-8, 8] (as test_prdc_gpu.int_features): every squared distance is an exact integer"""
    return np.random.RandomState(seed).randint(-8, 9, size=(n, D)).astype(np.float32)
