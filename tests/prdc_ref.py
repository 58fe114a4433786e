"""Float64 numpy reference of the k-nearest-neighbour manifold metrics (sbagan/prdc.py), written from the definitions:
squared distances as direct differences ((a - b) ** 2).sum(), never the Gram form; self excluded by INDEX in the k-NN
radius (a duplicate row counts, at distance 0); every ball test is d2 <= radius2."""
import numpy as np


def dist2(a, b):
    """[na][nb] float64: the squared distances between the rows of a and the rows of b, row by row"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.empty((a.shape[0], b.shape[0]))
    for i in range(a.shape[0]):
        d = b - a[i]
        out[i] = (d * d).sum(1)
    return out


def knn_radius(x, k):
    """[n] float64: the k-th smallest squared distance from each row to the OTHER rows"""
    d2 = dist2(x, x)
    n = d2.shape[0]
    assert 1 <= k <= n - 1
    out = np.empty(n)
    for i in range(n):
        out[i] = np.sort(np.delete(d2[i], i))[k - 1]
    return out


def ball_counts(a, b, radius_a=None, radius_b=None):
    """(in_b, in_own), int64 [na] or None: in_b[i] = #{j : d2(i, j) <= radius_b[j]}, in_own[i] = #{j : d2(i, j) <=
    radius_a[i]} over the rows j of b"""
    d2 = dist2(a, b)
    in_b = (d2 <= np.asarray(radius_b)[None, :]).sum(1) if radius_b is not None else None
    in_own = (d2 <= np.asarray(radius_a)[:, None]).sum(1) if radius_a is not None else None
    return in_b, in_own


def counts(real, fake, k):
    """(fake_in_real [n_fake], real_in_fake [n_real], real_own [n_real]): the three count vectors of the metrics"""
    r_real, r_fake = knn_radius(real, k), knn_radius(fake, k)
    fake_in_real, _ = ball_counts(fake, real, radius_b=r_real)
    real_in_fake, real_own = ball_counts(real, fake, radius_a=r_real, radius_b=r_fake)
    return fake_in_real, real_in_fake, real_own


def prdc(real, fake, k):
    """{'precision', 'recall', 'density', 'coverage'} from the definitions"""
    fake_in_real, real_in_fake, real_own = counts(real, fake, k)
    return {'precision': float((fake_in_real > 0).mean()), 'recall': float((real_in_fake > 0).mean()),
            'density': float(fake_in_real.sum()) / (k * len(fake)), 'coverage': float((real_own > 0).mean())}
