"""Precision, recall, density and coverage of generated images: the k-nearest-neighbour manifold metrics (improved
precision and recall, Kynkaanniemi et al. 2019; density and coverage, Naeem et al. 2020) on the project's own Inception-v3
trunk -- the same f32 2048-d pooled Mixed_7c rows FID uses (`InceptionHIP.last_pooled` / `pooled_features`).

Per side ('real', 'fake') the rows are appended to a device buffer that grows by doubling, without a host-device sync per
batch (sbagan/feature_rows.py).  result() runs four launches of the f64 matrix-core distance kernel of csrc/prdc.hip and
reads back once:

    r_real = ops.prdc_knn_radius(real, k)     r_fake = ops.prdc_knn_radius(fake, k)
        the squared distance from a row to its k-th nearest OTHER row of its own side (self excluded by index, so a
        duplicate row counts, at distance 0)
    in_b, _      = ops.prdc_ball_counts(fake, real, radius_b=r_real)
        precision = mean(in_b > 0)            a fake lies in the ball of some real
        density   = sum(in_b) / (k n_fake)    in how many, over k
    in_b, in_own = ops.prdc_ball_counts(real, fake, radius_a=r_real, radius_b=r_fake)
        recall    = mean(in_b > 0)            a real lies in the ball of some fake
        coverage  = mean(in_own > 0)          a real has a fake inside its own ball

Every comparison is d2 <= radius2 on float64 squared distances.  The trunk is the torchvision-lineage Inception-v3 of
image_encoder*.pth run in the compute dtype, NOT the network of the published implementations: the figures are comparable
between runs of this project only.

The evaluator draws no random numbers.
"""
import numpy as np
import torch

from . import ops
from .feature_rows import SIDES, Evaluator, FeatureRows, dtype_name

FIELDS = ('precision', 'recall', 'density', 'coverage', 'k', 'n_real', 'n_fake', 'dtype')


def prdc_from_counts(fake_in_real, real_in_fake, real_own, k, dtype=''):
    """The result dict from the three count vectors (host arithmetic only):
    fake_in_real [n_fake]: per generated row, the real balls it lies in; real_in_fake [n_real]: per real row, the fake
    balls it lies in; real_own [n_real]: per real row, the generated rows inside its own ball."""
    fr, rf, ro = (np.asarray(v) for v in (fake_in_real, real_in_fake, real_own))
    k = int(k)
    if fr.ndim != 1 or rf.ndim != 1 or ro.shape != rf.shape or fr.size < 1 or rf.size < 1:
        raise ValueError('prdc_from_counts: counts must be [n_fake], [n_real], [n_real] (got %s, %s, %s)'
                         % (fr.shape, rf.shape, ro.shape))
    if k < 1:
        raise ValueError('prdc_from_counts: k must be >= 1 (got %d)' % k)
    n_fake, n_real = int(fr.size), int(rf.size)
    return {'precision': float(np.count_nonzero(fr > 0)) / n_fake,
            'recall': float(np.count_nonzero(rf > 0)) / n_real,
            'density': float(fr.astype(np.int64).sum()) / (k * n_fake),
            'coverage': float(np.count_nonzero(ro > 0)) / n_real,
            'k': k, 'n_real': n_real, 'n_fake': n_fake, 'dtype': str(dtype)}


class PRDC(Evaluator):
    """Collects the feature rows of real and generated images.  features(images) -> f32 [B][D] on the device (an
    InceptionHIP's pooled_features, or any callable of that shape); k: the neighbour that sets a ball's radius (1 .. 8);
    key: a description of the run, kept for the caller; dtype: the compute-dtype name reported in the result."""

    def __init__(self, features, D=2048, k=5, key='', dtype=None, capacity=256):
        self.store = FeatureRows('PRDC', D, capacity)       # (sbagan.kid.KID(rows=<this>) reads it too)
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= ops.PRDC_MAX_K:
            raise ValueError('PRDC: k must be an integer in [1, %d] (got %r)' % (ops.PRDC_MAX_K, k))
        self.features, self.D, self.k, self.key, self.capacity = features, int(D), k, str(key), int(capacity)
        self.dtype = dtype_name(dtype)

    def update_features(self, side, feats):
        """one batch of feature rows [B][D] (f32, on the device); no host-device sync"""
        self.store.append(side, feats)

    def count(self, side):
        """rows held for a side"""
        return self.store.count(side)

    def rows(self, side):
        """the rows held for a side: f32 [n][D] on the device (a view of the buffer)"""
        return self.store.rows(side)

    def result(self):
        for side in SIDES:
            if self.count(side) <= self.k:
                raise RuntimeError('PRDC: the %s side holds %d rows; the %d-th nearest neighbour needs more than %d'
                                   % (side, self.count(side), self.k, self.k))
        real, fake = self.rows('real'), self.rows('fake')
        r_real = ops.prdc_knn_radius(real, self.k)
        r_fake = ops.prdc_knn_radius(fake, self.k)
        fake_in_real, _ = ops.prdc_ball_counts(fake, real, radius_b=r_real)
        real_in_fake, real_own = ops.prdc_ball_counts(real, fake, radius_a=r_real, radius_b=r_fake)
        counts = torch.cat([fake_in_real, real_in_fake, real_own]).cpu().numpy()        # the one read-back
        nf, nr = fake.shape[0], real.shape[0]
        return prdc_from_counts(counts[:nf], counts[nf:nf + nr], counts[nf + nr:], self.k, self.dtype)
