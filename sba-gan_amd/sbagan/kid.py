"""Kernel Inception Distance of generated images (Binkowski et al. 2018, "Demystifying MMD GANs"): the unbiased estimate
of the squared maximum mean discrepancy between real and generated feature rows under the polynomial kernel

    k(x, y) = (x . y / D + 1)^3                     gamma = 1 / D, coef0 = 1, degree 3

on the project's own Inception-v3 trunk -- the same f32 2048-d pooled Mixed_7c rows FID and PRDC use
(`InceptionHIP.last_pooled` / `pooled_features`).  Unlike FID it is unbiased at small sample counts (the CUB test split
has 2 933 images) and comes with a standard deviation over subsets.

S subsets; each takes m = min(subset_size, n_real, n_fake) rows a side, drawn without replacement.  Per subset

    mmd2 = Sxx / (m (m - 1)) + Syy / (m (m - 1)) - 2 Sxy / (m m)

Sxx, Syy: k summed over the pairs of DIFFERENT positions of the subset (the diagonal is left out by position, never
subtracted), Sxy over all m m pairs.  kid = the mean of mmd2 over the subsets, kid_std their population standard
deviation.  result() makes three launches of the f64 matrix-core kernel-sum kernel of csrc/kid.hip
(ops.kid_kernel_sums: xx, yy, xy, every subset of a term in one launch, rows gathered by index) and reads the 3 S sums
back in one copy.

The subset indices come from the evaluator's OWN numpy.random.RandomState(seed): choice(n, m, replace=False) for the S
subsets of the real side, then for the S subsets of the generated side.  The global numpy, torch and Python generators
are not touched, and the same seed and row counts give the same subsets.

The trunk is the torchvision-lineage Inception-v3 of image_encoder*.pth run in the compute dtype, NOT the network of the
published implementations: the figures are comparable between runs of this project only.
"""
import numpy as np
import torch

from . import ops
from .feature_rows import SIDES, Evaluator, FeatureRows, dtype_name

FIELDS = ('kid', 'kid_std', 'subsets', 'subset_size', 'n_real', 'n_fake', 'degree', 'coef0', 'gamma', 'dtype', 'seed')


def draw_subsets(n_real, n_fake, m, subsets, seed):
    """(idx_real, idx_fake), int32 [subsets][m] each: row numbers without replacement within a subset, from a private
    RandomState(seed); the real side's `subsets` draws come first, then the generated side's"""
    rng = np.random.RandomState(seed)
    return tuple(np.stack([rng.choice(n, m, replace=False) for _ in range(subsets)]).astype(np.int32)
                 for n in (n_real, n_fake))


def kid_from_sums(sxx, syy, sxy, m, n_real=None, n_fake=None, D=2048, dtype='', seed=None):
    """The result dict from the kernel sums of the subsets (host arithmetic only): sxx, syy [S]: the sums over pairs of
    different positions within the real / the generated subset; sxy [S]: over all m m cross pairs; m: rows per subset
    and side.  n_real, n_fake (default m), D (gamma = 1 / D), dtype and seed are reported as given."""
    sxx, syy, sxy = (np.asarray(v, dtype=np.float64) for v in (sxx, syy, sxy))
    m = int(m)
    if sxx.ndim != 1 or sxx.size < 1 or syy.shape != sxx.shape or sxy.shape != sxx.shape:
        raise ValueError('kid_from_sums: the sums must be three vectors of one length >= 1 (got %s, %s, %s)'
                         % (sxx.shape, syy.shape, sxy.shape))
    if m < 2:
        raise ValueError('kid_from_sums: a subset needs m >= 2 rows a side (got %d)' % m)
    mmd2 = sxx / (m * (m - 1.0)) + syy / (m * (m - 1.0)) - 2.0 * sxy / (float(m) * m)
    return {'kid': float(mmd2.mean()), 'kid_std': float(mmd2.std()), 'subsets': int(sxx.size), 'subset_size': m,
            'n_real': int(m if n_real is None else n_real), 'n_fake': int(m if n_fake is None else n_fake),
            'degree': 3, 'coef0': 1.0, 'gamma': 1.0 / int(D), 'dtype': str(dtype),
            'seed': None if seed is None else int(seed)}


class KID(Evaluator):
    """Collects the feature rows of real and generated images.  features(images) -> f32 [B][D] on the device (an
    InceptionHIP's pooled_features, or any callable of that shape); subsets (1 .. 1024) of at most subset_size (>= 2)
    rows a side; seed: of the subset draws; key: a description of the run, kept for the caller; dtype: the
    compute-dtype name reported in the result.  rows: a sbagan.prdc.PRDC (or anything with its `store`) whose rows
    are read instead of storing them a second time -- update / update_features then belong to that evaluator and are
    refused here."""

    def __init__(self, features, D=2048, subsets=100, subset_size=1000, seed=100, key='', dtype=None, rows=None,
                 capacity=256):
        for name, v, lo, hi in (('subsets', subsets, 1, ops.KID_MAX_SUBSETS), ('subset_size', subset_size, 2, None)):
            if isinstance(v, bool) or not isinstance(v, int) or v < lo or (hi is not None and v > hi):
                raise ValueError('KID: %s must be an integer %s (got %r)'
                                 % (name, 'in [%d, %d]' % (lo, hi) if hi is not None else '>= %d' % lo, v))
        if rows is not None and rows.store.D != D:
            raise ValueError('KID: the shared rows are %d wide, not %d' % (rows.store.D, D))
        self.shared = rows is not None
        self.store = rows.store if self.shared else FeatureRows('KID', D, capacity)
        self.features, self.D, self.subsets, self.subset_size = features, int(D), subsets, subset_size
        self.seed, self.key = int(seed), str(key)
        self.dtype = dtype_name(dtype)

    def update_features(self, side, feats):
        """one batch of feature rows [B][D] (f32, on the device); no host-device sync"""
        if self.shared:
            raise RuntimeError('KID: the rows belong to the evaluator given as rows=; feed that one')
        self.store.append(side, feats)

    def count(self, side):
        """rows held for a side"""
        return self.store.count(side)

    def rows(self, side):
        """the rows held for a side: f32 [n][D] on the device (a view of the buffer)"""
        return self.store.rows(side)

    def result(self):
        for side in SIDES:
            if self.count(side) < 2:
                raise RuntimeError('KID: the %s side holds %d rows; a subset needs at least 2' % (side, self.count(side)))
        real, fake = self.rows('real'), self.rows('fake')
        m = min(self.subset_size, real.shape[0], fake.shape[0])
        idx_real, idx_fake = draw_subsets(real.shape[0], fake.shape[0], m, self.subsets, self.seed)
        sums = torch.cat([ops.kid_kernel_sums(real, real, idx_real, idx_real, exclude_diag=True),
                          ops.kid_kernel_sums(fake, fake, idx_fake, idx_fake, exclude_diag=True),
                          ops.kid_kernel_sums(real, fake, idx_real, idx_fake)]).cpu().numpy()    # the one read-back
        S = self.subsets
        return kid_from_sums(sums[:S], sums[S:2 * S], sums[2 * S:], m, real.shape[0], fake.shape[0], self.D, self.dtype,
                             self.seed)
