"""Frechet Inception Distance of generated images, on the project's own Inception-v3 trunk.

The feature of an image is the 2048-d pooled Mixed_7c output of the DAMSM image encoder's frozen trunk, in f32 as
InceptionHIP's global average pool writes it (`InceptionHIP.last_pooled` / `pooled_features`).  Per side ('real',
'fake') the moments are taken in float64 on the device: feature rows are appended to a staging buffer of `chunk` rows and
ops.fid_accumulate (the f64 matrix-core kernel of csrc/fid.hip) adds sum and X^T X when it fills, without a host-device
sync per batch; ops.fid_finalize gives the mean and the ddof = 1 covariance.  The distance itself is host numpy:

    FID = |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^(1/2)

with tr (S1 S2)^(1/2) = sum_i sqrt(max(lambda_i, 0)), lambda = eigvalsh(sym(A S2 A)), A = S1^(1/2) from eigh(S1):
symmetric eigensolves only, no complex sqrtm and no eps I added to rank-deficient covariances.  The value is returned
unclipped.  The trunk is the torchvision-lineage Inception-v3 of image_encoder*.pth run in the compute dtype, NOT the TF
pool3 graph of the published FID code: figures are comparable between runs of this project only.

The evaluator draws no random numbers.
"""
import numpy as np
import torch

from . import ops
from .feature_rows import SIDES, Evaluator, check_features, check_side, dtype_name

FIELDS = ('fid', 'n_real', 'n_fake', 'trace_real', 'trace_fake', 'mean_term', 'dtype')


def _psd_sqrt(S):
    w, V = np.linalg.eigh(S)
    return (V * np.sqrt(np.maximum(w, 0.0))) @ V.T


def fid_from_stats(mu1, S1, mu2, S2):
    """The Frechet distance between N(mu1, S1) and N(mu2, S2): numpy float64 on the host, unclipped."""
    mu1, mu2 = np.asarray(mu1, dtype=np.float64), np.asarray(mu2, dtype=np.float64)
    S1, S2 = np.asarray(S1, dtype=np.float64), np.asarray(S2, dtype=np.float64)
    D = mu1.shape[0]
    if mu1.shape != (D,) or mu2.shape != (D,) or S1.shape != (D, D) or S2.shape != (D, D):
        raise ValueError('fid_from_stats: mu must be [D] and S [D][D] (got %s, %s, %s, %s)'
                         % (mu1.shape, S1.shape, mu2.shape, S2.shape))
    A = _psd_sqrt(S1)
    M = A @ S2 @ A
    lam = np.linalg.eigvalsh((M + M.T) * 0.5)
    d = mu1 - mu2
    return float(d @ d + np.trace(S1) + np.trace(S2) - 2.0 * np.sqrt(np.maximum(lam, 0.0)).sum())


def stats_key(encoder_path, dtype, split, image_side):
    """what cached real-side statistics depend on: the image-encoder checkpoint, the compute dtype, the split and the
    side of the images"""
    return 'encoder=%s|dtype=%s|split=%s|side=%d' % (encoder_path, dtype, split, int(image_side))


def summarize(real, fake, dtype):
    """the result dict from two (n, mu, sigma, trace) tuples"""
    (n1, mu1, S1, t1), (n2, mu2, S2, t2) = real, fake
    d = np.asarray(mu1, dtype=np.float64) - np.asarray(mu2, dtype=np.float64)
    return {'fid': fid_from_stats(mu1, S1, mu2, S2), 'n_real': int(n1), 'n_fake': int(n2), 'trace_real': float(t1),
            'trace_fake': float(t2), 'mean_term': float(d @ d), 'dtype': str(dtype)}


class FID(Evaluator):
    """Accumulates the feature moments of real and generated images.  features(images) -> f32 [B][D] on the device (an
    InceptionHIP's pooled_features, or any callable of that shape); chunk: rows of the device staging buffer per
    accumulate launch; key: stats_key() of this run, stored with saved real statistics and checked on loading;
    dtype: the compute-dtype name reported in the result."""

    def __init__(self, features, D=2048, chunk=1024, key='', dtype=None):
        if D < 64 or D % 64:
            raise ValueError('FID: D must be a positive multiple of 64 (got %d)' % D)
        if chunk < 1:
            raise ValueError('FID: chunk must be >= 1 (got %d)' % chunk)
        self.features, self.D, self.chunk, self.key = features, int(D), int(chunk), str(key)
        self.dtype = dtype_name(dtype)
        self._acc = {}                              # side -> [staging, rows staged, rows in all, sum, gram]
        self._stats = {}                            # side -> (n, mu, sigma, trace) in numpy, once finalized or loaded
        self._loaded = set()

    def _side(self, side):
        return check_side('FID', side)

    def update_features(self, side, feats):
        """one batch of feature rows [B][D] (f32, on the device); no host-device sync"""
        side = self._side(side)
        if side in self._loaded:
            raise RuntimeError('FID: the %s side was loaded from a file and takes no more rows' % side)
        check_features('FID', feats, self.D)
        acc = self._acc.get(side)
        if acc is None:
            dev = feats.device
            acc = self._acc[side] = [torch.empty((self.chunk, self.D), dtype=torch.float32, device=dev), 0, 0,
                                     torch.zeros(self.D, dtype=torch.float64, device=dev),
                                     torch.zeros((self.D, self.D), dtype=torch.float64, device=dev)]
        self._stats.pop(side, None)
        staging, done, B = acc[0], 0, feats.shape[0]
        while done < B:
            take = min(B - done, self.chunk - acc[1])
            staging[acc[1]:acc[1] + take].copy_(feats[done:done + take])
            acc[1] += take
            done += take
            if acc[1] == self.chunk:
                self._flush(acc)
        acc[2] += B

    @staticmethod
    def _flush(acc):
        if acc[1]:
            ops.fid_accumulate(acc[0][:acc[1]], acc[3], acc[4])
            acc[1] = 0

    def is_loaded(self, side):
        """whether load_real filled this side (it then takes no rows)"""
        return self._side(side) in self._loaded

    def stats(self, side):
        """(n, mu [D], sigma [D][D]) of a side as numpy float64: flushes the staged rows and finalizes (one sync)"""
        return self._full_stats(side)[:3]

    def _full_stats(self, side):
        side = self._side(side)
        if side not in self._stats:
            acc = self._acc.get(side)
            if acc is None or acc[2] < 2:
                raise RuntimeError('FID: the %s side holds %d rows; a covariance needs at least 2'
                                   % (side, acc[2] if acc else 0))
            self._flush(acc)
            mu, sigma, trace = ops.fid_finalize(acc[3], acc[4], acc[2])
            self._stats[side] = (acc[2], mu.cpu().numpy(), sigma.cpu().numpy(), float(trace.cpu().numpy()[0]))
        return self._stats[side]

    def save_real(self, path):
        """the real side's n, mu, sigma (and trace) with this run's key, as an .npz"""
        n, mu, sigma, trace = self._full_stats('real')
        with open(path, 'wb') as f:
            np.savez(f, n=np.int64(n), mu=mu, sigma=sigma, trace=np.float64(trace), key=np.str_(self.key))

    def load_real(self, path):
        """the real side from save_real's file; ValueError when it was written under another key"""
        with np.load(path, allow_pickle=False) as z:
            key = str(z['key'])
            if key != self.key:
                raise ValueError('FID: %s holds statistics for\n  %s\nbut this run is\n  %s' % (path, key, self.key))
            n, trace = int(z['n']), float(z['trace'])
            mu, sigma = z['mu'].astype(np.float64), z['sigma'].astype(np.float64)
        if mu.shape != (self.D,) or sigma.shape != (self.D, self.D) or n < 2:
            raise ValueError('FID: %s does not hold [%d] / [%d][%d] statistics of n >= 2 rows'
                             % (path, self.D, self.D, self.D))
        self._acc.pop('real', None)
        self._stats['real'] = (n, mu, sigma, trace)
        self._loaded.add('real')

    def real_stats(self):
        """(n, mu, sigma, trace) of the real side, as load_real or the rows gave it"""
        return self._full_stats('real')

    def set_real(self, stats):
        """the real side from real_stats() of an evaluator under the same key (a file read once, kept by the caller);
        like load_real, the side then takes no rows"""
        n, mu, sigma, trace = stats
        if mu.shape != (self.D,) or sigma.shape != (self.D, self.D) or n < 2:
            raise ValueError('FID: the statistics handed over are not [%d] / [%d][%d] of n >= 2 rows' % (self.D, self.D, self.D))
        self._acc.pop('real', None)
        self._stats['real'] = (int(n), mu, sigma, float(trace))
        self._loaded.add('real')

    def result(self):
        return summarize(self._full_stats('real'), self._full_stats('fake'), self.dtype)
