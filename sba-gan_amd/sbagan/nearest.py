"""Nearest training images and memorisation figures of generated images (--nearest K): what FID, KID, PRDC
and R-precision cannot see, because they compare the generated images with the evaluated split only -- a generator that
replays its training photos gets better under all of them.  On the project's own Inception-v3 trunk: the same f32 2048-d
pooled Mixed_7c rows FID uses (`InceptionHIP.last_pooled` / `pooled_features`).

Three sides, kept on the device as sbagan/feature_rows.py keeps them: 'train' (the training split's rows, with their
keys), 'real' (the evaluated split's real rows, as FID gets them: photos the generator never saw) and 'fake' (the generated
rows, with their keys).  result() makes four launches (the merge launch of a split one counts with it) and one read-back:

    d2_f, t_f = ops.knn_topk(fake, train, K)        the K nearest training rows of every generated row
    d2_r, t_r = ops.knn_topk(real, train, 1)        the nearest training row of every held-out real row
    r_T       = ops.prdc_knn_radius(train, 1)       a training row's squared distance to its nearest OTHER training row

all on the float64 squared distance of csrc/d2_tile.h, the same bits in the three.  With t*(x) the nearest training row
of x (ties to the smaller row number):

    authenticity        share of generated rows with d2(g, t*) > r_T[t*] (Alaa et al. 2022): strictly greater, so a NaN or
                        a missing neighbour counts against; authenticity_real: the same for the held-out real rows, the
                        baseline that goes with the figure
    nn_dist_fake / real median and mean of sqrt(d2(x, t*)); nn_ratio = median_fake / median_real: well below 1, the
                        generated images sit closer to the training set than unseen real photos do
    copy_fraction       share of generated rows with d2(g, t*) <= T, T the ceil(0.01 n_real)-th smallest d2(r, t*) over
                        the held-out real rows: about 0.01 for a generator that does not copy
    train_hit_distinct  distinct t* over the generated rows / min(n_fake, n_train)
    train_hit_max       the most generated rows that share one t*: collapse onto a few training images
    suspects            the M generated rows with the smallest d2(g, t*) (ties to the smaller row number): key, the K
                        squared distances and the K training keys

The trunk is the torchvision-lineage Inception-v3 of image_encoder*.pth run in the compute dtype, NOT the network of the
published implementations: the figures are comparable between runs of this project only.

The evaluator draws no random numbers; the training pass reads its images through retrieval.center_loader (centre window,
no flip, a torch.Generator of its own).
"""
import os

import numpy as np
import torch

from . import ops
from .feature_rows import Evaluator, FeatureRows, dtype_name
from .fid import stats_key                                          # noqa: F401  (the cache's key is FID's scheme)

SIDES = ('train', 'real', 'fake')
KEYED = ('train', 'fake')
FIELDS = ('authenticity', 'authenticity_real', 'nn_dist_fake', 'nn_dist_real', 'nn_ratio', 'copy_fraction',
          'copy_threshold', 'train_hit_distinct', 'train_hit_max', 'k', 'n_train', 'n_real', 'n_fake', 'n_nan', 'dtype',
          'suspects')
TILE = 128                                                          # side of a tile of nearest.png


def _lists(owner, what, d2, idx, k=None):
    d2, idx = np.asarray(d2, dtype=np.float64), np.asarray(idx)
    if d2.ndim == 1:
        d2, idx = d2[:, None], idx.reshape(-1, 1)
    if d2.ndim != 2 or d2.shape != idx.shape or d2.shape[0] < 1 or d2.shape[1] < 1 or (k and d2.shape[1] != k):
        raise ValueError('%s: %s lists must be [n >= 1][%s] distances with as many row numbers (got %s, %s)'
                         % (owner, what, k or 'k', d2.shape, idx.shape))
    if not np.issubdtype(idx.dtype, np.integer):
        raise ValueError('%s: %s row numbers must be integers' % (owner, what))
    return d2, idx.astype(np.int64)


def _side_figures(d2, idx, train_r2):
    """(authentic [n] bool, has a neighbour [n] bool, {'median', 'mean'} of sqrt(d2) over the rows that have one)"""
    has = idx[:, 0] >= 0
    own = np.where(has, train_r2[np.where(has, idx[:, 0], 0)], np.nan)
    with np.errstate(invalid='ignore'):
        authentic = has & (d2[:, 0] > own)                          # (a NaN on either side compares false)
    dist = np.sqrt(d2[has, 0])
    figures = {'median': float(np.median(dist)), 'mean': float(dist.mean())} if dist.size else \
        {'median': None, 'mean': None}
    return authentic, has, figures


def nearest_from_lists(fake_d2, fake_idx, real_d2, real_idx, train_r2, fake_keys=None, train_keys=None, show=16, dtype=''):
    """The result dict from the neighbour lists (host arithmetic only).
    fake_d2 / fake_idx [n_fake][K]: ops.knn_topk(fake, train, K), ascending, padded with +inf / -1;
    real_d2 / real_idx [n_real] or [n_real][1]: ops.knn_topk(real, train, 1);
    train_r2 [n_train]: ops.prdc_knn_radius(train, 1);
    fake_keys / train_keys: the names the suspects are reported by (row numbers when None); show: the number M of
    suspects."""
    fd, fi = _lists('nearest_from_lists', 'generated', fake_d2, fake_idx)
    rd, ri = _lists('nearest_from_lists', 'real', real_d2, real_idx, 1)
    r2 = np.asarray(train_r2, dtype=np.float64).reshape(-1)
    nf, nr, nt, k = fd.shape[0], rd.shape[0], r2.shape[0], fd.shape[1]
    if nt < 1 or max(int(fi.max()), int(ri.max())) >= nt or min(int(fi.min()), int(ri.min())) < -1:
        raise ValueError('nearest_from_lists: row numbers must lie in [-1, %d)' % nt)
    for what, keys, n in (('fake_keys', fake_keys, nf), ('train_keys', train_keys, nt)):
        if keys is not None and len(keys) != n:
            raise ValueError('nearest_from_lists: %d %s for %d rows' % (len(keys), what, n))
    show = int(show)
    if show < 0:
        raise ValueError('nearest_from_lists: show must be >= 0 (got %d)' % show)

    auth_f, has_f, dist_f = _side_figures(fd, fi, r2)
    auth_r, has_r, dist_r = _side_figures(rd, ri, r2)
    ratio = None
    if dist_f['median'] is not None and dist_r['median']:
        ratio = dist_f['median'] / dist_r['median']
    # the copy threshold: the ceil(n_real / 100)-th smallest nearest-training distance of the held-out real rows
    threshold = np.sort(np.where(has_r, rd[:, 0], np.inf))[-(-nr // 100) - 1]
    copies = has_f & (fd[:, 0] <= threshold)
    hits = np.bincount(fi[has_f, 0], minlength=nt)
    order = np.argsort(np.where(has_f, fd[:, 0], np.inf), kind='stable')        # (ties: the smaller row number first)
    suspects = []
    for g in order[:show]:
        if not has_f[g]:
            break
        listed = fi[g] >= 0
        suspects.append({'row': int(g), 'key': str(fake_keys[g]) if fake_keys is not None else int(g),
                         'd2': [float(v) for v in fd[g][listed]],
                         'train_rows': [int(j) for j in fi[g][listed]],
                         'train_keys': [str(train_keys[j]) if train_keys is not None else int(j) for j in fi[g][listed]]})
    return {'authenticity': float(np.count_nonzero(auth_f)) / nf,
            'authenticity_real': float(np.count_nonzero(auth_r)) / nr,
            'nn_dist_fake': dist_f, 'nn_dist_real': dist_r, 'nn_ratio': ratio,
            'copy_fraction': float(np.count_nonzero(copies)) / nf,
            'copy_threshold': float(threshold) if np.isfinite(threshold) else None,
            'train_hit_distinct': float(np.count_nonzero(hits)) / min(nf, nt),
            'train_hit_max': int(hits.max()),
            'k': int(k), 'n_train': int(nt), 'n_real': int(nr), 'n_fake': int(nf),
            'n_nan': int(nf - np.count_nonzero(has_f) + nr - np.count_nonzero(has_r)),
            'dtype': str(dtype), 'suspects': suspects}


def encode_train(dataset, features, batch, crop, resize, device, workers=0):
    """(rows [n][D] f32 on the device, keys): features(images) of every image of `dataset` in order, each prepared as
    retrieval._CenterCrops does (datasets.load_image, the middle `crop` px window, no flip, the data set's
    normalisation).  No global generator is touched."""
    from .retrieval import center_loader
    if len(dataset) < 1:
        raise ValueError('encode_train: the training split holds no image')
    rows = []
    with torch.no_grad():
        for imgs in center_loader(dataset, batch, crop, resize, workers):
            rows.append(features(imgs.to(device)).detach().float().clone())
    return torch.cat(rows, 0).contiguous(), [str(k) for k in dataset.filenames[:len(dataset)]]


class Nearest(Evaluator):
    """Collects the feature rows of the training, the real and the generated images.  features(images) -> f32 [B][D] on
    the device (an InceptionHIP's pooled_features, or any callable of that shape); k: training neighbours listed per
    generated row (1 .. 8); show: suspects reported; key: fid.stats_key() of this run's TRAINING pass, stored with cached
    training rows and checked on loading; dtype: the compute-dtype name reported in the result."""

    def __init__(self, features, D=2048, k=1, show=16, key='', dtype=None, capacity=256):
        self.store = FeatureRows('Nearest', D, capacity, sides=SIDES)
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= ops.KNN_MAX_K:
            raise ValueError('Nearest: k must be an integer in [1, %d] (got %r)' % (ops.KNN_MAX_K, k))
        if isinstance(show, bool) or not isinstance(show, int) or show < 0:
            raise ValueError('Nearest: show must be an integer >= 0 (got %r)' % (show,))
        self.features, self.D, self.k, self.show, self.key = features, int(D), k, show, str(key)
        self.dtype = dtype_name(dtype)
        self.keys = {side: [] for side in KEYED}
        self._loaded = False

    def update(self, side, images, keys=None):
        """one batch of images of a side, with their keys on the 'train' and 'fake' sides"""
        with torch.no_grad():
            feats = self.features(images)
        self.update_features(side, feats, keys)

    def update_features(self, side, feats, keys=None):
        """one batch of feature rows [B][D] (f32, on the device); no host-device sync.  keys: the B names of the rows of a
        'train' or 'fake' batch (their row numbers when None)"""
        first = self.store.count(side)
        if keys is not None and (not torch.is_tensor(feats) or len(keys) != feats.shape[0]):
            raise ValueError('Nearest: %d keys do not name the rows of this %s batch' % (len(keys), side))
        self.store.append(side, feats)
        if side in KEYED:
            self.keys[side].extend([str(k) for k in keys] if keys is not None else
                                   [str(first + b) for b in range(feats.shape[0])])

    def count(self, side):
        return self.store.count(side)

    def rows(self, side):
        return self.store.rows(side)

    def is_loaded(self):
        """whether load_train filled the training side (it then needs no pass)"""
        return self._loaded

    def save_train(self, path):
        """the training rows and keys with this run's key, as an .npz"""
        with open(path, 'wb') as f:
            np.savez(f, rows=self.rows('train').cpu().numpy(), keys=np.asarray(self.keys['train'], dtype=np.str_),
                     key=np.str_(self.key))

    def load_train(self, path, device):
        """the training side from save_train's file; ValueError when it was written under another key"""
        with np.load(path, allow_pickle=False) as z:
            key = str(z['key'])
            if key != self.key:
                raise ValueError('Nearest: %s holds training rows for\n  %s\nbut this run is\n  %s' % (path, key, self.key))
            rows, keys = z['rows'], [str(k) for k in z['keys']]
        if rows.ndim != 2 or rows.shape[1] != self.D or rows.shape[0] < 1 or rows.dtype != np.float32 \
                or len(keys) != rows.shape[0]:
            raise ValueError('Nearest: %s does not hold [n >= 1][%d] float32 rows with n keys' % (path, self.D))
        if self.count('train'):
            raise RuntimeError('Nearest: the training side already holds rows')
        self.update_features('train', torch.from_numpy(rows).to(device), keys)
        self._loaded = True

    def result(self):
        if self.count('train') < 2:
            raise RuntimeError('Nearest: the train side holds %d rows; a nearest other training row needs 2'
                               % self.count('train'))
        for side in ('real', 'fake'):
            if self.count(side) < 1:
                raise RuntimeError('Nearest: the %s side holds 0 rows' % side)
        train, real, fake = self.rows('train'), self.rows('real'), self.rows('fake')
        fd, fi = ops.knn_topk(fake, train, self.k)
        rd, ri = ops.knn_topk(real, train, 1)
        r2 = ops.prdc_knn_radius(train, 1)
        nf, nr, k = fake.shape[0], real.shape[0], self.k
        # the one read-back: the row numbers are exact in float64
        flat = torch.cat([fd.reshape(-1), fi.reshape(-1).double(), rd.reshape(-1), ri.reshape(-1).double(), r2])
        flat = flat.cpu().numpy()
        cuts = np.cumsum([0, nf * k, nf * k, nr, nr])
        fd, fi, rd, ri = (flat[cuts[s]:cuts[s + 1]] for s in range(4))
        return nearest_from_lists(fd.reshape(nf, k), fi.reshape(nf, k).astype(np.int64), rd, ri.astype(np.int64),
                                  flat[cuts[4]:], self.keys['fake'], self.keys['train'], self.show, self.dtype)


def write_sheet(path, suspects, k, fake_path, train_image):
    """<path>: one row per suspect -- the generated image (read back from fake_path(key)) and its nearest training images
    (train_image(row number) -> a PIL image), as TILE px tiles on a (1 + k) TILE wide sheet; places without a neighbour
    stay black.  Composed on the host with PIL: not a hot path.  No text is drawn."""
    from PIL import Image
    sheet = Image.new('RGB', ((1 + int(k)) * TILE, max(len(suspects), 1) * TILE))
    for r, s in enumerate(suspects):
        tiles = [Image.open(fake_path(s['key'])).convert('RGB')] + [train_image(j) for j in s['train_rows']]
        for c, img in enumerate(tiles):
            sheet.paste(img.resize((TILE, TILE), Image.BILINEAR), (c * TILE, r * TILE))
    sheet.save(path)
    return os.path.abspath(path)
