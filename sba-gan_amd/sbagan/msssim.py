"""Diversity within a class in pixel space, the measure of the AC-GAN paper (Odena et al. 2017): the mean multi-scale
structural similarity (MS-SSIM; Wang, Simoncelli, Bovik 2003) over random pairs of images of the SAME class, for the
generated images and, beside it, for the real images of the same pairs.  Lower means more diverse; a generated figure
well above the real one means collapse inside classes.  It needs no weights and no trunk.

Per pair and channel, on the uint8 pixels the run writes to its PNG files (L = 255, 11-tap Gaussian window of sigma
1.5 without padding, five scales of 2 x 2 mean pooling, a trailing odd row or column dropped):

    ms_ssim = prod_{s < 4} max(cs_s, 0)^w_s * max(ssim_4, 0)^w_4        w = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)

cs_s, ssim_s: the means of the contrast-structure term and of SSIM over the valid window positions of scale s
(csrc/msssim.hip, all arithmetic in float64); the three channels are averaged.  result() draws the pairs once from the
evaluator's OWN numpy.random.RandomState(seed), makes one launch of ops.msssim_pairs per side over the same pairs and
reads both outputs back in one copy.  The global numpy, torch and Python generators are not touched.

The images of both sides are kept on the device as uint8: n * 3 * H * W bytes a side (0.58 GB for the CUB test split at
256 px, 8 GB for COCO val).  Five scales need min(H, W) >> 4 >= 11: images of at least 176 px.
"""
import numpy as np
import torch

from . import ops
from .feature_rows import SIDES, check_side

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
SCALES = 5
MIN_SIZE = ops.MSSSIM_WINDOW << (SCALES - 1)        # 176
FIELDS = ('ms_ssim_fake', 'ms_ssim_real', 'ms_ssim_fake_std', 'ms_ssim_real_std', 'pairs', 'pairs_per_class', 'classes',
          'classes_skipped', 'n_images', 'size', 'scales', 'seed')


def quantize(images):
    """[B][3][H][W] float images in [-1, 1] -> uint8, with the torch operations that reproduce trainer._to_uint8 bit for
    bit: f32 + 1.0, * 127.5, clamp to [0, 255], truncate.  Stays on the device of `images`."""
    return ((images.detach().float() + 1.0) * 127.5).clamp(0, 255).to(torch.uint8)


def draw_pairs(class_ids, per_class, seed=100, with_counts=False):
    """int32 [P][2]: pairs (i < j) of positions of `class_ids` that hold the same class.  Classes in ascending id; a
    class with n_c >= 2 positions has n_c (n_c - 1) / 2 unordered pairs in lexicographic order, and when that is more
    than per_class, RandomState(seed).choice(total, per_class, replace=False), sorted ascending, picks among them (one
    RandomState for the whole call).  with_counts: (pairs, classes that gave pairs, classes skipped for holding fewer
    than two images)."""
    ids = np.asarray(class_ids).reshape(-1)
    if isinstance(per_class, bool) or not isinstance(per_class, (int, np.integer)) or per_class < 1:
        raise ValueError('draw_pairs: per_class must be an integer >= 1 (got %r)' % (per_class,))
    rng = np.random.RandomState(seed)
    out, used, skipped = [], 0, 0
    for c in np.unique(ids):
        pos = np.flatnonzero(ids == c)
        if pos.size < 2:
            skipped += 1
            continue
        used += 1
        i, j = np.triu_indices(pos.size, 1)             # row-major: the lexicographic order of (i, j)
        if i.size > per_class:
            pick = np.sort(rng.choice(i.size, int(per_class), replace=False))
            i, j = i[pick], j[pick]
        out.append(np.stack([pos[i], pos[j]], axis=1))
    pairs = (np.concatenate(out) if out else np.zeros((0, 2))).astype(np.int32)
    return (pairs, used, skipped) if with_counts else pairs


def combine(out):
    """[P] float64 from the per-scale means out [P][3][S][2] ({ssim, cs} last): per pair and channel
    v = (cs_0 .. cs_{S-2}, ssim_{S-1}) clipped at 0 and prod v^w with the first S of WEIGHTS, averaged over the
    channels"""
    out = np.asarray(out, dtype=np.float64)
    if out.ndim != 4 or out.shape[1] != 3 or out.shape[3] != 2 or not 1 <= out.shape[2] <= len(WEIGHTS):
        raise ValueError('combine: out must be [P][3][1 .. 5][2] (got %s)' % (out.shape,))
    S = out.shape[2]
    v = np.concatenate([out[:, :, :S - 1, 1], out[:, :, S - 1:, 0]], axis=2)
    v = np.maximum(v, 0.0)
    return np.prod(v ** np.asarray(WEIGHTS[:S]), axis=2).mean(axis=1)


class MSSSIM(object):
    """Collects the uint8 images of both sides with their class ids.  per_class: pairs drawn per class (100 is the AC-GAN
    setting); size: the side of the square images, at least 176; seed: of the pair draws."""

    def __init__(self, per_class, size=256, seed=100, capacity=256):
        if isinstance(per_class, bool) or not isinstance(per_class, int) or per_class < 1:
            raise ValueError('MSSSIM: per_class must be an integer >= 1 (got %r)' % (per_class,))
        if isinstance(size, bool) or not isinstance(size, int) or not MIN_SIZE <= size <= ops.MSSSIM_MAX_SIDE:
            raise ValueError('MSSSIM: %d scales of the %d-tap window need images of %d to %d px a side (got %r)'
                             % (SCALES, ops.MSSSIM_WINDOW, MIN_SIZE, ops.MSSSIM_MAX_SIDE, size))
        if capacity < 1:
            raise ValueError('MSSSIM: capacity must be >= 1 (got %d)' % capacity)
        self.per_class, self.size, self.seed, self.capacity = per_class, size, int(seed), int(capacity)
        self._held = {}                             # side -> [uint8 buffer [capacity][3][size][size], images held]
        self._ids = {side: [] for side in SIDES}    # side -> the class ids, on the host

    def update(self, side, images, class_ids):
        """one batch: images [B][3][size][size] float in [-1, 1] on the device, class_ids [B] on the host; no
        host-device sync"""
        side = check_side('MSSSIM', side)
        shape = (3, self.size, self.size)
        if not torch.is_tensor(images) or images.dim() != 4 or tuple(images.shape[1:]) != shape:
            raise ValueError('MSSSIM: images must be a [B]%s tensor (got %s)' % (
                ''.join('[%d]' % v for v in shape), tuple(images.shape) if torch.is_tensor(images) else type(images)))
        ops._need_gpu(images)
        if not images.is_floating_point():
            raise TypeError('MSSSIM: images must be floating point in [-1, 1] (got %s)' % images.dtype)
        ids = np.asarray(class_ids).reshape(-1)
        B = images.shape[0]
        if ids.size != B:
            raise ValueError('MSSSIM: %d images with %d class ids' % (B, ids.size))
        held = self._held.get(side)
        if held is None:
            held = self._held[side] = [torch.empty((self.capacity,) + shape, dtype=torch.uint8, device=images.device), 0]
        buf, n = held
        if n + B > buf.shape[0]:
            cap = buf.shape[0]
            while cap < n + B:
                cap *= 2
            grown = torch.empty((cap,) + shape, dtype=torch.uint8, device=buf.device)
            grown[:n].copy_(buf[:n])
            buf = held[0] = grown
        buf[n:n + B].copy_(quantize(images))
        held[1] = n + B
        self._ids[side].extend(int(v) for v in ids)

    def count(self, side):
        """images held for a side"""
        held = self._held.get(check_side('MSSSIM', side))
        return held[1] if held else 0

    def class_ids(self, side):
        """the class ids held for a side, int64 on the host"""
        return np.asarray(self._ids[check_side('MSSSIM', side)], dtype=np.int64)

    def images(self, side):
        """the images held for a side: uint8 [n][3][size][size] on the device (a view of the buffer)"""
        held = self._held.get(check_side('MSSSIM', side))
        if held is None:
            raise RuntimeError('MSSSIM: the %s side holds no images' % side)
        return held[0][:held[1]]

    def result(self):
        real_ids, fake_ids = self.class_ids('real'), self.class_ids('fake')
        if real_ids.size != fake_ids.size or not np.array_equal(real_ids, fake_ids):
            raise RuntimeError('MSSSIM: the two sides must hold the same images in the same order: %d real, %d generated '
                               'images%s' % (real_ids.size, fake_ids.size, '' if real_ids.size != fake_ids.size
                                             else ', and their class ids differ'))
        pairs, classes, skipped = draw_pairs(fake_ids, self.per_class, self.seed, with_counts=True)
        if not len(pairs):
            raise RuntimeError('MSSSIM: no class holds two images (%d images, %d classes): no pair to compare'
                               % (fake_ids.size, skipped))
        fake, real = self.images('fake'), self.images('real')
        pairs_dev = torch.from_numpy(pairs).to(fake.device)
        out = torch.stack([ops.msssim_pairs(fake, pairs_dev, SCALES),
                           ops.msssim_pairs(real, pairs_dev, SCALES)]).cpu().numpy()     # the one read-back
        f, r = combine(out[0]), combine(out[1])
        return {'ms_ssim_fake': float(f.mean()), 'ms_ssim_real': float(r.mean()), 'ms_ssim_fake_std': float(f.std()),
                'ms_ssim_real_std': float(r.std()), 'pairs': int(len(pairs)), 'pairs_per_class': int(self.per_class),
                'classes': int(classes), 'classes_skipped': int(skipped), 'n_images': int(fake_ids.size),
                'size': int(self.size), 'scales': SCALES, 'seed': self.seed}
