"""The distance between the real and the generated images in pixel space, per resolution: the sliced Wasserstein distance
(SWD) of Laplacian-pyramid patch descriptors of the progressive-GAN paper (Karras et al. 2018, section 5), written from
the paper's definition.  It needs no weights and no trunk, and reports one figure per pyramid level, finest first, x 10^3
as the paper's tables print it, and their average.

Per side, n images of S x S px (S in 32, 64, 128, 256), on the uint8 pixels the run writes to its PNG files, in float64:

  pyramid      L = log2(S / 16) + 1 levels per image and channel.  k = (1, 4, 6, 4, 1), K = k k^T / 256;
               G_{l+1} = conv(G_l, K)[::2, ::2];  up(G) = conv(Z, 4 K), Z zero except Z[::2, ::2] = G;  mirror boundary
               without repeating the edge sample (-1 -> 1, n -> n - 2);  Lap_l = G_l - up(G_{l+1}), Lap_{L-1} = G_{L-1}.
  descriptors  P = 128 patches of 7 x 7 x 3 per image and level, centres in [3, S_l - 4]; entry (c * 7 + dy) * 7 + dx =
               Lap_l[c][y - 3 + dy][x - 3 + dx].  Per level and side, over all n P descriptors, each channel's 49
               entries have that channel's mean subtracted and are divided by its population standard deviation.
  distance     per level 4 x 128 unit directions; both sides' descriptors are projected on a direction, each side's
               n P projections sorted, and mean |a_(i) - b_(i)| averaged over the 512 directions.

THE DRAWS all come from the evaluator's own numpy.random.RandomState(seed); the global generators are not touched.  Per
level, fine to coarse (S_l = S >> l, m = n P), in this order:

  1. randint(3, S_l - 3, m) four times: real x, real y, generated x, generated y (descriptor j belongs to image j // P);
  2. randn(147, 128) four times: the direction matrices, stacked to [147][512] and each column divided by
     sqrt(sum of its squares), in float64 on the host.

result() makes all draws, then runs the levels one after another through the four entry points of csrc/swd.hip
(ops.swd_descriptors, swd_project, swd_sort_columns, swd_abs_mean): only one level's descriptors and projections are live
at a time, in buffers allocated once.  The L x 512 means and the channel statistics come back in one copy.

Memory: the uint8 images of both sides (shared with an MSSSIM evaluator when one is given), one descriptor buffer of
n P 147 f64 and three projection buffers of 512 n P f64 (both sides and the sort's second buffer).
"""
import numpy as np
import torch

from . import ops
from .feature_rows import check_side
from .msssim import quantize

PATCHES = 128
DIR_REPEATS, DIRS_PER_REPEAT = 4, 128
DIRS = DIR_REPEATS * DIRS_PER_REPEAT
FIELDS = ('swd_x1e3', 'resolutions', 'swd_avg_x1e3', 'n_images', 'patches_per_image', 'dir_repeats', 'dirs_per_repeat',
          'size', 'levels', 'seed')


def draw(seed, size, n, patches=PATCHES, repeats=DIR_REPEATS, per_repeat=DIRS_PER_REPEAT):
    """every draw of one result(), in the order of the module docstring: a list over the levels, finest first, of
    (centres_real int32 [n P][2] {x, y}, centres_fake alike, dirs float64 [147][repeats * per_repeat], unit columns)"""
    levels = ops.swd_levels(size)
    rng = np.random.RandomState(seed)
    m, out = n * patches, []
    for lv in range(levels):
        Sl = size >> lv
        rx, ry, fx, fy = (rng.randint(3, Sl - 3, m) for _ in range(4))
        dirs = np.concatenate([rng.randn(ops.SWD_DESC, per_repeat) for _ in range(repeats)], axis=1)
        dirs = dirs / np.sqrt((dirs * dirs).sum(axis=0))
        out.append((np.stack([rx, ry], axis=1).astype(np.int32), np.stack([fx, fy], axis=1).astype(np.int32), dirs))
    return out


class SWD(object):
    """Collects the uint8 images of both sides, at most max_images a side (the first ones given; later ones are not
    stored).  size: the side of the square images, one of ops.SWD_SIZES; seed: of the draws; images: an MSSSIM
    evaluator whose buffers are read instead of keeping a second copy (update() then stores nothing)."""

    def __init__(self, max_images, size, seed=100, images=None, capacity=256):
        if isinstance(max_images, bool) or not isinstance(max_images, int) or max_images < 1:
            raise ValueError('SWD: max_images must be an integer >= 1 (got %r)' % (max_images,))
        self.levels = ops.swd_levels(size)
        if images is not None and getattr(images, 'size', None) != size:
            raise ValueError('SWD: the shared image store holds %r px images, not %d px'
                             % (getattr(images, 'size', None), size))
        if capacity < 1:
            raise ValueError('SWD: capacity must be >= 1 (got %d)' % capacity)
        self.max_images, self.size, self.seed, self.shared = max_images, int(size), int(seed), images
        self.capacity = min(int(capacity), max_images)
        self._held = {}                             # side -> [uint8 buffer [capacity][3][size][size], images held]

    def update(self, side, images):
        """one batch: images [B][3][size][size] float in [-1, 1] on the device; no host-device sync.  Images past
        max_images are dropped; with a shared store nothing is kept here."""
        side = check_side('SWD', side)
        shape = (3, self.size, self.size)
        if not torch.is_tensor(images) or images.dim() != 4 or tuple(images.shape[1:]) != shape:
            raise ValueError('SWD: images must be a [B]%s tensor (got %s)' % (
                ''.join('[%d]' % v for v in shape), tuple(images.shape) if torch.is_tensor(images) else type(images)))
        ops._need_gpu(images)
        if not images.is_floating_point():
            raise TypeError('SWD: images must be floating point in [-1, 1] (got %s)' % images.dtype)
        if self.shared is not None:
            return
        held = self._held.get(side)
        if held is None:
            held = self._held[side] = [torch.empty((self.capacity,) + shape, dtype=torch.uint8, device=images.device), 0]
        buf, n = held
        B = min(images.shape[0], self.max_images - n)
        if B <= 0:
            return
        if n + B > buf.shape[0]:
            cap = buf.shape[0]
            while cap < n + B:
                cap *= 2
            grown = torch.empty((min(cap, self.max_images),) + shape, dtype=torch.uint8, device=buf.device)
            grown[:n].copy_(buf[:n])
            buf = held[0] = grown
        buf[n:n + B].copy_(quantize(images[:B]))
        held[1] = n + B

    def count(self, side):
        """images that count for a side"""
        side = check_side('SWD', side)
        if self.shared is not None:
            return min(self.shared.count(side), self.max_images)
        held = self._held.get(side)
        return held[1] if held else 0

    def images(self, side):
        """the images of a side: uint8 [n][3][size][size] on the device (a view of the buffer)"""
        side = check_side('SWD', side)
        if self.shared is not None:
            return self.shared.images(side)[:self.max_images]
        held = self._held.get(side)
        if held is None:
            raise RuntimeError('SWD: the %s side holds no images' % side)
        return held[0][:held[1]]

    def result(self):
        n_real, n_fake = self.count('real'), self.count('fake')
        if n_real != n_fake or n_real < 1:
            raise RuntimeError('SWD: both sides must hold the same number of images, at least one: %d real, %d generated'
                               % (n_real, n_fake))
        n, m = n_real, n_real * PATCHES
        sides = (('real', self.images('real')), ('fake', self.images('fake')))
        dev = sides[0][1].device
        draws = draw(self.seed, self.size, n)       # (also keeps the host centres alive until the read-back)
        desc = torch.empty((m, ops.SWD_DESC), dtype=torch.float64, device=dev)
        proj = [torch.empty((DIRS, m), dtype=torch.float64, device=dev) for _ in range(3)]
        out = torch.empty((self.levels, DIRS + 12), dtype=torch.float64, device=dev)
        for lv, (c_real, c_fake, dirs) in enumerate(draws):
            dirs_dev = torch.from_numpy(dirs).to(dev)
            for s, ((_, imgs), centres) in enumerate(zip(sides, (c_real, c_fake))):
                _, stats = ops.swd_descriptors(imgs, lv, centres, desc=desc)
                ops.swd_project(desc, stats, dirs_dev, out=proj[s])
                ops.swd_sort_columns(proj[s], proj[2])
                out[lv, DIRS + 6 * s:DIRS + 6 * s + 6].copy_(stats)
            ops.swd_abs_mean(proj[0], proj[1], out=out[lv, :DIRS])
        host = out.cpu().numpy()                    # the one read-back
        count = float(m * ops.SWD_PATCH * ops.SWD_PATCH)
        for lv in range(self.levels):
            for s, (side, _) in enumerate(sides):
                st = host[lv, DIRS + 6 * s:DIRS + 6 * s + 6]
                var = st[3:] / count
                for c in range(3):
                    if not var[c] > 0.0:
                        raise RuntimeError('SWD: the %s side has zero deviation at level %d (%d px), channel %d: its '
                                           'descriptors cannot be normalised' % (side, lv, self.size >> lv, c))
        per_level = [float(host[lv, :DIRS].mean()) * 1e3 for lv in range(self.levels)]
        return {'swd_x1e3': per_level, 'resolutions': [self.size >> lv for lv in range(self.levels)],
                'swd_avg_x1e3': float(np.mean(per_level)), 'n_images': int(n), 'patches_per_image': PATCHES,
                'dir_repeats': DIR_REPEATS, 'dirs_per_repeat': DIRS_PER_REPEAT, 'size': int(self.size),
                'levels': int(self.levels), 'seed': self.seed}
