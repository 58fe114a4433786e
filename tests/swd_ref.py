"""Reference of the sliced Wasserstein distance of sbagan/swd.py in numpy, written from the definition (Karras et al.
2018, section 5), every step a function of its own, in float64 or -- with dtype=numpy.longdouble -- in extended
precision.  The draws are arguments; draws() makes them in the stated order:

    per level, fine to coarse, from ONE numpy.random.RandomState(seed):
      randint(3, S_l - 3, n P) for real x, real y, generated x, generated y, then four randn(147, 128) matrices,
      stacked to [147][512], every column scaled to unit length in float64.

The knobs `boundary`, `ddof` and `order` exist for the tests that show a wrong kernel is caught: the definition is
boundary='reflect' (mirror without repeating the edge sample), ddof=0, order='cyx'.

The error bounds of tests/test_swd_gpu.py live here as well, so that tests/test_swd_cpu.py can show on an emulated
kernel that a correct one passes them and a wrong one does not.
"""
import math

import numpy as np

K1 = np.array([1.0, 4.0, 6.0, 4.0, 1.0])
PATCH, DESC, PATCHES, REPEATS, PER_REPEAT = 7, 147, 128, 4, 128
U = 2.0 ** -53
SIZES = (32, 64, 128, 256)


def levels_of(size):
    assert size in SIZES, size
    return int(math.log2(size // 16)) + 1


def draws(seed, size, n, patches=PATCHES, repeats=REPEATS, per_repeat=PER_REPEAT):
    """list over the levels of (centres_real [n P][2] {x, y}, centres_fake, dirs [147][repeats * per_repeat])"""
    rng = np.random.RandomState(seed)
    out = []
    for lv in range(levels_of(size)):
        Sl = size >> lv
        pos = [rng.randint(3, Sl - 3, n * patches) for _ in range(4)]
        mats = [rng.randn(DESC, per_repeat) for _ in range(repeats)]
        dirs = np.concatenate(mats, axis=1)
        dirs = dirs / np.sqrt((dirs * dirs).sum(axis=0))
        out.append((np.stack(pos[0:2], axis=1), np.stack(pos[2:4], axis=1), dirs))
    return out


def conv5(x, kern, boundary='reflect', reverse=False):
    """x [..., H, W] filtered by the 5 x 5 kernel with the mirrored boundary, the 25 taps added in order (or reversed)"""
    pad = [(0, 0)] * (x.ndim - 2) + [(2, 2), (2, 2)]
    xp = np.pad(x, pad, mode=boundary)
    H, W = x.shape[-2:]
    taps = [(i, j) for i in range(5) for j in range(5)]
    if reverse:
        taps = taps[::-1]
    out = np.zeros_like(x)
    for i, j in taps:
        out = out + kern[i, j] * xp[..., i:i + H, j:j + W]
    return out


def down(g, boundary='reflect', reverse=False):
    K = (np.outer(K1, K1) / 256.0).astype(g.dtype)
    return conv5(g, K, boundary, reverse)[..., ::2, ::2]


def up(g, boundary='reflect', reverse=False):
    K = (np.outer(K1, K1) / 64.0).astype(g.dtype)            # 4 K
    z = np.zeros(g.shape[:-2] + (2 * g.shape[-2], 2 * g.shape[-1]), dtype=g.dtype)
    z[..., ::2, ::2] = g
    return conv5(z, K, boundary, reverse)


def laplacian_pyramid(images, levels=None, dtype=np.float64, boundary='reflect', reverse=False):
    """images [..., S, S] uint8 -> the list of Laplacian levels, finest first, the last one the Gaussian level"""
    g = np.asarray(images).astype(dtype)
    levels = levels_of(g.shape[-1]) if levels is None else levels
    out = []
    for _ in range(levels - 1):
        nxt = down(g, boundary, reverse)
        out.append(g - up(nxt, boundary, reverse))
        g = nxt
    out.append(g)
    return out


def gather(lap, centres, patches, order='cyx'):
    """lap [n][3][Sl][Sl], centres [n P][2] {x, y} -> descriptors [n P][147], entry (c * 7 + dy) * 7 + dx"""
    c = np.asarray(centres).astype(np.int64)
    m = c.shape[0]
    img = (np.arange(m) // patches)[:, None, None, None]
    ch = np.arange(3)[None, :, None, None]
    ys = (c[:, 1, None] - 3 + np.arange(PATCH))[:, None, :, None]
    xs = (c[:, 0, None] - 3 + np.arange(PATCH))[:, None, None, :]
    d = lap[img, ch, ys, xs]                                # [m][3][7][7]
    if order == 'yxc':
        d = d.transpose(0, 2, 3, 1)
    return np.ascontiguousarray(d).reshape(m, DESC)


def descriptors(images, level, centres, patches, dtype=np.float64, boundary='reflect', order='cyx'):
    return gather(laplacian_pyramid(images, dtype=dtype, boundary=boundary)[level], centres, patches, order)


def channel_stats(desc, ddof=0):
    """(mean [3], deviation [3]) over all the values of a channel (entries 49 c .. 49 c + 48 of every descriptor)"""
    d = desc.reshape(desc.shape[0], 3, PATCH * PATCH)
    return d.mean(axis=(0, 2)), d.std(axis=(0, 2), ddof=ddof)


def normalise(desc, ddof=0):
    mu, sd = channel_stats(desc, ddof)
    d = desc.reshape(desc.shape[0], 3, PATCH * PATCH)
    return ((d - mu[None, :, None]) / sd[None, :, None]).reshape(desc.shape)


def project(desc, dirs, ddof=0):
    """[D][m]: the normalised descriptors on every direction, direction-major"""
    return (normalise(desc, ddof) @ dirs.astype(desc.dtype)).T


def level_distance(desc_real, desc_fake, dirs, ddof=0):
    a = np.sort(project(desc_real, dirs, ddof), axis=1)
    b = np.sort(project(desc_fake, dirs, ddof), axis=1)
    return np.abs(a - b).mean(axis=1).mean()


def swd(real, fake, drawn, patches=PATCHES, dtype=np.float64, boundary='reflect', ddof=0, order='cyx'):
    """the distance per level, finest first (NOT x 1e3), of uint8 [n][3][S][S] stacks under the draws `drawn`"""
    pr = laplacian_pyramid(real, dtype=dtype, boundary=boundary)
    pf = laplacian_pyramid(fake, dtype=dtype, boundary=boundary)
    out = []
    for lv, (cr, cf, dirs) in enumerate(drawn):
        out.append(level_distance(gather(pr[lv], cr, patches, order), gather(pf[lv], cf, patches, order), dirs, ddof))
    return np.array(out, dtype=dtype)


# ---------------------------------------------------------------------------------------------------------------------
# the bounds of the GPU tests
def sum_bound(x):
    """a sum of the values x in ANY order against math.fsum: (count - 1) u sum |x|"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    return (x.size - 1) * U * math.fsum(np.abs(x))


def projection_bound(desc, dirs):
    """[D][m]: how far a float64 evaluation of sba_swd_project may lie from project(desc, dirs), to first order in u.

    The kernel computes out = sum_k (d_k - mu_c) w_k with w_k = dir_k / sigma_c, from mu_c = s1 / N and
    sigma_c^2 = s2 / N (N = 49 m values a channel; s1 their sum, s2 the sum of their squared deviations from mu_c, taken
    in a second pass).

    1. The contraction: 148 terms, each product rounded once; d_k - mu_c and w_k each carry one rounding more:
       (148 + 2) u sum_k |(d_k - mu_c) w_k|.
    2. The statistics.  A sum of N values in ANY order is within (N - 1) u sum|x| of the true one, so with the division
       |d mu_c| <= N u mean|x|.  Every term (x - mu)^2 of s2 carries two roundings and the sum (N - 1) u more; the
       error of mu enters s2 only in second order (sum (x - mu) = 0).  So sigma^2 is off by the relative amount
       (N + 2) u, and sigma, after the division, the square root and the reciprocal, by e = (N + 2) u / 2 + 3 u.
       (The kernel's sums are compensated and do far better; the bound does not rely on it.)
       out moves by at most sum_c ( |d mu_c| sum_{k in c} |w_k|  +  e sum_{k in c} |(d_k - mu_c) w_k| ).
    """
    desc = np.asarray(desc, dtype=np.float64)
    m = desc.shape[0]
    N = float(m * PATCH * PATCH)
    d3 = desc.reshape(m, 3, PATCH * PATCH)
    mu, sd = channel_stats(desc)
    dmu = N * U * np.abs(d3).mean(axis=(0, 2))
    e = np.full(3, (N + 2.0) * U / 2.0 + 3.0 * U)
    ch = np.repeat(np.arange(3), PATCH * PATCH)
    w = np.abs(dirs / sd[ch][:, None])                                      # [147][D]
    centred = np.abs(desc - mu[ch][None, :])
    contraction = (148 + 2) * U * (centred @ w)
    stats = (dmu[ch] @ w)[None, :] + (centred * e[ch][None, :]) @ w
    return (contraction + stats).T


def abs_mean_bound(a, b):
    """[D]: (m - 1) u sum |a - b| per column"""
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    return (d.shape[1] - 1) * U * np.array([math.fsum(row) for row in d])


def abs_mean(a, b):
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    return np.array([math.fsum(row) for row in d]) / d.shape[1]


def end_to_end_bound(real, fake, drawn, patches=PATCHES):
    """(reference per level in float64, the allowed error per level): 16 x the largest per-level difference between the
    float64 and the extended-precision evaluation of this reference, as the same shapes"""
    r64 = swd(real, fake, drawn, patches, dtype=np.float64)
    rld = swd(real, fake, drawn, patches, dtype=np.longdouble)
    diff = float(np.abs(r64.astype(np.longdouble) - rld).max())
    return r64, rld, diff, 16.0 * diff


def make_images(size, n, seed):
    """uint8 [n][3][size][size]: smooth structure plus noise, different per image and channel"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:size, 0:size]
    x = np.stack([[127.5 + 80.0 * np.sin(xx / (3.0 + i + c) + seed) * np.cos(yy / (5.0 + 2 * c + i)) for c in range(3)]
                  for i in range(n)])
    return np.clip(x + rng.normal(0.0, 25.0, x.shape), 0, 255).astype(np.uint8)
