"""The float64 numpy reference of the MS-SSIM evaluation, written from the definition (include/sbagan_hip.h,
sbagan/msssim.py), not from the kernel:

  * pixel values are the bytes 0 .. 255: L = 255, C1 = (0.01 L)^2, C2 = (0.03 L)^2;
  * the window g[k] = exp(-(k - 5)^2 / (2 * 1.5^2)), k = 0 .. 10, normalised to sum 1, applied separably, no padding;
  * scale s works on the image pooled s times by a 2 x 2 mean, a trailing odd row or column dropped;
  * per position mx, my, sxx = E[xx] - mx^2, syy, sxy, cs = (2 sxy + C2) / (sxx + syy + C2),
    ssim = cs * (2 mx my + C1) / (mx^2 + my^2 + C1); the mean over the (Hs - 10) x (Ws - 10) positions.

`order` picks one of two summation orders of the same definition ('rows': filter along the rows first, taps ascending,
numpy's pairwise mean; 'cols': down the columns first, taps descending, the mean as an exactly rounded math.fsum);
`dtype` evaluates the same lines in another precision (float32: what the bound of the GPU test must tell apart)."""
import math

import numpy as np

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
WIN = 11
KINDS = ('noise', 'smooth', 'noisy_copy', 'flat', 'identical', 'inverted')


def window(dtype=np.float64):
    k = np.arange(WIN, dtype=np.float64)
    g = np.exp(-(k - 5.0) ** 2 / (2.0 * 1.5 ** 2))
    return (g / g.sum()).astype(dtype)


def pool(a):
    """2 x 2 mean over the last two axes, a trailing odd row or column dropped"""
    H, W = a.shape[-2] // 2 * 2, a.shape[-1] // 2 * 2
    a = a[..., :H, :W]
    return (a[..., 0::2, 0::2] + a[..., 0::2, 1::2] + a[..., 1::2, 0::2] + a[..., 1::2, 1::2]) / a.dtype.type(4)


def _filter(a, g, order):
    """the valid 11 x 11 separable window over the last two axes"""
    taps = range(WIN) if order == 'rows' else range(WIN - 1, -1, -1)

    def along(a, axis):
        n = a.shape[axis] - WIN + 1
        acc = np.zeros(a.shape[:axis] + (n,) + a.shape[axis + 1:], dtype=a.dtype)
        for k in taps:
            acc = acc + g[k] * np.take(a, np.arange(k, k + n), axis=axis)
        return acc
    nd = a.ndim
    return along(along(a, nd - 1), nd - 2) if order == 'rows' else along(along(a, nd - 2), nd - 1)


def _mean(a, order):
    """the mean over the last two axes"""
    if order == 'rows':
        return a.mean(axis=(-2, -1))
    flat = a.reshape(a.shape[:-2] + (-1,))
    out = np.empty(flat.shape[:-1], dtype=a.dtype)
    for idx in np.ndindex(*flat.shape[:-1]):
        out[idx] = math.fsum(float(v) for v in flat[idx]) / flat.shape[-1]
    return out


def scale_means(x, y, scales, order='rows', dtype=np.float64):
    """[...][scales][2] ({mean ssim, mean cs} last) of the images x, y [...][H][W] (any leading axes, e.g. the channel)"""
    t = np.dtype(dtype).type
    x, y = np.asarray(x).astype(dtype), np.asarray(y).astype(dtype)
    g = window(dtype)
    C1, C2 = t((0.01 * 255.0) ** 2), t((0.03 * 255.0) ** 2)
    out = np.empty(x.shape[:-2] + (scales, 2), dtype=dtype)
    for s in range(scales):
        if s:
            x, y = pool(x), pool(y)
        mx, my = _filter(x, g, order), _filter(y, g, order)
        sxx = _filter(x * x, g, order) - mx * mx
        syy = _filter(y * y, g, order) - my * my
        sxy = _filter(x * y, g, order) - mx * my
        cs = (t(2) * sxy + C2) / (sxx + syy + C2)
        ssim = cs * (t(2) * mx * my + C1) / (mx * mx + my * my + C1)
        out[..., s, 0] = _mean(ssim, order)
        out[..., s, 1] = _mean(cs, order)
    return out


def pair_means(imgs, pairs, scales, order='rows', dtype=np.float64):
    """[P][3][scales][2]: scale_means of imgs[i], imgs[j] for every pair (i, j); NaN for a pair that names an image
    outside [0, n)"""
    imgs, pairs = np.asarray(imgs), np.asarray(pairs)
    out = np.full((len(pairs), imgs.shape[1], scales, 2), np.nan, dtype=dtype)
    for p, (i, j) in enumerate(pairs):
        if 0 <= i < len(imgs) and 0 <= j < len(imgs):
            out[p] = scale_means(imgs[i], imgs[j], scales, order, dtype)
    return out


def factors(out):
    """[P][3][S]: (cs_0 .. cs_{S-2}, ssim_{S-1}) clipped at 0"""
    out = np.asarray(out, dtype=np.float64)
    S = out.shape[2]
    return np.maximum(np.concatenate([out[:, :, :S - 1, 1], out[:, :, S - 1:, 0]], axis=2), 0.0)


def combine(out):
    """[P]: prod v^w over the scales with the first S weights, averaged over the channels"""
    v = factors(out)
    res = np.ones(v.shape[:2])
    for s in range(v.shape[2]):
        res = res * v[:, :, s] ** WEIGHTS[s]
    return res.mean(axis=1)


def kinds(H, W, seed=0):
    """{kind: (x, y)}, uint8 [3][H][W] each: the six kinds of input the bounds were measured on"""
    rng = np.random.RandomState(seed)
    noise_x, noise_y = rng.randint(0, 256, (2, 3, H, W))
    yy, xx = np.mgrid[0:H, 0:W]
    smooth = np.stack([127.5 + 120.0 * np.sin(xx / (7.0 + c) + c) * np.cos(yy / (11.0 - c)) for c in range(3)])
    smooth_y = np.stack([127.5 + 100.0 * np.sin(xx / (7.0 + c) + c + 0.6) * np.cos(yy / (11.0 - c) + 0.4) for c in range(3)])
    noisy = np.clip(smooth + rng.normal(0.0, 12.0, smooth.shape), 0, 255)
    flat_a, flat_b = np.full((3, H, W), 255), np.full((3, H, W), 254)
    checker = ((xx // 3 + yy // 5) % 2 * 255)[None].repeat(3, axis=0)
    u8 = lambda a: np.asarray(a).astype(np.uint8)        # noqa: E731
    return {'noise': (u8(noise_x), u8(noise_y)), 'smooth': (u8(smooth), u8(smooth_y)), 'noisy_copy': (u8(smooth), u8(noisy)),
            'flat': (u8(flat_a), u8(flat_b)), 'identical': (u8(noise_x), u8(noise_x)),
            'inverted': (u8(checker), u8(255 - checker))}


def kind_stack(H, W, seed=0):
    """(imgs uint8 [12][3][H][W], pairs int32 [8][2]): the six kinds as one image stack, pair k = images (2 k, 2 k + 1),
    then a pair (i, i) and a second use of images already paired, so an image serves several pairs"""
    ks = kinds(H, W, seed)
    imgs = np.stack([im for kind in KINDS for im in ks[kind]])
    pairs = [(2 * k, 2 * k + 1) for k in range(len(KINDS))] + [(3, 3), (5, 0)]
    return imgs, np.asarray(pairs, dtype=np.int32)
