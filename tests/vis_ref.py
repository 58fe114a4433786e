"""Float64 reference of the attention-map overlays (sbagan/visualize.py), independent of the code under test: maps are
expanded by scipy.ndimage (zoom, then gaussian_filter), blended by PIL's own paste, laid out in numpy.  Besides every
canvas it returns, per pixel, the float64 value that was truncated to the byte and the width of the band around an
integer inside which an f32 implementation may land on the neighbouring byte."""
import numpy as np
from PIL import Image
from scipy import ndimage

BAND, PAD = 50, 2
U = 2.0 ** -24


def expand(x, up):
    """[a][a] float64 -> [a up][a up]: bilinear half-pixel resize, Gaussian sigma 20 / radius 80, symmetric reflect"""
    x = np.asarray(x, dtype=np.float64)
    if up <= 1:
        return x.copy()
    z = ndimage.zoom(x, up, order=1, mode='reflect', grid_mode=True)
    return ndimage.gaussian_filter(z, sigma=20, mode='reflect', truncate=4.0)


def expand_tol(a, up, absmax):
    """|f32 kernel - float64| bound of one expanded value.  The kernel evaluates M x M^T as two passes of sequential f32
    FMA sums of length a whose weights are non-negative and sum to 1 (n u max|x| per pass, as score_tol of the
    R-precision tests), on operator entries rounded once to f32 (u relative per factor, two factors), plus the final
    rounding; nothing for up <= 1 (a copy)."""
    return 0.0 if up <= 1 else (2 * a + 4) * U * absmax


def conf_tol(a, sumabs):
    """a sum of n = a^2 f32 terms in ANY fixed order is within (n - 1) u sum|x| of the exact one"""
    return a * a * U * sumabs


def image_values(img, V):
    """[3][S][S] float64 in [-1, 1] -> the [V][V][3] values (x + 1) 127.5 clamped to [0, 255] after a bilinear
    align_corners resize"""
    img = np.asarray(img, dtype=np.float64)
    S = img.shape[1]
    if S != V:
        pos = np.arange(V) * (S - 1) / max(V - 1, 1)
        i0 = np.minimum(np.floor(pos).astype(np.int64), S - 1)
        i1 = np.minimum(i0 + 1, S - 1)
        f = pos - i0
        rows = img[:, i0, :] * (1 - f)[None, :, None] + img[:, i1, :] * f[None, :, None]
        img = rows[:, :, i0] * (1 - f)[None, None, :] + rows[:, :, i1] * f[None, None, :]
    return np.clip((np.transpose(img, (1, 2, 0)) + 1.0) * 127.5, 0.0, 255.0)


IMAGE_DELTA = 2.0 ** -20 * 255


def pil_blend(map_u8, img_u8, m):
    """PIL's paste of a gray map [V][V] over an RGB image [V][V][3] with the constant mask m"""
    base = Image.fromarray(img_u8, 'RGB')
    top = Image.fromarray(np.repeat(map_u8[:, :, None], 3, 2), 'RGB')
    mask = Image.new('L', base.size, int(m))
    base.paste(top, (0, 0), mask)
    return np.asarray(base)


class Canvas(object):
    """canvas: the uint8 picture; value: the float64 each byte was truncated from (NaN where the byte is exact by
    construction: pads, bands, black slots); delta: the half-width around an integer where +-1 is allowed; src: for
    blends, (map byte, image byte value arrays) are re-blended by the test when a neighbour byte is allowed"""

    def __init__(self, H, W):
        self.canvas = np.zeros((H, W, 3), dtype=np.uint8)
        self.kind = np.zeros((H, W), dtype=np.int8)            # 0 exact, 1 image, 2 map, 3 blend
        self.map_value = np.full((H, W), np.nan)
        self.map_delta = np.zeros((H, W))
        self.img_value = np.full((H, W, 3), np.nan)
        self.mask = np.zeros((H, W), dtype=np.int32)

    def put_image(self, y, x, vals):
        V = vals.shape[0]
        self.canvas[y:y + V, x:x + V] = vals.astype(np.uint8)
        self.kind[y:y + V, x:x + V] = 1
        self.img_value[y:y + V, x:x + V] = vals

    def put_map(self, y, x, vals, delta):
        V = vals.shape[0]
        self.canvas[y:y + V, x:x + V] = vals.astype(np.uint8)[:, :, None]
        self.kind[y:y + V, x:x + V] = 2
        self.map_value[y:y + V, x:x + V] = vals
        self.map_delta[y:y + V, x:x + V] = delta

    def put_blend(self, y, x, vals, delta, img_vals, m):
        V = vals.shape[0]
        self.canvas[y:y + V, x:x + V] = pil_blend(vals.astype(np.uint8), img_vals.astype(np.uint8), m)
        self.kind[y:y + V, x:x + V] = 3
        self.map_value[y:y + V, x:x + V] = vals
        self.map_delta[y:y + V, x:x + V] = delta
        self.img_value[y:y + V, x:x + V] = img_vals
        self.mask[y:y + V, x:x + V] = m


def grid_stack(m):
    """the map list of one sample, float64: [maximum over its words, then each word's map]"""
    m = np.asarray(m, dtype=np.float64)
    return np.concatenate([m.max(0, keepdims=True), m], 0)


def grid(imgs, maps, a, T, band_rgb, lr_imgs=None, expanded=None):
    """the grid builder: imgs [B][3][S][S], maps = one [T_i][a][a] array per sample, T = the word columns, band_rgb =
    T (r, g, b) triples.  expanded: per sample, expand() of every map of grid_stack(maps[i]), for a caller that has
    computed them already (a benchmark that spreads them over threads); None: they are computed here, one by one."""
    imgs = np.asarray(imgs, dtype=np.float64)
    lr = imgs if lr_imgs is None else np.asarray(lr_imgs, dtype=np.float64)
    rows = min(8, imgs.shape[0])
    V = 16 * a if a == 17 else imgs.shape[2]
    up = V // a
    Hs, cw = BAND + 2 * V, V + PAD
    out = Canvas(rows * Hs, (T + 2) * cw)
    for i in range(rows):
        y0 = i * Hs
        for j in range(T):
            out.canvas[y0:y0 + BAND, (j + 2) * cw:(j + 3) * cw] = band_rgb[j]
        stack = grid_stack(maps[i])
        e = np.stack([expand(s, up) for s in stack] if expanded is None else expanded[i])
        gmin, gmax = min(1.0, e.min()), max(0.0, e.max())
        if gmax > gmin:
            vals = np.clip(255.0 * (e - gmin) / (gmax - gmin), 0.0, 255.0)
            delta = 255.0 * expand_tol(a, up, np.abs(stack).max()) / (gmax - gmin)
        else:
            vals, delta = np.zeros_like(e), 0.0
        lo_vals, hi_vals = image_values(lr[i], V), image_values(imgs[i], V)
        out.put_image(y0 + BAND, 0, lo_vals)
        out.put_image(y0 + BAND + V, 0, hi_vals)
        for k in range(len(stack)):
            out.put_map(y0 + BAND, (1 + k) * cw, vals[k], delta)
            out.put_blend(y0 + BAND + V, (1 + k) * cw, vals[k], delta, hi_vals, 210)
    return out


def topk(img, maps, a, T):
    """the top-5 builder for one sample: img [3][S][S], maps [>= T][a][a] (f32 values); returns (Canvas, order, conf)"""
    V, up, cw = 256, 256 // a, 256 + PAD
    x = np.asarray(maps, dtype=np.float64)[:T]
    thresh = np.float64(np.float32(2.0 / T))
    conf = np.array([s[s > 2 * thresh].sum() for s in x])
    order = np.argsort(conf, kind='stable')[::-1][:5]
    out = Canvas(BAND + V, len(order) * cw)
    img_vals = image_values(img, V)
    for c, j in enumerate(order):
        cut = x[j] * (x[j] > thresh)
        e = expand(cut, up)
        den = e.max() - e.min() + 0.01
        vals = np.clip(255.0 * (e - e.min()) / den, 0.0, 255.0)
        delta = 255.0 * expand_tol(a, up, np.abs(cut).max()) / (e.max() - e.min()) if e.max() > e.min() else 0.0
        out.put_blend(BAND, c * cw, vals, delta, img_vals, 180)
    return out, order, conf


def label_cell(j, word, width, colour=(0, 0, 0)):
    """the caption cell [BAND][width][3] of word j: '%d:%s' % (j, word[:6]) (non-ASCII characters dropped) in white with
    PIL's default font at the cell's top-left corner, on `colour`"""
    from PIL import ImageDraw, ImageFont
    cell = Image.new('RGB', (width, BAND), tuple(int(c) for c in colour))
    text = '%d:%s' % (j, word.encode('ascii', 'ignore').decode('ascii')[:6])
    ImageDraw.Draw(cell).text((0, 0), text, font=ImageFont.load_default(), fill=(255, 255, 255))
    return np.asarray(cell)


def check_canvas(got, ref, text_rows=()):
    """Every byte of `got` equals the reference's, except where the float64 value lies within delta of an integer: there
    the neighbouring byte (and, in a blend, the blend OF the neighbouring byte) is allowed.  Returns the number of pixels
    that used the allowance.  text_rows: row ranges (the caption bands) to leave out when text was drawn."""
    assert got.shape == ref.canvas.shape and got.dtype == np.uint8, (got.shape, ref.canvas.shape)
    keep = np.ones(got.shape[:2], dtype=bool)
    for y0, y1 in text_rows:
        keep[y0:y1] = False
    bad = (got != ref.canvas).any(2) & keep
    used = 0
    for y, x in zip(*np.nonzero(bad)):
        k = ref.kind[y, x]
        assert k != 0, 'pad / band / black pixel (%d, %d): %s != %s' % (y, x, got[y, x], ref.canvas[y, x])

        def alternatives(v, delta):
            v = min(max(v, 0.0), 255.0)
            alts = {int(v)}
            if v - np.floor(v) <= delta and v >= 1:
                alts.add(int(v) - 1)
            if np.ceil(v) - v <= delta and int(v) < 255 and np.ceil(v) > v:
                alts.add(int(v) + 1)
            return alts
        if k == 1:
            for ch in range(3):
                assert int(got[y, x, ch]) in alternatives(ref.img_value[y, x, ch], IMAGE_DELTA), (y, x, ch)
        elif k == 2:
            assert len(set(got[y, x].tolist())) == 1 and \
                int(got[y, x, 0]) in alternatives(ref.map_value[y, x], ref.map_delta[y, x]), \
                (y, x, got[y, x], ref.map_value[y, x], ref.map_delta[y, x])
        else:
            m = int(ref.mask[y, x])
            for ch in range(3):
                allowed = set()
                for mv in alternatives(ref.map_value[y, x], ref.map_delta[y, x]):
                    for iv in alternatives(ref.img_value[y, x, ch], IMAGE_DELTA):
                        t = mv * m + iv * (255 - m) + 128
                        allowed.add(((t >> 8) + t) >> 8)
                assert int(got[y, x, ch]) in allowed, (y, x, ch, got[y, x], ref.map_value[y, x], ref.map_delta[y, x])
        used += 1
    return used
