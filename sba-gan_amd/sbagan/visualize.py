"""Attention-map overlay images (the reference's G_*.png / D_*.png / attention_maps*.png grids and the *_a<k>.png
top-5 strips), written from their contract, built on the device.

Every map is resized to the tile size and blurred with a Gaussian of sigma 20 (161 taps per axis).  Both steps are
linear and separable, so one V x a matrix M = G W (expand_operator, float64 on the host, cached) turns a map x into
M x M^T; ops.vis_expand does that for every map of a dump in one launch, ops.vis_compose writes the finished uint8
canvas (image tiles, normalised maps, blends, pads, colour bands) in one more, and one copy brings it to the host, where
PIL draws the caption words.  The per-map min / max / conf (3 n floats) come back once in between: the normalisation is
per sample and the top-5 order is a host-side sort.
"""
import colorsys
import functools

import numpy as np
import torch
from PIL import Image, ImageDraw, ImageFont

from miscc.config import cfg
from . import ops

SIGMA, RADIUS = 20.0, 80          # the blur: truncate = 4 sigma
BAND = 50                         # rows of the caption band
PAD = 2                           # black columns behind every tile
GRID_MASK, TOPK_MASK = 210, 180   # constant paste masks of the two builders
TOPK = 5


def resize_operator(a, up):
    """[a up][a] float64: bilinear resize with half-pixel centres, edges clamped"""
    V = a * up
    W = np.zeros((V, a))
    src = (np.arange(V) + 0.5) / up - 0.5
    i0 = np.floor(src).astype(np.int64)
    f = src - i0
    rows = np.arange(V)
    np.add.at(W, (rows, np.clip(i0, 0, a - 1)), 1.0 - f)
    np.add.at(W, (rows, np.clip(i0 + 1, 0, a - 1)), f)
    return W


def blur_operator(V):
    """[V][V] float64: Gaussian of sigma 20, radius 80, weights normalised to sum 1, symmetric-reflect boundary
    (d c b a | a b c d | d c b a), reflected as often as the radius needs"""
    k = np.arange(-RADIUS, RADIUS + 1)
    w = np.exp(-0.5 * (k / SIGMA) ** 2)
    w /= w.sum()
    G = np.zeros((V, V))
    o = np.arange(V)
    for kk, wk in zip(k, w):
        r = (o + kk) % (2 * V)
        r = np.where(r >= V, 2 * V - 1 - r, r)
        np.add.at(G, (o, r), wk)
    return G


@functools.lru_cache(maxsize=None)
def _expand_operator(a, up):
    M = blur_operator(a * up) @ resize_operator(a, up)
    M.setflags(write=False)
    return M


def expand_operator(a, up):
    """M [a up][a] float64 with expanded = M x M^T: resize by `up`, then the blur; the identity for up <= 1.  Cached per
    (a, up); the array is read-only."""
    a, up = int(a), int(up)
    if a < 1:
        raise ValueError('expand_operator: a must be positive (got %d)' % a)
    return _expand_operator(a, up) if up > 1 else _identity(a)


@functools.lru_cache(maxsize=None)
def _identity(a):
    M = np.eye(a)
    M.setflags(write=False)
    return M


_DEVICE_M = {}


def _device_operator(a, V, device):
    """M as the f32 device tensor ops.vis_expand takes (None: V // a <= 1, the map is left as it is)"""
    up = V // a
    if up <= 1:
        if V != a:
            raise ValueError('a %d x %d map cannot fill a %d px tile' % (a, a, V))
        return None
    if a * up != V:
        raise ValueError('the tile size %d is not a multiple of the map size %d' % (V, a))
    key = (a, up, str(device))
    M = _DEVICE_M.get(key)
    if M is None:
        M = _DEVICE_M[key] = torch.from_numpy(expand_operator(a, up).astype(np.float32)).to(device)
    return M


def word_colours(n=20):
    """n distinguishable RGB byte triples: an HSV wheel, alternating two brightness levels"""
    out = []
    for i in range(n):
        r, g, b = colorsys.hsv_to_rgb(i / float(n), 0.85, 1.0 if i % 2 == 0 else 0.6)
        out.append((int(r * 255), int(g * 255), int(b * 255)))
    return out


def _pack_rgb(c):
    return c[0] | (c[1] << 8) | (c[2] << 16)


def _word(ixtoword, token):
    return ixtoword[int(token)].encode('ascii', 'ignore').decode('ascii')


def _sentence(caption, ixtoword):
    """the caption's words up to its first 0 token"""
    words = []
    for token in caption:
        if int(token) == 0:
            break
        words.append(_word(ixtoword, token))
    return words


def _label(j, word):
    return '%d:%s' % (j, word[:6])


def topk_order(conf, k=TOPK):
    """the k maps of highest conf, ties to the higher index first: a stable ascending argsort, reversed"""
    return np.argsort(np.asarray(conf), kind='stable')[::-1][:k]


def _images(t):
    t = t.detach()
    if t.dim() == 3:
        t = t.unsqueeze(0)
    return t.float().contiguous()


def _sample_maps(maps, i):
    m = maps[i].detach()
    return m.reshape(-1, m.shape[-2], m.shape[-1]).float()


def build_super_images(imgs, captions, ixtoword, maps, a, lr_imgs=None):
    """The grid of G_*.png / D_*.png / attention_maps*.png for the first min(8, B) samples.  imgs [B][3][S][S] (device, in
    [-1, 1]); captions [B][L] token ids; maps: a [B][T][a][a] tensor or one [T_i][a][a] tensor per sample (device);
    lr_imgs: the previous stage's images, shown in the first row (imgs when None).  Per sample a caption band over two
    rows of tiles: image | max over the words | each word's map, and below them image | their blends over the image.
    Returns (uint8 [rows (50 + 2 V)][(WORDS_NUM + 2)(V + 2)][3], the samples' word lists)."""
    imgs = _images(imgs)
    lr = imgs if lr_imgs is None else _images(lr_imgs)
    a = int(a)
    rows = min(8, imgs.shape[0])
    V = 16 * a if a == 17 else imgs.shape[2]
    T = int(cfg.TEXT.WORDS_NUM)
    if T > 20:
        raise ValueError('build_super_images: cfg.TEXT.WORDS_NUM = %d, at most 20 word columns are drawn' % T)
    M = _device_operator(a, V, imgs.device)
    stacks, first = [], [0]
    for i in range(rows):
        m = _sample_maps(maps, i)
        if m.shape[0] < 1 or m.shape[0] > T or tuple(m.shape[1:]) != (a, a):
            raise ValueError('build_super_images: sample %d has maps %s, expected [1..%d][%d][%d]'
                             % (i, tuple(m.shape), T, a, a))
        stacks += [m.amax(0, keepdim=True), m]
        first.append(first[-1] + m.shape[0] + 1)
    expanded, stats = ops.vis_expand(torch.cat(stacks, 0).contiguous(), M)
    stats = stats.cpu().numpy().astype(np.float64)
    nc = T + 2
    desc = np.zeros((rows, 2, nc, 4), dtype=np.int32)
    par = np.zeros((rows, 2, nc, 2), dtype=np.float32)
    colours = [_pack_rgb(c) for c in word_colours(20)]
    band = np.zeros((rows, nc), dtype=np.uint32)
    band[:, 2:] = colours[:T]
    for i in range(rows):
        lo, hi = first[i], first[i + 1]
        gmin, gmax = min(1.0, stats[0, lo:hi].min()), max(0.0, stats[1, lo:hi].max())
        desc[i, 0, 0] = (ops.VIS_IMAGE, i, 0, 0)
        desc[i, 1, 0] = (ops.VIS_IMAGE, (1 << 16) | i, 0, 0)
        for k in range(hi - lo):
            desc[i, 0, 1 + k] = (ops.VIS_MAP, 0, lo + k, 0)
            desc[i, 1, 1 + k] = (ops.VIS_BLEND, (1 << 16) | i, lo + k, GRID_MASK)
            par[i, :, 1 + k] = (gmin, gmax - gmin)
    canvas = ops.vis_compose(V, BAND, desc, par, band, expanded, lr[:rows].contiguous(), imgs[:rows].contiguous())
    canvas = canvas.cpu().numpy()
    caps = captions.detach().cpu().numpy() if torch.is_tensor(captions) else np.asarray(captions)
    sentences = [_sentence(caps[i], ixtoword) for i in range(rows)]
    picture = Image.fromarray(canvas)
    draw, font = ImageDraw.Draw(picture), ImageFont.load_default()
    for i, words in enumerate(sentences):
        for j, word in enumerate(words):
            draw.text(((j + 2) * (V + PAD), i * (BAND + 2 * V)), _label(j, word), font=font, fill=(255, 255, 255))
    return np.asarray(picture).copy(), sentences


def build_super_images2(img, caption, cap_len, ixtoword, maps, a):
    """The top-5 strip of *_a<k>.png for ONE sample at 256 px: of the caption's cap_len words, the five whose maps hold
    the most mass above 2 thresh (thresh = 2 / cap_len), each map cut at thresh, expanded, normalised by its own range and
    blended over the image, under the word's label.  img [3][S][S], maps [>= cap_len][a][a] (device).
    Returns (uint8 [306][min(5, cap_len) 258][3], the caption's word list)."""
    img = _images(img)[:1].contiguous()
    a, T, V = int(a), int(cap_len), 256
    if T < 1:
        raise ValueError('build_super_images2: the caption is empty')
    m = maps.detach()
    m = m.reshape(-1, m.shape[-2], m.shape[-1]).float()
    if m.shape[0] < T or tuple(m.shape[1:]) != (a, a):
        raise ValueError('build_super_images2: maps %s, expected [>= %d][%d][%d]' % (tuple(m.shape), T, a, a))
    x = m[:T].contiguous()
    thresh = torch.full((T,), 2.0 / T, dtype=torch.float32, device=x.device)
    expanded, stats = ops.vis_expand(x, _device_operator(a, V, x.device), thresh)
    stats = stats.cpu().numpy().astype(np.float64)
    order = topk_order(stats[2])
    nc = len(order)
    desc = np.zeros((1, 1, nc, 4), dtype=np.int32)
    par = np.zeros((1, 1, nc, 2), dtype=np.float32)
    for c, j in enumerate(order):
        desc[0, 0, c] = (ops.VIS_BLEND, 0, int(j), TOPK_MASK)
        par[0, 0, c] = (stats[0, j], stats[1, j] - stats[0, j] + 0.01)
    canvas = ops.vis_compose(V, BAND, desc, par, np.zeros((1, nc), dtype=np.uint32), expanded, img).cpu().numpy()
    cap = caption.detach().cpu().numpy() if torch.is_tensor(caption) else np.asarray(caption)
    words = _sentence(cap.reshape(-1), ixtoword)
    font = ImageFont.load_default()
    for c, j in enumerate(order):                  # every label is clipped to its own cell
        if j < len(words):
            cell = Image.new('RGB', (V + PAD, BAND), (0, 0, 0))
            ImageDraw.Draw(cell).text((0, 0), _label(int(j), words[j]), font=font, fill=(255, 255, 255))
            canvas[:BAND, c * (V + PAD):(c + 1) * (V + PAD)] = np.asarray(cell)
    return canvas, words


def damsm_attention_maps(region_features, words_emb, cap_lens, gamma1):
    """The DAMSM word-to-region maps of each sample against ITS OWN image: a list of [T_i][17][17] f32 tensors.
    region_features [B][nef][17][17], words_emb [B][nef][L], cap_lens [B]."""
    from .nets import func_attention
    lens = [int(v) for v in (cap_lens.tolist() if torch.is_tensor(cap_lens) else cap_lens)]
    out = []
    with torch.no_grad():
        for i, T in enumerate(lens[:region_features.shape[0]]):
            T = min(T, words_emb.shape[2])
            word = words_emb[i:i + 1, :, :T].float().contiguous()
            _, attn = func_attention(word, region_features[i:i + 1].float().contiguous(), gamma1)
            out.append(attn[0].contiguous())
    return out
