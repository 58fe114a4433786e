"""Image-caption retrieval over a whole split: the quality measure of a DAMSM encoder pair (--retrieval).

Every image i < ni of the split has a code x_i (CNN_ENCODER's cnn_code, f32 [nef]) and a class c_i; every caption t < nt a
code y_t (the text encoder's sent_emb) and an owner o_t in [0, ni), in the data sets here t // embeddings_num.  The score
is the float64 cosine of csrc/retrieval.hip,

    s(i, t) = x_i . y_t / max(sqrt(|x_i|^2 |y_t|^2), eps),

with the same bits whichever launch computed it and whichever side is the query.  Per query the rank is the number of
candidates that are not its own and are not strictly below its own:

    image to text   best_i = max over {t : o_t = i} of s(i, t)     rank_i = #{t : o_t != i, NOT (s(i, t) < best_i)}
    text to image   thr_t  = s(o_t, t)                             rank_t = #{i : i != o_t, NOT (s(i, t) < thr_t)}

A tie counts against the query, and so does a NaN on either side.  Own pairs are left out by key, never by value.  Two
protocols come out of one pass: 'instance' as above, and 'class_masked', where the candidates of the query's own class
that are not its own are left out as well -- the mask the DAMSM losses train with.  Four launches in all (own_best and
counts per direction, the two sets swapped, both keyed by image number); the ni x nt matrix is never written and all
counts come back in one copy.

encode_images prepares every image deterministically (centre crop, no flip); the captions come from
rprecision.encode_pool.  Nothing here draws from python's, numpy's or torch's global generators.
"""
import numpy as np
import torch
import torch.utils.data as data

import datasets

from . import ops
from .feature_rows import dtype_name
from .rprecision import encode_pool

EPS = 1e-8
CAPTION_CHUNK = 512
DIRECTIONS = ('i2t', 't2i')
PROTOCOLS = ('instance', 'class_masked')
RANKS = tuple('%s_%s' % (d, p) for d in DIRECTIONS for p in PROTOCOLS)
FIGURES = ('r_at_1', 'r_at_5', 'r_at_10', 'median_rank', 'mean_rank')


def summarize(ranks):
    """the figures of one rank vector (host arithmetic only): the share of queries with rank < 1, 5, 10, and the median
    and the mean of rank + 1"""
    ranks = np.asarray(ranks).reshape(-1)
    if ranks.size < 1:
        raise ValueError('summarize: no ranks')
    out = {'r_at_%d' % k: float(np.count_nonzero(ranks < k)) / ranks.size for k in (1, 5, 10)}
    out['median_rank'] = float(np.median(ranks.astype(np.float64) + 1.0))
    out['mean_rank'] = float(ranks.astype(np.float64).mean() + 1.0)
    return out


def center_offsets(hw, crop):
    """int64 [n] x1, y1 of the `crop` px window in the middle of images of the sizes hw [n][2] = {H, W}"""
    hw = np.asarray(hw, dtype=np.int64).reshape(-1, 2)
    if (hw < crop).any():
        raise ValueError('retrieval: a %d px crop does not fit the smallest image side (%d)' % (crop, int(hw.min())))
    return (hw[:, 1] - crop) // 2, (hw[:, 0] - crop) // 2


class _CenterCrops(data.Dataset):
    """image i of `dataset`, deterministic: load_image, the middle `crop` px window, no flip, the data set's
    normalisation"""

    def __init__(self, dataset, crop, resize):
        self.dataset, self.crop, self.resize = dataset, int(crop), resize

    def __len__(self):
        return len(self.dataset)

    def window(self, index):
        """the PIL image before the normalisation"""
        img = datasets.load_image(self.dataset.image_path(index), self.dataset.image_box(index), self.resize)
        W, H = img.size
        x1, y1 = center_offsets([(H, W)], self.crop)
        x1, y1 = int(x1[0]), int(y1[0])
        return img.crop((x1, y1, x1 + self.crop, y1 + self.crop))

    def __getitem__(self, index):
        return self.dataset.norm(self.window(index))


def center_loader(dataset, batch, crop, resize, workers=0):
    """the images of `dataset` in order as _CenterCrops prepares them, in batches of `batch` (the last may be short).  The
    loader takes a torch.Generator of its own, so torch's global generator is not consumed (sbagan/nearest.py reads the
    training split through it too)"""
    return data.DataLoader(_CenterCrops(dataset, crop, resize), batch_size=int(batch), shuffle=False, drop_last=False,
                           num_workers=int(workers), generator=torch.Generator())


def encode_images(dataset, image_encoder, batch, crop, resize, cache=None, workers=0):
    """[ni][nef] f32 on the device: cnn_code of every image of the split, in order.  Each image is
    datasets.load_image(path, box, resize), its `crop` px window at ((W - crop) // 2, (H - crop) // 2), not flipped,
    normalised as the data set does; the last batch may be short.  cache: a device_data.DeviceImageCache of the split
    (made with the same `resize`); the batches then come from it through DeviceBatchLoader.center_batch, bit-identical
    to the host path.  The encoder runs in eval mode without gradients, on the HIP trunk (a fresh
    sbagan.inception_hip.InceptionHIP: its folded operands are made from the weights and BatchNorm statistics as they are
    NOW, whatever a training step's own trunk still holds), and goes back to the mode it was in; the host loader takes a
    torch.Generator of its own, so torch's global generator is not consumed."""
    n, batch, crop = len(dataset), int(batch), int(crop)
    if n < 1 or batch < 1:
        raise ValueError('encode_images: needs at least one image and a batch of at least 1 (got %d, %d)' % (n, batch))
    from .inception_hip import InceptionHIP
    device = next(image_encoder.parameters()).device
    if cache is not None and cache.device != device:
        raise ValueError('encode_images: the cache is on %s, the encoder on %s' % (cache.device, device))
    if cache is not None:
        from .device_data import DeviceBatchLoader
        loader = DeviceBatchLoader(dataset, cache, batch, crop, 1, 0, shuffle=False, drop_last=False)
        batches = (loader.center_batch(range(lo, min(lo + batch, n))) for lo in range(0, n, batch))
    else:
        batches = center_loader(dataset, batch, crop, resize, workers)
    mode = image_encoder.training
    image_encoder.eval()
    codes = []
    try:
        runner = InceptionHIP(image_encoder)
        with torch.no_grad():
            for imgs in batches:
                _, code = runner(imgs.to(device))
                codes.append(code.detach().float())
    finally:
        image_encoder.train(mode)
    return torch.cat(codes, 0).contiguous()


def text_hook(text_encoder):
    """encode(captions, cap_lens) -> (words_embs, sent_emb) for the bi-LSTM (text_encoder(captions, cap_lens, hidden)) or
    the BERT text side (text_encoder(captions)), without gradients.  The HIP bi-LSTM is given the LIVE weights: the
    module keeps a packed copy keyed on torch's version counters, which the fused Adam (it writes through raw pointers)
    does not move, so during training that copy can be older than the weights; it is neither used nor touched here."""
    def encode(captions, cap_lens):
        with torch.no_grad():
            if not hasattr(text_encoder, 'init_hidden'):
                return text_encoder(captions)
            hidden = text_encoder.init_hidden(captions.size(0))
            if not (hasattr(text_encoder, '_hip_ok') and text_encoder._hip_ok(captions)):
                return text_encoder(captions, cap_lens, hidden)
            r = text_encoder.rnn
            w_ih, w_hh, b_ih, b_hh = (torch.stack((a.detach().float(), b.detach().float())).contiguous() for a, b in (
                (r.weight_ih_l0, r.weight_ih_l0_reverse), (r.weight_hh_l0, r.weight_hh_l0_reverse),
                (r.bias_ih_l0, r.bias_ih_l0_reverse), (r.bias_hh_l0, r.bias_hh_l0_reverse)))
            return ops.lstm_bidir_forward(captions, cap_lens, text_encoder.encoder.weight.detach().float(), w_ih, w_hh,
                                          b_ih, b_hh, hidden)
    return encode


def encode_captions(dataset, text_encoder, device=None, chunk=CAPTION_CHUNK):
    """[nt][nef] f32 on the device: sent_emb of every caption of the split, caption t of image t // embeddings_num
    (rprecision.encode_pool, which restores numpy's global state).  The encoder runs in eval mode and goes back to the
    mode it was in."""
    mode = text_encoder.training
    text_encoder.eval()
    try:
        codes, _ = encode_pool(dataset, text_hook(text_encoder), chunk, device=device)
    finally:
        text_encoder.train(mode)
    return codes


class Retrieval(object):
    """The ranks and figures of one encoder pair.  image_codes [ni][nef], caption_codes [nt][nef]: f32 on the device;
    owner [nt]: the image of every caption; image_class [ni]: integer class per image (host sequences).  Refused
    before any launch: mismatched widths or counts, an owner outside [0, ni), an image without a caption."""

    def __init__(self, image_codes, caption_codes, owner, image_class, eps=EPS, dtype=None):
        for what, t in (('image_codes', image_codes), ('caption_codes', caption_codes)):
            if not torch.is_tensor(t) or t.dim() != 2 or t.dtype != torch.float32:
                raise ValueError('Retrieval: %s must be a 2-D float32 tensor' % what)
        ni, nt = int(image_codes.shape[0]), int(caption_codes.shape[0])
        if image_codes.shape[1] != caption_codes.shape[1]:
            raise ValueError('Retrieval: image codes are %d wide, caption codes %d'
                             % (image_codes.shape[1], caption_codes.shape[1]))
        owner = np.asarray(owner).reshape(-1)
        image_class = np.asarray(image_class).reshape(-1)
        if owner.shape[0] != nt or image_class.shape[0] != ni or ni < 1 or nt < 1:
            raise ValueError('Retrieval: %d images with %d classes, %d captions with %d owners'
                             % (ni, image_class.shape[0], nt, owner.shape[0]))
        if not (np.issubdtype(owner.dtype, np.integer) and np.issubdtype(image_class.dtype, np.integer)):
            raise ValueError('Retrieval: owners and classes must be integers')
        if (owner < 0).any() or (owner >= ni).any():
            raise ValueError('Retrieval: a caption\'s owner is outside [0, %d)' % ni)
        held = np.bincount(owner, minlength=ni)
        if (held == 0).any():
            raise ValueError('Retrieval: image %d has no caption' % int(np.flatnonzero(held == 0)[0]))
        if np.abs(image_class.astype(np.int64)).max() >= 2 ** 31:
            raise ValueError('Retrieval: a class id does not fit int32')
        eps = float(eps)
        if not eps > 0.0:
            raise ValueError('Retrieval: eps must be positive (got %r)' % eps)
        self.image_codes, self.caption_codes = image_codes, caption_codes
        self.owner, self.image_class = owner.astype(np.int32), image_class.astype(np.int32)
        self.ni, self.nt, self.eps, self.dtype = ni, nt, eps, dtype_name(dtype)
        self.captions_per_image = float(nt) / ni
        self._ranks = None

    def ranks(self, splits=0):
        """{'i2t_instance', 'i2t_class_masked' [ni], 't2i_instance', 't2i_class_masked' [nt]}: int32 numpy vectors"""
        if self._ranks is None:
            dev = self.image_codes.device
            ni, nt = self.ni, self.nt
            # one upload: image keys | caption owners | image classes | caption classes
            ints = np.concatenate([np.arange(ni, dtype=np.int32), self.owner, self.image_class,
                                   self.image_class[self.owner]])
            ints = torch.from_numpy(ints).to(dev)
            key_i, key_t = ints[:ni], ints[ni:ni + nt]
            cls_i, cls_t = ints[ni + nt:2 * ni + nt], ints[2 * ni + nt:]
            x, y = self.image_codes, self.caption_codes
            best = ops.retrieval_own_best(x, y, key_i, key_t, self.eps, splits)
            i_all, i_mask = ops.retrieval_counts(x, y, key_i, key_t, best, cls_i, cls_t, self.eps, splits)
            thr = ops.retrieval_own_best(y, x, key_t, key_i, self.eps, splits)
            t_all, t_mask = ops.retrieval_counts(y, x, key_t, key_i, thr, cls_t, cls_i, self.eps, splits)
            counts = torch.cat([i_all, i_mask, t_all, t_mask]).cpu().numpy()        # the one read-back
            cuts = np.cumsum([0, ni, ni, nt, nt])
            self._ranks = {name: counts[cuts[k]:cuts[k + 1]] for k, name in enumerate(RANKS)}
        return self._ranks

    def result(self):
        out = {name: summarize(r) for name, r in self.ranks().items()}
        out.update(n_images=self.ni, n_captions=self.nt, captions_per_image=self.captions_per_image, eps=self.eps,
                   dtype=self.dtype)
        return out


def evaluate_split(dataset, image_encoder, text_encoder, batch, crop, resize, cache=None, workers=0, dtype=None):
    """the Retrieval of a whole split: every caption of every image"""
    x = encode_images(dataset, image_encoder, batch, crop, resize, cache=cache, workers=workers)
    y = encode_captions(dataset, text_encoder, device=x.device)
    owner = np.arange(y.shape[0], dtype=np.int64) // dataset.embeddings_num
    return Retrieval(x, y, owner, np.asarray(dataset.class_id)[:len(dataset)], dtype=dtype)


def format_line(epoch, result):
    """'| end epoch N | retrieval i2t R@1 R@5 R@10 med | t2i ... | class-masked ... |'"""
    def part(r):
        return '{:5.3f} {:5.3f} {:5.3f} {:g}'.format(r['r_at_1'], r['r_at_5'], r['r_at_10'], r['median_rank'])
    return ('| end epoch {:3d} | retrieval i2t {} | t2i {} | class-masked i2t {} | t2i {} |'
            .format(epoch, part(result['i2t_instance']), part(result['t2i_instance']),
                    part(result['i2t_class_masked']), part(result['t2i_class_masked'])))
