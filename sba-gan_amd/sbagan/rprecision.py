"""R-precision of generated images (the retrieval measure of the AttnGAN paper), on the project's own DAMSM encoders.

For each generated image the candidate set is its own caption's sentence embedding plus M = R - 1 sentence embeddings of
captions drawn at random, without repetition, from images of a DIFFERENT class of the same split.  A candidate's score
is the clamped cosine of sent_loss, dot / max(|a| |c|, eps) in f32, between the image's global code (CNN_ENCODER's
cnn_code) and the candidate; rank = #{ mismatched m : NOT (s_m < s_0) }, so a tie counts against the image and so does
a NaN on either side; R@k is the share of images with rank < k.

The sentence embeddings of EVERY caption of the split are encoded once (`encode_pool`); per batch only indices are drawn
and the HIP kernel behind ops.rprec_rank gathers the candidate rows, scores, compares and counts in one launch.  The
indices come from a numpy Generator of the evaluator's own and the pool is encoded with numpy's global state saved and
restored: evaluating consumes none of the randomness the data path and the generator's noise draw from.
"""
import numpy as np
import torch

from . import ops

EPS = 1e-8


def draw_mismatched(rng, image_class, pool_class, M):
    """int32 [B][M]: per image, M distinct rows of the pool whose class differs from the image's, drawn from the
    numpy.random.Generator `rng` (never from numpy's global generator).  ValueError when an image has fewer than M
    eligible rows."""
    image_class = np.asarray(image_class).reshape(-1)
    pool_class = np.asarray(pool_class).reshape(-1)
    B = image_class.shape[0]
    if M < 0:
        raise ValueError('draw_mismatched: M must be >= 0 (got %d)' % M)
    out = np.empty((B, M), dtype=np.int32)
    if M == 0:
        return out
    eligible = {}
    for b in range(B):
        c = image_class[b].item()
        rows = eligible.get(c)
        if rows is None:
            rows = eligible[c] = np.flatnonzero(pool_class != c)
        if rows.shape[0] < M:
            raise ValueError('draw_mismatched: image %d (class %s) has %d mismatched pool rows, needs %d'
                             % (b, c, rows.shape[0], M))
        out[b] = rows[rng.choice(rows.shape[0], size=M, replace=False)]
    return out


def encode_pool(dataset, encode, batch, seed=0, device=None):
    """(pool [P][nef] f32 on the device, pool_class [P] numpy): the sentence embedding and the class of every caption
    of the split, caption i = dataset.get_caption(i) of image i // embeddings_num, in that order.  `encode(captions,
    cap_lens)` -> (words_embs, sent_emb) is the trainer's text hook; chunks of `batch` captions are sorted by length,
    descending (what the packed bi-LSTM takes, as prepare_data does) and un-permuted afterwards.  get_caption draws the
    word subset of an over-long caption from numpy's global generator: it is seeded with `seed` for the pool and its
    state restored afterwards."""
    P = dataset.number_example * dataset.embeddings_num
    device = device or torch.device('cuda', torch.cuda.current_device())
    pool_class = np.repeat(np.asarray(dataset.class_id)[:dataset.number_example], dataset.embeddings_num)
    chunks = []
    state = np.random.get_state()
    try:
        np.random.seed(seed)
        for lo in range(0, P, batch):
            caps, lens = zip(*(dataset.get_caption(i) for i in range(lo, min(lo + batch, P))))
            lens = np.asarray(lens, dtype=np.int64)
            caps = np.stack(caps).reshape(len(lens), -1)
            order = np.argsort(-lens, kind='stable')
            _, sent = encode(torch.from_numpy(caps[order]).to(device), torch.from_numpy(lens[order]).to(device))
            inverse = np.empty_like(order)
            inverse[order] = np.arange(len(order))
            chunks.append(sent.detach().float().index_select(0, torch.from_numpy(inverse).to(device)))
    finally:
        np.random.set_state(state)
    return torch.cat(chunks, 0).contiguous(), pool_class


def summarize(ranks, R, seed, splits=10):
    """the result dict from the ranks of all images (any integer sequence)"""
    ranks = np.asarray(ranks).reshape(-1)
    n = int(ranks.shape[0])
    out = {'n': n, 'R': int(R), 'seed': int(seed)}
    for k in (1, 5, 10):
        out['r_at_%d' % k] = float((ranks < k).mean()) if n else float('nan')
    ns = splits if n >= splits else 1
    per = n // ns                                   # the remainder n % ns is left out of the split figures only
    hit = (ranks[:per * ns] < 1).reshape(ns, per).mean(1) if per else np.full(ns, np.nan)
    out['r_at_1_splits_mean'], out['r_at_1_splits_std'] = float(hit.mean()), float(np.std(hit))
    out['splits'] = int(ns)
    return out


class RPrecision(object):
    """Accumulates the ranks of generated images.  image_encoder(images) -> (region features, cnn_code): a CNN_ENCODER
    behind InceptionHIP (or any callable of that shape); pool / pool_class: encode_pool's; R candidates per image."""

    def __init__(self, image_encoder, pool, pool_class, R=100, seed=100):
        if R < 2:
            raise ValueError('RPrecision: R must be >= 2 (got %d)' % R)
        self.image_encoder = image_encoder
        self.pool, self.pool_class = pool.float().contiguous(), np.asarray(pool_class)
        if self.pool.shape[0] != self.pool_class.shape[0]:
            raise ValueError('RPrecision: %d pool rows, %d classes' % (self.pool.shape[0], self.pool_class.shape[0]))
        self.R, self.seed = int(R), int(seed)
        self.rng = np.random.default_rng(self.seed)
        self._ranks = []            # int32 device tensors, one per batch

    def update(self, images, true_sent_emb, class_ids):
        """one batch: no host-device sync (the indices are drawn, checked and uploaded from the host)"""
        with torch.no_grad():
            _, code = self.image_encoder(images)
        idx = draw_mismatched(self.rng, class_ids, self.pool_class, self.R - 1)
        rank = ops.rprec_rank(code.detach().float().contiguous(), true_sent_emb.detach().float().contiguous(), self.pool,
                              idx, eps=EPS)
        self._ranks.append(rank)
        return rank

    def ranks(self):
        """all ranks so far as a numpy array (one sync)"""
        if not self._ranks:
            return np.zeros(0, dtype=np.int32)
        return torch.cat(self._ranks).cpu().numpy()

    def result(self, splits=10):
        return summarize(self.ranks(), self.R, self.seed, splits)
