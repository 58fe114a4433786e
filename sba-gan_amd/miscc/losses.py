"""Losses of the adversarial step with the reference's names and positional signatures
(AttnGAN2/code/miscc/losses.py:11-214), computed by fused HIP kernels.

Differences from the reference, none of which change a result:
  * no host synchronisation: cap_lens is read on the device (the reference calls
    .tolist(), losses.py:71), and the per-term log strings (losses.py:184,205, five
    .item() syncs) are replaced by a dict of device scalars;
  * words_loss evaluates all B x B (caption, image) pairs in one launch instead of a Python
    loop over captions, and does not return the per-caption attention maps: the third return
    value is an empty list (the PNG visualiser, their only reader, computes the maps of its
    <= 8 samples itself: sbagan.visualize.damsm_attention_maps);
  * the same-class mask is built on the host with numpy exactly like the reference
    (losses.py:24-32,73-76) -- it is integer work on `class_ids`, a host array.  The recorded training loop
    (--replay) cannot have a per-batch tensor built on the host: there `class_ids` is an ops.ClassMask, the same mask
    made on the device by sba_batch_masks, and is used as it is.
"""
import numpy as np

import torch

from miscc.config import cfg
from sbagan import ops


def cosine_similarity(x1, x2, dim=1, eps=1e-8):
    """losses.py:11-17 (API parity; the training path uses the fused kernels)."""
    w12 = torch.sum(x1 * x2, dim)
    w1 = torch.norm(x1, 2, dim)
    w2 = torch.norm(x2, 2, dim)
    return (w12 / (w1 * w2).clamp(min=eps)).squeeze()


class LossLogs(dict):
    """generator_loss's second return value.  The reference builds a string with five .item() host syncs inside the
    step (losses.py:184,205: 'g_loss0: 1.23 ... w_loss: 4.56 s_loss: 7.89 '); here the values stay device scalars in
    a dict, and the reference's string is produced on demand: str(logs), '%s' % logs, logs + '\n' all give the
    reference's text (and synchronise only then)."""

    def __str__(self):
        out = ''
        i = 0
        while 'g_loss%d' % i in self:
            out += 'g_loss%d: %.2f ' % (i, float(self['g_loss%d' % i]))
            i += 1
        if 'w_loss' in self and 's_loss' in self:
            out += 'w_loss: %.2f s_loss: %.2f ' % (float(self['w_loss']), float(self['s_loss']))
        return out

    def __add__(self, other):
        return str(self) + other

    def __radd__(self, other):
        return other + str(self)


_MASK_CACHE = {}
DIRECT_DAMSM = True     # damsm_image_terms: loss heads + gradients without autograd


def class_mask(class_ids, batch_size, device):
    """masks[i][j] = (class_ids[j] == class_ids[i]) and j != i  (losses.py:24-32).  Bit-exact
    integer work on the host; cached per (ids, device) so a training loop with fixed ids
    uploads it once.  A mask already on the device (ops.ClassMask, made by ops.batch_masks from device-side ids: the
    recorded training step, sbagan/static_batch.py) is returned as it is: no numpy, no cache, no upload."""
    if class_ids is None:
        return None
    if isinstance(class_ids, ops.ClassMask):
        m = class_ids.tensor
        if m.size(0) != batch_size or m.device != torch.device(device):
            raise ValueError('class_mask: the prepared mask is %s on %s, the batch needs [%d][%d] on %s'
                             % (tuple(m.shape), m.device, batch_size, batch_size, device))
        return m
    ids = np.asarray(class_ids).reshape(-1)[:batch_size]
    key = (ids.tobytes(), str(ids.dtype), batch_size, str(device))
    m = _MASK_CACHE.get(key)
    if m is None:
        masks = []
        for i in range(batch_size):
            mask = (ids == ids[i]).astype(np.uint8)
            mask[i] = 0
            masks.append(mask.reshape((1, -1)))
        m = torch.from_numpy(np.concatenate(masks, 0)).to(device)
        if len(_MASK_CACHE) > 64:
            _MASK_CACHE.clear()
        _MASK_CACHE[key] = m
    return m


def sent_loss(cnn_code, rnn_code, labels, class_ids, batch_size, eps=1e-8):
    """losses.py:20-59.  labels must be arange(batch_size) (the only value the reference
    ever passes, trainer.py:150) or None."""
    if labels is None:
        return None, None
    mask = class_mask(class_ids, batch_size, cnn_code.device)
    return ops.SentLossFn.apply(cnn_code, rnn_code, mask, float(cfg.TRAIN.SMOOTH.GAMMA3), float(eps))


def words_loss(img_features, words_emb, labels, cap_lens, class_ids, batch_size):
    """losses.py:62-132."""
    if labels is None:
        return None, None, []
    mask = class_mask(class_ids, batch_size, img_features.device)
    s = cfg.TRAIN.SMOOTH
    l0, l1 = ops.WordsLossFn.apply(img_features, words_emb, cap_lens, mask,
                                   (float(s.GAMMA1), float(s.GAMMA2), float(s.GAMMA3)))
    return l0, l1, []


def d_term_heads(n, uncond):
    """The heads of errD (losses.py:141-158) over feats = [n real | n fake] rows, as ops.Head records in the reference's
    call order: cond_real, cond_fake, cond_wrong (real rows 0..n-2 with conditions 1..n-1), then real and fake logits.
    errD = (real + cond_real)/2 + (fake + cond_fake + cond_wrong)/3; without the unconditional head
    cond_real + (cond_fake + cond_wrong)/2."""
    H = ops.Head
    if uncond:
        return (H(0, n, 0, 1., .5, 1), H(n, n, 0, 0., 1. / 3, 3), H(0, n - 1, 1, 0., 1. / 3, 4),
                H(0, n, None, 1., .5, 0), H(n, n, None, 0., 1. / 3, 2))
    return (H(0, n, 0, 1., 1., 0), H(n, n, 0, 0., .5, 1), H(0, n - 1, 1, 0., .5, 2))


def g_term_heads(n, uncond):
    """The heads of one discriminator's term of errG (losses.py:168-186) over the n fake rows."""
    H = ops.Head
    if uncond:
        return (H(0, n, 0, 1., 1., 1), H(0, n, None, 1., 1., 0))
    return (H(0, n, 0, 1., 1., 0),)


def _augmented(real, fake, augment):
    """ops.diffaug for an `augment` argument (rows, flags), ops.diffaug_gated for (rows, flags, gates, p_dev): the
    adaptive and fixed-p modes of sbagan.diffaug.DiffAugment, whose probability the kernel reads from device memory"""
    if len(augment) == 2:
        return ops.diffaug(real, fake, augment[0], augment[1])
    rows, flags, gates, p_dev = augment
    return ops.diffaug_gated(real, fake, rows, gates, p_dev, flags)


def _seen(real, fake, augment, geo):
    """what a discriminator sees of [real | fake] (real None: the fake images alone).  geo (mats, one row per image):
    ops.geoaug writes the warped, joined batch; augment then runs over that batch as it is -- geometry first, then
    colour, translation and cutout, the order of Karras et al."""
    if geo is None:
        return _augmented(real, fake, augment)
    seen = ops.geoaug(real, fake, geo)
    return seen if augment is None else _augmented(None, seen, augment)


def discriminator_loss(netD, real_imgs, fake_imgs, conditions, real_labels, fake_labels, real_features=None,
                       augment=None, count_sink=None, geo=None):
    """losses.py:136-161: the real and the fake.detach() trunk pass, five heads,
    errD = (real + cond_real)/2 + (fake + cond_fake + cond_wrong)/3.

    The two passes run as one over [real | fake] with per-half BatchNorm batches: same results and module state as the
    reference's two calls, half the launches and weight reads.  The heads and the BCE sum are one autograd node over
    that feature map (ops.DHeadsFn).

    real_features (optional, beyond the reference's signature): netD(real_imgs) evaluated AHEAD of this call (the
    data-parallel step runs it beside the generator's gradient exchange: it does not depend on the generator); the
    fake half then runs as its own pass, in the reference's order (real first), with the same per-pass BatchNorm
    batches and running-statistic updates.

    augment (optional, (rows, flags): f32 uniforms [2n][8] -- n rows for the real images, then n for the fake ones -- and
    the policy bits of sbagan.diffaug): Differentiable Augmentation of both halves.  ops.diffaug writes the augmented
    [real | fake] batch in one pass, in place of the concatenation; not available with real_features.  With
    (rows, flags, gates [2n][4], p_dev [1]) the gated kernels run instead (_augmented).

    count_sink (optional): handed to ops.d_heads -- the signs of the real rows' probabilities are counted on the device
    (the overfitting read-out of --ada).

    geo (optional, f32 [2n][4]: one matrix per image, real rows first -- sbagan.geoaug.GeoAugment.d_mats): the geometric
    augmentation of both halves (ops.geoaug), which does the concatenation; with `augment` as well the
    joined batch then goes through the kernels above (_seen).  Not available with real_features."""
    if augment is not None and real_features is not None:
        raise ValueError('discriminator_loss: augment does not go with real_features (the two-pass layout)')
    if geo is not None and real_features is not None:
        raise ValueError('discriminator_loss: geo does not go with real_features (the two-pass layout)')
    if real_features is not None:
        real, fake = real_features, netD(fake_imgs.detach())
    else:
        real, fake = real_imgs, fake_imgs.detach()
    if real.shape != fake.shape:
        raise ValueError('discriminator_loss: real %s and fake %s differ in shape'
                         % (tuple(real.shape), tuple(fake.shape)))
    if augment is not None or geo is not None:
        feats = _seen(real, fake, augment, geo)
    else:
        feats = torch.cat((real, fake), 0)
    if real_features is None:
        feats = netD(feats, groups=2)
    return ops.d_heads(netD, feats, conditions, d_term_heads(real.size(0), netD.UNCOND_DNET is not None),
                       sink=count_sink)


def damsm_image_terms(image_encoder, fake_img, words_embs, sent_emb, match_labels, cap_lens, class_ids):
    """The DAMSM ranking terms of generator_loss (losses.py:187-204) for one batch of fake images, together with
    their gradient with respect to the images: returns (w_loss, s_loss, d(w_loss + s_loss)/d fake_img).

    These terms depend on the generator's output only -- not on the discriminators -- so a trainer can evaluate
    them (image encoder forward, words / sentence loss, backward through the frozen encoder) beside the
    discriminator updates and hand the image gradient to the generator's backward pass later
    (generator_loss(..., damsm=...)); by linearity the parameter gradients are those of the reference's single
    backward pass of errG_total."""
    batch_size = fake_img.size(0)
    leaf = fake_img.detach().requires_grad_(True)
    region_features, cnn_code = image_encoder(leaf)
    if DIRECT_DAMSM and match_labels is not None and region_features.is_cuda:
        # the loss heads and their gradients as ten back-to-back launches (ops.damsm_terms_direct), then ONLY the encoder's
        # backward pass through autograd -- bit-identical to the Function path below
        s = cfg.TRAIN.SMOOTH
        mask = class_mask(class_ids, batch_size, region_features.device)
        w_loss, s_loss, dfeat, dcnn = ops.damsm_terms_direct(
            region_features, cnn_code, words_embs, sent_emb, cap_lens, mask,
            (float(s.GAMMA1), float(s.GAMMA2), float(s.GAMMA3)), float(s.LAMBDA))
        (grad,) = torch.autograd.grad([region_features, cnn_code],
                                      leaf, [dfeat.to(region_features.dtype), dcnn.to(cnn_code.dtype)])
        return w_loss, s_loss, grad
    w_loss0, w_loss1, _ = words_loss(region_features, words_embs, match_labels, cap_lens, class_ids, batch_size)
    w_loss = (w_loss0 + w_loss1) * cfg.TRAIN.SMOOTH.LAMBDA
    s_loss0, s_loss1 = sent_loss(cnn_code, sent_emb, match_labels, class_ids, batch_size)
    s_loss = (s_loss0 + s_loss1) * cfg.TRAIN.SMOOTH.LAMBDA
    (grad,) = torch.autograd.grad(w_loss + s_loss, leaf)
    return w_loss.detach(), s_loss.detach(), grad


def _g_term(netD, features, sent_emb):
    """the adversarial term of generator_loss for one discriminator's features of the fake images (losses.py:168-186)"""
    return ops.d_heads(netD, features, sent_emb, g_term_heads(features.size(0), netD.UNCOND_DNET is not None))


def generator_d_term(netD, fake_img, sent_emb, augment=None, geo=None):
    """One discriminator's term of generator_loss (losses.py:168-186) on its own, together with its gradient with
    respect to the fake images: returns (g_loss, d g_loss / d fake_img).

    The term needs discriminator i AFTER its update and fake image i, nothing else: a trainer can evaluate it -- forward
    through the discriminator, backward to the image -- on the stream of that discriminator's update, right behind its
    optimizer step, while the other discriminators are still updating, and hand the image gradients to the generator's
    single backward pass later (generator_loss(..., d_terms=...), backward_with_image_grads); by linearity the parameter
    gradients are those of the reference's backward pass of errG_total.  The discriminator's parameters must not
    require gradients (the reference computes and discards them, trainer.py:270,287).

    augment (optional, (rows [n][8], flags)): the discriminator sees the augmented image (ops.diffaug); the returned
    gradient is with respect to the image itself, through the augmentation.

    geo (optional, f32 [n][4]): the image is warped first (ops.geoaug); the gradient comes back through its adjoint."""
    leaf = fake_img.detach().requires_grad_(True)
    seen = leaf if augment is None and geo is None else _seen(None, leaf, augment, geo)
    g_loss = _g_term(netD, netD(seen), sent_emb)
    (grad,) = torch.autograd.grad(g_loss, leaf)
    return g_loss.detach(), grad


def generator_loss(netsD, image_encoder, fake_imgs, real_labels, words_embs, sent_emb, match_labels,
                   cap_lens, class_ids, streams=None, damsm=None, d_terms=None, augment=None, geo=None):
    """losses.py:164-206.  Returns (errG_total, logs) where logs is a dict of device scalars
    {'g_loss0', ..., 'w_loss', 's_loss'} (format with .item() outside the step).

    streams (optional, len(netsD) + 1 HIP streams): the per-discriminator terms and the
    encoder + DAMSM term are independent branches (forward and backward), so each may run on its
    own stream; autograd replays every branch's backward on the stream of its forward.

    damsm (optional, the (w_loss, s_loss, image gradient) of damsm_image_terms): the ranking terms were
    evaluated ahead of time; errG_total then carries their VALUES (same summation order as the reference) and the
    caller back-propagates with `backward_with_image_grad`.

    d_terms (optional, the g_loss values of generator_d_term, one per discriminator): likewise for the adversarial
    terms; the caller back-propagates with `backward_with_image_grads`.

    augment (optional, one (rows [n][8], flags) per discriminator): each discriminator sees its fake image through
    ops.diffaug; the ranking terms see the image itself.

    geo (optional, one f32 [n][4] per discriminator): each discriminator sees its fake image through ops.geoaug first."""
    import contextlib
    numDs = len(netsD)
    batch_size = real_labels.size(0)
    logs = LossLogs()
    main = torch.cuda.current_stream() if streams else None

    def branch(k):
        if not streams:
            return contextlib.nullcontext()
        streams[k].wait_stream(main)
        return torch.cuda.stream(streams[k])

    terms = []
    for i in range(numDs):
        if d_terms is not None:         # evaluated ahead of time (generator_d_term): the VALUES, same summation order
            g_loss = d_terms[i]
        else:
            with branch(i):
                seen = fake_imgs[i]
                if augment is not None or geo is not None:
                    seen = _seen(None, seen, None if augment is None else augment[i], None if geo is None else geo[i])
                g_loss = _g_term(netsD[i], netsD[i](seen), sent_emb)
        terms.append(g_loss)
        logs['g_loss%d' % i] = g_loss.detach()
    if damsm is not None:
        w_loss, s_loss = damsm[0], damsm[1]
    else:
        # ranking loss on the last scale (losses.py:187-204).  An encoder that schedules its own branches
        # (sbagan.inception_hip: it has a `mode`) stays on the calling stream: it already overlaps the D branches, and
        # nested forks (mode 'streams') inside a captured branch crash hipStreamEndCapture on ROCm 7.2.
        own = streams and not hasattr(image_encoder, 'mode')
        with (branch(numDs) if own else contextlib.nullcontext()):
            region_features, cnn_code = image_encoder(fake_imgs[numDs - 1])
            w_loss0, w_loss1, _ = words_loss(region_features, words_embs, match_labels, cap_lens, class_ids,
                                             batch_size)
            w_loss = (w_loss0 + w_loss1) * cfg.TRAIN.SMOOTH.LAMBDA
            s_loss0, s_loss1 = sent_loss(cnn_code, sent_emb, match_labels, class_ids, batch_size)
            s_loss = (s_loss0 + s_loss1) * cfg.TRAIN.SMOOTH.LAMBDA
    if streams:
        for st in streams[:numDs + 1]:
            main.wait_stream(st)
    errG_total = 0
    for i in range(numDs):
        errG_total = errG_total + terms[i]          # same summation order as the reference
    errG_total = errG_total + w_loss + s_loss
    logs['w_loss'] = w_loss.detach()
    logs['s_loss'] = s_loss.detach()
    return errG_total, logs


def backward_with_image_grads(errG_total, fake_imgs, image_grads):
    """One backward pass for errG_total whose adversarial AND ranking terms were evaluated ahead of time
    (generator_loss(..., d_terms=..., damsm=...)): their gradients enter at the generator's images; errG_total itself
    carries the graph of the KL term only."""
    torch.autograd.backward([errG_total] + list(fake_imgs), [None] + list(image_grads))


def backward_with_image_grad(errG_total, fake_img, image_grad):
    """One backward pass for errG_total whose DAMSM terms were evaluated ahead of time: their gradient enters at
    the generator's last image (generator_loss(..., damsm=...))."""
    torch.autograd.backward([errG_total, fake_img], [None, image_grad])


def KL_loss(mu, logvar):
    """losses.py:210-214."""
    return ops.KLFn.apply(mu, logvar)
