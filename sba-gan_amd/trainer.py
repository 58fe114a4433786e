"""condGANTrainer with the reference's surface (AttnGAN2/code/trainer.py:28-518): build_models,
define_optimizers, prepare_labels, save_model, train, sampling, gen_example -- driving the HIP modules.

What differs, none of it in results:
  * the optimizers are the fused Adam(+EMA) launches over flat parameter buffers (sbagan.trainer.GANStep):
    `define_optimizers` returns them in the reference's (optimizerG, [optimizerD...]) shape;
  * one training step is GANStep.step (same order as trainer.py:245-299), the per-100-iteration log lines are
    formatted from device scalars outside the step (the reference's five .item() syncs per step are gone);
  * with `replay` (--replay) the loop trains every batch through ONE recording of that step, re-issued by the native
    launch replayer from a static batch slot (sbagan.static_batch): per iteration the host draws the
    batch, uploads its integers, launches the image pyramid, draws the noise and replays;
  * `save_img_results` writes a plain image grid per scale; with `attention_maps` (--attention_maps) it writes the
    reference's attention overlays instead (G_*.png per attention stage, D_*.png for the DAMSM maps), built on the
    device by sbagan.visualize from the overlays' contract, and gen_example adds the top-5 strips;
  * checkpoints are the reference's files: Model/netG_epoch_N.pth (EMA weights, trainer.py:159-164) and
    Model/netD{i}.pth, loadable by either implementation.  With cfg.TRAIN.NET_E == '' the reference prints an
    error and fails; pass `allow_random_encoders=True` to train against randomly initialised frozen encoders
    (synthetic-data runs and tests);
  * with `track` (--track E) the EMA generator is evaluated on a held-out split at the end of every E-th epoch and after
    the final checkpoint (sbagan.track): Model/track.jsonl, and with `track_best` Model/netG_best.pth / best.json.
"""
import json
import os
import time

import numpy as np
import torch
from PIL import Image

from datasets import as_batch, prepare_data
from miscc.config import cfg
from miscc.utils import copy_G_params, load_params, mkdir_p, weights_init
from model import CNN_ENCODER, D_NET64, D_NET128, D_NET256, G_NET, RNN_ENCODER
from sbagan import evaluation, truncation
from sbagan.trainer import GANStep, build_mask, prepare_labels


def _to_uint8(img):
    """[-1, 1] CHW float -> HWC uint8 (trainer.py:419-422)."""
    im = (img.detach().float().cpu().numpy() + 1.0) * 127.5
    return np.transpose(im.clip(0, 255).astype(np.uint8), (1, 2, 0))


class condGANTrainer(object):
    def __init__(self, output_dir, data_loader, n_words, ixtoword, allow_random_encoders=False):
        if cfg.TRAIN.FLAG:
            self.model_dir = os.path.join(output_dir, 'Model')
            self.image_dir = os.path.join(output_dir, 'Image')
            mkdir_p(self.model_dir)
            mkdir_p(self.image_dir)
        torch.cuda.set_device(cfg.GPU_ID)
        self.device = torch.device('cuda', cfg.GPU_ID)
        self.batch_size = cfg.TRAIN.BATCH_SIZE
        self.max_epoch = cfg.TRAIN.MAX_EPOCH
        self.snapshot_interval = cfg.TRAIN.SNAPSHOT_INTERVAL
        self.n_words = n_words
        self.ixtoword = ixtoword
        self.data_loader = data_loader
        self.num_batches = len(self.data_loader)
        self.allow_random_encoders = allow_random_encoders

    # ------------------------------------------------------------------ models (trainer.py:47-130)
    def _generator(self):
        if cfg.GAN.B_DCGAN:
            raise NotImplementedError('G_DCGAN is dead code in the reference (SURVEY.md 2): not built')
        return G_NET()

    # hooks of the text side (trainer_bert.condGANTrainer overrides them with the BERT encoder)
    def _text_encoder(self):
        return RNN_ENCODER(self.n_words, nhidden=cfg.TEXT.EMBEDDING_DIM)

    def _noise_shape(self, n):
        return (n, cfg.GAN.Z_DIM)

    def build_models(self):
        dev = self.device
        image_encoder = CNN_ENCODER(cfg.TEXT.EMBEDDING_DIM)
        text_encoder = self._text_encoder()
        if cfg.TRAIN.NET_E == '':
            print('Error: no pretrained text-image encoders')
            if not self.allow_random_encoders:
                return
        else:
            img_encoder_path = cfg.TRAIN.NET_E.replace('text_encoder', 'image_encoder')
            image_encoder.load_state_dict(torch.load(img_encoder_path, map_location='cpu'))
            print('Load image encoder from:', img_encoder_path)
            text_encoder.load_state_dict(torch.load(cfg.TRAIN.NET_E, map_location='cpu'))
            print('Load text encoder from:', cfg.TRAIN.NET_E)
        for p in image_encoder.parameters():
            p.requires_grad = False
        image_encoder.eval()
        for p in text_encoder.parameters():
            p.requires_grad = False
        text_encoder.eval()
        netG = self._generator()
        netsD = [D() for D in (D_NET64, D_NET128, D_NET256)[:cfg.TREE.BRANCH_NUM]]
        netG.apply(weights_init)
        for d in netsD:
            d.apply(weights_init)
        print('# of netsD', len(netsD))
        epoch = 0
        if cfg.TRAIN.NET_G != '':
            netG.load_state_dict(torch.load(cfg.TRAIN.NET_G, map_location='cpu'))
            print('Load G from: ', cfg.TRAIN.NET_G)
            istart = cfg.TRAIN.NET_G.rfind('_') + 1
            iend = cfg.TRAIN.NET_G.rfind('.')
            epoch = int(cfg.TRAIN.NET_G[istart:iend]) + 1
            if cfg.TRAIN.B_NET_D:
                Gname = cfg.TRAIN.NET_G
                for i in range(len(netsD)):
                    Dname = '%s/netD%d.pth' % (Gname[:Gname.rfind('/')], i)
                    print('Load D from: ', Dname)
                    netsD[i].load_state_dict(torch.load(Dname, map_location='cpu'))
        text_encoder = text_encoder.to(dev)
        image_encoder = image_encoder.to(dev)
        netG.to(dev)
        for d in netsD:
            d.to(dev)
        return [text_encoder, image_encoder, netG, netsD, epoch]

    def define_optimizers(self, netG, netsD, image_encoder=None):
        """trainer.py:132-145.  Returns (optimizerG, optimizersD): the fused Adam objects of the GANStep that owns
        the flat parameter / gradient / moment buffers (kept as self.gan)."""
        enc = image_encoder
        if enc is not None and enc.__class__.__name__ == 'CNN_ENCODER':
            from sbagan.inception_hip import InceptionHIP
            enc = InceptionHIP(enc)
        self.gan = GANStep(netG, netsD, enc, self.batch_size)
        if self.diffaug and cfg.TRAIN.FLAG:
            # --diffaug: every image a discriminator sees goes through the augmentation; its uniforms are
            # drawn beside the noise, by the loops below and by the recorded step's own draws
            from sbagan.diffaug import DiffAugment
            self.gan.augment = DiffAugment(self.diffaug, self.batch_size, len(netsD), self.gan.device,
                                           p0=self.diffaug_p, target=self.ada, kimg=self.ada_kimg,
                                           interval=self.ada_interval, p_max=self.ada_pmax)
            if self.gan.augment.adaptive:
                self._restore_ada(self.gan.augment)
        if self.geoaug and cfg.TRAIN.FLAG:
            # --geoaug: the geometric family in front of the same discriminators, gated by the p of
            # --diffaug_p / --ada where there is one
            from sbagan.geoaug import GeoAugment
            aug = self.gan.augment
            self.gan.geo_augment = GeoAugment(self.geoaug, self.batch_size, len(netsD), self.gan.device,
                                              p=aug.p if aug is not None and aug.gated else None)
        return self.gan.optG, self.gan.optD

    def prepare_labels(self):
        return prepare_labels(self.batch_size, self.device)

    def save_model(self, netG, avg_param_G, netsD, epoch):
        """trainer.py:159-170: netG_epoch_N.pth holds the EMA weights."""
        backup_para = copy_G_params(netG)
        load_params(netG, avg_param_G)
        torch.save(netG.state_dict(), '%s/netG_epoch_%d.pth' % (self.model_dir, epoch))
        load_params(netG, backup_para)
        for i, netD in enumerate(netsD):
            torch.save(netD.state_dict(), '%s/netD%d.pth' % (self.model_dir, i))
        augment = getattr(getattr(self, 'gan', None), 'augment', None)
        if augment is not None and augment.adaptive:        # --ada: the controller's state beside the discriminators
            torch.save(augment.state_dict(), '%s/ada_state.pth' % self.model_dir)
        print('Save G/Ds models.')

    def _restore_ada(self, augment):
        """on resume (TRAIN.NET_G set): the controller state saved beside the generator checkpoint, if there is one"""
        if cfg.TRAIN.NET_G == '':
            return
        path = os.path.join(os.path.dirname(cfg.TRAIN.NET_G), 'ada_state.pth')
        if os.path.isfile(path):
            augment.load_state_dict(torch.load(path, map_location='cpu'))
            print('Load ada state from: ', path)
        else:
            print('no ada_state.pth beside %s: p restarts from its initial value %g' % (cfg.TRAIN.NET_G, augment.p0))

    def _report_ada(self, augment, gen_iterations):
        """the --ada line of the interval log and its JSON twin in Model/ada.jsonl: ONE read-back of p and r_t"""
        p, rt = augment.report()
        print('ada p: ' + ' '.join('%.3f' % v for v in p) + ' r_t: ' + ' '.join('%.2f' % v for v in rt))
        with open(os.path.join(self.model_dir, 'ada.jsonl'), 'a') as f:
            f.write(json.dumps({'iteration': gen_iterations, 'p': p, 'r_t': rt}) + '\n')

    def set_requires_grad_value(self, models_list, brequires):
        for m in models_list:
            for p in m.parameters():
                p.requires_grad = brequires

    def save_img_results(self, netG, noise, sent_emb, words_embs, mask, image_encoder, captions, cap_lens,
                         gen_iterations, name='current'):
        """trainer.py:177-216.  Without attention_maps: one plain grid (up to 8 samples) per scale.  With it: per
        attention stage i the overlay grid G_<name>_<it>_<i>.png (stage i + 1's images, stage i's in the first row), and
        D_<name>_<it>.png: the last stage through the image encoder and its DAMSM word-to-region maps."""
        was = netG.training
        netG.eval()
        if self.attention_maps:
            stages = [m for m in netG.modules() if hasattr(m, 'return_attention')]
            flags = [m.return_attention for m in stages]
            netG.set_return_attention(True)
        try:
            with torch.no_grad():
                fake_imgs, att_maps, _, _ = netG(noise, sent_emb, words_embs, mask)
        finally:
            if self.attention_maps:
                for m, flag in zip(stages, flags):
                    m.return_attention = flag
            netG.train(was)
        if self.attention_maps:
            from sbagan.visualize import build_super_images, damsm_attention_maps
            for i, att in enumerate(att_maps):
                img_set, _ = build_super_images(fake_imgs[i + 1], captions, self.ixtoword, att, att.size(2),
                                                lr_imgs=fake_imgs[i])
                Image.fromarray(img_set).save('%s/G_%s_%d_%d.png' % (self.image_dir, name, gen_iterations, i))
            n = min(8, fake_imgs[-1].size(0))
            with torch.no_grad():
                region_features, _ = image_encoder(fake_imgs[-1][:n].detach())
            maps = damsm_attention_maps(region_features, words_embs[:n], cap_lens[:n], cfg.TRAIN.SMOOTH.GAMMA1)
            img_set, _ = build_super_images(fake_imgs[-1][:n], captions[:n], self.ixtoword, maps,
                                            region_features.size(2))
            Image.fromarray(img_set).save('%s/D_%s_%d.png' % (self.image_dir, name, gen_iterations))
            return
        for i, f in enumerate(fake_imgs):
            tiles = [_to_uint8(f[j]) for j in range(min(8, f.size(0)))]
            Image.fromarray(np.concatenate(tiles, 1)).save('%s/G_%s_%d_%d.png' % (self.image_dir, name, gen_iterations, i))

    # ------------------------------------------------------------------ training loop (trainer.py:218-346)
    def _encode(self, text_encoder, captions, cap_lens, out=None):
        """out = (words_embs, sent_emb): the static-output form of the recorded loop -- no host sync, the full padded
        width out[0].size(2), the same zero hidden state every call (made on the first, eager one), results written
        into `out`"""
        if out is not None:
            key = (id(text_encoder), captions.size(0))
            if getattr(self, '_static_hidden', (None,))[0] != key:
                self._static_hidden = (key, text_encoder.init_hidden(captions.size(0)))
            with torch.no_grad():
                words_embs, sent_emb = text_encoder(captions, cap_lens, self._static_hidden[1],
                                                    max_len=out[0].size(2), out=out)
            if words_embs is not out[0]:        # (an encoder off the HIP path returns tensors of its own)
                out[0].copy_(words_embs)
                out[1].copy_(sent_emb)
            return out
        hidden = text_encoder.init_hidden(captions.size(0))
        with torch.no_grad():
            words_embs, sent_emb = text_encoder(captions, cap_lens, hidden, max_len=int(cap_lens.max()))
        return words_embs.detach(), sent_emb.detach()

    replay = False              # --replay: train() runs every batch through ONE recording of the step
    replay_eager = False        # with replay: the same loop over the static batch slot, the step launched eagerly
    diffaug = ''                # --diffaug POLICY: Differentiable Augmentation in front of the discriminators ('' = off)
    diffaug_p = None            # --diffaug_p P: each part with probability P (the gated kernels); None = always
    ada = None                  # --ada TARGET: p follows the overfitting read-out r_t on the device
    ada_kimg, ada_interval, ada_pmax = 500.0, 4, 1.0
    geoaug = ''                 # --geoaug POLICY: flip, rot90, scale, rotate in front of the discriminators ('' = off)
    log_interval = 100          # iterations between two loss lines
    average_interval = 1000     # iterations between the 'average' (EMA generator) image dumps

    track = 0                   # --track E: evaluate the EMA generator on a held-out split every E epochs
    track_split, track_n, track_captions, track_best = 'test', 0, 1, None

    def _tracker(self):
        """the held-out evaluation of --track (sbagan.track.Tracker), or None when the flag is off"""
        if not self.track:
            return None
        from sbagan.track import Tracker
        return Tracker(self, self.track, self.track_split, self.track_n, self.track_captions, self.track_best)

    def _replay_step(self, text_encoder, noise):
        """the static batch slot and the step over it (sbagan.static_batch); a device loader writes straight into it"""
        from miscc import cli
        from sbagan.static_batch import SlotStep, StaticBatch
        loader = self.data_loader
        if not getattr(loader, 'drop_last', False):
            raise RuntimeError('--replay needs a loader that drops the last, smaller batch (drop_last): the recorded '
                               'step reads a batch slot of fixed shape')
        slot = StaticBatch(self.batch_size, cfg.TEXT.WORDS_NUM, cfg.TREE.BRANCH_NUM,
                           getattr(loader, 'crop', None) or cli.image_size(), self.device)
        if hasattr(loader, 'bind'):
            loader.bind(slot)
        prologue = slot.prologue(text_encoder, encode=self._encode)
        return slot, SlotStep(self.gan, slot, prologue, noise, eager=self.replay_eager)

    def train(self, max_steps=None):
        try:
            return self._train(max_steps)
        finally:        # (--replay binds a device loader to the run's batch slot)
            if getattr(self.data_loader, 'slot', None) is not None:
                self.data_loader.bind(None)

    def _train(self, max_steps=None):
        built = self.build_models()
        if built is None:
            return
        text_encoder, image_encoder, netG, netsD, start_epoch = built
        self.define_optimizers(netG, netsD, image_encoder)
        gan = self.gan
        netG.set_return_attention(False)        # unused in the step (trainer.py:262)
        batch_size = self.batch_size
        noise = torch.empty(self._noise_shape(batch_size), device=self.device)
        fixed_noise = torch.randn(self._noise_shape(batch_size), device=self.device)
        gen_iterations = 0
        out = None
        slot = stepper = None
        if self.replay:
            slot, stepper = self._replay_step(text_encoder, noise)
        self.slot, self.slot_step = slot, stepper
        self.tracker = tracker = self._tracker()
        for epoch in range(start_epoch, self.max_epoch):
            start_t = time.time()
            step = 0
            for data in self.data_loader:
                if stepper is not None:
                    # the batch goes into the slot (one pinned upload; the device loader has put it there already), the
                    # step draws its own noise and eps and is re-issued from the recording: no host sync
                    imgs, captions, cap_lens, class_ids, keys = slot.load(as_batch(data))
                    out = stepper.train()
                    words_embs, sent_emb, mask = slot.words_embs, slot.sent_emb, slot.mask
                else:
                    imgs, captions, cap_lens, class_ids, keys = as_batch(data)
                    words_embs, sent_emb = self._encode(text_encoder, captions, cap_lens)
                    mask = build_mask(captions, words_embs.size(2))
                    noise.normal_(0, 1)
                    if gan.augment is not None:
                        gan.augment.draw()
                    if gan.geo_augment is not None:
                        gan.geo_augment.draw()
                    out = gan.step(imgs, sent_emb, words_embs, mask, cap_lens, class_ids, noise)
                step += 1
                gen_iterations += 1
                if gen_iterations % self.log_interval == 0:
                    v = {k: float(t) for k, t in out.items()}
                    nD = len(netsD)
                    print(' '.join('errD%d: %.2f' % (i, v['errD%d' % i]) for i in range(nD)) + '\n' +
                          ' '.join('g_loss%d: %.2f' % (i, v['g_loss%d' % i]) for i in range(nD)) +
                          ' w_loss: %.2f s_loss: %.2f kl_loss: %.2f' % (v['w_loss'], v['s_loss'], v['kl_loss']))
                    if gan.augment is not None and gan.augment.adaptive:
                        self._report_ada(gan.augment, gen_iterations)
                if gen_iterations % self.average_interval == 0:
                    gan.finish()        # (data-parallel: a pending generator update is applied before it is read)
                    backup_para = copy_G_params(netG)
                    load_params(netG, gan.flatG.ema_params())
                    self.save_img_results(netG, fixed_noise, sent_emb, words_embs, mask, image_encoder, captions,
                                          cap_lens, epoch, name='average')
                    load_params(netG, backup_para)
                    if stepper is not None:     # the parameters were edited behind the recording's back
                        stepper.resync()
                if max_steps is not None and gen_iterations >= max_steps:
                    break
            end_t = time.time()
            if out is not None:
                errD_total = sum(float(out['errD%d' % i]) for i in range(len(netsD)))
                print('[%d/%d][%d]\n                  Loss_D: %.2f Loss_G: %.2f Time: %.2fs'
                      % (epoch, self.max_epoch, self.num_batches, errD_total, float(out['errG_total']),
                         end_t - start_t))
            if epoch % cfg.TRAIN.SNAPSHOT_INTERVAL == 0:
                gan.finish()
                self.save_model(netG, gan.flatG.ema_params(), netsD, epoch)
                if stepper is not None:
                    stepper.resync()
            if tracker is not None and tracker.due(epoch):
                # --track: the EMA weights, as save_model would write them now, on the held-out set (sbagan.track)
                snapshot = epoch % cfg.TRAIN.SNAPSHOT_INTERVAL == 0
                tracker.evaluate(netG, text_encoder, epoch, gen_iterations, stepper,
                                 'netG_epoch_%d.pth' % epoch if snapshot else None)
            if max_steps is not None and gen_iterations >= max_steps:
                break
        gan.finish()
        self.save_model(netG, gan.flatG.ema_params(), netsD, self.max_epoch)
        if tracker is not None:
            tracker.evaluate(netG, text_encoder, self.max_epoch, gen_iterations, stepper,
                             'netG_epoch_%d.pth' % self.max_epoch)

    # ------------------------------------------------------------------ inference (trainer.py:348-518)
    # Written from the OUTPUT-FILE contract of the reference's three inference entry points (what a user of its eval
    # scripts finds on disk), not from their statements:
    #   save_singleimages  <save_dir>/single_samples/<split_dir>/<filename>_<sentenceID>.jpg
    #   sampling           <NET_G without .pth>/<split>/single/<key>_s-1.png          (last stage only; 'test' -> 'valid')
    #   gen_example        <NET_G without .pth>/<key>/0_s_<original caption index>_g<stage>.png
    @staticmethod
    def _write_image(tensor_chw, path, made=None):
        """one CHW image in [-1, 1] to `path`, creating its directory the first time it is seen"""
        parent = os.path.dirname(path)
        if made is None or parent not in made:
            if not os.path.isdir(parent):
                mkdir_p(parent)
            if made is not None:
                made.add(parent)
        Image.fromarray(_to_uint8(tensor_chw)).save(path)

    def save_singleimages(self, images, filenames, save_dir, split_dir, sentenceID=0):
        root = os.path.join(save_dir, 'single_samples', split_dir)
        made = set()
        for img, name in zip(images, filenames):
            self._write_image(img, '%s_%d.jpg' % (os.path.join(root, name), sentenceID), made)

    def _load_inference_models(self):
        dev = self.device
        netG = self._generator()
        netG.apply(weights_init)
        text_encoder = self._text_encoder()
        if cfg.TRAIN.NET_E != '':
            text_encoder.load_state_dict(torch.load(cfg.TRAIN.NET_E, map_location='cpu'))
            print('Load text encoder from:', cfg.TRAIN.NET_E)
        elif not self.allow_random_encoders:
            raise RuntimeError('cfg.TRAIN.NET_E is empty: no text encoder to load')
        netG.load_state_dict(torch.load(cfg.TRAIN.NET_G, map_location='cpu'))
        print('Load G from: ', cfg.TRAIN.NET_G)
        return self._inference_generator(netG.to(dev).eval()), text_encoder.to(dev).eval()

    fused_inference = False     # --fused_inference: sampling() / gen_example() call the generator through FusedGenerator

    def _inference_generator(self, netG):
        """netG (in eval mode, on the device) itself, or its fused inference wrapper (sbagan/infer.py)"""
        if not self.fused_inference:
            return netG
        from sbagan.infer import FusedGenerator
        return FusedGenerator(netG)

    @staticmethod
    def _output_root():
        """the directory named after the generator checkpoint (its path without the .pth suffix), or None"""
        ckpt = cfg.TRAIN.NET_G
        if not ckpt:
            print('cfg.TRAIN.NET_G is empty: inference needs a generator checkpoint')
            return None
        cut = ckpt.rfind('.pth')
        return ckpt[:cut] if cut >= 0 else ckpt

    def _generate(self, netG, text_encoder, captions, cap_lens, noise, with_sent=False, with_att=False, keep=None):
        """fake images of every stage for one caption batch (noise is refilled in place); with_sent: and the sentence
        embeddings they were generated from; with_att: and the attention maps of every later stage; keep: a dict that
        receives the call's inputs (sent_emb, words_embs, mask, eps) for a caller that runs the generator on them again
        (_forward_kept)"""
        words_embs, sent_emb = self._encode(text_encoder, captions, cap_lens)
        noise.normal_(0, 1)
        mask = build_mask(captions, words_embs.size(2))
        if keep is not None:
            keep.update(sent_emb=sent_emb, words_embs=words_embs, mask=mask)
            fake_imgs, att_maps = self._forward_kept(netG, noise, keep)
        else:
            with torch.no_grad():
                fake_imgs, att_maps, _, _ = netG(noise, sent_emb, words_embs, mask)
        if with_att:
            return fake_imgs, att_maps
        return (fake_imgs, sent_emb) if with_sent else fake_imgs

    @staticmethod
    def _forward_kept(netG, noise, kept):
        """(fake images, attention maps) of netG on `noise` and the inputs of `kept` (_generate's keep).  The conditioning
        eps is part of them: the first call draws it -- by the very call CA_NET would make at this point of the global
        generator's sequence, so the run's draws are those of a run that keeps nothing -- and every later call reads
        it back and draws nothing."""
        ca_net = truncation.unwrap(netG).ca_net
        held = ca_net.eps
        if 'eps' not in kept:
            kept['eps'] = held if held is not None else torch.randn(
                (kept['sent_emb'].size(0), ca_net.c_dim), dtype=torch.float32, device=kept['sent_emb'].device)
        ca_net.eps = kept['eps']
        try:
            with torch.no_grad():
                return netG(noise, kept['sent_emb'], kept['words_embs'], kept['mask'])[:2]
        finally:
            ca_net.eps = held

    truncation_n = truncation.DEFAULT_N     # --truncation_n: codes in the mean style (the module, read before the line below)
    truncation = None           # --truncation PSI[,PSI]: the truncation trick in W for sampling / gen_example
    truncation_sweep = None     # --truncation_sweep LIST: sampling's psi sweep over a frozen set; gen_example's psi strips
    truncation_sweep_n = 0      # --truncation_sweep_n: images of the frozen set (0: the whole split)

    def _set_truncation(self, *generators):
        """--truncation: set on every loaded generator (each takes the mean of its own mapping network); returns the
        first one's Truncation, or None when the flag is off"""
        if self.truncation is None:
            return None
        return [truncation.set_truncation(g, self.truncation, self.truncation_n) for g in generators][0]

    def _write_psi_strips(self, netG, noise, kept, order, out_dir):
        """--truncation_sweep in gen_example: <out_dir>/0_s_<original index>_psi.png per caption -- the last stage's image
        of netG at every psi of the list, left to right, over the noise and the inputs of the run's own call (`kept`);
        no text is drawn, nothing is drawn from a generator.  The generator's truncation is put back."""
        net = truncation.unwrap(netG)
        held, base, tiles = net.truncation, net.truncation, []
        try:
            for psi in self.truncation_sweep:
                if base is None:
                    base = truncation.Truncation(net, psi, self.truncation_n)
                net.truncation = base.with_psi(psi)
                tiles.append(self._forward_kept(netG, noise, kept)[0][-1])
        finally:
            net.truncation = held
        for j, src in enumerate(order):
            strip = np.concatenate([_to_uint8(batch[j]) for batch in tiles], axis=1)
            Image.fromarray(strip).save(os.path.join(out_dir, '0_s_%d_psi.png' % int(src)))

    attention_maps = False      # --attention_maps: the attention overlays of save_img_results / gen_example

    def _write_top_words(self, stages, att_maps, captions, cap_lens, order, out_dir, suffix=''):
        """<out_dir>/0_s_<original index>_a<k><suffix>.png: per caption and attention stage k, the top-5 word strip over
        stage k + 1's image (sbagan.visualize.build_super_images2)"""
        from sbagan.visualize import build_super_images2
        lens = [int(v) for v in cap_lens.tolist()]
        for k, att in enumerate(att_maps):
            for j, src in enumerate(order):
                img_set, _ = build_super_images2(stages[k + 1][j], captions[j], lens[j], self.ixtoword, att[j],
                                                 att.size(2))
                Image.fromarray(img_set).save(os.path.join(out_dir, '0_s_%d_a%d%s.png' % (int(src), k, suffix)))

    def _load_image_encoder(self):
        """the DAMSM image encoder beside cfg.TRAIN.NET_E (as build_models finds it), frozen, in eval mode, behind its
        HIP forward (as define_optimizers wraps it).  Built with the CPU generator forked: its initialisation must not
        move the state the data loader's shuffle draws from."""
        from sbagan.inception_hip import InceptionHIP
        with torch.random.fork_rng(devices=[]):
            image_encoder = CNN_ENCODER(cfg.TEXT.EMBEDDING_DIM)
        if cfg.TRAIN.NET_E != '':
            img_encoder_path = cfg.TRAIN.NET_E.replace('text_encoder', 'image_encoder')
            image_encoder.load_state_dict(torch.load(img_encoder_path, map_location='cpu'))
            print('Load image encoder from:', img_encoder_path)
        elif not self.allow_random_encoders:
            raise RuntimeError('cfg.TRAIN.NET_E is empty: no image encoder to load')
        for p in image_encoder.parameters():
            p.requires_grad = False
        return InceptionHIP(image_encoder.to(self.device).eval())

    def sampling(self, split_dir):
        """trainer.py:363-433: one image (the last stage's) per caption of the split; beside them what the evaluators
        that are on report (sbagan.evaluation: its table names their attributes here, set below the class).  With
        `truncation` the generator is truncated in W (every file and figure sees it; truncation.json); with
        `truncation_sweep` the psi sweep follows the run (sbagan.truncation.sweep; truncation_sweep.json)."""
        root = self._output_root()
        if root is None:
            return None
        suite = evaluation.Suite({opt.name: getattr(self, opt.name) for opt in evaluation.OPTIONS}, split_dir,
                                 self._encode, self._load_image_encoder, self.data_loader, self.batch_size, self.device)
        out_dir = os.path.join(root, 'valid' if split_dir == 'test' else split_dir)
        mkdir_p(out_dir)
        netG, text_encoder = self._load_inference_models()
        truncated = self._set_truncation(netG)
        w_rms = truncation.WDistance(truncated) if truncated is not None else None
        suite.attach(text_encoder)
        noise = torch.empty(self._noise_shape(self.batch_size), device=self.device)
        made = set()
        for nbatch, data in enumerate(self.data_loader):
            if nbatch % 100 == 0:
                print('step: ', nbatch)
            real_imgs, captions, cap_lens, class_ids, keys = prepare_data(data)
            fake_imgs, sent_emb = self._generate(netG, text_encoder, captions, cap_lens, noise, with_sent=True)
            last = fake_imgs[-1]
            if w_rms is not None:
                w_rms.update(noise)
            suite.update(last, real_imgs[-1], sent_emb, class_ids, keys)
            for img, key in zip(last, keys):
                self._write_image(img, os.path.join(out_dir, 'single', key) + '_s-1.png', made)
        for stem, (evaluator, result) in suite.finish(out_dir).items():
            setattr(self, stem + '_evaluator', evaluator)
            setattr(self, stem + '_result', result)
        if truncated is not None:
            self.truncation_result = truncation.write_json(out_dir, truncated, w_rms)
        if self.truncation_sweep:
            # behind the normal run and its files: the sweep measures on a frozen set of its own and draws nothing
            ranking = suite.on.get('r_precision')
            trunk = suite.image_encoder if suite.image_encoder is not None else getattr(ranking, 'image_encoder', None)
            self.truncation_sweep_result = truncation.sweep(self, netG, text_encoder, self.truncation_sweep, split_dir,
                                                            out_dir, n=self.truncation_sweep_n, image_encoder=trunk)
        return out_dir

    def gen_example(self, data_dic):
        """trainer.py:435-518: data_dic[key] = [captions (n x Lmax int64, sorted by length), cap_lens, sorted_indices];
        every stage's image per caption, named by the caption's ORIGINAL position; with attention_maps also the
        top-5 word strips 0_s_<index>_a<k>.png; with truncation_sweep also the psi strips 0_s_<index>_psi.png."""
        root = self._output_root()
        if root is None:
            return None
        netG, text_encoder = self._load_inference_models()
        self._set_truncation(netG)
        for key, (captions, cap_lens, order) in data_dic.items():
            out_dir = os.path.join(root, key)
            print(out_dir)
            mkdir_p(out_dir)
            captions = torch.from_numpy(np.ascontiguousarray(captions)).to(self.device)
            cap_lens = torch.from_numpy(np.ascontiguousarray(cap_lens)).to(self.device)
            noise = torch.empty(self._noise_shape(captions.shape[0]), device=self.device)
            kept = {} if self.truncation_sweep else None
            stages, att_maps = self._generate(netG, text_encoder, captions, cap_lens, noise, with_att=True, keep=kept)
            for stage, batch in enumerate(stages):
                for img, src in zip(batch, order):
                    self._write_image(img, os.path.join(out_dir, '0_s_%d_g%d.png' % (int(src), stage)))
            if self.attention_maps:
                self._write_top_words(stages, att_maps, captions, cap_lens, order, out_dir)
            if self.truncation_sweep:
                self._write_psi_strips(netG, noise, kept, order, out_dir)
        return root


# the evaluation attributes of sampling(): every option of sbagan.evaluation's table with its default, and per evaluator
# <stem>_evaluator / <stem>_result of the last sampling() that had it on
for _name, _default in evaluation.ATTRIBUTES:
    setattr(condGANTrainer, _name, _default)
