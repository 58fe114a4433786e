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
    (synthetic-data runs and tests).
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
from sbagan.trainer import GANStep, build_mask, prepare_labels


def _figure(value):
    """a figure that may be missing (sbagan.nearest reports None where no row has a neighbour)"""
    return 'n/a' if value is None else '%.6g' % value


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
            self.gan.augment = DiffAugment(self.diffaug, self.batch_size, len(netsD), self.gan.device)
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
        print('Save G/Ds models.')

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
    average_interval = 1000     # iterations between the 'average' (EMA generator) image dumps

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
                    out = gan.step(imgs, sent_emb, words_embs, mask, cap_lens, class_ids, noise)
                step += 1
                gen_iterations += 1
                if gen_iterations % 100 == 0:
                    v = {k: float(t) for k, t in out.items()}
                    nD = len(netsD)
                    print(' '.join('errD%d: %.2f' % (i, v['errD%d' % i]) for i in range(nD)) + '\n' +
                          ' '.join('g_loss%d: %.2f' % (i, v['g_loss%d' % i]) for i in range(nD)) +
                          ' w_loss: %.2f s_loss: %.2f kl_loss: %.2f' % (v['w_loss'], v['s_loss'], v['kl_loss']))
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
            if max_steps is not None and gen_iterations >= max_steps:
                break
        gan.finish()
        self.save_model(netG, gan.flatG.ema_params(), netsD, self.max_epoch)

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

    def _generate(self, netG, text_encoder, captions, cap_lens, noise, with_sent=False, with_att=False):
        """fake images of every stage for one caption batch (noise is refilled in place); with_sent: and the sentence
        embeddings they were generated from; with_att: and the attention maps of every later stage"""
        words_embs, sent_emb = self._encode(text_encoder, captions, cap_lens)
        noise.normal_(0, 1)
        with torch.no_grad():
            fake_imgs, att_maps, _, _ = netG(noise, sent_emb, words_embs, build_mask(captions, words_embs.size(2)))
        if with_att:
            return fake_imgs, att_maps
        return (fake_imgs, sent_emb) if with_sent else fake_imgs

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

    r_precision = 0             # --r_precision R: sampling() also ranks every image among R candidate captions
    r_precision_seed = 100      # seed of the evaluator's own index generator and of the pool's caption draws
    r_precision_result = None   # the result dict of the last sampling() with r_precision != 0

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

    def _r_precision_evaluator(self, text_encoder):
        """sbagan.rprecision.RPrecision over the sentence embeddings of every caption of the sampled split"""
        from sbagan.rprecision import RPrecision, encode_pool
        if self.r_precision < 2:
            raise ValueError('r_precision must be 0 (off) or >= 2 candidates per image (got %d)' % self.r_precision)
        pool, pool_class = encode_pool(self.data_loader.dataset, lambda c, n: self._encode(text_encoder, c, n),
                                       self.batch_size, seed=self.r_precision_seed, device=self.device)
        return RPrecision(self._load_image_encoder(), pool, pool_class, R=self.r_precision, seed=self.r_precision_seed)

    fid = False                 # --fid: sampling() also takes the FID between the split's real images and the fakes
    fid_stats = None            # --fid_stats PATH: the real side's statistics, read when present, written when not
    fid_result = None           # the result dict of the last sampling() with fid on

    def _fid_evaluator(self, image_encoder, split_dir):
        """sbagan.fid.FID on the pooled trunk feature of `image_encoder` (an InceptionHIP); the real side comes from
        fid_stats when that file exists"""
        from miscc import cli
        from sbagan.feature_rows import dtype_name
        from sbagan.fid import FID, stats_key
        dtype = dtype_name()
        key = stats_key(cfg.TRAIN.NET_E.replace('text_encoder', 'image_encoder'), dtype, split_dir, cli.image_size())
        evaluator = FID(image_encoder.pooled_features, D=2048, key=key, dtype=dtype)
        if self.fid_stats and os.path.exists(self.fid_stats):
            evaluator.load_real(self.fid_stats)
            print('Load real FID statistics from:', self.fid_stats)
        return evaluator

    prdc = 0                    # --prdc K: sampling() also takes precision / recall / density / coverage at k = K
    prdc_result = None          # the result dict of the last sampling() with prdc != 0

    def _prdc_evaluator(self, image_encoder):
        """sbagan.prdc.PRDC on the pooled trunk feature of `image_encoder` (an InceptionHIP)"""
        from sbagan import ops
        from sbagan.feature_rows import dtype_name
        from sbagan.prdc import PRDC
        if isinstance(self.prdc, bool) or not isinstance(self.prdc, int) or not 1 <= self.prdc <= ops.PRDC_MAX_K:
            raise ValueError('prdc must be 0 (off) or a neighbour count from 1 to %d (got %r)'
                             % (ops.PRDC_MAX_K, self.prdc))
        return PRDC(image_encoder.pooled_features, D=2048, k=self.prdc, dtype=dtype_name())

    kid = False                 # --kid: sampling() also takes the Kernel Inception Distance
    kid_subsets = 100           # --kid_subsets N
    kid_subset_size = 1000      # --kid_subset_size M: rows per subset and side, clamped to the smaller side
    kid_seed = 100              # of the evaluator's own generator for the subset draws
    kid_result = None           # the result dict of the last sampling() with kid on
    kid_evaluator = None

    def _kid_evaluator(self, image_encoder, prdc):
        """sbagan.kid.KID on the pooled trunk feature of `image_encoder` (an InceptionHIP); with a PRDC evaluator it
        reads that one's rows and stores none"""
        from sbagan.feature_rows import dtype_name
        from sbagan.kid import KID
        return KID(image_encoder.pooled_features, D=2048, subsets=self.kid_subsets, subset_size=self.kid_subset_size,
                   seed=self.kid_seed, dtype=dtype_name(), rows=prdc)

    ms_ssim = 0                 # --ms_ssim N: sampling() also takes the mean MS-SSIM over N same-class pairs per class
    ms_ssim_seed = 100          # of the evaluator's own generator for the pair draws
    ms_ssim_result = None       # the result dict of the last sampling() with ms_ssim != 0
    ms_ssim_evaluator = None

    def _ms_ssim_evaluator(self):
        """sbagan.msssim.MSSSIM on the uint8 pixels of the last stage's images; refuses a configuration whose images
        are too small for five scales"""
        from miscc import cli
        from sbagan.msssim import MSSSIM
        if isinstance(self.ms_ssim, bool) or not isinstance(self.ms_ssim, int) or self.ms_ssim < 1:
            raise ValueError('ms_ssim must be 0 (off) or a number of pairs per class (got %r)' % (self.ms_ssim,))
        return MSSSIM(self.ms_ssim, size=cli.image_size(), seed=self.ms_ssim_seed)

    swd = 0                     # --swd N: sampling() also takes the sliced Wasserstein distance per resolution between the
    #                             first N real and the first N generated images (0 = off)
    swd_seed = 100              # of the evaluator's own generator for the patch positions and the directions
    swd_result = None           # the result dict of the last sampling() with swd != 0
    swd_evaluator = None

    def _swd_evaluator(self, ms_ssim=None):
        """sbagan.swd.SWD on the uint8 pixels of the last stage's images; refuses an image size it has no pyramid for.
        ms_ssim: the MS-SSIM evaluator of the same run, whose stored images it then reads instead of keeping its own"""
        from miscc import cli
        from sbagan.swd import SWD
        if isinstance(self.swd, bool) or not isinstance(self.swd, int) or self.swd < 1:
            raise ValueError('swd must be 0 (off) or a number of images per side (got %r)' % (self.swd,))
        return SWD(self.swd, size=cli.image_size(), seed=self.swd_seed, images=ms_ssim)

    nearest = 0                 # --nearest K: sampling() also lists every generated image's K nearest TRAINING images and takes
    #                             the memorisation figures of sbagan.nearest (0 = off)
    nearest_stats = None        # --nearest_stats PATH: the training rows and keys, read when present, written when not
    nearest_show = 16           # --nearest_show M: suspects in nearest.json and rows of nearest.png (0: no picture)
    nearest_result = None       # the result dict of the last sampling() with nearest != 0
    nearest_evaluator = None

    def _nearest_evaluator(self, image_encoder):
        """sbagan.nearest.Nearest on the pooled trunk feature of `image_encoder` (an InceptionHIP); the training side
        comes from nearest_stats when that file exists"""
        from miscc import cli
        from sbagan import ops
        from sbagan.feature_rows import dtype_name
        from sbagan.nearest import Nearest, stats_key
        if isinstance(self.nearest, bool) or not isinstance(self.nearest, int) or not 1 <= self.nearest <= ops.KNN_MAX_K:
            raise ValueError('nearest must be 0 (off) or a neighbour count from 1 to %d (got %r)'
                             % (ops.KNN_MAX_K, self.nearest))
        dtype = dtype_name()
        key = stats_key(cfg.TRAIN.NET_E.replace('text_encoder', 'image_encoder'), dtype, 'train', cli.image_size())
        evaluator = Nearest(image_encoder.pooled_features, D=2048, k=self.nearest, show=int(self.nearest_show), key=key,
                            dtype=dtype)
        if self.nearest_stats and os.path.exists(self.nearest_stats):
            evaluator.load_train(self.nearest_stats, self.device)
            print('Load training rows from:', self.nearest_stats)
        return evaluator

    def _train_crops(self):
        """the training split as the nearest-neighbour pass reads it: the data set class of the sampled split on 'train',
        every image through retrieval._CenterCrops at the size the sampling loader yields for its last scale"""
        from miscc import cli
        from sbagan.retrieval import _CenterCrops
        sampled = self.data_loader.dataset
        extra = {'bert_dir': sampled.bert_dir} if hasattr(sampled, 'bert_dir') else {}
        train = type(sampled)(sampled.data_dir, 'train', base_size=cfg.TREE.BASE_SIZE, transform=None, **extra)
        imsize = cli.image_size()
        return _CenterCrops(train, imsize, int(imsize * 76 / 64))

    def _nearest_finish(self, nearest, res, out_dir, crops):
        """after the result: the cache of the training rows, and nearest.png (sbagan.nearest.write_sheet)"""
        from sbagan.nearest import write_sheet
        if self.nearest_stats and not nearest.is_loaded():
            nearest.save_train(self.nearest_stats)
            print('Save training rows to:', self.nearest_stats)
        if nearest.show:
            crops = crops if crops is not None else self._train_crops()
            if [str(k) for k in crops.dataset.filenames] != nearest.keys['train']:
                raise RuntimeError('nearest: the cached training keys are not those of the training split')
            write_sheet(os.path.join(out_dir, 'nearest.png'), res['suspects'], nearest.k,
                        lambda key: os.path.join(out_dir, 'single', key) + '_s-1.png', crops.window)

    def sampling(self, split_dir):
        """trainer.py:363-433: one image (the last stage's) per caption of the split."""
        root = self._output_root()
        if root is None:
            return None
        ms_ssim = self._ms_ssim_evaluator() if self.ms_ssim else None   # (refused before anything is written)
        swd = self._swd_evaluator(ms_ssim) if self.swd else None        # (likewise)
        out_dir = os.path.join(root, 'valid' if split_dir == 'test' else split_dir)
        mkdir_p(out_dir)
        netG, text_encoder = self._load_inference_models()
        evaluator = self._r_precision_evaluator(text_encoder) if self.r_precision else None
        fid = fid_real = prdc = kid = nearest = None
        if self.fid or self.prdc or self.kid or self.nearest:       # one image encoder serves the five evaluators
            image_encoder = evaluator.image_encoder if evaluator is not None else self._load_image_encoder()
        if self.fid:
            fid = self._fid_evaluator(image_encoder, split_dir)
            fid_real = not fid.is_loaded('real')
        if self.prdc:
            prdc = self._prdc_evaluator(image_encoder)
        if self.kid:
            kid = self._kid_evaluator(image_encoder, prdc)
        if self.nearest:
            nearest = self._nearest_evaluator(image_encoder)
        # who takes the fake rows and who the real ones: FID its moments, PRDC the rows, KID the rows unless PRDC has them
        keeps = [ev for ev in (prdc, kid if prdc is None else None) if ev is not None]
        takes_fake = ([fid] if fid is not None else []) + keeps
        takes_real = ([fid] if fid_real else []) + keeps
        noise = torch.empty(self._noise_shape(self.batch_size), device=self.device)
        made = set()
        for nbatch, data in enumerate(self.data_loader):
            if nbatch % 100 == 0:
                print('step: ', nbatch)
            real_imgs, captions, cap_lens, class_ids, keys = prepare_data(data)
            fake_imgs, sent_emb = self._generate(netG, text_encoder, captions, cap_lens, noise, with_sent=True)
            last = fake_imgs[-1]
            if evaluator is not None:
                evaluator.update(last, sent_emb, class_ids)
            if takes_fake or nearest is not None:       # each batch goes through the trunk once, for all of them
                if evaluator is None:           # (R-precision has otherwise just run this batch through it)
                    image_encoder.pooled_features(last)
                for ev in takes_fake:
                    ev.update_features('fake', image_encoder.last_pooled)
                if nearest is not None:         # (its rows go with their keys)
                    nearest.update_features('fake', image_encoder.last_pooled, keys)
                if takes_real or nearest is not None:   # with cached FID statistics: encoded for the others alone
                    real_feats = image_encoder.pooled_features(real_imgs[-1])
                    for ev in takes_real:
                        ev.update_features('real', real_feats)
                    if nearest is not None:
                        nearest.update_features('real', real_feats)
            if ms_ssim is not None:             # the pixels themselves: no trunk
                ms_ssim.update('fake', last, class_ids)
                ms_ssim.update('real', real_imgs[-1], class_ids)
            if swd is not None:                 # (stores nothing of its own beside an MS-SSIM evaluator)
                swd.update('fake', last)
                swd.update('real', real_imgs[-1])
            for img, key in zip(last, keys):
                self._write_image(img, os.path.join(out_dir, 'single', key) + '_s-1.png', made)
        train_crops = None
        if nearest is not None and not nearest.is_loaded():     # the training split, once, after the generation loop
            from sbagan.nearest import encode_train
            train_crops = self._train_crops()
            rows, train_keys = encode_train(train_crops.dataset, image_encoder.pooled_features, self.batch_size,
                                            train_crops.crop, train_crops.resize, self.device,
                                            getattr(self.data_loader, 'num_workers', 0))
            nearest.update_features('train', rows, train_keys)
        # (attribute stem and file name, evaluator, the printed line, the result fields it shows: a name, or a function
        # of the result)
        reports = (
            ('r_precision', evaluator,
             'R-precision (R = %d, %d images): R@1 %.4f  R@5 %.4f  R@10 %.4f  R@1 over %d splits %.4f +- %.4f',
             ('R', 'n', 'r_at_1', 'r_at_5', 'r_at_10', 'splits', 'r_at_1_splits_mean', 'r_at_1_splits_std')),
            ('fid', fid, 'FID (%d real, %d generated images, %s trunk): %.6g  (mean term %.6g, tr real %.6g, tr fake %.6g)',
             ('n_real', 'n_fake', 'dtype', 'fid', 'mean_term', 'trace_real', 'trace_fake')),
            ('prdc', prdc, 'PRDC (k = %d, %d real, %d generated images, %s trunk): precision %.4f  recall %.4f  '
             'density %.4f  coverage %.4f',
             ('k', 'n_real', 'n_fake', 'dtype', 'precision', 'recall', 'density', 'coverage')),
            ('kid', kid, 'KID (%d subsets of %d, %d real, %d generated images, %s trunk): %.6g +- %.6g',
             ('subsets', 'subset_size', 'n_real', 'n_fake', 'dtype', 'kid', 'kid_std')),
            ('ms_ssim', ms_ssim, 'MS-SSIM (%d same-class pairs of %d images, %d classes, %d skipped, %d px): generated '
             '%.6g +- %.6g  real %.6g +- %.6g',
             ('pairs', 'n_images', 'classes', 'classes_skipped', 'size', 'ms_ssim_fake', 'ms_ssim_fake_std',
              'ms_ssim_real', 'ms_ssim_real_std')),
            ('swd', swd, 'SWD x 1e3 (%d real and %d generated images, %d patches each, %d directions): %s  average %.6g',
             ('n_images', 'n_images', 'patches_per_image', lambda r: r['dir_repeats'] * r['dirs_per_repeat'],
              lambda r: '  '.join('%d px %.6g' % v for v in zip(r['resolutions'], r['swd_x1e3'])), 'swd_avg_x1e3')),
            ('nearest', nearest, 'Nearest training images (K = %d, %d training, %d real, %d generated images, %s trunk, this '
             'project\'s own features): authenticity %.4f (real %.4f)  median distance %s (real %s, ratio %s)  '
             'copies %.4f  distinct training images hit %.4f  most hits on one %d',
             ('k', 'n_train', 'n_real', 'n_fake', 'dtype', 'authenticity', 'authenticity_real',
              lambda r: _figure(r['nn_dist_fake']['median']), lambda r: _figure(r['nn_dist_real']['median']),
              lambda r: _figure(r['nn_ratio']), 'copy_fraction', 'train_hit_distinct', 'train_hit_max')))
        for stem, ev, line, fields in reports:
            if ev is None:
                continue
            setattr(self, stem + '_evaluator', ev)
            res = ev.result()
            setattr(self, stem + '_result', res)
            print(line % tuple(f(res) if callable(f) else res[f] for f in fields))
            with open(os.path.join(out_dir, stem + '.json'), 'w') as f:
                json.dump(res, f, indent=1, sort_keys=True)
            if ev is fid and self.fid_stats and fid_real:
                fid.save_real(self.fid_stats)
                print('Save real FID statistics to:', self.fid_stats)
            if ev is nearest:
                self._nearest_finish(nearest, res, out_dir, train_crops)
        return out_dir

    def gen_example(self, data_dic):
        """trainer.py:435-518: data_dic[key] = [captions (n x Lmax int64, sorted by length), cap_lens, sorted_indices];
        every stage's image per caption, named by the caption's ORIGINAL position; with attention_maps also the
        top-5 word strips 0_s_<index>_a<k>.png."""
        root = self._output_root()
        if root is None:
            return None
        netG, text_encoder = self._load_inference_models()
        for key, (captions, cap_lens, order) in data_dic.items():
            out_dir = os.path.join(root, key)
            print(out_dir)
            mkdir_p(out_dir)
            captions = torch.from_numpy(np.ascontiguousarray(captions)).to(self.device)
            cap_lens = torch.from_numpy(np.ascontiguousarray(cap_lens)).to(self.device)
            noise = torch.empty(self._noise_shape(captions.shape[0]), device=self.device)
            stages, att_maps = self._generate(netG, text_encoder, captions, cap_lens, noise, with_att=True)
            for stage, batch in enumerate(stages):
                for img, src in zip(batch, order):
                    self._write_image(img, os.path.join(out_dir, '0_s_%d_g%d.png' % (int(src), stage)))
            if self.attention_maps:
                self._write_top_words(stages, att_maps, captions, cap_lens, order, out_dir)
        return root
