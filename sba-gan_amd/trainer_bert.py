"""condGANTrainer of the BERT path (AttnGAN2/code/trainer_bert.py): trainer.condGANTrainer with the frozen
BertEncoder as the text side and model_bert's generators.

What differs from trainer.condGANTrainer:
  * the text encoder is a frozen eval-mode BertEncoder (`bert_dir`: a local HuggingFace directory with its config and
    weights; without it the trunk is randomly initialised), fed `text_encoder(captions)` -- the HIP forward of
    sbagan.bert_hip -- with mask = (captions == 0) cut to the length of words_embs;
  * the generator is model_bert.G_NET; with cfg.TRAIN.MIXING the noise is 2 x B x nz and the generator is
    model_bert.G_NET_MIX.  This deviates from the reference on purpose: it builds G_NET there, which cannot take that
    noise;
  * gen_example writes the reference's style-mixing set (trainer_bert.py:440-566): per caption and stage
    `0_s_<idx>_g<k>_AB.png` (G_NET_MIX on (z1, z2)), `_BA.png` (the halves swapped), `_A.png` (G_NET on z1) and
    `_B.png` (G_NET on z2), G_NET and G_NET_MIX loaded from the same checkpoint.
"""
import os

import numpy as np
import torch

import trainer
from miscc.config import cfg
from miscc.utils import mkdir_p, weights_init
from model_bert import G_NET, G_NET_MIX, BertEncoder


class condGANTrainer(trainer.condGANTrainer):
    def __init__(self, output_dir, data_loader, n_words, ixtoword, allow_random_encoders=False, bert_dir=None):
        super(condGANTrainer, self).__init__(output_dir, data_loader, n_words, ixtoword,
                                             allow_random_encoders=allow_random_encoders)
        self.bert_dir = bert_dir

    def _generator(self):
        if cfg.GAN.B_DCGAN:
            raise NotImplementedError('G_DCGAN is dead code in the reference (SURVEY.md 2): not built')
        return G_NET_MIX() if cfg.TRAIN.MIXING else G_NET()

    def _text_encoder(self):
        return BertEncoder(cfg.TEXT.EMBEDDING_DIM, bert_dir=self.bert_dir)

    def _noise_shape(self, n):
        return (2, n, cfg.GAN.Z_DIM) if cfg.TRAIN.MIXING else (n, cfg.GAN.Z_DIM)

    def _encode(self, text_encoder, captions, cap_lens, out=None):
        with torch.no_grad():
            words_embs, sent_emb = text_encoder(captions)
        if out is not None:         # the static-output form of the recorded loop (--replay)
            out[0].copy_(words_embs)
            out[1].copy_(sent_emb)
            return out
        return words_embs.detach(), sent_emb.detach()

    def gen_example(self, data_dic):
        """trainer_bert.py:440-566; with attention_maps also the top-5 word strips 0_s_<idx>_a<k>_<set>.png; with
        truncation_sweep also the psi strips 0_s_<idx>_psi.png of G_NET on z1 (the 'A' set)."""
        root = self._output_root()
        if root is None:
            return None
        dev = self.device
        text_encoder = self._text_encoder()
        if cfg.TRAIN.NET_E != '':
            text_encoder.load_state_dict(torch.load(cfg.TRAIN.NET_E, map_location='cpu'))
            print('Load text encoder from:', cfg.TRAIN.NET_E)
        elif not self.allow_random_encoders:
            raise RuntimeError('cfg.TRAIN.NET_E is empty: no text encoder to load')
        text_encoder = text_encoder.to(dev).eval()
        state = torch.load(cfg.TRAIN.NET_G, map_location='cpu')
        nets = []
        for net in (G_NET(), G_NET_MIX()):
            net.apply(weights_init)
            net.load_state_dict(state)
            nets.append(self._inference_generator(net.to(dev).eval()))
        netG, netG_mix = nets
        print('Load G from: ', cfg.TRAIN.NET_G)
        self._set_truncation(netG, netG_mix)
        for key, (captions, cap_lens, order) in data_dic.items():
            out_dir = os.path.join(root, key)
            print(out_dir)
            mkdir_p(out_dir)
            captions = torch.from_numpy(np.ascontiguousarray(captions)).to(dev)
            cap_lens = torch.from_numpy(np.ascontiguousarray(cap_lens)).to(dev)
            words_embs, sent_emb = self._encode(text_encoder, captions, cap_lens)
            mask = trainer.build_mask(captions, words_embs.size(2))
            noise = torch.empty((2, captions.shape[0], cfg.GAN.Z_DIM), device=dev)
            noise.normal_(0, 1)
            swapped = torch.cat([noise[1:], noise[:1]], 0)
            # (with truncation_sweep the 'A' call keeps its inputs, its eps among them, for the psi strips: the same draws)
            kept = {'sent_emb': sent_emb, 'words_embs': words_embs, 'mask': mask} if self.truncation_sweep else None
            with torch.no_grad():
                outs = {'AB': netG_mix(noise, sent_emb, words_embs, mask)[:2],
                        'BA': netG_mix(swapped, sent_emb, words_embs, mask)[:2]}
                outs['A'] = (netG(noise[0], sent_emb, words_embs, mask)[:2] if kept is None
                             else self._forward_kept(netG, noise[0], kept))
                outs['B'] = netG(noise[1], sent_emb, words_embs, mask)[:2]
            for tag in ('AB', 'BA', 'A', 'B'):
                stages, att_maps = outs[tag]
                for stage, batch in enumerate(stages):
                    for img, src in zip(batch, order):
                        self._write_image(img, os.path.join(out_dir, '0_s_%d_g%d_%s.png' % (int(src), stage, tag)))
                if self.attention_maps:
                    self._write_top_words(stages, att_maps, captions, cap_lens, order, out_dir, suffix='_' + tag)
            if self.truncation_sweep:       # from the plain G_NET on noise[0]: the 'A' set's inputs
                self._write_psi_strips(netG, noise[0], kept, order, out_dir)
        return root
