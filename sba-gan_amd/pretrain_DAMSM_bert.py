"""DAMSM pre-training with the BERT text side (AttnGAN2/code/pretrain_DAMSM_bert.py):

    python pretrain_DAMSM_bert.py --cfg cfg/DAMSM/bird.yml --gpu 0 [--data_dir ...] [--bert_dir DIR] [--manualSeed N]

pretrain_DAMSM.py's loop with datasets_bert.TextDataset and a BertEncoder: its trunk is frozen but runs in train mode
(dropout), only pooler / fc / conv_text and the image side's two embedding layers train (sbagan.damsm.DAMSMStep's BERT
path).  Checkpoints: Model/text_encoder<N>.pth, Model/image_encoder<N>.pth.  --bert_dir: a local HuggingFace BERT
directory whose config and weights BertEncoder loads (and whose vocab.txt the dataset reads); without it the trunk is
randomly initialised.  --track E and its companions belong to GAN training (main_bert.py): parsed here and ignored."""
import os
import sys

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import pretrain_DAMSM  # noqa: E402
from datasets_bert import TextDataset  # noqa: E402
from miscc import cli  # noqa: E402
from miscc.config import cfg  # noqa: E402
from model_bert import CNN_ENCODER, BertEncoder  # noqa: E402

train, evaluate = pretrain_DAMSM.train, pretrain_DAMSM.evaluate


def parse_args(argv=None):
    return cli.options('Train a DAMSM network', 'cfg/DAMSM/bird.yml', argv, bert=True)


def build_models(n_words, batch_size, bert_dir=None):
    """pretrain_DAMSM_bert.py:166-193 (n_words is unused: the BERT vocabulary is fixed)."""
    text_encoder = BertEncoder(cfg.TEXT.EMBEDDING_DIM, bert_dir=bert_dir)
    image_encoder = CNN_ENCODER(cfg.TEXT.EMBEDDING_DIM)
    labels = torch.arange(batch_size, dtype=torch.int64)
    start_epoch = 0
    if cfg.TRAIN.NET_E != '':
        text_encoder.load_state_dict(torch.load(cfg.TRAIN.NET_E, map_location='cpu'))
        print('Load ', cfg.TRAIN.NET_E)
        name = cfg.TRAIN.NET_E.replace('text_encoder', 'image_encoder')
        image_encoder.load_state_dict(torch.load(name, map_location='cpu'))
        print('Load ', name)
        start_epoch = cli.epoch_of(cfg.TRAIN.NET_E) + 1
        print('start_epoch', start_epoch)
    dev = torch.device('cuda', cfg.GPU_ID)
    return text_encoder.to(dev), image_encoder.to(dev), labels.to(dev), start_epoch


def main(argv=None, max_steps=None):
    args = parse_args(argv)

    def dataset(*a, **kw):
        return TextDataset(*a, bert_dir=args.bert_dir, **kw)

    def build(n_words, batch_size):
        return build_models(n_words, batch_size, bert_dir=args.bert_dir)

    return pretrain_DAMSM.main(max_steps=max_steps, args=args, dataset_cls=dataset, build=build)


if __name__ == '__main__':
    main()
