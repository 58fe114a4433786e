"""Entry point with the reference's command line (AttnGAN2/code/main.py:22-150):

    python main.py --cfg cfg/bird_style.yml --gpu 0 --data_dir ../data/birds [--manualSeed N]

cfg.TRAIN.FLAG: train; otherwise cfg.B_VALIDATION ? sampling(split) : gen_example(example_filenames.txt).
The flags beyond the reference's are this project's additions: miscc/cli.py lists and describes them."""
import os
import sys
import time

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

from datasets import TextDataset, tokenize  # noqa: E402
from miscc import cli, transforms  # noqa: E402
from miscc.config import cfg  # noqa: E402
from sbagan import evaluation, track, truncation  # noqa: E402


def parse_args(argv=None):
    return cli.options('Train a AttnGAN network', 'cfg/bird_attn2.yml', argv, gan=True)


def _encode_sentences(path, wordtoix):
    """word-id lists of the non-empty lines of a text file (words outside the vocabulary are skipped)"""
    with open(path, 'r') as f:
        lines = [ln.replace('\ufffd\ufffd', ' ') for ln in f.read().split('\n') if ln]
    token_lists = [t for t in (tokenize(ln) for ln in lines) if t]
    return [[wordtoix[w] for w in tokens if w in wordtoix] for tokens in token_lists]


def build_example_dic(wordtoix, data_dir=None):
    """The caption batches of gen_example (reference main.py:34-83), from their contract: for every file listed in
    <data_dir>/example_filenames.txt, key = its base name and value = [captions (n x Lmax int64, zero padded, rows by
    DESCENDING length: what the packed bi-LSTM takes), the lengths in that order, the permutation that sorted them]."""
    data_dir = data_dir or cfg.DATA_DIR
    with open(os.path.join(data_dir, 'example_filenames.txt'), 'r') as f:
        listed = [ln for ln in f.read().split('\n') if ln]
    batches = {}
    for name in listed:
        print('Load from:', name)
        ids = _encode_sentences(os.path.join(data_dir, name + '.txt'), wordtoix)
        lengths = np.array([len(s) for s in ids])
        order = np.argsort(lengths)[::-1]
        padded = np.zeros((len(ids), int(lengths.max())), dtype='int64')
        for row, src in enumerate(order):
            padded[row, :lengths[src]] = ids[src]
        batches[os.path.basename(name)] = [padded, lengths[order], order]
    return batches


def gen_example(wordtoix, algo):
    algo.gen_example(build_example_dic(wordtoix))


def main(argv=None, args=None, dataset_cls=TextDataset, make_trainer=None):
    """`args` / `dataset_cls` / `make_trainer` (output_dir, dataloader, n_words, ixtoword -> trainer): the BERT entry
    point (main_bert.py) passes its own; the defaults are this script's."""
    args = parse_args(argv) if args is None else args
    cli.configure(args)
    output_dir = cli.output_dir()
    training = bool(cfg.TRAIN.FLAG)
    split_dir = 'train' if training else 'test'
    imsize = cli.image_size()
    image_transform = transforms.Compose([transforms.Resize(int(imsize * 76 / 64)), transforms.RandomCrop(imsize),
                                          transforms.RandomHorizontalFlip()])
    dataset = dataset_cls(cfg.DATA_DIR, split_dir, base_size=cfg.TREE.BASE_SIZE, transform=image_transform)
    assert dataset
    dataloader = torch.utils.data.DataLoader(dataset, batch_size=cfg.TRAIN.BATCH_SIZE, drop_last=True,
                                             shuffle=True, num_workers=int(cfg.WORKERS))
    if getattr(args, 'device_data', False):
        if training:     # the split cached on the device, batches made there: same batch contract, its own draws
            from sbagan import device_data
            dataloader = device_data.from_cfg(dataset, imsize, args.manualSeed, args.device_data_gb)
        else:
            print('--device_data is ignored outside training')
    print(len(dataloader))
    if make_trainer is None:
        from trainer import condGANTrainer as make_trainer
    algo = make_trainer(output_dir, dataloader, dataset.n_words, dataset.ixtoword)
    algo.fused_inference = bool(getattr(args, 'fused_inference', False))
    algo.attention_maps = bool(getattr(args, 'attention_maps', False))
    for opt in evaluation.OPTIONS:      # the sampling evaluations: one attribute per flag of the table
        if opt.help is not None:
            setattr(algo, opt.name, getattr(args, opt.name, opt.default))
    algo.replay = bool(getattr(args, 'replay', False)) and training
    if getattr(args, 'replay', False) and not training:
        print('--replay is ignored outside training')
    algo.diffaug = getattr(args, 'diffaug', '') if training else ''
    if getattr(args, 'diffaug', '') and not training:
        print('--diffaug is ignored outside training')
    algo.geoaug = getattr(args, 'geoaug', '') if training else ''
    if getattr(args, 'geoaug', '') and not training:
        print('--geoaug is ignored outside training')
    ada_given = getattr(args, 'ada', None) is not None or getattr(args, 'diffaug_p', None) is not None
    if training:
        algo.ada, algo.diffaug_p = getattr(args, 'ada', None), getattr(args, 'diffaug_p', None)
        algo.ada_kimg, algo.ada_interval = getattr(args, 'ada_kimg', 500.0), getattr(args, 'ada_interval', 4)
        algo.ada_pmax = getattr(args, 'ada_pmax', 1.0)
    elif ada_given:
        print('--ada / --diffaug_p are ignored outside training')
    if training:
        algo.track = getattr(args, 'track', 0)
        algo.track_split, algo.track_n = getattr(args, 'track_split', 'test'), getattr(args, 'track_n', 0)
        algo.track_captions, algo.track_best = getattr(args, 'track_captions', 1), getattr(args, 'track_best', None)
        if algo.track and track.not_tracked_line(args):
            print(track.not_tracked_line(args))
    elif getattr(args, 'track', 0):
        print('--track is ignored outside training')
    given = [f for f in ('truncation', 'truncation_sweep') if getattr(args, f, None) is not None]
    if training:
        if given:
            print('%s %s ignored in training' % (' / '.join('--' + f for f in given), 'is' if len(given) == 1 else 'are'))
    else:
        algo.truncation, algo.truncation_n = getattr(args, 'truncation', None), getattr(args, 'truncation_n', 16384)
        algo.truncation_sweep = getattr(args, 'truncation_sweep', None)
        algo.truncation_sweep_n = getattr(args, 'truncation_sweep_n', 0)
        if algo.truncation_sweep and cfg.B_VALIDATION and truncation.not_swept_line(args):
            print(truncation.not_swept_line(args))
    start_t = time.time()
    if training:
        algo.train()
    elif cfg.B_VALIDATION:
        algo.sampling(split_dir)
    else:
        gen_example(dataset.wordtoix, algo)
    print('Total time for training:', time.time() - start_t)


if __name__ == '__main__':
    main()
