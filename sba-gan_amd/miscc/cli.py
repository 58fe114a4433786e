"""What the two entry points (main.py, pretrain_DAMSM.py) share, written from their command-line contract:

    --cfg FILE  --gpu ID  --data_dir DIR  --manualSeed N  [--fused_inference]  [--r_precision R]  [--attention_maps]  [--fid]  [--fid_stats PATH]  [--prdc K]
    [--kid]  [--kid_subsets N]  [--kid_subset_size M]  [--ms_ssim N]  [--swd N]
    [--nearest K]  [--nearest_stats PATH]  [--nearest_show M]
    [--device_data]  [--device_data_gb G]  [--replay]  [--diffaug POLICY]
    [--retrieval E]  [--retrieval_only: DAMSM pre-training]
    [--bert_dir DIR: the BERT entry points]

the yml file is merged into miscc.config.cfg, --gpu / --data_dir override it, the seed is 100 outside training (the
reference's evaluation runs are seeded that way), the given one or a random one in training, and every run gets an
output directory ../output/<DATASET>_<CONFIG>_<timestamp>."""
import argparse
import datetime
import pprint
import random
import re

import numpy as np
import torch

from .config import cfg, cfg_from_file

EVAL_SEED = 100


def _r_precision(text):
    r = int(text)
    if r < 0 or r == 1:
        raise argparse.ArgumentTypeError('R must be 0 (off) or at least 2 candidates per image')
    return r


def _prdc(text):
    k = int(text)
    if k < 0 or k > 8:
        raise argparse.ArgumentTypeError('K must be 0 (off) or a neighbour count from 1 to 8')
    return k


def _kid_subsets(text):
    n = int(text)
    if n < 1 or n > 1024:
        raise argparse.ArgumentTypeError('N must be a subset count from 1 to 1024')
    return n


def _kid_subset_size(text):
    m = int(text)
    if m < 2:
        raise argparse.ArgumentTypeError('M must be at least 2 rows a side')
    return m


def _ms_ssim(text):
    n = int(text)
    if n < 0:
        raise argparse.ArgumentTypeError('N must be 0 (off) or a number of pairs per class')
    return n


def _swd(text):
    n = int(text)
    if n < 0:
        raise argparse.ArgumentTypeError('N must be 0 (off) or a number of images per side')
    return n


def _nearest(text):
    k = int(text)
    if k < 0 or k > 8:
        raise argparse.ArgumentTypeError('K must be 0 (off) or a neighbour count from 1 to 8')
    return k


def _nearest_show(text):
    m = int(text)
    if m < 0:
        raise argparse.ArgumentTypeError('M must be 0 (no picture) or a number of generated images')
    return m


DIFFAUG_POLICIES = ('color', 'translation', 'cutout')


def _diffaug(text):
    names = [n.strip() for n in text.split(',')] if text else []
    for n in names:
        if n not in DIFFAUG_POLICIES:
            raise argparse.ArgumentTypeError('unknown policy %r; valid names are %s (comma separated)'
                                             % (n, ', '.join(DIFFAUG_POLICIES)))
    return ','.join(names)


def _retrieval(text):
    e = int(text)
    if e < 0:
        raise argparse.ArgumentTypeError('E must be 0 (off) or an interval in epochs')
    return e


def options(what, default_cfg, argv=None, bert=False):
    ap = argparse.ArgumentParser(description=what)
    ap.add_argument('--cfg', dest='cfg_file', type=str, default=default_cfg, help='optional config file')
    ap.add_argument('--gpu', dest='gpu_id', type=int, default=0)
    ap.add_argument('--data_dir', dest='data_dir', type=str, default='')
    ap.add_argument('--manualSeed', type=int, help='manual seed')
    ap.add_argument('--fused_inference', dest='fused_inference', action='store_true', default=False,
                    help='sampling / gen_example: run the generator through sbagan.infer.FusedGenerator (BatchNorm '
                         'folded into the convs, GLU in the conv epilogue)')
    ap.add_argument('--r_precision', dest='r_precision', type=_r_precision, default=0, metavar='R',
                    help='sampling: also rank every generated image among R candidate captions (its own and R - 1 of '
                         'other classes) with the DAMSM encoders and write r_precision.json; 0 = off, 100 = the '
                         'AttnGAN paper\'s setting')
    ap.add_argument('--attention_maps', dest='attention_maps', action='store_true', default=False,
                    help='write the attention-map overlays (sbagan.visualize): Image/G_*.png and D_*.png in training, '
                         '<key>/0_s_<i>_a<k>.png from gen_example, Image/attention_maps<step>.png in DAMSM '
                         'pre-training')
    ap.add_argument('--fid', dest='fid', action='store_true', default=False,
                    help='sampling: also take the Frechet Inception Distance between the real images of the split and '
                         'the generated ones on the DAMSM image encoder\'s Inception-v3 trunk (sbagan.fid) and write '
                         'fid.json')
    ap.add_argument('--fid_stats', dest='fid_stats', type=str, default=None, metavar='PATH',
                    help='with --fid: an .npz of the real images\' statistics; read instead of the real pass when it '
                         'exists, written after the run when it does not')
    ap.add_argument('--prdc', dest='prdc', type=_prdc, default=0, metavar='K',
                    help='sampling: also take precision, recall, density and coverage (the K-nearest-neighbour manifold '
                         'metrics, sbagan.prdc) between the real images of the split and the generated ones on the same '
                         'trunk features as --fid and write prdc.json; 0 = off, K from 1 to 8, 5 = the usual setting.  '
                         'On this project\'s own trunk and compute dtype: not comparable with published numbers')
    ap.add_argument('--kid', dest='kid', action='store_true', default=False,
                    help='sampling: also take the Kernel Inception Distance (the unbiased MMD^2 estimate under the '
                         'kernel (x.y / D + 1)^3 with its standard deviation over subsets, sbagan.kid) between the real '
                         'images of the split and the generated ones on the same trunk features as --fid and write '
                         'kid.json.  On this project\'s own trunk and compute dtype: not comparable with published '
                         'numbers')
    ap.add_argument('--kid_subsets', dest='kid_subsets', type=_kid_subsets, default=100, metavar='N',
                    help='with --kid: the number of subsets, 1 to 1024')
    ap.add_argument('--kid_subset_size', dest='kid_subset_size', type=_kid_subset_size, default=1000, metavar='M',
                    help='with --kid: rows per subset and side (at least 2); clamped to the smaller side')
    ap.add_argument('--ms_ssim', dest='ms_ssim', type=_ms_ssim, default=0, metavar='N',
                    help='sampling: also take the mean multi-scale structural similarity (MS-SSIM, the within-class '
                         'diversity measure of the AC-GAN paper, sbagan.msssim) over N random pairs of images per class, '
                         'for the generated images and for the real images of the same pairs, and write ms_ssim.json; '
                         '0 = off, 100 = the AC-GAN setting.  In pixel space on the written uint8 images: it uses no '
                         'trunk; images of at least 176 px')
    ap.add_argument('--swd', dest='swd', type=_swd, default=0, metavar='N',
                    help='sampling: also take the sliced Wasserstein distance (SWD, Karras et al. 2018, sbagan.swd) between '
                         'the first N real and the first N generated images, per level of a Laplacian pyramid and on '
                         'average, x 1e3, and write swd.json; 0 = off, 16384 = the setting of the paper.  In pixel '
                         'space on the written uint8 images: it uses no trunk; square images of 32, 64, 128 or 256 px')
    ap.add_argument('--nearest', dest='nearest', type=_nearest, default=0, metavar='K',
                    help='sampling: also list the K nearest TRAINING images of every generated image on the same trunk '
                         'features as --fid (float64 distances on the matrix cores, sbagan.nearest) and take the '
                         'memorisation figures the other evaluations cannot see: authenticity (Alaa et al. 2022) with its '
                         'baseline on the split\'s real images, the nearest-training-image distance of generated against '
                         'unseen real images, the share of near-copies and how many distinct training images are hit; '
                         'writes nearest.json and nearest.png; 0 = off, K from 1 to 8.  The training split is encoded '
                         'once after the generation loop.  On this project\'s own trunk and compute dtype: not '
                         'comparable with published numbers.  Ignored by the DAMSM entry points and in training')
    ap.add_argument('--nearest_stats', dest='nearest_stats', type=str, default=None, metavar='PATH',
                    help='with --nearest: an .npz of the training images\' feature rows and keys; read instead of the '
                         'training pass when it exists, written after the run when it does not')
    ap.add_argument('--nearest_show', dest='nearest_show', type=_nearest_show, default=16, metavar='M',
                    help='with --nearest: the M generated images closest to a training image are listed in nearest.json '
                         'and shown in nearest.png, one row each beside their K training images; 0 = no picture')
    ap.add_argument('--device_data', dest='device_data', action='store_true', default=False,
                    help='training: decode the split once into a device-resident uint8 cache and make every batch '
                         'there -- crop, flip, every scale of the pyramid and the normalisation in one HIP launch '
                         '(sbagan.device_data), bit-identical to the PIL path for the same draws; the draws come from '
                         'the loader\'s own generator, seeded by --manualSeed')
    ap.add_argument('--device_data_gb', dest='device_data_gb', type=float, default=64.0, metavar='G',
                    help='with --device_data: refuse a split whose cache would need more than G GiB')
    ap.add_argument('--replay', dest='replay', action='store_true', default=False,
                    help='GAN training: run every batch through ONE recording of the training step, re-issued by the '
                         'native launch replayer from a static batch slot (sbagan.static_batch) -- the step at the '
                         'benchmarked speed; best with --device_data.  The step draws its own noise, so a seeded run '
                         'differs from one without the flag.  DAMSM pre-training (pretrain_DAMSM.py): the whole update '
                         '-- both encoders\' trainable parts, the gradient clip and Adam -- is one recording '
                         '(sbagan.damsm.DAMSMSlotStep), the dropout mask is drawn per batch outside it and the losses '
                         'are read only where the interval line is printed.  Ignored by pretrain_DAMSM_bert.py and '
                         'outside training')
    ap.add_argument('--diffaug', dest='diffaug', type=_diffaug, default='', metavar='POLICY',
                    help='GAN training: Differentiable Augmentation (Zhao et al., NeurIPS 2020) of every image a '
                         'discriminator sees -- real and fake images in the discriminator updates, fake images in the '
                         'generator\'s adversarial terms, each with its own random draws, gradients flowing through to '
                         'the generator (sbagan.diffaug, one fused HIP pass in place of the step\'s concatenation).  '
                         'POLICY: a comma-separated subset of color,translation,cutout; empty = off.  The DAMSM terms, '
                         'sampling, the image dumps and checkpoints see un-augmented images.  Single GPU only.  Ignored '
                         'outside training and by the DAMSM pre-training entry points')
    ap.add_argument('--retrieval', dest='retrieval', type=_retrieval, default=0, metavar='E',
                    help='DAMSM pre-training: after the validation pass of every E-th epoch and of the last one, rank '
                         'every image of the validation split against every caption and every caption against every '
                         'image with the two encoders (sbagan.retrieval: float64 cosine scores on the matrix cores, the '
                         'score matrix never written), print R@1 / R@5 / R@10 and the median rank for both directions, '
                         'instance-level and class-masked, and append them to Model/retrieval.jsonl; 0 = off.  It draws '
                         'no random numbers and leaves the training untouched.  Ignored by main.py and main_bert.py')
    ap.add_argument('--retrieval_only', dest='retrieval_only', action='store_true', default=False,
                    help='DAMSM pre-training: load the encoder pair of TRAIN.NET_E, rank the validation split once, '
                         'print the figures, write retrieval.json and return without training')
    if bert:        # the BERT entry points (pretrain_DAMSM_bert.py, main_bert.py)
        ap.add_argument('--bert_dir', dest='bert_dir', type=str, default=None,
                        help='local HuggingFace BERT directory (config, weights, vocab.txt); default: random trunk')
    return ap.parse_args(argv)


def configure(args):
    """merge the yml file and the command-line overrides into cfg, seed every generator; returns the seed"""
    if args.cfg_file:
        cfg_from_file(args.cfg_file)
    if args.gpu_id < 0:
        raise RuntimeError('--gpu -1 (CPU): the HIP modules have no CPU path; the CPU restatement of the step is the '
                           'test oracle (oracle/), not a product path')
    cfg.GPU_ID = args.gpu_id
    if args.data_dir:
        cfg.DATA_DIR = args.data_dir
    print('Using config:')
    pprint.pprint(cfg)
    seed = args.manualSeed
    if not cfg.TRAIN.FLAG:
        seed = EVAL_SEED
    elif seed is None:
        seed = random.randint(1, 10000)
    args.manualSeed = seed
    for seeder in (random.seed, np.random.seed, torch.manual_seed, torch.cuda.manual_seed_all):
        seeder(seed)
    return seed


def output_dir():
    stamp = datetime.datetime.now().strftime('%Y_%m_%d_%H_%M_%S')
    return '../output/%s_%s_%s' % (cfg.DATASET_NAME, cfg.CONFIG_NAME, stamp)


def image_size():
    """side of the largest generated image: BASE_SIZE doubled per extra stage"""
    return cfg.TREE.BASE_SIZE << (cfg.TREE.BRANCH_NUM - 1)


def epoch_of(checkpoint_path):
    """the epoch number at the end of a checkpoint's file name (text_encoder200.pth, netG_epoch_600.pth), or None"""
    m = re.search(r'(\d+)\.[^./\\]+$', checkpoint_path)
    return int(m.group(1)) if m else None
