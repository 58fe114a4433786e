"""What the two entry points (main.py, pretrain_DAMSM.py) share, written from their command-line contract:

    --cfg FILE  --gpu ID  --data_dir DIR  --manualSeed N  [--fused_inference]  [--r_precision R]  [--attention_maps]  [--fid]  [--fid_stats PATH]  [--prdc K]
    [--kid]  [--kid_subsets N]  [--kid_subset_size M]  [--ms_ssim N]  [--swd N]
    [--nearest K]  [--nearest_stats PATH]  [--nearest_show M]
    [--device_data]  [--device_data_gb G]  [--replay]  [--diffaug POLICY]
    [--diffaug_p P]  [--ada TARGET]  [--ada_kimg K]  [--ada_interval N]  [--ada_pmax P]
    [--geoaug POLICY: flip,rot90,scale,rotate in front of the discriminators]
    [--track E]  [--track_split NAME]  [--track_n N]  [--track_captions C]  [--track_best KEY: GAN training]
    [--truncation PSI[,PSI]]  [--truncation_n N]  [--truncation_sweep LIST]  [--truncation_sweep_n N: sampling / gen_example]
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

from sbagan import evaluation, track, truncation

from .config import cfg, cfg_from_file

EVAL_SEED = 100


def _ranged_int(metavar, lo, hi, what, also=None):
    """the argparse type of an integer in [lo, hi] (hi None: unbounded) or equal to `also`"""
    def parse(text):
        v = int(text)
        if v != also and (v < lo or (hi is not None and v > hi)):
            raise argparse.ArgumentTypeError('%s must be %s' % (metavar, what))
        return v
    return parse


def _add_evaluator(ap, record):
    """the flags of one record of sbagan.evaluation's table: a switch, a path or a ranged integer each"""
    for opt in record.options:
        if opt.help is None:        # (an attribute of the trainer alone)
            continue
        kind = dict(action='store_true') if opt.metavar is None else dict(type=str, metavar=opt.metavar)
        if opt.lo is not None:
            kind['type'] = _ranged_int(opt.metavar, opt.lo, opt.hi, opt.cli_what or opt.what, also=opt.default)
        ap.add_argument('--' + opt.name, dest=opt.name, default=opt.default, help=opt.help, **kind)


DIFFAUG_POLICIES = ('color', 'translation', 'cutout')


def _diffaug(text):
    names = [n.strip() for n in text.split(',')] if text else []
    for n in names:
        if n not in DIFFAUG_POLICIES:
            raise argparse.ArgumentTypeError('unknown policy %r; valid names are %s (comma separated)'
                                             % (n, ', '.join(DIFFAUG_POLICIES)))
    return ','.join(names)


GEOAUG_POLICIES = ('flip', 'rot90', 'scale', 'rotate')


def _geoaug(text):
    names = [n.strip() for n in text.split(',')] if text else []
    for n in names:
        if n not in GEOAUG_POLICIES:
            raise argparse.ArgumentTypeError('unknown policy %r; valid names are %s (comma separated)'
                                             % (n, ', '.join(GEOAUG_POLICIES)))
    return ','.join(names)


def _ranged_float(metavar, lo, hi, what, open_ends=False):
    """the argparse type of a float in [lo, hi] ((lo, hi) with open_ends; hi None: unbounded above)"""
    def parse(text):
        v = float(text)
        inside = (lo < v if open_ends else lo <= v) and (hi is None or (v < hi if open_ends else v <= hi))
        if not inside:          # (a NaN fails both comparisons)
            raise argparse.ArgumentTypeError('%s must be %s' % (metavar, what))
        return v
    return parse


def _track_key(text):
    if text not in track.BEST_KEYS:
        raise argparse.ArgumentTypeError('unknown key %r; valid keys are %s' % (text, ', '.join(track.BEST_KEYS)))
    return text


def options(what, default_cfg, argv=None, bert=False, gan=False):
    """gan: the entry point trains the GAN (main.py, main_bert.py) -- the only ones --track means something to, so the
    only ones that refuse a --track that would measure nothing"""
    ap = argparse.ArgumentParser(description=what)
    ap.add_argument('--cfg', dest='cfg_file', type=str, default=default_cfg, help='optional config file')
    ap.add_argument('--gpu', dest='gpu_id', type=int, default=0)
    ap.add_argument('--data_dir', dest='data_dir', type=str, default='')
    ap.add_argument('--manualSeed', type=int, help='manual seed')
    ap.add_argument('--fused_inference', dest='fused_inference', action='store_true', default=False,
                    help='sampling / gen_example: run the generator through sbagan.infer.FusedGenerator (BatchNorm '
                         'folded into the convs, GLU in the conv epilogue)')
    _add_evaluator(ap, evaluation.EVALUATORS[0])
    ap.add_argument('--attention_maps', dest='attention_maps', action='store_true', default=False,
                    help='write the attention-map overlays (sbagan.visualize): Image/G_*.png and D_*.png in training, '
                         '<key>/0_s_<i>_a<k>.png from gen_example, Image/attention_maps<step>.png in DAMSM '
                         'pre-training')
    for record in evaluation.EVALUATORS[1:]:
        _add_evaluator(ap, record)
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
    ap.add_argument('--diffaug_p', dest='diffaug_p', default=None, metavar='P',
                    type=_ranged_float('P', 0.0, 1.0, 'a probability in [0, 1]'),
                    help='with --diffaug: apply each part of the policy to an image with probability P instead of '
                         'always (the gated HIP kernels; P lives in device memory, one value per discriminator).  '
                         'Without --ada P stays fixed -- the fixed-p ablation of Karras et al. -- and no controller '
                         'launch is issued; with --ada it is the initial value (default then: 0).  Default: the '
                         'ungated kernels')
    ap.add_argument('--ada', dest='ada', default=None, metavar='TARGET',
                    type=_ranged_float('TARGET', -1.0, 1.0, 'in (-1, 1)', open_ends=True),
                    help='with --diffaug: adaptive augmentation strength (Karras et al., NeurIPS 2020, "Training GANs '
                         'with Limited Data").  Per discriminator, the overfitting read-out r_t = E[sign(D(real))] is '
                         'counted on the device behind every update, and every --ada_interval iterations p moves one '
                         'step towards r_t = TARGET (0.6 in the paper).  Counting, the controller and p itself stay '
                         'on the device, so --replay records them with the step.  Every 100 iterations one line shows '
                         'p and r_t per discriminator; the same goes to Model/ada.jsonl, the state to '
                         'Model/ada_state.pth (restored on resume).  Default: off')
    ap.add_argument('--ada_kimg', dest='ada_kimg', default=500.0, metavar='K',
                    type=_ranged_float('K', 0.0, None, 'positive', open_ends=True),
                    help='with --ada: p can travel from 0 to 1 in K thousand real images (default 500)')
    ap.add_argument('--ada_interval', dest='ada_interval', default=4, metavar='N',
                    type=_ranged_int('N', 1, 1024, 'an interval of 1 to 1024 iterations'),
                    help='with --ada: iterations between two controller updates (default 4)')
    ap.add_argument('--ada_pmax', dest='ada_pmax', default=1.0, metavar='P',
                    type=_ranged_float('P', 0.0, 1.0, 'a probability in [0, 1]'),
                    help='with --ada: the largest p the controller sets (default 1.0)')
    ap.add_argument('--geoaug', dest='geoaug', type=_geoaug, default='', metavar='POLICY',
                    help='GAN training: geometric augmentation (Karras et al., NeurIPS 2020) of every image a '
                         'discriminator sees, real and fake, gradients flowing through to the generator: per image one '
                         'affine warp about the centre, bilinear, zero padded (sbagan.geoaug, one HIP pass in place of '
                         'the step\'s concatenation).  POLICY: a comma-separated subset of flip,rot90,scale,rotate; '
                         'empty = off.  With --diffaug it runs first, then colour, translation and cutout; with '
                         '--diffaug_p / --ada each part is applied with the same per-discriminator probability p.  '
                         'Single GPU only.  Ignored outside training and by the DAMSM pre-training entry points')
    ap.add_argument('--retrieval', dest='retrieval', default=0, metavar='E',
                    type=_ranged_int('E', 0, None, '0 (off) or an interval in epochs'),
                    help='DAMSM pre-training: after the validation pass of every E-th epoch and of the last one, rank '
                         'every image of the validation split against every caption and every caption against every '
                         'image with the two encoders (sbagan.retrieval: float64 cosine scores on the matrix cores, the '
                         'score matrix never written), print R@1 / R@5 / R@10 and the median rank for both directions, '
                         'instance-level and class-masked, and append them to Model/retrieval.jsonl; 0 = off.  It draws '
                         'no random numbers and leaves the training untouched.  Ignored by main.py and main_bert.py')
    ap.add_argument('--retrieval_only', dest='retrieval_only', action='store_true', default=False,
                    help='DAMSM pre-training: load the encoder pair of TRAIN.NET_E, rank the validation split once, '
                         'print the figures, write retrieval.json and return without training')
    ap.add_argument('--track', dest='track', default=0, metavar='E',
                    type=_ranged_int('E', 0, None, '0 (off) or an interval in epochs'),
                    help='GAN training: at the end of every epoch with epoch %% E == 0 and once more after the final '
                         'checkpoint, evaluate the EMA generator -- the weights save_model would write at that moment -- '
                         'on a held-out split (sbagan.track): the figures of those of --fid, --kid, --prdc and '
                         '--r_precision that are on (at least one must be), over a frozen set of captions, noise and '
                         'real-image rows, one printed line and one JSON line in Model/track.jsonl per evaluation, no '
                         'image written; 0 = off.  It draws from no global generator and leaves the training untouched, '
                         'with --replay too.  On this project\'s own trunk and compute dtype: comparable between epochs '
                         'and runs of this project only.  Ignored outside training and by the DAMSM entry points')
    ap.add_argument('--track_split', dest='track_split', type=str, default='test', metavar='NAME',
                    help='with --track: the held-out split (default test)')
    ap.add_argument('--track_n', dest='track_n', default=0, metavar='N',
                    type=_ranged_int('N', 0, None, '0 (the whole split) or a number of images'),
                    help='with --track: the first N images of the split in the data set\'s own order; 0 = all of them')
    ap.add_argument('--track_captions', dest='track_captions', default=1, metavar='C',
                    type=_ranged_int('C', 1, None, 'a number of captions per image, at least 1'),
                    help='with --track: captions 0 .. C - 1 of every image, 1 to TEXT.CAPTIONS_PER_IMAGE (default 1)')
    ap.add_argument('--track_best', dest='track_best', default=None, metavar='KEY', type=_track_key,
                    help='with --track: whenever an evaluation improves on the best KEY so far, write '
                         'Model/netG_best.pth (the bytes of that epoch\'s checkpoint) and Model/best.json; KEY one of '
                         + ', '.join(track.BEST_KEYS) + '.  On resume a best.json beside TRAIN.NET_G is honoured')
    ap.add_argument('--truncation', dest='truncation', default=None, metavar='PSI[,PSI]', type=truncation.parse_psi,
                    help='sampling / gen_example: the truncation trick in W (sbagan.truncation) -- every style the later '
                         'stages read is pulled towards the mean style, w_avg + PSI (w - w_avg), PSI in [0, 1]: 1 is the '
                         'generator as trained (bit for bit the run without the flag), 0 the mean style; a pair sets '
                         'stage 2 and stage 3 apart (BRANCH_NUM 3).  w_avg is the mean of the checkpoint\'s own mapping '
                         'network over --truncation_n codes from a generator of its own, summed in a fixed float64 order '
                         '(HIP).  The PNGs, every evaluator that is on and the attention maps see the truncated images; '
                         'sampling writes truncation.json.  model.G_NET also feeds z to its first stage: its 64 px '
                         'image does not move.  Default: off.  Ignored in training and by the DAMSM entry points')
    ap.add_argument('--truncation_n', dest='truncation_n', default=truncation.DEFAULT_N, metavar='N',
                    type=_ranged_int('N', 1, truncation.MAX_N, 'a number of codes from 1 to %d' % truncation.MAX_N),
                    help='with --truncation / --truncation_sweep: codes in the mean style (default %d)'
                         % truncation.DEFAULT_N)
    ap.add_argument('--truncation_sweep', dest='truncation_sweep', default=None, metavar='LIST',
                    type=truncation.parse_sweep,
                    help='sampling: after the normal run has written its files, evaluate the generator at every psi of '
                         'the comma-separated LIST (each in [0, 1], none twice) over ONE frozen set of the sampled split '
                         '-- the same captions, noise and eps for every psi, the real images through the trunk once -- '
                         'with those of --fid, --kid, --prdc and --r_precision that are on (at least one must be): one '
                         'line per psi, truncation_sweep.json, no image written.  With or without --truncation.  '
                         'gen_example: also write <key>/0_s_<idx>_psi.png, the last stage at every psi of LIST over one '
                         'noise draw.  On this project\'s own trunk and compute dtype: comparable between runs of this '
                         'project only')
    ap.add_argument('--truncation_sweep_n', dest='truncation_sweep_n', default=0, metavar='N',
                    type=_ranged_int('N', 0, None, '0 (the whole split) or a number of images'),
                    help='with --truncation_sweep: the first N images of the split, caption 0 of each; 0 = all of them')
    if bert:        # the BERT entry points (pretrain_DAMSM_bert.py, main_bert.py)
        ap.add_argument('--bert_dir', dest='bert_dir', type=str, default=None,
                        help='local HuggingFace BERT directory (config, weights, vocab.txt); default: random trunk')
    args = ap.parse_args(argv)
    for flag in ('ada', 'diffaug_p'):
        if getattr(args, flag) is not None and not args.diffaug:
            ap.error('--%s needs a non-empty --diffaug POLICY' % flag)
    if args.ada is not None and args.diffaug_p is not None and args.diffaug_p > args.ada_pmax:
        ap.error('--diffaug_p %g is above --ada_pmax %g' % (args.diffaug_p, args.ada_pmax))
    problem = truncation.check_flags(args) if gan else None
    if problem:
        ap.error(problem)
    if args.track and gan:
        problem = track.check_flags(args)
        if problem:
            ap.error(problem)
    return args


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
