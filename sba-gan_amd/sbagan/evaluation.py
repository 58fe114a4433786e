"""The evaluations sampling() can take beside the images it writes: one ordered table (EVALUATORS) with a record per
evaluator, and the Suite that builds the ones that are on, routes every batch to them and reports.

The table is what the command line (miscc.cli.options), the trainer's attributes (trainer.condGANTrainer), main.py's
argument copy and the sampling loop are generated from; an evaluator is one record here and its class in its own module.
Host code only: nothing here launches a kernel, and importing it loads no device library (miscc.cli imports it)."""
import collections
import json
import os

from miscc.config import cfg

# one option of an evaluator: a trainer attribute `name` with `default`; with `help` also the command-line flag --name.
# metavar None: a switch; lo None: a path; otherwise an integer in [lo, hi] (hi None: unbounded) -- `what` completes
# "<name> must be ..." where the suite refuses a value, `cli_what` (default: what) "<metavar> must be ..." where the
# parser does.  The parser also takes the default itself (0 = off).
Option = collections.namedtuple('Option', 'name default metavar lo hi what cli_what help')
Option.__new__.__defaults__ = (None,) * 6

# stem: the attribute prefix (<stem>_evaluator, <stem>_result) and the <stem>.json name; options[0] switches it on
# build(suite, text_encoder) -> the evaluator object
# consumes: 'ranking' (update(fake images, sentence embeddings, class ids), through the trunk on its own), 'rows'
#   (update_features(side, pooled trunk rows)) or 'images' (update(side, images)); extra: what goes with them -- 'keys'
#   with the fake rows, 'class_ids' with the images of both sides
# line, fields: the printed report and the result fields it shows (a name, or a function of the result)
# shares: (stem, fed) -- built on that evaluator's store when it is on, and then still fed its batches or not
# real_cached(evaluator): true when it needs no real rows (read from a file instead)
# finish(suite, evaluator, result, out_dir): what follows the report
Evaluator = collections.namedtuple('Evaluator', 'stem options build consumes line fields extra shares real_cached finish')
Evaluator.__new__.__defaults__ = (None,) * 4

MAX_K = 8       # neighbour counts: ops.PRDC_MAX_K and ops.KNN_MAX_K (held equal by tests/test_evaluation_cpu.py)


def _int_option(name, value, lo, hi, what):
    if isinstance(value, bool) or not isinstance(value, int) or value < lo or (hi is not None and value > hi):
        raise ValueError('%s must be %s (got %r)' % (name, what, value))
    return value


def _figure(value):
    """a figure that may be missing (sbagan.nearest reports None where no row has a neighbour)"""
    return 'n/a' if value is None else '%.6g' % value


# ------------------------------------------------------------------ builders
def _build_r_precision(suite, text_encoder):
    """sbagan.rprecision.RPrecision over the sentence embeddings of every caption of the sampled split"""
    from sbagan.rprecision import RPrecision, encode_pool
    v = suite.values
    if 'pool' not in suite.cache:   # (a caller that evaluates more than once keeps the encoded pool: sbagan.track)
        suite.cache['pool'] = encode_pool(suite.data_loader.dataset, lambda c, n: suite.encode(text_encoder, c, n),
                                          suite.batch_size, seed=v['r_precision_seed'], device=suite.device)
    pool, pool_class = suite.cache['pool']
    return RPrecision(suite.load_image_encoder(), pool, pool_class, R=v['r_precision'], seed=v['r_precision_seed'])


def _build_fid(suite, text_encoder):
    """sbagan.fid.FID on the pooled trunk feature; the real side comes from fid_stats when that file exists"""
    from miscc import cli
    from sbagan.feature_rows import dtype_name
    from sbagan.fid import FID, stats_key
    dtype, path = dtype_name(), suite.values['fid_stats']
    key = stats_key(cfg.TRAIN.NET_E.replace('text_encoder', 'image_encoder'), dtype, suite.split_dir, cli.image_size())
    evaluator = FID(suite.image_encoder.pooled_features, D=2048, key=key, dtype=dtype)
    if 'fid_real' in suite.cache:   # (read and checked against the key by an earlier Suite of the same caller)
        evaluator.set_real(suite.cache['fid_real'])
    elif path and os.path.exists(path):
        evaluator.load_real(path)
        print('Load real FID statistics from:', path)
        suite.cache['fid_real'] = evaluator.real_stats()
    return evaluator


def _finish_fid(suite, fid, res, out_dir):
    path = suite.values['fid_stats']
    if path and not fid.is_loaded('real'):
        fid.save_real(path)
        print('Save real FID statistics to:', path)


def _build_prdc(suite, text_encoder):
    from sbagan.feature_rows import dtype_name
    from sbagan.prdc import PRDC
    return PRDC(suite.image_encoder.pooled_features, D=2048, k=suite.values['prdc'], dtype=dtype_name())


def _build_kid(suite, text_encoder):
    """sbagan.kid.KID; with a PRDC evaluator it reads that one's rows and stores none"""
    from sbagan.feature_rows import dtype_name
    from sbagan.kid import KID
    v = suite.values
    return KID(suite.image_encoder.pooled_features, D=2048, subsets=v['kid_subsets'], subset_size=v['kid_subset_size'],
               seed=v['kid_seed'], dtype=dtype_name(), rows=suite.on.get('prdc'))


def _build_ms_ssim(suite, text_encoder):
    """sbagan.msssim.MSSSIM on the uint8 pixels of the last stage's images; refuses images too small for five scales"""
    from miscc import cli
    from sbagan.msssim import MSSSIM
    return MSSSIM(suite.values['ms_ssim'], size=cli.image_size(), seed=suite.values['ms_ssim_seed'])


def _build_swd(suite, text_encoder):
    """sbagan.swd.SWD on the same pixels (beside an MS-SSIM evaluator: on its store); refuses a size without a pyramid"""
    from miscc import cli
    from sbagan.swd import SWD
    return SWD(suite.values['swd'], size=cli.image_size(), seed=suite.values['swd_seed'], images=suite.on.get('ms_ssim'))


def _build_nearest(suite, text_encoder):
    """sbagan.nearest.Nearest on the pooled trunk feature; the training side from nearest_stats when that file exists"""
    from miscc import cli
    from sbagan.feature_rows import dtype_name
    from sbagan.nearest import Nearest, stats_key
    v, dtype = suite.values, dtype_name()
    key = stats_key(cfg.TRAIN.NET_E.replace('text_encoder', 'image_encoder'), dtype, 'train', cli.image_size())
    evaluator = Nearest(suite.image_encoder.pooled_features, D=2048, k=v['nearest'], show=v['nearest_show'], key=key,
                        dtype=dtype)
    if v['nearest_stats'] and os.path.exists(v['nearest_stats']):
        evaluator.load_train(v['nearest_stats'], suite.device)
        print('Load training rows from:', v['nearest_stats'])
    return evaluator


def _train_crops(suite):
    """the training split as the nearest-neighbour pass reads it: the data set class of the sampled split on 'train',
    every image through retrieval._CenterCrops at the size the sampling loader yields for its last scale"""
    from miscc import cli
    from sbagan.retrieval import _CenterCrops
    sampled = suite.data_loader.dataset
    extra = {'bert_dir': sampled.bert_dir} if hasattr(sampled, 'bert_dir') else {}
    train = type(sampled)(sampled.data_dir, 'train', base_size=cfg.TREE.BASE_SIZE, transform=None, **extra)
    imsize = cli.image_size()
    return _CenterCrops(train, imsize, int(imsize * 76 / 64))


def _nearest_finish(suite, nearest, res, out_dir):
    """after the result: the cache of the training rows, and nearest.png (sbagan.nearest.write_sheet)"""
    from sbagan.nearest import write_sheet
    path = suite.values['nearest_stats']
    if path and not nearest.is_loaded():
        nearest.save_train(path)
        print('Save training rows to:', path)
    if nearest.show:
        crops = suite.train_crops if suite.train_crops is not None else _train_crops(suite)
        if [str(k) for k in crops.dataset.filenames] != nearest.keys['train']:
            raise RuntimeError('nearest: the cached training keys are not those of the training split')
        write_sheet(os.path.join(out_dir, 'nearest.png'), res['suspects'], nearest.k,
                    lambda key: os.path.join(out_dir, 'single', key) + '_s-1.png', crops.window)


# ------------------------------------------------------------------ the table
EVALUATORS = (
    Evaluator('r_precision', (
         Option('r_precision', 0, 'R', 2, None, '0 (off) or >= 2 candidates per image',
                '0 (off) or at least 2 candidates per image',
                'sampling: also rank every generated image among R candidate captions (its own and R - 1 of '
                'other classes) with the DAMSM encoders and write r_precision.json; 0 = off, 100 = the '
                'AttnGAN paper\'s setting'),
         Option('r_precision_seed', 100)),      # of the evaluator's own index generator and of the pool's caption draws
        _build_r_precision, 'ranking',
        'R-precision (R = %d, %d images): R@1 %.4f  R@5 %.4f  R@10 %.4f  R@1 over %d splits %.4f +- %.4f',
        ('R', 'n', 'r_at_1', 'r_at_5', 'r_at_10', 'splits', 'r_at_1_splits_mean', 'r_at_1_splits_std')),
    Evaluator('fid', (
         Option('fid', False, help='sampling: also take the Frechet Inception Distance between the real images of the '
                'split and the generated ones on the DAMSM image encoder\'s Inception-v3 trunk (sbagan.fid) and write '
                'fid.json'),
         Option('fid_stats', None, 'PATH', help='with --fid: an .npz of the real images\' statistics; read instead of the '
                'real pass when it exists, written after the run when it does not')),
        _build_fid, 'rows',
        'FID (%d real, %d generated images, %s trunk): %.6g  (mean term %.6g, tr real %.6g, tr fake %.6g)',
        ('n_real', 'n_fake', 'dtype', 'fid', 'mean_term', 'trace_real', 'trace_fake'),
        real_cached=lambda fid: fid.is_loaded('real'), finish=_finish_fid),
    Evaluator('prdc', (
         Option('prdc', 0, 'K', 1, MAX_K, '0 (off) or a neighbour count from 1 to %d' % MAX_K,
                help='sampling: also take precision, recall, density and coverage (the K-nearest-neighbour manifold '
                'metrics, sbagan.prdc) between the real images of the split and the generated ones on the same '
                'trunk features as --fid and write prdc.json; 0 = off, K from 1 to 8, 5 = the usual setting.  '
                'On this project\'s own trunk and compute dtype: not comparable with published numbers'),),
        _build_prdc, 'rows',
        'PRDC (k = %d, %d real, %d generated images, %s trunk): precision %.4f  recall %.4f  '
        'density %.4f  coverage %.4f',
        ('k', 'n_real', 'n_fake', 'dtype', 'precision', 'recall', 'density', 'coverage')),
    Evaluator('kid', (
         Option('kid', False, help='sampling: also take the Kernel Inception Distance (the unbiased MMD^2 estimate under '
                'the kernel (x.y / D + 1)^3 with its standard deviation over subsets, sbagan.kid) between the real '
                'images of the split and the generated ones on the same trunk features as --fid and write '
                'kid.json.  On this project\'s own trunk and compute dtype: not comparable with published '
                'numbers'),
         Option('kid_subsets', 100, 'N', 1, 1024, 'a subset count from 1 to 1024',
                help='with --kid: the number of subsets, 1 to 1024'),
         Option('kid_subset_size', 1000, 'M', 2, None, 'at least 2 rows a side',
                help='with --kid: rows per subset and side (at least 2); clamped to the smaller side'),
         Option('kid_seed', 100)),              # of the evaluator's own generator for the subset draws
        _build_kid, 'rows',
        'KID (%d subsets of %d, %d real, %d generated images, %s trunk): %.6g +- %.6g',
        ('subsets', 'subset_size', 'n_real', 'n_fake', 'dtype', 'kid', 'kid_std'), shares=('prdc', False)),
    Evaluator('ms_ssim', (
         Option('ms_ssim', 0, 'N', 1, None, '0 (off) or a number of pairs per class',
                help='sampling: also take the mean multi-scale structural similarity (MS-SSIM, the within-class '
                'diversity measure of the AC-GAN paper, sbagan.msssim) over N random pairs of images per class, '
                'for the generated images and for the real images of the same pairs, and write ms_ssim.json; '
                '0 = off, 100 = the AC-GAN setting.  In pixel space on the written uint8 images: it uses no '
                'trunk; images of at least 176 px'),
         Option('ms_ssim_seed', 100)),          # of the evaluator's own generator for the pair draws
        _build_ms_ssim, 'images',
        'MS-SSIM (%d same-class pairs of %d images, %d classes, %d skipped, %d px): generated '
        '%.6g +- %.6g  real %.6g +- %.6g',
        ('pairs', 'n_images', 'classes', 'classes_skipped', 'size', 'ms_ssim_fake', 'ms_ssim_fake_std',
         'ms_ssim_real', 'ms_ssim_real_std'), extra='class_ids'),
    Evaluator('swd', (
         Option('swd', 0, 'N', 1, None, '0 (off) or a number of images per side',
                help='sampling: also take the sliced Wasserstein distance (SWD, Karras et al. 2018, sbagan.swd) between '
                'the first N real and the first N generated images, per level of a Laplacian pyramid and on '
                'average, x 1e3, and write swd.json; 0 = off, 16384 = the setting of the paper.  In pixel '
                'space on the written uint8 images: it uses no trunk; square images of 32, 64, 128 or 256 px'),
         Option('swd_seed', 100)),              # of the evaluator's own generator for the patch positions and directions
        _build_swd, 'images',
        'SWD x 1e3 (%d real and %d generated images, %d patches each, %d directions): %s  average %.6g',
        ('n_images', 'n_images', 'patches_per_image', lambda r: r['dir_repeats'] * r['dirs_per_repeat'],
         lambda r: '  '.join('%d px %.6g' % v for v in zip(r['resolutions'], r['swd_x1e3'])), 'swd_avg_x1e3'),
        shares=('ms_ssim', True)),
    Evaluator('nearest', (
         Option('nearest', 0, 'K', 1, MAX_K, '0 (off) or a neighbour count from 1 to %d' % MAX_K,
                help='sampling: also list the K nearest TRAINING images of every generated image on the same trunk '
                'features as --fid (float64 distances on the matrix cores, sbagan.nearest) and take the '
                'memorisation figures the other evaluations cannot see: authenticity (Alaa et al. 2022) with its '
                'baseline on the split\'s real images, the nearest-training-image distance of generated against '
                'unseen real images, the share of near-copies and how many distinct training images are hit; '
                'writes nearest.json and nearest.png; 0 = off, K from 1 to 8.  The training split is encoded '
                'once after the generation loop.  On this project\'s own trunk and compute dtype: not '
                'comparable with published numbers.  Ignored by the DAMSM entry points and in training'),
         Option('nearest_stats', None, 'PATH', help='with --nearest: an .npz of the training images\' feature rows and '
                'keys; read instead of the training pass when it exists, written after the run when it does not'),
         Option('nearest_show', 16, 'M', 0, None, '0 (no picture) or a number of generated images',
                help='with --nearest: the M generated images closest to a training image are listed in nearest.json '
                'and shown in nearest.png, one row each beside their K training images; 0 = no picture')),
        _build_nearest, 'rows',
        'Nearest training images (K = %d, %d training, %d real, %d generated images, %s trunk, this '
        'project\'s own features): authenticity %.4f (real %.4f)  median distance %s (real %s, ratio %s)  '
        'copies %.4f  distinct training images hit %.4f  most hits on one %d',
        ('k', 'n_train', 'n_real', 'n_fake', 'dtype', 'authenticity', 'authenticity_real',
         lambda r: _figure(r['nn_dist_fake']['median']), lambda r: _figure(r['nn_dist_real']['median']),
         lambda r: _figure(r['nn_ratio']), 'copy_fraction', 'train_hit_distinct', 'train_hit_max'),
        extra='keys', finish=_nearest_finish))

OPTIONS = tuple(opt for rec in EVALUATORS for opt in rec.options)


# (name, default) of every trainer attribute the table stands for: the options, <stem>_evaluator, <stem>_result
ATTRIBUTES = tuple((opt.name, opt.default) for opt in OPTIONS) + tuple(
    (rec.stem + tail, None) for rec in EVALUATORS for tail in ('_evaluator', '_result'))


class Suite(object):
    """The evaluators of one sampling() run.  values: {option name: value}.  The rest is what builders need of the trainer:
    its _encode and _load_image_encoder, its data loader, batch size and device.  cache: a dict of the caller's in which
    the builders keep what does not change from one Suite to the next -- 'pool', rprecision.encode_pool's result, and
    'fid_real', the statistics read from fid_stats -- for a caller that evaluates many times in one run (sbagan.track)."""

    def __init__(self, values, split_dir, encode, load_image_encoder, data_loader, batch_size, device, cache=None):
        self.values, self.split_dir, self.encode, self.load_image_encoder = values, split_dir, encode, load_image_encoder
        self.data_loader, self.batch_size, self.device = data_loader, batch_size, device
        self.cache = {} if cache is None else cache
        self.image_encoder = self.train_crops = None
        self.records = [rec for rec in EVALUATORS if values[rec.stem]]
        for opt in (opt for rec in self.records for opt in rec.options if opt.lo is not None):
            _int_option(opt.name, values[opt.name], opt.lo, opt.hi, opt.what)
        self.on = {}                # stem -> evaluator, filled in table order
        self._build(('images',))    # (they touch no model: a size they refuse is refused before anything is written)

    def _build(self, kinds, text_encoder=None):
        for rec in self.records:
            if rec.consumes in kinds:
                if rec.consumes == 'rows' and self.image_encoder is None:   # one image encoder serves them all
                    ranking = self.on.get('r_precision')
                    self.image_encoder = ranking.image_encoder if ranking is not None else self.load_image_encoder()
                self.on[rec.stem] = rec.build(self, text_encoder)

    def attach(self, text_encoder):
        """after the models are loaded: the evaluators that need the text encoder or the image encoder, and the routes"""
        self._build(('ranking', 'rows'), text_encoder)
        fed = [(rec, self.on[rec.stem]) for rec in self.records
               if rec.shares is None or rec.shares[1] or rec.shares[0] not in self.on]
        self._ranking = [ev for rec, ev in fed if rec.consumes == 'ranking']
        self._fake_rows = [(ev, rec.extra == 'keys') for rec, ev in fed if rec.consumes == 'rows']
        self._real_rows = [ev for rec, ev in fed if rec.consumes == 'rows'
                           and not (rec.real_cached is not None and rec.real_cached(ev))]
        self._images = [(ev, rec.extra == 'class_ids') for rec, ev in fed if rec.consumes == 'images']

    def update(self, last, real_last, sent_emb, class_ids, keys):
        """one batch.  Each side goes through the trunk once for every consumer of rows: the generated side not at all
        when R-precision has just run it through, the real side only when somebody takes real rows.  real_last None: the
        real rows come through feed_real_rows instead (evaluators of rows and rankings only)"""
        for ev in self._ranking:
            ev.update(last, sent_emb, class_ids)
        if self._fake_rows:
            if not self._ranking:
                self.image_encoder.pooled_features(last)
            for ev, with_keys in self._fake_rows:
                ev.update_features('fake', self.image_encoder.last_pooled, *((keys,) if with_keys else ()))
            if self._real_rows and real_last is not None:
                real_feats = self.image_encoder.pooled_features(real_last)
                for ev in self._real_rows:
                    ev.update_features('real', real_feats)
        if real_last is None and self._images:
            raise ValueError('the evaluators of pixels (%s) need the real images of every batch'
                             % ', '.join(rec.stem for rec in self.records if rec.consumes == 'images'))
        for ev, with_classes in self._images:       # the pixels themselves: no trunk
            extra = (class_ids,) if with_classes else ()
            ev.update('fake', last, *extra)
            ev.update('real', real_last, *extra)

    def feed_real_rows(self, rows):
        """the real side as pooled trunk rows [n][2048] the caller has kept (f32, on the device), to every evaluator that
        still takes real rows; goes with update(..., real_last=None)"""
        for ev in self._real_rows:
            ev.update_features('real', rows)

    def finish(self, out_dir):
        """the result of every evaluator, in table order: printed, written to <stem>.json, followed by its finish step.
        Returns {stem: (evaluator, result)}"""
        nearest = self.on.get('nearest')
        if nearest is not None and not nearest.is_loaded():     # the training split, once, after the generation loop
            from sbagan.nearest import encode_train
            self.train_crops = crops = _train_crops(self)
            nearest.update_features('train', *encode_train(
                crops.dataset, self.image_encoder.pooled_features, self.batch_size, crops.crop, crops.resize, self.device,
                getattr(self.data_loader, 'num_workers', 0)))
        done = {}
        for rec in self.records:
            ev = self.on[rec.stem]
            res = ev.result()
            print(rec.line % tuple(f(res) if callable(f) else res[f] for f in rec.fields))
            with open(os.path.join(out_dir, rec.stem + '.json'), 'w') as f:
                json.dump(res, f, indent=1, sort_keys=True)
            if rec.finish is not None:
                rec.finish(self, ev, res, out_dir)
            done[rec.stem] = (ev, res)
        return done
