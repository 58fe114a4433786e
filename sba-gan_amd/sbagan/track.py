"""--track E: held-out evaluation curves while the GAN trains.

At the end of every epoch that is due (`due`) and once more after the final checkpoint, the EMA generator -- the weights
save_model would write at that moment -- is evaluated on a held-out split by those of sampling()'s evaluators that read
trunk rows or rankings (--fid, --kid, --prdc, --r_precision; their values and seeds are the trainer's, from
sbagan.evaluation's table).  One line is printed and one JSON line appended to Model/track.jsonl per evaluation; with
--track_best the best weights so far are kept as Model/netG_best.pth beside Model/best.json.

What makes it an instrument of training rather than a second sampling run:

  * the evaluation set is FROZEN, made once per run at the first evaluation (Tracker.prepare): the first N images of the
    split through the trunk the step already holds (centre window, no flip, as --nearest reads the training split), their
    captions 0 .. C - 1 through the frozen text encoder at the full WORDS_NUM width, the noise and the conditioning eps
    from a torch.Generator of the tracker's own (seed 100), and the R-precision candidate pool.  Every evaluation of a
    run sees the same inputs: differences between epochs are differences between generators;
  * nothing here draws from a global generator, runs a module in training mode or writes an image; numpy's global state is
    saved around the caption reads (TextDataset.get_caption draws the word subset of an over-long caption from it);
  * the EMA weights go in and out of the generator the way the 'average' dump does it, followed by the recorded step's
    resync(), so a --replay recording survives and is not rebuilt;
  * the evaluators are built afresh for every evaluation (sbagan.evaluation.Suite, with its route for cached real rows):
    a record is a function of the weights alone.

The figures live on this project's own trunk and compute dtype, as their sampling twins do: comparable between epochs and
runs of this project only.

The frozen set and the measurement over it are FrozenSet, which needs no trainer and no training step: Tracker derives
from it, and sampling()'s --truncation_sweep measures every psi on one (sbagan.truncation.sweep).

Host code; importing this module loads no device library (miscc.cli imports it for the flags)."""
import collections
import json
import math
import os
import shutil
import tempfile
import time

from . import evaluation

SEED = 100                                              # of the tracker's own torch.Generator (noise, eps)
TRACKED = ('fid', 'kid', 'prdc', 'r_precision')         # the evaluators of trunk rows and rankings
NOT_TRACKED = ('ms_ssim', 'swd', 'nearest')             # pixels of both sides / the training split: sampling only

# --track_best KEY -> direction: -1 lower is better, +1 higher is better.  KEY = <stem>.<field of its result>
BEST_KEYS = collections.OrderedDict((
    ('fid.fid', -1), ('kid.kid', -1),
    ('prdc.precision', 1), ('prdc.recall', 1), ('prdc.density', 1), ('prdc.coverage', 1), ('r_precision.r_at_1', 1)))


def due(epoch, every):
    """whether the end of `epoch` is an evaluation point of --track `every` (0 = off); the evaluation after the final
    checkpoint is the loop's own and not decided here"""
    every = int(every)
    if every < 0:
        raise ValueError('due: the interval must be >= 0 (got %d)' % every)
    return every > 0 and int(epoch) % every == 0


def check_flags(args):
    """what is wrong with the --track flags of a parsed command line, as one message, or None.  (--track_captions is
    held against TEXT.CAPTIONS_PER_IMAGE where the configuration is known: Tracker.)"""
    on = [stem for stem in TRACKED if getattr(args, stem, None)]
    if not on:
        return '--track needs at least one of --fid, --kid, --prdc K, --r_precision R: they are what it measures'
    best = getattr(args, 'track_best', None)
    if best is not None:
        if best not in BEST_KEYS:
            return '--track_best: unknown key %r; valid keys are %s' % (best, ', '.join(BEST_KEYS))
        if best.split('.')[0] not in on:
            return '--track_best %s needs --%s' % (best, best.split('.')[0])
    return None


def not_tracked_line(args):
    """the one line an entry point prints when --track meets evaluators that stay out of training, or None"""
    left_out = ['--' + stem for stem in NOT_TRACKED if getattr(args, stem, None)]
    if not left_out:
        return None
    return '--track: %s %s not tracked in training (sampling only)' % (', '.join(left_out),
                                                                       'is' if len(left_out) == 1 else 'are')


def tracked_values(values):
    """{option name: value} for a Suite of the tracked evaluators only: the others at their defaults (off)"""
    out = dict(values)
    for rec in evaluation.EVALUATORS:
        if rec.stem in NOT_TRACKED:
            out.update((opt.name, opt.default) for opt in rec.options)
    return out


def figure(metrics, key):
    """the figure `key` = <stem>.<field> of a record's metrics"""
    stem, field = key.split('.')
    return metrics[stem][field]


def append_jsonl(path, record):
    with open(path, 'a') as f:
        f.write(json.dumps(record, sort_keys=True) + '\n')


def format_line(epoch, metrics, seconds):
    """| end epoch N | track kid ... fid ... prdc p r d c | r@1 ... | S.s s |  (the parts that were taken)"""
    parts = []
    if 'kid' in metrics:
        parts.append('kid %.6g' % metrics['kid']['kid'])
    if 'fid' in metrics:
        parts.append('fid %.6g' % metrics['fid']['fid'])
    if 'prdc' in metrics:
        parts.append('prdc %.4f %.4f %.4f %.4f' % tuple(metrics['prdc'][k] for k in ('precision', 'recall', 'density',
                                                                                      'coverage')))
    line = '| end epoch %d | track %s |' % (epoch, ' '.join(parts))
    if 'r_precision' in metrics:
        line += ' r@1 %.4f |' % metrics['r_precision']['r_at_1']
    return line + ' %.1f s |' % seconds


class Best(object):
    """The best figure of --track_best so far.  key: one of BEST_KEYS; model_dir: where best.json (key, value, epoch,
    iteration) lives beside netG_best.pth; resume_dir: the directory of the checkpoint a run resumes from -- a best.json
    there under the same key is where this run starts, so a worse later epoch does not replace it."""

    def __init__(self, key, model_dir, resume_dir=None):
        if key not in BEST_KEYS:
            raise ValueError('track_best: unknown key %r; valid keys are %s' % (key, ', '.join(BEST_KEYS)))
        self.key, self.sign, self.model_dir = key, BEST_KEYS[key], model_dir
        self.value = self.epoch = self.iteration = None
        path = os.path.join(resume_dir, 'best.json') if resume_dir else None
        if path and os.path.isfile(path):
            with open(path) as f:
                held = json.load(f)
            if held.get('key') == key and self._is_number(held.get('value')):
                self.value, self.epoch, self.iteration = float(held['value']), held.get('epoch'), held.get('iteration')
                print('Load best %s from: %s (%.6g at epoch %s)' % (key, path, self.value, self.epoch))
            else:
                print('%s holds %r, not %s: the best so far starts empty' % (path, held.get('key'), key))

    @staticmethod
    def _is_number(v):
        return isinstance(v, (int, float)) and not isinstance(v, bool) and not math.isnan(v)

    def improves(self, value):
        """strictly better than the best so far (a tie keeps the earlier epoch); a NaN or a missing figure never is"""
        if not self._is_number(value):
            return False
        return self.value is None or (value - self.value) * self.sign > 0

    def offer(self, value, epoch, iteration):
        """take `value` if it improves: best.json is written; returns whether it did (the caller writes the weights)"""
        if not self.improves(value):
            return False
        self.value, self.epoch, self.iteration = float(value), int(epoch), int(iteration)
        with open(os.path.join(self.model_dir, 'best.json'), 'w') as f:
            json.dump({'key': self.key, 'value': self.value, 'epoch': self.epoch, 'iteration': self.iteration}, f,
                      indent=1, sort_keys=True)
        return True


class _First(object):
    """the first n images of a data set, with everything else of it"""

    def __init__(self, dataset, n):
        self.dataset, self.n = dataset, int(n)

    def __len__(self):
        return self.n

    def __getattr__(self, name):
        if name in ('dataset', 'n') or name.startswith('__'):       # (unpickled or copied: not set yet, no recursion)
            raise AttributeError(name)
        return getattr(self.dataset, name)


class _Loader(object):
    """what a Suite's builders read of a data loader"""

    def __init__(self, dataset, num_workers):
        self.dataset, self.num_workers = dataset, num_workers


class FrozenSet(object):
    """The frozen evaluation set (see the module's text) and the measurement over it, without a trainer or a GANStep:
    what --track evaluates every due epoch (Tracker) and what sampling()'s --truncation_sweep evaluates per psi
    (sbagan.truncation.sweep).

    encode: the trainer's _encode hook (text_encoder, captions, cap_lens) -> (words_embs, sent_emb); noise_shape: n ->
    the shape of the noise of n rows; batch_size, device; values: {option name: value} of sbagan.evaluation's options
    (those of the tracked evaluators count); split: the name the evaluators are told; n: the first n images of the data
    set (0: all); captions: captions 0 .. captions - 1 of each; num_workers: of the real-image pass.  The image encoder
    (InceptionHIP) and the data set arrive with prepare()."""

    def __init__(self, encode, noise_shape, batch_size, device, values, split, n=0, captions=1, num_workers=0):
        self.encode, self.noise_shape, self.batch_size, self.device = encode, noise_shape, int(batch_size), device
        self.values, self.split, self.n, self.captions = tracked_values(values), str(split), int(n), int(captions)
        self.num_workers = num_workers
        if self.n < 0:
            raise ValueError('n must be 0 (the whole split) or a number of images (got %d)' % self.n)
        if not any(self.values[stem] for stem in TRACKED):
            raise ValueError('a frozen set needs at least one of fid, kid, prdc, r_precision: they are what it measures')
        self.prepared = False
        self.timing = {}            # seconds of the last measurement's parts (tools/bench_track.py)

    # ------------------------------------------------------------------ once per run
    def prepare(self, text_encoder, image_encoder, dataset, what='--track'):
        """the frozen evaluation set (see the module's text) over `dataset`; what: the flag named in messages"""
        import numpy as np
        import torch
        from miscc import cli
        from miscc.config import cfg
        from . import ops
        from .nearest import encode_train
        from .trainer import build_mask
        t0 = time.time()
        dev, B = self.device, self.batch_size
        self.image_encoder = enc = image_encoder
        if enc is None or not hasattr(enc, 'pooled_features'):
            raise RuntimeError('%s needs the HIP image encoder (InceptionHIP.pooled_features)' % what)
        self.dataset = ds = dataset
        total = len(ds)
        n = total if self.n == 0 else self.n
        if n > total:
            raise ValueError('%s: %d is more than the %d images of the %s split' % (what, n, total, self.split))
        C, W, per = self.captions, cfg.TEXT.WORDS_NUM, ds.embeddings_num
        workers = self.num_workers
        loader = _Loader(ds, workers)

        # the evaluators are built once here for what is refused at construction (a value out of range, a --fid_stats
        # file under another key) and for what every later Suite is handed in self.cache: the R-precision pool and the
        # real statistics read from --fid_stats
        def encode(enc_, captions, cap_lens):
            return self.encode(enc_, captions, cap_lens)
        self._suite_args = (self.values, self.split, encode, lambda: self.image_encoder, loader, B, dev)
        self.cache = {}
        suite = evaluation.Suite(*self._suite_args, cache=self.cache)
        suite.attach(text_encoder)
        self.pool = self.cache.get('pool')
        need_real = bool(suite._real_rows)

        def features(imgs):
            ops.det_reset()
            return enc.pooled_features(imgs)
        imsize = cli.image_size()
        self.real_rows = self.real_keys = None
        if need_real:
            self.real_rows, self.real_keys = encode_train(_First(ds, n), features, B, imsize, int(imsize * 76 / 64), dev,
                                                          workers)

        # captions 0 .. C - 1 of every image, by index (dataset[i] would draw one of them at random)
        state = np.random.get_state()
        try:
            np.random.seed(SEED)
            picked = [ds.get_caption(i * per + c) for i in range(n) for c in range(C)]
        finally:
            np.random.set_state(state)
        caps = np.stack([p[0] for p in picked]).reshape(n * C, -1)[:, :W]
        lens = np.asarray([p[1] for p in picked], dtype=np.int64)
        words, sents = [], []
        for lo in range(0, n * C, B):       # chunks sorted by length, descending (what the packed bi-LSTM takes)
            order = np.argsort(-lens[lo:lo + B], kind='stable')
            inverse = np.empty_like(order)
            inverse[order] = np.arange(len(order))
            w, s = self.encode(text_encoder, torch.from_numpy(caps[lo:lo + B][order]).to(dev),
                               torch.from_numpy(lens[lo:lo + B][order]).to(dev))
            full = torch.zeros((w.size(0), w.size(1), W), dtype=torch.float32, device=dev)
            full[:, :, :min(W, w.size(2))] = w.detach().float()[:, :, :W]   # (the columns past the longest caption: zeros)
            back = torch.from_numpy(inverse).to(dev)
            words.append(full.index_select(0, back))
            sents.append(s.detach().float().index_select(0, back))
        self.words_embs, self.sent_emb = torch.cat(words).contiguous(), torch.cat(sents).contiguous()
        self.caps = torch.from_numpy(caps).to(dev)
        self.mask = build_mask(self.caps, W).contiguous()
        self.class_ids = np.repeat(np.asarray(ds.class_id)[:n], C)
        self.keys = [str(k) for k in ds.filenames[:n] for _ in range(C)]
        gen = torch.Generator(device=dev)
        gen.manual_seed(SEED)
        self.noise = torch.randn(self.noise_shape(n * C), generator=gen, device=dev, dtype=torch.float32)
        self.eps = torch.randn((n * C, cfg.GAN.CONDITION_DIM), generator=gen, device=dev, dtype=torch.float32)
        self.images, self.rows = n, n * C
        self.prepared = True
        torch.cuda.synchronize()
        self.timing['prepare'] = time.time() - t0
        print('%s: %d images x %d captions of the %s split prepared in %.1f s'
              % (what, n, C, self.split, self.timing['prepare']))

    # ------------------------------------------------------------------ per evaluation
    def slices(self):
        return [(lo, min(lo + self.batch_size, self.rows)) for lo in range(0, self.rows, self.batch_size)]

    def measure(self, generator, ca_net):
        """{stem: result} of `generator` (netG in eval mode, or its fused wrapper) over the frozen set: fresh evaluators,
        the same slices, noise and eps every time.  ca_net: the generator's conditioning module, whose eps is set per
        slice (it would draw from the global generator otherwise) and put back."""
        import torch
        from . import ops
        suite = evaluation.Suite(*self._suite_args, cache=self.cache)
        suite.attach(None)
        held = ca_net.eps
        t0 = time.time()
        try:
            with torch.no_grad():
                for lo, hi in self.slices():
                    ops.det_reset()
                    ca_net.eps = self.eps[lo:hi]
                    fake_imgs = generator(self.noise[..., lo:hi, :].contiguous(), self.sent_emb[lo:hi],
                                          self.words_embs[lo:hi], self.mask[lo:hi])[0]
                    suite.update(fake_imgs[-1], None, self.sent_emb[lo:hi], self.class_ids[lo:hi], self.keys[lo:hi])
        finally:
            ca_net.eps = held
        if self.real_rows is not None:
            suite.feed_real_rows(self.real_rows)
        torch.cuda.synchronize()
        t1 = time.time()
        results = collections.OrderedDict()
        per = {}
        for rec in suite.records:
            ts = time.time()
            results[rec.stem] = suite.on[rec.stem].result()
            per[rec.stem] = time.time() - ts
        self.timing.update(generate=t1 - t0, results=time.time() - t1, result_of=per)
        return results


class Tracker(FrozenSet):
    """trainer: the condGANTrainer (its device, batch size, data loader, model directory, text and noise hooks, evaluator
    options and, by the time of the first evaluation, its GANStep); every / split / n / captions / best: --track,
    --track_split, --track_n, --track_captions, --track_best."""

    def __init__(self, trainer, every, split='test', n=0, captions=1, best=None):
        from miscc.config import cfg
        self.trainer, self.every = trainer, int(every)
        if self.every < 1:
            raise ValueError('track must be an interval of at least 1 epoch (got %d)' % self.every)
        if int(n) < 0:
            raise ValueError('track_n must be 0 (the whole split) or a number of images (got %d)' % int(n))
        if not 1 <= int(captions) <= cfg.TEXT.CAPTIONS_PER_IMAGE:
            raise ValueError('track_captions must be from 1 to TEXT.CAPTIONS_PER_IMAGE = %d (got %d)'
                             % (cfg.TEXT.CAPTIONS_PER_IMAGE, int(captions)))
        values = tracked_values({opt.name: getattr(trainer, opt.name) for opt in evaluation.OPTIONS})
        if not any(values[stem] for stem in TRACKED):
            raise ValueError('track needs at least one of fid, kid, prdc, r_precision: they are what it measures')
        if best is not None and not values[best.split('.')[0]]:
            raise ValueError('track_best %s needs %s' % (best, best.split('.')[0]))
        # (the hooks are read off the trainer when they are called: a test or a tool may have replaced them since)
        super(Tracker, self).__init__(lambda *a: trainer._encode(*a), lambda rows: trainer._noise_shape(rows),
                                      trainer.batch_size, trainer.device, values, split, n, captions,
                                      getattr(trainer.data_loader, 'num_workers', 0))
        resume = os.path.dirname(cfg.TRAIN.NET_G) if cfg.TRAIN.NET_G else None
        self.best = Best(best, trainer.model_dir, resume) if best is not None else None
        self.path = os.path.join(trainer.model_dir, 'track.jsonl')
        self.records = []           # of this run, as appended

    def due(self, epoch):
        return due(epoch, self.every)

    # ------------------------------------------------------------------ once per run
    def _dataset(self):
        from miscc.config import cfg
        sampled = self.trainer.data_loader.dataset
        extra = {'bert_dir': sampled.bert_dir} if hasattr(sampled, 'bert_dir') else {}
        return type(sampled)(sampled.data_dir, self.split, base_size=cfg.TREE.BASE_SIZE, transform=None, **extra)

    def prepare(self, text_encoder, dataset=None):
        """the frozen evaluation set; dataset: the held-out data set when the caller has one"""
        self.batch_size = self.trainer.batch_size
        super(Tracker, self).prepare(text_encoder, self.trainer.gan.image_encoder,
                                     dataset if dataset is not None else self._dataset())

    def evaluate(self, netG, text_encoder, epoch, iteration, stepper=None, checkpoint=None):
        """One evaluation of the EMA weights at the end of `epoch`.  checkpoint: the name of the netG_epoch_N.pth save_model
        has just written for these very weights, or None.  Returns the record appended to track.jsonl."""
        import torch
        from miscc.utils import copy_G_params, load_params
        tr = self.trainer
        gan = tr.gan
        if not self.prepared:
            self.prepare(text_encoder)
        t0 = time.time()
        gan.finish()
        backup = copy_G_params(netG)
        was = netG.training
        load_params(netG, gan.flatG.ema_params())
        netG.eval()
        try:
            metrics = self.measure(tr._inference_generator(netG), netG.ca_net)
            if self.best is not None and self.best.offer(figure(metrics, self.best.key), epoch, iteration):
                # the bytes save_model writes for this epoch: its file where it has just been written, else the same call
                path = os.path.join(tr.model_dir, 'netG_best.pth')
                if checkpoint is not None:
                    shutil.copyfile(os.path.join(tr.model_dir, checkpoint), path)
                else:
                    # torch.save names the records of its archive after the file: written under the name save_model
                    # would use (in a directory of its own), then moved
                    tmp = tempfile.mkdtemp(prefix='best_', dir=tr.model_dir)
                    try:
                        torch.save(netG.state_dict(), os.path.join(tmp, 'netG_epoch_%d.pth' % epoch))
                        os.replace(os.path.join(tmp, 'netG_epoch_%d.pth' % epoch), path)
                    finally:
                        shutil.rmtree(tmp, ignore_errors=True)
                print('Save best G model (%s %.6g).' % (self.best.key, self.best.value))
        finally:
            load_params(netG, backup)
            netG.train(was)
            if stepper is not None:     # the parameters were edited behind the recording's back
                stepper.resync()
        seconds = time.time() - t0
        record = {'epoch': int(epoch), 'iteration': int(iteration), 'split': self.split, 'images': self.images,
                  'captions_per_image': self.captions, 'checkpoint': checkpoint, 'seconds': seconds, 'metrics': metrics}
        print(format_line(epoch, metrics, seconds))
        append_jsonl(self.path, record)
        self.records.append(record)
        return record
