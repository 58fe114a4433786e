"""--truncation PSI: the truncation trick in W (Karras et al., CVPR 2019, appendix B).

Every later stage of the generators takes its style from w = MAPPING_NET(z).  A set truncation replaces it, inside
_GBase._styles and on the stream the mapping network ran on, by

    w' = w_avg + psi (w - w_avg),        w_avg = the mean of MAPPING_NET(z) over z ~ N(0, I),

which trades diversity for fidelity: psi = 1 is the generator as trained (the kernel copies, so that run is bit for bit
the run without a truncation), psi = 0 gives every image the mean style.

What is and is not truncated:

  * model.G_NET feeds z itself to the first stage (INIT_STAGE_G reads [c_code, z]).  Only the AdaIN styles of stages 2 and
    3 are truncated there: the 64 px image does not move with psi, and z still acts on the later images through the
    first stage's feature map;
  * in the BERT generators (model_bert.G_NET, G_NET_MIX) the first stage reads the conditioning alone and z acts through
    w alone: psi = 0 makes the images independent of the noise (not of the conditioning's eps);
  * G_NET_MIX maps two codes: w(z[0]) styles stage 2 and w(z[1]) stage 3; a pair of psi gives the first value to the first.

w_avg is the Monte-Carlo mean over the checkpoint's OWN mapping network (mean_style: n codes from a generator of its
own, the column means by ops.style_mean in a fixed float64 order) -- exact for that network up to sampling error, and
available for every existing checkpoint; nothing is tracked during training.  There is no backward: a truncation is refused
in training mode and with grad enabled.

Also here: the psi sweep of sampling() over a frozen set (sweep; sbagan.track.FrozenSet), the flags' argparse types and
the schemas of truncation.json / truncation_sweep.json.

Host code; importing this module loads no device library (miscc.cli imports it for the flags)."""
import argparse
import copy
import json
import math
import os
import time

SEED = 100                          # of mean_style's own torch.Generator
DEFAULT_N = 16384                   # codes in the Monte-Carlo mean
MAX_N = 1 << 20                     # what one sba_style_mean call takes
CHUNK = 4096                        # codes per mapping-network pass, at most (pass_rows)


# ------------------------------------------------------------------ flags
def _psi(text, flag):
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError('%s: %r is not a number' % (flag, text))
    if not 0.0 <= v <= 1.0:         # (a NaN fails both comparisons)
        raise argparse.ArgumentTypeError('%s: psi must be in [0, 1] (got %s)' % (flag, text))
    return v


def parse_psi(text):
    """the argparse type of --truncation: PSI or PSI,PSI (stage 2, stage 3), each in [0, 1] -> a float or a pair"""
    parts = [p.strip() for p in str(text).split(',')]
    if len(parts) not in (1, 2):
        raise argparse.ArgumentTypeError('--truncation takes PSI or PSI,PSI (stage 2, stage 3), got %r' % text)
    values = [_psi(p, '--truncation') for p in parts]
    return values[0] if len(values) == 1 else tuple(values)


def parse_sweep(text):
    """the argparse type of --truncation_sweep: at least one psi in [0, 1], comma separated, no duplicates -> a tuple"""
    parts = [p.strip() for p in str(text).split(',')]
    if parts == ['']:
        raise argparse.ArgumentTypeError('--truncation_sweep needs at least one psi')
    values = tuple(_psi(p, '--truncation_sweep') for p in parts)
    if len(set(values)) != len(values):
        raise argparse.ArgumentTypeError('--truncation_sweep: a psi is listed twice in %r' % text)
    return values


def check_flags(args):
    """what is wrong with the truncation flags of a parsed command line, as one message, or None"""
    from . import track
    if getattr(args, 'truncation_sweep', None) and not any(getattr(args, stem, None) for stem in track.TRACKED):
        return ('--truncation_sweep needs at least one of --fid, --kid, --prdc K, --r_precision R: they are what it '
                'measures')
    return None


def not_swept_line(args):
    """the one line an entry point prints when --truncation_sweep meets evaluators that stay with the normal run, or None"""
    from . import track
    left = ['--' + stem for stem in track.NOT_TRACKED if getattr(args, stem, None)]
    if not left:
        return None
    return '--truncation_sweep: %s %s not swept (the normal run only)' % (', '.join(left),
                                                                         'is' if len(left) == 1 else 'are')


# ------------------------------------------------------------------ the mean style and the hook's object
def pass_rows(net, chunk=CHUNK):
    """codes per mapping-network pass: `chunk`, held to what the dense f32 kernels take in one call -- they keep the
    whole input [rows][K] in LDS, rows * K * 4 <= 64 KB (64 rows at W_DIM 256)"""
    return max(1, min(int(chunk), (64 * 1024) // (4 * max(net.z_dim, net.w_dim))))


def mapped_styles(netG, n=DEFAULT_N, seed=SEED, chunk=CHUNK):
    """w [n][W_DIM] f32 = netG.mapping_net(z) over n codes z ~ N(0, I) drawn in ONE call from a torch.Generator of this
    call's own on the generator's device (seeded with `seed`; no global generator is touched), mapped under no_grad in
    passes of pass_rows(mapping_net, chunk) codes"""
    import torch
    n, chunk = int(n), int(chunk)
    if not 1 <= n <= MAX_N:
        raise ValueError('mean_style: n must be from 1 to %d (got %d)' % (MAX_N, n))
    if chunk < 1:
        raise ValueError('mean_style: chunk must be at least 1 (got %d)' % chunk)
    net = netG.mapping_net
    dev = next(net.parameters()).device
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    z = torch.randn((n, net.z_dim), generator=gen, device=dev, dtype=torch.float32)
    w = torch.empty((n, net.w_dim), dtype=torch.float32, device=dev)
    rows = pass_rows(net, chunk)
    with torch.no_grad():
        for lo in range(0, n, rows):
            w[lo:lo + rows] = net(z[lo:lo + rows])
    return w


def mean_style(netG, n=DEFAULT_N, seed=SEED, chunk=CHUNK):
    """(mean64 [W_DIM] float64, mean32 [W_DIM] float32): the mean of mapped_styles(netG, n, seed, chunk) by ONE
    ops.style_mean call over all n rows (16 MB at the defaults), in its fixed float64 order"""
    from . import ops
    return ops.style_mean(mapped_styles(netG, n, seed, chunk))


def stage_psi(psi, branches):
    """(psi of stage 2, psi of stage 3) from one value or a pair, held against the number of stages; ValueError otherwise"""
    pair = isinstance(psi, (tuple, list))
    values = tuple(float(v) for v in psi) if pair else (float(psi),)
    if len(values) not in (1, 2):
        raise ValueError('truncation: psi must be one value or a pair (stage 2, stage 3), got %r' % (psi,))
    for v in values:
        if not 0.0 <= v <= 1.0:         # (a NaN fails both comparisons)
            raise ValueError('truncation: psi must be in [0, 1] (got %r)' % v)
    if branches < 2:
        raise ValueError('truncation: TREE.BRANCH_NUM = %d: no stage reads a style' % branches)
    if len(values) == 2 and branches < 3:
        raise ValueError('truncation: a pair of psi needs TREE.BRANCH_NUM = 3 (got %d): there is one later stage'
                         % branches)
    return values if len(values) == 2 else values * 2


class Truncation(object):
    """w_avg (f32 [W_DIM] on the generator's device; w_avg64: the float64 mean it is the rounding of) of netG's mapping
    network and the psi of each later stage.  psi: one value in [0, 1] for both later stages, or a pair (stage 2, stage 3);
    n, seed: of mean_style.  Set as `netG.truncation = Truncation(netG, psi)`; None (the class attribute) is off."""

    def __init__(self, netG, psi, n=DEFAULT_N, seed=SEED):
        self.psi = stage_psi(psi, int(netG.branch_num))
        if not 1 <= int(n) <= MAX_N:
            raise ValueError('truncation: n must be from 1 to %d (got %d)' % (MAX_N, int(n)))
        self.netG, self.n, self.seed = netG, int(n), int(seed)
        self.refresh()

    def refresh(self):
        """recompute w_avg: after the generator's weights changed"""
        self.w_avg64, self.w_avg = mean_style(self.netG, self.n, self.seed)
        return self

    def with_psi(self, psi):
        """a Truncation of the same generator at another psi, sharing this one's w_avg (not recomputed)"""
        other = copy.copy(self)
        other.psi = stage_psi(psi, int(self.netG.branch_num))
        return other

    def apply(self, ws):
        """the truncated styles of _GBase._styles' list `ws` (one w, or G_NET_MIX's two), on the current stream: one
        launch per w with equal psi; with a pair and one w two launches, [w of stage 2, w of stage 3]"""
        from . import ops
        a, b = self.psi
        if len(ws) == 1:
            w2 = ops.style_truncate(ws[0], self.w_avg, a)
            return [w2] if a == b else [w2, ops.style_truncate(ws[0], self.w_avg, b)]
        return [ops.style_truncate(ws[0], self.w_avg, a), ops.style_truncate(ws[-1], self.w_avg, b)]

    def describe(self):
        """the fields of truncation.json that need no sampled w"""
        return {'psi': list(self.psi), 'n': self.n, 'seed': self.seed,
                'w_avg_norm': float(self.w_avg64.norm().item())}


def unwrap(generator):
    """the _GBase module behind a generator or its FusedGenerator wrapper"""
    return getattr(generator, 'netG', generator)


def set_truncation(generator, psi, n=DEFAULT_N, seed=SEED):
    """set (psi None: clear) the truncation of a loaded generator or of its fused wrapper; returns the Truncation"""
    net = unwrap(generator)
    net.truncation = None if psi is None else Truncation(net, psi, n, seed)
    return net.truncation


class WDistance(object):
    """the RMS distance of the w a sampling run draws from w_avg, accumulated on the device in float64 from the run's
    own noise (the mapping network is run once more per batch, on the untruncated w: |w - w_avg| over rows, squared)"""

    def __init__(self, truncation):
        self.t, self.sum, self.rows = truncation, None, 0

    def update(self, noise):
        import torch
        net = self.t.netG.mapping_net
        with torch.no_grad():
            z = noise.reshape(-1, noise.size(-1))
            d = net(z).double() - self.t.w_avg64
            s = (d * d).sum()
        self.sum = s if self.sum is None else self.sum + s
        self.rows += z.size(0)

    def result(self):
        return math.sqrt(float(self.sum.item()) / self.rows) if self.rows else None


def write_json(out_dir, truncation, w_rms):
    """<out_dir>/truncation.json: {psi [stage 2, stage 3], n, seed, w_avg_norm, w_rms_distance, w_rows}"""
    record = truncation.describe()
    record['w_rms_distance'] = w_rms.result()
    record['w_rows'] = w_rms.rows
    check_record(record)
    with open(os.path.join(out_dir, 'truncation.json'), 'w') as f:
        json.dump(record, f, indent=1, sort_keys=True)
    return record


# ------------------------------------------------------------------ schemas
def _number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def check_record(record):
    """raises ValueError unless `record` is what truncation.json holds"""
    want = {'psi', 'n', 'seed', 'w_avg_norm', 'w_rms_distance', 'w_rows'}
    if not isinstance(record, dict) or set(record) != want:
        raise ValueError('truncation.json: keys %s, expected %s' % (sorted(record) if isinstance(record, dict) else record,
                                                                    sorted(want)))
    psi = record['psi']
    if not (isinstance(psi, list) and len(psi) == 2 and all(_number(v) and 0.0 <= v <= 1.0 for v in psi)):
        raise ValueError('truncation.json: psi must be [stage 2, stage 3], each in [0, 1] (got %r)' % (psi,))
    for key in ('n', 'seed', 'w_rows'):
        if not isinstance(record[key], int) or isinstance(record[key], bool) or record[key] < 0:
            raise ValueError('truncation.json: %s must be a non-negative integer (got %r)' % (key, record[key]))
    if not 1 <= record['n'] <= MAX_N:
        raise ValueError('truncation.json: n must be from 1 to %d (got %r)' % (MAX_N, record['n']))
    if not (_number(record['w_avg_norm']) and record['w_avg_norm'] >= 0):
        raise ValueError('truncation.json: w_avg_norm must be a non-negative number (got %r)' % (record['w_avg_norm'],))
    rms = record['w_rms_distance']
    if not (rms is None or (_number(rms) and rms >= 0)):
        raise ValueError('truncation.json: w_rms_distance must be a non-negative number or null (got %r)' % (rms,))
    return record


def check_sweep(records):
    """raises ValueError unless `records` is what truncation_sweep.json holds: a list of {psi, seconds, metrics}, one per
    psi, no psi twice, metrics = {stem: the evaluator's result dict} over the swept evaluators"""
    from . import track
    if not isinstance(records, list) or not records:
        raise ValueError('truncation_sweep.json: a non-empty list of records, got %r' % (records,))
    seen = set()
    for r in records:
        if not isinstance(r, dict) or set(r) != {'psi', 'seconds', 'metrics'}:
            raise ValueError('truncation_sweep.json: a record has keys psi, seconds, metrics; got %r' % (r,))
        if not (_number(r['psi']) and 0.0 <= r['psi'] <= 1.0) or r['psi'] in seen:
            raise ValueError('truncation_sweep.json: psi must be in [0, 1] and listed once (got %r)' % (r['psi'],))
        seen.add(r['psi'])
        if not (_number(r['seconds']) and r['seconds'] >= 0):
            raise ValueError('truncation_sweep.json: seconds must be a non-negative number (got %r)' % (r['seconds'],))
        m = r['metrics']
        if not isinstance(m, dict) or not m or not set(m) <= set(track.TRACKED) or not all(isinstance(v, dict)
                                                                                            for v in m.values()):
            raise ValueError('truncation_sweep.json: metrics must hold result dicts under some of %s (got %r)'
                             % (', '.join(track.TRACKED), m))
    return records


def format_line(psi, metrics, seconds):
    """track.format_line with psi in place of the epoch:  | psi 0.7 | track kid ... | r@1 ... | S.s s |"""
    from . import track
    return track.format_line(0, metrics, seconds).replace('| end epoch 0 |', '| psi %g |' % psi, 1)


# ------------------------------------------------------------------ the sweep
def sweep(trainer, generator, text_encoder, psis, split_dir, out_dir, n=0, image_encoder=None):
    """The psi sweep of sampling(): one frozen set over the sampled split (track.FrozenSet: the first n images -- 0: all
    of them -- caption 0 of each, centre window, no flip, real rows through the trunk once, noise and eps from a generator
    of its own), then for each psi of `psis`, in the given order, the truncation is set on `generator` and measure()
    taken.  No image is written; one line per psi is printed and <out_dir>/truncation_sweep.json written.  The
    generator's truncation is put back afterwards.  image_encoder: the trunk the normal run has loaded, or None to load
    it.  Returns the records."""
    from . import evaluation, track
    values = track.tracked_values({opt.name: getattr(trainer, opt.name) for opt in evaluation.OPTIONS})
    if not any(values[stem] for stem in track.TRACKED):
        raise ValueError('truncation_sweep needs at least one of fid, kid, prdc, r_precision: they are what it measures')
    net = unwrap(generator)
    held = net.truncation
    if image_encoder is None:
        image_encoder = trainer._load_image_encoder()
    frozen = track.FrozenSet(trainer._encode, trainer._noise_shape, trainer.batch_size, trainer.device, values, split_dir,
                             n=n, captions=1, num_workers=getattr(trainer.data_loader, 'num_workers', 0))
    frozen.prepare(text_encoder, image_encoder, plain_dataset(trainer.data_loader.dataset, split_dir),
                   what='--truncation_sweep')
    records = []
    try:
        base = held     # (the normal run's w_avg where there is one: the same weights)
        for psi in psis:
            t0 = time.time()
            if base is None:
                base = Truncation(net, psi, getattr(trainer, 'truncation_n', DEFAULT_N), SEED)
            net.truncation = base.with_psi(psi)
            metrics = frozen.measure(generator, net.ca_net)
            seconds = time.time() - t0
            print(format_line(psi, metrics, seconds))
            records.append({'psi': float(psi), 'seconds': seconds, 'metrics': metrics})
    finally:
        net.truncation = held
    check_sweep(json.loads(json.dumps(records)))
    with open(os.path.join(out_dir, 'truncation_sweep.json'), 'w') as f:
        json.dump(records, f, indent=1, sort_keys=True)
    return records


def plain_dataset(sampled, split):
    """the sampled split as the frozen set reads it: the same class and directory, no transform (centre window)"""
    from miscc.config import cfg
    extra = {'bert_dir': sampled.bert_dir} if hasattr(sampled, 'bert_dir') else {}
    return type(sampled)(sampled.data_dir, split, base_size=cfg.TREE.BASE_SIZE, transform=None, **extra)
