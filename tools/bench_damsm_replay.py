#!/usr/bin/env python3
"""pretrain_DAMSM.py --replay measured (run alone on the GPU, profiler off).

pretrain_DAMSM.train -- the entry point's own loop, its interval line and its host reads included -- at the sizes of
cfg/DAMSM/bird.yml (299 px, WORDS_NUM 18, bf16; B = 48, --batch) with randomly initialised encoders, over a synthetic
device-resident cache (seeded uint8 images, seeded captions), in two arms:

    --device_data --replay     sbagan.damsm.DAMSMSlotStep: the update re-issued from one recording, the device loader
                               bound to its batch slot, the losses read where the interval line is printed
    --device_data              sbagan.damsm.DAMSMStep: the eager update, four float() reads per batch

alternated in ONE process: per round and arm, `--iters` iterations after `--warm_iters`, between two device
synchronises.  Also printed: the node counts of the recording, and the launches of one eager update, counted by
stream-capturing DAMSMStep.step once (nothing of that capture is ever launched).

    python tools/bench_damsm_replay.py [--out profiles/damsm_replay.txt] [--iters 200] [--warm_iters 40] [--rounds 3]
"""
import argparse
import ctypes
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'sba-gan_amd')
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

LINES = []
INFO_KEYS = ('nodes', 'kernels', 'copies', 'memsets', 'streams', 'waits', 'events', 'host_calls')


def say(text=''):
    print(text, flush=True)
    LINES.append(text)


class SynthCaptions(object):
    """what DeviceBatchLoader asks of a dataset: seeded captions (lengths 5 .. WORDS_NUM), class ids, keys"""
    embeddings_num = 10

    def __init__(self, n, words_num, vocab, seed=0):
        rng = np.random.RandomState(seed)
        self.n, self.n_words = n, vocab
        self.lengths = rng.randint(5, words_num + 1, n * self.embeddings_num)
        self.captions = rng.randint(1, vocab, (n * self.embeddings_num, words_num)).astype(np.int64)
        self.captions[np.arange(words_num)[None, :] >= self.lengths[:, None]] = 0
        self.class_id = [1 + i % 200 for i in range(n)]
        self.filenames = ['cls/img%04d' % i for i in range(n)]
        self.ixtoword = {i: 'w%d' % i for i in range(vocab)}

    def __len__(self):
        return self.n

    def get_caption(self, index):
        return self.captions[index].reshape(-1, 1), int(self.lengths[index])


class Timed(object):
    """hands a loader's batches, epoch after epoch, to the loop and times iterations [warm, warm + steps) between two
    synchronises"""

    def __init__(self, loader, warm, steps):
        self.loader, self.warm, self.steps, self.ms = loader, warm, steps, None

    def __len__(self):
        return self.warm + self.steps + 1

    def __iter__(self):
        n, t0 = 0, None
        while True:
            for data in self.loader:
                if n == self.warm:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                elif n == self.warm + self.steps:
                    torch.cuda.synchronize()
                    self.ms = (time.perf_counter() - t0) * 1e3 / self.steps
                n += 1
                yield data


def count_eager_launches(step, batch):
    """nodes of ONE DAMSMStep.step, stream-captured after the arm's last window and never launched"""
    from miscc import losses
    from sbagan import ops
    from sbagan._lib import call, lib
    from sbagan.trainer import _CAPTURE_MODE
    imgs, captions, cap_lens, class_ids, keys = batch
    dev = step.device
    # (the same-class mask of host ids is built on the host and uploaded: a copy, not allowed in a capture, not a launch)
    class_ids = ops.ClassMask(losses.class_mask(class_ids, step.batch_size, dev))
    rng = torch.cuda.get_rng_state(dev)
    cap = torch.cuda.Stream(device=dev)
    cap.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, stream=cap, capture_error_mode=_CAPTURE_MODE):
        step.step(imgs[-1], captions, cap_lens, class_ids)
    torch.cuda.synchronize()
    torch.cuda.set_rng_state(rng, dev)
    handle, info = ctypes.c_void_p(), (ctypes.c_int * 8)()
    rc = lib.sba_replay_create(ctypes.c_void_p(int(graph.raw_cuda_graph())), 1, 0, ctypes.byref(handle))
    if rc != 0:
        return None
    call('sba_replay_info', handle, info)
    call('sba_replay_destroy', handle)
    return dict(zip(INFO_KEYS, list(info)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warm_iters', type=int, default=40)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--images', type=int, default=240, help='synthetic images in the device cache')
    ap.add_argument('--batch', type=int, default=48, help='batch size (cfg/DAMSM/bird.yml itself sets 32)')
    args = ap.parse_args()

    import pretrain_DAMSM
    from miscc import cli
    from miscc.config import cfg, cfg_from_file, reset_cfg
    from model import CNN_ENCODER, RNN_ENCODER
    from sbagan import ops
    from sbagan.damsm import DAMSMSlotStep, DAMSMStep
    from sbagan.device_data import DeviceBatchLoader, DeviceImageCache
    reset_cfg()
    cfg_from_file(os.path.join(PKG, 'cfg', 'DAMSM', 'bird.yml'))
    cfg.TRAIN.NET_E, cfg.CUDA, cfg.GPU_ID, cfg.TRAIN.BATCH_SIZE = '', True, 0, args.batch
    ops.set_compute_dtype(torch.bfloat16)
    dev = torch.device('cuda', 0)
    torch.manual_seed(1)
    B, imsize, W = cfg.TRAIN.BATCH_SIZE, cli.image_size(), cfg.TEXT.WORDS_NUM
    side = int(imsize * 76 / 64)
    say('device %s | torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    say('pretrain_DAMSM.train at cfg/DAMSM/bird.yml sizes: B = %d, %d px, WORDS_NUM %d, bf16, random encoders, synthetic '
        'cache of %d images; ms per iteration over %d iterations after %d, %d alternated rounds'
        % (B, imsize, W, args.images, args.iters, args.warm_iters, args.rounds))
    rng = np.random.RandomState(1)
    arrays = [rng.randint(0, 256, (side, side + 7 * (i % 5), 3)).astype(np.uint8) for i in range(args.images)]
    ds = SynthCaptions(args.images, W, 5450)
    cache = DeviceImageCache.from_arrays(arrays, dev)
    loader = DeviceBatchLoader(ds, cache, B, imsize, cfg.TREE.BRANCH_NUM, seed=1)
    labels = torch.arange(B, dtype=torch.int64, device=dev)
    image_dir = tempfile.mkdtemp(prefix='sbagan_damsm_replay_')

    def build(make):
        text = RNN_ENCODER(ds.n_words, nhidden=cfg.TEXT.EMBEDDING_DIM).to(dev)
        enc = CNN_ENCODER(cfg.TEXT.EMBEDDING_DIM).to(dev)
        return text, enc, make(text, enc)

    arms = {
        '--device_data --replay': build(lambda t, e: DAMSMSlotStep(t, e, B, imsize, lr=cfg.TRAIN.ENCODER_LR,
                                                                   levels=cfg.TREE.BRANCH_NUM)),
        '--device_data': build(lambda t, e: DAMSMStep(t, e, B, lr=cfg.TRAIN.ENCODER_LR)),
    }
    out = {name: [] for name in arms}
    for r in range(args.rounds):
        for name, (text, enc, step) in arms.items():
            loader.bind(step.slot if hasattr(step, 'slot') else None)
            timed = Timed(loader, args.warm_iters, args.iters)
            step.set_lr(cfg.TRAIN.ENCODER_LR * 0.98 ** r)
            pretrain_DAMSM.train(timed, enc, text, B, labels, step, r, ds.ixtoword, image_dir,
                                 max_steps=args.warm_iters + args.iters + 1)
            torch.cuda.synchronize()
            out[name].append(timed.ms)
    loader.bind(None)
    say()
    for name, ms in out.items():
        say('    %-24s %7.2f ms / iteration = %6.0f images/s   (runs: %s)'
            % (name, float(np.median(ms)), B * 1e3 / float(np.median(ms)), ' '.join('%.2f' % v for v in ms)))
    pairs = list(zip(out['--device_data --replay'], out['--device_data']))
    wins = sum(1 for a, b in pairs if a < b)
    say('    --replay faster than the eager loop in %d of %d alternated pairs; median margin %.2f ms (%.1f %%)'
        % (wins, len(pairs), float(np.median([b - a for a, b in pairs])),
           100.0 * float(np.median([(b - a) / b for a, b in pairs]))))
    slot_step = arms['--device_data --replay'][2]
    if slot_step.recording is None:
        say('    the update could NOT be recorded: the --replay arm ran its eager fallback')
    else:
        say('    the recording: %s; %d launches of it in this run'
            % (', '.join('%d %s' % (slot_step.info[k], k) for k in INFO_KEYS), slot_step.launched))
    try:
        eager = count_eager_launches(arms['--device_data'][2], next(iter(loader)))
        say('    one eager update (DAMSMStep.step, captured once to count, never launched): %s'
            % ('not countable' if eager is None else ', '.join('%d %s' % (eager[k], k) for k in INFO_KEYS[:4])))
    except Exception as e:      # (the count is an extra: the timings above stand without it)
        say('    one eager update: not counted (%s: %s)' % (type(e).__name__, e))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
