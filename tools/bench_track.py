#!/usr/bin/env python3
"""--track: what an evaluation in training costs, next to the only route there was before it (one sampling() process per
checkpoint), and what it does to the replayed step.  One MI355X, synthetic data at the CUB sizes: 2 933 held-out images
(10 captions each), 256 px, B = 20, bf16, random encoders and generator, --kid --prdc 5 --fid --r_precision 100.

    (a) track      a training process (2 steps an epoch, 1 epoch) with --track 1: the once-per-run preparation, and of the
                   SECOND evaluation (the first carries the warm-up of every kernel) generation + trunk, the evaluators'
                   result() in all and each, and FID's host part (fid_from_stats: the eigensolves)
    (b) sampling   sampling() in a fresh process on the checkpoint the track arm wrote, same flags: the whole call, the
                   evaluators' set-up (Suite.attach: the caption pool, a second image encoder), Suite.finish and FID's
                   host part; the rest is the loop -- generation, both trunk passes, one PNG per caption through PIL
    (c) replay     --device_data --replay over 200 training images (10 steps an epoch, 25 epochs) with --track 12
                   (--kid --prdc 5 on the first 400 held-out images) and without: ms per step over the 60-step windows
                   [10, 70) [70, 130) [130, 190) [190, 250); with the flag, evaluations sit at steps 10, 130 and 250, so
                   the first and third window start right behind one (and its resync), the second and fourth end in front of one

One fresh process per arm, the arms of a pair alternated, `--pairs` (3) pairs; medians.  Nothing is asserted.

    python tools/bench_track.py [--pairs 3] [--work DIR] [--out FILE]
"""
import argparse
import json
import os
import pickle
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'sba-gan_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

N_TEST, N_TRAIN, PER_IMAGE, BATCH, SIZE = 2933, 200, 10, 20, 256
FLAGS = dict(kid=True, prdc=5, fid=True, r_precision=100)
WINDOW, FIRST, WINDOWS = 60, 10, 4
CHILD_TIMEOUT = 900


def make_dataset(root):
    """a CUB-shaped directory of smooth random images (330 x 300) with 10 captions of 5 to 18 words each"""
    from PIL import Image
    rng = np.random.RandomState(0)
    words = ['w%d' % i for i in range(300)]
    for sub in ('images/cls', 'text/cls', 'train', 'test'):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    names = {'train': ['cls/a%d' % i for i in range(N_TRAIN)], 'test': ['cls/t%d' % i for i in range(N_TEST)]}
    for split, keys in names.items():
        with open(os.path.join(root, split, 'filenames.pickle'), 'wb') as f:
            pickle.dump(keys, f)
        with open(os.path.join(root, split, 'class_info.pickle'), 'wb') as f:
            pickle.dump([1 + i % 50 for i in range(len(keys))], f)
        for k in keys:
            small = Image.fromarray(rng.randint(0, 255, (10, 11, 3)).astype(np.uint8))
            small.resize((330, 300), Image.BILINEAR).save(os.path.join(root, 'images', k + '.jpg'))
            with open(os.path.join(root, 'text', k + '.txt'), 'w') as f:
                for _ in range(PER_IMAGE):
                    f.write(' '.join(words[rng.randint(0, len(words))] for _ in range(rng.randint(5, 19))) + '\n')


def configure(root, training, max_epoch=1, net_g=''):
    import torch
    from miscc.config import cfg, reset_cfg
    from sbagan import ops
    reset_cfg()
    cfg.DATA_DIR, cfg.TREE.BRANCH_NUM, cfg.TREE.BASE_SIZE = root, 3, 64
    cfg.GAN.GF_DIM, cfg.GAN.DF_DIM, cfg.GAN.R_NUM = 32, 64, 2             # (cfg/bird_style.yml)
    s = cfg.TRAIN.SMOOTH
    s.GAMMA1, s.GAMMA2, s.GAMMA3, s.LAMBDA = 4.0, 5.0, 10.0, 5.0
    cfg.TEXT.CAPTIONS_PER_IMAGE, cfg.TEXT.EMBEDDING_DIM = PER_IMAGE, 256
    cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.MAX_EPOCH, cfg.TRAIN.SNAPSHOT_INTERVAL = BATCH, max_epoch, max(max_epoch, 1)
    cfg.TRAIN.NET_E, cfg.TRAIN.NET_G, cfg.TRAIN.FLAG, cfg.CUDA, cfg.GPU_ID, cfg.B_VALIDATION = '', net_g, training, True, 0, True
    ops.set_compute_dtype(torch.bfloat16)
    for seeder in (np.random.seed, torch.manual_seed, torch.cuda.manual_seed_all):
        seeder(100)
    return cfg


def host_loader(root, split):
    import datasets
    import torch
    from miscc import transforms
    tfm = transforms.Compose([transforms.Resize(int(SIZE * 76 / 64)), transforms.RandomCrop(SIZE),
                              transforms.RandomHorizontalFlip()])
    ds = datasets.TextDataset(root, split, base_size=64, transform=tfm)
    if split == 'train':
        ds.filenames, ds.number_example = ds.filenames[:2 * BATCH], 2 * BATCH       # (two steps an epoch)
    return ds, torch.utils.data.DataLoader(ds, batch_size=BATCH, drop_last=True, shuffle=True, num_workers=0)


def time_fid_host():
    """the seconds of every sbagan.fid.fid_from_stats call from now on"""
    import sbagan.fid as F
    spent, plain = [], F.fid_from_stats

    def timed(*a):
        t = time.time()
        out = plain(*a)
        spent.append(time.time() - t)
        return out
    F.fid_from_stats = timed
    return spent


def arm_track(root, out_dir):
    import torch
    from trainer import condGANTrainer
    configure(root, True)
    ds, loader = host_loader(root, 'train')
    algo = condGANTrainer(out_dir, loader, ds.n_words, ds.ixtoword, allow_random_encoders=True)
    for k, v in FLAGS.items():
        setattr(algo, k, v)
    algo.track = 1
    fid_host = time_fid_host()
    t0 = time.time()
    algo.train()
    torch.cuda.synchronize()
    tk = algo.tracker
    first, second = tk.records
    return {'process_s': time.time() - t0, 'prepare_s': tk.timing['prepare'], 'first_evaluation_s': first['seconds'],
            'evaluation_s': second['seconds'], 'generate_trunk_s': tk.timing['generate'], 'results_s': tk.timing['results'],
            'result_of_s': tk.timing['result_of'], 'fid_host_s': fid_host[-1], 'images': tk.images,
            'checkpoint': os.path.join(out_dir, 'Model', second['checkpoint']),
            'figures': {k: second['metrics'][k.split('.')[0]][k.split('.')[1]] for k in
                        ('kid.kid', 'fid.fid', 'prdc.coverage', 'r_precision.r_at_1')}}


def arm_sampling(root, checkpoint):
    import torch
    from sbagan import evaluation
    from trainer import condGANTrainer
    configure(root, False, net_g=checkpoint)
    ds, loader = host_loader(root, 'test')
    algo = condGANTrainer(os.path.dirname(checkpoint), loader, ds.n_words, ds.ixtoword, allow_random_encoders=True)
    for k, v in FLAGS.items():
        setattr(algo, k, v)
    fid_host = time_fid_host()
    parts = {}

    def timed(name):
        plain = getattr(evaluation.Suite, name)

        def run(self, *a):
            torch.cuda.synchronize()
            t = time.time()
            out = plain(self, *a)
            torch.cuda.synchronize()
            parts[name] = time.time() - t
            return out
        setattr(evaluation.Suite, name, run)
    timed('attach')
    timed('finish')
    t0 = time.time()
    algo.sampling('test')
    torch.cuda.synchronize()
    total = time.time() - t0
    return {'sampling_s': total, 'attach_s': parts['attach'], 'finish_s': parts['finish'], 'fid_host_s': fid_host[-1],
            'loop_s': total - parts['attach'] - parts['finish'], 'images': len(loader) * BATCH,
            'figures': {'kid.kid': algo.kid_result['kid'], 'fid.fid': algo.fid_result['fid']}}


def arm_replay(root, out_dir, track):
    import datasets
    import torch
    from sbagan import static_batch
    from sbagan.device_data import DeviceBatchLoader, DeviceImageCache
    from trainer import condGANTrainer
    epochs = (FIRST + WINDOW * WINDOWS) // (N_TRAIN // BATCH)
    configure(root, True, max_epoch=epochs)
    ds = datasets.TextDataset(root, 'train', base_size=64, transform=None)
    dev = torch.device('cuda', 0)
    cache = DeviceImageCache(ds, int(SIZE * 76 / 64), dev, max_bytes=4 << 30, workers=0)
    loader = DeviceBatchLoader(ds, cache, BATCH, SIZE, 3, seed=100)
    algo = condGANTrainer(out_dir, loader, ds.n_words, ds.ixtoword, allow_random_encoders=True)
    algo.replay, algo.kid, algo.prdc = True, True, 5
    algo.track, algo.track_n = (12, 400) if track else (0, 0)
    starts, ends, plain, n = {}, {}, static_batch.SlotStep.train, [0]

    def train(self):
        if (n[0] - FIRST) % WINDOW == 0:
            torch.cuda.synchronize()
            starts[n[0]] = time.time()
        out = plain(self)
        n[0] += 1
        if (n[0] - FIRST) % WINDOW == 0:
            torch.cuda.synchronize()
            ends[n[0]] = time.time()
        return out
    static_batch.SlotStep.train = train
    algo.train()
    torch.cuda.synchronize()
    lo = [FIRST + WINDOW * w for w in range(WINDOWS)]
    return {'steps': n[0], 'recorded': algo.slot_step.recording is not None,
            'window_ms_per_step': [1e3 * (ends[s + WINDOW] - starts[s]) / WINDOW for s in lo],
            'evaluations': [[r['epoch'], r['iteration'], r['seconds']] for r in algo.tracker.records] if track else []}


def child(args):
    if args.arm == 'track':
        res = arm_track(args.root, args.dir)
    elif args.arm == 'sampling':
        res = arm_sampling(args.root, args.checkpoint)
    else:
        res = arm_replay(args.root, args.dir, args.arm == 'replay_track')
    with open(args.result, 'w') as f:
        json.dump(res, f)


def run_child(work, tag, arm, **kw):
    """one arm in a fresh process, under its own time limit; a failure ends the bench"""
    result = os.path.join(work, tag + '.json')
    d = os.path.join(work, tag)
    os.makedirs(d, exist_ok=True)
    cmd = [sys.executable, os.path.abspath(__file__), '--arm', arm, '--root', os.path.join(work, 'data'), '--dir', d,
           '--result', result] + [x for k, v in kw.items() for x in ('--' + k, v)]
    with open(os.path.join(work, tag + '.log'), 'w') as log:
        subprocess.run(cmd, stdout=log, stderr=subprocess.STDOUT, timeout=CHILD_TIMEOUT, check=True)
    with open(result) as f:
        return json.load(f)


def median_of(runs, key):
    vals = [r[key] for r in runs]
    if isinstance(vals[0], dict):
        return {k: median_of(vals, k) for k in vals[0]}
    if isinstance(vals[0], list):
        return [float(np.median(col)) for col in zip(*vals)]
    return float(np.median(vals))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=3)
    ap.add_argument('--work', default='')
    ap.add_argument('--out', default='')
    ap.add_argument('--skip_replay', action='store_true')
    for name in ('arm', 'root', 'dir', 'result', 'checkpoint'):
        ap.add_argument('--' + name, default='')
    args = ap.parse_args()
    if args.arm:
        return child(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_track.py measures on the GPU: no device visible')
    work = args.work or tempfile.mkdtemp(prefix='bench_track_')
    if not os.path.isdir(os.path.join(work, 'data')):
        make_dataset(os.path.join(work, 'data'))
    track, sampling, with_flag, without = [], [], [], []
    for i in range(args.pairs):
        track.append(run_child(work, 'track%d' % i, 'track'))
        print('track', json.dumps(track[-1]), flush=True)
        sampling.append(run_child(work, 'sampling%d' % i, 'sampling', checkpoint=track[-1]['checkpoint']))
        print('sampling', json.dumps(sampling[-1]), flush=True)
    if not args.skip_replay:
        for i in range(args.pairs):
            with_flag.append(run_child(work, 'replay_track%d' % i, 'replay_track'))
            print('replay_track', json.dumps(with_flag[-1]), flush=True)
            without.append(run_child(work, 'replay_plain%d' % i, 'replay_plain'))
            print('replay_plain', json.dumps(without[-1]), flush=True)
    res = {'device': torch.cuda.get_device_name(0), 'pairs': args.pairs, 'images': N_TEST, 'size': SIZE, 'batch': BATCH,
           'dtype': 'bfloat16', 'flags': FLAGS, 'workers': 0,
           'track': {k: median_of(track, k) for k in ('prepare_s', 'first_evaluation_s', 'evaluation_s', 'generate_trunk_s',
                                                       'results_s', 'result_of_s', 'fid_host_s')},
           'sampling': {k: median_of(sampling, k) for k in ('sampling_s', 'attach_s', 'loop_s', 'finish_s', 'fid_host_s')},
           'sampling_images': sampling[0]['images'], 'runs': {'track': track, 'sampling': sampling}}
    res['sampling_over_track_evaluation'] = res['sampling']['sampling_s'] / res['track']['evaluation_s']
    res['fid_host_share_of_evaluation'] = res['track']['fid_host_s'] / res['track']['evaluation_s']
    if with_flag:
        res['replay'] = {'window': WINDOW, 'windows_start_at_step': [FIRST + WINDOW * w for w in range(WINDOWS)],
                         'evaluations_at_step': [10, 130, 250], 'track_n': 400,
                         'with_track_ms_per_step': [r['window_ms_per_step'] for r in with_flag],
                         'without_ms_per_step': [r['window_ms_per_step'] for r in without],
                         'with_track_median': median_of(with_flag, 'window_ms_per_step'),
                         'without_median': median_of(without, 'window_ms_per_step'),
                         'recorded': all(r['recorded'] for r in with_flag + without),
                         'evaluations': with_flag[0]['evaluations']}
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
