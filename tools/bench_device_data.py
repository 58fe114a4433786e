#!/usr/bin/env python3
"""--device_data measured (run alone on the GPU, profiler off).

  (a) the kernel alone, by device events: us per sba_batch_pyramid launch at B = 20, T = 256, levels = 3 (the GAN batch)
      and B = 48, T = 299, levels = 1 (the DAMSM batch), and the algorithmic bytes B T^2 3 + 12 B sum_l T_l^2 over that
      time beside the 6.3 TB/s the project's streaming kernels reach;
  (b) batches/s of DeviceBatchLoader alone against the torch DataLoader + prepare_data at WORKERS 4 and 16, on a seeded
      synthetic CUB-shaped directory of 1000 JPEGs (500 x 375, with boxes), the paths alternated in the same call;
  (c) ms per iteration of condGANTrainer.train on that directory at the bird_style sizes with random encoders: with
      --device_data --replay (the loop through one recording of the step), with --device_data alone and
      with neither, alternated; and the node and stream counts of the recording.

Every window is at least 200 batches (300 iterations in (c)) after a warm-up and ends in a device synchronise.

    python tools/bench_device_data.py [--parts abc] [--dir DIR] [--out profiles/device_data.txt]
"""
import argparse
import os
import subprocess
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

ACHIEVABLE_TBS = 6.3
LINES = []


def say(text=''):
    print(text, flush=True)
    LINES.append(text)


def make_directory(root, n=1000, seed=0):
    """<root>/birds: n JPEGs of 500 x 375 (smooth colour fields + noise), CUB's box / name files, 10 captions each"""
    import pickle
    from PIL import Image
    data_dir = os.path.join(root, 'birds')
    if os.path.isfile(os.path.join(data_dir, 'train', 'filenames.pickle')):
        return data_dir
    rng = np.random.RandomState(seed)
    cub = os.path.join(data_dir, 'CUB_200_2011', 'CUB_200_2011')
    for d in (os.path.join(cub, 'images', 'cls'), os.path.join(data_dir, 'text', 'cls'), os.path.join(data_dir, 'train'),
              os.path.join(data_dir, 'test')):
        os.makedirs(d, exist_ok=True)
    words = ['bird', 'red', 'small', 'wing', 'blue', 'beak', 'long', 'white', 'yellow', 'belly', 'tail', 'black']
    keys = ['cls/img%04d' % i for i in range(n)]
    with open(os.path.join(cub, 'images.txt'), 'w') as fi, open(os.path.join(cub, 'bounding_boxes.txt'), 'w') as fb:
        for i, k in enumerate(keys):
            low = Image.fromarray(rng.randint(0, 256, (12, 16, 3)).astype(np.uint8)).resize((500, 375), Image.BICUBIC)
            img = np.asarray(low).astype(np.int16) + rng.randint(-12, 13, (375, 500, 3))
            Image.fromarray(img.clip(0, 255).astype(np.uint8)).save(os.path.join(cub, 'images', k + '.jpg'), quality=90)
            w, h = rng.randint(150, 400), rng.randint(120, 300)
            x, y = rng.randint(0, 500 - w), rng.randint(0, 375 - h)
            fi.write('%d %s.jpg\n' % (i + 1, k))
            fb.write('%d %d.0 %d.0 %d.0 %d.0\n' % (i + 1, x, y, w, h))
            with open(os.path.join(data_dir, 'text', k + '.txt'), 'w') as f:
                for _ in range(10):
                    f.write('the ' + ' '.join(words[rng.randint(0, len(words))] for _ in range(3 + rng.randint(0, 9))) + '\n')
    for split, names in (('train', keys), ('test', keys[:20])):
        with open(os.path.join(data_dir, split, 'filenames.pickle'), 'wb') as f:
            pickle.dump(names, f)
        with open(os.path.join(data_dir, split, 'class_info.pickle'), 'wb') as f:
            pickle.dump([1 + i % 200 for i in range(len(names))], f)
    return data_dir


def part_a(args):
    """the raw C entry on preallocated outputs (no validation, no allocation in the loop).  A launch this short can be
    bounded by how fast the host issues it, so the host's own time per call (the same loop, clocked on the host before
    the synchronise) is printed beside the device time: where the two are equal the figure is the issue rate."""
    from sbagan import _lib, ops
    from sbagan.device_data import DeviceImageCache, pyramid_tables
    dev = torch.device('cuda', 0)
    say('(a) sba_batch_pyramid alone, device events, %d launches per window, %d windows' % (args.launches, args.windows))
    rng = np.random.RandomState(1)
    for B, T, levels, side in ((20, 256, 3, 304), (48, 299, 1, 355)):
        arrays = [rng.randint(0, 256, (side, side + 7 * (i % 5), 3)).astype(np.uint8) for i in range(64)]
        cache = DeviceImageCache.from_arrays(arrays, dev)
        params = np.stack([rng.randint(0, 64, B), rng.randint(0, side - T + 1, B), rng.randint(0, side - T + 1, B),
                           rng.randint(0, 2, B)], 1).astype(np.int32)
        outs = ops.batch_pyramid(cache, params, T, levels)             # (validates the rows once)
        p_dev = torch.from_numpy(params).to(dev)
        tab1, tab2, lut = pyramid_tables(T, levels, dev)
        ptr = [t.data_ptr() if t is not None else None for t in (tab1, tab2, lut)] + \
              [outs[l].data_ptr() if l < levels else None for l in range(3)]
        st = torch.cuda.current_stream().cuda_stream
        fixed = (cache.data.data_ptr(), cache.offset.data_ptr(), cache.hw.data_ptr(), len(cache), p_dev.data_ptr(), B, T,
                 levels) + tuple(ptr) + (st,)
        entry = _lib.lib.sba_batch_pyramid

        def window():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            t0 = time.perf_counter()
            for _ in range(args.launches):
                entry(*fixed)
            host = (time.perf_counter() - t0) * 1e6 / args.launches
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e3 / args.launches, host

        window()
        torch.cuda.synchronize()
        got = [window() for _ in range(args.windows)]
        us, host = [g[0] for g in got], [g[1] for g in got]
        nbytes = B * T * T * 3 + 12 * B * sum((T >> l) ** 2 for l in range(levels))
        med = float(np.median(us))
        say('    B = %2d T = %3d levels = %d: %7.2f us / launch (median of %d windows, min %.2f, max %.2f; host issue '
            '%.2f us / call), %.1f MB algorithmic = %.2f TB/s (achievable %.1f TB/s)'
            % (B, T, levels, med, len(us), min(us), max(us), float(np.median(host)), nbytes / 1e6, nbytes / med / 1e6,
               ACHIEVABLE_TBS))


def _style_cfg(data_dir, workers):
    from miscc.config import cfg, cfg_from_file, reset_cfg
    reset_cfg()
    cfg_from_file(os.path.join(PKG, 'cfg', 'bird_style.yml'))
    cfg.DATA_DIR, cfg.WORKERS, cfg.TRAIN.NET_E, cfg.TRAIN.NET_G, cfg.TRAIN.B_NET_D = data_dir, workers, '', '', False
    cfg.TRAIN.SNAPSHOT_INTERVAL, cfg.TRAIN.MAX_EPOCH, cfg.CUDA, cfg.GPU_ID = 100000, 100000, True, 0
    return cfg


def _dataset(data_dir):
    import datasets
    from miscc import cli, transforms
    imsize = cli.image_size()
    tf = transforms.Compose([transforms.Resize(int(imsize * 76 / 64)), transforms.RandomCrop(imsize),
                             transforms.RandomHorizontalFlip()])
    return datasets.TextDataset(data_dir, 'train', base_size=64, transform=tf), imsize


def _batches(loader):
    """endless batches of a loader, epoch after epoch, prepared"""
    import datasets
    while True:
        for data in loader:
            yield datasets.as_batch(data)


def part_b(args, data_dir):
    from sbagan import device_data
    say('(b) loader alone, batches/s of 20 images (3 scales, 256 px), windows of %d batches after %d, alternated'
        % (args.batches, args.warm_batches))
    cfg = _style_cfg(data_dir, 4)
    ds, imsize = _dataset(data_dir)
    # the DataLoader workers are started first, before this process touches the device (persistent: they are not
    # restarted per epoch as the entry points' loader is, which favours the DataLoader)
    sources = {}
    for w in (4, 16):
        loader = torch.utils.data.DataLoader(ds, batch_size=cfg.TRAIN.BATCH_SIZE, drop_last=True, shuffle=True,
                                             num_workers=w, persistent_workers=True)
        iter(loader)                                  # the workers start here and stay
        sources['DataLoader WORKERS %d' % w] = _batches(loader)
    t0 = time.perf_counter()
    dev_loader = device_data.from_cfg(ds, imsize, seed=1, gb=4.0)
    torch.cuda.synchronize()
    say('    cache: %d images, %.1f MiB, built in %.1f s with WORKERS %d'
        % (len(dev_loader.cache), dev_loader.cache.nbytes / 2.0 ** 20, time.perf_counter() - t0, int(cfg.WORKERS)))
    sources = dict([('device_data', _batches(dev_loader))] + list(sources.items()))
    rates = {k: [] for k in sources}
    for name, it in sources.items():
        for _ in range(args.warm_batches):
            next(it)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, it in sources.items():
            t0 = time.perf_counter()
            for _ in range(args.batches):
                next(it)
            torch.cuda.synchronize()
            rates[name].append(args.batches / (time.perf_counter() - t0))
    for name, r in rates.items():
        say('    %-22s %9.1f batches/s = %9.0f images/s   (windows: %s)'
            % (name, float(np.median(r)), 20 * float(np.median(r)), ' '.join('%.1f' % v for v in r)))
    return 20 * float(np.median(rates['device_data']))


class _Timed(object):
    """hands a loader's batches to the trainer and times iterations [warm, warm + steps) between two synchronises"""

    def __init__(self, loader, warm, steps):
        self.loader, self.warm, self.steps, self.n, self.t0, self.ms = loader, warm, steps, 0, None, None
        self.dataset = getattr(loader, 'dataset', None)

    def __len__(self):
        return len(self.loader)

    def __getattr__(self, name):        # drop_last, crop, bind, slot: what the trainer asks its loader
        return getattr(self.loader, name)

    def __iter__(self):
        for data in self.loader:
            if self.n == self.warm:
                torch.cuda.synchronize()
                self.t0 = time.perf_counter()
            elif self.n == self.warm + self.steps:
                torch.cuda.synchronize()
                self.ms = (time.perf_counter() - self.t0) * 1e3 / self.steps
            self.n += 1
            yield data


def part_c(args, data_dir):
    from sbagan import device_data, ops
    from trainer import condGANTrainer
    say('(c) condGANTrainer.train, bird_style sizes (B = 20, 3 stages, 256 px, bf16), random encoders: ms per iteration over '
        '%d iterations after %d, alternated' % (args.iters, args.warm_iters))
    cfg = _style_cfg(data_dir, 4)
    ops.set_compute_dtype(torch.bfloat16)
    ds, imsize = _dataset(data_dir)
    dev_loader = device_data.from_cfg(ds, imsize, seed=1, gb=4.0)
    pil_loader = torch.utils.data.DataLoader(ds, batch_size=cfg.TRAIN.BATCH_SIZE, drop_last=True, shuffle=True,
                                             num_workers=int(cfg.WORKERS))
    arms = (('--device_data --replay', dev_loader, True), ('--device_data', dev_loader, False),
            ('DataLoader WORKERS 4', pil_loader, False))
    out = {name: [] for name, _, _ in arms}
    info = None
    for r in range(args.rounds):
        for name, loader, replay in arms:
            timed = _Timed(loader, args.warm_iters, args.iters)
            algo = condGANTrainer(os.path.join(args.dir, 'out_%d' % r), timed, ds.n_words, ds.ixtoword,
                                  allow_random_encoders=True)
            algo.replay = replay
            algo.train(max_steps=args.warm_iters + args.iters + 1)
            out[name].append(timed.ms)
            if replay:
                rec = algo.slot_step.recording
                info = None if rec is None else dict(rec.info)
            del algo
    for name, ms in out.items():
        say('    %-22s %7.2f ms / iteration = %6.0f images/s   (runs: %s)'
            % (name, float(np.median(ms)), 20e3 / float(np.median(ms)), ' '.join('%.2f' % v for v in ms)))
    pairs = list(zip(out['--device_data --replay'], out['--device_data']))
    say('    --replay faster than the eager loop in %d of %d alternated pairs'
        % (sum(1 for a, b in pairs if a < b), len(pairs)))
    if info is None:
        say('    the step could NOT be recorded: the --replay arm ran its eager fallback')
    else:
        say('    the recording (prologue + step): %s' % ', '.join('%d %s' % (info[k], k) for k in (
            'nodes', 'kernels', 'copies', 'memsets', 'streams', 'waits', 'events', 'host_calls')))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', default='abc')
    ap.add_argument('--dir', default=os.path.join(tempfile.gettempdir(), 'sbagan_device_data_bench'))
    ap.add_argument('--out', default=None)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--windows', type=int, default=10)
    ap.add_argument('--batches', type=int, default=200)
    ap.add_argument('--warm_batches', type=int, default=20)
    ap.add_argument('--iters', type=int, default=300)
    ap.add_argument('--warm_iters', type=int, default=60, help='past the first epoch (50 batches) and its checkpoint')
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--step_images_per_s', type=float, default=None,
                    help='images/s bench.py printed for the step in the same session: (b) is held against it')
    args = ap.parse_args()
    if len(args.parts) > 1:
        # one fresh process per part: (b) starts its DataLoader workers before the process touches the device
        passed = [a for a in sys.argv[1:]]
        for flag in ('--parts', '--out'):
            if flag in passed:
                i = passed.index(flag)
                del passed[i:i + 2]
        for part in args.parts:
            tmp = os.path.join(tempfile.gettempdir(), 'sbagan_device_data_part_%s_%d.txt' % (part, os.getpid()))
            subprocess.check_call([sys.executable, os.path.abspath(__file__), '--parts', part, '--out', tmp] + passed)
            with open(tmp) as f:
                LINES.extend(f.read().splitlines())
            os.remove(tmp)
    else:
        data_dir = None
        if args.parts in ('b', 'c'):
            t0 = time.perf_counter()
            data_dir = make_directory(args.dir)
            say('synthetic directory: 1000 JPEGs 500 x 375 with boxes (%.1f s)' % (time.perf_counter() - t0))
        if args.parts == 'a':
            say('device %s | torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
            part_a(args)
        elif args.parts == 'b':
            rate = part_b(args, data_dir)
            if args.step_images_per_s:
                say('    the step consumes %.0f images/s (bench.py, same session): the device loader delivers %.1f x that'
                    % (args.step_images_per_s, rate / args.step_images_per_s))
        elif args.parts == 'c':
            part_c(args, data_dir)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
