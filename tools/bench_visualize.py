#!/usr/bin/env python3
"""Attention-map overlay grid: sbagan.visualize.build_super_images (HIP expand + compose, one copy of the canvas, PIL
text) against the float64 host reference of the same picture (scipy zoom + gaussian_filter per map, numpy layout, PIL
paste: tests/vis_ref.py) with its 152 expansions spread over 16 threads and its layout on one, at the two dump shapes
of a training run:

    8 samples x 19 maps, 17 -> 272   (D_*.png, attention_maps*.png)
    8 samples x 19 maps, 128 -> 256  (G_*_1.png of a three-stage generator)

One sample = one whole grid, wall clock between device synchronisations (the builder ends with a device-to-host copy);
median and interquartile range.  The device time of the two kernels alone is reported beside it.  Recorded, not
asserted.

    python tools/bench_visualize.py [--reps 10] [--warmup 2] [--out profiles/vis_bench.json]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'sba-gan_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

THREADS = 16


def _stats(t):
    q1, med, q3 = np.percentile(t, [25, 50, 75])
    return dict(median_ms=float(med), iqr_ms=float(q3 - q1), min_ms=float(min(t)), n=len(t))


def host_grid(imgs, maps, a, T, colours, pool):
    """One grid of the float64 reference: the 152 expansions are mapped over the thread pool ONCE and handed to
    vis_ref.grid, which then only normalises, pastes and lays out, on one thread.  Returns the seconds of (the pooled
    expansions, the layout, both)."""
    import vis_ref
    up = (16 * a if a == 17 else imgs.shape[2]) // a
    stacks = [vis_ref.grid_stack(m) for m in maps]
    flat = [s for st in stacks for s in st]
    t0 = time.perf_counter()
    done = list(pool.map(lambda s: vis_ref.expand(s, up), flat))
    t_expand = time.perf_counter() - t0
    first = np.cumsum([0] + [len(st) for st in stacks])
    expanded = [done[first[i]:first[i + 1]] for i in range(len(stacks))]
    t1 = time.perf_counter()
    vis_ref.grid(imgs, maps, a, T, colours, expanded=expanded)
    t2 = time.perf_counter()
    return t_expand, t2 - t1, t2 - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--host-reps', type=int, default=2)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_visualize.py measures on the GPU: no device visible')
    from miscc.config import cfg
    from sbagan import ops
    from sbagan.visualize import _device_operator, build_super_images, word_colours
    dev = torch.device('cuda:0')
    cfg.TEXT.WORDS_NUM = 18
    ixtoword = {i: 'word%d' % i for i in range(32)}
    rng = np.random.RandomState(0)
    caps = rng.randint(1, 32, size=(8, 18))
    pool = ThreadPoolExecutor(THREADS)
    res = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup, host_threads=THREADS, shapes={})
    for name, a, S in (('17_to_272', 17, 272), ('128_to_256', 128, 256)):
        V = 16 * a if a == 17 else S
        imgs = (rng.rand(8, 3, S, S) * 2 - 1).astype(np.float32)
        maps = rng.rand(8, 18, a, a).astype(np.float32) ** 6
        maps /= maps.reshape(8, 18, -1).sum(2).reshape(8, 18, 1, 1)
        imgs_d, maps_d = torch.from_numpy(imgs).to(dev), torch.from_numpy(maps).to(dev)
        times = []
        for k in range(args.warmup + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            build_super_images(imgs_d, caps, ixtoword, maps_d, a)
            torch.cuda.synchronize()
            if k >= args.warmup:
                times.append((time.perf_counter() - t0) * 1e3)
        # the expand launch alone, by device events
        x = torch.cat([torch.cat([m.amax(0, keepdim=True), m], 0) for m in maps_d], 0).contiguous()
        M = _device_operator(a, V, dev)
        ev = []
        for k in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.vis_expand(x, M)
            e1.record()
            e1.synchronize()
            if k >= args.warmup:
                ev.append(e0.elapsed_time(e1))
        host, host_expand, host_layout = [], [], []
        for _ in range(args.host_reps):
            te, tl, tt = host_grid(imgs, list(maps), a, 18, word_colours(20)[:18], pool)
            host.append(tt * 1e3)
            host_expand.append(te * 1e3)
            host_layout.append(tl * 1e3)
        res['shapes'][name] = dict(samples=8, maps=int(x.shape[0]), a=a, V=V, gpu_grid=_stats(times),
                                   gpu_expand_launch=_stats(ev), host_float64_expand_pooled=_stats(host_expand),
                                   host_float64_layout_one_thread=_stats(host_layout),
                                   host_float64_grid=_stats(host))
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
