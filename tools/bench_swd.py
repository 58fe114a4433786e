#!/usr/bin/env python3
"""Sliced Wasserstein distance: SWD.result() at the real shape -- 2933 images of 256 px a side (a CUB test split), 128
patches an image, 5 levels, 512 directions -- next to the float64 device route in torch for the same figures:

    hip      SWD.result(): per level and side sba_swd_descriptors (pyramid in LDS), sba_swd_project (f64 matrix
             instruction, direction-major), sba_swd_sort_columns (LDS tiles + merge passes), then sba_swd_abs_mean; one
             descriptor buffer and three projection buffers, allocated once
    torch    per chunk of images .double(), the Gaussian / Laplacian pyramid by depthwise f64 conv2d on reflect-padded
             maps (computed ONCE per image for all levels), the patches gathered by index; then per level and side
             mean / std over a channel, matmul with the directions, torch.sort along the descriptors, mean |a - b|

in the SAME process on the same images and the same draws, alternated after a warm-up; a sample is one whole evaluation
between two device synchronisations (result() ends in its one read-back).  The per-level figures of the two routes are
compared first.  Peak device memory of each route is torch's peak allocation during one evaluation, the uint8 images of
both sides (resident for both) included.  The stages of the hip route are also timed one by one at level 0 with device
events.  Recorded, not asserted.

    python tools/bench_swd.py [--reps 3] [--warmup 1] [--out profiles/swd_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'sba-gan_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)


def _quartiles(t):
    q1, med, q3 = np.percentile(t, [25, 50, 75])
    return dict(median_ms=float(med), iqr_ms=float(q3 - q1), min_ms=float(min(t)), n=len(t))


def _wall_sample(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def _device_sample(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def images(n, size, seed, dev):
    """uint8 [n][3][size][size]: smooth structure plus noise"""
    g = torch.Generator(device='cpu').manual_seed(seed)
    base = F.interpolate(torch.rand(n, 3, 16, 16, generator=g), size=size, mode='bilinear')
    x = base * 200.0 + torch.rand(n, 3, size, size, generator=g) * 55.0
    return x.to(torch.uint8).to(dev)


def torch_route(sides, draws, patches, chunk):
    """the distance per level (a [L] f64 tensor on the device)"""
    dev = sides[0].device
    k = torch.tensor([1.0, 4.0, 6.0, 4.0, 1.0], dtype=torch.float64, device=dev)
    K = (torch.outer(k, k) / 256.0).view(1, 1, 5, 5).repeat(3, 1, 1, 1)
    L = len(draws)
    r7 = torch.arange(7, device=dev) - 3
    ch = torch.arange(3, device=dev)[None, :, None, None]
    desc = []
    for s, imgs in enumerate(sides):
        n = imgs.shape[0]
        per_level = [torch.empty((n * patches, 147), dtype=torch.float64, device=dev) for _ in range(L)]
        centres = [torch.from_numpy(d[s]).to(dev).long() for d in draws]
        for at in range(0, n, chunk):
            g = imgs[at:at + chunk].double()
            laps = []
            for lv in range(L - 1):
                nxt = F.conv2d(F.pad(g, (2, 2, 2, 2), mode='reflect'), K, stride=2, groups=3)
                z = torch.zeros_like(g)
                z[:, :, ::2, ::2] = nxt
                laps.append(g - F.conv2d(F.pad(z, (2, 2, 2, 2), mode='reflect'), 4.0 * K, groups=3))
                g = nxt
            laps.append(g)
            c = g.shape[0]
            for lv, lap in enumerate(laps):
                cc = centres[lv][at * patches:(at + c) * patches]
                img = (torch.arange(c * patches, device=dev) // patches)[:, None, None, None]
                ys = (cc[:, 1, None] + r7)[:, None, :, None]
                xs = (cc[:, 0, None] + r7)[:, None, None, :]
                per_level[lv][at * patches:(at + c) * patches] = lap[img, ch, ys, xs].reshape(c * patches, 147)
        desc.append(per_level)
    out = torch.empty(L, dtype=torch.float64, device=dev)
    for lv in range(L):
        dirs = torch.from_numpy(draws[lv][2]).to(dev)
        proj = []
        for s in range(2):
            d = desc[s][lv].view(-1, 3, 49)
            d = (d - d.mean(dim=(0, 2), keepdim=True)) / d.std(dim=(0, 2), unbiased=False, keepdim=True)
            proj.append(torch.sort(d.view(-1, 147) @ dirs, dim=0).values)
        out[lv] = (proj[0] - proj[1]).abs().mean(dim=0).mean()
    return out


def stages(ev, draws):
    """device time of the four entry points at level 0, real side (the abs-mean against the same side's own buffer)"""
    from sbagan import ops
    imgs = ev.images('real')
    dev = imgs.device
    m = imgs.shape[0] * 128
    desc = torch.empty((m, ops.SWD_DESC), dtype=torch.float64, device=dev)
    proj, tmp = (torch.empty((512, m), dtype=torch.float64, device=dev) for _ in range(2))
    dirs = torch.from_numpy(draws[0][2]).to(dev)
    out = {}
    stats = ops.swd_descriptors(imgs, 0, draws[0][0], desc=desc)[1]
    torch.cuda.synchronize()
    out['descriptors_ms'] = _device_sample(lambda: ops.swd_descriptors(imgs, 0, draws[0][0], desc=desc))
    out['project_ms'] = _device_sample(lambda: ops.swd_project(desc, stats, dirs, out=proj))
    out['sort_columns_ms'] = _device_sample(lambda: ops.swd_sort_columns(proj, tmp))
    out['abs_mean_ms'] = _device_sample(lambda: ops.swd_abs_mean(proj, tmp))
    return out


def bench(n, size, reps, warmup, chunk):
    from sbagan import swd
    dev = torch.device('cuda:0')
    real, fake = images(n, size, 1, dev), images(n, size, 2, dev)
    ev = swd.SWD(n, size=size)
    ev._held = {'real': [real, n], 'fake': [fake, n]}          # (the stacks are uint8 already)
    draws = swd.draw(100, size, n)

    def hip():
        return np.array(ev.result()['swd_x1e3']) / 1e3

    def route():
        return torch_route((real, fake), draws, swd.PATCHES, chunk).cpu().numpy()
    fns = {'hip': hip, 'torch': route}
    out, peak, values = {}, {}, {}
    for k, f in fns.items():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        values[k] = f()
        torch.cuda.synchronize()
        peak[k] = int(torch.cuda.max_memory_allocated())
    out['swd_hip'], out['swd_torch'] = values['hip'].tolist(), values['torch'].tolist()
    out['max_abs_diff_hip_vs_torch_f64'] = float(np.abs(values['hip'] - values['torch']).max())
    for _ in range(warmup):
        for f in fns.values():
            f()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            times[k].append(_wall_sample(f)[0])
    for k, t in times.items():
        out[k] = _quartiles(t)
    out['torch_over_hip'] = out['torch']['median_ms'] / out['hip']['median_ms']
    m = n * swd.PATCHES
    out.update(n=n, size=size, levels=ev.levels, patches_per_image=swd.PATCHES, directions=swd.DIRS, torch_chunk=chunk,
               images_bytes_both_sides=int(real.numel() + fake.numel()), peak_allocated_bytes=peak,
               hip_descriptor_buffer_bytes=m * 147 * 8, hip_projection_buffers_bytes=3 * swd.DIRS * m * 8,
               hip_stages_level0_one_side=stages(ev, draws))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--images', type=int, default=2933)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--chunk', type=int, default=256, help='images per pyramid pass of the torch route')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_swd.py measures on the GPU: no device visible')
    res = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup,
               measured_against='torch: .double() -> depthwise f64 conv2d pyramids on reflect-padded maps (once per image '
                                'for all levels) -> gather -> mean / std -> matmul -> torch.sort -> mean |a - b|, on the '
                                'same device, in the same process, on the same draws, alternated with SWD.result(); a '
                                'sample is one whole evaluation, wall clock between device synchronisations',
               shape=bench(args.images, args.size, args.reps, args.warmup, args.chunk))
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
