#!/usr/bin/env python3
"""MS-SSIM evaluation: the two launches of MSSSIM.result() (sba_msssim_pairs, one per side over the same pairs) at the
real shape -- 5000 same-class pairs (50 classes x 100) of 256 px images, 5 scales, drawn from N = 2933 images a side
(a CUB test split) -- next to the float64 device route in torch for the same per-scale means:

    hip_fake / hip_real       one call per side: every scale pools from the uint8 images while staging, the five window
                              means live in LDS only; the workspace holds the workgroups' partial sums
    torch_fake / torch_real   per chunk of pairs: gather -> .double() -> per scale five depthwise f64 conv2d (mx, my,
                              E[xx], E[yy], E[xy]; --window 2d: one 11 x 11 window each, separable: a 1 x 11 and an
                              11 x 1 pass each) -> cs, ssim -> mean, then avg_pool2d; it writes five N x 3 x H x W f64
                              maps per side and scale, so it runs in chunks that fit

in the SAME process on the same images and the same pairs, alternated sample by sample after a warm-up; a sample is one
call between two device events.  Reported per call as median and interquartile range.  The outputs of the two routes
are compared first.  Recorded, not asserted.

    python tools/bench_msssim.py [--reps 5] [--warmup 1] [--out profiles/msssim_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'sba-gan_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

SCALES = 5


def _quartiles(t):
    q1, med, q3 = np.percentile(t, [25, 50, 75])
    return dict(median_ms=float(med), iqr_ms=float(q3 - q1), min_ms=float(min(t)), n=len(t))


def _device_sample(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def images(n, size, seed, dev):
    """uint8 [n][3][size][size]: smooth structure shared within a "class" of 60 images plus noise, so the pairs are
    neither identical nor unrelated"""
    g = torch.Generator(device='cpu').manual_seed(seed)
    base = F.interpolate(torch.rand((n + 59) // 60, 3, 16, 16, generator=g), size=size, mode='bilinear')
    x = base.repeat_interleave(60, 0)[:n] * 200.0 + torch.rand(n, 3, size, size, generator=g) * 55.0
    return x.to(torch.uint8).to(dev)


def torch_route(imgs, pairs, out, chunk, separable):
    g = torch.arange(11, dtype=torch.float64, device=imgs.device)
    g = torch.exp(-(g - 5.0) ** 2 / (2.0 * 1.5 ** 2))
    g = g / g.sum()
    C1, C2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2
    if separable:
        wr, wc = g.view(1, 1, 1, 11).repeat(3, 1, 1, 1), g.view(1, 1, 11, 1).repeat(3, 1, 1, 1)

        def win(a):
            return F.conv2d(F.conv2d(a, wr, groups=3), wc, groups=3)
    else:
        w2 = torch.outer(g, g).view(1, 1, 11, 11).repeat(3, 1, 1, 1)

        def win(a):
            return F.conv2d(a, w2, groups=3)
    for at in range(0, pairs.shape[0], chunk):
        pc = pairs[at:at + chunk].long()
        x, y = imgs.index_select(0, pc[:, 0]).double(), imgs.index_select(0, pc[:, 1]).double()
        for s in range(SCALES):
            if s:
                x, y = F.avg_pool2d(x, 2), F.avg_pool2d(y, 2)
            mx, my = win(x), win(y)
            sxx, syy, sxy = win(x * x) - mx * mx, win(y * y) - my * my, win(x * y) - mx * my
            cs = (2.0 * sxy + C2) / (sxx + syy + C2)
            ssim = cs * (2.0 * mx * my + C1) / (mx * mx + my * my + C1)
            out[at:at + chunk, :, s, 0] = ssim.mean(dim=(2, 3))
            out[at:at + chunk, :, s, 1] = cs.mean(dim=(2, 3))


def bench(n, classes, per_class, size, reps, warmup, chunk, separable):
    from sbagan import _lib
    from sbagan.msssim import combine, draw_pairs
    dev = torch.device('cuda:0')
    fake, real = images(n, size, 1, dev), images(n, size, 2, dev)
    ids = np.arange(n) * classes // n
    pairs_host = draw_pairs(ids, per_class, 100)
    P = len(pairs_host)
    pairs = torch.from_numpy(pairs_host).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    nbytes = int(_lib.lib.sba_msssim_workspace_bytes(size, size, P, SCALES))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    hip_out = torch.empty((2, P, 3, SCALES, 2), dtype=torch.float64, device=dev)
    torch_out = torch.empty((2, P, 3, SCALES, 2), dtype=torch.float64, device=dev)

    # the launches alone: the operator's host-side checks, uploads and allocations are not device work
    def hip(imgs, out):
        _lib.call('sba_msssim_pairs', imgs.data_ptr(), n, size, size, pairs.data_ptr(), P, SCALES, out.data_ptr(),
                  ws.data_ptr(), nbytes, st)

    fns = {'hip_fake': lambda: hip(fake, hip_out[0]), 'torch_fake': lambda: torch_route(fake, pairs, torch_out[0], chunk,
                                                                                       separable),
           'hip_real': lambda: hip(real, hip_out[1]), 'torch_real': lambda: torch_route(real, pairs, torch_out[1], chunk,
                                                                                       separable)}
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    out = {'max_abs_diff_hip_vs_torch_f64': float((hip_out - torch_out).abs().max())}
    h = hip_out.cpu().numpy()
    out['result'] = {'ms_ssim_fake': float(combine(h[0]).mean()), 'ms_ssim_real': float(combine(h[1]).mean())}
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            times[k].append(_device_sample(f))
    for k, t in times.items():
        out[k] = _quartiles(t)
    for route_name in ('hip', 'torch'):
        both = [sum(v) for v in zip(*(times[k] for k in fns if k.startswith(route_name + '_')))]
        out[route_name + '_two_sides'] = _quartiles(both)
    out['torch_over_hip_two_sides'] = out['torch_two_sides']['median_ms'] / out['hip_two_sides']['median_ms']
    positions = sum(((size >> s) - 10) ** 2 for s in range(SCALES)) * 3 * P
    out.update(n=n, size=size, pairs=P, classes=classes, pairs_per_class=per_class, scales=SCALES, torch_chunk=chunk,
               torch_window='separable' if separable else '2d', workspace_bytes=nbytes, window_positions_per_side=positions,
               hip_positions_per_second=positions / (out['hip_two_sides']['median_ms'] * 0.5e-3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--images', type=int, default=2933)
    ap.add_argument('--classes', type=int, default=50)
    ap.add_argument('--per_class', type=int, default=100)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--chunk', type=int, default=250, help='pairs per pass of the torch route')
    ap.add_argument('--window', choices=('separable', '2d'), default='separable')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_msssim.py measures on the GPU: no device visible')
    res = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup,
               measured_against='torch: gather -> .double() -> per scale five depthwise f64 conv2d windows -> cs, ssim -> '
                                'mean -> avg_pool2d, in chunks of pairs, on the same device, in the same process, on the '
                                'same pairs, alternated with the kernel sample by sample',
               shape=bench(args.images, args.classes, args.per_class, args.size, args.reps, args.warmup, args.chunk,
                           args.window == 'separable'))
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
