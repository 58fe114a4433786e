#!/usr/bin/env python3
"""Kernel Inception Distance: the three launches of KID.result() (sba_kid_kernel_sums for the xx, yy and xy terms) at the
real shape -- 100 subsets of 1000 rows a side, D = 2048, gathered from N = 2933 rows a side (a CUB test split) -- next to
the float64 device route in torch for the same sums:

    hip_xx / hip_yy / hip_xy       one launch per term over all subsets, rows gathered by index inside the kernel, the
                                   polynomial and the sum in the epilogue; the kernel matrices are never written
    torch_xx / torch_yy / torch_xy index_select -> .double() -> bmm -> (g / D + 1)^3 -> (diagonal zeroed) -> sum, which
                                   writes the gathered f64 rows and the [S][m][m] kernel matrix

in the SAME process on the same inputs and the same subsets, alternated sample by sample after a warm-up; a sample is
`inner` back-to-back calls between two device events.  Reported per call as median and interquartile range, with the
f64 rate 2 S m m D / t and its fraction of the matrix-core f64 peak of the data sheet (78.6 TFLOP/s).  The sums of the
two routes are compared first.  Recorded, not asserted.

    python tools/bench_kid.py [--reps 10] [--warmup 2] [--out profiles/kid_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'sba-gan_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

D = 2048
F64_MATRIX_PEAK_TFLOPS = 78.6       # MI355X data sheet, FP64 matrix


def _quartiles(t):
    q1, med, q3 = np.percentile(t, [25, 50, 75])
    return dict(median_ms=float(med), iqr_ms=float(q3 - q1), min_ms=float(min(t)), n=len(t))


def _device_sample(f, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def bench(n, subsets, m, reps, warmup, inner):
    from sbagan import _lib
    from sbagan.kid import draw_subsets, kid_from_sums
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(n)
    scale = rng.uniform(0.1, 1.0, D)
    real = torch.from_numpy((np.abs(rng.randn(n, D)) * scale).astype(np.float32)).to(dev)
    fake = torch.from_numpy((np.abs(0.9 * rng.randn(n, D) + 0.1) * scale).astype(np.float32)).to(dev)
    idx_real, idx_fake = (torch.from_numpy(i).to(dev) for i in draw_subsets(n, n, m, subsets, 100))
    long_real, long_fake = idx_real.long().reshape(-1), idx_fake.long().reshape(-1)
    st = torch.cuda.current_stream().cuda_stream
    nbytes = int(_lib.lib.sba_kid_workspace_bytes(m, m, subsets, 0))
    ws = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=dev)
    hip_out = torch.empty((3, subsets), dtype=torch.float64, device=dev)
    torch_out = torch.empty((3, subsets), dtype=torch.float64, device=dev)

    # the launches alone: the operator's host-side checks, uploads and allocations are not device work
    def hip(a, b, ia, ib, diag, out):
        _lib.call('sba_kid_kernel_sums', a.data_ptr(), n, D, ia.data_ptr(), m, b.data_ptr(), n, D, ib.data_ptr(), m, D,
                  subsets, diag, 0, out.data_ptr(), ws.data_ptr(), nbytes, st)

    def route(a, b, ia, ib, diag, out):
        x = a.index_select(0, ia).double().view(subsets, m, D)
        y = x if (b is a and ib is ia) else b.index_select(0, ib).double().view(subsets, m, D)
        t = torch.bmm(x, y.transpose(1, 2)).div_(float(D)).add_(1.0)
        k = t * t * t
        if diag:
            k.diagonal(dim1=1, dim2=2).zero_()
        torch.sum(k, dim=(1, 2), out=out)

    fns = {'hip_xx': lambda: hip(real, real, idx_real, idx_real, 1, hip_out[0]),
           'torch_xx': lambda: route(real, real, long_real, long_real, 1, torch_out[0]),
           'hip_yy': lambda: hip(fake, fake, idx_fake, idx_fake, 1, hip_out[1]),
           'torch_yy': lambda: route(fake, fake, long_fake, long_fake, 1, torch_out[1]),
           'hip_xy': lambda: hip(real, fake, idx_real, idx_fake, 0, hip_out[2]),
           'torch_xy': lambda: route(real, fake, long_real, long_fake, 0, torch_out[2])}
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    out = {'max_rel_diff_hip_vs_torch_f64': float(((hip_out - torch_out).abs() / torch_out.abs()).max())}
    h = hip_out.cpu().numpy()
    out['result'] = kid_from_sums(h[0], h[1], h[2], m, n, n, D, 'synthetic', 100)
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            times[k].append(_device_sample(f, inner))
    flop = 2.0 * subsets * m * m * D
    for k, t in times.items():
        q = _quartiles(t)
        q['f64_tflops'] = flop / (q['median_ms'] * 1e-3) / 1e12
        q['fraction_of_f64_matrix_peak'] = q['f64_tflops'] / F64_MATRIX_PEAK_TFLOPS
        out[k] = q
    for route_name in ('hip', 'torch'):
        three = [sum(v) for v in zip(*(times[k] for k in fns if k.startswith(route_name + '_')))]
        out[route_name + '_three_terms'] = _quartiles(three)
    out['torch_over_hip_three_terms'] = out['torch_three_terms']['median_ms'] / out['hip_three_terms']['median_ms']
    blocks = (m + 63) // 64
    out.update(n=n, D=D, subsets=subsets, subset_size=m, inner=inner, f64_flop_per_term=flop, workspace_bytes=nbytes,
               splits=(nbytes // (8 * subsets * blocks)) if nbytes else 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--inner', type=int, default=2)
    ap.add_argument('--rows', type=int, default=2933)
    ap.add_argument('--subsets', type=int, default=100)
    ap.add_argument('--subset_size', type=int, default=1000)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_kid.py measures on the GPU: no device visible')
    res = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup,
               f64_matrix_peak_tflops=F64_MATRIX_PEAK_TFLOPS,
               measured_against='torch: index_select -> .double() -> bmm -> (g / D + 1)^3 -> sum per term on the same '
                                'device, in the same process, on the same subsets, alternated with the kernel sample '
                                'by sample',
               shape=bench(args.rows, args.subsets, min(args.subset_size, args.rows), args.reps, args.warmup, args.inner))
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
