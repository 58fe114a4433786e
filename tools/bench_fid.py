#!/usr/bin/env python3
"""FID moments: the f64 matrix-core kernel (sba_fid_accumulate) against the same Gram matrix taken two other ways, at
D = 2048 and n = 1024 (one staging chunk) and n = 29330 (the CUB test split, streamed in chunks of 1024 rows):

    hip_kernel    sum and the upper-triangular tiles of X^T X, f32 rows widened in registers
    torch_f64     x.double().T @ x.double() on the device (the BLAS f64 product, widening included)
    numpy_host    x.astype(float64).T @ same, on the host with the BLAS threads the environment gives (16 intended)

in the SAME process on the same inputs.  The candidates are alternated sample by sample after a warm-up; device samples
are `inner` back-to-back calls between two device events, host samples one call under a host clock; reported per call as
median and interquartile range.  The kernel's Gram is compared with the device product first.  Recorded, not asserted.

    python tools/bench_fid.py [--reps 20] [--host-reps 5] [--warmup 3] [--out profiles/fid_bench.json]
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault('OMP_NUM_THREADS', '16')

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'sba-gan_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

D, CHUNK = 2048, 1024


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


def _host_sample(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def bench_shape(n, args):
    from sbagan import _lib
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(n)
    xh = (np.abs(rng.randn(n, D)) * rng.uniform(0.1, 3.0, D)).astype(np.float32)
    x = torch.from_numpy(xh).to(dev)
    s = torch.zeros(D, dtype=torch.float64, device=dev)
    g = torch.zeros((D, D), dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def kernel():          # the launches alone: ops.fid_accumulate's host-side checks are not device work
        for lo in range(0, n, CHUNK):
            rows = min(CHUNK, n - lo)
            _lib.call('sba_fid_accumulate', x.data_ptr() + 4 * D * lo, rows, D, D, s.data_ptr(), g.data_ptr(), st)

    def torch_f64():
        xd = x.double()
        return xd.t() @ xd

    def numpy_host():
        xd = xh.astype(np.float64)
        return xd.T @ xd

    kernel()
    ref = torch_f64()
    up = torch.triu(torch.ones((D, D), dtype=torch.bool, device=dev))
    rel = float(((g - ref).abs()[up] / ref.abs()[up].clamp(min=1e-300)).max())
    inner = 10 if n <= CHUNK else 1
    dev_fns = {'hip_kernel': kernel, 'torch_f64': torch_f64}
    for _ in range(args.warmup):
        for f in dev_fns.values():
            f()
    numpy_host()
    torch.cuda.synchronize()
    times = {k: [] for k in list(dev_fns) + ['numpy_host']}
    for r in range(args.reps):
        for k, f in dev_fns.items():
            times[k].append(_device_sample(f, inner))
        if r < args.host_reps:
            times['numpy_host'].append(_host_sample(numpy_host))
    out = {k: _quartiles(t) for k, t in times.items()}
    tiles = (D // 64) * (D // 64 + 1) // 2
    out['hip_kernel']['f64_tflops_issued'] = 2.0 * n * 64 * 64 * tiles / (out['hip_kernel']['median_ms'] * 1e-3) / 1e12
    for k in ('torch_f64', 'numpy_host'):
        out[k]['f64_tflops_full_product'] = 2.0 * n * D * D / (out[k]['median_ms'] * 1e-3) / 1e12
    out.update(n=n, D=D, chunk=CHUNK, launches=(n + CHUNK - 1) // CHUNK, inner=inner,
               kernel_vs_torch_max_rel_diff_upper=rel)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host-reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_fid.py measures on the GPU: no device visible')
    res = dict(device=torch.cuda.get_device_name(0), reps=args.reps, host_reps=args.host_reps, warmup=args.warmup,
               host_threads=os.environ.get('OMP_NUM_THREADS'),
               shapes=[bench_shape(n, args) for n in (1024, 29330)])
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
