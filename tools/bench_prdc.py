#!/usr/bin/env python3
"""Precision / recall / density / coverage: the four launches of PRDC.result() (two sba_prdc_knn_radius, two
sba_prdc_ball_counts) at D = 2048, k = 5 and N = 2933 rows a side (a CUB test split) and N = 30000, next to the float64
device product of the same size:

    hip_knn_real / hip_knn_fake        radius2 of a side: all N x N distances, the 8 smallest per row kept in registers
    hip_counts_fr / hip_counts_rf      one and two ball counts per row over all N x N distances
    torch_f64                          a.double() @ b.double().T on the device (the BLAS f64 product, widening included;
                                       it WRITES the N x N matrix the kernels never form, and selects nothing)

in the SAME process on the same inputs, alternated sample by sample after a warm-up; a sample is `inner` back-to-back
calls between two device events.  Reported per call as median and interquartile range, with the f64 rate 2 N N D / t and
its fraction of the matrix-core f64 peak of the data sheet (78.6 TFLOP/s), beside what profiles/fid_bench.json records
for sba_fid_accumulate.  The counts of the library's launches are compared with a torch evaluation of the same definitions
first (at the small size).  Recorded, not asserted.

    python tools/bench_prdc.py [--reps 10] [--warmup 2] [--out profiles/prdc_bench.json]
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

D, K = 2048, 5
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


def bench_shape(n, reps, warmup):
    from sbagan import _lib, ops
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(n)
    scale = rng.uniform(0.1, 3.0, D)
    real = torch.from_numpy((np.abs(rng.randn(n, D)) * scale).astype(np.float32)).to(dev)
    fake = torch.from_numpy((np.abs(0.9 * rng.randn(n, D) + 0.1) * scale).astype(np.float32)).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    nbytes = int(_lib.lib.sba_prdc_workspace_bytes(n, n, 0))
    ws = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=dev)
    r_real = torch.empty(n, dtype=torch.float64, device=dev)
    r_fake = torch.empty(n, dtype=torch.float64, device=dev)
    cnt = torch.empty((3, n), dtype=torch.int32, device=dev)

    # the launches alone: the operators' host-side checks and allocations are not device work
    def knn(x, out):
        _lib.call('sba_prdc_knn_radius', x.data_ptr(), n, D, D, K, 0, out.data_ptr(), ws.data_ptr(), nbytes, st)

    def counts(a, b, ra, rb, in_b, in_own):
        _lib.call('sba_prdc_ball_counts', a.data_ptr(), n, D, b.data_ptr(), n, D, D, ra, rb, 0, in_b, in_own,
                  ws.data_ptr(), nbytes, st)

    fns = {'hip_knn_real': lambda: knn(real, r_real), 'hip_knn_fake': lambda: knn(fake, r_fake),
           'hip_counts_fr': lambda: counts(fake, real, None, r_real.data_ptr(), cnt[0].data_ptr(), None),
           'hip_counts_rf': lambda: counts(real, fake, r_real.data_ptr(), r_fake.data_ptr(), cnt[1].data_ptr(),
                                           cnt[2].data_ptr()),
           'torch_f64': lambda: real.double() @ fake.double().t()}
    for f in fns.values():
        f()
    out = {}
    if n <= 4096:       # the same definitions in torch f64 (Gram form): how many of the 3 n counts differ, if any
        rd, fd = real.double(), fake.double()

        def d2(a, b):
            return ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.t())).clamp_(min=0.0)
        rr = d2(rd, rd)
        rr.fill_diagonal_(float('inf'))
        t_real = rr.kthvalue(K, dim=1).values
        ff = d2(fd, fd)
        ff.fill_diagonal_(float('inf'))
        t_fake = ff.kthvalue(K, dim=1).values
        rf = d2(rd, fd)
        want = torch.stack([(rf.t() <= t_real[None, :]).sum(1), (rf <= t_fake[None, :]).sum(1),
                            (rf <= t_real[:, None]).sum(1)]).to(torch.int32)
        out['counts_differing_from_torch_f64'] = int((want != cnt).sum())
        out['radius_max_rel_diff_from_torch_f64'] = float(((r_real - t_real).abs() / t_real).max())
        from sbagan.prdc import prdc_from_counts
        c = cnt.cpu().numpy()
        out['metrics'] = prdc_from_counts(c[0], c[1], c[2], K, 'synthetic')
        del rd, fd, rr, ff, rf
    inner = 5 if n <= 4096 else 1
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            times[k].append(_device_sample(f, inner))
    flop = 2.0 * n * n * D
    for k, t in times.items():
        q = _quartiles(t)
        q['f64_tflops'] = flop / (q['median_ms'] * 1e-3) / 1e12
        q['fraction_of_f64_matrix_peak'] = q['f64_tflops'] / F64_MATRIX_PEAK_TFLOPS
        out[k] = q
    four = [sum(v) for v in zip(*(times[k] for k in fns if k.startswith('hip_')))]
    out['hip_four_launches'] = _quartiles(four)
    out.update(n=n, D=D, k=K, inner=inner, splits=int(nbytes // (n * 64)) if nbytes else 1, workspace_bytes=nbytes)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--sizes', type=int, nargs='+', default=[2933, 30000])
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_prdc.py measures on the GPU: no device visible')
    res = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup,
               f64_matrix_peak_tflops=F64_MATRIX_PEAK_TFLOPS,
               measured_against='torch_f64: a.double() @ b.double().T of the same N x N x D on the same device, in the '
                                'same process, alternated with the kernels sample by sample',
               shapes=[bench_shape(n, args.reps, args.warmup) for n in args.sizes])
    fid_path = os.path.join(ROOT, 'profiles', 'fid_bench.json')
    if os.path.exists(fid_path):        # the figure recorded for sba_fid_accumulate, for comparison
        with open(fid_path) as f:
            fid = json.load(f)
        res['fid_accumulate_f64_tflops_issued'] = [s['hip_kernel']['f64_tflops_issued'] for s in fid['shapes']]
        res['fid_accumulate_fraction_of_f64_matrix_peak'] = [v / F64_MATRIX_PEAK_TFLOPS
                                                              for v in res['fid_accumulate_f64_tflops_issued']]
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
