#!/usr/bin/env python3
"""R-precision ranking: the HIP kernel (sba_rprec_rank) against the PyTorch composition of the same thing -- index
gather to [B][M][nef], bmm, norms, clamp, compare, count -- at the product shape B = 20, M = 99, nef = 256, P = 29330
(the CUB test split: 2933 images x 10 captions), in the SAME process on the same device-resident inputs.

The two paths are alternated sample by sample after a warm-up; one sample = `inner` back-to-back calls between two device
events (a single call is a few microseconds of GPU work: one call per event pair would time the events), reported per
call as median and interquartile range.  The ranks of the two paths are compared first.  Recorded, not asserted: the
evaluation's time is the generator's and the Inception forward's; the kernel removes the gathered intermediate and the
launch tail.

    python tools/bench_rprec.py [--reps 30] [--warmup 5] [--inner 50] [--out profiles/rprec_bench.json]
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


def torch_rank(cnn, true_emb, pool, idx64, eps):
    cand = torch.cat([true_emb.unsqueeze(1), pool[idx64]], 1)                    # [B][M + 1][nef]
    dot = torch.bmm(cand, cnn.unsqueeze(2)).squeeze(2)
    den = (cnn.norm(dim=1, keepdim=True) * cand.norm(dim=2)).clamp(min=eps)
    s = dot / den
    return (~(s[:, 1:] < s[:, :1])).sum(1, dtype=torch.int32)


def _time_alternating(fns, reps, warmup, inner):
    for _ in range(warmup):
        for f in fns.values():
            for _ in range(inner):
                f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3 / inner)
    out = {}
    for k, t in times.items():
        q1, med, q3 = np.percentile(t, [25, 50, 75])
        out[k] = dict(median_us=float(med), iqr_us=float(q3 - q1), min_us=float(min(t)), n=len(t))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--inner', type=int, default=50)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_rprec.py measures on the GPU: no device visible')
    from sbagan import _lib, ops
    dev = torch.device('cuda:0')
    B, M, nef, P, eps = 20, 99, 256, 29330, 1e-8
    rng = np.random.RandomState(0)
    cnn, true_emb, pool = (torch.from_numpy(rng.randn(n, nef).astype(np.float32)).to(dev) for n in (B, B, P))
    idx = torch.from_numpy(rng.randint(0, P, size=(B, M)).astype(np.int32)).to(dev)
    idx64 = idx.long()
    rank = torch.empty(B, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def kernel():          # the launch alone: ops.rprec_rank's host-side checks are not device work
        _lib.call('sba_rprec_rank', cnn.data_ptr(), true_emb.data_ptr(), pool.data_ptr(), idx.data_ptr(), eps,
                  rank.data_ptr(), None, B, M, nef, P, st)

    def composition():
        return torch_rank(cnn, true_emb, pool, idx64, eps)
    same = bool(torch.equal(ops.rprec_rank(cnn, true_emb, pool, idx), composition()))
    r = _time_alternating({'hip_kernel': kernel, 'torch_composition': composition}, args.reps, args.warmup, args.inner)
    res = dict(shape=dict(B=B, M=M, nef=nef, P=P), reps=args.reps, warmup=args.warmup, inner=args.inner,
               device=torch.cuda.get_device_name(0), ranks_equal=same,
               bytes_gathered=B * (M + 2) * nef * 4, intermediate_bytes_avoided=B * (M + 1) * nef * 4, **r)
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
