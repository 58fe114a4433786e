#!/usr/bin/env python3
"""Nearest training images: the launches of Nearest.result() at the CUB sizes -- 2 933 generated and 2 933 real rows
against 8 855 training rows, D = 2048, K = 8 -- next to the device float64 route in torch:

    hip_fake_topk      sba_knn_topk(fake, train, 8)   (the merge launch of its column splits included)
    hip_real_top1      sba_knn_topk(real, train, 1)
    hip_train_radius   sba_prdc_knn_radius(train, 1)  (8 855 x 8 855, self excluded)
    torch_*            the same three in torch: .double() of both sets, the matmul form of the squared distance
                       (|a|^2 + |b|^2 - 2 a b^T, clamped at 0) in chunks of `--chunk` query rows, and torch.topk of the
                       negated chunk (the self column set to +inf for the radius).  It writes a chunk x nb matrix per step
                       and the f64 copies of both sets; the kernels form neither.

Both routes run in the SAME process on the same inputs, alternated sample by sample after a warm-up; a sample is one call
between two device events; medians of `--reps` (5).  The indices of the two routes are compared first: a row is compared
where the torch route's own gaps between consecutive neighbours (the first K + 1) all exceed the error bound of the two
distance formulas, 2 (4 D + 9) 2^-53 (|a|^2 + max |b|^2); the other rows are counted and reported as left out.  The tool
fails (exit status 1) when a compared row differs.  The speed is recorded, not asserted.

    python tools/bench_nearest.py [--reps 5] [--warmup 1] [--chunk 1024] [--out profiles/nearest_bench.json]
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

D, K = 2048, 8
N_EVAL, N_TRAIN = 2933, 8855
U = 2.0 ** -53


def _median(t):
    return dict(median_ms=float(np.median(t)), min_ms=float(min(t)), max_ms=float(max(t)), n=len(t))


def _device_sample(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def torch_topk(a, b, k, chunk, exclude_self=False):
    """(d2 [na][k], idx [na][k], smallest gap among the first k + 1 per row [na]) by the f64 matmul route"""
    ad, bd = a.double(), b.double()
    nb2 = (bd * bd).sum(1)
    kk = min(k + 1, b.shape[0] - (1 if exclude_self else 0))
    ds, js, gaps = [], [], []
    for lo in range(0, a.shape[0], chunk):
        x = ad[lo:lo + chunk]
        d2 = ((x * x).sum(1)[:, None] + nb2[None, :] - 2.0 * (x @ bd.t())).clamp_(min=0.0)
        if exclude_self:
            rows = torch.arange(x.shape[0], device=a.device)
            d2[rows, rows + lo] = float('inf')
        neg, j = torch.topk(d2, kk, dim=1, largest=False, sorted=True)
        ds.append(neg[:, :k])
        js.append(j[:, :k])
        gaps.append((neg[:, 1:] - neg[:, :-1]).min(1).values if kk > 1 else torch.full_like(neg[:, 0], float('inf')))
    return torch.cat(ds), torch.cat(js), torch.cat(gaps)


def compare(name, hip_idx, a, b, k, chunk, exclude_self=False):
    """rows compared / left out / differing between the kernel's row numbers and the torch route's"""
    _, want, gaps = torch_topk(a, b, k, chunk, exclude_self)
    na2, nb2 = (a.double() ** 2).sum(1), (b.double() ** 2).sum(1)
    bound = 2.0 * (4 * D + 9) * U * (na2 + nb2.max())
    sure = gaps > bound
    differ = ((hip_idx.long() != want).any(1) & sure)
    return {'rows': int(a.shape[0]), 'rows_compared': int(sure.sum()), 'rows_left_out': int((~sure).sum()),
            'rows_differing': int(differ.sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--chunk', type=int, default=1024)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_nearest.py measures on the GPU: no device visible')
    from sbagan import _lib, ops
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(8855)
    scale = rng.uniform(0.1, 3.0, D)                # pooled features are non-negative and unevenly scaled

    def rows(n, shift):
        return torch.from_numpy((np.abs(0.9 * rng.randn(n, D) + shift) * scale).astype(np.float32)).to(dev)
    train, real, fake = rows(N_TRAIN, 0.0), rows(N_EVAL, 0.0), rows(N_EVAL, 0.1)
    st = torch.cuda.current_stream().cuda_stream
    size = _lib.lib.sba_knn_workspace_bytes
    nbytes = max(int(size(N_EVAL, N_TRAIN, K, 0)), int(size(N_EVAL, N_TRAIN, 1, 0)),
                 int(_lib.lib.sba_prdc_workspace_bytes(N_TRAIN, N_TRAIN, 0)))
    ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=dev)
    fd = torch.empty((N_EVAL, K), dtype=torch.float64, device=dev)
    fi = torch.empty((N_EVAL, K), dtype=torch.int32, device=dev)
    rd = torch.empty((N_EVAL, 1), dtype=torch.float64, device=dev)
    ri = torch.empty((N_EVAL, 1), dtype=torch.int32, device=dev)
    r2 = torch.empty(N_TRAIN, dtype=torch.float64, device=dev)

    # the launches alone: the operators' host-side checks and allocations are not device work
    def knn(a, k, d2, idx):
        _lib.call('sba_knn_topk', a.data_ptr(), a.shape[0], D, train.data_ptr(), N_TRAIN, D, D, k, 0, d2.data_ptr(),
                  idx.data_ptr(), ws.data_ptr(), nbytes, st)

    fns = {'hip_fake_topk': lambda: knn(fake, K, fd, fi), 'torch_fake_topk': lambda: torch_topk(fake, train, K, args.chunk),
           'hip_real_top1': lambda: knn(real, 1, rd, ri), 'torch_real_top1': lambda: torch_topk(real, train, 1, args.chunk),
           'hip_train_radius': lambda: _lib.call('sba_prdc_knn_radius', train.data_ptr(), N_TRAIN, D, D, 1, 0, r2.data_ptr(),
                                                 ws.data_ptr(), nbytes, st),
           'torch_train_radius': lambda: torch_topk(train, train, 1, args.chunk, exclude_self=True)}
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    # the operator gives what the raw launches gave
    d2, idx = ops.knn_topk(fake, train, K)
    assert torch.equal(d2, fd) and torch.equal(idx, fi)
    agreement = {'fake_topk': compare('fake', fi, fake, train, K, args.chunk),
                 'real_top1': compare('real', ri, real, train, 1, args.chunk)}
    t_r2, _, _ = torch_topk(train, train, 1, args.chunk, exclude_self=True)
    agreement['train_radius_max_rel_diff'] = float(((r2 - t_r2[:, 0]).abs() / t_r2[:, 0]).max())

    for _ in range(args.warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(args.reps):
        for k, f in fns.items():
            times[k].append(_device_sample(f))
    res = {k: _median(t) for k, t in times.items()}
    for route in ('hip', 'torch'):
        res[route + '_all_launches'] = _median([sum(v) for v in zip(*(times[k] for k in fns if k.startswith(route)))])
    res['torch_over_hip'] = res['torch_all_launches']['median_ms'] / res['hip_all_launches']['median_ms']
    res.update(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup, chunk=args.chunk, D=D, k=K,
               n_train=N_TRAIN, n_real=N_EVAL, n_fake=N_EVAL, agreement=agreement,
               splits={'fake_topk': int(size(N_EVAL, N_TRAIN, K, 0)) // (N_EVAL * K * 12) or 1,
                       'train_radius': int(_lib.lib.sba_prdc_workspace_bytes(N_TRAIN, N_TRAIN, 0)) // (N_TRAIN * 64) or 1},
               torch_route_extra_bytes={'f64_copies': 8 * D * (N_TRAIN + N_EVAL), 'chunk_matrix': 8 * args.chunk * N_TRAIN},
               measured_against='torch f64 on the same device, in the same process, alternated with the kernels sample by '
                                'sample: .double(), |a|^2 + |b|^2 - 2 a b^T per chunk of query rows, torch.topk')
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(line)
    if any(agreement[k]['rows_differing'] for k in ('fake_topk', 'real_top1')):
        raise SystemExit(1)


if __name__ == '__main__':
    main()
