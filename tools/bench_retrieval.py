#!/usr/bin/env python3
"""Image-caption retrieval: the four launches of Retrieval.ranks() (sba_retrieval_own_best and sba_retrieval_counts, once
with the images and once with the captions as the query side) at D = 256, next to the float64 route in torch on the same
device:

    hip_i2t_best / hip_i2t_counts / hip_t2i_best / hip_t2i_counts     the launches alone, workspace preallocated
    torch_f64      x.double(), y.double(), then per direction in row chunks that fit `--chunk_gib`: matmul, the division
                   by max(sqrt(nx ny), eps), the own threshold, the comparison and sum(1) for both protocols.  It WRITES
                   every chunk of the ni x nt matrix, twice (once per direction)

at the CUB test split (2 933 images x 29 330 captions, a planted signal) and at the COCO validation split's size
(40 504 x 202 520, random rows), in the SAME process on the same inputs, alternated sample by sample after a warm-up; a
sample is one pass between two device events.  Reported as median and interquartile range, with the f64 rate of the four
launches (4 x 2 ni nt D / t: every pair is scored by all four) and the peak device memory either route adds to the codes.
The counts of the two routes are compared first.  Recorded, not asserted.

    python tools/bench_retrieval.py [--reps 5] [--warmup 1] [--out profiles/retrieval_bench.json]
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

D, EPS = 256, 1e-8
F64_MATRIX_PEAK_TFLOPS = 78.6       # MI355X data sheet, FP64 matrix
SIZES = {'cub_test': (2933, 10, 50), 'coco_val': (40504, 5, 1)}     # images, captions per image, images per class


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


def _peak(f):
    """bytes the call adds to what is allocated before it, at its peak"""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    f()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def torch_route(x, y, owner, cls, chunk_bytes):
    """the four count vectors by the float64 route in torch, row chunk by row chunk"""
    xd, yd = x.double(), y.double()
    nx, ny = (xd * xd).sum(1), (yd * yd).sum(1)
    ni, nt = x.shape[0], y.shape[0]
    key_i = torch.arange(ni, device=x.device)
    cls_t = cls[owner]
    out = [torch.empty(n, dtype=torch.int64, device=x.device) for n in (ni, ni, nt, nt)]

    def side(a, b, na, nb, key_a, key_b, cls_a, cls_b, above, masked, own_one):
        rows = max(1, int(chunk_bytes // (8 * b.shape[0])))
        for lo in range(0, a.shape[0], rows):
            hi = min(lo + rows, a.shape[0])
            s = a[lo:hi] @ b.t()
            s /= torch.sqrt(na[lo:hi, None] * nb[None, :]).clamp_(min=EPS)
            own = key_a[lo:hi, None] == key_b[None, :]
            if own_one:
                thr = s.gather(1, key_a[lo:hi, None])
            else:
                thr = torch.where(own, s, s.new_full((), float('-inf'))).max(1, keepdim=True).values
            hit = ~(s < thr) & ~own
            above[lo:hi] = hit.sum(1)
            masked[lo:hi] = (hit & (cls_a[lo:hi, None] != cls_b[None, :])).sum(1)

    side(xd, yd, nx, ny, key_i, owner, cls, cls_t, out[0], out[1], False)
    side(yd, xd, ny, nx, owner, key_i, cls_t, cls, out[2], out[3], True)
    return out


def bench_shape(name, reps, warmup, chunk_bytes):
    from sbagan import _lib
    ni, per, group = SIZES[name]
    nt = ni * per
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev)
    g.manual_seed(ni)
    x = torch.randn((ni, D), generator=g, device=dev)
    owner = torch.arange(nt, device=dev) // per
    y = torch.randn((nt, D), generator=g, device=dev)
    if name == 'cub_test':      # a planted signal: the own captions lie about two standard deviations above the others
        y += x[owner] * (2.0 / D ** 0.5)
    cls = torch.arange(ni, device=dev) // group
    ints = torch.cat([torch.arange(ni, device=dev), owner, cls, cls[owner]]).to(torch.int32)
    key_i, key_t, cls_i, cls_t = ints[:ni], ints[ni:ni + nt], ints[ni + nt:2 * ni + nt], ints[2 * ni + nt:]
    st = torch.cuda.current_stream().cuda_stream
    nbytes = max(int(_lib.lib.sba_retrieval_workspace_bytes(ni, nt, 0)), int(_lib.lib.sba_retrieval_workspace_bytes(nt, ni, 0)))

    def hip_alloc():
        return (torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=dev),
                torch.empty(ni + nt, dtype=torch.float64, device=dev),
                torch.empty(2 * (ni + nt), dtype=torch.int32, device=dev))
    ws, best, cnt = hip_alloc()

    # the launches alone: the operators' host-side checks and allocations are not device work
    def own_best(a, na, b, nb, ka, kb, out):
        _lib.call('sba_retrieval_own_best', a.data_ptr(), na, D, b.data_ptr(), nb, D, D, ka.data_ptr(), kb.data_ptr(), EPS,
                  0, out.data_ptr(), ws.data_ptr(), nbytes, st)

    def counts(a, na, b, nb, ka, kb, ca, cb, thr, above, masked):
        _lib.call('sba_retrieval_counts', a.data_ptr(), na, D, b.data_ptr(), nb, D, D, ka.data_ptr(), kb.data_ptr(),
                  ca.data_ptr(), cb.data_ptr(), thr.data_ptr(), EPS, 0, above.data_ptr(), masked.data_ptr(),
                  ws.data_ptr(), nbytes, st)

    hip = {'hip_i2t_best': lambda: own_best(x, ni, y, nt, key_i, key_t, best[:ni]),
           'hip_i2t_counts': lambda: counts(x, ni, y, nt, key_i, key_t, cls_i, cls_t, best[:ni], cnt[:ni], cnt[ni:2 * ni]),
           'hip_t2i_best': lambda: own_best(y, nt, x, ni, key_t, key_i, best[ni:]),
           'hip_t2i_counts': lambda: counts(y, nt, x, ni, key_t, key_i, cls_t, cls_i, best[ni:], cnt[2 * ni:2 * ni + nt],
                                            cnt[2 * ni + nt:])}

    def hip_all():
        for f in hip.values():
            f()

    def torch_all():
        return torch_route(x, y, owner, cls, chunk_bytes)

    out = dict(name=name, n_images=ni, n_captions=nt, D=D, workspace_bytes=nbytes, chunk_bytes=int(chunk_bytes),
               score_matrix_f64_bytes=8 * ni * nt)
    hip_all()
    want = torch.cat(torch_all()).to(torch.int32)
    torch.cuda.synchronize()
    out['counts_differing_from_torch_f64'] = int((want != cnt).sum())
    from sbagan.retrieval import RANKS, summarize
    c = cnt.cpu().numpy()
    cuts = np.cumsum([0, ni, ni, nt, nt])
    out['figures'] = {r: summarize(c[cuts[k]:cuts[k + 1]]) for k, r in enumerate(RANKS)}
    del want

    def hip_fresh():        # with its allocations, as ops.retrieval_* make them
        nonlocal ws, best, cnt
        ws, best, cnt = hip_alloc()
        hip_all()
    ws = best = cnt = None
    out['hip_peak_bytes'] = _peak(hip_fresh)
    out['torch_f64_peak_bytes'] = _peak(torch_all)
    for _ in range(warmup):
        hip_all()
        torch_all()
    torch.cuda.synchronize()
    fns = dict(hip, torch_f64=torch_all)
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            times[k].append(_device_sample(f))
    for k, t in times.items():
        out[k] = _quartiles(t)
    four = [sum(v) for v in zip(*(times[k] for k in hip))]
    q = _quartiles(four)
    q['f64_tflops'] = 4 * 2.0 * ni * nt * D / (q['median_ms'] * 1e-3) / 1e12
    q['fraction_of_f64_matrix_peak'] = q['f64_tflops'] / F64_MATRIX_PEAK_TFLOPS
    out['hip_four_launches'] = q
    out['torch_over_hip'] = out['torch_f64']['median_ms'] / q['median_ms']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--sizes', nargs='+', default=['cub_test', 'coco_val'], choices=sorted(SIZES))
    ap.add_argument('--chunk_gib', type=float, default=4.0, help='f64 bytes of one row chunk of the torch route')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_retrieval.py measures on the GPU: no device visible')
    if args.reps < 5:
        raise SystemExit('bench_retrieval.py: at least 5 repetitions')
    res = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup,
               f64_matrix_peak_tflops=F64_MATRIX_PEAK_TFLOPS,
               measured_against='torch_f64: .double(), matmul in row chunks of --chunk_gib, division, comparison and sum on '
                                'the same device, in the same process, alternated with the kernels sample by sample',
               shapes=[bench_shape(n, args.reps, args.warmup, args.chunk_gib * (1 << 30)) for n in args.sizes])
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
