#!/usr/bin/env python3
"""--truncation measured (run alone on the GPU, profiler off).  Writes profiles/truncation_bench.json.
The protocol of tools/bench_ada.py (bench_diffaug's `windows`: medians of 9 windows of 200 launches between device events;
fresh child processes, the arms alternated):

  (a) the mean style at n = 16384, W_DIM = 256: the mapping passes of mean_style (256 passes of 64 codes through the
      8-layer mapping network -- what its dense kernels take in one call -- host-timed around a synchronise, 9 times),
      the two launches of sba_style_mean on their own, and the same mean through torch on the device
      (w.double().mean(0));
  (b) sba_style_truncate at 20 and 40 rows of 256, psi = 0.7 and psi = 1 (the copy), beside torch.lerp on the same
      tensors;
  (c) one sampling() batch at the bird_style sizes (model_bert.G_NET, B = 20, three stages, 256 px, bf16; synthetic
      caption embeddings): the noise draw and the generator's forward as sampling()'s loop issues them, without a
      truncation and with --truncation 0.7 (the launch in _styles and the per-batch distance of truncation.json), one
      fresh process per arm, the arms alternated; ms per batch.

    python tools/bench_truncation.py [--parts abc] [--out profiles/truncation_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'sba-gan_amd')
for p in (ROOT, PKG, os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_diffaug import windows  # noqa: E402

ARMS = ('plain', 'truncated')
N, W_DIM, PSI = 16384, 256, 0.7


def _summary(got):
    return {'us_median': {k: float(np.median(v)) for k, v in got.items()},
            'us_min': {k: float(min(v)) for k, v in got.items()}, 'us_max': {k: float(max(v)) for k, v in got.items()}}


def part_a(args):
    import model_bert
    from miscc.config import cfg, reset_cfg
    from sbagan import _lib, truncation
    reset_cfg()
    cfg.GAN.W_DIM = W_DIM
    dev = torch.device('cuda', 0)
    st = torch.cuda.current_stream().cuda_stream
    lib = _lib.lib
    torch.manual_seed(1)
    net = model_bert.G_NET().to(dev).eval()
    truncation.mean_style(net, N)                       # warm-up: code objects, the allocator's blocks
    torch.cuda.synchronize()
    whole = []
    for _ in range(args.windows):
        t0 = time.perf_counter()
        truncation.mean_style(net, N)
        torch.cuda.synchronize()
        whole.append((time.perf_counter() - t0) * 1e3)
    w = truncation.mapped_styles(net, N)
    passes = -(-N // truncation.pass_rows(net.mapping_net))
    m64 = torch.empty(W_DIM, dtype=torch.float64, device=dev)
    m32 = torch.empty(W_DIM, dtype=torch.float32, device=dev)
    ws = torch.empty((N // 256, W_DIM), dtype=torch.float64, device=dev)
    mean = (w.data_ptr(), N, W_DIM, m64.data_ptr(), m32.data_ptr(), ws.data_ptr(), st)
    assert lib.sba_style_mean(*mean) == 0
    got = windows({'sba_style_mean': lambda: lib.sba_style_mean(*mean),
                   'torch_double_mean': lambda: w.double().mean(0)}, args.launches, args.windows)
    torch.cuda.synchronize()
    mapping = []
    for _ in range(args.windows):
        t0 = time.perf_counter()
        truncation.mapped_styles(net, N)
        torch.cuda.synchronize()
        mapping.append((time.perf_counter() - t0) * 1e3)
    out = dict(_summary(got), n=N, W_DIM=W_DIM, mapping_passes=passes, rows_per_pass=truncation.pass_rows(net.mapping_net),
               mean_style_ms_median=float(np.median(whole)), mean_style_ms=whole,
               mapping_passes_ms_median=float(np.median(mapping)), mapping_passes_ms=mapping,
               max_abs_diff_to_torch=float((m64 - w.double().mean(0)).abs().max()))
    med = out['us_median']
    print('(a) n %d x %d: mean_style %.3f ms whole | %d mapping passes %.3f ms, sba_style_mean (2 launches) %.2f us, '
          'torch .double().mean(0) %.2f us' % (N, W_DIM, out['mean_style_ms_median'], passes,
                                               out['mapping_passes_ms_median'], med['sba_style_mean'],
                                               med['torch_double_mean']), flush=True)
    return out


def part_b(args):
    from sbagan import _lib
    dev = torch.device('cuda', 0)
    st = torch.cuda.current_stream().cuda_stream
    lib = _lib.lib
    cases = []
    for rows in (20, 40):
        g = torch.Generator(device='cpu')
        g.manual_seed(rows)
        w = torch.randn((rows, W_DIM), generator=g).to(dev)
        avg = (0.1 * torch.randn((W_DIM,), generator=g)).to(dev)
        out = torch.empty_like(w)
        wide = avg.expand_as(w)
        fns = {}
        for psi in (PSI, 1.0):
            a = (w.data_ptr(), avg.data_ptr(), psi, out.data_ptr(), rows, W_DIM, st)
            assert lib.sba_style_truncate(*a) == 0
            fns['sba_style_truncate_psi%g' % psi] = lambda a=a: lib.sba_style_truncate(*a)
        fns['torch_lerp'] = lambda: torch.lerp(wide, w, PSI)
        fns['torch_lerp_out'] = lambda: torch.lerp(wide, w, PSI, out=out)
        got = windows(fns, args.launches, args.windows)
        cases.append(dict(_summary(got), rows=rows, W_DIM=W_DIM))
        med = cases[-1]['us_median']
        print('(b) %d rows: sba_style_truncate psi=%g %.2f us, psi=1 %.2f us | torch.lerp %.2f us (out= %.2f us)'
              % (rows, PSI, med['sba_style_truncate_psi%g' % PSI], med['sba_style_truncate_psi1'], med['torch_lerp'],
                 med['torch_lerp_out']), flush=True)
    return {'launches_per_window': args.launches, 'windows': args.windows, 'cases': cases}


def batch_child(args):
    """one arm of (c) in a process of its own; prints one JSON line"""
    import model_bert
    from miscc.config import cfg, reset_cfg
    from miscc.utils import weights_init
    from sbagan import ops, truncation
    reset_cfg()
    cfg.GAN.GF_DIM, cfg.GAN.DF_DIM, cfg.TREE.BRANCH_NUM, cfg.GAN.R_NUM, cfg.GAN.W_DIM = 32, 64, 3, 2, W_DIM
    cfg.TEXT.EMBEDDING_DIM = 256
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(0)
    ops.set_compute_dtype(torch.bfloat16)
    B, L = 20, 18
    torch.manual_seed(1)
    net = model_bert.G_NET()
    net.apply(weights_init)
    net.to(dev).eval()
    t0 = time.perf_counter()
    held = truncation.set_truncation(net, PSI if args.child == 'truncated' else None, N)
    torch.cuda.synchronize()
    setup_ms = (time.perf_counter() - t0) * 1e3
    w_rms = truncation.WDistance(held) if held is not None else None
    g = torch.Generator(device=dev)
    g.manual_seed(100)
    sent = torch.randn((B, 256), generator=g, device=dev)
    words = torch.randn((B, 256, L), generator=g, device=dev)
    mask = torch.zeros((B, L), dtype=torch.bool, device=dev)
    noise = torch.empty((B, cfg.GAN.Z_DIM), device=dev)

    def batch():
        noise.normal_(0, 1)
        with torch.no_grad():
            imgs = net(noise, sent, words, mask)[0]
        if w_rms is not None:
            w_rms.update(noise)
        return imgs[-1]
    for _ in range(args.warm_steps):
        last = batch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.step_windows):
        t0 = time.perf_counter()
        for _ in range(args.steps):
            last = batch()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / args.steps)
    print('CHILD ' + json.dumps({'arm': args.child, 'ms': ms, 'setup_ms': setup_ms,
                                 'finite': bool(torch.isfinite(last.float()).all())}), flush=True)


def part_c(args):
    runs, setup = {k: [] for k in ARMS}, {k: [] for k in ARMS}
    for r in range(args.rounds):
        for arm in ARMS:
            cmd = [sys.executable, os.path.abspath(__file__), '--child', arm, '--steps', str(args.steps),
                   '--step_windows', str(args.step_windows), '--warm_steps', str(args.warm_steps)]
            text = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=args.child_timeout).stdout.decode()
            got = json.loads([ln for ln in text.splitlines() if ln.startswith('CHILD ')][-1][6:])
            assert got['finite'], 'an image of the %s arm is not finite' % arm
            runs[arm] += got['ms']
            setup[arm].append(got['setup_ms'])
            print('(c) round %d, %-9s: %s ms / batch' % (r, arm, ' '.join('%.3f' % v for v in got['ms'])), flush=True)
    med = {k: float(np.median(v)) for k, v in runs.items()}
    print('(c) one sampling batch (B = 20, 256 px), median: plain %.3f ms, --truncation %g %.3f ms (%+.3f); w_avg once per '
          'run: %.1f ms' % (med['plain'], PSI, med['truncated'], med['truncated'] - med['plain'],
                            float(np.median(setup['truncated']))), flush=True)
    return {'batches_per_window': args.steps, 'ms_windows': runs, 'ms_median': med, 'psi': PSI, 'truncation_n': N,
            'set_truncation_ms': setup, 'batch': 20, 'px': 256, 'dtype': 'bfloat16', 'generator': 'model_bert.G_NET'}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', default='abc')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'truncation_bench.json'))
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--windows', type=int, default=9)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--step_windows', type=int, default=3)
    ap.add_argument('--warm_steps', type=int, default=10)
    ap.add_argument('--child_timeout', type=int, default=240)
    ap.add_argument('--child', default=None, choices=list(ARMS), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_truncation needs the GPU: nothing is measured without one')
    if args.child:
        return batch_child(args)
    result = {'device': torch.cuda.get_device_name(0), 'torch': torch.__version__}
    if 'a' in args.parts:
        result['mean'] = part_a(args)
    if 'b' in args.parts:
        result['truncate'] = part_b(args)
    if 'c' in args.parts:       # (children only: this process keeps its device context idle meanwhile)
        result['batch'] = part_c(args)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
