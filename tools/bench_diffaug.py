#!/usr/bin/env python3
"""--diffaug measured (run alone on the GPU, profiler off).  Writes profiles/diffaug_bench.json.

  (a) the launches alone, by device events: us per sba_diffaug_fwd (the [real | fake] concatenation and the augmentation,
      policy color,translation,cutout) and per sba_diffaug_bwd at 40 and 20 rows of 64, 128 and 256 px, the median over
      the windows, with the algorithmic bytes over that time; beside them, in the same windows, a torch restatement of the
      paper's functions on the device (torch.cat, then DiffAugment_pytorch's color / translation / cutout with the same
      draws; its backward through autograd) and the plain torch.cat the forward replaces;
  (b) the replayed training step at the bird_style sizes (B = 20, three stages, 256 px, bf16, bench.py's networks and
      synthetic batch) with and without the flag: one fresh process per arm, the arms alternated, ms per replayed step
      over windows that end in a device synchronise; and the node counts of the two recordings.

    python tools/bench_diffaug.py [--parts ab] [--out profiles/diffaug_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'sba-gan_amd')
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

POLICY = 'color,translation,cutout'


def torch_diffaug(x, u):
    """DiffAugment_pytorch.py (Zhao et al.), f32 on the device, its random draws taken from the uniforms u [n][8]"""
    n, _, S, _ = x.shape
    col = lambda k: u[:, k].view(n, 1, 1, 1)
    x = x + (col(0) - 0.5)
    m = x.mean(dim=1, keepdim=True)
    x = (x - m) * (col(1) * 2) + m
    m = x.mean(dim=[1, 2, 3], keepdim=True)
    x = (x - m) * (col(2) + 0.5) + m
    shift, cut = int(S * 0.125 + 0.5), int(S * 0.5 + 0.5)
    draw = lambda k, hi: (u[:, k] * hi).long().clamp(max=hi - 1).view(n, 1, 1)
    tx, ty = draw(3, 2 * shift + 1) - shift, draw(4, 2 * shift + 1) - shift
    ar = torch.arange(S, device=x.device)
    gb, gx, gy = torch.meshgrid(torch.arange(n, device=x.device), ar, ar, indexing='ij')
    gx, gy = torch.clamp(gx + tx + 1, 0, S + 1), torch.clamp(gy + ty + 1, 0, S + 1)
    x = F.pad(x, [1, 1, 1, 1, 0, 0, 0, 0]).permute(0, 2, 3, 1).contiguous()[gb, gx, gy].permute(0, 3, 1, 2)
    ox, oy = draw(5, S + 1 - cut % 2), draw(6, S + 1 - cut % 2)
    ac = torch.arange(cut, device=x.device)
    gb, gx, gy = torch.meshgrid(torch.arange(n, device=x.device), ac, ac, indexing='ij')
    gx, gy = torch.clamp(gx + ox - cut // 2, 0, S - 1), torch.clamp(gy + oy - cut // 2, 0, S - 1)
    mask = torch.ones((n, S, S), dtype=x.dtype, device=x.device)
    mask[gb, gx, gy] = 0
    return x * mask.unsqueeze(1)


def windows(fns, launches, rounds):
    """us per call of every fn: `rounds` windows of `launches` calls each between two device events, the fns alternated
    window by window; returns {name: [us per window]}"""
    out = {k: [] for k in fns}
    for k, fn in fns.items():       # warm-up: code objects, the allocator's blocks
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) * 1e3 / launches)
    return out


def part_a(args):
    from sbagan import _lib
    dev = torch.device('cuda', 0)
    flags = 7
    st = torch.cuda.current_stream().cuda_stream
    rows_out = []
    for rows in (40, 20):
        for S in (64, 128, 256):
            h = rows // 2
            g = torch.Generator(device='cpu')
            g.manual_seed(S + rows)
            real = (torch.rand((h, 3, S, S), generator=g) * 2 - 1).to(dev)
            fake = (torch.rand((h, 3, S, S), generator=g) * 2 - 1).to(dev)
            u = torch.rand((rows, 8), generator=g).to(dev)
            dout = torch.randn((rows, 3, S, S), generator=g).to(dev)
            out, dx = torch.empty_like(dout), torch.empty_like(dout)
            ws = torch.empty(_lib.lib.sba_diffaug_workspace_bytes(rows, S) // 8, dtype=torch.float64, device=dev)
            fwd_args = (real.data_ptr(), h, fake.data_ptr(), h, u.data_ptr(), out.data_ptr(), S, flags, ws.data_ptr(), st)
            bwd_args = (dout.data_ptr(), rows, u.data_ptr(), dx.data_ptr(), S, flags, ws.data_ptr(), st)
            assert _lib.lib.sba_diffaug_fwd(*fwd_args) == 0 and _lib.lib.sba_diffaug_bwd(*bwd_args) == 0
            # the restatement computes what the launch computes (f32 against f32: a loose bar, the tests hold the tight one)
            leaf = torch.cat((real, fake), 0).requires_grad_(True)
            ref = torch_diffaug(leaf, u)
            (dref,) = torch.autograd.grad(ref, leaf, dout, retain_graph=True)
            err_f, err_b = float((out - ref.detach()).abs().max()), float((dx - dref).abs().max())
            assert err_f < 1e-4 and err_b < 1e-4, (err_f, err_b)

            def torch_fwd():
                return torch_diffaug(torch.cat((real, fake), 0), u)

            def torch_bwd():
                torch.autograd.grad(ref, leaf, dout, retain_graph=True)

            got = windows({'hip_fwd': lambda: _lib.lib.sba_diffaug_fwd(*fwd_args),
                           'hip_bwd': lambda: _lib.lib.sba_diffaug_bwd(*bwd_args),
                           'torch_cat': lambda: torch.cat((real, fake), 0),
                           'torch_fwd': torch_fwd, 'torch_bwd': torch_bwd}, args.launches, args.windows)
            med = {k: float(np.median(v)) for k, v in got.items()}
            nbytes = 2 * rows * 3 * S * S * 4           # every element read once and written once (the sum pass re-reads)
            row = {'rows': rows, 'S': S, 'flags': flags, 'us_median': med,
                   'us_min': {k: float(min(v)) for k, v in got.items()}, 'us_max': {k: float(max(v)) for k, v in got.items()},
                   'algorithmic_MB': nbytes / 1e6, 'hip_fwd_TBs': nbytes / med['hip_fwd'] / 1e6,
                   'hip_bwd_TBs': nbytes / med['hip_bwd'] / 1e6, 'max_abs_diff_vs_torch': [err_f, err_b]}
            rows_out.append(row)
            print('(a) %2d rows %3d px: fwd %7.2f us (%.2f TB/s), bwd %7.2f us | torch.cat %7.2f us | torch restatement '
                  'fwd %8.2f us, bwd %8.2f us' % (rows, S, med['hip_fwd'], row['hip_fwd_TBs'], med['hip_bwd'],
                                                 med['torch_cat'], med['torch_fwd'], med['torch_bwd']), flush=True)
    return {'launches_per_window': args.launches, 'windows': args.windows, 'cases': rows_out}


def step_child(args):
    """one arm of (b) in a process of its own: bench.py's step, recorded, replayed in timed windows; prints one JSON line"""
    import bench
    from sbagan.diffaug import DiffAugment
    from sbagan.synth import synthetic_batch
    from sbagan.trainer import ReplayedStep
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(0)
    bargs = argparse.Namespace(branch=3, batch=20, dtype='bf16', attn_fp8=False, variant='model',
                               image_encoder='inception', gpus=1)
    step = bench.build(bargs, dev)
    if args.child == 'on':
        step.augment = DiffAugment(POLICY, 20, 3, dev)
    b = synthetic_batch(20, branch_num=3, device=dev, seed=100)
    noise = torch.empty((20, 100), device=dev)
    torch.manual_seed(100)
    rec = ReplayedStep(step, b['imgs'], b['sent_emb'], b['words_embs'], b['mask'], b['cap_lens'], b['class_ids'], noise)
    for _ in range(args.warm_steps):
        rec.replay()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.step_windows):
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = rec.replay()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / args.steps)
    finite = all(bool(torch.isfinite(v.float()).all()) for v in out.values())
    print('CHILD ' + json.dumps({'arm': args.child, 'ms': ms, 'info': rec.info, 'finite': finite}), flush=True)


def part_b(args):
    runs = {'off': [], 'on': []}
    info = {}
    for r in range(args.rounds):
        for arm in ('off', 'on'):
            cmd = [sys.executable, os.path.abspath(__file__), '--child', arm, '--steps', str(args.steps),
                   '--step_windows', str(args.step_windows), '--warm_steps', str(args.warm_steps)]
            text = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=args.child_timeout).stdout.decode()
            line = [l for l in text.splitlines() if l.startswith('CHILD ')][-1]
            got = json.loads(line[6:])
            assert got['finite'], 'a loss of the %s arm is not finite' % arm
            runs[arm] += got['ms']
            info[arm] = got['info']
            print('(b) round %d, --diffaug %-3s: %s ms / step, %d nodes' % (r, arm, ' '.join('%.3f' % v for v in got['ms']),
                                                                             got['info']['nodes']), flush=True)
    med = {k: float(np.median(v)) for k, v in runs.items()}
    print('(b) replayed step, median: off %.3f ms, on %.3f ms (+%.3f ms, %.1f %%)'
          % (med['off'], med['on'], med['on'] - med['off'], 100 * (med['on'] / med['off'] - 1)), flush=True)
    return {'steps_per_window': args.steps, 'ms_windows': runs, 'ms_median': med, 'recording': info, 'policy': POLICY}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', default='ab')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'diffaug_bench.json'))
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--windows', type=int, default=9)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--step_windows', type=int, default=3)
    ap.add_argument('--warm_steps', type=int, default=20)
    ap.add_argument('--child_timeout', type=int, default=240)
    ap.add_argument('--child', default=None, choices=['on', 'off'], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_diffaug needs the GPU: nothing is measured without one')
    if args.child:
        return step_child(args)
    result = {'device': torch.cuda.get_device_name(0), 'torch': torch.__version__}
    if 'a' in args.parts:
        result['launches'] = part_a(args)
    if 'b' in args.parts:       # (children only: this process keeps its device context idle meanwhile)
        result['step'] = part_b(args)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
