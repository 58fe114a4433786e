#!/usr/bin/env python3
"""--diffaug_p / --ada measured (run alone on the GPU, profiler off).  Writes profiles/ada_bench.json.
The protocol of tools/bench_diffaug.py (its `windows` and its child processes are used as they are):

  (a) the launches alone, by device events: us per sba_diffaug_gated_fwd / _bwd at p = 0, 0.5 and 1 (fresh uniform
      gates) at 40 rows of 256, 128 and 64 px, policy color,translation,cutout, the median over 9 windows of 200
      launches; in the same windows the ungated pair and the plain torch.cat the forward replaces; and the two
      controller launches (sba_ada_count over 40 probabilities, sba_ada_adjust over 3 rows);
  (b) the replayed training step at the bird_style sizes (B = 20, three stages, 256 px, bf16, bench.py's networks and
      synthetic batch), one fresh process per arm, the arms alternated: --diffaug alone (the comparison), --diffaug
      --diffaug_p 0.5, --diffaug --ada 0.6; ms per replayed step and the node counts of the recordings.

    python tools/bench_ada.py [--parts ab] [--out profiles/ada_bench.json]
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

from bench_diffaug import POLICY, windows  # noqa: E402

ARMS = ('diffaug', 'fixed_p', 'ada')


def part_a(args):
    from sbagan import _lib
    dev = torch.device('cuda', 0)
    flags, rows = 7, 40
    st = torch.cuda.current_stream().cuda_stream
    lib = _lib.lib
    cases = []
    for S in (256, 128, 64):
        h = rows // 2
        g = torch.Generator(device='cpu')
        g.manual_seed(S + rows)
        real = (torch.rand((h, 3, S, S), generator=g) * 2 - 1).to(dev)
        fake = (torch.rand((h, 3, S, S), generator=g) * 2 - 1).to(dev)
        u = torch.rand((rows, 8), generator=g).to(dev)
        gates = torch.rand((rows, 4), generator=g).to(dev)
        dout = torch.randn((rows, 3, S, S), generator=g).to(dev)
        out, dx = torch.empty_like(dout), torch.empty_like(dout)
        ws = torch.empty(lib.sba_diffaug_workspace_bytes(rows, S) // 8, dtype=torch.float64, device=dev)
        fns = {'ungated_fwd': lambda: lib.sba_diffaug_fwd(real.data_ptr(), h, fake.data_ptr(), h, u.data_ptr(),
                                                          out.data_ptr(), S, flags, ws.data_ptr(), st),
               'ungated_bwd': lambda: lib.sba_diffaug_bwd(dout.data_ptr(), rows, u.data_ptr(), dx.data_ptr(), S, flags,
                                                          ws.data_ptr(), st),
               'torch_cat': lambda: torch.cat((real, fake), 0)}
        keep, parts_on = [], {}
        for p in (0.0, 0.5, 1.0):
            p_dev = torch.tensor([p], device=dev)
            applied = torch.empty(rows, dtype=torch.int32, device=dev)
            keep += [p_dev, applied]
            fwd = (real.data_ptr(), h, fake.data_ptr(), h, u.data_ptr(), gates.data_ptr(), p_dev.data_ptr(),
                   out.data_ptr(), applied.data_ptr(), S, flags, ws.data_ptr(), st)
            bwd = (dout.data_ptr(), rows, u.data_ptr(), applied.data_ptr(), dx.data_ptr(), S, flags, ws.data_ptr(), st)
            assert lib.sba_diffaug_gated_fwd(*fwd) == 0 and lib.sba_diffaug_gated_bwd(*bwd) == 0
            parts_on['%g' % p] = int(sum(bin(v).count('1') for v in applied.tolist()))
            fns['gated_fwd_p%g' % p] = lambda a=fwd: lib.sba_diffaug_gated_fwd(*a)
            fns['gated_bwd_p%g' % p] = lambda a=bwd: lib.sba_diffaug_gated_bwd(*a)
        got = windows(fns, args.launches, args.windows)
        med = {k: float(np.median(v)) for k, v in got.items()}
        cases.append({'rows': rows, 'S': S, 'flags': flags, 'us_median': med,
                      'us_min': {k: float(min(v)) for k, v in got.items()},
                      'us_max': {k: float(max(v)) for k, v in got.items()}, 'parts_applied_of_120': parts_on})
        print('(a) %d rows %3d px: fwd ungated %6.2f | gated p=0 %6.2f  p=.5 %6.2f  p=1 %6.2f | cat %6.2f us; '
              'bwd ungated %6.2f | gated p=0 %6.2f  p=.5 %6.2f  p=1 %6.2f us'
              % (rows, S, med['ungated_fwd'], med['gated_fwd_p0'], med['gated_fwd_p0.5'], med['gated_fwd_p1'],
                 med['torch_cat'], med['ungated_bwd'], med['gated_bwd_p0'], med['gated_bwd_p0.5'], med['gated_bwd_p1']),
              flush=True)
    prob = torch.rand(40, device=dev)
    state = torch.zeros((2, 3), device=dev)
    counters = torch.zeros((3, 4), dtype=torch.int32, device=dev)
    got = windows({'ada_count': lambda: lib.sba_ada_count(prob.data_ptr(), 40, counters.data_ptr(), st),
                   'ada_adjust': lambda: lib.sba_ada_adjust(state[0].data_ptr(), state[1].data_ptr(),
                                                            counters.data_ptr(), 3, 4, 0.6, 1.6e-4, 1.0, st)},
                  args.launches, args.windows)
    ctl = {k: float(np.median(v)) for k, v in got.items()}
    print('(a) controller: count %.2f us, adjust %.2f us' % (ctl['ada_count'], ctl['ada_adjust']), flush=True)
    return {'launches_per_window': args.launches, 'windows': args.windows, 'cases': cases, 'controller_us_median': ctl}


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
    kw = {'diffaug': {}, 'fixed_p': {'p0': 0.5}, 'ada': {'target': 0.6}}[args.child]
    step.augment = DiffAugment(POLICY, 20, 3, dev, **kw)
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
    report = step.augment.report() if step.augment.gated else None
    print('CHILD ' + json.dumps({'arm': args.child, 'ms': ms, 'info': rec.info, 'finite': finite, 'p_rt': report}),
          flush=True)


def part_b(args):
    runs, info, last = {k: [] for k in ARMS}, {}, {}
    for r in range(args.rounds):
        for arm in ARMS:
            cmd = [sys.executable, os.path.abspath(__file__), '--child', arm, '--steps', str(args.steps),
                   '--step_windows', str(args.step_windows), '--warm_steps', str(args.warm_steps)]
            text = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=args.child_timeout).stdout.decode()
            got = json.loads([ln for ln in text.splitlines() if ln.startswith('CHILD ')][-1][6:])
            assert got['finite'], 'a loss of the %s arm is not finite' % arm
            runs[arm] += got['ms']
            info[arm], last[arm] = got['info'], got['p_rt']
            print('(b) round %d, %-8s: %s ms / step, %d nodes' % (r, arm, ' '.join('%.3f' % v for v in got['ms']),
                                                                   got['info']['nodes']), flush=True)
    med = {k: float(np.median(v)) for k, v in runs.items()}
    print('(b) replayed step, median: --diffaug %.3f ms, --diffaug_p 0.5 %.3f ms (%+.3f), --ada 0.6 %.3f ms (%+.3f)'
          % (med['diffaug'], med['fixed_p'], med['fixed_p'] - med['diffaug'], med['ada'], med['ada'] - med['diffaug']),
          flush=True)
    return {'steps_per_window': args.steps, 'ms_windows': runs, 'ms_median': med, 'recording': info, 'policy': POLICY,
            'p_and_rt_at_the_end': last}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', default='ab')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ada_bench.json'))
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--windows', type=int, default=9)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--step_windows', type=int, default=3)
    ap.add_argument('--warm_steps', type=int, default=20)
    ap.add_argument('--child_timeout', type=int, default=240)
    ap.add_argument('--child', default=None, choices=list(ARMS), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_ada needs the GPU: nothing is measured without one')
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
