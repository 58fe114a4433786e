#!/usr/bin/env python3
"""--geoaug measured (run alone on the GPU, profiler off).  Writes profiles/geoaug_bench.json.

  (a) the launches alone, by device events: us per sba_geoaug_fwd (the [real | fake] concatenation and the warp), per
      sba_geoaug_bwd and per sba_geoaug_prepare at 40 rows of 256, 128 and 64 px, the median over the windows, with the
      algorithmic bytes over that time -- at the identity (the copy path), at flip / rot90 only (permutations) and at the
      full policy; beside them, in the same windows, the plain torch.cat the forward replaces and the device route in
      torch (affine_grid + grid_sample over the concatenation with the same matrices; its backward through autograd,
      which scatters with float atomics);
  (b) the replayed training step at the bird_style sizes (B = 20, three stages, 256 px, bf16, bench.py's networks and
      synthetic batch) without augmentation, with --geoaug alone, with --diffaug --diffaug_p 0.5 --ada 0.6 and with
      both: one fresh process per arm, the arms alternated, ms per replayed step over windows that end in a device
      synchronise; and the kernel counts of the recordings.

    python tools/bench_geoaug.py [--parts ab] [--out profiles/geoaug_bench.json]
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

DIFFAUG, GEO = 'color,translation,cutout', 'flip,rot90,scale,rotate'
ARMS = ('off', 'geo', 'ada', 'ada_geo')
POLICIES = (('identity', 0), ('flip_rot90', 3), ('full', 15))


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


def torch_route(x, mats):
    n, _, S, _ = x.shape
    theta = torch.zeros((n, 2, 3), dtype=x.dtype, device=x.device)
    theta[:, :, :2] = mats.view(n, 2, 2)
    return F.grid_sample(x, F.affine_grid(theta, (n, 3, S, S), align_corners=True), 'bilinear', 'zeros',
                         align_corners=True)


def part_a(args):
    from sbagan import _lib
    dev = torch.device('cuda', 0)
    st = torch.cuda.current_stream().cuda_stream
    lib = _lib.lib
    rows, cases = 40, []
    for S in (256, 128, 64):
        h = rows // 2
        g = torch.Generator(device='cpu')
        g.manual_seed(S + rows)
        real = (torch.rand((h, 3, S, S), generator=g) * 2 - 1).to(dev)
        fake = (torch.rand((h, 3, S, S), generator=g) * 2 - 1).to(dev)
        u = torch.rand((rows, 8), generator=g).to(dev)
        dout = torch.randn((rows, 3, S, S), generator=g).to(dev)
        out, dx = torch.empty_like(dout), torch.empty_like(dout)
        applied = torch.zeros(rows, dtype=torch.int32, device=dev)
        for name, flags in POLICIES:
            mats = torch.zeros((rows, 4), device=dev)
            if flags:
                assert lib.sba_geoaug_prepare(u.data_ptr(), None, None, 1, rows, flags, mats.data_ptr(), applied.data_ptr(),
                                              st) == 0
            else:
                mats[:, 0] = mats[:, 3] = 1
            prep_args = (u.data_ptr(), None, None, 1, rows, flags or 15, out.data_ptr(), applied.data_ptr(), st)
            fwd_args = (real.data_ptr(), h, fake.data_ptr(), h, mats.data_ptr(), out.data_ptr(), S, st)
            bwd_args = (dout.data_ptr(), rows, mats.data_ptr(), dx.data_ptr(), S, st)
            assert lib.sba_geoaug_fwd(*fwd_args) == 0 and lib.sba_geoaug_bwd(*bwd_args) == 0
            # the torch route computes what the launches compute (f32 against f32: a loose bar, the tests hold the tight one)
            leaf = torch.cat((real, fake), 0).requires_grad_(True)
            ref = torch_route(leaf, mats)
            (dref,) = torch.autograd.grad(ref, leaf, dout, retain_graph=True)
            err_f, err_b = float((out - ref.detach()).abs().max()), float((dx - dref).abs().max())
            assert err_f < 1e-2 and err_b < 1e-2, (err_f, err_b)

            def torch_bwd():
                torch.autograd.grad(ref, leaf, dout, retain_graph=True)

            got = windows({'hip_fwd': lambda: lib.sba_geoaug_fwd(*fwd_args),
                           'hip_bwd': lambda: lib.sba_geoaug_bwd(*bwd_args),
                           'hip_prepare': lambda: lib.sba_geoaug_prepare(*prep_args),
                           'torch_cat': lambda: torch.cat((real, fake), 0),
                           'torch_fwd': lambda: torch_route(torch.cat((real, fake), 0), mats),
                           'torch_bwd': torch_bwd}, args.launches, args.windows)
            med = {k: float(np.median(v)) for k, v in got.items()}
            nbytes = 2 * rows * 3 * S * S * 4           # every element read once (taps from cache) and written once
            case = {'rows': rows, 'S': S, 'policy': name, 'flags': flags, 'us_median': med,
                    'us_min': {k: float(min(v)) for k, v in got.items()},
                    'us_max': {k: float(max(v)) for k, v in got.items()},
                    'algorithmic_MB': nbytes / 1e6, 'hip_fwd_TBs': nbytes / med['hip_fwd'] / 1e6,
                    'hip_bwd_TBs': nbytes / med['hip_bwd'] / 1e6, 'max_abs_diff_vs_torch': [err_f, err_b]}
            cases.append(case)
            print('(a) %3d px %-10s: fwd %7.2f us (%.2f TB/s), bwd %7.2f us, prepare %5.2f us | torch.cat %7.2f us | '
                  'torch route fwd %8.2f us, bwd %8.2f us' % (S, name, med['hip_fwd'], case['hip_fwd_TBs'], med['hip_bwd'],
                                                             med['hip_prepare'], med['torch_cat'], med['torch_fwd'],
                                                             med['torch_bwd']), flush=True)
    return {'launches_per_window': args.launches, 'windows': args.windows, 'cases': cases}


def step_child(args):
    """one arm of (b) in a process of its own: bench.py's step, recorded, replayed in timed windows; prints one JSON line"""
    import bench
    from sbagan.diffaug import DiffAugment
    from sbagan.geoaug import GeoAugment
    from sbagan.synth import synthetic_batch
    from sbagan.trainer import ReplayedStep
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(0)
    bargs = argparse.Namespace(branch=3, batch=20, dtype='bf16', attn_fp8=False, variant='model',
                               image_encoder='inception', gpus=1)
    step = bench.build(bargs, dev)
    if args.child in ('ada', 'ada_geo'):
        step.augment = DiffAugment(DIFFAUG, 20, 3, dev, p0=0.5, target=0.6)
    if args.child in ('geo', 'ada_geo'):
        step.geo_augment = GeoAugment(GEO, 20, 3, dev, p=None if step.augment is None else step.augment.p)
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
    p = None if step.augment is None else step.augment.p.tolist()
    print('CHILD ' + json.dumps({'arm': args.child, 'ms': ms, 'info': rec.info, 'finite': finite, 'p': p}), flush=True)


def part_b(args):
    arms = [a for a in args.arms.split(',') if a]
    runs = {a: [] for a in arms}
    info = {}
    for r in range(args.rounds):
        for arm in arms:
            cmd = [sys.executable, os.path.abspath(__file__), '--child', arm, '--steps', str(args.steps),
                   '--step_windows', str(args.step_windows), '--warm_steps', str(args.warm_steps)]
            text = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=args.child_timeout).stdout.decode()
            line = [ln for ln in text.splitlines() if ln.startswith('CHILD ')][-1]
            got = json.loads(line[6:])
            assert got['finite'], 'a loss of the %s arm is not finite' % arm
            runs[arm] += got['ms']
            info[arm] = dict(got['info'], p=got['p'])
            print('(b) round %d, %-8s: %s ms / step, %d kernels' % (r, arm, ' '.join('%.3f' % v for v in got['ms']),
                                                                   got['info']['kernels']), flush=True)
    med = {k: float(np.median(v)) for k, v in runs.items()}
    print('(b) replayed step, median ms: ' + ', '.join('%s %.3f' % (k, v) for k, v in med.items()), flush=True)
    return {'steps_per_window': args.steps, 'ms_windows': runs, 'ms_median': med, 'recording': info,
            'policies': {'diffaug': DIFFAUG, 'geoaug': GEO}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', default='ab')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'geoaug_bench.json'))
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--windows', type=int, default=9)
    ap.add_argument('--arms', default=','.join(ARMS))
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--step_windows', type=int, default=3)
    ap.add_argument('--warm_steps', type=int, default=20)
    ap.add_argument('--child_timeout', type=int, default=240)
    ap.add_argument('--child', default=None, choices=list(ARMS), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_geoaug needs the GPU: nothing is measured without one')
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
