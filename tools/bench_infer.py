#!/usr/bin/env python3
"""Generator-only inference timing: the existing netG.eval() forward against sbagan.infer.FusedGenerator in the SAME
process on the same inputs -- B = 20, three stages built, timed up to the 64 / 128 / 256 px output, bf16 and f32.

Device events around each forward, the two paths alternated call by call after a warm-up, median and spread (the
interquartile range of the per-call times) per path.  Also: the last upBlock alone (64 -> 2 x 32 channels to 256 x 256),
with the output-side bytes predicted from its shapes and the achieved GB/s.

    python tools/bench_infer.py [--reps 30] [--warmup 5] [--out profiles/infer_bench.json]
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


def _time_alternating(fns, reps, warmup):
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    out = {}
    for k, t in times.items():
        q1, med, q3 = np.percentile(t, [25, 50, 75])
        out[k] = dict(median_ms=float(med), iqr_ms=float(q3 - q1), min_ms=float(min(t)), n=len(t))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=20)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_infer.py measures on the GPU: no device visible')
    from miscc.config import cfg
    from oracle import fill
    from sbagan import ops
    from sbagan.infer import FusedGenerator
    import model
    dev = torch.device('cuda:0')
    B, L = args.batch, 18
    res = dict(batch=B, reps=args.reps, warmup=args.warmup, device=torch.cuda.get_device_name(0), generator={},
               last_upblock={})
    for dt in (torch.bfloat16, torch.float32):
        ops.set_compute_dtype(dt)
        name = 'bf16' if dt == torch.bfloat16 else 'f32'
        for branch in (1, 2, 3):
            cfg.GAN.GF_DIM, cfg.TREE.BRANCH_NUM = 32, branch
            net = model.G_NET()
            net.load_state_dict(fill.fill_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}))
            net.to(dev).eval()
            net.set_return_attention(False)
            z, sent = fill.unit((B, 100), 1).to(dev), fill.unit((B, 256), 2).to(dev)
            words = fill.unit((B, 256, L), 3).to(dev)
            caps, _ = fill.synthetic_captions(B, L, L, tag=5)
            mask = (caps == 0)[:, :L].to(dev)
            net.ca_net.eps = fill.unit((B, 100), 4).to(dev)
            fused = FusedGenerator(net)
            with torch.no_grad():
                r = _time_alternating({'unfused': lambda: net(z, sent, words, mask),
                                       'fused': lambda: fused(z, sent, words, mask)}, args.reps, args.warmup)
            spread = max(r['unfused']['iqr_ms'], r['fused']['iqr_ms'])
            r['gain_ms'] = r['unfused']['median_ms'] - r['fused']['median_ms']
            r['faster_beyond_spread'] = bool(r['gain_ms'] > spread)
            res['generator']['%s_%dpx' % (name, 64 << (branch - 1))] = r
            print(name, 64 << (branch - 1), json.dumps(r), flush=True)
            if branch == 3:
                up = net.h_net3.upsample
                x = ops.as_act(fill.unit((B, 64, 128, 128), 7).to(dev), dt)
                with torch.no_grad():
                    r = _time_alternating({'unfused': lambda: up(x), 'fused': lambda: fused.conv_glu(up, x)},
                                          args.reps, args.warmup)
                es = 2 if dt == torch.bfloat16 else 4
                pix = B * 256 * 256
                r['bytes_model'] = dict(input=B * 128 * 128 * 64 * es, unfused_output_side=pix * (64 + 64 + 32) * es,
                                        fused_output_side=pix * 32 * es)
                for k in ('unfused', 'fused'):
                    byt = r['bytes_model']['input'] + r['bytes_model'][k + '_output_side']
                    r[k]['achieved_GBps'] = byt / (r[k]['median_ms'] * 1e-3) / 1e9
                res['last_upblock'][name] = r
                print(name, 'last upBlock', json.dumps(r), flush=True)
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
