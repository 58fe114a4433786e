#!/usr/bin/env python3
"""One SHA-256 per result of the Inception trunk driver (sbagan/inception_hip.py) at the four cases of
tests/test_encoder_trace_gpu.py (N = 2, 64 px input): features, code, the image gradient, last_pooled, the outputs of
trunk_features(train=True) and pooled_features, and the BatchNorm running statistics afterwards.  It uses only what the
driver has always offered, so the same file runs in a checkout of an older commit: run it there and here, each in a
fresh process, and diff the listings -- a refactor of the driver must leave every 'det' line equal (deterministic-reduction
mode); a 'default' line may differ only where split-K partial sums are added by atomics.

    python tools/encoder_bytes.py > branch.txt"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'sba-gan_amd'))
import torch  # noqa: E402

import model  # noqa: E402
from sbagan import ops  # noqa: E402
from sbagan.inception_hip import InceptionHIP  # noqa: E402

CASES = (('bf16-group-fwd-bwd', torch.bfloat16, 'fwd_bwd'),
         ('f32-streams-fwd-bwd', torch.float32, 'fwd_bwd'),
         ('f32-trunk-features-train', torch.float32, 'trunk_train'),
         ('bf16-pooled-features', torch.bfloat16, 'pooled'))


def run_case(dt, what, dev):
    ops.set_compute_dtype(dt)
    torch.manual_seed(7)
    enc = model.CNN_ENCODER(256).to(dev)
    enc.train(what == 'trunk_train')
    img = (torch.rand(2, 3, 64, 64, device=dev) * 2 - 1).requires_grad_(what == 'fwd_bwd')
    gf, gc = torch.randn(2, 256, 17, 17, device=dev), torch.randn(2, 256, device=dev)
    run = InceptionHIP(enc)
    ops.det_reset()
    if what == 'fwd_bwd':
        f, c = run(img)
        pooled = run.last_pooled
        (g,) = torch.autograd.grad([f, c], img, [gf, gc])
        out = dict(features=f, code=c, dimg=g, last_pooled=pooled)
    elif what == 'trunk_train':
        f768, pooled = run.trunk_features(img, train=True)
        out = dict(f768=f768, pooled=pooled, last_pooled=run.last_pooled)
    else:
        out = dict(last_pooled=run.pooled_features(img))
    bufs = sorted((k, v) for k, v in enc.state_dict().items() if k.endswith(('running_mean', 'running_var', 'num_batches_tracked')))
    out['bn_buffers'] = torch.cat([v.detach().double().flatten() for _, v in bufs])
    return out


def main():
    dev = torch.device('cuda:0')
    for part in ('det', 'default'):
        ops.set_deterministic(part == 'det', dev)
        for name, dt, what in CASES:
            res = run_case(dt, what, dev)
            torch.cuda.synchronize()
            for k, t in res.items():
                h = hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()
                print('%-8s %-26s %-12s %s' % (part, name, k, h), flush=True)


if __name__ == '__main__':
    main()
