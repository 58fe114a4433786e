"""The launch schedule of the discriminator / generator loss heads (miscc/losses.py discriminator_loss and
generator_d_term, ops.DHeadsFn), pinned call by call.

tests/golden/heads_trace.jsonl holds every C-ABI call of eight cases -- the discriminator's trunk included, so that the
wiring of its feature map into the heads is part of the record -- taken with the recorder of
tests/test_encoder_trace_gpu.py (entry point, scalars, geometry without tile / ksplit / first_write, pointers and streams
as ordinals of first appearance) from the commit BEFORE the heads became one table and one grouped path
(tools/make_golden.py heads_trace, run in that commit's tree).  The driver below therefore uses only what that commit
had: losses.discriminator_loss, losses.generator_d_term and ops.d_heads with plain tuples.  The fixture changes only when
the schedule does.

D_NET64 at the FULL dims, B = 3, 64 px: the real, fake and wrong-pair heads read 3, 3 and 2 rows at distinct offsets, so a
head wired to other rows, another order of the heads or of their gradients, or a store where an accumulation belongs
shows as a differing launch."""
import json
import os
from unittest import mock

import pytest
import torch

from helpers import FULL, d_shapes
from oracle import fill
from test_encoder_trace_gpu import Recorder, first_difference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'heads_trace.jsonl')
B, PX = 3, 64

# case -> (compute dtype, b_jcu = the discriminator has an unconditional head, what runs)
CASES = {'D5-f32': (torch.float32, True, 'd_loss'),
         'D5-bf16': (torch.bfloat16, True, 'd_loss'),
         'D3-f32': (torch.float32, False, 'd_loss'),
         'D5-real-features': (torch.float32, True, 'd_loss_real_features'),
         'D5-eval': (torch.float32, True, 'heads_eval'),
         'D5-feats-detached': (torch.float32, True, 'heads_detached'),
         'G2-frozen': (torch.float32, True, 'g_term'),
         'G1-frozen': (torch.float32, False, 'g_term')}


def _d5(n):
    """the five heads of errD over [n real | n fake] rows (losses.py:141-158): row0, rows, cond_row0, target, weight, segment"""
    return ((0, n, 0, 1., .5, 1), (n, n, 0, 0., 1. / 3, 3), (0, n - 1, 1, 0., 1. / 3, 4),
            (0, n, None, 1., .5, 0), (n, n, None, 0., 1. / 3, 2))


def run_case(name, dev):
    """the launches of one case, as Recorder normalises them"""
    import model
    from miscc import losses
    from miscc.config import cfg, reset_cfg
    from sbagan import ops
    dt, b_jcu, what = CASES[name]
    reset_cfg()
    cfg.GAN.GF_DIM, cfg.GAN.DF_DIM = 32, 64
    dt_before, det_before = ops.COMPUTE_DTYPE, ops.deterministic()
    ops.set_compute_dtype(dt)
    ops.set_deterministic(False)
    P = fill.fill_state_dict(d_shapes(FULL, 0), salt=0)
    if not b_jcu:
        P = {k: v for k, v in P.items() if not k.startswith('UNCOND_DNET')}
    net = model.D_NET64(b_jcu=b_jcu)
    net.load_state_dict(P)
    net.to(dev).train()
    real, fake = fill.uniform((B, 3, PX, PX), 960).to(dev), fill.uniform((B, 3, PX, PX), 961).to(dev)
    sent = fill.unit((B, 256), 962).to(dev)
    feats = fill.unit((2 * B, 512, 4, 4), 963).to(dev)
    ones, zeros = torch.ones(B, device=dev), torch.zeros(B, device=dev)
    ops.reduce_scratch(dev)         # (handed to the library by the first operator that uses it in a process: not a launch)
    ops.join_wgrads()
    torch.cuda.synchronize()
    try:
        with mock.patch.object(ops, 'SIDE_WGRAD', False), Recorder() as rec:
            if what == 'd_loss':
                losses.discriminator_loss(net, real, fake, sent, ones, zeros).backward()
            elif what == 'd_loss_real_features':
                sent.requires_grad_(True)
                losses.discriminator_loss(net, real, fake, sent, ones, zeros, real_features=net(real)).backward()
            elif what == 'heads_eval':      # conditional heads in groups of one, BatchNorm on its running statistics
                net.eval()
                ops.d_heads(net, feats.requires_grad_(True), sent.requires_grad_(True), _d5(B)).backward()
            elif what == 'heads_detached':  # parameter gradients only
                ops.d_heads(net, feats, sent, _d5(B)).backward()
            else:
                for p in net.parameters():
                    p.requires_grad_(False)
                losses.generator_d_term(net, fake, sent)
            ops.join_wgrads()
            torch.cuda.synchronize()
    finally:
        ops.set_compute_dtype(dt_before)
        ops.set_deterministic(det_before)
    return rec.trace


def load_golden():
    want = {}
    with open(GOLDEN) as f:
        for line in f:
            case, name, args = json.loads(line)
            want.setdefault(case, []).append([name, args])
    return want


@pytest.mark.parametrize('case', sorted(CASES))
def test_heads_launch_trace(case):
    want = load_golden()[case]
    assert len(want) > 10
    diff = first_difference(run_case(case, torch.device('cuda:0')), want)
    if diff:
        print(diff)
    assert diff is None, diff
