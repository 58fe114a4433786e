"""The launch schedule of the Inception trunk driver (sbagan/inception_hip.py), pinned launch by launch.

tests/golden/encoder_trace.jsonl holds every C-ABI call the driver makes in four cases, recorded through
sbagan._lib.AUDIT_HOOK (tools/make_golden.py encoder_trace) from the driver of the commit BEFORE its three issue modes
became one block scheduler: entry point, scalar arguments, the sba_conv_geom fields the driver itself sets (not tile /
ksplit / first_write, which ops.tune_geom and the launcher fill from the tile table), the tile id and the items of a grouped
launch.  Device pointers and stream handles appear as the ordinal of their first appearance in the case's trace; while a
trace records, every tensor whose address is taken stays alive, so that one ordinal is one tensor and not whatever the
caching allocator put at a recycled address.  The fixture changes only when the driver's schedule does."""
import ctypes
import json
import os
from unittest import mock

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'encoder_trace.jsonl')

# (case, compute dtype, what runs).  N = 2 (the smallest batch at which training-mode BatchNorm means anything), 64 px input:
# the trunk runs at 299 px whatever the input size.
CASES = (('bf16-group-fwd-bwd', torch.bfloat16, 'fwd_bwd'),
         ('f32-streams-fwd-bwd', torch.float32, 'fwd_bwd'),
         ('f32-trunk-features-train', torch.float32, 'trunk_train'),
         ('bf16-pooled-features', torch.bfloat16, 'pooled'))
N, PX = 2, 64
GEOM_SKIP = ('tile', 'ksplit', 'first_write')


def _geom(g):
    out = []
    for name, _ in type(g)._fields_:
        if name in ('ty', 'tx'):
            out.append(list(getattr(g, name))[:g.ntaps])
        elif name not in GEOM_SKIP:
            out.append(getattr(g, name))
    return out


class Recorder(object):
    """with Recorder() as r: ... ; r.trace = [[entry point, normalised arguments], ...]"""

    def __enter__(self):
        from sbagan import _lib
        self._lib, self.trace, self._ptr, self._stream, self._alive = _lib, [], {}, {}, []
        data_ptr, alive = torch.Tensor.data_ptr, self._alive

        def pinned(t):
            alive.append(t)
            return data_ptr(t)
        self._patch = mock.patch.object(torch.Tensor, 'data_ptr', pinned)
        self._patch.start()
        self._prev, _lib.AUDIT_HOOK = _lib.AUDIT_HOOK, self._on_call
        return self

    def __exit__(self, *exc):
        self._lib.AUDIT_HOOK = self._prev
        self._patch.stop()
        del self._alive[:]

    @staticmethod
    def _ordinal(table, prefix, a):
        a = a.value if hasattr(a, 'value') else a
        if not a and prefix == 'p':
            return None
        return prefix + str(table.setdefault(int(a or 0), len(table)))

    def _on_call(self, name, args):
        sig, out = self._lib.SIGNATURES[name], []
        for i, (a, t) in enumerate(zip(args, sig)):
            if t is ctypes.c_void_p:
                stream = i == len(sig) - 1
                out.append(self._ordinal(self._stream if stream else self._ptr, 's' if stream else 'p', a))
            elif t is self._lib.G:
                out.append(_geom(a._obj))
            elif isinstance(a, ctypes.Array):           # the items of a grouped launch
                out.append([[self._ordinal(self._ptr, 'p', p) for p in (it.x, it.w, it.y, it.addend, it.bias, it.relu_mask)]
                            + [_geom(it.g.contents)] for it in a])
            else:
                out.append(a)
        self.trace.append([name, out])


def run_case(module, dt, what, dev):
    """the launches of one case by the driver in `module` (sbagan.inception_hip, or the recorder's copy of an older one)"""
    import model
    from sbagan import ops
    ops.set_compute_dtype(dt)
    torch.manual_seed(7)
    enc = model.CNN_ENCODER(256).to(dev)
    enc.train(what == 'trunk_train')
    img = (torch.rand(N, 3, PX, PX, device=dev) * 2 - 1).requires_grad_(what == 'fwd_bwd')
    gf, gc = torch.randn(N, 256, 17, 17, device=dev), torch.randn(N, 256, device=dev)
    run = module.InceptionHIP(enc)
    torch.cuda.synchronize()
    with Recorder() as rec:
        if what == 'fwd_bwd':
            f, c = run(img)
            torch.autograd.grad([f, c], img, [gf, gc])
        elif what == 'trunk_train':
            run.trunk_features(img, train=True)
        else:
            run.pooled_features(img)
        torch.cuda.synchronize()
    return rec.trace


def load_golden():
    want = {}
    with open(GOLDEN) as f:
        for line in f:
            case, name, args = json.loads(line)
            want.setdefault(case, []).append([name, args])
    return want


def first_difference(got, want):
    """None, or a description of the first launch at which two traces differ"""
    got = json.loads(json.dumps(got))           # (tuples and ctypes ints as the fixture holds them)
    for i, (a, b) in enumerate(zip(got, want)):
        if a != b:
            return 'launch %d:\n  got      %s\n  expected %s' % (i, json.dumps(a), json.dumps(b))
    if len(got) != len(want):
        return '%d launches, expected %d; the first %d agree' % (len(got), len(want), min(len(got), len(want)))
    return None


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_encoder_launch_trace(case):
    from sbagan import inception_hip
    name, dt, what = case
    want = load_golden()[name]
    assert len(want) > 50
    diff = first_difference(run_case(inception_hip, dt, what, torch.device('cuda:0')), want)
    if diff:
        print(diff)
    assert diff is None, diff
