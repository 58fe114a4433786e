"""--diffaug_p / --ada on the device.  The gated kernels through the C ABI on guarded buffers against the EXISTING entry
points image by image (the contract is bit equality: no tolerance anywhere in this file), the two controller kernels
against the integer / float32 reference of tests/ada_ref.py, the operator, and the training step: fixed p = 1 and p = 0
against the steps they must reproduce, the counters against the probabilities they counted, the recorded loop against
the eager one, the launches each flag adds, the stream audit, and the entry point with its log line and checkpoint."""
import json
import os

import numpy as np
import pytest
import torch

import ada_ref as A
from test_diffaug_gpu import FILL, GUARD, body, gpu_params, guarded, guards_intact, ptr, workspace

pytestmark = pytest.mark.gpu

SIZES = [8, 10, 64, 96]         # smallest; rows no multiple of 4 pixels; one partial sum per image; two
BATCHES = [(8, 8), (0, 16), (16, 0), (1, 0)]
SENTINEL = -77
_CASES = {}


def i32(t):
    return t.contiguous().view(torch.int32)


def hand_gates(n):
    """gates of 0.25 / 0.75: with p = 0.5 image k gets g = (7 - k) % 8 -- all eight values, twice in 16 images"""
    g = np.full((n, 4), 0.75, dtype=np.float32)
    for k in range(n):
        for b in range(3):
            if ((7 - k) % 8) >> b & 1:
                g[k, b] = 0.25
    g[:, 3] = 9.0               # the unused column: nothing may depend on it
    return g


def case(S, n):
    key = (S, n)
    if key not in _CASES:
        rng = np.random.RandomState(100 * S + n)
        x = rng.standard_normal((n, 3, S, S)).astype(np.float32)
        x[0, 0, 0, 0] = -0.0
        _CASES[key] = {'x': x, 'g': rng.standard_normal((n, 3, S, S)).astype(np.float32),
                       'params': gpu_params(max(n, 3), 31 * S + n)[:n]}
    return _CASES[key]


def stream():
    return torch.cuda.current_stream().cuda_stream


def plain_fwd(x, params, S, flags, dev):
    """the EXISTING forward entry point over the images x (all as `fake`); returns [n][3][S][S] on the device"""
    from sbagan import _lib
    n = x.shape[0]
    out = guarded(n * 3 * S * S, dev)
    ws = workspace(n, S, dev)
    assert _lib.lib.sba_diffaug_fwd(None, 0, ptr(x), n, ptr(params), ptr(out, GUARD), S, flags, ptr(ws), stream()) == 0
    torch.cuda.synchronize()
    assert guards_intact(out)
    return body(out).view(n, 3, S, S)


def plain_bwd(g, params, S, flags, dev):
    from sbagan import _lib
    n = g.shape[0]
    dx = guarded(n * 3 * S * S, dev)
    ws = workspace(n, S, dev)
    assert _lib.lib.sba_diffaug_bwd(ptr(g), n, ptr(params), ptr(dx, GUARD), S, flags, ptr(ws), stream()) == 0
    torch.cuda.synchronize()
    assert guards_intact(dx)
    return body(dx).view(n, 3, S, S)


def gated_fwd(x, nr, params, gates, p, S, flags, dev):
    """sba_diffaug_gated_fwd over [real = x[:nr] | fake = x[nr:]]; returns (guarded out, guarded applied)"""
    from sbagan import _lib
    n = x.shape[0]
    real = x[:nr].contiguous() if nr else None
    fake = x[nr:].contiguous() if n - nr else None
    out = guarded(n * 3 * S * S, dev)
    applied = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    ws = workspace(n, S, dev)
    p_dev = torch.tensor([p], dtype=torch.float32, device=dev)
    rc = _lib.lib.sba_diffaug_gated_fwd(ptr(real), nr, ptr(fake), n - nr, ptr(params), ptr(gates), ptr(p_dev),
                                        ptr(out, GUARD), ptr(applied, GUARD), S, flags, ptr(ws), stream())
    assert rc == 0
    torch.cuda.synchronize()
    return out, applied


def gated_bwd(g, params, applied, S, flags, dev):
    from sbagan import _lib
    n = g.shape[0]
    dx = guarded(n * 3 * S * S, dev)
    ws = workspace(n, S, dev)
    rc = _lib.lib.sba_diffaug_gated_bwd(ptr(g), n, ptr(params), ptr(applied), ptr(dx, GUARD), S, flags, ptr(ws),
                                        stream())
    assert rc == 0
    torch.cuda.synchronize()
    return dx


def applied_intact(t):
    return bool((t[:GUARD] == SENTINEL).all()) and bool((t[-GUARD:] == SENTINEL).all())


def check_against_the_plain_entry_points(got, src, params, f, S, dev, plain):
    """image n of `got` has the bits of the plain entry point with flags f[n] on that image; f[n] = 0: of src[n]"""
    for value in sorted(set(f.tolist())):
        idx = torch.from_numpy(np.flatnonzero(f == value)).to(dev)
        if value == 0:
            want = src[idx]
        else:
            want = plain(src[idx].contiguous(), params[idx].contiguous(), S, int(value), dev)
        assert torch.equal(i32(got[idx]), i32(want)), (S, value)


@pytest.mark.parametrize('flags', [7, 5])
@pytest.mark.parametrize('nr,nf', BATCHES)
@pytest.mark.parametrize('S', SIZES)
def test_gated_forward_and_backward_have_the_bits_of_the_ungated_kernels(S, nr, nf, flags):
    dev = torch.device('cuda', 0)
    n = nr + nf
    c = case(S, n)
    x, g, params = (torch.from_numpy(c[k]).to(dev) for k in ('x', 'g', 'params'))
    gates_np = hand_gates(n)
    gates = torch.from_numpy(gates_np).to(dev)
    f = A.applied(gates_np, 0.5, flags)
    if n == 16:
        assert sorted(A.gate_bits(gates_np, 0.5).tolist()) == sorted(list(range(8)) * 2)
    out_t, app_t = gated_fwd(x, nr, params, gates, 0.5, S, flags, dev)
    assert guards_intact(out_t) and applied_intact(app_t)
    applied = app_t[GUARD:-GUARD]
    assert applied.cpu().numpy().tolist() == f.tolist()
    out = body(out_t).view(n, 3, S, S)
    check_against_the_plain_entry_points(out, x, params, f, S, dev, plain_fwd)
    dx_t = gated_bwd(g, params, applied, S, flags, dev)
    assert guards_intact(dx_t)
    check_against_the_plain_entry_points(body(dx_t).view(n, 3, S, S), g, params, f, S, dev, plain_bwd)
    # twice: the same bits
    out2, app2 = gated_fwd(x, nr, params, gates, 0.5, S, flags, dev)
    assert torch.equal(i32(out_t), i32(out2)) and torch.equal(app_t, app2)
    assert torch.equal(i32(dx_t), i32(gated_bwd(g, params, applied, S, flags, dev)))


def test_gated_edges():
    dev = torch.device('cuda', 0)
    S, nr, nf, flags = 10, 3, 3, 7
    n = nr + nf
    c = case(S, n)
    x, g, params = (torch.from_numpy(c[k]).to(dev) for k in ('x', 'g', 'params'))
    gates_np = np.random.RandomState(5).random_sample((n, 4)).astype(np.float32)
    gates = torch.from_numpy(gates_np).to(dev)
    whole = plain_fwd(x, params, S, flags, dev)
    assert not torch.equal(whole, x)
    for p, want, f in ((0.0, x, 0), (-0.0, x, 0), (float('nan'), x, 0), (1.0, whole, 7), (2.0, whole, 7),
                       (float('inf'), whole, 7)):
        out_t, app_t = gated_fwd(x, nr, params, gates, p, S, flags, dev)
        assert guards_intact(out_t) and applied_intact(app_t)
        assert torch.equal(i32(body(out_t).view(n, 3, S, S)), i32(want)), p          # p = 0: the bits of torch.cat
        assert app_t[GUARD:-GUARD].tolist() == [f] * n, p
    # a gate equal to p is not applied; the next float32 below it is
    p = 0.625
    below = float(np.nextafter(np.float32(p), np.float32(0)))
    eq = torch.tensor([[p, p, p, 0.0], [below, p, p, 0.0], [p, below, p, 0.0], [p, p, below, 0.0],
                       [below, below, below, 0.0], [p, p, p, 0.0]], dtype=torch.float32, device=dev)
    out_t, app_t = gated_fwd(x, nr, params, eq, p, S, flags, dev)
    f = np.array([0, 1, 2, 4, 7, 0])
    assert app_t[GUARD:-GUARD].tolist() == f.tolist() == A.applied(eq.cpu().numpy(), p, flags).tolist()
    check_against_the_plain_entry_points(body(out_t).view(n, 3, S, S), x, params, f, S, dev, plain_fwd)
    # backward: any int32 in `applied` is masked with flags, never an address
    for flags in (7, 6):
        raw = torch.tensor([8, -1, 0x7fffffff, -8, 1, 0x7ffffff8], dtype=torch.int32, device=dev)
        f = raw.cpu().numpy().astype(np.int64) & flags
        assert f.tolist() == [0, flags, flags, 0, 1 & flags, 0]
        dx_t = gated_bwd(g, params, raw, S, flags, dev)
        assert guards_intact(dx_t)
        check_against_the_plain_entry_points(body(dx_t).view(n, 3, S, S), g, params, f, S, dev, plain_bwd)
        assert np.array_equal(A.backward(c['g'], c['params'], raw.cpu().numpy(), flags).view(np.int32)[f == 0],
                              c['g'].view(np.int32)[f == 0])


def test_gated_refusals_write_nothing():
    from sbagan import _lib
    dev = torch.device('cuda', 0)
    S, nr, nf = 8, 2, 2
    n = nr + nf
    real, fake = torch.zeros((nr, 3, S, S), device=dev), torch.zeros((nf, 3, S, S), device=dev)
    params = torch.from_numpy(gpu_params(n, 1)).to(dev)
    gates = torch.full((n + 1, 4), 0.25, device=dev)
    p_dev = torch.ones(4, device=dev)
    out, ws = guarded(n * 3 * S * S, dev), workspace(n, S, dev)
    applied = torch.full((n + 4,), SENTINEL, dtype=torch.int32, device=dev)
    r, f, pr, gt, pd, o, ap, w = (ptr(real), ptr(fake), ptr(params), ptr(gates), ptr(p_dev), ptr(out, GUARD),
                                  ptr(applied), ptr(ws))
    ok = [r, nr, f, nf, pr, gt, pd, o, ap, S, 7, w]
    bad = [(0, None), (0, r + 4), (2, None), (2, f + 8), (4, None), (5, None), (5, gt + 2), (6, None), (6, pd + 1),
           (7, None), (7, o + 4), (8, None), (8, ap + 2), (9, 6), (9, 9), (9, 4098), (10, 0), (10, 8), (10, -1),
           (11, None), (11, w + 4), (1, -1), (3, -1), (1, 65535)]
    for i, v in bad:
        a = list(ok)
        a[i] = v
        assert _lib.lib.sba_diffaug_gated_fwd(*a, stream()) == _lib.CONSTANTS['SBA_E_ARG'], (i, v)
    a = list(ok)
    a[1], a[3] = 0, 0
    assert _lib.lib.sba_diffaug_gated_fwd(*a, stream()) == _lib.CONSTANTS['SBA_E_ARG']
    okb = [f, nf, pr, ap, o, S, 7, w]
    for i, v in ((0, None), (0, f + 4), (1, 0), (1, -1), (2, None), (3, None), (3, ap + 1), (4, None), (4, o + 8),
                 (5, 6), (5, 9), (6, 0), (6, 8), (7, None)):
        a = list(okb)
        a[i] = v
        assert _lib.lib.sba_diffaug_gated_bwd(*a, stream()) == _lib.CONSTANTS['SBA_E_ARG'], (i, v)
    torch.cuda.synchronize()
    assert bool((out == FILL).all()) and bool((applied == SENTINEL).all())
    # what is allowed: no real images with a NULL pointer, no workspace with color off, p and gates 4-byte aligned
    assert _lib.lib.sba_diffaug_gated_fwd(None, 0, f, nf, pr, gt + 16, pd + 4, o, ap + 4, S, 6, None, stream()) == 0
    torch.cuda.synchronize()
    assert guards_intact(out) and applied[1:1 + nf].tolist() == [6] * nf and int(applied[0]) == SENTINEL


COUNT_VALUES = np.array([0, 0.25, 0.5, 0.75, 1, np.nan, np.nextafter(np.float32(0.5), np.float32(1)),
                         np.nextafter(np.float32(0.5), np.float32(0))], dtype=np.float32)


@pytest.mark.parametrize('n', [1, 63, 64, 65, 257, 1000])
def test_ada_count_adds_exact_integers_to_its_row_alone(n):
    from sbagan import _lib
    dev = torch.device('cuda', 0)
    rng = np.random.RandomState(n)
    start = np.array([[11, 12, 13, 14], [100, 200, 300, 400], [21, 22, 23, 24]], dtype=np.int32)
    counters = torch.from_numpy(start.copy()).to(dev)
    ref = A.Controller(3)
    ref.counters[1] = start[1].tolist()
    for call in range(3):
        prob_np = COUNT_VALUES[rng.randint(0, len(COUNT_VALUES), n)]
        if n >= 63:
            prob_np[:len(COUNT_VALUES)] = COUNT_VALUES                      # every value at least once
        prob = guarded(n, dev)
        body(prob).copy_(torch.from_numpy(prob_np))
        assert _lib.lib.sba_ada_count(ptr(prob, GUARD), n, ptr(counters, 4), stream()) == 0
        torch.cuda.synchronize()
        ref.count(1, prob_np)
        got = counters.cpu().numpy()
        assert got[1].tolist() == ref.counters[1], (call, got[1], ref.counters[1])
        assert np.array_equal(got[0], start[0]) and np.array_equal(got[2], start[2])
    assert ref.counters[1][2] == 300 + 3 * n and ref.counters[1][3] == 403
    if n >= 63:
        assert ref.counters[1][0] > 100 and ref.counters[1][1] > 200
        assert ref.counters[1][0] - 100 + ref.counters[1][1] - 200 < 3 * n          # 0.5 and NaN: in cnt only
    bad = _lib.CONSTANTS['SBA_E_ARG']
    assert _lib.lib.sba_ada_count(ptr(prob, GUARD), 0, ptr(counters, 4), stream()) == bad
    assert _lib.lib.sba_ada_count(None, n, ptr(counters, 4), stream()) == bad
    assert _lib.lib.sba_ada_count(ptr(prob, GUARD), n, None, stream()) == bad
    assert _lib.lib.sba_ada_count(ptr(prob, GUARD), (1 << 20) + 1, ptr(counters, 4), stream()) == bad
    torch.cuda.synchronize()
    assert counters.cpu().numpy()[1].tolist() == ref.counters[1]


def test_ada_adjust_follows_the_reference_through_a_scripted_sequence():
    """nD = 3, interval 4, target 0.5, 12 rounds.  Row 0 counts every round with r_t above the target: p rises at the
    boundaries 4 and 8 and is held by p_max at 8 and 12.  Row 1 counts every round: below the target at 4 and 8 (p
    reaches 0 and is held there), equal to it at 12 (p unchanged).  Row 2 counts every other round -- below the interval
    at rounds 4 and 12, full at round 7 -- and at round 10 gets calls = 4 with cnt = 0 written into it."""
    from sbagan import _lib
    dev = torch.device('cuda', 0)
    nD, interval, target, step, p_max = 3, 4, 0.5, 0.0625, 0.3
    above = np.array([0.9, 0.8, 0.7, 0.6, 0.9, 0.2, 0.5], dtype=np.float32)         # (5 - 1) / 7
    below = np.array([0.1, 0.2, 0.9, 0.5, np.nan], dtype=np.float32)                # (1 - 2) / 5
    equal = np.array([0.9, 0.9, 0.9, 0.1], dtype=np.float32)                        # (3 - 1) / 4 = 0.5 exactly
    ref = A.Controller(nD)
    ref.p[:] = np.array([0.2, 0.05, 0.15], dtype=np.float32)
    state = torch.zeros((2, nD), dtype=torch.float32, device=dev)
    p, rt = state[0], state[1]
    p.copy_(torch.from_numpy(ref.p))
    counters = torch.zeros((nD, 4), dtype=torch.int32, device=dev)
    probs = {k: torch.from_numpy(v).to(dev) for k, v in (('above', above), ('below', below), ('equal', equal))}
    seen = set()
    for rnd in range(1, 13):
        plan = [(0, 'above'), (1, 'equal' if rnd > 8 else 'below')] + ([(2, 'above')] if rnd % 2 else [])
        for row, name in plan:
            t = probs[name]
            assert _lib.lib.sba_ada_count(ptr(t), t.numel(), ptr(counters, 4 * row), stream()) == 0
            ref.count(row, {'above': above, 'below': below, 'equal': equal}[name])
        if rnd == 10:
            counters[2] = torch.tensor([0, 0, 0, 4], dtype=torch.int32, device=dev)
            ref.counters[2] = [0, 0, 0, 4]
        before = [list(c) for c in ref.counters]
        p_before = ref.p.copy()
        assert _lib.lib.sba_ada_adjust(ptr(p), ptr(rt), ptr(counters), nD, interval, target, step, p_max,
                                       stream()) == 0
        torch.cuda.synchronize()
        ref.adjust(interval, target, step, p_max)
        assert np.array_equal(p.cpu().numpy().view(np.int32), ref.p.view(np.int32)), (rnd, p.tolist(), ref.p)
        assert np.array_equal(rt.cpu().numpy().view(np.int32), ref.rt.view(np.int32)), (rnd, rt.tolist(), ref.rt)
        assert counters.cpu().numpy().tolist() == ref.counters, rnd
        for row in range(nD):       # which situation this row was in
            if before[row][3] < interval:
                assert ref.counters[row] == before[row] and ref.p[row] == p_before[row]
                seen.add('below the interval' if before[row][3] else 'idle')
                continue
            assert ref.counters[row] == [0, 0, 0, 0]
            if before[row][2] == 0:
                assert ref.p[row] == p_before[row] and ref.rt[row] == 0
                seen.add('cnt 0')
            elif ref.rt[row] > np.float32(target):
                seen.add('up' if ref.p[row] > p_before[row] else 'held at p_max')
            elif ref.rt[row] < np.float32(target):
                seen.add('down' if ref.p[row] < p_before[row] else 'held at 0')
            else:
                assert ref.p[row] == p_before[row]
                seen.add('equal')
    assert seen >= {'below the interval', 'cnt 0', 'up', 'held at p_max', 'down', 'held at 0', 'equal'}, seen
    assert ref.p.tolist() == [np.float32(0.3), 0.0, np.float32(np.float32(0.15) + np.float32(step))]
    bad = _lib.CONSTANTS['SBA_E_ARG']
    for args in ((None, ptr(rt), ptr(counters), nD, interval, target, step, p_max),
                 (ptr(p), ptr(rt), ptr(counters), 0, interval, target, step, p_max),
                 (ptr(p), ptr(rt), ptr(counters), 9, interval, target, step, p_max),
                 (ptr(p), ptr(rt), ptr(counters), nD, 0, target, step, p_max),
                 (ptr(p), ptr(rt), ptr(counters), nD, 1025, target, step, p_max),
                 (ptr(p), ptr(rt), ptr(counters), nD, interval, target, -1.0, p_max),
                 (ptr(p), ptr(rt), ptr(counters), nD, interval, target, float('inf'), p_max),
                 (ptr(p), ptr(rt), ptr(counters), nD, interval, target, step, 1.5)):
        assert _lib.lib.sba_ada_adjust(*args, stream()) == bad, args


def test_operator_matches_the_entry_points_and_skips_the_detached_backward():
    from sbagan import _lib, ops
    dev = torch.device('cuda', 0)
    S, nr, nf, flags = 10, 3, 3, 7
    n = nr + nf
    c = case(S, n)
    x, g, params = (torch.from_numpy(c[k]).to(dev) for k in ('x', 'g', 'params'))
    gates = torch.from_numpy(hand_gates(n)).to(dev)
    p_dev = torch.tensor([0.5], device=dev)
    want_t, app_t = gated_fwd(x, nr, params, gates, 0.5, S, flags, dev)
    leaf = x[nr:].clone().requires_grad_(True)
    out = ops.diffaug_gated(x[:nr], leaf, params, gates, p_dev, flags)
    assert torch.equal(i32(out), i32(body(want_t).view(n, 3, S, S)))
    assert torch.equal(ops.DiffAugGatedFn.last_applied, app_t[GUARD:-GUARD])
    p_dev.fill_(1.0)            # the controller moves p between forward and backward: the backward does not care
    (grad,) = torch.autograd.grad(out, leaf, g)
    dwant = gated_bwd(g[nr:].contiguous(), params[nr:].contiguous(), app_t[GUARD + nr:-GUARD].contiguous(), S, flags, dev)
    assert torch.equal(i32(grad), i32(body(dwant).view(nf, 3, S, S)))
    calls = []
    hook_before = _lib.AUDIT_HOOK
    _lib.AUDIT_HOOK = lambda name, args: calls.append(name)
    try:
        w = torch.ones((), device=dev, requires_grad=True)
        out = ops.diffaug_gated(x[:nr], x[nr:], params, gates, p_dev, flags)
        assert not out.requires_grad
        (out * w).sum().backward()
    finally:
        _lib.AUDIT_HOOK = hook_before
    assert calls == ['sba_diffaug_gated_fwd']
    for bad in ((params[:-1], gates, p_dev), (params, gates[:-1], p_dev), (params, gates, torch.zeros(2, device=dev))):
        with pytest.raises(ValueError):
            ops.diffaug_gated(x[:nr], x[nr:], *bad, flags)


# ---- the training step: the toy data set and settings of tests/test_replay_train_gpu.py ---------------------------------
POLICY = 'color,translation,cutout'


@pytest.fixture()
def det():
    from miscc.config import reset_cfg
    from sbagan import ops
    from test_replay_train_gpu import toy_cfg
    toy_cfg()
    dt = ops.compute_dtype()
    ops.set_deterministic(True)
    yield
    ops.set_deterministic(False)
    ops.set_compute_dtype(dt)
    reset_cfg()


@pytest.fixture(scope='module')
def toy(tmp_path_factory):
    import datasets
    from sbagan.device_data import DeviceImageCache
    from test_replay_train_gpu import CROP, make_dataset, toy_cfg
    toy_cfg()
    root = make_dataset(str(tmp_path_factory.mktemp('ada') / 'toy'))
    ds = datasets.TextDataset(root, 'train', base_size=64, transform=None)
    cache = DeviceImageCache(ds, int(CROP * 76 / 64), torch.device('cuda', 0), max_bytes=1 << 30, workers=0)
    return {'root': root, 'ds': ds, 'cache': cache, 'tmp': tmp_path_factory, 'runs': {}}


def run(toy, monkeypatch, policy=POLICY, p=None, ada=None, steps=1, eager=True, fixed_draws=False, kimg=500.0,
        interval=4, audit_from=None):
    """one --device_data --replay run of the trainer in f32 (cached per arguments).  fixed_draws: draw() copies the
    same uniforms and gates in every run instead of drawing (so that runs with and without gates see the same noise).
    Records per step: the losses, every gradient, the library calls (eager steps), the counters and last_prob."""
    key = (policy, p, ada, steps, bool(eager), fixed_draws, kimg, interval, audit_from)
    if key in toy['runs']:
        return toy['runs'][key]
    from sbagan import _lib, diffaug, ops
    from sbagan.device_data import DeviceBatchLoader
    from sbagan.stream_audit import StreamAudit
    from sbagan.trainer import GANStep
    from test_replay_train_gpu import B, CROP, SEED
    from trainer import condGANTrainer
    ops.set_compute_dtype(torch.float32)
    dev = torch.device('cuda', 0)
    if fixed_draws:
        gen = torch.Generator().manual_seed(11)
        fixed_u, fixed_g = torch.rand((2 * 3 * B, 8), generator=gen).to(dev), torch.rand((2 * 3 * B, 4), generator=gen).to(dev)

        def draw(self):
            self.uniforms.copy_(fixed_u)
            if self.gated:
                self.gates.copy_(fixed_g)
        monkeypatch.setattr(diffaug.DiffAugment, 'draw', draw)
    per_step, calls, audit = [], [], {}
    plain_step = GANStep.step

    def step(self, *a, **k):
        if torch.cuda.is_current_stream_capturing():
            return plain_step(self, *a, **k)
        if audit_from is not None and len(per_step) == audit_from:
            audit['a'] = StreamAudit(dev).start()
        calls.append([])
        hook = _lib.AUDIT_HOOK          # (the audit's own, when one is recording)

        def both(name, args):
            calls[-1].append(name)
            if hook is not None:
                hook(name, args)
        _lib.AUDIT_HOOK = both
        try:
            out = plain_step(self, *a, **k)
        finally:
            _lib.AUDIT_HOOK = hook
        torch.cuda.synchronize()
        rec = {'out': {n: v.detach().clone() for n, v in out.items()},
               'grads': [self.flatG.grad.clone()] + [f.grad.clone() for f in self.flatD]}
        aug = self.augment
        if aug is not None and aug.adaptive:
            rec['counters'] = aug.counters.cpu().clone()
            rec['last_prob'] = [[s.cpu().clone() for s in lp] for lp in aug.last_prob]
            rec['p'] = aug.p.cpu().clone()
        per_step.append(rec)
        return out
    monkeypatch.setattr(GANStep, 'step', step)
    ds = toy['ds']
    loader = DeviceBatchLoader(ds, toy['cache'], B, CROP, 2, seed=SEED)
    torch.manual_seed(3)
    out_dir = str(toy['tmp'].mktemp('out'))
    algo = condGANTrainer(out_dir, loader, ds.n_words, ds.ixtoword, allow_random_encoders=True)
    algo.replay, algo.replay_eager, algo.diffaug = True, eager, policy
    algo.diffaug_p, algo.ada, algo.ada_kimg, algo.ada_interval = p, ada, kimg, interval
    try:
        algo.train(max_steps=steps)
        torch.cuda.synchronize()
    finally:
        hazards = audit['a'].stop() if audit else None
    monkeypatch.setattr(GANStep, 'step', plain_step)
    gan, state = algo.gan, {}
    for name, flat, opt in [('G', gan.flatG, gan.optG)] + [('D%d' % i, f, o) for i, (f, o) in
                                                            enumerate(zip(gan.flatD, gan.optD))]:
        state[name + '/param'], state[name + '/m'], state[name + '/v'] = flat.data.cpu(), flat.m.cpu(), flat.v.cpu()
        state[name + '/adam_state'] = opt.state.cpu()
        if flat.avg is not None:
            state[name + '/ema'] = flat.avg.cpu()
    aug = gan.augment
    if aug is not None and aug.gated:
        state['ada/p'], state['ada/rt'], state['ada/counters'] = aug.p.cpu(), aug.rt.cpu(), aug.counters.cpu()
    res = {'state': state, 'steps': per_step, 'calls': calls, 'augment': aug, 'hazards': hazards, 'out_dir': out_dir,
           'audit_stats': audit['a'].stats if audit else None,
           'recorded': algo.slot_step.recording is not None,
           # what the four augmentation forwards of the last step (D update and G term of either discriminator) applied
           'applied': torch.cat([t.cpu() for t in list(ops.DiffAugGatedFn.applied_log)[-4:]])
           if aug is not None and aug.gated else None}
    toy['runs'][key] = res
    return res


def assert_same_step(a, b):
    """one step's losses and every parameter gradient, bit for bit"""
    assert sorted(a['out']) == sorted(b['out'])
    bad = [k for k in a['out'] if not torch.equal(i32(a['out'][k].reshape(1)), i32(b['out'][k].reshape(1)))]
    assert not bad, bad
    assert len(a['grads']) == len(b['grads']) == 3
    for k, (x, y) in enumerate(zip(a['grads'], b['grads'])):
        assert torch.equal(i32(x), i32(y)) and bool(x.abs().sum() > 0), k


def test_step_at_p_one_is_the_diffaug_step_and_at_p_zero_the_plain_step(toy, det, monkeypatch):
    full = run(toy, monkeypatch, fixed_draws=True)
    one = run(toy, monkeypatch, p=1.0, fixed_draws=True)
    zero = run(toy, monkeypatch, p=0.0, fixed_draws=True)
    plain = run(toy, monkeypatch, policy='', fixed_draws=True)
    assert one['augment'].gated and not one['augment'].adaptive and not full['augment'].gated
    assert plain['augment'] is None
    assert_same_step(one['steps'][0], full['steps'][0])
    assert_same_step(zero['steps'][0], plain['steps'][0])
    for k in ('G/param', 'D0/param', 'D1/param'):
        assert torch.equal(one['state'][k], full['state'][k]) and torch.equal(zero['state'][k], plain['state'][k])
        assert not torch.equal(full['state'][k], plain['state'][k]), k
    # the launches each flag adds (one eager step, nD = 2)
    new = ('sba_ada_', 'sba_diffaug_gated_')
    assert not [c for c in full['calls'][0] if c.startswith(new)] and 'sba_diffaug_fwd' in full['calls'][0]
    assert not [c for c in plain['calls'][0] if 'diffaug' in c or c.startswith('sba_ada_')]
    for r in (one, zero):
        names = r['calls'][0]
        assert not [c for c in names if c.startswith('sba_ada_') or c in ('sba_diffaug_fwd', 'sba_diffaug_bwd')]
        assert names.count('sba_diffaug_gated_fwd') == full['calls'][0].count('sba_diffaug_fwd') == 4
        assert names.count('sba_diffaug_gated_bwd') == full['calls'][0].count('sba_diffaug_bwd') == 2


def test_counters_are_the_counts_of_the_probabilities_and_the_step_audits_clean(toy, det, monkeypatch):
    """three eager steps with a long interval: after each, row i holds the signs of every last_prob[i] so far; exactly
    nD counts and one adjust per step; the stream audit of the last step reports nothing"""
    from test_replay_train_gpu import B
    r = run(toy, monkeypatch, ada=0.6, steps=3, interval=1000, audit_from=2)
    assert r['augment'].adaptive and len(r['steps']) == 3
    ref = A.Controller(2)
    for k, s in enumerate(r['steps']):
        for i in range(2):
            assert len(s['last_prob'][i]) == 1 and s['last_prob'][i][0].numel() == 2 * B       # real and cond_real rows
            ref.count(i, s['last_prob'][i][0].numpy())
        assert s['counters'].tolist() == ref.counters, k
        assert [c[2:] for c in ref.counters] == [[2 * B * (k + 1), k + 1]] * 2
        assert s['p'].tolist() == [0.0, 0.0]                                              # below the interval
        names = r['calls'][k]
        assert names.count('sba_ada_count') == 2 and names.count('sba_ada_adjust') == 1
        last = max(j for j, c in enumerate(names) if c.startswith('sba_diffaug_gated_') or c == 'sba_ada_count')
        assert names.index('sba_ada_adjust') > last                                       # the tail of the step
        at = [j for j, c in enumerate(names) if c == 'sba_ada_count']
        assert all(names[j - 1] == 'sba_bce_multi' for j in at)                           # right behind the loss
        assert 'sba_diffaug_gated_fwd' in names and 'sba_diffaug_fwd' not in names
    assert r['hazards'] == [], r['hazards'][:4]
    assert r['audit_stats']['launches'] > 100


def test_recorded_loop_with_the_controller_trains_what_the_eager_loop_trains(toy, det, monkeypatch):
    """--device_data --replay --diffaug color,translation,cutout --ada 0.6, five steps, an update behind every one and
    a step of p of 0.25 (--ada_interval 1 --ada_kimg 0.016 at B = 4): five boundaries.  The toy discriminators' r_t over
    8 probabilities swings around the target, so p goes up and comes down again within the run."""
    kw = dict(ada=0.6, steps=5, kimg=0.016, interval=1)
    a, b = run(toy, monkeypatch, eager=False, **kw), run(toy, monkeypatch, eager=True, **kw)
    assert a['recorded'] and not b['recorded']
    assert a['augment'].adjust_step == 4 * 1 / (0.016 * 1000.0) and abs(a['augment'].adjust_step - 0.25) < 1e-12
    assert {'ada/p', 'ada/rt', 'ada/counters', 'G/ema', 'D1/m'} <= set(a['state'])
    bad = [k for k in a['state'] if not torch.equal(a['state'][k], b['state'][k])]
    assert not bad, bad
    assert all(bool(torch.isfinite(t.float()).all()) for t in a['state'].values())
    print('p', a['state']['ada/p'].tolist(), 'rt', a['state']['ada/rt'].tolist(), 'applied', a['applied'].tolist())
    assert bool(a['state']['ada/p'].any())                          # the controller acted
    assert not bool(a['state']['ada/counters'].any())               # every step's counts were consumed behind it
    assert len(set(a['applied'].tolist())) >= 2 and torch.equal(a['applied'], b['applied'])
    ps = [s['p'].tolist() for s in b['steps']]
    assert len(ps) == 5 and ps[0] == [0.0, 0.0] and len({tuple(v) for v in ps}) >= 3 and ps[4] == a['state']['ada/p'].tolist()
    assert all(v in (0.0, 0.25, 0.5, 0.75, 1.0) for row in ps for v in row)


def test_entry_point_logs_checkpoints_and_resumes(toy, tmp_path, monkeypatch, capsys):
    import main
    from miscc.config import reset_cfg
    from sbagan import ops
    from test_replay_train_gpu import _checkpoints, _yml
    from trainer import condGANTrainer
    reset_cfg()
    ops.set_compute_dtype(torch.bfloat16)
    (tmp_path / 'cwd').mkdir()
    monkeypatch.chdir(tmp_path / 'cwd')
    monkeypatch.setattr(condGANTrainer, 'log_interval', 2)
    trainers = []

    def make(output_dir, dataloader, n_words, ixtoword):
        trainers.append(condGANTrainer(output_dir, dataloader, n_words, ixtoword, allow_random_encoders=True))
        return trainers[-1]

    flags = ['--gpu', '0', '--manualSeed', '5', '--device_data', '--device_data_gb', '1', '--replay', '--diffaug', POLICY,
             '--ada', '0.6', '--ada_kimg', '0.032', '--ada_interval', '1', '--diffaug_p', '0.5']
    capsys.readouterr()
    main.main(['--cfg', _yml(tmp_path, toy['root'])] + flags, make_trainer=make)          # one epoch: 2 steps
    text = capsys.readouterr().out
    algo = trainers[0]
    aug = algo.gan.augment
    assert (algo.ada, algo.diffaug_p, algo.ada_kimg, algo.ada_interval) == (0.6, 0.5, 0.032, 1)
    assert aug.adaptive and aug.p0 == 0.5 and algo.slot_step.recording is not None
    lines = [ln for ln in text.split('\n') if ln.startswith('ada p: ')]
    assert len(lines) == 1 and ' r_t: ' in lines[0], text[-2000:]
    p, rt = aug.report()
    assert lines[0] == 'ada p: ' + ' '.join('%.3f' % v for v in p) + ' r_t: ' + ' '.join('%.2f' % v for v in rt)
    assert all(v in (0.25, 0.5, 0.75) for v in p)               # two updates, each 0.125 up, down or (r_t = target) none
    assert aug.counters[:, 3].tolist() == [0, 0] and aug.counters[:, 2].tolist() == [0, 0]      # both consumed
    files = _checkpoints(tmp_path)
    assert 'ada_state.pth' in files and files['ada_state.pth']['p'].tolist() == p
    model_dir = os.path.join(algo.model_dir)
    with open(os.path.join(model_dir, 'ada.jsonl')) as f:
        rows = [json.loads(ln) for ln in f]
    assert rows == [{'iteration': 2, 'p': p, 'r_t': rt}]
    # resume: the state beside the loaded checkpoint is restored; without one, one line says so
    starts = []
    plain = condGANTrainer._restore_ada

    def restore(self, augment):
        plain(self, augment)
        starts.append(augment.p.tolist())
    monkeypatch.setattr(condGANTrainer, '_restore_ada', restore)
    net_g = os.path.join(model_dir, 'netG_epoch_1.pth')
    main.main(['--cfg', _yml(tmp_path, toy['root'], NET_G=net_g, MAX_EPOCH=2)] + flags, make_trainer=make)
    text = capsys.readouterr().out
    assert starts == [p] and 'Load ada state from: ' in text
    os.remove(os.path.join(model_dir, 'ada_state.pth'))
    main.main(['--cfg', _yml(tmp_path, toy['root'], NET_G=net_g, MAX_EPOCH=2)] + flags, make_trainer=make)
    text = capsys.readouterr().out
    assert starts[1] == [0.5, 0.5] and text.count('p restarts from its initial value 0.5') == 1
    # outside training the flags are ignored, in one line
    made = []

    class Stub(object):
        def __init__(self, *a):
            made.append(self)

        def sampling(self, split_dir):
            pass

    monkeypatch.setattr(main, 'gen_example', lambda wordtoix, algo: None)
    main.main(['--cfg', _yml(tmp_path, toy['root'], FLAG=False), '--gpu', '0', '--diffaug', 'cutout', '--ada', '0.6'],
              make_trainer=Stub)
    assert capsys.readouterr().out.count('--ada / --diffaug_p are ignored outside training') == 1
    assert not hasattr(made[0], 'ada') or made[0].ada is None
    reset_cfg()
