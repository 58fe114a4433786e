"""--diffaug on the device: sba_diffaug_fwd / sba_diffaug_bwd through the C ABI on guarded buffers against the float64
reference of tests/diffaug_ref.py -- bit for bit where nothing is computed (color off; every cut or out-of-view element),
element by element within the reference's counted bound elsewhere --, twice for identical bits, the refusals, the
wiring into the two loss functions with no tolerance, and the training loop: the recorded loop against the eager one.

Measured on an MI355X, the largest |error| / bound over every case below (each bound test prints its own): 0.15 forward,
0.20 backward; the bound's constants are counted in diffaug_ref, not taken from these."""
import numpy as np
import pytest
import torch

import diffaug_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64                      # floats in front of and behind every output: 256 bytes, the body stays 16-byte aligned
FILL = 7.25
SIZES = [8, 10, 20, 64]         # 10: cut = 5 is odd and rows are no multiple of 4 pixels; 64: more than one block per image
SPLITS = [(0, 3), (3, 3), (1, 2)]
ALL_FLAGS = [1, 2, 3, 4, 5, 6, 7]
_CASES = {}


def gpu_params(n, seed):
    """n >= 3 rows; the corners in the first three: ty, tx = -shift / +shift / mixed; oy, ox = 0 / maximum / mixed (the
    cut rectangle partly outside); u0..u2 = 0 / the largest float32 below 1 / drawn"""
    p = np.random.RandomState(seed).random_sample((n, 8)).astype(np.float32)
    lo, hi = np.float32(0), R.BELOW_ONE
    p[0, :7] = lo
    p[1, :7] = hi
    p[2, 3:7] = lo, hi, hi, lo
    return p


def case(S, nr, nf):
    """inputs of one shape, made once and never changed: images, output gradient, parameter rows"""
    key = (S, nr, nf)
    if key not in _CASES:
        n = nr + nf
        rng = np.random.RandomState(1000 * S + 10 * nr + nf)
        x = rng.standard_normal((n, 3, S, S)).astype(np.float32)
        x[0, 0, 0, 0], x[n - 1, 2, S - 1, S - 1] = -0.0, -0.0        # a signed zero must come through as it is
        _CASES[key] = {'x': x, 'g': rng.standard_normal((n, 3, S, S)).astype(np.float32),
                       'params': gpu_params(n, 77 * S + n), 'ref': {}}
    return _CASES[key]


def reference(c, flags):
    if flags not in c['ref']:
        c['ref'][flags] = (R.forward(c['x'], c['params'], flags), R.backward(c['g'], c['params'], flags))
    return c['ref'][flags]


def guarded(numel, dev):
    return torch.full((numel + 2 * GUARD,), FILL, dtype=torch.float32, device=dev)


def body(t):
    return t[GUARD:-GUARD]


def guards_intact(t):
    return bool((t[:GUARD] == FILL).all()) and bool((t[-GUARD:] == FILL).all())


def ptr(t, off=0):
    return None if t is None else t.data_ptr() + 4 * off


def workspace(n, S, dev):
    from sbagan import _lib
    return torch.empty(_lib.lib.sba_diffaug_workspace_bytes(n, S) // 8, dtype=torch.float64, device=dev)


def run_fwd(x, nr, params, S, flags, dev):
    """the forward entry point over [real = x[:nr] | fake = x[nr:]] on a guarded output; returns the guarded tensor"""
    from sbagan import _lib
    n = x.shape[0]
    real = torch.from_numpy(x[:nr]).to(dev) if nr else None
    fake = torch.from_numpy(x[nr:]).to(dev)
    out = guarded(n * 3 * S * S, dev)
    ws = workspace(n, S, dev)
    rows = torch.from_numpy(params).to(dev)
    rc = _lib.lib.sba_diffaug_fwd(ptr(real), nr, ptr(fake), n - nr, ptr(rows), ptr(out, GUARD), S, flags, ptr(ws),
                                  torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return out


def run_bwd(g, params, S, flags, dev):
    from sbagan import _lib
    n = g.shape[0]
    dx = guarded(n * 3 * S * S, dev)
    ws = workspace(n, S, dev)
    dout, rows = torch.from_numpy(g).to(dev), torch.from_numpy(params).to(dev)      # (both alive across the call)
    rc = _lib.lib.sba_diffaug_bwd(ptr(dout), n, ptr(rows), ptr(dx, GUARD), S, flags, ptr(ws),
                                  torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return dx


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def index_forward(x, params, flags):
    """color off: every output element is the input element it reads, or +0.0"""
    out = np.zeros_like(x)
    for a in range(x.shape[0]):
        live, si, sj = R.gather_plan(params[a], x.shape[2], flags)
        out[a] = np.where(live, x[a][:, si, sj], np.float32(0))
    return out


def index_backward(g, params, flags):
    return np.stack([R.scatter_G(g[a], params[a], g.shape[2], flags) for a in range(g.shape[0])])


@pytest.mark.parametrize('flags', ALL_FLAGS)
@pytest.mark.parametrize('nr,nf', SPLITS)
@pytest.mark.parametrize('S', SIZES)
def test_forward_and_backward_against_the_reference(S, nr, nf, flags):
    dev = torch.device('cuda', 0)
    c = case(S, nr, nf)
    x, g, params = c['x'], c['g'], c['params']
    n = nr + nf
    if flags == 7:      # the rows do sit on the corners
        maps = [R.int_maps(p, S, 7) for p in params[:3]]
        sh, top = R.shift_of(S), S - R.cut_of(S) % 2
        assert maps[0] == (-sh, -sh, 0, 0) and maps[1] == (sh, sh, top, top) and maps[2] == (-sh, sh, top, 0)
    out_t, dx_t = run_fwd(x, nr, params, S, flags, dev), run_bwd(g, params, S, flags, dev)
    out = body(out_t).cpu().numpy().reshape(n, 3, S, S)
    dx = body(dx_t).cpu().numpy().reshape(n, 3, S, S)
    assert guards_intact(out_t) and guards_intact(dx_t)
    # two calls, identical bits
    assert torch.equal(out_t.view(torch.int32), run_fwd(x, nr, params, S, flags, dev).view(torch.int32))
    assert torch.equal(dx_t.view(torch.int32), run_bwd(g, params, S, flags, dev).view(torch.int32))
    if not flags & 1:
        want, dwant = index_forward(x, params, flags), index_backward(g, params, flags)
        assert torch.equal(torch.from_numpy(out), torch.from_numpy(want))
        assert torch.equal(torch.from_numpy(dx), torch.from_numpy(dwant))
        assert np.array_equal(bits(out), bits(want)) and np.array_equal(bits(dx), bits(dwant))     # signed zeros too
        return
    (ref, A, live), (dref, Ab) = reference(c, flags)
    dead = ~np.broadcast_to(live[:, None], out.shape)
    assert not bits(out)[dead].any()                    # every cut or out-of-view output is exactly +0.0
    if flags != 1:
        assert dead.any() and not dead.all()
    err, bound = np.abs(out.astype(np.float64) - ref), R.bound_forward(A)
    derr, dbound = np.abs(dx.astype(np.float64) - dref), R.bound_backward(Ab)
    assert (bound[~dead] > 0).all() and (dbound > 0).all()
    print('S %d (%d, %d) flags %d: forward max err / bound %.3f, backward %.3f'
          % (S, nr, nf, flags, (err[~dead] / bound[~dead]).max(), (derr / dbound).max()))
    assert np.isfinite(out).all() and np.isfinite(dx).all()
    assert (err <= bound).all(), (err - bound).max()            # every element; the dead ones at bound 0
    assert (derr <= dbound).all(), (derr - dbound).max()


def test_bad_arguments_are_refused_and_write_nothing():
    from sbagan import _lib
    dev = torch.device('cuda', 0)
    S, nr, nf = 8, 2, 2
    n = nr + nf
    real = torch.zeros((nr, 3, S, S), device=dev)
    fake = torch.zeros((nf, 3, S, S), device=dev)
    params = torch.from_numpy(gpu_params(n, 1)).to(dev)
    out, ws = guarded(n * 3 * S * S, dev), workspace(n, S, dev)
    st = torch.cuda.current_stream().cuda_stream
    r, f, p, o, w = ptr(real), ptr(fake), ptr(params), ptr(out, GUARD), ptr(ws)
    fwd = [(r, nr, f, nf, p, o, 6, 7, w), (r, nr, f, nf, p, o, 4, 7, w),          # S < 8
           (r, nr, f, nf, p, o, 9, 7, w),                                         # S odd
           (r, nr, f, nf, p, o, S, 0, w), (r, nr, f, nf, p, o, S, 8, w), (r, nr, f, nf, p, o, S, -1, w),
           (r, 0, f, 0, p, o, S, 7, w), (None, 0, f, 0, p, o, S, 7, w),           # nr + nf = 0
           (r, -1, f, nf, p, o, S, 7, w), (r, nr, f, -1, p, o, S, 7, w), (r, -2, f, 2, p, o, S, 7, w),
           (None, nr, f, nf, p, o, S, 7, w), (r, nr, None, nf, p, o, S, 7, w), (r, nr, f, nf, None, o, S, 7, w),
           (r, nr, f, nf, p, None, S, 7, w), (r, nr, f, nf, p, o, S, 7, None), (r, nr, f, nf, p, o, S, 1, None)]
    for a in fwd:
        assert _lib.lib.sba_diffaug_fwd(*a, st) != 0, a
    bwd = [(f, nf, p, o, 6, 7, w), (f, nf, p, o, 9, 7, w), (f, nf, p, o, S, 0, w), (f, nf, p, o, S, 8, w),
           (f, 0, p, o, S, 7, w), (f, -1, p, o, S, 7, w), (None, nf, p, o, S, 7, w), (f, nf, None, o, S, 7, w),
           (f, nf, p, None, S, 7, w), (f, nf, p, o, S, 7, None)]
    for a in bwd:
        assert _lib.lib.sba_diffaug_bwd(*a, st) != 0, a
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    # what is allowed: no real images with a NULL pointer, and no workspace with color off
    assert _lib.lib.sba_diffaug_fwd(None, 0, f, nf, p, o, S, 6, None, st) == 0
    torch.cuda.synchronize()
    assert guards_intact(out) and not bool((body(out)[:nf * 3 * S * S] == FILL).any())


def test_operator_matches_the_entry_points_and_skips_the_detached_backward():
    """ops.diffaug: the same bits as the C ABI; a gradient for `fake` only; no launch when `fake` needs none"""
    from sbagan import _lib, ops
    dev = torch.device('cuda', 0)
    S, nr, nf, flags = 20, 3, 3, 7
    c = case(S, nr, nf)
    real, fake = torch.from_numpy(c['x'][:nr]).to(dev), torch.from_numpy(c['x'][nr:]).to(dev)
    params, g = torch.from_numpy(c['params']).to(dev), torch.from_numpy(c['g']).to(dev)
    want = body(run_fwd(c['x'], nr, c['params'], S, flags, dev)).view(nr + nf, 3, S, S)
    leaf = fake.clone().requires_grad_(True)
    out = ops.diffaug(real, leaf, params, flags)
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    (grad,) = torch.autograd.grad(out, leaf, g)
    dwant = body(run_bwd(c['g'][nr:], c['params'][nr:], S, flags, dev)).view(nf, 3, S, S)
    assert torch.equal(grad.view(torch.int32), dwant.view(torch.int32))
    calls = []
    hook_before = _lib.AUDIT_HOOK
    _lib.AUDIT_HOOK = lambda name, args: calls.append(name)
    try:
        w = torch.ones((), device=dev, requires_grad=True)
        out = ops.diffaug(real, fake, params, flags)             # detached fake images: the discriminator update
        assert not out.requires_grad
        (out * w).sum().backward()
    finally:
        _lib.AUDIT_HOOK = hook_before
    assert calls == ['sba_diffaug_fwd']
    with pytest.raises(ValueError):
        ops.diffaug(real, fake, params[:-1], flags)


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


def _grads(net):
    return [None if p.grad is None else p.grad.detach().clone() for p in net.parameters()]


def test_losses_route_the_images_through_the_kernel(det, monkeypatch):
    """D_NET64 at the toy widths, B = 4, deterministic mode, no tolerance: the augmented discriminator loss is the plain
    one on the kernel's own output, and the generator term's image gradient is sba_diffaug_bwd of the plain one's"""
    import model
    from miscc import losses
    from sbagan import ops
    from sbagan.diffaug import DiffAugment
    dev = torch.device('cuda', 0)
    ops.set_compute_dtype(torch.float32)
    monkeypatch.setattr(ops, 'SIDE_WGRAD', False)
    B, S = 4, 64
    torch.manual_seed(5)
    net = model.D_NET64().to(dev).train()
    real, fake = torch.randn((B, 3, S, S), device=dev), torch.randn((B, 3, S, S), device=dev).tanh()
    sent = torch.randn((B, 256), device=dev)
    ones, zeros = torch.ones(B, device=dev), torch.zeros(B, device=dev)
    aug = DiffAugment('color,translation,cutout', B, 1, dev)
    aug.draw()
    rows, flags = aug.d_arg(0)
    assert flags == 7 and tuple(rows.shape) == (2 * B, 8)

    out = ops.diffaug(real, fake, rows, flags)
    assert not torch.equal(out, torch.cat((real, fake), 0))
    results = []
    for kw, r, f in (({'augment': aug.d_arg(0)}, real, fake), ({}, out[:B], out[B:])):
        net.zero_grad(set_to_none=True)
        ops.det_reset()
        err = losses.discriminator_loss(net, r, f.clone().requires_grad_(True), sent, ones, zeros, **kw)
        err.backward()
        ops.join_wgrads()
        results.append((err.detach().clone(), _grads(net)))
    (e0, g0), (e1, g1) = results
    assert torch.equal(e0.view(torch.int32), e1.view(torch.int32)) and bool(torch.isfinite(e0))
    assert any(g is not None and bool(g.abs().sum() > 0) for g in g0)
    for a, b in zip(g0, g1):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))

    for p in net.parameters():
        p.requires_grad_(False)
    g_rows, _ = aug.g_arg(0)
    assert g_rows.data_ptr() != rows.data_ptr()
    seen = ops.diffaug(None, fake, g_rows, flags)
    ops.det_reset()
    value, grad = losses.generator_d_term(net, fake, sent, augment=aug.g_arg(0))
    ops.det_reset()
    value_plain, grad_plain = losses.generator_d_term(net, seen, sent)
    assert torch.equal(value.view(torch.int32), value_plain.view(torch.int32))
    want = body(run_bwd(grad_plain.cpu().numpy(), g_rows.cpu().numpy(), S, flags, dev)).view(B, 3, S, S)
    assert torch.equal(grad.view(torch.int32), want.view(torch.int32)) and bool(grad.abs().sum() > 0)
    # and through generator_loss's own inline terms: the same value
    ops.det_reset()
    leaf = fake.clone().requires_grad_(True)
    inline = losses._g_term(net, net(ops.diffaug(None, leaf, g_rows, flags)), sent)
    assert torch.equal(inline.detach().view(torch.int32), value.view(torch.int32))


def test_step_refuses_the_two_pass_layouts():
    from sbagan.diffaug import DiffAugment
    from sbagan.trainer import GANStep
    aug = DiffAugment('cutout', 2, 1, torch.device('cuda', 0))

    class Augmented(GANStep):
        augment = aug

    class Overlapped(Augmented):
        force_overlap_layout = True

    with pytest.raises(ValueError, match='distributed'):
        Augmented(None, None, None, 2, distributed=True)
    with pytest.raises(ValueError, match='force_overlap_layout'):
        Overlapped(None, None, None, 2)


# ---- the training loop: the toy data set and settings of tests/test_replay_train_gpu.py, built the same way ----------
STEPS = 5


@pytest.fixture(scope='module')
def toy(tmp_path_factory):
    import datasets
    from sbagan.device_data import DeviceImageCache
    from test_replay_train_gpu import CROP, make_dataset, toy_cfg
    toy_cfg()
    root = make_dataset(str(tmp_path_factory.mktemp('diffaug') / 'toy'))
    ds = datasets.TextDataset(root, 'train', base_size=64, transform=None)
    cache = DeviceImageCache(ds, int(CROP * 76 / 64), torch.device('cuda', 0), max_bytes=1 << 30, workers=0)
    return {'root': root, 'ds': ds, 'cache': cache, 'tmp': tmp_path_factory, 'runs': {}}


def trained(toy, policy, eager, monkeypatch):
    """one --device_data --replay [--diffaug policy] run of the trainer in f32 (cached): the final training state and
    the uniforms after every draw"""
    key = (policy, bool(eager))
    if key in toy['runs']:
        return toy['runs'][key]
    from sbagan import diffaug, ops
    from sbagan.device_data import DeviceBatchLoader
    from test_replay_train_gpu import B, CROP, SEED
    from trainer import condGANTrainer
    ops.set_compute_dtype(torch.float32)
    draws = []
    plain_draw = diffaug.DiffAugment.draw

    def recording_draw(self):
        plain_draw(self)
        draws.append(self.uniforms.clone())
    monkeypatch.setattr(diffaug.DiffAugment, 'draw', recording_draw)
    ds = toy['ds']
    loader = DeviceBatchLoader(ds, toy['cache'], B, CROP, 2, seed=SEED)
    torch.manual_seed(3)
    algo = condGANTrainer(str(toy['tmp'].mktemp('out')), loader, ds.n_words, ds.ixtoword, allow_random_encoders=True)
    algo.replay, algo.replay_eager, algo.diffaug = True, eager, policy
    algo.train(max_steps=STEPS)
    torch.cuda.synchronize()
    gan, state = algo.gan, {}
    for name, flat, opt in [('G', gan.flatG, gan.optG)] + [('D%d' % i, f, o) for i, (f, o) in
                                                            enumerate(zip(gan.flatD, gan.optD))]:
        state[name + '/param'], state[name + '/m'], state[name + '/v'] = flat.data.cpu(), flat.m.cpu(), flat.v.cpu()
        state[name + '/adam_state'] = opt.state.cpu()
        if flat.avg is not None:
            state[name + '/ema'] = flat.avg.cpu()
    res = {'state': state, 'draws': [d.cpu() for d in draws], 'recorded': algo.slot_step.recording is not None,
           'augment': gan.augment, 'nodes': None if algo.slot_step.recording is None else
           algo.slot_step.recording.info['nodes']}
    toy['runs'][key] = res
    return res


def test_recorded_loop_with_augmentation_trains_what_the_eager_loop_trains(toy, det, monkeypatch):
    policy = 'color,translation,cutout'
    a, b = trained(toy, policy, False, monkeypatch), trained(toy, policy, True, monkeypatch)
    assert a['recorded'] and not b['recorded']
    assert a['augment'] is not None and a['augment'].flags == 7
    assert 'G/ema' in a['state'] and 'D1/m' in a['state']
    bad = [k for k in a['state'] if not torch.equal(a['state'][k], b['state'][k])]
    assert not bad, bad
    assert all(bool(torch.isfinite(t.float()).all()) for t in a['state'].values())
    # one draw per step, by whoever draws the noise; the recorded launches saw fresh uniforms every time
    for r in (a, b):
        assert len(r['draws']) == STEPS
        assert all(not torch.equal(r['draws'][i], r['draws'][i + 1]) for i in range(STEPS - 1))
        assert all(bool((d >= 0).all()) and bool((d < 1).all()) for d in r['draws'])
    assert all(torch.equal(x, y) for x, y in zip(a['draws'], b['draws']))


def test_augmentation_changes_the_training(toy, det, monkeypatch):
    a, plain = trained(toy, 'color,translation,cutout', False, monkeypatch), trained(toy, '', False, monkeypatch)
    assert plain['recorded'] and plain['augment'] is None and plain['draws'] == []
    for k in ('G/param', 'D0/param', 'D1/param'):
        assert not torch.equal(a['state'][k], plain['state'][k]), k
    assert a['nodes'] > plain['nodes']          # the augmentation launches are in the recording


def test_entry_point_hands_the_flag_over_and_trains(toy, tmp_path, monkeypatch, capsys):
    """main.main --device_data --replay --diffaug ...: one epoch of the toy directory (2 steps) through the recording"""
    import main
    from miscc.config import reset_cfg
    from sbagan import ops
    from test_replay_train_gpu import _checkpoints, _yml
    from trainer import condGANTrainer
    reset_cfg()
    ops.set_compute_dtype(torch.bfloat16)
    yml = _yml(tmp_path, toy['root'])
    (tmp_path / 'cwd').mkdir()
    monkeypatch.chdir(tmp_path / 'cwd')
    trainers = []

    def make(output_dir, dataloader, n_words, ixtoword):
        trainers.append(condGANTrainer(output_dir, dataloader, n_words, ixtoword, allow_random_encoders=True))
        return trainers[-1]

    main.main(['--cfg', yml, '--gpu', '0', '--manualSeed', '5', '--device_data', '--device_data_gb', '1', '--replay',
               '--diffaug', 'color,translation,cutout'], make_trainer=make)
    algo = trainers[0]
    assert algo.diffaug == 'color,translation,cutout' and algo.replay is True
    assert algo.gan.augment is not None and algo.gan.augment.flags == 7 and algo.slot_step.recording is not None
    assert tuple(algo.gan.augment.uniforms.shape) == (2 * 3 * 4, 8) and bool(algo.gan.augment.uniforms.any())
    _checkpoints(tmp_path)
    # outside training the flag is ignored, in one line
    made = []

    class Stub(object):
        def __init__(self, *a):
            made.append(self)

        def sampling(self, split_dir):
            pass

    capsys.readouterr()
    yml_eval = _yml(tmp_path, toy['root'], FLAG=False)
    monkeypatch.setattr(main, 'gen_example', lambda wordtoix, algo: None)
    main.main(['--cfg', yml_eval, '--gpu', '0', '--diffaug', 'cutout'], make_trainer=Stub)
    assert made[0].diffaug == '' and capsys.readouterr().out.count('--diffaug is ignored outside training') == 1
    reset_cfg()
