"""--geoaug on the device: sba_geoaug_prepare / _fwd / _bwd through the C ABI on guarded buffers against the float64
reference of tests/geoaug_ref.py and its bounds (derived there on the CPU, not from these kernels), the permutations bit
for bit, adjointness, identical bits from two calls, the operator and its wiring into the losses with no tolerance, and
the training step: the recorded loop against the eager one, and the launches the flag adds.

Every bound test prints its largest |error| / bound."""
import numpy as np
import pytest
import torch

import geoaug_ref as R
from test_diffaug_gpu import GUARD, bits, body, guarded, guards_intact, ptr

pytestmark = pytest.mark.gpu

SENTINEL = -77
SPLITS = {1: [(0, 1), (1, 0)], 3: [(0, 3), (3, 0), (1, 2)], 5: [(0, 5), (5, 0), (2, 3)]}
_CASES = {}


def stream():
    return torch.cuda.current_stream().cuda_stream


def prepare(u, flags, dev, gates=None, p=None, rows_per_p=1):
    """sba_geoaug_prepare on guarded outputs: (mats f32 [N][4], applied int32 [N]) as numpy"""
    from sbagan import _lib
    N = len(u)
    ut = torch.from_numpy(np.ascontiguousarray(u, dtype=np.float32)).to(dev)
    gt = None if gates is None else torch.from_numpy(np.ascontiguousarray(gates, dtype=np.float32)).to(dev)
    pt = None if p is None else torch.tensor(p, dtype=torch.float32, device=dev)
    mats = guarded(N * 4, dev)
    applied = torch.full((N + 32,), SENTINEL, dtype=torch.int32, device=dev)
    rc = _lib.lib.sba_geoaug_prepare(ptr(ut), ptr(gt), ptr(pt), rows_per_p, N, flags, ptr(mats, GUARD), ptr(applied, 16),
                                     stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(mats) and applied[:16].tolist() == [SENTINEL] * 16 == applied[-16:].tolist()
    return body(mats).view(N, 4).cpu().numpy(), applied[16:-16].cpu().numpy()


def run_fwd(x, nr, mats, dev):
    """sba_geoaug_fwd over [real = x[:nr] | fake = x[nr:]] on a guarded output; returns the guarded tensor"""
    from sbagan import _lib
    n, _, S, _ = x.shape
    real = torch.from_numpy(x[:nr]).to(dev) if nr else None
    fake = torch.from_numpy(x[nr:]).to(dev) if n - nr else None
    out = guarded(n * 3 * S * S, dev)
    mt = torch.from_numpy(np.ascontiguousarray(mats, dtype=np.float32)).to(dev)
    rc = _lib.lib.sba_geoaug_fwd(ptr(real), nr, ptr(fake), n - nr, ptr(mt), ptr(out, GUARD), S, stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(out)
    return out


def run_bwd(g, mats, dev):
    from sbagan import _lib
    n, _, S, _ = g.shape
    dx = guarded(n * 3 * S * S, dev)
    dout = torch.from_numpy(g).to(dev)
    mt = torch.from_numpy(np.ascontiguousarray(mats, dtype=np.float32)).to(dev)
    rc = _lib.lib.sba_geoaug_bwd(ptr(dout), n, ptr(mt), ptr(dx, GUARD), S, stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(dx)
    return dx


def host(t, shape):
    return body(t).view(shape).cpu().numpy()


def case(S, n):
    """inputs and the f64 reference of one shape, made once and never changed.  Matrices: the hand-made ones of
    geoaug_ref.case_mats, and (kind 'drawn') what the device's own prepare launch writes for random rows"""
    key = (S, n)
    if key not in _CASES:
        dev = torch.device('cuda', 0)
        x, g = R.case_images(n, S, 1), R.case_images(n, S, 2)
        u = np.random.RandomState(100 * S + n).random_sample((n, 8)).astype(np.float32)
        c = {'x': x, 'g': g}
        for kind, mats in (('hand', R.case_mats(n)), ('drawn', prepare(u, 15, dev)[0])):
            c[kind] = {'mats': mats, 'out': R.forward(x, mats), 'dx': R.backward(g, mats),
                       'fb': R.forward_bound(x, mats), 'bb': R.backward_bound(g, mats)}
        _CASES[key] = c
    return _CASES[key]


# ---- prepare ---------------------------------------------------------------------------------------------------------
def rows(n, seed):
    return np.concatenate([R.edge_rows(), np.random.RandomState(seed).random_sample((n, 8)).astype(np.float32)])


@pytest.mark.parametrize('flags', range(1, 16))
def test_prepare_every_subset_ungated(flags):
    dev = torch.device('cuda', 0)
    u = rows(300, flags)                    # more than one block of rows
    want, on = R.matrices(u, flags)
    mats, applied = prepare(u, flags, dev)
    assert applied.tolist() == on.tolist() == [flags] * len(u)
    err = float(np.abs(mats - want).max())
    print('flags %d: matrix error %.3g of %.3g' % (flags, err, R.MATRIX_BOUND))
    assert err <= R.MATRIX_BOUND
    if not flags & (R.SCALE | R.ROTATE):    # flip / rot90 alone: exactly 0 and +-1
        assert np.array_equal(mats, want.astype(np.float32))
    # the edge rows: k = 3, s = 1, u0 = 0.5 flips
    flipped, k, s, _ = R.draws(u)
    assert k[0] == 3 and s[1] == 1.0 and bool(flipped[2])
    if flags == R.ROT90:
        assert mats[0].tolist() == [0.0, 1.0, -1.0, 0.0]                # Q^3
    if flags == R.SCALE:
        assert mats[1].tolist() == [1.0, 0.0, 0.0, 1.0]
    if flags == R.FLIP:
        assert mats[2].tolist() == [-1.0, 0.0, 0.0, 1.0] and mats[7].tolist() == [1.0, 0.0, 0.0, 1.0]


@pytest.mark.parametrize('p', [0.0, 0.5, 1.0, float('nan')])
def test_prepare_gated(p):
    dev = torch.device('cuda', 0)
    u = rows(40, 3)
    gates = np.random.RandomState(4).random_sample((len(u), 4)).astype(np.float32)
    gates[0], gates[1] = 0.5, np.nextafter(np.float32(0.5), np.float32(0))        # strictly below p only
    for flags in (15, 10):
        want, on = R.matrices(u, flags, gates, [p], len(u))
        mats, applied = prepare(u, flags, dev, gates, [p], len(u))
        assert applied.tolist() == on.tolist()
        assert float(np.abs(mats - want).max()) <= R.MATRIX_BOUND
        if p == 0.5 and flags == 15:
            assert applied[0] == 0 and applied[1] == 15 and len(set(applied.tolist())) > 4
        if p != 0.5:
            assert set(applied.tolist()) == ({flags} if p == 1.0 else {0})
        off = applied == 0
        assert np.array_equal(mats[off], np.tile(np.float32([1, 0, 0, 1]), (int(off.sum()), 1)))


def test_prepare_reads_the_p_of_each_group_of_rows():
    dev = torch.device('cuda', 0)
    u = rows(4, 6)                          # 12 rows, 5 per p: groups of 5, 5 and 2
    gates = np.full((len(u), 4), 0.5, dtype=np.float32)
    p = [1.0, 0.25, 0.75]
    want, on = R.matrices(u, 15, gates, p, 5)
    mats, applied = prepare(u, 15, dev, gates, p, 5)
    assert applied.tolist() == on.tolist() == [15] * 5 + [0] * 5 + [15] * 2
    assert float(np.abs(mats - want).max()) <= R.MATRIX_BOUND


# ---- the warp --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['hand', 'drawn'])
@pytest.mark.parametrize('S,n', R.SHAPES)
def test_forward_and_backward_against_the_reference(S, n, kind):
    dev = torch.device('cuda', 0)
    c = case(S, n)
    k = c[kind]
    outs = []
    for nr, nf in SPLITS[n]:
        assert nr + nf == n
        outs.append(host(run_fwd(c['x'], nr, k['mats'], dev), (n, 3, S, S)))
        assert np.array_equal(bits(outs[-1]), bits(outs[0])), (nr, nf)             # the split moves no bit
    out = outs[0]
    dx = host(run_bwd(c['g'], k['mats'], dev), (n, 3, S, S))
    rf, rb = R.ratio(out, k['out'], k['fb']), R.ratio(dx, k['dx'], k['bb'])
    print('S %d n %d %s: forward %.3f, backward %.3f of the bound' % (S, n, kind, rf, rb))
    assert rf <= 1 and rb <= 1
    assert np.isfinite(out).all() and np.isfinite(dx).all() and np.abs(out).max() > 0 and np.abs(dx).max() > 0
    if kind == 'hand' and n > 1:
        # image 1 is constant under the smallest scale (the source window is 1.5 x the image): inside, exactly the
        # constant; and its zero border is there
        mid = slice(S // 2 - 1, S // 2 + 1)
        assert (out[1, :, mid, mid] == np.float32(0.75)).all() and (out[1, :, 0, 0] == 0).all()
        exact = k['fb'][1] == 0
        assert exact.any() and np.array_equal(out[1][exact], k['out'][1][exact].astype(np.float32))
    if kind == 'hand' and n > 2:
        # image 2 is one-hot: only the outputs inside the box of the inverse see it
        assert 0 < (out[2] != 0).sum() <= 3 * 49


def test_rotation_by_45_degrees_of_a_constant_image():
    """interior pixels come back exactly, the corners fall to zero"""
    dev = torch.device('cuda', 0)
    for S in (8, 10, 64):
        x = np.full((1, 3, S, S), 0.75, dtype=np.float32)
        mats = R.case_mats(1)
        out = host(run_fwd(x, 0, mats, dev), (1, 3, S, S))
        assert R.ratio(out, R.forward(x, mats), R.forward_bound(x, mats)) <= 1
        # no spread and the full value over the 4 x 4 pixels around the position: all of them inside the image
        interior = R.forward_model(x, mats)[0] == 2.0 ** -23 * 0.75
        assert interior[:, S // 2, S // 2].all() and (out[0][interior] == np.float32(0.75)).all()
        assert (out[0, :, [0, 0, -1, -1], [0, -1, 0, -1]] == 0).all()


@pytest.mark.parametrize('S', [8, 10, 64])
def test_flip_rot90_and_identity_are_permutations_bit_for_bit(S):
    dev = torch.device('cuda', 0)
    rng = np.random.RandomState(S)
    x = rng.standard_normal((9, 3, S, S)).astype(np.float32)
    u = np.zeros((9, 8), dtype=np.float32)
    combos = [(f, k) for f in (False, True) for k in range(4)]
    for i, (f, k) in enumerate(combos):
        u[i, 0], u[i, 1] = (0.75 if f else 0.25), (k + 0.5) / 4
    mats, applied = prepare(u, R.FLIP | R.ROT90, dev)
    mats[8] = (1, 0, 0, 1)                  # the identity: the copy path
    assert set(np.abs(mats).ravel().tolist()) == {0.0, 1.0}
    want = np.stack([np.rot90(x[i, :, :, ::-1] if f else x[i], k, axes=(1, 2)) for i, (f, k) in enumerate(combos)]
                    + [x[8]])
    out = host(run_fwd(x, 4, mats, dev), x.shape)
    assert np.array_equal(out, want)
    assert np.array_equal(bits(out[8]), bits(x[8]))
    back = host(run_bwd(want, mats, dev), x.shape)           # the adjoint of a permutation is its inverse
    assert np.array_equal(back, x)


@pytest.mark.parametrize('S,n', R.SHAPES)
def test_adjointness_and_identical_bits_from_two_calls(S, n):
    dev = torch.device('cuda', 0)
    c = case(S, n)
    k = c['drawn']
    a, b = run_fwd(c['x'], n // 2, k['mats'], dev), run_fwd(c['x'], n // 2, k['mats'], dev)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    ga, gb = run_bwd(c['g'], k['mats'], dev), run_bwd(c['g'], k['mats'], dev)
    assert torch.equal(ga.view(torch.int32), gb.view(torch.int32))
    out, dx = host(a, (n, 3, S, S)).astype(np.float64), host(ga, (n, 3, S, S)).astype(np.float64)
    lhs, rhs = float((out * c['g']).sum()), float((c['x'].astype(np.float64) * dx).sum())
    # each side is off its exact value by at most its elements' bounds weighted with the other factor
    slack = float((k['fb'] * np.abs(c['g'])).sum() + (k['bb'] * np.abs(c['x'])).sum())
    print('S %d: <fwd x, g> - <x, bwd g> = %.3g, slack %.3g' % (S, lhs - rhs, slack))
    assert abs(lhs - rhs) <= slack and abs(lhs) > 0


def test_operator_matches_the_entry_points_and_skips_the_detached_backward(monkeypatch):
    from sbagan import _lib, ops
    dev = torch.device('cuda', 0)
    S, n, nr = 10, 3, 1
    c = case(S, n)
    mats = torch.from_numpy(c['drawn']['mats']).to(dev)
    x, g = torch.from_numpy(c['x']).to(dev), torch.from_numpy(c['g']).to(dev)
    want = body(run_fwd(c['x'], nr, c['drawn']['mats'], dev)).view(n, 3, S, S)
    want_dx = body(run_bwd(c['g'][nr:], c['drawn']['mats'][nr:], dev)).view(n - nr, 3, S, S)
    names = []
    monkeypatch.setattr(_lib, 'AUDIT_HOOK', lambda name, args: names.append(name))
    leaf, real = x[nr:].clone().requires_grad_(True), x[:nr].clone().requires_grad_(True)
    out = ops.geoaug(real, leaf, mats)
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    out.backward(g)
    assert torch.equal(leaf.grad.view(torch.int32), want_dx.view(torch.int32))
    assert real.grad is None                        # no gradient for the real half
    assert names == ['sba_geoaug_fwd', 'sba_geoaug_bwd']
    del names[:]
    out = ops.geoaug(x[:nr], x[nr:], mats)          # a detached fake: nothing to launch backward
    assert not out.requires_grad and names == ['sba_geoaug_fwd']
    monkeypatch.setattr(_lib, 'AUDIT_HOOK', None)
    for bad in (mats[:2], mats.double(), mats.t().contiguous().t()):
        with pytest.raises(ValueError, match='mats must be'):
            ops.geoaug(x[:nr], x[nr:], bad)
    # geoaug_prepare through ops: the same bits as the entry point
    u = np.random.RandomState(100 * S + n).random_sample((n, 8)).astype(np.float32)
    m2, a2 = torch.zeros((n, 4), device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    ops.geoaug_prepare(torch.from_numpy(u).to(dev), None, None, 1, 15, m2, a2)
    assert torch.equal(m2, mats) and a2.tolist() == [15] * n
    with pytest.raises(ValueError, match='values of p'):
        ops.geoaug_prepare(torch.from_numpy(u).to(dev), torch.zeros((n, 4), device=dev), torch.zeros(1, device=dev), 2, 15,
                           m2, a2)


# ---- the losses: geometry first, then colour, translation and cutout --------------------------------------------------
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


def test_chained_path_is_the_two_units_one_after_the_other(det, monkeypatch):
    import model
    from miscc import losses
    from sbagan import ops
    from sbagan.diffaug import DiffAugment
    from sbagan.geoaug import GeoAugment
    dev = torch.device('cuda', 0)
    ops.set_compute_dtype(torch.float32)
    monkeypatch.setattr(ops, 'SIDE_WGRAD', False)
    B, S = 4, 64
    torch.manual_seed(7)
    real, fake = torch.randn((B, 3, S, S), device=dev), torch.randn((B, 3, S, S), device=dev).tanh()
    g = torch.randn((2 * B, 3, S, S), device=dev)
    for gated in (False, True):
        aug = DiffAugment('color,translation,cutout', B, 1, dev, p0=0.5 if gated else None)
        geo = GeoAugment('flip,rot90,scale,rotate', B, 1, dev, p=aug.p if gated else None)
        aug.draw()
        geo.draw()
        geo.prepare()
        assert geo.gated == gated and bool(geo.mats.any())
        if gated:
            assert len(set(geo.applied.tolist())) > 1
        # the D update: [real | fake] joined by the warp, then the existing kernels over the joined batch
        seen = losses._seen(real, fake, aug.d_arg(0), geo.d_mats(0))
        warped = ops.geoaug(real, fake, geo.d_mats(0))
        assert not torch.equal(warped, torch.cat((real, fake), 0))
        assert torch.equal(seen, losses._augmented(None, warped, aug.d_arg(0)))
        assert torch.equal(losses._seen(real, fake, None, geo.d_mats(0)), warped)
        assert torch.equal(losses._seen(real, fake, aug.d_arg(0), None), losses._augmented(real, fake, aug.d_arg(0)))
        # the G term: the gradient comes back through both adjoints
        a, b = fake.clone().requires_grad_(True), fake.clone().requires_grad_(True)
        losses._seen(None, a, aug.g_arg(0), geo.g_mats(0)).backward(g[:B])
        losses._augmented(None, ops.geoaug(None, b, geo.g_mats(0)), aug.g_arg(0)).backward(g[:B])
        assert torch.equal(a.grad, b.grad) and bool(a.grad.abs().sum() > 0)
    # through the loss functions, no tolerance: the augmented loss is the plain loss on the units' own output
    net = model.D_NET64().to(dev).train()
    sent = torch.randn((B, 256), device=dev)
    ones, zeros = torch.ones(B, device=dev), torch.zeros(B, device=dev)
    errs = []
    for kw, r, f in (({'augment': aug.d_arg(0), 'geo': geo.d_mats(0)}, real, fake), ({}, seen[:B], seen[B:])):
        ops.det_reset()
        errs.append(losses.discriminator_loss(net, r, f, sent, ones, zeros, **kw).detach().clone())
    assert torch.equal(errs[0].view(torch.int32), errs[1].view(torch.int32)) and bool(torch.isfinite(errs[0]))
    for p in net.parameters():
        p.requires_grad_(False)
    ops.det_reset()
    value, grad = losses.generator_d_term(net, fake, sent, augment=aug.g_arg(0), geo=geo.g_mats(0))
    leaf = fake.clone().requires_grad_(True)
    ops.det_reset()
    inline = losses._g_term(net, net(losses._augmented(None, ops.geoaug(None, leaf, geo.g_mats(0)), aug.g_arg(0))), sent)
    inline.backward()
    assert torch.equal(inline.detach().view(torch.int32), value.view(torch.int32))
    assert torch.equal(leaf.grad, grad) and bool(grad.abs().sum() > 0)
    with pytest.raises(ValueError, match='geo does not go with real_features'):
        losses.discriminator_loss(net, real, fake, sent, ones, zeros, real_features=real, geo=geo.d_mats(0))


# ---- the training step: the toy data set and settings of tests/test_replay_train_gpu.py --------------------------------
POLICY, GEO = 'color,translation,cutout', 'flip,rot90,scale,rotate'


@pytest.fixture(scope='module')
def toy(tmp_path_factory):
    import datasets
    from sbagan.device_data import DeviceImageCache
    from test_replay_train_gpu import CROP, make_dataset, toy_cfg
    toy_cfg()
    root = make_dataset(str(tmp_path_factory.mktemp('geoaug') / 'toy'))
    ds = datasets.TextDataset(root, 'train', base_size=64, transform=None)
    cache = DeviceImageCache(ds, int(CROP * 76 / 64), torch.device('cuda', 0), max_bytes=1 << 30, workers=0)
    return {'root': root, 'ds': ds, 'cache': cache, 'tmp': tmp_path_factory, 'runs': {}}


def run(toy, geoaug, eager, steps, diffaug=POLICY, ada=0.6, touch=True):
    """one --device_data --replay [--diffaug ... --ada ...] [--geoaug ...] run of the trainer in f32 (cached): the final
    training state, every draw of the geometry's uniforms and the recording's node counts.  touch=False: the trainer's
    geoaug attribute is left as the class has it."""
    key = (geoaug, bool(eager), steps, diffaug, ada, touch)
    if key in toy['runs']:
        return toy['runs'][key]
    from sbagan import ops
    from sbagan.device_data import DeviceBatchLoader
    from test_replay_train_gpu import B, CROP, SEED
    from trainer import condGANTrainer
    ops.set_compute_dtype(torch.float32)
    ds = toy['ds']
    loader = DeviceBatchLoader(ds, toy['cache'], B, CROP, 2, seed=SEED)
    torch.manual_seed(3)
    algo = condGANTrainer(str(toy['tmp'].mktemp('out')), loader, ds.n_words, ds.ixtoword, allow_random_encoders=True)
    algo.replay, algo.replay_eager, algo.diffaug = True, eager, diffaug
    if diffaug:         # an update behind every step and a step of p of 0.25, as in tests/test_ada_gpu.py
        algo.ada, algo.ada_kimg, algo.ada_interval, algo.diffaug_p = ada, 0.016, 1, 0.5       # (p starts at 0.5)
    if touch:
        algo.geoaug = geoaug
    algo.train(max_steps=steps)
    torch.cuda.synchronize()
    gan, state = algo.gan, {}
    for name, flat, opt in [('G', gan.flatG, gan.optG)] + [('D%d' % i, f, o) for i, (f, o) in
                                                            enumerate(zip(gan.flatD, gan.optD))]:
        state[name + '/param'], state[name + '/m'], state[name + '/v'] = flat.data.cpu(), flat.m.cpu(), flat.v.cpu()
        state[name + '/adam_state'] = opt.state.cpu()
        if flat.avg is not None:
            state[name + '/ema'] = flat.avg.cpu()
    if gan.augment is not None and gan.augment.gated:
        a = gan.augment
        state['ada/p'], state['ada/rt'], state['ada/counters'] = a.p.cpu(), a.rt.cpu(), a.counters.cpu()
    geo = gan.geo_augment
    if geo is not None:
        state['geo/uniforms'], state['geo/mats'], state['geo/applied'] = geo.uniforms.cpu(), geo.mats.cpu(), geo.applied.cpu()
        if geo.gated:
            state['geo/gates'] = geo.gates.cpu()
    rec = algo.slot_step.recording
    res = {'state': state, 'geo': geo, 'augment': gan.augment, 'info': None if rec is None else dict(rec.info)}
    toy['runs'][key] = res
    return res


def test_recorded_loop_trains_what_the_eager_loop_trains(toy, det):
    """--device_data --replay --diffaug color,translation,cutout --geoaug flip,rot90,scale,rotate --ada 0.6, five steps
    in the deterministic mode: weights, Adam moments, EMA, p, the counters, and the last step's matrices, bit for bit"""
    a, b = run(toy, GEO, False, 5), run(toy, GEO, True, 5)
    assert a['info'] is not None and b['info'] is None
    geo = a['geo']
    assert geo.flags == 15 and geo.gated and geo.p is a['augment'].p
    assert {'ada/p', 'ada/counters', 'G/ema', 'D1/m', 'geo/mats', 'geo/applied', 'geo/gates'} <= set(a['state'])
    bad = [k for k in a['state'] if not torch.equal(a['state'][k], b['state'][k])]
    assert not bad, bad
    assert all(bool(torch.isfinite(t.float()).all()) for t in a['state'].values())
    # the recorded prepare launch saw the last draw: its matrices are those of the final uniforms (p has moved since
    # that launch read it, so check the rows where every part was on, and the rows where none was)
    u, mats, applied = (a['state'][k].numpy() for k in ('geo/uniforms', 'geo/mats', 'geo/applied'))
    full = applied == 15
    if full.any():
        want, _ = R.matrices(u[full], 15)
        assert float(np.abs(mats[full] - want).max()) <= R.MATRIX_BOUND
    ident = applied == 0
    assert np.array_equal(mats[ident], np.tile(np.float32([1, 0, 0, 1]), (int(ident.sum()), 1)))


def test_geometry_changes_the_training_and_adds_its_launches(toy, det):
    """per discriminator two forwards (the D update, the G term) and one backward (the G term: the D update has no
    image gradient), plus the single prepare: 3 nD + 1 kernels more in the recording"""
    with_geo, without = run(toy, GEO, False, 5), run(toy, '', False, 2)
    nD = 2
    assert with_geo['info']['kernels'] == without['info']['kernels'] + 3 * nD + 1
    assert with_geo['info']['nodes'] >= without['info']['nodes'] + 3 * nD + 1
    assert without['geo'] is None


def test_flag_off_is_the_step_as_it_was(toy, det):
    """a step built with geo_augment = None records what a step built without the attribute being touched records, and
    trains the same weights"""
    off, untouched = run(toy, '', False, 2), run(toy, '', False, 2, touch=False)
    assert off['geo'] is None and untouched['geo'] is None
    # (the counts of event and wait nodes move by one or two between two captures of the same step: not compared)
    for k in ('nodes', 'kernels', 'copies', 'memsets', 'host_calls'):
        assert off['info'][k] == untouched['info'][k], (k, off['info'], untouched['info'])
    bad = [k for k in off['state'] if not torch.equal(off['state'][k], untouched['state'][k])]
    assert not bad, bad


def test_entry_point_hands_the_flag_over_and_trains(toy, tmp_path, monkeypatch, capsys):
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

    capsys.readouterr()
    main.main(['--cfg', _yml(tmp_path, toy['root']), '--gpu', '0', '--manualSeed', '5', '--device_data',
               '--device_data_gb', '1', '--replay', '--diffaug', POLICY, '--geoaug', GEO, '--ada', '0.6'], make_trainer=make)
    text = capsys.readouterr().out
    algo = trainers[0]
    geo = algo.gan.geo_augment
    assert algo.geoaug == GEO and geo is not None and geo.flags == 15 and algo.slot_step.recording is not None
    assert geo.gated and geo.p is algo.gan.augment.p
    assert tuple(geo.uniforms.shape) == (2 * 3 * 4, 8) and bool(geo.uniforms.any()) and bool(geo.mats.any())
    assert len([ln for ln in text.split('\n') if ln.startswith('ada p: ')]) == 1
    _checkpoints(tmp_path)
    made = []

    class Stub(object):
        def __init__(self, *a):
            made.append(self)

        def sampling(self, split_dir):
            pass

    monkeypatch.setattr(main, 'gen_example', lambda wordtoix, algo: None)
    main.main(['--cfg', _yml(tmp_path, toy['root'], FLAG=False), '--gpu', '0', '--geoaug', 'flip'], make_trainer=Stub)
    assert made[0].geoaug == '' and capsys.readouterr().out.count('--geoaug is ignored outside training') == 1
    reset_cfg()
