"""--truncation / --truncation_sweep on the device.  The two kernels through the C ABI on guarded buffers against the numpy
restatement of tests/truncation_ref.py (the contract is bit equality: no tolerance anywhere in this file), the hook in
the three generator classes at toy widths, sampling() with the flag, the psi sweep over its frozen set, and the psi
strips of gen_example."""
import io
import json
import os
import random

import numpy as np
import pytest
import torch

import sampling_harness as sh
import truncation_ref as R
from test_nearest_gpu import _rnn_generator, random_encoders  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
SHAPES = [(1, 1), (1, 256), (255, 3), (256, 256), (257, 260), (513, 256), (600, 100)]
PSIS = [0.0, 0.3, 0.7, 1.0]
GUARD = 32                       # elements in front of and behind every output: the bodies stay 8 / 16-byte aligned
FILL = -77.5
N_MEAN = 600                     # the tests' truncation_n: crosses two chunk edges with a ragged tail
_CASES = {}


def stream():
    return torch.cuda.current_stream().cuda_stream


def case(n, D):
    if (n, D) not in _CASES:
        rng = np.random.RandomState(1000 * n + D)
        w = (rng.standard_normal((n, D)) * 2 + 0.5).astype(np.float32)
        avg = (0.3 * rng.standard_normal(D)).astype(np.float32)
        _CASES[(n, D)] = (w, avg, R.style_mean(w))
    return _CASES[(n, D)]


def guarded(numel, dtype):
    return torch.full((numel + 2 * GUARD,), FILL, dtype=dtype, device=DEV)


def body(t):
    return t[GUARD:-GUARD]


def intact(t):
    return bool((t[:GUARD] == FILL).all()) and bool((t[-GUARD:] == FILL).all())


def bptr(t):
    """the address of a guarded tensor's body"""
    return t.data_ptr() + GUARD * t.element_size()


def run_mean(w_np):
    """sba_style_mean over w on guarded outputs and a guarded workspace of exactly the stated size; (mean64, mean32) numpy"""
    from sbagan import _lib
    n, D = w_np.shape
    w = torch.from_numpy(w_np).to(DEV)
    chunks = (n + 255) // 256
    m64, m32 = guarded(D, torch.float64), guarded(D, torch.float32)
    ws = guarded(chunks * D, torch.float64)
    rc = _lib.lib.sba_style_mean(w.data_ptr(), n, D, bptr(m64), bptr(m32), bptr(ws) if chunks > 1 else None, stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert intact(m64) and intact(m32) and intact(ws)
    if chunks == 1:
        assert bool((ws == FILL).all())              # (a single launch: the workspace is not needed)
    return body(m64).cpu().numpy(), body(m32).cpu().numpy()


def run_truncate(w_np, avg_np, psi, in_place=False):
    from sbagan import _lib
    n, D = w_np.shape
    avg = torch.from_numpy(avg_np).to(DEV)
    out = guarded(n * D, torch.float32)
    if in_place:
        body(out).copy_(torch.from_numpy(w_np).to(DEV).reshape(-1))
        src = bptr(out)
    else:
        w = torch.from_numpy(w_np).to(DEV)
        src = w.data_ptr()
    rc = _lib.lib.sba_style_truncate(src, avg.data_ptr(), float(psi), bptr(out), n, D, stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert intact(out)
    return body(out).cpu().numpy().reshape(n, D)


def same_bits(a, b):
    """bit equality as integer views; NaNs by position (equal_nan)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    nan = np.isnan(a)
    if not np.array_equal(nan, np.isnan(b)):
        return False
    view = np.int32 if a.dtype == np.float32 else np.int64
    return np.array_equal(a[~nan].view(view), b[~nan].view(view))


# ------------------------------------------------------------------ sba_style_mean
@pytest.mark.parametrize('n,D', SHAPES + [(16384, 256)])
def test_style_mean_has_the_bits_of_the_reference(n, D):
    w, _, (want64, want32) = case(n, D)
    got64, got32 = run_mean(w)
    assert np.array_equal(got64.view(np.int64), want64.view(np.int64))
    assert np.array_equal(got32.view(np.int32), got64.astype(np.float32).view(np.int32))
    assert np.array_equal(got32.view(np.int32), want32.view(np.int32))
    again64, again32 = run_mean(w)                   # two calls: the same bits
    assert np.array_equal(again64.view(np.int64), got64.view(np.int64))
    assert np.array_equal(again32.view(np.int32), got32.view(np.int32))


@pytest.mark.parametrize('n,D', [(255, 3), (600, 100)])
def test_a_nan_and_an_inf_reach_their_column_only(n, D):
    w, _, (clean64, _) = case(n, D)
    w = w.copy()
    w[n // 2, 1], w[n - 1, D - 1] = np.nan, -np.inf
    got64, got32 = run_mean(w)
    want64, want32 = R.style_mean(w)
    assert np.isnan(got64[1]) and np.isneginf(got64[D - 1]) and np.isnan(got32[1]) and np.isneginf(got32[D - 1])
    keep = np.ones(D, dtype=bool)
    keep[[1, D - 1]] = False
    assert np.array_equal(got64[keep].view(np.int64), clean64[keep].view(np.int64))
    assert same_bits(got64, want64) and same_bits(got32, want32)


def test_style_mean_refusals_write_nothing():
    from sbagan import _lib
    bad = _lib.CONSTANTS['SBA_E_ARG']
    n, D = 257, 8
    w = torch.zeros((n, D), dtype=torch.float32, device=DEV)
    m64, m32, ws = guarded(D + 1, torch.float64), guarded(D, torch.float32), guarded(2 * D, torch.float64)
    ok = [w.data_ptr(), n, D, bptr(m64), bptr(m32), bptr(ws)]
    cases = {'n = 0': (1, 0), 'D = 0': (2, 0), 'D = 4097': (2, 4097), 'n above 2^20': (1, (1 << 20) + 1),
             'w NULL': (0, None), 'mean64 NULL': (3, None), 'mean32 NULL': (4, None),
             'mean64 offset by 4 bytes': (3, bptr(m64) + 4), 'workspace NULL at n = 257': (5, None),
             'workspace offset by 4 bytes': (5, bptr(ws) + 4), 'w offset by 2 bytes': (0, w.data_ptr() + 2)}
    for what, (i, v) in cases.items():
        args = list(ok)
        args[i] = v
        assert _lib.lib.sba_style_mean(*args, stream()) == bad, what
    torch.cuda.synchronize()
    for t in (m64, m32, ws):
        assert bool((t == FILL).all())
    assert _lib.lib.sba_style_mean(*ok, stream()) == 0          # (and the call they were made from is accepted)
    assert _lib.lib.sba_style_mean(w.data_ptr(), 256, D, bptr(m64), bptr(m32), None, stream()) == 0   # NULL at n = 256
    torch.cuda.synchronize()


def test_the_operator_against_the_reference():
    from sbagan import ops
    w_np, avg_np, (want64, want32) = case(600, 100)
    w = torch.from_numpy(w_np).to(DEV)
    m64, m32 = ops.style_mean(w)
    assert m64.dtype == torch.float64 and m32.dtype == torch.float32 and m64.shape == m32.shape == (100,)
    assert np.array_equal(m64.cpu().numpy().view(np.int64), want64.view(np.int64))
    assert np.array_equal(m32.cpu().numpy().view(np.int32), want32.view(np.int32))
    avg = torch.from_numpy(avg_np).to(DEV)
    out = ops.style_truncate(w, avg, 0.7)
    assert out.data_ptr() != w.data_ptr() and same_bits(out.cpu().numpy(), R.style_truncate(w_np, avg_np, 0.7))
    assert ops.style_truncate(w, avg, 0.7, out=w) is w and torch.equal(w, out)
    for bad in (w.double(), w[:, ::2], w.cpu(), w.reshape(-1)):
        with pytest.raises((ValueError, RuntimeError)):
            ops.style_mean(bad)
    with pytest.raises(ValueError):
        ops.style_truncate(w, avg[:50], 0.5)
    with pytest.raises(RuntimeError, match='SBA_E_ARG'):
        ops.style_truncate(w, avg, float('nan'))


# ------------------------------------------------------------------ sba_style_truncate
@pytest.mark.parametrize('psi', PSIS)
@pytest.mark.parametrize('n,D', SHAPES)
def test_style_truncate_has_the_bits_of_the_reference(n, D, psi):
    w, avg, _ = case(n, D)
    w = w.copy()
    w[0, 0] = -0.0
    if n * D >= 6:
        w.reshape(-1)[[3, 4, 5]] = [np.nan, np.inf, -np.inf]
    want = R.style_truncate(w, avg, psi)
    got = run_truncate(w, avg, psi)
    assert same_bits(got, want), (n, D, psi)
    if psi == 1.0:                                   # a copy: the bits of the input, the NaN's too
        assert np.array_equal(got.view(np.int32), w.view(np.int32))
    assert np.array_equal(run_truncate(w, avg, psi, in_place=True).view(np.int32), got.view(np.int32))


def test_style_truncate_refusals_write_nothing():
    from sbagan import _lib
    bad = _lib.CONSTANTS['SBA_E_ARG']
    n, D = 3, 8
    w = torch.zeros((n, D), dtype=torch.float32, device=DEV)
    avg = torch.zeros((D,), dtype=torch.float32, device=DEV)
    out = guarded(n * D, torch.float32)
    ok = [w.data_ptr(), avg.data_ptr(), 0.5, bptr(out), n, D]
    for i, v in ((2, float('nan')), (2, float('inf')), (2, float('-inf')), (0, None), (1, None), (3, None),
                 (0, w.data_ptr() + 2), (1, avg.data_ptr() + 1), (3, bptr(out) + 2), (4, 0), (4, (1 << 20) + 1), (5, 0),
                 (5, 4097)):
        args = list(ok)
        args[i] = v
        assert _lib.lib.sba_style_truncate(*args, stream()) == bad, (i, v)
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    assert _lib.lib.sba_style_truncate(*ok, stream()) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the generators
@pytest.fixture()
def det():
    from miscc.config import reset_cfg
    from sbagan import ops
    ops.set_compute_dtype(torch.bfloat16)
    ops.set_deterministic(True, DEV)
    yield
    ops.set_deterministic(False)
    reset_cfg()


def generator(kind, branch):
    """an eval-mode generator of the class at toy widths (GF_DIM 32), seeded"""
    from miscc.config import cfg, reset_cfg
    from miscc.utils import weights_init
    reset_cfg()
    cfg.GAN.GF_DIM, cfg.GAN.DF_DIM, cfg.TREE.BRANCH_NUM = 32, 64, branch
    import model
    import model_bert
    torch.manual_seed(1)
    net = {'model': model.G_NET, 'bert': model_bert.G_NET, 'mix': model_bert.G_NET_MIX}[kind]()
    net.apply(weights_init)
    return net.to(DEV).eval()


def inputs(kind, seed=5, B=2, L=6):
    from miscc.config import cfg
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)

    def rnd(*shape):
        return torch.randn(shape, generator=g, device=DEV, dtype=torch.float32)
    z = rnd(2, B, cfg.GAN.Z_DIM) if kind == 'mix' else rnd(B, cfg.GAN.Z_DIM)
    sent, words = rnd(B, cfg.TEXT.EMBEDDING_DIM), rnd(B, cfg.TEXT.EMBEDDING_DIM, L)
    mask = torch.zeros((B, L), dtype=torch.bool, device=DEV)
    mask[1, L - 2:] = True
    return z, sent, words, mask, rnd(B, cfg.GAN.CONDITION_DIM)


def forward(net, z, sent, words, mask, eps, call=None):
    """the images of every stage; eps fixed (CA_NET would draw it from the global generator)"""
    from sbagan import ops
    net.ca_net.eps = eps
    try:
        with torch.no_grad():
            ops.det_reset()
            imgs = (call or net)(z, sent, words, mask)[0]
        torch.cuda.synchronize()
        return [i.clone() for i in imgs]
    finally:
        net.ca_net.eps = None


@pytest.mark.parametrize('kind', ['model', 'bert', 'mix'])
def test_styles_returns_the_reference_applied_to_the_mapping_network(det, kind):
    from sbagan.truncation import Truncation, mapped_styles, mean_style, pass_rows
    net = generator(kind, 3)
    z, _, words, _, _ = inputs(kind)
    zs = (z[0], z[1]) if kind == 'mix' else (z,)
    with torch.no_grad():
        plain = [net.mapping_net(v).cpu().numpy() for v in zs]
    # w_avg: the reference's mean over the rows mean_style averages -- the mapping network on the codes of a generator
    # of its own, seeded the same way (a pass of the dense kernels takes 64 rows at W_DIM 256: the first 20 checked here)
    rows = mapped_styles(net, N_MEAN, 100)
    assert rows.shape == (N_MEAN, net.mapping_net.w_dim) and pass_rows(net.mapping_net) == 64
    g = torch.Generator(device=DEV)
    g.manual_seed(100)
    codes = torch.randn((N_MEAN, net.mapping_net.z_dim), generator=g, device=DEV, dtype=torch.float32)
    with torch.no_grad():           # (another batch size may take another dense kernel: the f32 bound of 8 layers of K <= 256)
        for part in (slice(0, 20), slice(N_MEAN - 20, N_MEAN)):
            again = net.mapping_net(codes[part])
            assert float((rows[part] - again).abs().max()) <= 8 * 256 * 2.0 ** -24 * float(again.abs().max())
    want64, want32 = R.style_mean(rows.cpu().numpy())
    state = torch.cuda.get_rng_state(), torch.get_rng_state()
    got64, got32 = mean_style(net, N_MEAN, 100)
    assert torch.equal(torch.cuda.get_rng_state(), state[0]) and torch.equal(torch.get_rng_state(), state[1])
    assert np.array_equal(got64.cpu().numpy().view(np.int64), want64.view(np.int64))
    assert np.array_equal(got32.cpu().numpy().view(np.int32), want32.view(np.int32))
    for psi in (0.5, (0.7, 0.2), 1.0):
        net.truncation = t = Truncation(net, psi, N_MEAN)
        assert np.array_equal(t.w_avg.cpu().numpy().view(np.int32), want32.view(np.int32)) and t.w_avg.device == z.device
        with torch.no_grad():
            ws, _ = net._styles(*zs, word_embs=words)
        torch.cuda.synchronize()
        a, b = t.psi
        if kind == 'mix':
            want = [R.style_truncate(plain[0], want32, a), R.style_truncate(plain[1], want32, b)]
        else:
            want = [R.style_truncate(plain[0], want32, a)] + ([R.style_truncate(plain[0], want32, b)] if a != b else [])
        assert len(ws) == len(want)
        for got, w in zip(ws, want):
            assert same_bits(got.cpu().numpy(), w), (kind, psi)
    net.truncation = None
    with torch.no_grad():
        ws, _ = net._styles(*zs, word_embs=words)
    torch.cuda.synchronize()
    assert [same_bits(a.cpu().numpy(), b) for a, b in zip(ws, plain)] == [True] * len(plain)


@pytest.mark.parametrize('kind', ['model', 'bert', 'mix'])
def test_psi_1_is_the_generator_without_a_truncation_and_training_mode_raises(det, kind):
    from sbagan.truncation import Truncation
    net = generator(kind, 2)
    args = inputs(kind)
    plain = forward(net, *args)
    net.truncation = Truncation(net, 1.0, N_MEAN)
    one = forward(net, *args)
    assert len(one) == 2 and all(torch.equal(a, b) for a, b in zip(one, plain))
    net.truncation = Truncation(net, 0.25, N_MEAN)
    quarter = forward(net, *args)
    assert not torch.equal(quarter[-1], plain[-1])
    # no backward: training mode and grad mode are refused, and the generator still runs once the truncation is cleared
    with pytest.raises(RuntimeError, match='eval mode under no_grad'):
        net(*args[:4])
    net.train()
    with pytest.raises(RuntimeError, match='eval mode under no_grad'), torch.no_grad():
        net(*args[:4])
    net.eval()
    torch.cuda.synchronize()
    net.truncation = None
    assert all(torch.equal(a, b) for a, b in zip(forward(net, *args), plain))


def test_construction_refuses_what_cannot_be_truncated(det):
    from sbagan.truncation import Truncation
    net = generator('model', 2)
    for psi in (1.5, -0.1, float('nan'), (0.5, 0.5), (0.5, 0.5, 0.5)):      # (a pair needs BRANCH_NUM 3)
        with pytest.raises(ValueError):
            Truncation(net, psi, N_MEAN)
    with pytest.raises(ValueError, match='no stage reads a style'):
        Truncation(generator('model', 1), 0.5, N_MEAN)
    t = Truncation(generator('bert', 3), (0.5, 1.0), N_MEAN)
    assert t.psi == (0.5, 1.0)
    held = t.w_avg.clone()
    with torch.no_grad():
        t.netG.mapping_net.fc[0].weight.mul_(2.0)
    assert torch.equal(t.w_avg, held) and not torch.equal(t.refresh().w_avg, held)


def test_bert_generator_at_psi_0_does_not_depend_on_the_noise(det):
    from sbagan.truncation import Truncation
    net = generator('bert', 3)
    z1, sent, words, mask, eps = inputs('bert', seed=5)
    z2 = inputs('bert', seed=6)[0]
    plain = [forward(net, z, sent, words, mask, eps) for z in (z1, z2)]
    assert not torch.equal(plain[0][-1], plain[1][-1])
    net.truncation = Truncation(net, 0.0, N_MEAN)
    a, b = (forward(net, z, sent, words, mask, eps) for z in (z1, z2))
    assert len(a) == 3 and all(torch.equal(x, y) for x, y in zip(a, b))


def test_model_generator_keeps_its_first_stage(det):
    from sbagan.truncation import Truncation
    net = generator('model', 2)
    args = inputs('model')
    plain = forward(net, *args)
    net.truncation = Truncation(net, 0.5, N_MEAN)
    half = forward(net, *args)
    assert torch.equal(half[0], plain[0]) and not torch.equal(half[-1], plain[-1])


def test_mix_generator_at_psi_0_does_not_tell_its_two_codes_apart(det):
    from sbagan.truncation import Truncation
    net = generator('mix', 3)
    z, sent, words, mask, eps = inputs('mix')
    swapped = torch.cat([z[1:], z[:1]], 0).contiguous()
    plain = forward(net, z, sent, words, mask, eps), forward(net, swapped, sent, words, mask, eps)
    assert not torch.equal(plain[0][-1], plain[1][-1])
    net.truncation = Truncation(net, 0.0, N_MEAN)
    a, b = forward(net, z, sent, words, mask, eps), forward(net, swapped, sent, words, mask, eps)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('kind', ['model', 'mix'])
def test_a_pair_sets_the_stages_apart(det, kind):
    from sbagan.truncation import Truncation
    net = generator(kind, 3)
    args = inputs(kind)
    plain = forward(net, *args)
    net.truncation = Truncation(net, (1.0, 0.0), N_MEAN)
    got = forward(net, *args)
    assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1]) and not torch.equal(got[2], plain[2])


def test_fused_generator_with_a_truncation(det):
    from sbagan.infer import FusedGenerator
    from sbagan.truncation import Truncation, set_truncation, unwrap
    net = generator('model', 2)
    fused = FusedGenerator(net)
    assert unwrap(fused) is net and unwrap(net) is net
    args = inputs('model')
    plain = forward(net, *args, call=fused)
    assert set_truncation(fused, 1.0, N_MEAN) is net.truncation and isinstance(net.truncation, Truncation)
    one = forward(net, *args, call=fused)
    assert all(torch.equal(a, b) for a, b in zip(one, plain))
    set_truncation(fused, 0.5, N_MEAN)
    half = forward(net, *args, call=fused)
    assert torch.equal(half[0], plain[0]) and not torch.equal(half[-1], plain[-1])
    assert bool(torch.isfinite(half[-1].float()).all())
    assert set_truncation(fused, None) is None and net.truncation is None


# ------------------------------------------------------------------ sampling()
EVALS = dict(prdc=2, kid=True, kid_subsets=4, kid_subset_size=4, r_precision=3)


@pytest.fixture(scope='module')
def toy(tmp_path_factory):
    """the toy data set of the sampling harness with one checkpoint copy per run, and the runs made so far"""
    names = ('plain', 'one', 'half', 'half_again', 'evals', 'sweep', 'sweep_reversed')
    make, loader, ds, ckpts = sh.setup(tmp_path_factory.mktemp('truncation'), names)
    return {'make': make, 'loader': loader, 'ds': ds, 'ckpts': dict(zip(names, ckpts)), 'runs': {}}


def run(toy, name, **attrs):
    """(trainer, files, generator states, trunk forwards, what its sweep was handed) of one seeded deterministic sampling
    run, made once"""
    from sbagan import ops, truncation
    if name not in toy['runs']:
        sh.toy_cfg()
        ops.set_compute_dtype(torch.bfloat16)
        seen, sweep = {}, truncation.sweep

        def spy(trainer, generator, text_encoder, psis, split_dir, out_dir, n=0, image_encoder=None):
            seen.update(generator=generator, text_encoder=text_encoder, image_encoder=image_encoder, split=split_dir, n=n)
            return sweep(trainer, generator, text_encoder, psis, split_dir, out_dir, n=n, image_encoder=image_encoder)
        truncation.sweep = spy
        try:
            algo, files, states, calls = sh.sample(toy['make'], toy['loader'], toy['ds'], toy['ckpts'][name], **attrs)
        finally:
            truncation.sweep = sweep
        toy['runs'][name] = (algo, files, states + (random.getstate(),), calls, seen)
    return toy['runs'][name]


def same_states(a, b):
    return sh.same_states(a, b) and a[3] == b[3]                        # numpy, torch.cuda, torch; python's


def test_sampling_at_psi_1_is_the_run_without_the_flag(toy):
    from sbagan.truncation import check_record
    _, files0, states0, calls0, _ = run(toy, 'plain')
    algo1, files1, states1, calls1, _ = run(toy, 'one', truncation=1.0, truncation_n=N_MEAN)
    assert len(files0) == 6 and all(k.endswith('.png') for k in files0) and calls0 == calls1 == 0
    assert sorted(files1) == sorted(list(files0) + ['truncation.json']) and sh.images(files1) == files0
    assert same_states(states1, states0)
    record = json.loads(files1['truncation.json'].decode())
    assert check_record(record) == algo1.truncation_result
    assert (record['psi'], record['n'], record['seed'], record['w_rows']) == ([1.0, 1.0], N_MEAN, 100, 6)
    assert record['w_rms_distance'] > 0


def test_sampling_at_psi_half_differs_and_repeats(toy):
    import model
    from sbagan.truncation import mapped_styles
    files0 = run(toy, 'plain')[1]
    _, files1, states1, _, _ = run(toy, 'half', truncation=0.5, truncation_n=N_MEAN)
    _, files2, states2, _, _ = run(toy, 'half_again', truncation=0.5, truncation_n=N_MEAN)
    assert sorted(sh.images(files1)) == sorted(files0)
    assert all(sh.images(files1)[k] != files0[k] for k in files0)
    assert files1 == files2 and same_states(states1, states2)
    # |w_avg|: the reference's mean over the checkpoint's own mapping network, the same seed and n
    sh.toy_cfg()
    net = model.G_NET()
    net.load_state_dict(torch.load(toy['ckpts']['half'], map_location='cpu'))
    net.to(DEV).eval()
    want64, _ = R.style_mean(mapped_styles(net, N_MEAN, 100).cpu().numpy())
    record = json.loads(files1['truncation.json'].decode())
    assert record['psi'] == [0.5, 0.5]
    assert record['w_avg_norm'] == pytest.approx(float(np.sqrt(np.sum(want64 * want64))), rel=1e-12)


def test_main_with_the_flag(tmp_path, random_encoders):  # noqa: F811
    import main
    from miscc.config import reset_cfg
    from sbagan.truncation import check_record
    root = _rnn_generator(tmp_path)
    files, _, calls = sh.run_main(main, tmp_path, 'with', ['--truncation', '0.5', '--truncation_n', str(N_MEAN),
                                                           '--prdc', '2'], root)
    assert sorted(k for k in files if not k.endswith('.png')) == ['prdc.json', 'truncation.json'] and calls == 3 + 3
    assert check_record(json.loads(files['truncation.json'].decode()))['psi'] == [0.5, 0.5]
    assert len(sh.images(files)) == 6
    reset_cfg()


# ------------------------------------------------------------------ the sweep
def _metrics(records):
    return {r['psi']: json.loads(json.dumps(r['metrics'])) for r in records}


def test_the_sweep_leaves_the_normal_run_alone_and_measures_on_one_frozen_set(toy):
    from sbagan import evaluation, ops, track, truncation
    _, files0, states0, calls0, _ = run(toy, 'evals', **EVALS)
    algo, files1, states1, calls1, seen = run(toy, 'sweep', truncation_sweep=(1.0, 0.5), truncation_n=N_MEAN, **EVALS)
    # the normal run: the same files, figures and generator states
    assert sorted(files1) == sorted(list(files0) + ['truncation_sweep.json'])
    assert {k: v for k, v in files1.items() if k in files0} == files0 and same_states(states1, states0)
    records = json.loads(files1['truncation_sweep.json'].decode())
    assert truncation.check_sweep(records) and [r['psi'] for r in records] == [1.0, 0.5]
    for r in records:
        assert sorted(r['metrics']) == ['kid', 'prdc', 'r_precision'] and r['seconds'] > 0
        assert r['metrics']['prdc']['n_real'] == r['metrics']['prdc']['n_fake'] == r['metrics']['r_precision']['n'] == 6
    # the trunk: each real image once in the sweep, each generated batch once per psi (R-precision's pass is shared)
    assert calls0 == 3 + 3 and calls1 - calls0 == 3 + 2 * 3
    # psi = 1 is the measurement of a frozen set over the same checkpoint with no truncation set
    assert seen['split'] == 'test' and seen['n'] == 0 and seen['image_encoder'] is not None
    net = truncation.unwrap(seen['generator'])
    assert net.truncation is None                                       # (put back behind the sweep)
    values = {opt.name: getattr(algo, opt.name) for opt in evaluation.OPTIONS}
    sh.toy_cfg()
    ops.set_deterministic(True, DEV)
    try:
        frozen = track.FrozenSet(algo._encode, algo._noise_shape, algo.batch_size, algo.device, values, 'test')
        frozen.prepare(seen['text_encoder'], seen['image_encoder'],
                       truncation.plain_dataset(toy['loader'].dataset, 'test'), what='test')
        assert frozen.rows == frozen.images == 6 and frozen.slices() == [(0, 2), (2, 4), (4, 6)]
        want = json.loads(json.dumps(frozen.measure(seen['generator'], net.ca_net)))
    finally:
        ops.set_deterministic(False)
    assert _metrics(records)[1.0] == want
    assert _metrics(records)[0.5] != want


def test_a_sweep_record_is_a_function_of_psi_alone(toy):
    files1 = run(toy, 'sweep', truncation_sweep=(1.0, 0.5), truncation_n=N_MEAN, **EVALS)[1]
    files2 = run(toy, 'sweep_reversed', truncation_sweep=(0.5, 1.0), truncation_n=N_MEAN, **EVALS)[1]
    a, b = (json.loads(f['truncation_sweep.json'].decode()) for f in (files1, files2))
    assert [r['psi'] for r in b] == [0.5, 1.0] and _metrics(a) == _metrics(b)


def test_the_sweep_refuses_a_run_that_measures_nothing(toy):
    from sbagan import truncation
    sh.toy_cfg()
    algo = toy['make'](os.path.dirname(toy['ckpts']['plain']), toy['loader'], toy['ds'].n_words, toy['ds'].ixtoword)
    algo.ms_ssim = 2
    with pytest.raises(ValueError, match='needs at least one of fid, kid, prdc, r_precision'):
        truncation.sweep(algo, None, None, (1.0,), 'test', '.')


# ------------------------------------------------------------------ gen_example
def _files(root):
    return sh.files_under(root)


@pytest.mark.parametrize('bert', [False, True], ids=['rnn', 'bert'])
def test_gen_example_writes_the_psi_strips(tmp_path, bert):
    from miscc.config import cfg, reset_cfg
    from PIL import Image
    from sbagan import ops
    make, loader, ds, ckpts = sh.setup(tmp_path, ('off', 'on'), bert=bert)
    caps = np.array([[1, 2, 3, 4, 5, 6, 7], [3, 2, 1, 0, 0, 0, 0]], dtype=np.int64)
    psis = (1.0, 0.5, 0.0)
    roots, states = [], []
    ops.set_deterministic(True, DEV)
    try:
        for ckpt, sweep in zip(ckpts, (None, psis)):
            cfg.TRAIN.NET_G = ckpt
            algo = make(os.path.dirname(ckpt), loader, ds.n_words, ds.ixtoword)
            algo.truncation_sweep, algo.truncation_n = sweep, N_MEAN
            sh.seed_all(100)
            roots.append(algo.gen_example({'bird': [caps, np.array([7, 3]), np.array([1, 0])]}))
            states.append(sh.rng_states())
    finally:
        ops.set_deterministic(False)
    files0, files1 = _files(roots[0]), _files(roots[1])
    strips = ['bird/0_s_%d_psi.png' % i for i in (0, 1)]
    assert sorted(files1) == sorted(list(files0) + strips)
    assert {k: v for k, v in files1.items() if k in files0} == files0      # the run's own images: byte for byte
    assert sh.same_states(states[0], states[1])                            # the strips draw nothing
    S, last = 128, '_g1_A.png' if bert else '_g1.png'
    for i in (0, 1):
        strip = Image.open(io.BytesIO(files1['bird/0_s_%d_psi.png' % i]))
        assert strip.size == (len(psis) * S, S)
        tiles = [np.asarray(strip.crop((S * k, 0, S * k + S, S))) for k in range(len(psis))]
        image = np.asarray(Image.open(io.BytesIO(files0['bird/0_s_%d%s' % (i, last)])))
        assert np.array_equal(tiles[0], image)                              # psi = 1: the image the run wrote
        assert not np.array_equal(tiles[1], image) and not np.array_equal(tiles[2], tiles[1])
    reset_cfg()
