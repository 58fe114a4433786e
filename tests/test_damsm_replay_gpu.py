"""pretrain_DAMSM.py --replay on the device: the kernels of csrc/damsm_step.hip through the C ABI against the float64
references (tests/damsm_step_ref.py), sbagan.damsm.DAMSMSlotStep against the existing DAMSMStep.step, the replayed loop
against the same loop launched eagerly over the same slot (bit for bit in the deterministic mode), and the BERT entry
point, which ignores the flag.

The toy directory is the one tests/test_replay_train_gpu.py writes: 8 training images in 2 classes, captions of 3 to 8
words, WORDS_NUM = 8."""
import copy
import glob
import os
import pickle
import re

import numpy as np
import pytest
import torch

import damsm_step_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64                      # floats around every kernel output, checked untouched
EPS24, EPS22 = 2.0 ** -24, 2.0 ** -22


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _st():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from sbagan import _lib
    return _lib.lib


# ---------------------------------------------------------------------------------------------------------------
# embedding + dropout
# ---------------------------------------------------------------------------------------------------------------
def _ed_case(name):
    """(ids, ntoken, ninput, keep, p).  Every id list holds repeats unless it says otherwise."""
    rng = np.random.RandomState(sum(map(ord, name)))
    ntoken, p = 11, 0.3
    if name == 'n1':
        N, ninput, p = 1, 4, 0.5
        ids = np.array([2], dtype=np.int64)
    elif name == 'n37_c4':
        N, ninput = 37, 4
        ids = rng.randint(0, ntoken, N).astype(np.int64)
    elif name in ('n37_c300', 'all_keep', 'all_drop', 'p_half'):
        N, ninput = 37, 300
        ids = rng.randint(0, ntoken, N).astype(np.int64)
        p = 0.5 if name == 'p_half' else 0.3
    elif name == 'one_id':              # one row of dW owns all N positions
        N, ninput = 37, 300
        ids = np.full(N, 6, dtype=np.int64)
    elif name == 'edge_rows':           # the first and the last row of W, each held twice
        N, ninput = 37, 300
        ids = rng.randint(1, ntoken - 1, N).astype(np.int64)
        ids[[3, 20]], ids[[0, 36]] = 0, ntoken - 1
    elif name == 'bad_ids':             # ntoken and -1: compared before they index; rows of zeros, nothing added
        N, ninput = 37, 300
        ids = rng.randint(0, ntoken, N).astype(np.int64)
        ids[5], ids[17], ids[36] = ntoken, -1, 2 ** 40 + 3
    elif name == 'max_n':               # the largest batch the entry points take: grid-stride forward, full LDS table
        N, ninput, ntoken = 8192, 300, 50
        ids = rng.randint(0, ntoken, N).astype(np.int64)
    else:
        raise KeyError(name)
    keep = (rng.rand(N, ninput) >= p).astype(np.uint8)
    if name == 'all_keep':
        keep[:] = 1
    if name == 'all_drop':
        keep[:] = 0
    if name == 'n37_c4':                # any non-zero byte keeps
        keep[keep != 0] = rng.randint(1, 256, int((keep != 0).sum())).astype(np.uint8)
    return ids, ntoken, ninput, keep, p


ED_CASES = ['n1', 'n37_c4', 'n37_c300', 'one_id', 'edge_rows', 'all_keep', 'all_drop', 'p_half', 'bad_ids', 'max_n']


def _guarded(n, dev, fill=-7.5):
    return torch.full((n + 2 * GUARD,), fill, dtype=torch.float32, device=dev)


@pytest.mark.parametrize('name', ED_CASES)
def test_embed_dropout_forward(dev, name):
    ids, ntoken, ninput, keep, p = _ed_case(name)
    N = len(ids)
    rng = np.random.RandomState(N + ninput)
    W = rng.uniform(-0.1, 0.1, (ntoken, ninput)).astype(np.float32)
    scale = float(1.0 / (1.0 - p))
    d_ids, d_W, d_keep = (torch.from_numpy(a).to(dev) for a in (ids, W, keep))
    outs = []
    for _ in range(2):
        buf = _guarded(N * ninput, dev)
        rc = _lib().sba_embed_dropout_fwd(d_ids.data_ptr(), d_W.data_ptr(), d_keep.data_ptr(), scale,
                                          buf.data_ptr() + 4 * GUARD, N, ntoken, ninput, _st())
        assert rc == 0
        torch.cuda.synchronize()
        outs.append(buf)
    assert torch.equal(outs[0], outs[1])
    host = outs[0].cpu().numpy()
    assert (host[:GUARD] == -7.5).all() and (host[-GUARD:] == -7.5).all()
    got = host[GUARD:-GUARD].reshape(N, ninput)
    valid = (ids >= 0) & (ids < ntoken)
    want = np.zeros((N, ninput), dtype=np.float32)
    want[valid] = W[ids[valid]] * np.float32(scale)                 # one f32 multiply
    want[keep == 0] = 0.0
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))        # bit for bit, dropped = +0
    ref = R.embed_dropout_fwd(ids, W, keep, np.float32(scale))
    assert (np.abs(got - ref) <= EPS24 * np.abs(ref)).all()
    if name == 'bad_ids':
        assert not got[[5, 17, 36]].any()


def _run_bwd(dev, ids, ntoken, ninput, keep, scale, dout, dW0):
    N = len(ids)
    d_ids, d_keep, d_dout = (torch.from_numpy(a).to(dev) for a in (ids, keep, dout))
    buf = _guarded(ntoken * ninput, dev)
    buf[GUARD:-GUARD].copy_(torch.from_numpy(dW0.reshape(-1)))
    rc = _lib().sba_embed_dropout_bwd(d_ids.data_ptr(), d_keep.data_ptr(), scale, d_dout.data_ptr(),
                                      buf.data_ptr() + 4 * GUARD, N, ntoken, ninput, _st())
    assert rc == 0
    torch.cuda.synchronize()
    return buf


@pytest.mark.parametrize('name', ED_CASES)
def test_embed_dropout_backward(dev, name):
    """|got - ref| <= (k + 2) 2^-24 sum|terms| per element, k = the positions that hold the row's id: the first-order
    bound of k f32 multiply-adds.  dW starts from zero (zero_grad has cleared it)."""
    ids, ntoken, ninput, keep, p = _ed_case(name)
    N = len(ids)
    rng = np.random.RandomState(N + ninput + 1)
    dout = rng.randn(N, ninput).astype(np.float32)
    scale = float(1.0 / (1.0 - p))
    dW0 = np.zeros((ntoken, ninput), dtype=np.float32)
    a = _run_bwd(dev, ids, ntoken, ninput, keep, scale, dout, dW0)
    b = _run_bwd(dev, ids, ntoken, ninput, keep, scale, dout, dW0)
    assert torch.equal(a, b)
    host = a.cpu().numpy()
    assert (host[:GUARD] == -7.5).all() and (host[-GUARD:] == -7.5).all()
    got = host[GUARD:-GUARD].reshape(ntoken, ninput).astype(np.float64)
    ref, mag, count = R.embed_dropout_bwd(ids, keep, np.float32(scale), dout, ntoken)
    err, bound = np.abs(got - ref), (count[:, None] + 2) * EPS24 * mag
    print('%s: worst error / bound %.3g' % (name, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all()
    assert not got[count == 0].any()                       # rows nobody holds stay as they were
    if name == 'one_id':
        assert count[6] == N
    if name == 'all_drop':
        assert not got.any()


def test_embed_dropout_backward_adds_to_the_gradient_and_leaves_other_rows(dev):
    """dW += : on a gradient that already holds values (one more term of the sum: |dW0| joins sum|terms|); the rows
    of ids nobody holds -- the bad ones have no row at all -- keep their bits"""
    ids, ntoken, ninput, keep, p = _ed_case('bad_ids')
    ids = np.where(ids == 4, 3, ids)                       # nobody holds row 4
    rng = np.random.RandomState(9)
    dout = rng.randn(len(ids), ninput).astype(np.float32)
    dW0 = rng.randn(ntoken, ninput).astype(np.float32)
    scale = float(1.0 / (1.0 - p))
    host = _run_bwd(dev, ids, ntoken, ninput, keep, scale, dout, dW0).cpu().numpy()
    assert (host[:GUARD] == -7.5).all() and (host[-GUARD:] == -7.5).all()
    got = host[GUARD:-GUARD].reshape(ntoken, ninput)
    ref, mag, count = R.embed_dropout_bwd(ids, keep, np.float32(scale), dout, ntoken, dW0)
    assert count[4] == 0 and np.array_equal(got[4].view(np.uint32), dW0[4].view(np.uint32))
    assert (np.abs(got - ref) <= (count[:, None] + 2) * EPS24 * mag).all()


def test_embed_dropout_refuses_bad_shapes(dev):
    t = torch.zeros(64, dtype=torch.float32, device=dev)
    i = torch.zeros(8, dtype=torch.int64, device=dev)
    k = torch.zeros(64, dtype=torch.uint8, device=dev)
    P = lambda x: x.data_ptr()
    lib = _lib()
    assert lib.sba_embed_dropout_fwd(P(i), P(t), P(k), 1.0, P(t), 2, 4, 6, _st()) == -1        # ninput % 4
    assert lib.sba_embed_dropout_fwd(P(i), P(t), P(k), 1.0, P(t), 8193, 4, 4, _st()) == -1     # more ids than the LDS table
    assert lib.sba_embed_dropout_fwd(None, P(t), P(k), 1.0, P(t), 2, 4, 4, _st()) == -1
    assert lib.sba_embed_dropout_bwd(P(i), P(k), 1.0, P(t), P(t) + 4, 2, 4, 4, _st()) == -1    # dW not 16-byte aligned
    assert lib.sba_embed_dropout_bwd(P(i), P(k), 1.0, P(t), P(t), 0, 4, 4, _st()) == -1
    torch.cuda.synchronize()


def test_embed_dropout_fn_autograd(dev):
    """ops.EmbedDropoutFn: the backward adds into weight.grad (a view of a flat buffer) and returns nothing for it"""
    from sbagan import ops
    rng = np.random.RandomState(4)
    B, T, ntoken, ninput = 3, 5, 9, 8
    caps = torch.from_numpy(rng.randint(0, ntoken, (B, T)).astype(np.int64)).to(dev)
    keep = torch.from_numpy((rng.rand(B, T, ninput) >= 0.5).astype(np.uint8)).to(dev)
    Wn = rng.randn(ntoken, ninput).astype(np.float32)
    flat_grad = torch.zeros(ntoken * ninput + 8, dtype=torch.float32, device=dev)
    W = torch.nn.Parameter(torch.from_numpy(Wn).to(dev))
    W.grad = flat_grad[:ntoken * ninput].view(ntoken, ninput)
    out = ops.EmbedDropoutFn.apply(caps, W, keep, 2.0)
    g = torch.from_numpy(rng.randn(B, T, ninput).astype(np.float32)).to(dev)
    (out * g).sum().backward()
    torch.cuda.synchronize()
    assert W.grad.data_ptr() == flat_grad.data_ptr()
    ref, mag, count = R.embed_dropout_bwd(caps.cpu().numpy().reshape(-1), keep.cpu().numpy().reshape(-1, ninput), 2.0,
                                          g.cpu().numpy().reshape(-1, ninput), ntoken)
    assert (np.abs(W.grad.cpu().numpy() - ref) <= (count[:, None] + 2) * EPS24 * mag).all()
    assert not flat_grad[ntoken * ninput:].any()


# ---------------------------------------------------------------------------------------------------------------
# gradient norm, clip coefficient, Adam's bias corrections from a device-side learning rate
# ---------------------------------------------------------------------------------------------------------------
MAX_NORM, NPARTS = 0.25, 64


def _norm_run(dev, g, lr, state=None, offset=0, nparts=NPARTS):
    """(norm, coef, partials, state) of one sba_sqnorm_partials + sba_clip_adam_prepare; offset: floats by which the
    range starts off a 16-byte boundary"""
    n = len(g)
    buf = torch.zeros(n + 8, dtype=torch.float32, device=dev)
    buf[offset:offset + n].copy_(torch.from_numpy(g))
    partials = torch.full((nparts + 2,), -3.0, dtype=torch.float64, device=dev)
    out = torch.full((4,), -3.0, dtype=torch.float32, device=dev)
    state = torch.zeros(4, dtype=torch.int32, device=dev) if state is None else state
    lr_dev = torch.tensor([lr], dtype=torch.float32, device=dev)
    lib = _lib()
    assert lib.sba_sqnorm_partials(buf.data_ptr() + 4 * offset, n, partials.data_ptr() + 8, nparts, _st()) == 0
    assert lib.sba_clip_adam_prepare(state.data_ptr(), partials.data_ptr() + 8, nparts, lr_dev.data_ptr(), MAX_NORM,
                                     0.5, 0.999, out.data_ptr() + 4, _st()) == 0
    torch.cuda.synchronize()
    assert float(partials[0]) == -3.0 and float(partials[-1]) == -3.0 and float(out[0]) == -3.0 and float(out[3]) == -3.0
    return out[1:3].cpu().numpy(), partials[1:-1].cpu().numpy(), state


@pytest.mark.parametrize('kind', ['zeros', 'below', 'above'])
@pytest.mark.parametrize('n', [1, 3, 255, 256, 257, 100003])
def test_norm_and_coef(dev, n, kind):
    rng = np.random.RandomState(n)
    g = rng.randn(n)
    target = {'zeros': 0.0, 'below': 0.1, 'above': 3.0}[kind]
    g = (g / np.sqrt((g * g).sum()) * target).astype(np.float32)
    norm, coef = R.norm_and_coef(g, MAX_NORM)
    (got, parts, _), (got2, parts2, _) = _norm_run(dev, g, 1e-3), _norm_run(dev, g, 1e-3)
    assert np.array_equal(got.view(np.uint32), got2.view(np.uint32)) and np.array_equal(parts, parts2)      # bit-equal
    print('n %d %s: norm %.9g (ref %.9g) coef %.9g (ref %.9g)' % (n, kind, got[0], norm, got[1], coef))
    if kind == 'zeros':
        assert got[0] == 0.0 and got[1] == 1.0
        return
    assert abs(float(got[0]) - norm) <= EPS22 * norm
    assert abs(float(got[1]) - coef) <= EPS22 * coef
    assert (coef == 1.0) == (kind == 'below') and (float(got[1]) == 1.0) == (kind == 'below')


def test_norm_of_a_range_off_the_16_byte_grid_and_other_part_counts(dev):
    g = (np.random.RandomState(2).randn(1001) * 0.05).astype(np.float32)
    norm, coef = R.norm_and_coef(g, MAX_NORM)
    for offset, nparts in ((1, NPARTS), (3, 1), (0, 1024), (2, 7)):
        got, _, _ = _norm_run(dev, g, 1e-3, offset=offset, nparts=nparts)
        assert abs(float(got[0]) - norm) <= EPS22 * norm and abs(float(got[1]) - coef) <= EPS22 * coef
    buf = torch.zeros(8, dtype=torch.float32, device=dev)
    part = torch.zeros(2, dtype=torch.float64, device=dev)
    assert _lib().sba_sqnorm_partials(buf.data_ptr(), 8, part.data_ptr(), 1025, _st()) == -1
    assert _lib().sba_sqnorm_partials(buf.data_ptr(), 0, part.data_ptr(), 1, _st()) == -1


def test_prepare_reads_the_learning_rate_from_the_device(dev):
    """step_size = lr / (1 - beta1^t) for t = 1, 2 with lr changed between the calls; one f32 rounding of a double"""
    g = np.ones(5, dtype=np.float32)
    lr1, lr2 = 2e-3, 2e-3 * 0.98
    _, _, state = _norm_run(dev, g, lr1)
    s1 = state.clone()
    _, _, state = _norm_run(dev, g, lr2, state=state)
    for t, lr, s in ((1, lr1, s1), (2, lr2, state)):
        assert int(s[0]) == t
        f = s.view(torch.float32).cpu().numpy().astype(np.float64)
        want = R.adam_step_size(float(np.float32(lr)), 0.5, t)
        assert abs(f[1] - want) <= 2.0 ** -23 * want, (t, f[1], want)
        bc2 = 1.0 / np.sqrt(1.0 - float(np.float32(0.999)) ** t)
        assert abs(f[2] - bc2) <= 1e-6 * bc2


@pytest.mark.parametrize('ema', [False, True])
@pytest.mark.parametrize('n', [3, 1003, 70000])
def test_adam_step_dscale_is_adam_step(dev, n, ema):
    """null scale == sba_adam_step(grad_scale = 1); a device 0.25 == sba_adam_step on the gradient times 0.25 in f32"""
    lib = _lib()
    rng = np.random.RandomState(n)
    mk = lambda s=1.0: torch.from_numpy((rng.randn(n + 4) * s).astype(np.float32)).to(dev)
    p0, g0, m0, v0, a0 = mk(), mk(0.1), mk(0.01), mk(0.01).abs(), mk()
    state = torch.zeros(4, dtype=torch.int32, device=dev)
    assert lib.sba_adam_prepare(state.data_ptr(), 2e-3, 0.5, 0.999, _st()) == 0
    quarter = torch.tensor([0.25], dtype=torch.float32, device=dev)

    def run(entry, g, scale):
        t = [x.clone() for x in (p0, m0, v0, a0)]
        rc = entry(t[0].data_ptr(), g.data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr() if ema else None,
                   None, state.data_ptr(), n, 0.5, 0.999, 1e-8, scale, _st())
        assert rc == 0
        torch.cuda.synchronize()
        return t

    for scale_dev, g_host, what in ((None, g0, 'null'), (quarter.data_ptr(), g0 * 0.25, '0.25')):
        a = run(lib.sba_adam_step_dscale, g0, scale_dev)
        b = run(lib.sba_adam_step, g_host, 1.0)
        for x, y, name in zip(a, b, 'pmva'):
            assert torch.equal(x, y), (what, name)
            assert torch.equal(x[n:], (p0, m0, v0, a0)['pmva'.index(name)][n:])       # nothing past n
        assert not torch.equal(a[0], p0) and (ema or torch.equal(a[3], a0))


# ---------------------------------------------------------------------------------------------------------------
# the slot step against DAMSMStep.step (the shapes of test_damsm_update_vs_oracle)
# ---------------------------------------------------------------------------------------------------------------
def test_slot_step_vs_damsm_step(dev):
    import model
    from miscc.config import cfg, reset_cfg
    from oracle import fill
    from sbagan import ops
    from sbagan.damsm import DAMSMSlotStep, DAMSMStep
    reset_cfg()
    B, T, lr = 6, 12, 2e-3
    cfg.TEXT.EMBEDDING_DIM, cfg.TRAIN.RNN_GRAD_CLIP, cfg.TEXT.WORDS_NUM = 256, 0.25, T
    s = cfg.TRAIN.SMOOTH
    s.GAMMA1, s.GAMMA2, s.GAMMA3 = 4.0, 5.0, 10.0
    ops.set_compute_dtype(torch.float32)
    ops.set_deterministic(True)
    try:
        torch.manual_seed(5)
        text = model.RNN_ENCODER(200, ninput=300, drop_prob=0.0, nhidden=256)
        enc = model.CNN_ENCODER(256)
        with torch.no_grad():
            for m in enc.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.weight.uniform_(0.5, 1.5)
                    m.bias.uniform_(-0.2, 0.2)
                    m.running_mean.uniform_(-0.1, 0.1)
                    m.running_var.uniform_(0.8, 1.2)
        text2, enc2 = copy.deepcopy(text), copy.deepcopy(enc)
        caps, lens = fill.synthetic_captions(B, words_num=T, lmax=T - 2, vocab=200, tag=31)
        class_ids = np.array([0, 1, 2, 0, 3, 4])
        img = fill.uniform((B, 3, 128, 128), 32).to(dev)
        text.to(dev).train(), enc.to(dev).train()
        a = DAMSMStep(text, enc, B, lr=lr)
        out = a.step(img, caps.to(dev), lens.to(dev), class_ids)
        torch.cuda.synchronize()
        text2.to(dev).train(), enc2.to(dev).train()
        b = DAMSMSlotStep(text2, enc2, B, 128, lr=lr, eager=True)
        assert b.text_hi == sum((p.numel() + 3) // 4 * 4 for p in text2.parameters()) and 0 < b.text_hi < b.flat.n
        b.load([[img], caps, lens, class_ids, None])
        b.train()
        torch.cuda.synchronize()
        assert b.recording is None
        for k, name in enumerate(('w_loss0', 'w_loss1', 's_loss0', 's_loss1')):
            assert torch.equal(b.last[k], out[name]), (name, float(b.last[k]), float(out[name]))
        na, nb = float(out['rnn_grad_norm']), float(b.out[0])
        print('rnn_grad_norm: step %.9g, slot step %.9g; coef %.9g' % (na, nb, float(b.out[1])))
        assert abs(na - nb) <= 1e-5 * na
        assert abs(float(b.out[1]) - min(1.0, 0.25 / (nb + 1e-6))) <= 1e-6
        pa = dict(a.trainable.named_parameters())
        for n, p in b.trainable.named_parameters():
            err = (p.detach().double() - pa[n].detach().double()).abs()
            share, worst = float((err > 0.05 * lr).double().mean()), float(err.max())
            print('%-40s share off by > 0.05 lr: %.3g, max error / lr: %.3g' % (n, share, worst / lr))
            assert share <= 2e-2 and worst <= 2.05 * lr, n
        # .grad keeps the UNCLIPPED gradient (the clip is folded into Adam); DAMSMStep scaled it in place
        ga = torch.cat([p.grad.reshape(-1) for p in a._rnn_params]).double()
        gb = torch.cat([p.grad.reshape(-1) for p in b.base._rnn_params]).double()
        assert float((gb * float(b.out[1]) - ga).norm()) <= 1e-4 * float(ga.norm())
        bufs = dict(enc.named_buffers())
        for n, t in enc2.named_buffers():
            assert torch.equal(t, bufs[n]), n
        m = b.read_losses()
        assert m['batches'] == 1 and m['w_loss0'] == float(out['w_loss0']) and float(b.acc.abs().sum()) == 0.0
    finally:
        ops.set_deterministic(False)
        reset_cfg()


# ---------------------------------------------------------------------------------------------------------------
# the replayed loop against the eager loop over the same slot, through pretrain_DAMSM.main
# ---------------------------------------------------------------------------------------------------------------
WORDS = ['bird', 'red', 'small', 'wing', 'blue', 'beak', 'long', 'white', 'yellow', 'belly', 'tail', 'black']
LENGTHS = [(8, 8), (3, 5), (4, 4), (6, 3), (5, 7), (8, 7), (3, 3), (4, 6)]
CLASSES = [1, 1, 1, 1, 2, 2, 2, 2]
B, WORDS_NUM, CROP, LR = 4, 8, 128, 0.002


def make_dataset(root):
    """a CUB-shaped toy data_dir with its own class_info.pickle: 8 training images in 2 classes"""
    from PIL import Image
    rng = np.random.RandomState(0)
    for sub in ('images/cls', 'text/cls', 'train', 'test'):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    names = {'train': ['cls/a%d' % i for i in range(8)], 'test': ['cls/t0', 'cls/t1']}
    lengths = {'train': LENGTHS, 'test': [(4, 5), (3, 6)]}
    classes = {'train': CLASSES, 'test': [1, 2]}
    for split, keys in names.items():
        with open(os.path.join(root, split, 'filenames.pickle'), 'wb') as f:
            pickle.dump(keys, f)
        with open(os.path.join(root, split, 'class_info.pickle'), 'wb') as f:
            pickle.dump(classes[split], f)
        for k, lens in zip(keys, lengths[split]):
            Image.fromarray(rng.randint(0, 255, (90, 110, 3)).astype(np.uint8)).save(
                os.path.join(root, 'images', k + '.jpg'))
            with open(os.path.join(root, 'text', k + '.txt'), 'w') as f:
                for n in lens:
                    f.write(' '.join(WORDS[rng.randint(0, len(WORDS))] for _ in range(n)) + '\n')
    return root


@pytest.fixture(scope='module')
def toy(tmp_path_factory):
    root = make_dataset(str(tmp_path_factory.mktemp('damsm_replay') / 'toy'))
    return {'root': root, 'tmp': tmp_path_factory, 'runs': {}}


def _yml(path, root, epochs):
    import yaml
    with open(path, 'w') as f:
        f.write(yaml.safe_dump({
            'CONFIG_NAME': 'DAMSM', 'DATASET_NAME': 'toy', 'DATA_DIR': root, 'GPU_ID': 0, 'WORKERS': 0,
            'TREE': {'BRANCH_NUM': 1, 'BASE_SIZE': CROP},
            'TRAIN': {'FLAG': True, 'NET_E': '', 'BATCH_SIZE': B, 'MAX_EPOCH': epochs, 'SNAPSHOT_INTERVAL': 1,
                      'ENCODER_LR': LR, 'RNN_GRAD_CLIP': 0.25,
                      'SMOOTH': {'GAMMA1': 4.0, 'GAMMA2': 5.0, 'GAMMA3': 10.0}},
            'TEXT': {'EMBEDDING_DIM': 256, 'CAPTIONS_PER_IMAGE': 2, 'WORDS_NUM': WORDS_NUM}}))
    return path


def _interval_lines(text):
    """the interval lines without their timing"""
    return [re.sub(r'ms/batch\s*[0-9.]+', 'ms/batch', l) for l in text.splitlines() if l.startswith('| epoch')]


def run_main(toy, capsys, monkeypatch, dtype, eager, device_data=True, epochs=2, seed=3):
    """one pretrain_DAMSM.main --replay run from one seed (cached): checkpoints, final training state, what every batch
    left in the step's static tensors, the interval lines"""
    key = (str(dtype), bool(eager), device_data, epochs, seed)
    if key in toy['runs']:
        return toy['runs'][key]
    import pretrain_DAMSM
    from miscc.config import reset_cfg
    from sbagan import ops
    from sbagan.damsm import DAMSMSlotStep
    reset_cfg()
    ops.set_compute_dtype(dtype)
    work = toy['tmp'].mktemp('run')
    (work / 'cwd').mkdir()
    monkeypatch.chdir(work / 'cwd')                 # the entry point writes to ../output/<name>
    yml = _yml(str(work / 'toy.yml'), toy['root'], epochs)
    log = {'keep': [], 'class_mask': [], 'delta': [], 'state': [], 'lr': [], 'out': [], 'last': []}

    def make(*a, **kw):
        st = DAMSMSlotStep(*a, eager=eager, **kw)
        inner = st.train

        def train():
            before = st.flat.data.clone()
            inner()
            log['keep'].append(st.keep.clone())
            log['class_mask'].append(st.slot.class_mask.tensor.clone())
            log['delta'].append(st.flat.data - before)
            log['state'].append(st.opt.state.clone())
            log['lr'].append(st.lr_dev.clone())
            log['out'].append(st.out.clone())
            log['last'].append(st.last.clone())
        st.train = train
        log['step'] = st
        return st

    capsys.readouterr()
    argv = ['--cfg', yml, '--gpu', '0', '--manualSeed', str(seed), '--replay'] + \
        (['--device_data', '--device_data_gb', '1'] if device_data else [])
    model_dir = pretrain_DAMSM.main(argv, make_step=make)
    torch.cuda.synchronize()
    text = capsys.readouterr().out
    st = log.pop('step')
    res = {k: [t.cpu() for t in v] for k, v in log.items()}
    res.update(files={os.path.basename(p): torch.load(p, map_location='cpu')
                      for p in sorted(glob.glob(os.path.join(model_dir, '*.pth')))},
               param=st.flat.data.cpu(), m=st.flat.m.cpu(), v=st.flat.v.cpu(), grad=st.flat.grad.cpu(),
               recorded=st.recording is not None, launched=st.launched, batches=st.batches, info=st.info,
               lines=_interval_lines(text), text=text)
    reset_cfg()
    toy['runs'][key] = res
    return res


@pytest.fixture()
def det():
    from sbagan import ops
    ops.set_deterministic(True)
    yield
    ops.set_deterministic(False)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_replayed_pretraining_is_the_eager_pretraining(toy, det, capsys, monkeypatch, dtype):
    """2 epochs of 2 batches (B = 4, drop_prob 0.5), the learning rate decayed between them, a checkpoint after each:
    once through the recording, once with eager=True, from one seed"""
    a = run_main(toy, capsys, monkeypatch, dtype, eager=False)
    b = run_main(toy, capsys, monkeypatch, dtype, eager=True)
    # the recording exists and was launched; the eager run has none
    assert a['recorded'], [l for l in a['text'].splitlines() if '--replay' in l]
    assert a['batches'] == 4 and a['launched'] == 3, (a['batches'], a['launched'])
    assert not b['recorded'] and b['batches'] == 4 and b['launched'] == 0 and b['info'] is None
    info = a['info']
    print('recording:', info)
    assert info['nodes'] > 0 and info['kernels'] > 0 and info['host_calls'] == 0 and info['copies'] >= 0
    assert info['kernels'] + info['copies'] + info['memsets'] <= info['nodes']
    assert 'could not be recorded' not in a['text']
    # checkpoints and training state
    want = {'text_encoder0.pth', 'text_encoder1.pth', 'image_encoder0.pth', 'image_encoder1.pth'}
    assert set(a['files']) == want == set(b['files'])
    for name in sorted(want):
        sa, sb = a['files'][name], b['files'][name]
        assert sorted(sa) == sorted(sb)
        bad = [k for k in sa if not torch.equal(sa[k], sb[k])]
        assert not bad, (name, bad[:5], len(bad))
        assert all(bool(torch.isfinite(v).all()) for v in sa.values() if v.is_floating_point())
    for k in ('param', 'm', 'v', 'grad'):
        assert torch.equal(a[k], b[k]), k
    assert float(a['m'].abs().sum()) > 0 and bool(torch.isfinite(a['param']).all())
    # the batches differ: dropout masks drawn per batch, class masks made per batch from the slot's ids
    keep, cm = a['keep'], a['class_mask']
    assert all(not torch.equal(keep[i], keep[i + 1]) for i in range(3))
    assert all(0.3 < float(k.float().mean()) < 0.7 and int(k.max()) == 1 for k in keep)
    assert any(not torch.equal(cm[i], cm[j]) for i in range(4) for j in range(i))
    for i in range(4):
        assert torch.equal(keep[i], b['keep'][i]) and torch.equal(cm[i], b['class_mask'][i])
    # the second epoch's first update (batch 2) ran with the second learning rate, from restarted moments
    lr2 = np.float32(LR * 0.98)
    assert float(a['lr'][1]) == float(np.float32(LR)) and float(a['lr'][2]) == float(lr2)
    for i, t in enumerate((1, 2, 1, 2)):
        assert int(a['state'][i][0]) == t and torch.equal(a['state'][i], b['state'][i])
    step_size = float(a['state'][2].view(torch.float32)[1])
    assert abs(step_size - float(lr2) / 0.5) <= 2.0 ** -23 * float(lr2) / 0.5
    for i in range(4):
        assert torch.equal(a['delta'][i], b['delta'][i]), i
        assert float(a['delta'][i].abs().max()) > 0
    # Adam's first step from zero moments moves a parameter by lr (g / (|g| + eps)): the largest moves of batch 0 and
    # batch 2 are in the ratio of the two rates
    r = float(a['delta'][2].abs().max()) / float(a['delta'][0].abs().max())
    assert abs(r - 0.98) <= 1e-3, r
    # the interval lines: one per epoch (UPDATE_INTERVAL = 50), means over the batches since the last one
    assert len(a['lines']) == 2 and a['lines'] == b['lines']


def test_replay_from_the_torch_loader(toy, det, capsys, monkeypatch):
    """--replay without --device_data: the batches of the torch DataLoader go into the slot with slot.load"""
    r = run_main(toy, capsys, monkeypatch, torch.bfloat16, eager=False, device_data=False, epochs=1, seed=5)
    assert r['recorded'] and r['batches'] == 2 and r['launched'] == 1
    for i in range(2):
        print('batch %d: (norm, coef) %s losses %s class mask %s' % (
            i, r['out'][i].tolist(), r['last'][i].tolist(), r['class_mask'][i].tolist()))
        # a condition on the INPUT: the shuffled batch is not one class alone (every other row masked: all losses 0)
        assert int(r['class_mask'][i].sum()) < B * (B - 1), 'choose another seed: batch %d is one class' % i
        assert float(r['out'][i][0]) > 0 and float(r['last'][i][:4].min()) > 0
    assert set(r['files']) == {'text_encoder0.pth', 'image_encoder0.pth'}
    assert bool(torch.isfinite(r['param']).all()) and float(r['delta'][1].abs().max()) > 0
    assert len(r['lines']) == 1


def test_fallback_when_the_update_cannot_be_recorded(toy, det, capsys, monkeypatch):
    """a Python exception while the recording is constructed: one line, and the same run with eager updates"""
    import sbagan._lib as L

    real = L.lib

    class Refusing(object):
        def __getattr__(self, name):
            if name == 'sba_replay_create':
                return lambda *a: -3
            return getattr(real, name)
    monkeypatch.setattr(L, 'lib', Refusing())
    r = run_main(toy, capsys, monkeypatch, torch.float32, eager=False, epochs=1)
    del toy['runs'][(str(torch.float32), False, True, 1, 3)]
    assert r['text'].count('--replay: the DAMSM update could not be recorded') == 1
    assert not r['recorded'] and r['launched'] == 0 and r['batches'] == 2
    monkeypatch.undo()
    e = run_main(toy, capsys, monkeypatch, torch.float32, eager=True, epochs=1)
    assert torch.equal(r['param'], e['param']) and torch.equal(r['m'], e['m'])


def test_bert_entry_point_ignores_the_flag(tmp_path, capsys, monkeypatch):
    """pretrain_DAMSM_bert.main --replay: one line, and the run of one step matches the run without the flag"""
    import yaml
    import pretrain_DAMSM_bert
    from miscc.config import reset_cfg
    from sbagan import ops
    from test_bert_entry_gpu import _bert_dir
    from test_host_cpu import _make_dataset
    root = str(tmp_path / 'toy')
    _make_dataset(root, n_train=4, n_test=4)
    bert_dir = _bert_dir(tmp_path)
    yml = tmp_path / 'damsm_bert_toy.yml'
    yml.write_text(yaml.safe_dump({
        'CONFIG_NAME': 'DAMSM', 'DATASET_NAME': 'toy', 'DATA_DIR': root, 'GPU_ID': 0, 'WORKERS': 0,
        'TREE': {'BRANCH_NUM': 1, 'BASE_SIZE': 128},
        'TRAIN': {'FLAG': True, 'NET_E': '', 'BATCH_SIZE': 4, 'MAX_EPOCH': 1, 'SNAPSHOT_INTERVAL': 1,
                  'ENCODER_LR': 0.002, 'RNN_GRAD_CLIP': 0.25,
                  'SMOOTH': {'GAMMA1': 4.0, 'GAMMA2': 5.0, 'GAMMA3': 10.0}},
        'TEXT': {'EMBEDDING_DIM': 256, 'CAPTIONS_PER_IMAGE': 2, 'WORDS_NUM': 8}}))
    ops.set_deterministic(True)
    try:
        files = []
        for k, flag in enumerate((['--replay'], [])):
            reset_cfg()
            ops.set_compute_dtype(torch.bfloat16)
            cwd = tmp_path / ('cwd%d' % k) / 'run'
            cwd.mkdir(parents=True)
            monkeypatch.chdir(cwd)
            capsys.readouterr()
            model_dir = pretrain_DAMSM_bert.main(['--cfg', str(yml), '--gpu', '0', '--manualSeed', '7', '--bert_dir',
                                                  bert_dir] + flag, max_steps=1)
            text = capsys.readouterr().out
            assert text.count('--replay is ignored') == (1 if flag else 0)
            files.append({os.path.basename(p): torch.load(p, map_location='cpu')
                          for p in glob.glob(os.path.join(model_dir, '*.pth'))})
        assert set(files[0]) == {'text_encoder0.pth', 'image_encoder0.pth'} == set(files[1])
        for name in files[0]:
            bad = [k for k in files[0][name] if not torch.equal(files[0][name][k], files[1][name][k])]
            assert not bad, (name, bad[:5])
    finally:
        ops.set_deterministic(False)
        reset_cfg()
