"""Attention-map overlays on the GPU: ops.vis_expand / ops.vis_compose and the two builders of sbagan/visualize.py against
the float64 reference of tests/vis_ref.py (scipy expand, PIL blend, numpy layout), the kernels' edge behaviour, the
wrappers' refusals, the C ABI's, and the flag end to end through both trainers and one pre-training step."""
import functools
import glob
import os

import numpy as np
import pytest
import torch
from PIL import Image

import sampling_harness as sh
import vis_ref

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'

# (n, a, V)
EXPAND_CASES = [(1, 1, 16), (3, 3, 6), (4, 5, 20),
                (19, 17, 272),        # the DAMSM shape: V is not a multiple of 64
                (5, 64, 128), (3, 64, 256),
                (3, 128, 256),        # the LDS-tiling case: the widest map the kernel takes
                (2, 64, 64)]          # up = 1: the maps themselves


@functools.lru_cache(maxsize=None)
def _expand_case(case, with_thresh):
    """inputs and float64 reference, computed once per case: attention-like maps (non-negative, rows sum to 1)"""
    n, a, V = case
    rng = np.random.RandomState(n * 1000 + a)
    x = rng.rand(n, a, a).astype(np.float32) ** 4
    x /= x.reshape(n, -1).sum(1).reshape(n, 1, 1)
    x = x.astype(np.float32)
    thresh = (np.float32(1.0 / (a * a)) * (0.5 + rng.rand(n))).astype(np.float32) if with_thresh else None
    x64 = x.astype(np.float64)
    if with_thresh:
        t64 = thresh.astype(np.float64).reshape(n, 1, 1)
        cut = x64 * (x64 > t64)
        conf = np.array([x64[i][x64[i] > 2 * t64[i, 0, 0]].sum() for i in range(n)])
    else:
        cut, conf = x64, x64.reshape(n, -1).sum(1)
    ref = np.stack([vis_ref.expand(c, V // a) for c in cut])
    return x, thresh, ref, conf


@pytest.mark.parametrize('with_thresh', [False, True], ids=['plain', 'thresh'])
@pytest.mark.parametrize('case', EXPAND_CASES, ids=lambda c: 'n%d-a%d-V%d' % c)
def test_expand_vs_float64(case, with_thresh):
    """Bound (vis_ref.expand_tol): the kernel sums a terms per pass in sequential f32 FMAs with non-negative weights that
    sum to 1 -- a u max|x| per pass, two passes -- on operator entries rounded once to f32 (2 u) and rounds the results
    (2 u): (2 a + 4) 2^-24 max|x|; 0 for up = 1.  min / max: the same bound.  conf: a^2 2^-24 sum|x| (vis_ref.conf_tol)."""
    from sbagan import ops
    from sbagan.visualize import _device_operator
    n, a, V = case
    x, thresh, ref, conf = _expand_case(case, with_thresh)
    xd = torch.from_numpy(x).to(DEV)
    td = torch.from_numpy(thresh).to(DEV) if with_thresh else None
    out, stats = ops.vis_expand(xd, _device_operator(a, V, DEV), td)
    assert out.shape == (n, V, V) and stats.shape == (3, n)
    out, stats = out.cpu().numpy().astype(np.float64), stats.cpu().numpy().astype(np.float64)
    tol = vis_ref.expand_tol(a, V // a, np.abs(x).max())
    err = np.abs(out - ref).max()
    emin = np.abs(stats[0] - ref.reshape(n, -1).min(1)).max()
    emax = np.abs(stats[1] - ref.reshape(n, -1).max(1)).max()
    ctol = vis_ref.conf_tol(a, np.abs(x.astype(np.float64)).reshape(n, -1).sum(1).max())
    econf = np.abs(stats[2] - conf).max()
    print('case %s thresh %s: err %.3e min %.3e max %.3e (tol %.3e)  conf %.3e (tol %.3e)'
          % (case, with_thresh, err, emin, emax, tol, econf, ctol))
    assert err <= tol and emin <= tol and emax <= tol
    assert econf <= ctol


def test_expand_twice_is_bit_identical():
    from sbagan import ops
    from sbagan.visualize import _device_operator
    x, thresh, _, _ = _expand_case((19, 17, 272), True)
    xd, td, M = torch.from_numpy(x).to(DEV), torch.from_numpy(thresh).to(DEV), _device_operator(17, 272, DEV)
    o1, s1 = ops.vis_expand(xd, M, td)
    o2, s2 = ops.vis_expand(xd, M, td)
    assert torch.equal(o1, o2) and torch.equal(s1, s2)


# ------------------------------------------------------------------ compose
IXTOWORD = {i: w for i, w in enumerate(['<end>', 'bird', 'with', 'red', 'wings', 'and', 'a', 'long', 'yellow', 'beak',
                                         'café'])}


def _attention_like(rng, T, a):
    x = rng.rand(T, a, a).astype(np.float32) ** 6
    return (x / x.reshape(T, -1).sum(1).reshape(T, 1, 1)).astype(np.float32)


def _grid_inputs(B, a, S, lens, lr_size, seed):
    rng = np.random.RandomState(seed)
    imgs = (rng.rand(B, 3, S, S) * 2.4 - 1.2).astype(np.float32)           # (some values clamp at both ends)
    lr = (rng.rand(B, 3, lr_size, lr_size) * 2 - 1).astype(np.float32) if lr_size else None
    maps = [_attention_like(rng, T, a) for T in lens]
    caps = np.zeros((B, 8), dtype=np.int64)
    for i, T in enumerate(lens):
        caps[i, :T] = rng.randint(1, len(IXTOWORD), size=T)
    return imgs, lr, maps, caps


@pytest.mark.parametrize('lr_size', [0, 8], ids=['no-lr', 'lr'])
def test_grid_vs_reference_canvas(lr_size):
    """a = 17 (V = 272), B = 3 < 8, T_i < WORDS_NUM (black slots), with and without lr_imgs.  Every byte outside the
    text equals the reference's unless the float64 value is within delta of an integer (vis_ref.check_canvas)."""
    from miscc.config import cfg, reset_cfg
    from sbagan.visualize import build_super_images, word_colours
    reset_cfg()
    cfg.TEXT.WORDS_NUM = 6
    lens = [4, 6, 1]
    imgs, lr, maps, caps = _grid_inputs(3, 17, 16, lens, lr_size, 3)
    got, sentences = build_super_images(torch.from_numpy(imgs).to(DEV), caps, IXTOWORD,
                                        [torch.from_numpy(m).to(DEV) for m in maps], 17,
                                        lr_imgs=None if lr is None else torch.from_numpy(lr).to(DEV))
    ref = vis_ref.grid(imgs, maps, 17, 6, word_colours(20)[:6], lr_imgs=lr)
    assert got.shape == (3 * (50 + 2 * 272), 8 * 274, 3)
    Hs = 50 + 2 * 272
    used = vis_ref.check_canvas(got, ref, text_rows=[(i * Hs, i * Hs + 50) for i in range(3)])
    print('pixels on a rounding boundary: %d of %d' % (used, got.shape[0] * got.shape[1]))
    # the caption band: columns 0-1 black; word column j is its colour, under the label 'j:word' of the caption's j-th
    # word at the cell's own corner (PIL's rendering of the same string, vis_ref.label_cell) or, past the caption, bare
    for i in range(3):
        band = got[i * Hs:i * Hs + 50]
        assert not band[:, :2 * 274].any()
        for j in range(6):
            cell = band[:, (j + 2) * 274:(j + 3) * 274]
            colour = word_colours(20)[j]
            if j < lens[i]:
                want = vis_ref.label_cell(j, IXTOWORD[int(caps[i, j])], 274, colour)
                assert (want != np.array(colour, dtype=np.uint8)).any()          # (the label is visible)
            else:
                want = np.broadcast_to(np.array(colour, dtype=np.uint8), cell.shape)
            assert np.array_equal(cell, want), (i, j)
    # black slots of the short captions, both rows
    assert not got[50:50 + 544, (2 + 4) * 274:].any() and not got[2 * Hs + 50:, 3 * 274:].any()
    assert [len(s) for s in sentences] == lens and all(w.isascii() for s in sentences for w in s)
    reset_cfg()


@pytest.mark.parametrize('T,a', [(3, 64), (9, 128)], ids=['T3-a64', 'T9-a128'])
def test_topk_vs_reference_canvas(T, a):
    from sbagan.visualize import build_super_images2
    for seed in range(50):
        # the generator's maps: per pixel a softmax over the T words (T = 3: 2 thresh > 1, every conf is an exact 0 tie)
        rng = np.random.RandomState(seed)
        img = (rng.rand(3, 2 * a, 2 * a) * 2 - 1).astype(np.float32)
        logits = 3.0 * rng.randn(T + 2, a, a)
        logits[T:] = -np.inf
        maps = (np.exp(logits) / np.exp(logits).sum(0)).astype(np.float32)
        cap = np.zeros(12, dtype=np.int64)
        cap[:T] = rng.randint(1, len(IXTOWORD), size=T)
        x64 = maps[:T].astype(np.float64)
        th2 = 2 * np.float64(np.float32(2.0 / T))
        conf = np.array([m[m > th2].sum() for m in x64])
        gaps = np.diff(np.sort(conf))
        # the order is decided by the reference alone: exact ties or gaps beyond twice the f32 summation bound
        if (gaps[gaps > 0] > 2 * vis_ref.conf_tol(a, x64.reshape(T, -1).sum(1).max())).all():
            break
    else:
        raise AssertionError('no seed in 0..49 gives a decided order')
    got, words = build_super_images2(torch.from_numpy(img).to(DEV), cap, T, IXTOWORD, torch.from_numpy(maps).to(DEV), a)
    ref, order, conf = vis_ref.topk(img, maps, a, T)
    assert got.shape == (306, min(5, T) * 258, 3) and len(words) == T
    used = vis_ref.check_canvas(got, ref, text_rows=[(0, 50)])
    print('order %s, pixels on a rounding boundary: %d' % (order.tolist(), used))
    assert not got[50:, 256:258].any()
    # the text band: over blend c the label of the word it shows, at the cell's own corner, on black
    for c, j in enumerate(order):
        want = vis_ref.label_cell(int(j), IXTOWORD[int(cap[j])], 258)
        assert want.any() and np.array_equal(got[:50, c * 258:(c + 1) * 258], want), (c, j)


def test_blend_is_bit_exact_for_every_byte_pair():
    """all 256 x 256 (map, image) byte pairs at m = 210 and m = 180 against PIL: maps fed as (r + 0.5) / 255 with
    lo = 0, den = 1, images as (byte + 0.5) / 127.5 - 1.  PIL's paste is also the integer formula of the contract, which
    vis_ref.check_canvas applies to a neighbouring byte."""
    from sbagan import ops
    mv, iv = np.meshgrid(np.arange(256), np.arange(256), indexing='ij')
    E = torch.from_numpy(((mv + 0.5) / 255.0).astype(np.float32)[None]).to(DEV)
    img = ((iv + 0.5) / 127.5 - 1.0).astype(np.float32)
    img3 = torch.from_numpy(np.stack([img, img, img])[None]).to(DEV)
    for m in (210, 180):
        desc = np.array([ops.VIS_BLEND, 0, 0, m], dtype=np.int32).reshape(1, 1, 1, 4)
        par = np.array([0.0, 1.0], dtype=np.float32).reshape(1, 1, 1, 2)
        got = ops.vis_compose(256, 0, desc, par, np.zeros((1, 1), np.uint32), E, img3).cpu().numpy()
        want = vis_ref.pil_blend(mv.astype(np.uint8), np.repeat(iv[:, :, None], 3, 2).astype(np.uint8), m)
        assert got.shape == (256, 258, 3) and np.array_equal(got[:, :256], want) and not got[:, 256:].any()
        t = mv * m + iv * (255 - m) + 128
        assert np.array_equal(want[:, :, 0], ((t >> 8) + t) >> 8)


def test_flat_maps_give_zeros_and_no_nan():
    """gmax = gmin: a sample whose maps are all zero normalises to zero bytes"""
    from miscc.config import cfg, reset_cfg
    from sbagan import ops
    from sbagan.visualize import build_super_images
    reset_cfg()
    cfg.TEXT.WORDS_NUM = 2
    imgs = torch.zeros(1, 3, 16, 16, device=DEV)
    zeros = [torch.zeros(2, 17, 17, device=DEV)]        # gmin = 0 = gmax
    got, _ = build_super_images(imgs, np.array([[1, 2]]), IXTOWORD, zeros, 17)
    assert not got[50:50 + 272, 274:].any()
    out, stats = ops.vis_expand(torch.zeros(2, 5, 5, device=DEV))
    assert not torch.isnan(out).any() and not torch.isnan(stats).any() and not stats.any()
    reset_cfg()


def test_wrappers_refuse_before_any_launch(monkeypatch):
    from sbagan import ops
    launched = []
    monkeypatch.setattr(ops, 'call', lambda *a: launched.append(a))

    def t(*shape):
        return torch.zeros(*shape, device=DEV)
    with pytest.raises(TypeError):
        ops.vis_expand(t(2, 4, 4).double())
    with pytest.raises(ValueError):
        ops.vis_expand(t(2, 4, 5))                                               # not square
    with pytest.raises(ValueError):
        ops.vis_expand(t(2, 129, 129))                                           # a > 128
    with pytest.raises(ValueError):
        ops.vis_expand(t(2, 4, 8)[:, :, ::2])                                    # not contiguous
    with pytest.raises(ValueError):
        ops.vis_expand(t(2, 4, 4), t(8, 5))                                      # M columns != a
    with pytest.raises(ValueError):
        ops.vis_expand(t(2, 4, 4), t(1028, 4))                                   # V > 1024
    with pytest.raises(TypeError):
        ops.vis_expand(t(2, 4, 4), t(8, 4).half())
    with pytest.raises(ValueError):
        ops.vis_expand(t(2, 4, 4), t(8, 4), t(3))                                # thresh rows != n
    desc = np.zeros((1, 1, 2, 4), np.int32)
    par, band = np.zeros((1, 1, 2, 2), np.float32), np.zeros((1, 2), np.uint32)

    def compose(d=desc, p=par, b=band, E=None, i0=None, V=4):
        return ops.vis_compose(V, 50, d, p, b, t(2, 4, 4) if E is None else E, t(1, 3, 8, 8) if i0 is None else i0)
    with pytest.raises(TypeError):
        compose(d=desc.astype(np.int64))
    with pytest.raises(ValueError):
        compose(p=par[:, :, :1])
    with pytest.raises(ValueError):
        compose(E=t(2, 5, 5))                                                    # expanded is not V x V
    with pytest.raises(ValueError):
        compose(i0=t(1, 4, 8, 8))                                                # not 3 channels
    for bad in ((4, 0, 0, 0), (ops.VIS_MAP, 0, 2, 0), (ops.VIS_MAP, 0, -1, 0), (ops.VIS_IMAGE, 1, 0, 0),
                (ops.VIS_IMAGE, 1 << 16, 0, 0), (ops.VIS_BLEND, 0, 0, 256), (ops.VIS_IMAGE, 2 << 16, 0, 0)):
        d = desc.copy()
        d[0, 0, 1] = bad
        with pytest.raises(ValueError):
            compose(d=d)
    assert launched == []


def test_c_abi_rejects_bad_sizes_and_null_pointers():
    from sbagan import _lib
    buf = torch.zeros(4096, device=DEV)
    p, st = buf.data_ptr(), torch.cuda.current_stream().cuda_stream

    def ex(x, M, out, n, a, V):
        return _lib.lib.sba_vis_expand(x, None, M, out, p, p, p, n, a, V, st)
    for args in ((None, p, p, 1, 4, 8), (p, p, None, 1, 4, 8), (p, None, p, 1, 4, 8), (p, p, p, 0, 4, 8),
                 (p, p, p, 1, 0, 8), (p, p, p, 1, 129, 258), (p, p, p, 1, 8, 4), (p, p, p, 1, 4, 1028),
                 (p, p + 4, p, 1, 4, 8)):
        assert ex(*args) == -1, args
    assert _lib.lib.sba_vis_expand(p, None, p, p + 1024, None, p, p, 1, 4, 8, st) == -1
    # a valid call, every array its own region of buf: x 16 floats, M 32, out 64, min / max / conf one each
    assert _lib.lib.sba_vis_expand(p, None, p + 1024, p + 2048, p + 4096, p + 4160, p + 4224, 1, 4, 8, st) == 0

    def co(canvas, W, H, V, band, nS, nr, nc, desc=p, E=p, nE=1, img0=p, n0=1, S0=4):
        return _lib.lib.sba_vis_compose(canvas, W, H, V, band, nS, nr, nc, desc, p, p, E, nE, img0, n0, S0, None, 0, 0, st)
    assert co(None, 6, 9, 4, 5, 1, 1, 1) == -1
    assert co(p, 6, 9, 4, 5, 1, 1, 1, desc=None) == -1
    assert co(p, 7, 9, 4, 5, 1, 1, 1) == -1                # W != nc (V + 2)
    assert co(p, 6, 10, 4, 5, 1, 1, 1) == -1               # H != nS (band + nr V)
    assert co(p, 6, 9, 4, 5, 1, 1, 1, E=None) == -1        # maps counted but no pointer
    assert co(p, 6, 9, 4, 5, 1, 1, 1, img0=None) == -1
    assert co(p, 6, 9, 4, 5, 1, 1, 1, S0=0) == -1
    assert co(p, 0, 5, -2, 5, 1, 1, 1) == -1
    assert co(p + 8192, 6, 9, 4, 5, 1, 1, 1) == 0          # (an all-zero table: one black cell over a black band)
    torch.cuda.synchronize()
    assert not buf[2048:2048 + 6 * 9 * 3 // 4 + 1].any()


# ------------------------------------------------------------------ end to end, on the toy config of test_rprecision_gpu
def _rng_states():
    return np.random.get_state(), torch.cuda.get_rng_state(), torch.get_rng_state()


def _files(root):
    return sorted(os.path.relpath(f, root) for f in glob.glob(os.path.join(root, '**', '*'), recursive=True)
                  if os.path.isfile(f))


def _toy(tmp_path, bert):
    from test_host_cpu import _make_dataset
    sh.toy_cfg()
    from miscc import transforms
    from sbagan import ops
    ops.set_compute_dtype(torch.bfloat16)
    root = str(tmp_path / 'toy')
    _make_dataset(root, n_test=6)
    tf = transforms.Compose([transforms.Resize(int(128 * 76 / 64)), transforms.RandomCrop(128),
                             transforms.RandomHorizontalFlip()])
    if bert:
        import datasets_bert
        from test_bert_entry_gpu import _bert_dir
        bert_dir = _bert_dir(tmp_path)
        ds = datasets_bert.TextDataset(root, 'test', base_size=64, transform=tf, bert_dir=bert_dir)
    else:
        import datasets
        bert_dir = None
        ds = datasets.TextDataset(root, 'test', base_size=64, transform=tf)
    loader = torch.utils.data.DataLoader(ds, batch_size=2, drop_last=True, shuffle=False)
    return ds, loader, bert_dir


def _trainer(tmp_path, name, ds, loader, bert_dir, train_flag):
    from miscc.config import cfg
    cfg.TRAIN.FLAG = train_flag
    out = str(tmp_path / name)
    if bert_dir is None:
        from trainer import condGANTrainer
        return condGANTrainer(out, loader, ds.n_words, ds.ixtoword, allow_random_encoders=True), out
    from trainer_bert import condGANTrainer
    return condGANTrainer(out, loader, ds.n_words, ds.ixtoword, allow_random_encoders=True, bert_dir=bert_dir), out


def test_save_img_results_with_and_without_the_flag(tmp_path):
    from datasets import prepare_data
    from miscc.config import reset_cfg
    from sbagan.trainer import build_mask
    import trainer
    from sbagan import ops
    ds, loader, _ = _toy(tmp_path, bert=False)
    data = prepare_data(next(iter(loader)))
    _, captions, cap_lens = data[0], data[1], data[2]
    written = {}
    ops.set_deterministic(True)          # (two forward passes are bit-identical only in the deterministic mode)
    try:
        _save_img_runs(tmp_path, ds, loader, captions, cap_lens, written, trainer, build_mask)
    finally:
        ops.set_deterministic(False)
    assert sorted(written['on']) == ['Image/D_average_3.png', 'Image/G_average_3_0.png']
    assert Image.open(str(tmp_path / 'on' / 'Image' / 'G_average_3_0.png')).size == (1300, 612)
    assert Image.open(str(tmp_path / 'on' / 'Image' / 'D_average_3.png')).size == (2740, 1188)
    # without the flag: today's plain grids (one per scale, the samples side by side), byte-identical between runs
    assert sorted(written['off']) == ['Image/G_average_3_0.png', 'Image/G_average_3_1.png']
    assert written['off'] == written['off2']
    reset_cfg()


def _save_img_runs(tmp_path, ds, loader, captions, cap_lens, written, trainer, build_mask):
    for name, flag in (('on', True), ('off', False), ('off2', False)):
        algo, out = _trainer(tmp_path, name, ds, loader, None, True)
        algo.attention_maps = flag
        sh.seed_all(7)
        text_encoder, image_encoder, netG, netsD, _ = algo.build_models()
        netG.set_return_attention(False)
        words_embs, sent_emb = algo._encode(text_encoder, captions, cap_lens)
        noise = torch.randn(algo._noise_shape(2), device=DEV)
        before = torch.cuda.get_rng_state(), torch.get_rng_state()     # (CA_NET draws its eps in every forward)
        algo.save_img_results(netG, noise, sent_emb, words_embs, build_mask(captions, words_embs.size(2)),
                              image_encoder, captions, cap_lens, 3, name='average')
        assert netG.training and not any(m.return_attention for m in netG.modules() if hasattr(m, 'return_attention'))
        written[name] = {f: open(os.path.join(out, f), 'rb').read() for f in _files(out)}
        if not flag:                     # the plain grid: the samples of each scale side by side, as bytes
            netG.eval()
            torch.cuda.set_rng_state(before[0])
            torch.set_rng_state(before[1])
            with torch.no_grad():
                fake = netG(noise, sent_emb, words_embs, build_mask(captions, words_embs.size(2)))[0]
            netG.train()
            for i, f in enumerate(fake):
                want = np.concatenate([trainer._to_uint8(f[j]) for j in range(2)], 1)
                path = os.path.join(out, 'Image', 'G_average_3_%d.png' % i)
                assert np.array_equal(np.asarray(Image.open(path)), want), path


def _gen_example(tmp_path, name, ds, loader, bert_dir, netG, flag, fused=False):
    from miscc.config import cfg
    algo, out = _trainer(tmp_path, name, ds, loader, bert_dir, False)
    algo.fused_inference = fused
    os.makedirs(out)
    cfg.TRAIN.NET_G = os.path.join(out, 'netG_epoch_0.pth')
    torch.save(netG.state_dict(), cfg.TRAIN.NET_G)
    algo.attention_maps = flag
    caps = np.array([[1, 2, 3, 4, 5, 6, 7], [3, 2, 1, 0, 0, 0, 0]], dtype=np.int64)
    sh.seed_all(100)
    root = algo.gen_example({'bird': [caps, np.array([7, 3]), np.array([1, 0])]})
    return root, _rng_states()


@pytest.mark.parametrize('bert,fused', [(False, False), (True, False), (False, True)], ids=['rnn', 'bert', 'rnn-fused'])
def test_gen_example_with_and_without_the_flag(tmp_path, bert, fused):
    """fused: with fused_inference too (FusedGenerator hands the wrapped generator's maps through)"""
    from miscc.config import reset_cfg
    from miscc.utils import weights_init
    ds, loader, bert_dir = _toy(tmp_path, bert=bert)
    torch.manual_seed(1)
    if bert:
        import model_bert
        netG = model_bert.G_NET()
    else:
        import model
        netG = model.G_NET()
    netG.apply(weights_init)
    from sbagan import ops
    ops.set_deterministic(True)          # (the images of two runs are bit-identical only in the deterministic mode)
    try:
        root, states = _gen_example(tmp_path, 'on', ds, loader, bert_dir, netG, True, fused)
        root0, states0 = _gen_example(tmp_path, 'off', ds, loader, bert_dir, netG, False, fused)
    finally:
        ops.set_deterministic(False)
    files, files0 = _files(root), _files(root0)
    extra = sorted(set(files) - set(files0))
    tags = ['_AB', '_BA', '_A', '_B'] if bert else ['']
    assert extra == sorted('bird/0_s_%d_a0%s.png' % (i, t) for i in (0, 1) for t in tags)
    assert sorted(set(files) - set(extra)) == files0 and len(files0) == 4 * len(tags)
    for f in files0:                                       # the images themselves do not change
        assert open(os.path.join(root, f), 'rb').read() == open(os.path.join(root0, f), 'rb').read(), f
    for t in tags:                                         # caption 1 (7 words) is row 0, caption 0 (3 words) row 1
        assert Image.open(os.path.join(root, 'bird/0_s_1_a0%s.png' % t)).size == (5 * 258, 306)
        assert Image.open(os.path.join(root, 'bird/0_s_0_a0%s.png' % t)).size == (3 * 258, 306)
    assert sh.same_states(states, states0)
    reset_cfg()


@pytest.mark.parametrize('bert', [False, True], ids=['rnn', 'bert'])
def test_pretraining_step_writes_attention_maps(tmp_path, monkeypatch, bert):
    """one update of pretrain_DAMSM.py's (pretrain_DAMSM_bert.py's) main() with the flag on the toy data_dir: the step-0
    log line's overlay"""
    import yaml
    from miscc.config import reset_cfg
    from test_host_cpu import _make_dataset
    reset_cfg()
    root = str(tmp_path / 'toy')
    _make_dataset(root, n_train=4, n_test=4)
    yml = tmp_path / 'damsm_toy.yml'
    yml.write_text(yaml.safe_dump({
        'CONFIG_NAME': 'DAMSM', 'DATASET_NAME': 'toy', 'DATA_DIR': root, 'GPU_ID': 0, 'WORKERS': 0,
        'TREE': {'BRANCH_NUM': 1, 'BASE_SIZE': 128},
        'TRAIN': {'FLAG': True, 'NET_E': '', 'BATCH_SIZE': 4, 'MAX_EPOCH': 1, 'SNAPSHOT_INTERVAL': 1,
                  'ENCODER_LR': 0.002, 'RNN_GRAD_CLIP': 0.25,
                  'SMOOTH': {'GAMMA1': 4.0, 'GAMMA2': 5.0, 'GAMMA3': 10.0}},
        'TEXT': {'EMBEDDING_DIM': 256, 'CAPTIONS_PER_IMAGE': 2, 'WORDS_NUM': 8}}))
    monkeypatch.chdir(tmp_path / 'toy')
    from sbagan import ops
    ops.set_compute_dtype(torch.bfloat16)
    argv = ['--cfg', str(yml), '--gpu', '0', '--manualSeed', '7', '--attention_maps']
    if bert:
        import pretrain_DAMSM_bert
        from test_bert_entry_gpu import _bert_dir
        model_dir = pretrain_DAMSM_bert.main(argv + ['--bert_dir', _bert_dir(tmp_path)], max_steps=1)
    else:
        import pretrain_DAMSM
        model_dir = pretrain_DAMSM.main(argv, max_steps=1)
    image_dir = os.path.join(os.path.dirname(model_dir), 'Image')
    assert _files(image_dir) == ['attention_maps0.png']
    assert Image.open(os.path.join(image_dir, 'attention_maps0.png')).size == (10 * 274, 4 * (50 + 544))
    reset_cfg()
