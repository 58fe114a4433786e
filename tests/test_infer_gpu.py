"""GPU checks of the fused inference generator (sbagan/infer.py): the folded conv + GLU / conv + bias + residual
kernels against a float64 composition of conv -> eval BatchNorm -> GLU, FusedGenerator against the reference's
eval-mode fixtures (tests/golden/infer_*.npz), module state, determinism, refusals, and sampling with the flag."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import FULL, TINY, g_shapes, load_golden, make_inputs, rel_l2
from oracle import fill

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
# tests/test_kernels_gpu.py::tol
F32_RTOL, F32_ATOL, BF16_L2 = 2e-4, 2e-5, 2e-2


def _set_dims(d, branch=3):
    from miscc.config import cfg, reset_cfg
    reset_cfg()
    cfg.GAN.GF_DIM, cfg.GAN.DF_DIM, cfg.TREE.BRANCH_NUM = d['ngf'], d['ndf'], branch
    cfg.TEXT.EMBEDDING_DIM, cfg.GAN.CONDITION_DIM, cfg.GAN.Z_DIM, cfg.GAN.W_DIM = d['nef'], d['ncf'], d['nz'], d['nw']
    cfg.GAN.R_NUM = 2
    return cfg


@pytest.fixture(autouse=True)
def _reset():
    yield
    from miscc.config import reset_cfg
    from sbagan import ops
    reset_cfg()
    ops.set_compute_dtype(torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------------------------------------------
# (kind, N, H, Cin, C, residual half?, fragment-major weights offered?, expected family bf16, f32)
#   GF_DIM 32: INIT_STAGE upBlocks 512 -> 256 (4^2 -> 8^2) ... 64 -> 32 (32^2 -> 64^2); ResBlocks 64 -> 2 x 64 / 64 -> 64 at
#   64^2 and 128^2; NEXT_STAGE upBlock 64 -> 32 to 128^2 / 256^2.  GF_DIM 64: the same with every width doubled
#   (1024 -> 512 at 4^2; ResBlocks and NEXT_STAGE upBlock with Cin = 128: the halo kernels' two-chunk walk).
#   Families: GLU launches through sba_conv_igemm_glu_plan ('halo' conv3x3_halo_kernel, 'halo3' conv3x3_halo3_kernel,
#   'igemm' igemm_kernel); residual halves through sba_conv_igemm_plan ('halo' = family 0, 'dma2' igemm_dma2_kernel -- the
#   existing dispatcher's choice for a 3-image batch, below the halo kernels' 128 tiles -- 'igemm').
KERNEL_CASES = [
    ('3x3up', 20, 4, 512, 256, False, False, 'igemm', 'igemm'),
    ('3x3up', 3, 4, 512, 256, False, False, 'igemm', 'igemm'),
    ('3x3up', 20, 4, 1024, 512, False, False, 'igemm', 'igemm'),
    ('3x3up', 20, 8, 256, 128, False, False, 'igemm', 'igemm'),
    ('3x3up', 20, 32, 64, 32, False, False, 'halo', 'igemm'),
    ('3x3', 20, 64, 64, 64, False, True, 'halo3', 'igemm'),
    ('3x3', 20, 64, 64, 64, False, False, 'halo', 'igemm'),      # LDS weights, no upsample
    ('3x3', 3, 64, 64, 64, True, True, 'dma2', 'igemm'),
    ('3x3', 20, 64, 64, 64, True, True, 'halo', 'igemm'),
    ('3x3', 3, 128, 128, 128, True, True, 'halo', 'igemm'),
    ('3x3up', 3, 64, 64, 32, False, False, 'halo', 'igemm'),
    ('3x3up', 3, 64, 128, 64, False, False, 'halo', 'igemm'),
    ('3x3', 3, 128, 128, 128, False, True, 'halo3', 'igemm'),
    ('3x3up', 20, 128, 64, 32, False, False, 'halo', 'igemm'),
    ('3x3up', 2, 16, 128, 64, False, False, 'igemm', 'igemm'),
    ('3x3', 3, 8, 16, 8, False, False, None, 'igemm'),          # the reduced-size fixtures' widths (f32 only: Cin % 32)
]


def _family(plan):
    if plan[0] == 0:
        return 'halo3' if plan[1] & 2 else 'halo'
    return {3: 'igemm'}[plan[0]]


# (bf16 MFMA slabs are 32 channels deep: the Cin = 16 width exists only in the f32 reduced-size fixtures)
KERNEL_PARAMS = [(dt,) + c for dt in (torch.float32, torch.bfloat16) for c in KERNEL_CASES
                 if not (dt == torch.bfloat16 and c[3] % 32)]


@pytest.mark.parametrize('dt,kind,N,H,Cin,C,res,frag,fam_bf16,fam_f32', KERNEL_PARAMS)
def test_folded_conv_kernels_vs_float64(dt, kind, N, H, Cin, C, res, frag, fam_bf16, fam_f32):
    from sbagan import _lib, infer, ops
    ops.set_compute_dtype(dt)
    O = C if res else 2 * C
    w = (fill.unit((O, Cin, 3, 3), 11) * (2.0 / (9 * Cin) ** 0.5)).contiguous(memory_format=torch.channels_last)
    x = fill.unit((N, Cin, H, H), 12)
    gamma, beta = 1 + 0.3 * fill.unit((O,), 13), 0.2 * fill.unit((O,), 14)
    mean, var = 0.1 * fill.unit((O,), 15), 0.5 + 0.4 * fill.unit((O,), 16).abs()

    class BN(object):
        pass
    bn = BN()
    bn.weight, bn.bias, bn.running_mean, bn.running_var = (t.to(DEV).contiguous() for t in (gamma, beta, mean, var))
    xd = ops.as_act(x.to(DEV), dt)
    x64 = xd.double().cpu()                      # the kernel's own (rounded) input
    if kind == '3x3up':
        x64 = F.interpolate(x64, scale_factor=2, mode='nearest')
    y = F.conv2d(x64, w.double(), None, 1, 1)
    s = (gamma.double() / torch.sqrt(var.double() + ops.BN_EPS))
    y = (y - mean.double()[None, :, None, None]) * s[None, :, None, None] + beta.double()[None, :, None, None]
    fg = infer.FusedGenerator.__new__(infer.FusedGenerator)
    fg._dtype = dt
    f = infer._fold(w.to(DEV), bn, 9, Cin, not res, dt, frag=frag)
    want_fam = fam_bf16 if dt == torch.bfloat16 else fam_f32
    plan = (ctypes.c_int * 3)()
    if res:
        want = y + xd.double().cpu()
        got = fg._conv_bias_add(xd, f, xd)
        g = ops._geom(('3x3', N, H, H, Cin, C, None))            # the (tuned) geometry _conv_bias_add launched with
        g.w_layout = 1 if (f.wf is not None and ops._halo_family(g)) else 0
        _lib.call('sba_conv_igemm_plan', ops._dt(xd), ctypes.byref(g), ops.WORKSPACE_BYTES, plan)
        g.w_layout = 0
        assert {0: 'halo', 1: 'dma2', 2: 'dma', 3: 'igemm', 4: 'halo3g'}[plan[0]] == want_fam, list(plan)
        assert (f.wf is not None) == (dt == torch.bfloat16)
    else:
        want = y[:, :C] * torch.sigmoid(y[:, C:])
        got = fg._conv_glu(xd, f, kind)
        g = fg._glu_geom(kind, xd, f)
        g.w_layout = 1 if (f.wf is not None and g._glu_halo) else 0
        _lib.call('sba_conv_igemm_glu_plan', ops._dt(xd), ctypes.byref(g), C, plan)
        g.w_layout = 0
        assert _family(plan) == want_fam, (list(plan), f.wf is None, g._glu_halo)
        assert plan[2] == 1
    torch.cuda.synchronize()
    assert got.shape == want.shape and got.dtype == dt
    got = got.double().cpu()
    r = rel_l2(got, want)
    print('folded %s N%d H%d Cin%d C%d res=%s frag=%s %s: rel L2 %.3e max abs %.3e' % (
        kind, N, H, Cin, C, res, frag, dt, r, float((got - want).abs().max())))
    if dt == torch.float32:
        assert bool(((got - want).abs() <= F32_ATOL + F32_RTOL * want.abs()).all()), float((got - want).abs().max())
    else:
        assert r <= BF16_L2, r


# ---------------------------------------------------------------------------------------------------------------
# module level
# ---------------------------------------------------------------------------------------------------------------
# (the reduced-size fixtures infer_tiny_*.npz are CPU-only, tests/test_infer_cpu.py: at GF_DIM = 8 the image head and the
# attention kernels of the existing forward refuse the widths -- sba_img_head_fwd returns SBA_E_ARG -- with or without
# the wrapper; their conv widths are covered at kernel level above)
CASES = [('infer_full_model_b4.npz', FULL, 'model'), ('infer_full_bert_b4.npz', FULL, 'bert'),
         ('infer_full_mix_b4.npz', FULL, 'mix')]

# f32: the bound tests/test_step_gpu.py::test_generator_forward_backward applies to f32 images (relative L2 2e-4 * (1 + stage)).
# The c-only first stage makes the bert / mix fixtures less well conditioned: the reference's OWN float32 run is up to
# 6.3e-4 from a float64 evaluation at stage 2 (tests/test_infer_cpu.py: REF_F32_L2, asserted there), above that bound.
# For those two fixtures the bound is the one above plus twice the reference's own error (two independent float32
# evaluations are compared); the model fixture keeps the bound as it is.
F32_IMG_L2 = 2e-4


def _f32_bound(name, i):
    from test_infer_cpu import REF_F32_L2
    extra = 0.0 if name == 'infer_full_model_b4.npz' else 2 * REF_F32_L2[name][i]
    return F32_IMG_L2 * (1 + i) + extra
# bf16, full-size fixture, relative L2 per stage against the reference's eval-mode images.  Measured on an MI355X:
# existing netG.eval() path BF16_EVAL_MEASURED; the fused path is allowed that + 25 % (one rounding moves from the
# activation to the weight: neither side is systematically better).  See DESIGN.md section "Fused inference".
BF16_EVAL_MEASURED = (6.9e-3, 0.146, 0.358)        # (the fused path measured 6.0e-3, 0.122, 0.335 in the same run)
BF16_MARGIN = 1.25


def _build(d, variant, salt=0):
    import model
    import model_bert
    net = {'model': model.G_NET, 'bert': model_bert.G_NET, 'mix': model_bert.G_NET_MIX}[variant]()
    P = fill.fill_state_dict(g_shapes(d, 3, 'model' if variant == 'model' else 'bert'), salt=salt)
    net.load_state_dict(P)
    return net.to(DEV).eval(), P


def _inputs(G, d, variant):
    B, tag = int(G['B']), int(G['tag'])
    x = make_inputs(d, B, 18, lmax=18, tag=tag)
    z = x['z2'] if variant == 'mix' else x['z']
    return z.to(DEV), x['sent'].to(DEV), x['words'].to(DEV), x['mask'].to(DEV), torch.from_numpy(G['eps']).to(DEV)


def _fixture_l2(G, name, t):
    t = t.detach().double().flatten().cpu()
    if name + '/full' in G.files:
        ref = torch.from_numpy(G[name + '/full']).double()
    else:
        ref = torch.from_numpy(G[name + '/sample']).double()
        t = t[::int(G[name + '/stride'])][:ref.numel()]
    return float((t - ref).norm() / ref.norm())


@pytest.mark.parametrize('name,d,variant', CASES)
def test_fused_generator_f32_vs_reference_fixture(golden_dir, name, d, variant):
    from sbagan import ops
    from sbagan.infer import FusedGenerator
    _set_dims(d)
    ops.set_compute_dtype(torch.float32)
    G = load_golden(golden_dir, name)
    net, _ = _build(d, variant)
    z, sent, words, mask, eps = _inputs(G, d, variant)
    net.ca_net.eps = eps
    fused = FusedGenerator(net)
    with torch.no_grad():
        outs = {'eval': net(z, sent, words, mask), 'fused': fused(z, sent, words, mask)}
    torch.cuda.synchronize()
    for tag, (imgs, atts, mu, lv) in outs.items():
        assert len(imgs) == 3 and len(atts) == 2
        for i, im in enumerate(imgs):
            assert im.dtype == torch.float32 and im.shape == (int(G['B']), 3, 64 << i, 64 << i)
            r = _fixture_l2(G, 'img%d' % i, im)
            print('%s %s f32 img%d rel L2 %.3e' % (name, tag, i, r))
            assert r <= _f32_bound(name, i), (tag, i, r)
        assert _fixture_l2(G, 'mu', mu) <= F32_IMG_L2 and _fixture_l2(G, 'logvar', lv) <= F32_IMG_L2
    for a, b in zip(outs['eval'][1], outs['fused'][1]):
        assert a.shape == b.shape and a.dtype == b.dtype
    # The two paths against each other over the WHOLE tensors, at the same bound.  Stage 2 of the bert / mix fixtures is
    # printed, not asserted: behind two attention stages of the c-only generators a few isolated pixels carry the
    # full-tensor L2 (the reference's own float32 run is 2e-2 off a float64 evaluation at single pixels there), and the
    # fixture's strided sample above is what pins that stage (measured over the whole tensor: 2.3e-3 bert, 2.8e-3 mix).
    for i, (a, b) in enumerate(zip(outs['eval'][0], outs['fused'][0])):
        r = rel_l2(b, a)
        print('%s f32 img%d fused vs eval rel L2 %.3e' % (name, i, r))
        if i < 2 or variant == 'model':
            assert r <= _f32_bound(name, i), (i, r)


@pytest.mark.parametrize('name,d,variant', CASES)
def test_fused_generator_bf16_vs_reference_fixture(golden_dir, name, d, variant):
    """Stages 1 / 2 follow the measured-bound recipe and, with these filled parameters, are NOT a parity statement (the
    existing path itself is 15 % / 36 % off in bf16).  What pins the bf16 module path is stage 0, which is well
    conditioned: both paths against the fixture, and the fused path against the existing one, at the project's bf16
    per-tensor bound (relative L2 2e-2, tests/test_kernels_gpu.py::tol)."""
    from sbagan import ops
    from sbagan.infer import FusedGenerator
    _set_dims(d)
    ops.set_compute_dtype(torch.bfloat16)
    G = load_golden(golden_dir, name)
    net, _ = _build(d, variant)
    z, sent, words, mask, eps = _inputs(G, d, variant)
    net.ca_net.eps = eps
    fused = FusedGenerator(net)
    with torch.no_grad():
        ev = net(z, sent, words, mask)
        fu = fused(z, sent, words, mask)
    torch.cuda.synchronize()
    re = [_fixture_l2(G, 'img%d' % i, im) for i, im in enumerate(ev[0])]
    rf = [_fixture_l2(G, 'img%d' % i, im) for i, im in enumerate(fu[0])]
    rx = [rel_l2(b, a) for a, b in zip(ev[0], fu[0])]
    print('%s bf16 eval-mode rel L2 per stage: existing' % name, re, 'fused', rf, 'fused vs existing', rx)
    assert re[0] <= BF16_L2 and rf[0] <= BF16_L2 and rx[0] <= BF16_L2, (re[0], rf[0], rx[0])
    assert _fixture_l2(G, 'mu', fu[2]) <= F32_IMG_L2 and _fixture_l2(G, 'logvar', fu[3]) <= F32_IMG_L2
    if variant == 'model':          # the measured pair below is of this fixture
        for i in range(3):
            assert re[i] <= BF16_EVAL_MEASURED[i] * BF16_MARGIN, ('eval', i, re[i])
            assert rf[i] <= BF16_EVAL_MEASURED[i] * BF16_MARGIN, ('fused', i, rf[i])


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('variant', ['model', 'mix'])
def test_state_determinism_refold(golden_dir, dt, variant):
    from sbagan import ops
    from sbagan.infer import FusedGenerator
    _set_dims(FULL)
    ops.set_compute_dtype(dt)
    # (the shared attention / AdaIN kernels add partial sums with f32 atomics in the default mode: bit-equality is a
    # property of the deterministic-reduction mode, as in tests/test_determinism_gpu.py)
    ops.set_deterministic(True, DEV)
    try:
        _state_determinism_refold(golden_dir, dt, variant)
    finally:
        ops.set_deterministic(False)


def _state_determinism_refold(golden_dir, dt, variant):
    from sbagan import ops
    from sbagan.infer import FusedGenerator
    G = load_golden(golden_dir, CASES[0][0])
    net, _ = _build(FULL, variant)
    z, sent, words, mask, eps = _inputs(G, FULL, variant)
    net.ca_net.eps = eps
    before = {k: v.clone() for k, v in net.state_dict().items()}
    fused = FusedGenerator(net)
    with torch.no_grad():
        a = fused(z, sent, words, mask)
        b = fused(z, sent, words, mask)
    torch.cuda.synchronize()
    for k, v in net.state_dict().items():
        assert torch.equal(v, before[k]), k
    for x, y in zip(a[0] + [a[2], a[3]], b[0] + [b[2], b[3]]):
        assert torch.equal(x, y)
    # refold after loading other parameters == a freshly built wrapper
    P2 = fill.fill_state_dict(g_shapes(FULL, 3, 'model' if variant == 'model' else 'bert'), salt=5)
    net.load_state_dict(P2)
    fused.refold()
    fresh = FusedGenerator(net)
    with torch.no_grad():
        c = fused(z, sent, words, mask)
        e = fresh(z, sent, words, mask)
    for x, y in zip(c[0], e[0]):
        assert torch.equal(x, y)
    assert not torch.equal(a[0][-1], c[0][-1])


def test_refusals(golden_dir):
    from sbagan import ops
    from sbagan.infer import FusedGenerator
    _set_dims(FULL)
    ops.set_compute_dtype(torch.bfloat16)
    G = load_golden(golden_dir, CASES[0][0])
    net, _ = _build(FULL, 'model')
    z, sent, words, mask, eps = _inputs(G, FULL, 'model')
    fused = FusedGenerator(net)
    with pytest.raises(RuntimeError, match='no_grad'):
        fused(z, sent, words, mask)
    net.train()
    with torch.no_grad(), pytest.raises(RuntimeError, match='eval'):
        fused(z, sent, words, mask)
    net.eval()
    with torch.no_grad():
        assert len(fused(z, sent, words, mask)[0]) == 3


def _toy_yml(tmp_path, root, net_g, validation, mixing=False, net_e=''):
    import yaml
    yml = tmp_path / ('toy_%s.yml' % os.path.basename(os.path.dirname(net_g)))
    yml.write_text(yaml.safe_dump({
        'CONFIG_NAME': 'toy', 'DATASET_NAME': 'toy', 'DATA_DIR': root, 'GPU_ID': 0, 'WORKERS': 0,
        'B_VALIDATION': validation, 'TREE': {'BRANCH_NUM': 2, 'BASE_SIZE': 64},
        'TRAIN': {'FLAG': False, 'NET_G': net_g, 'NET_E': net_e, 'BATCH_SIZE': 2, 'MIXING': mixing},
        'GAN': {'DF_DIM': 64, 'GF_DIM': 32, 'Z_DIM': 100, 'R_NUM': 2},
        'TEXT': {'EMBEDDING_DIM': 256, 'CAPTIONS_PER_IMAGE': 2, 'WORDS_NUM': 8}}))
    return str(yml)


def _pngs(root_dir):
    from PIL import Image
    files = sorted(glob.glob(os.path.join(root_dir, '**', '*.png'), recursive=True))
    return {os.path.relpath(f, root_dir): np.asarray(Image.open(f)).astype(np.int32) for f in files}


def _compare(imgs, dt, what, f32_mean_only=None):
    assert len(imgs[False]) > 0 and set(imgs[False]) == set(imgs[True])
    diff = [np.abs(imgs[False][k] - imgs[True][k]) for k in imgs[False]]
    mx, mean = max(int(d.max()) for d in diff), float(np.mean([d.mean() for d in diff]))
    print('%s %s: %d files, max grey-level difference %d, mean %.4f' % (what, dt, len(diff), mx, mean))
    if f32_mean_only is not None:
        assert mean <= f32_mean_only, mean
    elif dt == torch.float32:
        assert mx <= 1, mx
    else:
        # mean absolute difference below the module-level bf16 bound in grey levels (images span 255 levels)
        assert mean <= BF16_EVAL_MEASURED[1] * BF16_MARGIN * 255, mean


def _example_files(root, text):
    with open(os.path.join(root, 'example_filenames.txt'), 'w') as f:
        f.write('example_captions\n')
    with open(os.path.join(root, 'example_captions.txt'), 'w') as f:
        f.write(text)


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16])
def test_main_sampling_and_gen_example_with_and_without_the_flag(tmp_path, dt):
    """main.main() on the toy data set of test_train_checkpoint_resume_and_sampling, evaluation seed, without and with
    --fused_inference: sampling (B_VALIDATION) and gen_example write the same files; f32 images within one grey level."""
    from test_host_cpu import _make_dataset
    from miscc.config import reset_cfg
    import main
    import model
    from sbagan import ops
    from trainer import condGANTrainer
    root = str(tmp_path / 'toy')
    _make_dataset(root)
    _example_files(root, 'the small red bird\nblue wing\na long white yellow belly tail\n')
    _set_dims(FULL, branch=2)
    net = model.G_NET()
    sd = fill.fill_state_dict(g_shapes(FULL, 2, 'model'))
    seen = []

    def make_trainer(out, loader, n_words, ixtoword):      # (the toy data set has no pre-trained text encoder)
        algo = condGANTrainer(out, loader, n_words, ixtoword, allow_random_encoders=True)
        seen.append(algo)
        return algo
    for validation in (True, False):
        imgs = {}
        for flag in (False, True):
            ck = str(tmp_path / ('g%d%d' % (validation, flag)) / 'netG_epoch_1.pth')
            os.makedirs(os.path.dirname(ck))
            torch.save(sd, ck)
            reset_cfg()
            ops.set_compute_dtype(dt)
            argv = ['--cfg', _toy_yml(tmp_path, root, ck, validation), '--gpu', '0']
            main.main(argv + (['--fused_inference'] if flag else []), make_trainer=make_trainer)
            assert seen[-1].fused_inference is flag
            imgs[flag] = _pngs(ck[:-4])
        _compare(imgs, dt, 'main.main sampling' if validation else 'main.main gen_example')
        assert len(imgs[True]) == (2 if validation else 6)


def test_main_bert_gen_example_with_the_flag(tmp_path):
    """main_bert.main() gen_example (trainer_bert: G_NET and G_NET_MIX around one checkpoint, (2, B, Z) noise) without
    and with --fused_inference, f32: the same _AB / _BA / _A / _B files, images within one grey level."""
    from test_bert_entry_gpu import _bert_dir
    from test_host_cpu import _make_dataset
    from miscc.config import reset_cfg
    import main_bert
    import model_bert
    from sbagan import ops
    root = str(tmp_path / 'toy')
    _make_dataset(root)
    _example_files(root, 'the small red bird\nthe bird is blue with a long tail\nwhite belly\n')
    bert_dir = _bert_dir(tmp_path)
    cfg = _set_dims(FULL, branch=2)
    sd = fill.fill_state_dict(g_shapes(FULL, 2, 'bert'))
    torch.manual_seed(5)
    net_e = str(tmp_path / 'text_encoder0.pth')
    torch.save(model_bert.BertEncoder(cfg.TEXT.EMBEDDING_DIM, bert_dir=bert_dir).state_dict(), net_e)
    imgs = {}
    for flag in (False, True):
        ck = str(tmp_path / ('b%d' % flag) / 'netG_epoch_1.pth')
        os.makedirs(os.path.dirname(ck))
        torch.save(sd, ck)
        reset_cfg()
        ops.set_compute_dtype(torch.float32)
        argv = ['--cfg', _toy_yml(tmp_path, root, ck, False, net_e=net_e), '--gpu', '0', '--bert_dir', bert_dir]
        main_bert.main(argv + (['--fused_inference'] if flag else []))
        imgs[flag] = _pngs(ck[:-4])
    # The c-only generators amplify float32-level differences at isolated pixels (module level: relative L2 up to
    # _f32_bound at stage 1), so "one rounding boundary" does not hold pixel by pixel here (2 levels observed at single
    # pixels).  Asserted instead, as for bf16 in main.main: the mean absolute difference below the module-level bound in
    # grey levels -- the chance that a difference d (in levels) crosses a rounding boundary is d, so the mean uint8
    # difference is the mean |d| <= rms d <= bound * 127.5 (tanh outputs, rms <= 1).
    _compare(imgs, torch.float32, 'main_bert.main gen_example',
             f32_mean_only=max(_f32_bound(n, 1) for n in ('infer_full_bert_b4.npz', 'infer_full_mix_b4.npz')) * 127.5)
    assert len(imgs[True]) == 3 * 2 * 4
