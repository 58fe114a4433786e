"""GPU parity tests, kernel level: every C-ABI entry point (through sbagan.ops / the module
classes) against the CPU oracle or a plain torch fp32 CPU reference of the same op.

Tolerances (stated per dtype):
  float32 path (exact f32 MFMA): elementwise rtol 2e-4 / atol 2e-5 unless noted;
  bfloat16 path (bf16 storage + MFMA, f32 accumulate): relative L2 error <= 2e-2 per tensor
  (bf16 has an 8-bit mantissa; fixed elementwise tolerances are not meaningful).  The raw convolutions are held
  tighter (test_conv_fwd_dgrad_wgrad): y and dx element by element to one bf16 rounding of the float64 result plus
  1e-5 x the contraction of the absolute values (tests/conv_ref.py), the f32 weight gradient to the f32 tolerances
  and to 1e-5 x the sum of the absolute products.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import conv_ref as CR  # noqa: E402
from helpers import rel_l2  # noqa: E402
from oracle import fill  # noqa: E402
from oracle import sbagan_oracle as O  # noqa: E402

DTYPES = [torch.float32, torch.bfloat16]


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@pytest.fixture(autouse=True)
def _reset_cfg():
    from miscc.config import cfg, reset_cfg
    reset_cfg()
    cfg.GAN.GF_DIM, cfg.GAN.DF_DIM = 32, 64
    cfg.TRAIN.SMOOTH.GAMMA1, cfg.TRAIN.SMOOTH.GAMMA2, cfg.TRAIN.SMOOTH.GAMMA3 = 4.0, 5.0, 10.0
    cfg.TRAIN.SMOOTH.LAMBDA = 5.0
    yield


def tol(dt):
    return dict(l2=3e-5, rtol=2e-4, atol=2e-5) if dt == torch.float32 else dict(l2=2e-2, rtol=None, atol=None)


def close(got, ref, dt, name='', scale=1.0):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    t = tol(dt)
    r = rel_l2(got, ref)
    assert r <= t['l2'] * scale, '%s: rel L2 %.3e > %.1e' % (name, r, t['l2'] * scale)
    if t['rtol'] is not None:
        err = (got - ref).abs()
        bound = scale * (t['atol'] + t['rtol'] * ref.abs()) + 1e-6 * float(ref.abs().max())
        assert bool((err <= bound).all()), '%s: max err %.3e' % (name, float(err.max()))


def elem_bound(got, ref, A, name, u=CR.U_BF16):
    """a bf16 convolution output element by element (tests/conv_ref.py): one rounding of an f32 accumulator,
    |got - ref| <= u |ref| + c A with A the same contraction on absolute values"""
    got, ref, A = got.detach().double().cpu(), ref.detach().double().cpu(), A.detach().double().cpu()
    assert got.shape == ref.shape == A.shape, (name, got.shape, ref.shape, A.shape)
    assert bool(torch.isfinite(got).all()), name
    worst = float(((got - ref).abs() / (u * ref.abs() + CR.C_ACC * A).clamp(min=1e-300)).max())
    print('%-34s elementwise: worst err / bound = %.3f' % (name, worst))
    assert worst <= 1.0, '%s: worst err / bound = %.3f' % (name, worst)


def sums_bound(got, ref, A, name):
    """an f32 sum of products (weight gradient): |got - ref| <= c x the float64 sum of the absolute products"""
    got, ref, A = got.detach().double().cpu(), ref.detach().double().cpu(), A.detach().double().cpu()
    assert got.shape == ref.shape == A.shape, (name, got.shape, ref.shape, A.shape)
    worst = float(((got - ref).abs() / A.clamp(min=1e-30)).max())
    print('%-34s f32 sums: worst |err| / sum |products| = %.2e' % (name, worst))
    assert worst <= CR.C_ACC, '%s: %.3e > %.0e' % (name, worst, CR.C_ACC)


def act(x, dt, dev):
    return x.detach().to(dev).to(dt).contiguous(memory_format=torch.channels_last).clone()


def rounded(x, dt):
    """what the kernel actually sees of an input tensor"""
    return x.detach().to(dt).float().clone()


# ------------------------------------------------------------------ raw convolutions
CONV_CASES = [
    # kind, N, Cin, Cout, H, W
    ('3x3', 2, 64, 64, 16, 16),
    ('3x3', 3, 32, 128, 7, 5),        # ragged M (105 rows), odd sizes
    ('3x3', 1, 64, 192, 4, 4),        # Cout not a multiple of 128
    ('3x3up', 2, 64, 64, 8, 8),
    ('3x3up', 1, 128, 256, 4, 4),
    ('3x3up', 3, 32, 64, 5, 3),
    ('4x4s2', 2, 64, 128, 16, 16),
    ('4x4s2', 3, 128, 64, 8, 8),
    ('3x3', 1, 64, 64, 96, 96),       # M = 9216 -> 256-row tiles
    ('3x3', 1, 64, 128, 72, 64),      # M = 4608 -> 128x128 tiles
    ('4x4s2', 2, 512, 256, 8, 8),     # M = 32, K = 8192: split-K path + small-M wgrad (f32; bf16: kernel-row wgrad, OW = 4)
    ('3x3', 4, 256, 512, 4, 4),       # M = 64, K = 2304: split-K with a ragged last split
    ('3x3up', 2, 512, 512, 4, 4),     # generator stage-1 shape
    ('3x3', 2, 64, 64, 128, 128),     # M = 32768: kernel-row wgrad with 79 pixel splits in bf16, generic wgrad_kernel x21 in f32
    ('3x3up', 2, 64, 128, 64, 64),    # same with the fused nearest x2 (output 128 x 128)
    ('3x3', 1, 128, 64, 128, 256),    # two ci tiles, non-square map
    ('3x3', 8, 64, 64, 128, 128),     # 512 8 x 32 tiles: halo-tile forward kernel; M = 131072: f32 all-taps halo-row wgrad (wgrad_rows_kernel)
    ('3x3', 5, 64, 128, 128, 128),    # ... two 64-channel blocks of Cout, 320 tiles per block
    ('3x3up', 9, 64, 64, 64, 64),     # ... behind the nearest x2 upsample (576 tiles, LDS-weight conv3x3_halo_kernel)
    ('3x3up', 2, 128, 128, 64, 64),   # halo-tile kernel walking TWO 64-channel chunks of Cin = 128, behind the nearest x2 upsample
    ('3x3', 8, 128, 64, 64, 64),      # ... plain 3x3 (the shape of the data gradient of the ResBlocks' 64 -> 128 conv)
    ('3x3', 20, 768, 512, 4, 4),      # D_GET_LOGITS.jointConv at B = 20 (M = 320): kernel-row wgrad on 4 x 4 maps (two images per chunk), 10 stages
    ('3x3', 3, 224, 544, 4, 4),       # LDS-DMA small-pixel-count wgrad, ragged: last ci / co tiles 32 channels wide, M = 48 (half-empty second stage)
    ('3x3', 16, 256, 512, 8, 8),      # M = 1024: two pixel splits, f32 atomics (bf16: kernel-row wgrad, f32: wgrad_small_kernel)
    ('3x3', 2, 1024, 1024, 4, 4),     # 576 workgroups of the small-pixel-count kernels in f32; bf16: kernel-row wgrad, one 32-pixel chunk of two 4 x 4 maps
    ('4x4s2', 2, 64, 128, 64, 64),    # wgrad_row_dma_kernel<4, 2, 10, 4> (the four kw taps of a kernel row share one staged input row): OW = 32
    ('4x4s2', 3, 128, 64, 32, 32),    # ... OW = 16 (two output rows per 32-pixel chunk), two ci tiles
    ('4x4s2', 2, 64, 64, 256, 128),   # ... OW = 64 (two chunks per output row), non-square, pixel splits
    ('4x4s2', 5, 192, 128, 16, 16),   # ... OW = 8 (four output rows per chunk), three ci tiles
    ('3x3', 2, 1056, 1024, 4, 4),     # Cin % 64 = 32: not kernel-row; M = 32, 624 workgroups: bf16 first write wgrad_small_dma_kernel<2, 3> (one
                                      # 32-pixel stage in a depth-3 ring, half-empty last ci tile), bf16 accumulate / f32: wgrad_small_kernel
    ('3x3', 12, 224, 544, 8, 8),      # M = 768, 81 workgroups: wgrad_small_dma_kernel<1, 4> with two pixel splits, ragged last co and ci tiles
    ('3x3', 2, 32, 64, 256, 256),     # M = 131072, Cin = 32: wgrad_rows_kernel in bf16 too (Cin % 64 != 0 keeps the kernel-row kernel away)
]

# The weight-gradient kernel a case is there for: case -> {(dtype, first_write): sba_conv_wgrad_plan as
# _lib.wgrad_plan_name, 'family<template arguments> x pixel splits'}.  Checked without a device by
# tests/test_wgrad_plan_cpu.py::test_conv_cases_take_the_kernels_they_name; between them the cases reach every kernel.
WGRAD_KERNELS = {
    ('3x3', 2, 64, 64, 16, 16): {('f32', 0): 'generic<f32> x1', ('bf16', 0): 'row_dma<3,1,5,4> x1'},
    ('3x3', 1, 64, 64, 96, 96): {('f32', 0): 'generic<f32> x6', ('bf16', 0): 'small_dma<1,4> x24'},
    ('4x4s2', 2, 512, 256, 8, 8): {('f32', 0): 'small<f32> x1', ('bf16', 0): 'row_dma<4,2,10,4> x1'},
    ('3x3', 2, 64, 64, 128, 128): {('f32', 0): 'generic<f32> x21', ('bf16', 0): 'row_dma<3,1,5,4> x79'},
    ('3x3', 8, 64, 64, 128, 128): {('f32', 0): 'rows<f32> x128', ('bf16', 0): 'row_dma<3,1,5,4> x128'},
    ('3x3up', 9, 64, 64, 64, 64): {('f32', 1): 'rows<f32> x144', ('bf16', 1): 'row_dma<3,1,5,4> x128'},
    ('3x3', 20, 768, 512, 4, 4): {('f32', 0): 'small<f32> x1', ('bf16', 0): 'row_dma<3,1,6,4> x1', ('bf16', 1): 'row_dma<3,1,6,4> x1'},
    ('3x3', 3, 224, 544, 4, 4): {('bf16', 0): 'small_dma<1,4> x1', ('bf16', 1): 'small_dma<1,4> x1'},
    ('3x3', 16, 256, 512, 8, 8): {('f32', 0): 'small<f32> x2', ('bf16', 0): 'row_dma<3,1,5,4> x2'},
    ('3x3', 2, 1024, 1024, 4, 4): {('f32', 1): 'small<f32> x1', ('bf16', 0): 'row_dma<3,1,6,4> x1', ('bf16', 1): 'row_dma<3,1,6,4> x1'},
    ('4x4s2', 2, 64, 128, 64, 64): {('bf16', 0): 'row_dma<4,2,10,4> x5'},
    ('4x4s2', 3, 128, 64, 32, 32): {('bf16', 0): 'row_dma<4,2,10,4> x2'},
    ('4x4s2', 2, 64, 64, 256, 128): {('bf16', 0): 'row_dma<4,2,10,4> x40'},
    ('4x4s2', 5, 192, 128, 16, 16): {('bf16', 0): 'row_dma<4,2,10,4> x1'},
    ('3x3', 2, 1056, 1024, 4, 4): {('f32', 0): 'small<f32> x1', ('bf16', 0): 'small<bf16> x1', ('bf16', 1): 'small_dma<2,3> x1'},
    ('3x3', 12, 224, 544, 8, 8): {('bf16', 0): 'small_dma<1,4> x2', ('bf16', 1): 'small_dma<1,4> x2'},
    ('3x3', 2, 32, 64, 256, 256): {('f32', 0): 'rows<f32> x128', ('bf16', 0): 'rows<bf16> x128', ('bf16', 1): 'rows<bf16> x128'},
}


def torch_conv(x, w, kind):
    if kind == '3x3':
        return F.conv2d(x, w, None, 1, 1)
    if kind == '3x3up':
        return F.conv2d(x.repeat_interleave(2, 2).repeat_interleave(2, 3), w, None, 1, 1)
    return F.conv2d(x, w, None, 2, 1)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('case', CONV_CASES)
def test_conv_fwd_dgrad_wgrad(dev, dt, case):
    from sbagan import ops
    kind, N, Cin, Cout, H, W = case
    k = 4 if kind == '4x4s2' else 3
    x = fill.unit((N, Cin, H, W), 1)
    w = fill.unit((Cout, Cin, k, k), 2) / np.sqrt(Cin * k * k)
    # the reference in float64: a float32 weight gradient summed over 10^5 pixels on the host is itself off by up to
    # twice the elementwise bound, by an amount that depends on the host's thread count
    xr, wr = rounded(x, dt).double().requires_grad_(True), rounded(w, dt).double().requires_grad_(True)
    yref = torch_conv(xr, wr, kind)
    dy = fill.unit(tuple(yref.shape), 3)
    dyr = rounded(dy, dt).double()
    gx, gw = torch.autograd.grad(yref, [xr, wr], dyr)

    bf = dt == torch.bfloat16
    if bf:
        # the same contractions on absolute values: the scale of the f32 partial sums (tests/conv_ref.py)
        xb, wb = xr.detach().abs().requires_grad_(True), wr.detach().abs().requires_grad_(True)
        ya = torch_conv(xb, wb, kind)
        gxa, gwa = torch.autograd.grad(ya, [xb, wb], dyr.abs())
        ya = ya.detach()

    def dw_close(got, name):
        close(got, gw, dt, name)
        if bf:
            # f32 accumulation of bf16-rounded inputs: the only error is the summation order, whatever the storage
            # type of the activations -- held to the f32 tolerances and to c x the sum of the absolute products
            close(got, gw, torch.float32, name + ' at the f32 tolerances')
            sums_bound(got, gw, gwa, name)

    wp = torch.nn.Parameter(w.to(dev).contiguous(memory_format=torch.channels_last))
    pw = ops.PackedWeight(wp)
    xa = act(x, dt, dev)
    y, stats = ops.conv_forward(xa, pw, kind)
    torch.cuda.synchronize()
    close(y, yref, dt, 'y')
    if bf:
        elem_bound(y, yref, ya, 'y')
    # BN statistics of the f32 accumulators
    stats = stats.sum(0)                # add the statistics slots up
    close(stats[:Cout], yref.sum((0, 2, 3)), torch.float32, 'sum', scale=30 if dt == torch.float32 else 2000)
    close(stats[Cout:], (yref ** 2).sum((0, 2, 3)), torch.float32, 'sumsq', scale=30 if dt == torch.float32 else 2000)
    dya = act(dy, dt, dev)
    dx = ops.conv_dgrad(dya, pw, kind, (H, W))
    close(dx, gx, dt, 'dx')
    if bf and kind != '3x3up':
        elem_bound(dx, gx, gxa, 'dx')
    elif bf:
        # behind the nearest x2 upsample the data gradient is ONE 4x4 / stride-2 conv over dy whose operand holds SUMS of
        # up to four weights (sba_pack_weight mode 3), formed in f32 from the master weights and rounded once: the
        # storage-rounded operand of this launch is that tensor, not the per-tap rounded weights behind gx.  So the
        # operand is pinned at one rounding of the float64 tap sums, and dx at the elementwise bound on the operand.
        wd = pw.dgrad(dt, kind).float().cpu().view(Cin, 16, Cout).double()
        S = [[2], [1, 2], [0, 1], [0]]
        wm = w.double()                                                     # [Cout][Cin][kh][kw]
        wsum = torch.stack([sum(wm[:, :, kh, kw] for kh in S[t // 4] for kw in S[t % 4]).t() for t in range(16)], 1)
        wabs = torch.stack([sum(wm[:, :, kh, kw].abs() for kh in S[t // 4] for kw in S[t % 4]).t() for t in range(16)], 1)
        assert bool(((wd - wsum).abs() <= CR.U_BF16 * wsum.abs() + 2.0 ** -22 * wabs).all()), 'mode-3 operand'
        g4 = CR.geom(N, 2 * H, 2 * W, Cout, H, W, Cin, [(t // 4 - 1, t % 4 - 1) for t in range(16)], sy=2)
        dyn = dyr.permute(0, 2, 3, 1).contiguous()
        elem_bound(dx.permute(0, 2, 3, 1), CR.contract(dyn, wd, g4), CR.contract(dyn.abs(), wd.abs(), g4), 'dx (4x4 collapse)')
    ops.conv_wgrad(xa, dya, wp, kind)
    ops.conv_wgrad(xa, dya, wp, kind)        # accumulates: twice -> 2x
    torch.cuda.synchronize()
    dw_close(wp.grad * 0.5, 'dw')
    # a parameter whose cleared gradient buffer is tracked (trainer.FlatParams): the first launch may STORE
    # (sba_conv_geom.first_write), the second accumulates; a clear + epoch bump re-arms the store
    wq = torch.nn.Parameter(w.to(dev).contiguous(memory_format=torch.channels_last))
    wq.grad = torch.zeros_like(wq)
    wq._sba_gepoch = [1]
    ops.conv_wgrad(xa, dya, wq, kind)
    assert wq._sba_wepoch == 1
    ops.conv_wgrad(xa, dya, wq, kind)
    torch.cuda.synchronize()
    dw_close(wq.grad * 0.5, 'dw (first write + accumulate)')
    wq.grad.zero_()
    wq._sba_gepoch[0] += 1
    ops.conv_wgrad(xa, dya, wq, kind)
    torch.cuda.synchronize()
    dw_close(wq.grad, 'dw (first write after a clear)')


@pytest.mark.parametrize('dt', DTYPES)
def test_conv_addend_epilogue(dev, dt):
    from sbagan import ops
    x, w = fill.unit((2, 64, 8, 8), 1), fill.unit((64, 64, 3, 3), 2) / 24
    add = fill.unit((2, 64, 8, 8), 3)
    wp = torch.nn.Parameter(w.to(dev).contiguous(memory_format=torch.channels_last))
    dx = ops.conv_dgrad(act(x, dt, dev), ops.PackedWeight(wp), '3x3', (8, 8), addend=act(add, dt, dev))
    ref = F.conv_transpose2d(rounded(x, dt), rounded(w, dt), None, 1, 1) + rounded(add, dt)
    close(dx, ref, dt, 'dgrad+addend')


@pytest.mark.parametrize('case', [(2, 64, 128, 16, 16), (3, 128, 320, 8, 8), (20, 512, 1024, 8, 8), (5, 64, 64, 6, 10)])
def test_dgrad4_grouped_plans(dev, case):
    """the four parity classes of the 4x4 / stride-2 data gradient as ONE grouped launch (sba_conv_igemm_group_splitk):
    every tile and K split the host may plan, with and without an addend, against conv_transpose2d and against the
    four single launches"""
    from sbagan import ops
    dt = torch.bfloat16
    N, Cin, Cout, H, W = case
    w = fill.unit((Cout, Cin, 4, 4), 2) / np.sqrt(Cin * 16)
    dy = fill.unit((N, Cout, H // 2, W // 2), 3)
    add = fill.unit((N, Cin, H, W), 4)
    wp = torch.nn.Parameter(w.to(dev).contiguous(memory_format=torch.channels_last))
    pw = ops.PackedWeight(wp)
    ref = F.conv_transpose2d(rounded(dy, dt), rounded(w, dt), None, 2, 1)
    dya, adda = act(dy, dt, dev), act(add, dt, dev)
    old = (ops.DGRAD4_GROUP, ops._DGRAD4_FORCE)
    try:
        ops.DGRAD4_GROUP = False
        single = ops.conv_dgrad(dya, pw, '4x4s2', (H, W)).float().cpu()
        ops.DGRAD4_GROUP = True
        for plan in [None, '1,1', '3,1', '5,1', '1,2', '3,3', '5,4', '1,8']:
            ops._DGRAD4_FORCE = plan
            dx = ops.conv_dgrad(dya, pw, '4x4s2', (H, W))
            close(dx, ref, dt, 'dx plan %s' % plan)
            if plan in ('1,1', '3,1', '5,1'):       # no K split: the same sums in the same order as a single launch
                assert torch.equal(dx.float().cpu(), single) or (dx.float().cpu() - single).abs().max() < 1e-2
            dxa = ops.conv_dgrad(dya, pw, '4x4s2', (H, W), addend=adda)
            close(dxa, ref + rounded(add, dt), dt, 'dx + addend plan %s' % plan)
        # the split-K workspace is left zero-filled
        torch.cuda.synchronize()
        assert int(ops.workspace(dev).count_nonzero()) == 0
    finally:
        ops.DGRAD4_GROUP, ops._DGRAD4_FORCE = old


def test_conv_addend_epilogue_halo_tile(dev):
    """the halo-tile kernel (conv3x3_halo3_kernel, 512 tiles) with the residual-add epilogue (ResBlock skip gradient)"""
    from sbagan import ops
    dt = torch.bfloat16
    x, w = fill.unit((8, 64, 128, 128), 1), fill.unit((64, 64, 3, 3), 2) / 24
    add = fill.unit((8, 64, 128, 128), 3)
    wp = torch.nn.Parameter(w.to(dev).contiguous(memory_format=torch.channels_last))
    dx = ops.conv_dgrad(act(x, dt, dev), ops.PackedWeight(wp), '3x3', (128, 128), addend=act(add, dt, dev))
    ref = F.conv_transpose2d(rounded(x, dt), rounded(w, dt), None, 1, 1) + rounded(add, dt)
    close(dx, ref, dt, 'dgrad+addend')


# ------------------------------------------------------------------ the image encoder's conv geometries
# (KH, KW, stride, pad_h, pad_w, input size): every distinct BasicConv2d shape of the Inception-v3 trunk
# (model.py:170-267).  The module-level test (test_step_gpu.py::test_image_encoder_hip_vs_torch) pins the graph in f32;
# in bf16 ReLU-mask flips blur the image gradient, so the bf16 kernels and the operand packing of
# sbagan.inception_hip._Conv (BN fold, channel padding to 32, flipped / parity-split data-gradient taps) are pinned
# here per geometry, elementwise-tight, on inputs already rounded to the storage type.
INCEPTION_GEOMS = [
    (1, 1, 1, 0, 0, 17), (3, 3, 2, 0, 0, 35), (3, 3, 1, 0, 0, 19), (3, 3, 1, 1, 1, 17), (5, 5, 1, 2, 2, 17),
    (1, 7, 1, 0, 3, 17), (7, 1, 1, 3, 0, 17), (1, 3, 1, 0, 1, 8), (3, 1, 1, 1, 0, 8), (3, 3, 2, 0, 0, 17),
]


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('geom', INCEPTION_GEOMS)
def test_inception_conv_geometries(dev, dt, geom):
    import ctypes
    from sbagan import _lib, ops
    from sbagan.inception_hip import _Conv, _geom
    KH, KW, s, ph, pw, S = geom
    N, I, O = 2, 80, 112                     # 80 input channels: padded to 96 inside the packed operands
    conv = torch.nn.Conv2d(I, O, (KH, KW), stride=s, padding=(ph, pw), bias=False)
    bn = torch.nn.BatchNorm2d(O, eps=1e-3).eval()
    with torch.no_grad():
        conv.weight.copy_(fill.unit((O, I, KH, KW), 11) / np.sqrt(I * KH * KW))
        bn.weight.copy_(1.0 + 0.2 * fill.uniform((O,), 12))
        bn.bias.copy_(0.1 * fill.uniform((O,), 13))
        bn.running_mean.copy_(0.1 * fill.uniform((O,), 14))
        bn.running_var.copy_(1.0 + 0.3 * fill.uniform((O,), 15))
    L = _Conv(conv.to(dev), bn.to(dev), dt, relu=True)
    dtc = _lib.SBA_BF16 if dt == torch.bfloat16 else _lib.SBA_F32
    ws = ops.workspace(dev)

    def igemm(x, w, y, bias, g):
        _lib.call('sba_conv_igemm_bias', dtc, x.data_ptr(), w.data_ptr(), y.data_ptr(), None, None,
                  None if bias is None else bias.data_ptr(), None, ctypes.byref(g), ws.data_ptr(),
                  ops.WORKSPACE_BYTES, ops._stream())

    x = fill.unit((N, I, S, S), 16)
    xa = torch.zeros((N, S, S, L.Ip), dtype=dt, device=dev)
    xa[..., :I] = x.permute(0, 2, 3, 1).to(dev).to(dt)
    OH, OW = (S + 2 * ph - KH) // s + 1, (S + 2 * pw - KW) // s + 1
    y = torch.empty((N, OH, OW, L.Op), dtype=dt, device=dev)
    taps = [(t // KW - ph, t % KW - pw) for t in range(KH * KW)]
    igemm(xa, L.w_fwd, y, L.bias, _geom(N, S, S, L.Ip, OH, OW, L.Op, taps, sy=s, xcs=L.Ip, ycs=L.Op, relu=1))
    torch.cuda.synchronize()
    # reference on the operands the kernel sees: the folded weight rounded to the storage type, f32 bias
    wf = L.w_fwd.float().cpu()[:O, :, :I].reshape(O, KH, KW, I).permute(0, 3, 1, 2).contiguous()
    xr = rounded(x, dt).requires_grad_(True)
    pre = F.conv2d(xr, wf, None, s, (ph, pw))
    yr = torch.relu(pre + L.bias.cpu()[:O].view(1, -1, 1, 1))
    close(y[..., :O].permute(0, 3, 1, 2), yr, dt, 'y')
    assert float(y[..., O:].float().abs().max()) == 0.0, 'padded output channels'
    # data gradient of the linear part (the ReLU mask is a separate pass / epilogue, tested with the module)
    dy = fill.unit((N, O, OH, OW), 17)
    dyr = rounded(dy, dt)
    (gx_ref,) = torch.autograd.grad(pre, xr, dyr)
    dya = torch.zeros((N, OH, OW, L.Op), dtype=dt, device=dev)
    dya[..., :O] = dy.permute(0, 2, 3, 1).to(dev).to(dt)
    gx = torch.zeros((N, S, S, L.Ip), dtype=dt, device=dev)
    if s == 1:
        igemm(dya, L.w_dgrad[0], gx, None, _geom(N, OH, OW, L.Op, S, S, L.Ip, L.dtaps[0], xcs=L.Op, ycs=L.Ip))
    else:
        for cls in range(4):
            py, px = cls // 2, cls % 2
            OHs, OWs = (S - py + 1) // 2, (S - px + 1) // 2
            if OHs <= 0 or OWs <= 0 or not L.dtaps[cls]:
                continue
            igemm(dya, L.w_dgrad[cls], gx, None, _geom(N, OH, OW, L.Op, S, S, L.Ip, L.dtaps[cls], OHs=OHs, OWs=OWs,
                                                       osy=2, ooy=py, oox=px, xcs=L.Op, ycs=L.Ip))
    torch.cuda.synchronize()
    close(gx[..., :I].permute(0, 3, 1, 2), gx_ref, dt, 'dx')


@pytest.mark.parametrize('geom', [(32, 32, 0, 149, 2), (32, 64, 1, 147, 2), (80, 192, 0, 73, 6), (64, 96, 1, 67, 5)])
def test_register_weight_halo_kernel_general(dev, geom):
    """conv3x3_halo3g_kernel (fragment-major weights, include/sbagan_hip.h: w_layout = 1) on the geometries of the
    Inception trunk's first 3 x 3 layers -- 'valid' and 'same' windows, ragged maps, 32- and 64-channel chunks, 32 / 64
    output channels per workgroup -- forward (bias + ReLU) and data gradient (addend + ReLU mask) against F.conv2d and
    against the implicit-GEMM kernels on row-major weights (same products, another summation order)."""
    import ctypes
    from sbagan import _lib, ops
    from sbagan.inception_hip import _Conv, _geom
    I, O, pad, S, N = geom
    dt = torch.bfloat16
    conv = torch.nn.Conv2d(I, O, 3, stride=1, padding=pad, bias=False)
    bn = torch.nn.BatchNorm2d(O, eps=1e-3).eval()
    with torch.no_grad():
        conv.weight.copy_(fill.unit((O, I, 3, 3), 21) / np.sqrt(I * 9))
        bn.weight.copy_(1.0 + 0.2 * fill.uniform((O,), 22))
        bn.bias.copy_(0.1 * fill.uniform((O,), 23))
        bn.running_mean.copy_(0.1 * fill.uniform((O,), 24))
        bn.running_var.copy_(1.0 + 0.3 * fill.uniform((O,), 25))
    L = _Conv(conv.to(dev), bn.to(dev), dt, relu=True)
    ws = ops.workspace(dev)

    def frag(w):
        R, taps, K = w.shape
        dst = torch.zeros((R + 63) // 64 * 64 * taps * K, dtype=w.dtype, device=dev)
        ops._pack_frag([(w, dst, R, taps, K)], dev)
        return dst

    def run(x, w, y, bias, g, layout, addend=None, mask=None):
        g.w_layout = layout
        plan = (ctypes.c_int * 3)()
        _lib.call('sba_conv_igemm_plan', _lib.SBA_BF16, ctypes.byref(g), ops.WORKSPACE_BYTES, plan)
        _lib.call('sba_conv_igemm_bias', _lib.SBA_BF16, x.data_ptr(), w.data_ptr(), y.data_ptr(),
                  None if addend is None else addend.data_ptr(), None, None if bias is None else bias.data_ptr(),
                  None if mask is None else mask.data_ptr(), ctypes.byref(g), ws.data_ptr(), ops.WORKSPACE_BYTES,
                  ops._stream())
        g.w_layout = 0
        return plan[0]

    x = fill.unit((N, I, S, S), 26)
    xa = torch.zeros((N, S, S, L.Ip), dtype=dt, device=dev)
    xa[..., :I] = x.permute(0, 2, 3, 1).to(dev).to(dt)
    OH = OW = S + 2 * pad - 2
    taps = [(t // 3 - pad, t % 3 - pad) for t in range(9)]
    g = _geom(N, S, S, L.Ip, OH, OW, L.Op, taps, xcs=L.Ip, ycs=L.Op, relu=1)
    y0 = torch.empty((N, OH, OW, L.Op), dtype=dt, device=dev)
    y1 = torch.full((N, OH, OW, L.Op), float('nan'), dtype=dt, device=dev)
    assert run(xa, L.w_fwd, y0, L.bias, g, 0) != 4
    assert run(xa, frag(L.w_fwd), y1, L.bias, g, 1) in (0, 4)
    torch.cuda.synchronize()
    wf = L.w_fwd.float().cpu()[:O, :, :I].reshape(O, 3, 3, I).permute(0, 3, 1, 2).contiguous()
    xr = rounded(x, dt).requires_grad_(True)
    pre = F.conv2d(xr, wf, None, 1, pad)
    close(y1[..., :O].permute(0, 3, 1, 2), torch.relu(pre + L.bias.cpu()[:O].view(1, -1, 1, 1)), dt, 'y')
    assert rel_l2(y1.float().cpu(), y0.float().cpu()) < 1e-3, 'register-weight kernel vs implicit GEMM'
    assert float(y1[..., O:].float().abs().max()) == 0.0 if L.Op > O else True, 'padded output channels'
    # data gradient with an addend and the ReLU mask of the tensor it completes
    dy = fill.unit((N, O, OH, OW), 27)
    (gx_ref,) = torch.autograd.grad(pre, xr, rounded(dy, dt))
    dya = torch.zeros((N, OH, OW, L.Op), dtype=dt, device=dev)
    dya[..., :O] = dy.permute(0, 2, 3, 1).to(dev).to(dt)
    add = fill.unit((N, S, S, L.Ip), 28).to(dev).to(dt)
    mask = fill.unit((N, S, S, L.Ip), 29).to(dev).to(dt)
    gd = _geom(N, OH, OW, L.Op, S, S, L.Ip, L.dtaps[0], xcs=L.Op, ycs=L.Ip)
    gx0 = torch.zeros((N, S, S, L.Ip), dtype=dt, device=dev)
    gx1 = torch.full((N, S, S, L.Ip), float('nan'), dtype=dt, device=dev)
    run(dya, L.w_dgrad[0], gx0, None, gd, 0, addend=add, mask=mask)
    assert run(dya, frag(L.w_dgrad[0]), gx1, None, gd, 1, addend=add, mask=mask) in (0, 4)
    torch.cuda.synchronize()
    want = (gx_ref + add.float().cpu()[..., :I].permute(0, 3, 1, 2)) * (mask.float().cpu()[..., :I].permute(0, 3, 1, 2) > 0)
    close(gx1[..., :I].permute(0, 3, 1, 2), want, dt, 'dx')
    assert rel_l2(gx1.float().cpu(), gx0.float().cpu()) < 1e-3, 'data gradient: register-weight kernel vs implicit GEMM'


# ------------------------------------------------------------------ every bf16 tile configuration, forced
# sba_conv_geom.tile / .ksplit (include/sbagan_hip.h) pick the kernel instantiation; the measured table only ever uses a
# few per shape, so each id is forced here on the weight-streaming shapes of the discriminator tails (model.py:560-607:
# 4x4 maps, M = 16 B rows): one full 320-row tile, a ragged one (B - 1 = 19 images), two M tiles, a ragged 5x5 map.
# The last two have Cin % 64 == 32: ids 1..12 are then the first-generation LDS-DMA kernels (32-channel slabs).
SKINNY_CASES = [(20, 4, 128, 192), (19, 4, 64, 72), (40, 4, 128, 64), (7, 5, 192, 136), (20, 4, 96, 192), (7, 5, 160, 72)]


@pytest.mark.parametrize('case', SKINNY_CASES)
def test_igemm_every_tile_configuration(dev, case):
    import ctypes
    from sbagan import _lib, ops
    from sbagan.inception_hip import _geom
    N, S, I, O = case
    dt = torch.bfloat16
    x = fill.unit((N, I, S, S), 21)
    w = fill.unit((O, I, 3, 3), 22) / np.sqrt(9 * I)
    bias = 0.1 * fill.uniform((O,), 23)
    ref = torch.relu(F.conv2d(rounded(x, dt), rounded(w, dt), bias, 1, 1))
    xa = x.permute(0, 2, 3, 1).contiguous().to(dev).to(dt)
    wa = w.permute(0, 2, 3, 1).contiguous().to(dev).to(dt)          # [Cout][tap][Cin]
    ba = bias.to(dev)
    ws = ops.workspace(dev)
    taps = [(t // 3 - 1, t % 3 - 1) for t in range(9)]
    for tile in range(1, _lib.IGEMM_TILES + 1):
        for ksplit in (1, 3):
            g = _geom(N, S, S, I, S, S, O, taps, relu=1)
            g.tile, g.ksplit = tile, ksplit
            y = torch.full((N, S, S, O), 7.0, dtype=dt, device=dev)
            _lib.call('sba_conv_igemm_bias', _lib.SBA_BF16, xa.data_ptr(), wa.data_ptr(), y.data_ptr(), None, None,
                      ba.data_ptr(), None, ctypes.byref(g), ws.data_ptr(), ops.WORKSPACE_BYTES, ops._stream())
            torch.cuda.synchronize()
            close(y.permute(0, 3, 1, 2), ref, dt, 'tile %d split %d' % (tile, ksplit))


@pytest.mark.parametrize('dt', DTYPES)
def test_maxpool3x3s2_pairs(dev, dt):
    """max_pool2d(3, 2) of the image encoder (model.py:215,221 and the reduction blocks): forward, the backward that
    re-derives the argmax from x, and the pair that keeps the argmax (one byte per element) -- on a channel slice of a
    wider NHWC tensor, accumulating into an existing gradient, with ties (torch's rule: first maximum in scan order)."""
    from sbagan import _lib
    from sbagan import ops
    N, C, H, W, Ct, co = 2, 32, 19, 17, 48, 8
    dtc = _lib.SBA_BF16 if dt == torch.bfloat16 else _lib.SBA_F32
    x = (fill.uniform((N, C, H, W), 31) * 4).round() / 4           # quantised: plenty of exact ties
    xr = rounded(x, dt).requires_grad_(True)
    yr = F.max_pool2d(xr, 3, 2)
    OH, OW = yr.shape[2:]
    dy = rounded(fill.unit((N, C, OH, OW), 32), dt)
    (gref,) = torch.autograd.grad(yr, xr, dy)
    base = rounded(fill.unit((N, C, H, W), 33), dt)                 # existing gradient to accumulate into
    xa = torch.zeros((N, H, W, Ct), dtype=dt, device=dev)
    xa[..., co:co + C] = x.permute(0, 2, 3, 1).to(dev).to(dt)
    dya = dy.permute(0, 2, 3, 1).contiguous().to(dev).to(dt)
    st = ops._stream()
    for keep in (False, True):
        y = torch.empty((N, OH, OW, C), dtype=dt, device=dev)
        gx = torch.zeros((N, H, W, Ct), dtype=dt, device=dev)
        gx[..., co:co + C] = base.permute(0, 2, 3, 1).to(dev).to(dt)
        if keep:
            arg = torch.empty((N, OH, OW, C), dtype=torch.uint8, device=dev)
            _lib.call('sba_maxpool3x3s2_fwd_arg', dtc, xa.data_ptr(), y.data_ptr(), arg.data_ptr(), N, H, W, C, Ct, co,
                      C, 0, st)
            _lib.call('sba_maxpool3x3s2_bwd_arg', dtc, arg.data_ptr(), dya.data_ptr(), gx.data_ptr(), N, H, W, C, C, 0,
                      Ct, co, 1, None, st)
            # the same with the ReLU mask of the pooled tensor folded in (x doubles as the mask: zeroed where x <= 0)
            gm = torch.zeros((N, H, W, Ct), dtype=dt, device=dev)
            gm[..., co:co + C] = base.permute(0, 2, 3, 1).to(dev).to(dt)
            _lib.call('sba_maxpool3x3s2_bwd_arg', dtc, arg.data_ptr(), dya.data_ptr(), gm.data_ptr(), N, H, W, C, C, 0,
                      Ct, co, 1, xa.data_ptr(), st)
            torch.cuda.synchronize()
            want = gx[..., co:co + C] * (xa[..., co:co + C] > 0)
            assert torch.equal(gm[..., co:co + C], want), 'masked maxpool backward'
        else:
            _lib.call('sba_maxpool3x3s2_fwd', dtc, xa.data_ptr(), y.data_ptr(), N, H, W, C, Ct, co, C, 0, st)
            _lib.call('sba_maxpool3x3s2_bwd', dtc, xa.data_ptr(), dya.data_ptr(), gx.data_ptr(), N, H, W, C, Ct, co, C, 0,
                      Ct, co, 1, st)
        torch.cuda.synchronize()
        assert torch.equal(y.float().cpu().permute(0, 3, 1, 2), yr.detach()), 'max is exact'
        close(gx[..., co:co + C].permute(0, 3, 1, 2), gref + base, dt, 'dx keep=%s' % keep)
        assert float(gx[..., :co].float().abs().max()) == 0.0 and float(gx[..., co + C:].float().abs().max()) == 0.0


@pytest.mark.parametrize('dt', DTYPES)
def test_stem_conv_on_the_resized_image(dev, dt):
    """Conv2d_1a_3x3 reading the 299 x 299 bilinear resize on the fly (sba_enc_stem_resize_fwd) against the two launches
    it replaces (sba_resize_bilinear + sba_enc_stem_fwd) and against F.interpolate + F.conv2d (model.py:210-213)."""
    from sbagan import _lib, ops
    N, S, D, C = 3, 64, 75, 32
    dtc = _lib.SBA_BF16 if dt == torch.bfloat16 else _lib.SBA_F32
    img = fill.unit((N, 3, S, S), 41)
    w = fill.unit((C, 3, 3, 3), 42) / 5
    b = fill.unit((C,), 43) / 10
    st = ops._stream()
    imga = img.to(dev)
    wa = w.to(dev).contiguous(memory_format=torch.channels_last)
    ba = b.to(dev)
    O = (D - 3) // 2 + 1
    x = torch.empty((N, 3, D, D), dtype=torch.float32, device=dev)
    y2 = torch.empty((N, O, O, C), dtype=dt, device=dev)
    y1 = torch.full((N, O, O, C), float('nan'), dtype=dt, device=dev)
    _lib.call('sba_resize_bilinear', imga.data_ptr(), x.data_ptr(), N * 3, S, D, 0, st)
    _lib.call('sba_enc_stem_fwd', dtc, x.data_ptr(), wa.data_ptr(), ba.data_ptr(), y2.data_ptr(), N, D, C, st)
    _lib.call('sba_enc_stem_resize_fwd', dtc, imga.data_ptr(), wa.data_ptr(), ba.data_ptr(), y1.data_ptr(), N, S, D, C, st)
    torch.cuda.synchronize()
    ref = torch.relu(F.conv2d(F.interpolate(img, size=(D, D), mode='bilinear', align_corners=True), w, b, stride=2))
    close(y1.permute(0, 3, 1, 2), ref, dt, 'fused stem')
    assert rel_l2(y1.float().cpu(), y2.float().cpu()) < (2e-3 if dt == torch.bfloat16 else 1e-6), 'fused vs two launches'
    # no bias: the raw conv output of the training-mode trunk (no ReLU either)
    _lib.call('sba_enc_stem_resize_fwd', dtc, imga.data_ptr(), wa.data_ptr(), None, y1.data_ptr(), N, S, D, C, st)
    torch.cuda.synchronize()
    ref = F.conv2d(F.interpolate(img, size=(D, D), mode='bilinear', align_corners=True), w, None, stride=2)
    close(y1.permute(0, 3, 1, 2), ref, dt, 'fused stem, raw')


@pytest.mark.parametrize('shape', [(20, 200, 16384), (20, 100, 512), (3, 256, 2080), (40, 200, 4096)])
def test_dense_layers_all_widths(dev, shape):
    """sba_linear_fwd / sba_linear_bwd (nn.Linear; model.py:278,306-313,330,354): the batch <= 32 layers on the f32 matrix
    cores at every width -- INIT_STAGE_G.fc has 16384 columns -- and the wave-per-row kernels beyond batch 32, against
    torch; dW and db accumulate."""
    from sbagan import _lib, ops
    B, K, N = shape
    x, w, b = fill.unit((B, K), 71), fill.unit((N, K), 72) / np.sqrt(K), fill.unit((N,), 73)
    dy = fill.unit((B, N), 74)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    yref = F.linear(xr, wr, br)
    gx, gw, gb = torch.autograd.grad(yref, [xr, wr, br], dy)
    st = ops._stream()
    xa, wa, ba, dya = x.to(dev), w.to(dev), b.to(dev), dy.to(dev)
    y = torch.empty((B, N), dtype=torch.float32, device=dev)
    _lib.call('sba_linear_fwd', xa.data_ptr(), wa.data_ptr(), ba.data_ptr(), y.data_ptr(), B, K, N, st)
    dx = torch.full((B, K), float('nan'), dtype=torch.float32, device=dev)
    dw = torch.ones((N, K), dtype=torch.float32, device=dev)
    db = torch.ones((N,), dtype=torch.float32, device=dev)
    _lib.call('sba_linear_bwd', xa.data_ptr(), wa.data_ptr(), dya.data_ptr(), dx.data_ptr(), dw.data_ptr(), db.data_ptr(),
              B, K, N, st)
    torch.cuda.synchronize()
    assert rel_l2(y.cpu(), yref.detach()) < 1e-5
    assert rel_l2(dx.cpu(), gx) < 1e-5
    assert rel_l2(dw.cpu() - 1.0, gw) < 1e-5
    assert rel_l2(db.cpu() - 1.0, gb) < 1e-5


@pytest.mark.parametrize('sd', [(64, 75), (256, 299), (17, 17), (5, 64)])
def test_resize_backward_is_the_adjoint(dev, sd):
    """sba_resize_bilinear(backward): the gather form of the adjoint of F.interpolate(bilinear, align_corners=True)
    (model.py:210), with the candidates of every input index tabulated per workgroup, against autograd"""
    from sbagan import _lib, ops
    S, D = sd
    NC = 6
    x = fill.unit((2, 3, S, S), 61).requires_grad_(True)
    y = F.interpolate(x, size=(D, D), mode='bilinear', align_corners=True)
    dy = fill.unit((2, 3, D, D), 62)
    (gref,) = torch.autograd.grad(y, x, dy)
    dya = dy.to(dev).contiguous()
    dx = torch.full((2, 3, S, S), float('nan'), dtype=torch.float32, device=dev)
    _lib.call('sba_resize_bilinear', dya.data_ptr(), dx.data_ptr(), NC, S, D, 1, ops._stream())
    torch.cuda.synchronize()
    # (source coordinates up to S - 1 in f32: one ulp of 255 is 1.5e-5 of a pixel, and so is the interpolation weight)
    assert rel_l2(dx.cpu(), gref) < 3e-5, rel_l2(dx.cpu(), gref)
    ya = torch.empty((2, 3, D, D), dtype=torch.float32, device=dev)
    _lib.call('sba_resize_bilinear', x.detach().to(dev).contiguous().data_ptr(), ya.data_ptr(), NC, S, D, 0, ops._stream())
    torch.cuda.synchronize()
    assert rel_l2(ya.cpu(), y.detach()) < 3e-5


@pytest.mark.parametrize('S', [75, 40, 299])
def test_stem_backward_matrix_cores(dev, S):
    """sba_enc_stem_bwd for bf16 features (enc_stem_bwd_mfma_kernel: the 3x3 / stride-2 stem's data gradient as a 2 x 2
    conv of dpre with 12 "channels" on the matrix cores) against autograd through F.conv2d + ReLU (model.py:212), odd and
    even image sizes, ragged 16-block tiles."""
    from sbagan import _lib, ops
    N, C = 2, 32
    dt = torch.bfloat16
    x = fill.unit((N, 3, S, S), 51)
    w = fill.unit((C, 3, 3, 3), 52) / 5
    b = fill.unit((C,), 53) / 10
    xr = x.clone().requires_grad_(True)
    y = torch.relu(F.conv2d(xr, w, b, stride=2))
    O = y.shape[2]
    dy = rounded(fill.unit((N, C, O, O), 54), dt)
    # the kernel sees the bf16 features: the mask is out > 0 of the ROUNDED output
    yb = rounded(y.detach(), dt)
    pre = F.conv2d(xr, w, b, stride=2)
    (gref,) = torch.autograd.grad(pre, xr, dy * (yb > 0))
    st = ops._stream()
    wa = w.to(dev).contiguous(memory_format=torch.channels_last)
    outa = yb.permute(0, 2, 3, 1).contiguous().to(dev).to(dt)
    dya = dy.permute(0, 2, 3, 1).contiguous().to(dev).to(dt)
    dimg = torch.full((N, 3, S, S), float('nan'), dtype=torch.float32, device=dev)
    _lib.call('sba_enc_stem_bwd', _lib.SBA_BF16, wa.data_ptr(), outa.data_ptr(), dya.data_ptr(), dimg.data_ptr(), N, S, C, st)
    torch.cuda.synchronize()
    assert torch.isfinite(dimg).all(), 'every image pixel is written'
    assert rel_l2(dimg.cpu(), gref) < 1e-5, rel_l2(dimg.cpu(), gref)


# ------------------------------------------------------------------ fused blocks vs the oracle
def _load(mod, P, dev):
    mod.load_state_dict(P)
    return mod.to(dev).train()


def _grads_of(mod):
    return {n: p.grad for n, p in mod.named_parameters()}


def _oracle_P(P, prefix=''):
    Q = {}
    for k, v in P.items():
        Q[prefix + k] = v.clone().requires_grad_(True) if k.endswith(('.weight', '.bias')) else v.clone()
    return Q


def _check_module(mod, Q, dt, prefix, buffers=True, gscale=1.0):
    """float32: every gradient tensor elementwise.  bfloat16: the concatenation of all gradients
    in relative L2 (<= 2e-2 * gscale) plus a loose per-tensor bound -- some tensors (e.g. the
    beta gradient of a BatchNorm that feeds another BatchNorm) are sums of almost cancelling
    terms, whose relative error under 8-bit mantissas is large although every summand is fine."""
    got, ref = [], []
    for n, p in mod.named_parameters():
        r = Q[prefix + n].grad
        if r is None:
            continue
        if dt == torch.float32:
            close(p.grad, r, dt, 'grad ' + n, scale=gscale)
        else:
            assert rel_l2(p.grad, r) <= 0.35, ('grad ' + n, rel_l2(p.grad, r))
            got.append(p.grad.detach().float().cpu().flatten())
            ref.append(r.detach().float().flatten())
    if got:
        assert rel_l2(torch.cat(got), torch.cat(ref)) <= 2e-2 * gscale, rel_l2(torch.cat(got), torch.cat(ref))
    if buffers:
        for n, b in mod.named_buffers():
            if n.endswith(('running_mean', 'running_var')):
                close(b, Q[prefix + n], dt if dt == torch.float32 else torch.bfloat16, 'buffer ' + n)
            elif n.endswith('num_batches_tracked'):
                assert int(b) == int(Q[prefix + n]), n


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('which', ['up', 'leak', 'down', 'res'])
def test_conv_bn_act_blocks(dev, dt, which):
    from sbagan import nets, ops
    ops.set_compute_dtype(dt)
    N, C, H = 3, 64, 8
    if which == 'up':
        mod, fn = nets.upBlock(C, C // 2), lambda x, Q: O.up_block(x, Q, 'm')
    elif which == 'leak':
        mod, fn = nets.Block3x3_leakRelu(C, 128), lambda x, Q: O._block3x3_leak(x, Q, 'm', True)
    elif which == 'down':
        mod, fn = nets.downBlock(C, 128), lambda x, Q: O._down(x, Q, 'm', 0, 1, True)
    else:
        mod, fn = nets.ResBlock(C), lambda x, Q: O.res_block(x, Q, 'm')
    P = fill.fill_state_dict({k: tuple(v.shape) for k, v in mod.state_dict().items()})
    _load(mod, P, dev)
    x = fill.unit((N, C, H, H), 5)
    xr = rounded(x, dt).requires_grad_(True)
    Q = _oracle_P(P, 'm.')
    yref = fn(xr, Q)
    dy = fill.unit(tuple(yref.shape), 6)
    yref.backward(rounded(dy, dt))
    xa = act(x, dt, dev).requires_grad_(True)
    y = mod(xa)
    y.backward(act(dy, dt, dev))
    torch.cuda.synchronize()
    assert y.dtype == dt and y.is_contiguous(memory_format=torch.channels_last)
    close(y, yref, dt, 'out', scale=3)
    close(xa.grad, xr.grad, dt, 'dx', scale=3)
    _check_module(mod, Q, dt, 'm.', gscale=3)


@pytest.mark.parametrize('which', ['up', 'leak', 'down', 'res'])
def test_conv_bn_act_blocks_binary16_conv_output(dev, which):
    """SBA_Y_F16=1 / SBA_BF16_YH: the raw conv output between the conv epilogue and the BatchNorm kernels stored as IEEE
    binary16 instead of bf16 (forward, both backward passes, grouped and fused variants go through the same blocks)."""
    from sbagan import ops
    was = ops.Y_F16
    ops.Y_F16 = True
    try:
        test_conv_bn_act_blocks(dev, torch.bfloat16, which)
        if which == 'leak':
            test_grouped_real_fake_pass_equals_two_calls(dev, torch.bfloat16)
    finally:
        ops.Y_F16 = was


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('mask_mode', [0, 1])
def test_word_attention(dev, dt, mask_mode):
    from sbagan import nets, ops
    ops.set_compute_dtype(dt)
    B, idf, cdf, L, H = 3, 32, 256, 7, 12
    att = nets.GlobalAttentionGeneral(idf, cdf)
    P = fill.fill_state_dict({'conv_context.weight': (idf, cdf, 1, 1)})
    _load(att, P, dev)
    att.reference_mask_order = (mask_mode == 0)
    h, words = fill.unit((B, idf, H, H), 1), fill.unit((B, cdf, L), 2)
    caps, _ = fill.synthetic_captions(B, L, L, tag=3)
    mask = (caps == 0)[:, :L]
    mask[1, 3:] = True
    hr = rounded(h, dt).requires_grad_(True)
    wq = P['conv_context.weight'].clone().requires_grad_(True)
    if mask_mode == 0:
        cref, aref = O.word_attention(hr, words, wq, mask)
    else:   # per-sample mask: plain masked attention
        src = torch.einsum('ic,bcl->bil', wq.view(idf, -1), words)
        s = torch.bmm(hr.reshape(B, idf, -1).transpose(1, 2), src).masked_fill(mask[:, None, :], -float('inf'))
        a = torch.softmax(s, 2).transpose(1, 2)
        cref, aref = torch.bmm(src, a).reshape(B, idf, H, H), a.reshape(B, L, H, H)
    dctx = fill.unit(tuple(cref.shape), 4)
    cref.backward(rounded(dctx, dt))
    ha = act(h, dt, dev).requires_grad_(True)
    att.applyMask(mask.to(dev))
    ctx, a = att(ha, words.to(dev))
    ctx.backward(act(dctx, dt, dev))
    torch.cuda.synchronize()
    # bool part of the quirk: exactly the reference's entries are masked out
    assert torch.equal((a.cpu() == 0), (aref.detach() == 0))
    close(ctx, cref, dt, 'ctx'); close(a, aref, dt, 'att', scale=2)
    close(ha.grad, hr.grad, dt, 'dh', scale=2)
    close(att.conv_context.weight.grad, wq.grad, dt, 'dW', scale=3)


@pytest.mark.parametrize('dt', DTYPES)
def test_adain_and_stage_entry(dev, dt):
    from sbagan import nets, ops
    from miscc.config import cfg
    ops.set_compute_dtype(dt)
    B, ngf, nef, L, H = 2, 32, 256, 6, 16
    st = nets.NEXT_STAGE_G(ngf, nef, 100)
    P = fill.fill_state_dict({k: tuple(v.shape) for k, v in st.state_dict().items()})
    _load(st, P, dev)
    h, w_code, words = fill.unit((B, ngf, H, H), 1), fill.unit((B, 256), 2), fill.unit((B, nef, L), 3)
    caps, _ = fill.synthetic_captions(B, L, L, tag=4)
    mask = (caps == 0)[:, :L]
    Q = _oracle_P(P, 'h_net2.')
    hr = rounded(h, dt).requires_grad_(True)
    wr = w_code.clone().requires_grad_(True)
    yref, aref = O.next_stage_g(hr, wr, words, mask, Q, 'h_net2')
    dy = fill.unit(tuple(yref.shape), 5)
    yref.backward(rounded(dy, dt))
    ha = act(h, dt, dev).requires_grad_(True)
    wa = w_code.to(dev).requires_grad_(True)
    y, a = st(ha, None, wa, words.to(dev), mask.to(dev))
    y.backward(act(dy, dt, dev))
    torch.cuda.synchronize()
    close(y, yref, dt, 'stage out', scale=4); close(a, aref, dt, 'att', scale=2)
    close(ha.grad, hr.grad, dt, 'dh', scale=5)
    close(wa.grad, wr.grad, dt, 'dw_code', scale=5)
    _check_module(st, Q, dt, 'h_net2.', gscale=5)
    # stand-alone ADAIN_NORM
    ad = st.adain
    ad.zero_grad()
    ha2 = act(h, dt, dev).requires_grad_(True)
    o = ad(ha2, w_code.to(dev))
    ref = O.adain_norm(rounded(h, dt), w_code, {k: v.detach() for k, v in Q.items()}, 'h_net2.adain')
    close(o, ref, dt, 'adain')


@pytest.mark.parametrize('dt', DTYPES)
def test_image_head_and_d_stem_and_logits(dev, dt):
    from sbagan import nets, ops
    ops.set_compute_dtype(dt)
    B, ngf, H = 2, 32, 20
    head = nets.GET_IMAGE_G(ngf)
    P = fill.fill_state_dict({'img.0.weight': (3, ngf, 3, 3)})
    _load(head, P, dev)
    h = fill.unit((B, ngf, H, H + 3), 1)
    hr = rounded(h, dt).requires_grad_(True)
    wq = P['img.0.weight'].clone().requires_grad_(True)
    ref = O.get_image_g(hr, {'m.img.0.weight': wq}, 'm')
    dimg = fill.unit(tuple(ref.shape), 2)
    ref.backward(dimg)
    ha = act(h, dt, dev).requires_grad_(True)
    img = head(ha)
    img.backward(dimg.to(dev))
    torch.cuda.synchronize()
    assert img.dtype == torch.float32 and img.is_contiguous()
    close(img, ref, dt, 'img'); close(ha.grad, hr.grad, dt, 'dh'); close(head.img[0].weight.grad, wq.grad, dt, 'dw', scale=2)

    # discriminator stem + full D_NET64 trunk + heads
    from miscc.config import cfg
    cfg.GAN.DF_DIM = 64
    d = nets.D_NET64()
    PD = fill.fill_state_dict({k: tuple(v.shape) for k, v in d.state_dict().items()})
    _load(d, PD, dev)
    x = fill.uniform((3, 3, 64, 64), 3)
    sent = fill.unit((3, 256), 4)
    Q = _oracle_P(PD)
    xr = x.clone().requires_grad_(True)
    fr = O.d_net(Q, xr)
    pr_c = O.d_get_logits(Q, 'COND_DNET', fr, sent)
    pr_u = O.d_get_logits(Q, 'UNCOND_DNET', fr)
    gl = fill.unit((3,), 5)
    ((pr_c * gl).sum() + (pr_u * gl * 0.5).sum()).backward()
    xa = x.to(dev).requires_grad_(True)
    f = d(xa)
    pc = d.COND_DNET(f, sent.to(dev))
    pu = d.UNCOND_DNET(f)
    ((pc * gl.to(dev)).sum() + (pu * gl.to(dev) * 0.5).sum()).backward()
    torch.cuda.synchronize()
    close(f, fr, dt, 'D feat', scale=3); close(pc, pr_c, dt, 'cond prob', scale=3); close(pu, pr_u, dt, 'uncond prob', scale=3)
    close(xa.grad, xr.grad, dt, 'dimg', scale=5)
    _check_module(d, Q, dt, '', gscale=5)


@pytest.mark.parametrize('shape', [(2, 16, 32), (3, 64, 64), (20, 128, 128), (1, 8, 96), (2, 12, 48)])
def test_image_head_matrix_cores(dev, shape):
    """GET_IMAGE_G (model.py:426-437), bf16 features, W % 32 == 0 and H % 8 == 0: forward and backward (dh and dw)
    on the bf16 matrix cores with hi + lo split f32 operands (the ragged 20 x 23 map of
    test_image_head_and_d_stem_and_logits and the 12 x 48 one here stay on the VALU kernels).
    dh is a bf16 tensor (2^-9 relative rounding per element), dw f32.  20 x 128 x 128: 1280 tiles on 1024 persistent
    workgroups, partial sums through the scratch ring; then the same launch accumulating into an existing dh."""
    from sbagan import _lib, nets, ops
    ops.set_compute_dtype(torch.bfloat16)
    N, H, W = shape
    ngf = 32
    h = rounded(fill.unit((N, ngf, H, W), 41), torch.bfloat16)
    w = fill.unit((3, ngf, 3, 3), 42) / np.sqrt(9 * ngf)
    dimg = fill.unit((N, 3, H, W), 43)
    hr, wr = h.clone().requires_grad_(True), w.clone().requires_grad_(True)
    ref = torch.tanh(F.conv2d(hr, wr, None, 1, 1))
    gh, gw = torch.autograd.grad(ref, [hr, wr], dimg)
    head = nets.GET_IMAGE_G(ngf)
    _load(head, {'img.0.weight': w}, dev)
    ha = act(h, torch.bfloat16, dev).requires_grad_(True)
    img = head(ha)
    img.backward(dimg.to(dev))
    torch.cuda.synchronize()
    assert rel_l2(img.cpu(), ref) <= 1e-4, rel_l2(img.cpu(), ref)       # forward: one 16x16x32 MFMA pair per tap
    # the kernel differentiates tanh at ITS forward value (f32 accumulation order differs from torch's conv in the last bits)
    assert rel_l2(ha.grad.float().cpu(), gh) <= 4e-3, rel_l2(ha.grad.float().cpu(), gh)
    assert rel_l2(head.img[0].weight.grad.cpu(), gw) <= 3e-4, rel_l2(head.img[0].weight.grad.cpu(), gw)
    # accumulate = 1: dh += ...
    dh = ha.grad.detach().clone()
    dw = torch.zeros_like(head.img[0].weight)
    _lib.call('sba_img_head_bwd', _lib.SBA_BF16, ha.data_ptr(), head.img[0].weight.data_ptr(), img.data_ptr(),
              dimg.to(dev).data_ptr(), dh.data_ptr(), dw.data_ptr(), N, H, W, ngf, 1, ops._stream())
    torch.cuda.synchronize()
    assert rel_l2(dh.float().cpu(), 2 * gh) <= 6e-3
    assert rel_l2(dw.cpu(), gw) <= 3e-4


@pytest.mark.parametrize('shape', [(3, 64), (2, 128), (3, 32), (1, 24), (2, 256)])
def test_d_stem_backward_matrix_cores(dev, shape):
    """encode_image_by_16times' first conv (model.py:563-564), bf16 activations: data and weight gradient on the bf16 matrix
    cores with hi + lo split f32 operands -- held to the torch f32 gradients far below the bf16 bound (the operands of the
    contraction are exact to ~16 bits; only dout itself is a bf16 tensor).  O = 12 (S = 24): ragged pixel tiles in the weight
    gradient, the data gradient on the VALU kernel; S = 256: the persistent data-gradient workgroups walk several tiles."""
    from sbagan import ops
    ops.set_compute_dtype(torch.bfloat16)
    N, S = shape
    img = fill.uniform((N, 3, S, S), 31)
    w = fill.unit((64, 3, 4, 4), 32) / np.sqrt(48)
    xr, wr = img.clone().requires_grad_(True), w.clone().requires_grad_(True)
    pre = F.conv2d(xr, wr, None, 2, 1)
    dy = rounded(fill.unit(tuple(pre.shape), 33), torch.bfloat16)
    wp = torch.nn.Parameter(w.to(dev).contiguous(memory_format=torch.channels_last))
    xa = img.to(dev).requires_grad_(True)
    out = ops.DStemFn.apply(xa, wp)
    out.backward(act(dy, torch.bfloat16, dev))
    torch.cuda.synchronize()
    close(out, F.leaky_relu(pre, 0.2), torch.bfloat16, 'out')
    # the LeakyReLU slope follows the sign of the STORED activation (a pre-activation within rounding of zero may have
    # either sign; a handful of flipped slopes among 10^6 outputs would dominate the bound below)
    slope = torch.where(out.detach().float().cpu() > 0, 1.0, 0.2)
    gx, gw = torch.autograd.grad(pre, [xr, wr], dy * slope)
    assert rel_l2(xa.grad.cpu(), gx) <= 3e-4, rel_l2(xa.grad.cpu(), gx)
    assert rel_l2(wp.grad.cpu(), gw) <= 3e-4, rel_l2(wp.grad.cpu(), gw)


@pytest.mark.parametrize('dt', DTYPES)
def test_init_stage_and_conditioning(dev, dt):
    from sbagan import nets, ops
    from miscc.config import cfg
    ops.set_compute_dtype(dt)
    cfg.TREE.BRANCH_NUM = 1
    g = nets.G_NET()
    P = fill.fill_state_dict({k: tuple(v.shape) for k, v in g.state_dict().items()})
    _load(g, P, dev)
    B = 4
    z, sent, eps = fill.unit((B, 100), 1), fill.unit((B, 256), 2), fill.unit((B, 100), 3)
    Q = _oracle_P(P)
    imgs_r, _, mu_r, lv_r = O.g_net(Q, z, sent, None, None, eps, 1)
    dimg = fill.unit(tuple(imgs_r[0].shape), 4)
    ((imgs_r[0] * dimg).sum() + O.kl_loss(mu_r, lv_r)).backward()
    from miscc.losses import KL_loss
    g.ca_net.eps = eps.to(dev)
    imgs, atts, mu, lv = g(z.to(dev), sent.to(dev), None, None)
    ((imgs[0] * dimg.to(dev)).sum() + KL_loss(mu, lv)).backward()
    torch.cuda.synchronize()
    close(imgs[0], imgs_r[0], dt, 'img64', scale=4)
    close(mu, mu_r, torch.float32, 'mu'); close(lv, lv_r, torch.float32, 'logvar')
    # BatchNorm1d over a batch of 4 right behind the fc amplifies summation-order differences of the
    # dense layers (each within 5e-7 of an f64 reference, tools/debug_linear.py: 3.2e-7 / 4.5e-7 / 7e-8 for y / dx / dW of
    # the 16384-column fc on the matrix-core kernels) by |x|/sigma: the per-element bound is 40x the plain f32 one
    _check_module(g, Q, dt, '', gscale=40)


def test_damsm_losses(dev):
    from miscc import losses
    from miscc.config import cfg
    B, nef, L = 5, 256, 9
    feat = fill.unit((B, nef, 17, 17), 1)
    words = fill.unit((B, nef, L), 2)
    code, sent = fill.unit((B, nef), 3), fill.unit((B, nef), 4)
    lens = torch.tensor([9, 7, 7, 5, 2])
    labels = torch.arange(B)
    for cids in (np.arange(B), np.array([0, 1, 0, 2, 1])):
        fr, wr = feat.clone().requires_grad_(True), words.clone().requires_grad_(True)
        w0, w1 = O.words_loss(fr, wr, labels, lens, cids, B, 4.0, 5.0, 10.0)
        (w0 * 1.5 + w1 * 0.7).backward()
        fa, wa = feat.to(dev).requires_grad_(True), words.to(dev).requires_grad_(True)
        g0, g1, _ = losses.words_loss(fa, wa, labels.to(dev), lens.to(dev), cids, B)
        (g0 * 1.5 + g1 * 0.7).backward()
        torch.cuda.synchronize()
        assert abs(float(g0) - float(w0)) < 2e-4 * max(1, abs(float(w0)))
        assert abs(float(g1) - float(w1)) < 2e-4 * max(1, abs(float(w1)))
        close(fa.grad, fr.grad, torch.float32, 'dfeat', scale=20)
        close(wa.grad, wr.grad, torch.float32, 'dwords', scale=20)
        cr, sr = code.clone().requires_grad_(True), sent.clone().requires_grad_(True)
        s0, s1 = O.sent_loss(cr, sr, labels, cids, B, 10.0)
        (s0 + 2 * s1).backward()
        ca, sa = code.to(dev).requires_grad_(True), sent.to(dev).requires_grad_(True)
        t0, t1 = losses.sent_loss(ca, sa, labels.to(dev), cids, B)
        (t0 + 2 * t1).backward()
        assert abs(float(t0) - float(s0)) < 1e-4 * max(1, abs(float(s0)))
        assert abs(float(t1) - float(s1)) < 1e-4 * max(1, abs(float(s1)))
        close(ca.grad, cr.grad, torch.float32, 'dcnn', scale=10); close(sa.grad, sr.grad, torch.float32, 'drnn', scale=10)


@pytest.mark.parametrize('shape', [(20, 256, 17, 18), (3, 64, 17, 32), (4, 128, 10, 5), (2, 256, 17, 1)])
def test_damsm_words_matrix_cores(dev, shape):
    """words_loss on the bf16 matrix cores (csrc/damsm_mfma.hip: hi + lo operands, one contraction per image for
    d(features)) against the oracle (losses.py:62-132) and against the f32 kernels it replaces: losses, d(features),
    d(words); d(features) is bit-reproducible run to run (no atomics)."""
    from miscc import losses
    from sbagan import ops
    B, nef, S, L = shape
    feat = fill.unit((B, nef, S, S), 11)
    words = fill.unit((B, nef, L), 12)
    lens = torch.tensor([max(1, L - (k * 3) % L) for k in range(B)])
    labels = torch.arange(B)
    cids = np.arange(B)
    fr, wr = feat.clone().requires_grad_(True), words.clone().requires_grad_(True)
    w0, w1 = O.words_loss(fr, wr, labels, lens, cids, B, 4.0, 5.0, 10.0)
    (w0 * 1.5 + w1 * 0.7).backward()

    def run():
        fa, wa = feat.to(dev).requires_grad_(True), words.to(dev).requires_grad_(True)
        g0, g1, _ = losses.words_loss(fa, wa, labels.to(dev), lens.to(dev), cids, B)
        (g0 * 1.5 + g1 * 0.7).backward()
        torch.cuda.synchronize()
        return float(g0), float(g1), fa.grad.cpu(), wa.grad.cpu()
    old = ops.DAMSM_MFMA
    try:
        ops.DAMSM_MFMA = True
        assert ops._damsm_prep(feat.to(dev), words.to(dev), lens.to(dev), B, nef, S * S, L) is not None
        m0, m1, mf, mw = run()
        _, _, mf2, _ = run()
        ops.DAMSM_MFMA = False
        v0, v1, vf, vw = run()
    finally:
        ops.DAMSM_MFMA = old
    for got, ref in ((m0, float(w0)), (m1, float(w1)), (m0, v0), (m1, v1)):
        assert abs(got - ref) < 2e-4 * max(1, abs(ref)), (got, ref)
    close(mf, fr.grad, torch.float32, 'dfeat vs oracle', scale=20)
    close(mw, wr.grad, torch.float32, 'dwords vs oracle', scale=20)
    close(mf, vf, torch.float32, 'dfeat vs f32 kernels', scale=20)
    close(mw, vw, torch.float32, 'dwords vs f32 kernels', scale=20)
    assert torch.equal(mf, mf2), 'd(features) of the matrix-core path is not reproducible'


def test_public_func_attention_vs_reference_golden(dev, golden_dir):
    """GlobalAttention.func_attention (GlobalAttention.py:31-69) as exported by the drop-in package, on the GPU,
    against the output of the reference's own function (tests/golden/units_tiny.npz, tools/make_golden.py)."""
    import GlobalAttention
    from helpers import TINY, check, load_golden, make_inputs
    G = load_golden(golden_dir, 'units_tiny.npz')
    x = make_inputs(TINY, 3, 6, tag=100)
    feat = fill.unit((3, TINY['nef'], 17, 17), 211)
    wc, at = GlobalAttention.func_attention(x['words'].to(dev), feat.to(dev), 4.0)
    torch.cuda.synchronize()
    check(G, 'funcattn/wctx', wc.cpu())
    check(G, 'funcattn/att', at.cpu())


def test_generator_loss_vs_oracle(dev):
    """miscc.losses.generator_loss (losses.py:164-206) stand-alone, 3 discriminators + stand-in image encoder, f32:
    the total, every logged component (and the reference's log string format), and the gradient w.r.t. each fake
    image against the oracle."""
    import model
    from helpers import FULL, d_shapes
    from miscc import losses
    from miscc.config import cfg
    from sbagan import ops
    ops.set_compute_dtype(torch.float32)
    B, L = 3, 7
    nets, Ps = [], []
    for i, cls in enumerate((model.D_NET64, model.D_NET128, model.D_NET256)):
        P = fill.fill_state_dict(d_shapes(FULL, i), salt=i)
        for k in P:
            if k.endswith('outlogits.0.weight'):
                P[k] = P[k] * 0.1          # keep the sigmoids out of saturation (see test_discriminator_loss)
        n = cls()
        n.load_state_dict(P)
        nets.append(n.to(dev).train())
        Ps.append({k: v.clone() for k, v in P.items()})
    enc = fill.StandInImageEncoder(256, device=dev)
    enc_cpu = fill.StandInImageEncoder(256, device=torch.device('cpu'))
    fakes = [fill.uniform((B, 3, 64 * 2 ** i, 64 * 2 ** i), 970 + i) for i in range(3)]
    words, sent = fill.unit((B, 256, L), 975), fill.unit((B, 256), 976)
    lens = torch.tensor([7, 5, 2])
    labels, cids = torch.arange(B), np.array([0, 1, 0])
    fr = [f.clone().requires_grad_(True) for f in fakes]
    smooth = dict(GAMMA1=4.0, GAMMA2=5.0, GAMMA3=10.0, LAMBDA=5.0)
    tot_r, logs_r = O.generator_loss(Ps, enc_cpu, fr, torch.ones(B), words, sent, labels, lens, cids, smooth)
    tot_r.backward()
    fa = [f.to(dev).requires_grad_(True) for f in fakes]
    tot, logs = losses.generator_loss(nets, enc, fa, torch.ones(B, device=dev), words.to(dev), sent.to(dev),
                                      labels.to(dev), lens.to(dev), cids)
    tot.backward()
    torch.cuda.synchronize()
    assert abs(float(tot) - float(tot_r)) <= 2e-4 * abs(float(tot_r)), (float(tot), float(tot_r))
    for k, v in logs_r.items():
        assert abs(float(logs[k]) - float(v)) <= 2e-4 * max(1.0, abs(float(v))), (k, float(logs[k]), float(v))
    ref_str = ''.join('g_loss%d: %.2f ' % (i, float(logs_r['g_loss%d' % i])) for i in range(3)) + \
        'w_loss: %.2f s_loss: %.2f ' % (float(logs_r['w_loss']), float(logs_r['s_loss']))
    assert str(logs) == ref_str and ('x' + logs) == 'x' + ref_str and (logs + '\n') == ref_str + '\n'
    for i in range(3):
        # through four train-mode BatchNorms at B = 3: the f32 atomic order of the batch statistics moves this gradient by
        # up to ~2e-3 from run to run (seen 2.1e-3 once in six runs); a wrong head / tap / scale is >= 1e-1
        assert rel_l2(fa[i].grad, fr[i].grad) <= 1e-2, ('dfake%d' % i, rel_l2(fa[i].grad, fr[i].grad))


def test_bce_kl_adam(dev):
    from sbagan import ops
    from sbagan.trainer import FlatParams, FusedAdam
    p = [torch.tensor([0.3, 0.9, 1e-9, 1.0]), torch.tensor([0.2, 0.5, 0.0])]
    pr = [t.clone().requires_grad_(True) for t in p]
    ref = 0.5 * O.bce(pr[0], torch.ones(4)) + (1 / 3) * O.bce(pr[1], torch.zeros(3))
    ref.backward()
    pa = [t.to(dev).requires_grad_(True) for t in p]
    out = ops.BCEMultiFn.apply((1., 0.), (.5, 1. / 3), *pa)
    (out * 2.0).backward()
    assert abs(float(out) - float(ref)) < 1e-5 * abs(float(ref))
    for a, b in zip(pa, pr):
        close(a.grad * 0.5, b.grad, torch.float32, 'dprob')
    # Adam + EMA vs the oracle's restatement of torch.optim.Adam, three steps
    net = torch.nn.Linear(37, 11).to(dev)
    w0, b0 = net.weight.detach().cpu().clone(), net.bias.detach().cpu().clone()
    flat = FlatParams(net, with_ema=True)
    opt = FusedAdam(flat, 2e-4)
    ps = [w0.clone(), b0.clone()]
    ms, vs = [torch.zeros_like(t) for t in ps], [torch.zeros_like(t) for t in ps]
    avg = [t.clone() for t in ps]
    for step in range(1, 4):
        gs = [fill.unit(tuple(t.shape), 10 * step + i) * (1e-3 if i else 1.0) for i, t in enumerate(ps)]
        flat.zero_grad()
        net.weight.grad += gs[0].to(dev)
        net.bias.grad += gs[1].to(dev)
        opt.step()
        for t, g, m, v, a in zip(ps, gs, ms, vs, avg):
            O.adam_update(t, g, m, v, step, 2e-4)
            O.ema_update(a, t)
    torch.cuda.synchronize()
    close(net.weight, ps[0], torch.float32, 'adam w'); close(net.bias, ps[1], torch.float32, 'adam b')
    ema = flat.ema_params()
    close(ema[0], avg[0], torch.float32, 'ema w'); close(ema[1], avg[1], torch.float32, 'ema b')


def test_adam_step_in_pieces_is_bit_equal(dev):
    """FusedAdam.step() is prepare() + step_range(0, n) + done(); the same update issued as two disjoint ranges -- on two
    streams, or in the other order on one -- must give the same bits in the parameters, both moments, the EMA shadow and
    the device state, and a piece must not touch an element outside its range.

    lo = one full pass of the 4096 x 256-thread grid plus 257 vectors (a multiple of 4: piece starts must be 16-byte
    aligned), so the first piece wraps the grid-stride loop; the second piece, 1027 elements, ends in the 3-element
    scalar tail that the whole launch also ends in: every element takes the same code path both ways."""
    from sbagan.trainer import FlatParams, FusedAdam
    lo = 4 * (4096 * 256) + 4 * 257
    n = lo + 1027

    class One(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(n, device=dev))

    flat = FlatParams(One(), with_ema=True)
    # FlatParams pads its buffers to a multiple of four elements (here n + 1); the update is confined to the parameter's
    # own n elements, so that the whole launch ends in the scalar tail.  The padding element must then never change.
    assert flat.n == n + 1 and lo % 4 == 0
    flat.n = n
    opt = FusedAdam(flat, 2e-4)
    opt.step()                                      # a state that is not all zeros (step counter 1)
    gen = torch.Generator(device='cpu')
    gen.manual_seed(20260)
    bufs = {'data': flat.data, 'grad': flat.grad, 'm': flat.m, 'v': flat.v, 'avg': flat.avg}
    for name, t in bufs.items():
        src = torch.rand(n + 1, generator=gen) if name == 'v' else torch.randn(n + 1, generator=gen)
        t.copy_(src.to(dev))
    snap = {k: t.clone() for k, t in bufs.items()}
    snap['state'] = opt.state.clone()
    cur, side = torch.cuda.current_stream(), torch.cuda.Stream(device=dev)

    def restore():
        for k, t in bufs.items():
            t.copy_(snap[k])
        opt.state.copy_(snap['state'])

    def result():
        torch.cuda.synchronize()
        r = {k: t.clone() for k, t in bufs.items() if k != 'grad'}
        r['state'] = opt.state.clone()
        return r

    def whole():
        opt.step(0.5)

    def two_streams():
        opt.prepare()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            opt.step_range(lo, n, 0.5)
        opt.step_range(0, lo, 0.5)
        cur.wait_stream(side)
        opt.done()

    def other_order():
        opt.prepare()
        opt.step_range(lo, n, 0.5)
        opt.step_range(0, lo, 0.5)
        opt.done()

    def only(a, b):
        def f():
            opt.prepare()
            opt.step_range(a, b, 0.5)
        return f

    res = {}
    for name, fn in (('whole', whole), ('two_streams', two_streams), ('other_order', other_order),
                     ('upper', only(lo, n)), ('lower', only(0, lo)), ('empty', only(lo, lo)), ('empty0', only(0, 0))):
        restore()
        fn()
        res[name] = result()
    a = res['whole']
    for k in ('data', 'm', 'v', 'avg'):
        assert not torch.equal(a[k][:n], snap[k][:n]), k               # (the update moves every buffer)
        for name in ('two_streams', 'other_order'):
            assert torch.equal(res[name][k], a[k]), (name, k)
        # one piece alone: its own range as in the whole update, everything outside bit-unchanged
        assert torch.equal(res['upper'][k][:lo], snap[k][:lo]), ('upper piece wrote below lo', k)
        assert torch.equal(res['upper'][k][lo:n], a[k][lo:n]), ('upper piece', k)
        assert torch.equal(res['lower'][k][lo:], snap[k][lo:]), ('lower piece wrote at or above lo', k)
        assert torch.equal(res['lower'][k][:lo], a[k][:lo]), ('lower piece', k)
        for name in ('empty', 'empty0'):
            assert torch.equal(res[name][k], snap[k]), ('an empty range changed', name, k)
        for name in res:
            assert torch.equal(res[name][k][n:], snap[k][n:]), ('padding element changed', name, k)
    for name in res:
        assert torch.equal(res[name]['state'], a['state']), (name, 'state')
    assert not torch.equal(a['state'], snap['state'])


def test_mask_and_sort_bit_exact(dev):
    from sbagan.trainer import build_mask, sort_by_caption_length
    caps, lens = fill.synthetic_captions(6, 20, 18, tag=9)
    perm = torch.randperm(6)
    l2, idx = sort_by_caption_length(lens[perm].to(dev))
    r2, ridx = O.sort_by_caption_length(lens[perm])
    assert torch.equal(l2.cpu(), r2)
    m = build_mask(caps.to(dev), 18)
    assert torch.equal(m.cpu(), O.build_mask(caps, 18)) and m.dtype == torch.bool


def test_errors_are_loud(dev):
    from sbagan import ops, _lib
    x = torch.zeros((1, 24, 4, 4), device=dev).contiguous(memory_format=torch.channels_last)
    w = torch.nn.Parameter(torch.zeros((8, 24, 3, 3), device=dev).contiguous(memory_format=torch.channels_last))
    with pytest.raises(RuntimeError):      # Cin = 24 is not a multiple of the K slab
        ops.conv_forward(x, ops.PackedWeight(w), '3x3')
    with pytest.raises(RuntimeError):      # CPU tensors never silently fall back
        ops.LinearFn.apply(torch.zeros(2, 3), torch.zeros(4, 3), None)


@pytest.mark.parametrize('dt', DTYPES)
def test_grouped_real_fake_pass_equals_two_calls(dev, dt):
    """netD(cat(real, fake), groups=2) == (netD(real), netD(fake)): features, BatchNorm buffers
    (running stats updated twice, in order) and parameter gradients."""
    import copy
    from sbagan import nets, ops
    from miscc.config import cfg
    ops.set_compute_dtype(dt)
    cfg.GAN.DF_DIM = 64
    d1 = nets.D_NET128()
    P = fill.fill_state_dict({k: tuple(v.shape) for k, v in d1.state_dict().items()})
    d1.load_state_dict(P)
    d2 = copy.deepcopy(d1)
    d1.to(dev).train(); d2.to(dev).train()
    B = 3
    real, fake = fill.uniform((B, 3, 128, 128), 1).to(dev), fill.uniform((B, 3, 128, 128), 2).to(dev)
    g = fill.unit((2 * B, 512, 4, 4), 3).to(dev).to(dt).contiguous(memory_format=torch.channels_last)
    f1 = d1(torch.cat((real, fake), 0), groups=2)
    f1.backward(g)
    fr, ff = d2(real), d2(fake)
    (fr * g[:B].float()).sum().backward()
    (ff * g[B:].float()).sum().backward()
    torch.cuda.synchronize()
    # (the grouped pass takes its BN statistics from the stored activations, the single pass from the
    # f32 accumulators of the conv epilogue: equal up to rounding)
    close(f1[:B], fr, dt, 'real half', scale=0.2 if dt == torch.float32 else 0.6)
    close(f1[B:], ff, dt, 'fake half', scale=0.2 if dt == torch.float32 else 0.6)
    for (n, a), (_, b) in zip(d1.named_buffers(), d2.named_buffers()):
        if n.endswith('num_batches_tracked'):
            assert int(a) == int(b) == (2 if 'img_code' in n else 0), n
        else:
            close(a, b, torch.float32, n, scale=10 if dt == torch.float32 else 300)
    for (n, a), (_, b) in zip(d1.named_parameters(), d2.named_parameters()):
        if b.grad is None:
            assert a.grad is None
            continue
        r = rel_l2(a.grad, b.grad)
        # f32: accumulation order differs (conv-epilogue statistics slots and atomics vs the separate
        # statistics pass); a rounding-level change can flip a LeakyReLU mask bit of a near-zero
        # activation, which moves a gradient by ~1e-3 relative -- hence not 1e-6
        assert r < (1e-2 if dt == torch.float32 else 0.12), (n, r)


@pytest.mark.parametrize('name', ['small', 'bird'])
def test_text_encoder_lstm(dev, name, golden_dir):
    """sba_lstm_bidir_fwd (frozen RNN_ENCODER forward, cap_lens read on the device) against the reference's
    golden outputs and the numpy oracle: f32, 1e-5.  Also the sync-free shape contract (max_len=None -> full
    padded width, extra columns zero) and a non-zero initial state against the module's torch path."""
    import model
    from helpers import load_golden
    from oracle import text_encoder as TE
    T = load_golden(golden_dir, 'text_encoder.npz')
    ntoken, ninput, nhidden = (int(v) for v in T['%s/dims' % name])
    net = model.RNN_ENCODER(ntoken, ninput=ninput, nhidden=nhidden)
    P = fill.fill_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, salt=7)
    net.load_state_dict(P)
    net.to(dev).eval()
    cap = torch.from_numpy(T['%s/captions' % name]).to(dev)
    lens = torch.from_numpy(T['%s/cap_lens' % name]).to(dev)
    B, Tw = cap.shape
    lmax = int(T['%s/cap_lens' % name].max())
    with torch.no_grad():
        assert net._hip_ok(cap)
        words, sent = net(cap, lens, net.init_hidden(B), max_len=lmax)
        wfull, sfull = net(cap, lens, net.init_hidden(B))
    assert words.shape == T['%s/words_emb' % name].shape and wfull.shape == (B, nhidden, Tw)
    np.testing.assert_allclose(words.cpu().numpy(), T['%s/words_emb' % name], rtol=0, atol=1e-5)
    np.testing.assert_allclose(sent.cpu().numpy(), T['%s/sent_emb' % name], rtol=0, atol=1e-5)
    ow, osent = TE.rnn_encoder_forward({k: v.numpy() for k, v in P.items()}, T['%s/captions' % name],
                                       T['%s/cap_lens' % name])
    np.testing.assert_allclose(words.cpu().numpy(), ow, rtol=0, atol=1e-5)
    np.testing.assert_allclose(sent.cpu().numpy(), osent, rtol=0, atol=1e-5)
    assert torch.equal(wfull[:, :, :lmax], words) and float(wfull[:, :, lmax:].abs().max() if lmax < Tw else 0) == 0
    assert torch.equal(sfull, sent)
    # non-zero initial state: HIP path vs the torch (MIOpen) path of the same module
    h0 = (0.3 * torch.randn(2, B, nhidden // 2, device=dev), 0.3 * torch.randn(2, B, nhidden // 2, device=dev))
    with torch.no_grad():
        w1, s1 = net(cap, lens, h0, max_len=lmax)
        net.use_hip = False
        w2, s2 = net(cap, lens, h0)
        net.use_hip = True
    np.testing.assert_allclose(w1.cpu().numpy(), w2.cpu().numpy(), rtol=0, atol=2e-5)
    np.testing.assert_allclose(s1.cpu().numpy(), s2.cpu().numpy(), rtol=0, atol=2e-5)


def test_attention_key_projection_fp8(dev):
    """BASELINE config 5: the attention key projection on v_mfma_f32_32x32x16_fp8_fp8 (csrc/linear.hip).
    (1) layout / scaling: on data that e4m3 represents exactly (integers in [-2, 2], block amax 2 -> scaled by 128) the result equals the f32 kernel's bit for bit; (2) stated tolerance on N(0,1) data: relative
    L2 <= 8e-2; (3) through the module: attention output within 1e-1 of the f32-operand path."""
    import ctypes
    from sbagan import ops
    from sbagan._lib import call
    st = torch.cuda.current_stream().cuda_stream
    B, C, cdf, L = 5, 32, 256, 18
    g = torch.Generator().manual_seed(11)
    words = torch.randint(-2, 3, (B, cdf, L), generator=g).float().to(dev)
    W = torch.randint(-2, 3, (C, cdf), generator=g).float().to(dev)
    W[:, 0], words[:, 0, :] = 2.0, 2.0          # every tile reaches amax 2
    ref, got = torch.empty((B, C, L), device=dev), torch.empty((B, C, L), device=dev)
    call('sba_ctx_proj_fwd', words.data_ptr(), W.data_ptr(), ref.data_ptr(), B, C, cdf, L, st)
    call('sba_ctx_proj_fwd_fp8', words.data_ptr(), W.data_ptr(), got.data_ptr(), B, C, cdf, L, st)
    torch.cuda.synchronize()
    assert torch.equal(ref, torch.einsum('ic,bcl->bil', W, words))
    assert torch.equal(got, ref), (float((got - ref).abs().max()), got[0, :2, :4], ref[0, :2, :4])
    words, W = torch.randn((B, cdf, L), generator=g).to(dev), (torch.randn((C, cdf), generator=g) / 16).to(dev)
    call('sba_ctx_proj_fwd', words.data_ptr(), W.data_ptr(), ref.data_ptr(), B, C, cdf, L, st)
    call('sba_ctx_proj_fwd_fp8', words.data_ptr(), W.data_ptr(), got.data_ptr(), B, C, cdf, L, st)
    torch.cuda.synchronize()
    r = rel_l2(got, ref)
    assert 1e-3 < r <= 8e-2, r
    import GlobalAttention as GA
    ops.set_compute_dtype(torch.float32)
    att = GA.GlobalAttentionGeneral(32, 256).to(dev)
    h = torch.randn((B, 32, 16, 16), generator=g).to(dev)
    mask = torch.zeros((B, L), dtype=torch.bool, device=dev)
    mask[:, 12:] = True
    att.applyMask(mask)
    try:
        o32, _ = att(h, words)
        ops.set_attention_fp8(True)
        o8, _ = att(h, words)
    finally:
        ops.set_attention_fp8(False)
    torch.cuda.synchronize()
    assert 0 < rel_l2(o8, o32) <= 1e-1, rel_l2(o8, o32)      # measured 5.9e-2 (the softmax sharpens the key error)


@pytest.mark.parametrize('shape', [(3, 18, 12 * 12, 0, 0), (20, 18, 64 * 64, 0, 1), (5, 20, 1000, 1, 0), (2, 32, 33, 1, 1)])
def test_word_attention_matrix_core_backward(dev, shape):
    """The bf16 backward at idf = 32 (GlobalAttention.py:103-117 differentiated): scores and dA recomputed on the matrix
    cores with hi + lo split keys, softmax backward in-lane, dh with hi + lo split dS, dsrc over the query axis through
    LDS -- against torch autograd in f32 on the same bf16 inputs.  dh is a bf16 tensor (2^-9 per element); dsrc contracts
    bf16-rounded dS / probabilities (as the VALU kernel does).  Ragged query counts, L up to 32, both mask modes, dctx
    read from a channel slice, dh accumulated onto an existing gradient.  Every shape here selects ONE tile per wave (the
    largest, 20 x 4096 queries, is 2560 tiles, below the 4096 at which the host picks two); two and four tiles per wave,
    the VALU arms and every edge are in tests/test_attention_kernels_gpu.py, element by element against float64."""
    from sbagan._lib import call
    B, L, Q, mode, accumulate = shape
    idf = 32
    g = torch.Generator().manual_seed(7)
    h = torch.randn((B, Q, idf), generator=g).to(dev).bfloat16()
    src = (torch.randn((B, idf, L), generator=g) * 0.5).to(dev)
    mask = (torch.rand((B, L), generator=g) < 0.3).to(dev)
    mask[:, 0] = False
    m8 = mask.to(torch.uint8).contiguous()
    dcs, dco = 2 * idf, idf
    dfull = torch.randn((B, Q, dcs), generator=g).to(dev).bfloat16()
    dctx = dfull[:, :, dco:dco + idf]
    hf, sf = h.float().requires_grad_(True), src.clone().requires_grad_(True)
    s = torch.bmm(hf, sf)
    rows = torch.arange(B * Q, device=dev).view(B, Q)
    mrow = (rows % B) if mode == 0 else torch.arange(B, device=dev).view(B, 1).expand(B, Q)
    a = torch.softmax(s.masked_fill(mask[mrow], float('-inf')), 2)
    ctx = torch.bmm(a, sf.transpose(1, 2))
    gh, gs = torch.autograd.grad(ctx, [hf, sf], dctx.float())
    prev = torch.randn((B, Q, idf), generator=g).to(dev).bfloat16()
    dh = prev.clone() if accumulate else torch.empty_like(prev)
    dsrc = torch.zeros((B, idf, L), device=dev)
    st = torch.cuda.current_stream().cuda_stream
    call('sba_word_attn_bwd', 1, h.data_ptr(), src.data_ptr(), m8.data_ptr(), dfull.data_ptr(), dh.data_ptr(),
         dsrc.data_ptr(), B, Q, idf, L, mode, dcs, dco, accumulate, st)
    torch.cuda.synchronize()
    want = gh + prev.float() if accumulate else gh
    assert rel_l2(dh.float(), want) <= 4e-3, rel_l2(dh.float(), want)
    assert rel_l2(dsrc, gs) <= 6e-3, rel_l2(dsrc, gs)


@pytest.mark.parametrize('shape', [(3, 32, 7, 12 * 12, 0), (20, 32, 18, 64 * 64, 0), (5, 64, 20, 1000, 1), (2, 32, 32, 33, 1)])
def test_word_attention_matrix_core_forward(dev, shape):
    """The bf16 forward runs both contractions (GlobalAttention.py:103,117) on v_mfma_f32_32x32x16_bf16 with the keys
    and the probabilities split into hi + lo bf16 parts: it must agree with an f32 evaluation of the same bf16 inputs to
    f32 rounding (NOT to bf16 rounding: only the stored context is rounded), for ragged query counts, L up to 32, both
    mask modes, an output written into a channel slice, and the optional attention map.  No row is fully masked here
    (word 0 is always live); that a fully masked row gives NaN exactly where the reference's softmax does is checked by
    tests/test_attention_kernels_gpu.py (test_fully_masked_row), with every other arm of the dispatch."""
    from sbagan._lib import call
    B, idf, L, Q, mode = shape
    g = torch.Generator().manual_seed(5)
    h = torch.randn((B, Q, idf), generator=g).to(dev).bfloat16()
    src = (torch.randn((B, idf, L), generator=g) * 0.5).to(dev)
    mask = (torch.rand((B, L), generator=g) < 0.3).to(dev)
    mask[:, 0] = False
    m8 = mask.to(torch.uint8).contiguous()
    ocs, oco = 2 * idf, idf
    out = torch.zeros((B, Q, ocs), device=dev, dtype=torch.bfloat16)
    att = torch.empty((B, L, Q), device=dev)
    st = torch.cuda.current_stream().cuda_stream
    call('sba_word_attn_fwd', 1, h.data_ptr(), src.data_ptr(), m8.data_ptr(), out.data_ptr(), att.data_ptr(), B, Q, idf,
         L, mode, ocs, oco, st)
    torch.cuda.synchronize()
    s = torch.bmm(h.float(), src)                                         # B x Q x L
    rows = torch.arange(B * Q, device=dev).view(B, Q)
    mrow = (rows % B) if mode == 0 else torch.arange(B, device=dev).view(B, 1).expand(B, Q)
    s = s.masked_fill(mask[mrow], float('-inf'))
    a = torch.softmax(s, 2)
    ctx = torch.bmm(a, src.transpose(1, 2))                               # B x Q x idf
    assert float((att.transpose(1, 2) - a).abs().max()) <= 3e-5       # keys carried as hi + lo bf16: ~2^-17 relative
    assert torch.equal(out[..., :oco], torch.zeros_like(out[..., :oco]))  # the other half of the slice is untouched
    got = out[..., oco:].float()
    assert float((got - ctx.bfloat16().float()).abs().max()) <= 1e-2 * float(ctx.abs().max())     # <= 1 bf16 ulp
    assert rel_l2(got, ctx) <= 3e-3


def test_word_attention_fp8(dev):
    """BASELINE config 5: both attention contractions on v_mfma_f32_32x32x16_fp8_fp8 (sba_word_attn_fwd_fp8).
    (1) layout / scaling: with inputs e4m3 represents exactly and ONE live word per query (probability exactly 1) the
    context equals the selected key column bit for bit; (2) stated tolerance on N(0,1)-scaled inputs (e4m3: 2^-4 relative
    per operand, 32-term scores of standard deviation ~1.7): attention map within 0.12 absolute (measured 0.081), context
    within 8e-2 relative L2 (measured 5.6e-2) of the f32 evaluation."""
    from sbagan._lib import call
    st = torch.cuda.current_stream().cuda_stream
    B, idf, L, Q = 4, 32, 9, 1000
    g = torch.Generator().manual_seed(7)
    h = torch.randint(-2, 3, (B, Q, idf), generator=g).float().to(dev).bfloat16()
    src = torch.randint(-4, 5, (B, idf, L), generator=g).float().to(dev) * 0.25
    mask = torch.ones((B, L), dtype=torch.bool, device=dev)
    for b in range(B):
        mask[b, (3 * b) % L] = False
    m8 = mask.to(torch.uint8).contiguous()
    out = torch.empty((B, Q, idf), device=dev, dtype=torch.bfloat16)
    call('sba_word_attn_fwd_fp8', h.data_ptr(), src.data_ptr(), m8.data_ptr(), out.data_ptr(), None, B, Q, idf, L, 1, idf, 0,
         st)
    torch.cuda.synchronize()
    want = torch.stack([src[b, :, (3 * b) % L] for b in range(B)])[:, None, :].expand(B, Q, idf)
    assert torch.equal(out.float(), want), float((out.float() - want).abs().max())
    h = torch.randn((B, Q, idf), generator=g).to(dev).bfloat16()
    src = (torch.randn((B, idf, L), generator=g) * 0.3).to(dev)
    mask = (torch.rand((B, L), generator=g) < 0.3).to(dev)
    mask[:, 0] = False
    m8 = mask.to(torch.uint8).contiguous()
    att = torch.empty((B, L, Q), device=dev)
    call('sba_word_attn_fwd_fp8', h.data_ptr(), src.data_ptr(), m8.data_ptr(), out.data_ptr(), att.data_ptr(), B, Q, idf,
         L, 1, idf, 0, st)
    torch.cuda.synchronize()
    s = torch.bmm(h.float(), src).masked_fill(mask[:, None, :], float('-inf'))
    a = torch.softmax(s, 2)
    ctx = torch.bmm(a, src.transpose(1, 2))
    da, dc = float((att.transpose(1, 2) - a).abs().max()), rel_l2(out.float(), ctx)
    assert 1e-4 < da <= 0.12 and 1e-3 < dc <= 8e-2, (da, dc)


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16])
def test_bert_encoder_hip_vs_module(dev, dt):
    """BertEncoder.forward (model_bert.py:177-189) on the HIP kernels against the same module evaluated by
    PyTorch (HuggingFace BertModel, the available substitute for pytorch_pretrained_bert: parity unpinned w.r.t.
    the reference's dependency) on random-init BERT-base weights, no attention mask, L = 20:
    f32 path 2e-4, bf16 path 3e-2 relative L2."""
    import model_bert
    from miscc.config import cfg
    from sbagan import ops
    ops.set_compute_dtype(dt)
    cfg.TEXT.WORDS_NUM = 20
    torch.manual_seed(3)
    enc = model_bert.BertEncoder(256).to(dev).eval()
    B, L = 6, 20
    cap = torch.randint(1000, 30522, (B, L), device=dev)
    cap[2, 12:] = 0                 # padded captions: no mask is applied (reference behaviour)
    enc.use_hip = False
    with torch.no_grad():
        w_ref, s_ref = enc(cap)
    enc.use_hip = True
    with torch.no_grad():
        w, s = enc(cap)
    torch.cuda.synchronize()
    assert w.shape == (B, 256, L) and s.shape == (B, 256) and w.dtype == torch.float32
    tol = 2e-4 if dt == torch.float32 else 3e-2
    assert rel_l2(w, w_ref) <= tol, rel_l2(w, w_ref)
    assert rel_l2(s, s_ref) <= tol, rel_l2(s, s_ref)
