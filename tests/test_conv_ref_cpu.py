"""tests/conv_ref.py pinned without a device: (a) the reference equals F.conv2d / F.conv_transpose2d in float64 on
dense cases of every geometry kind the slice tests use, and slices change nothing; (b) a CORRECT low-precision
implementation -- emulated from the reference alone: the float32 contraction of the rounded operands, rounded to the
storage type, + addend, rounded again -- is inside the bounds at every element of every case of
tests/test_conv_slices_gpu.py (a condition, not a measurement), while half the unit roundoff is not enough; (c) the
bounds reject each kind of kernel error they are there for, injected into a copy of a correct output."""
from types import SimpleNamespace as NS

import pytest
import torch
import torch.nn.functional as F

import conv_ref as R
import test_conv_slices_gpu as S
from oracle import fill

NAN = float('nan')


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def oihw(w, KH, KW):
    """[Cout][KH * KW][Cin] -> [Cout][Cin][KH][KW]"""
    return w.view(w.shape[0], KH, KW, w.shape[2]).permute(0, 3, 1, 2).contiguous()


def draw(N, H, W, Cin, Cout, ntaps, tag):
    x = fill.unit((N, H, W, Cin), tag).double()
    w = fill.unit((Cout, ntaps, Cin), tag + 1).double() / (ntaps * Cin) ** 0.5
    return x, w


# ------------------------------------------------------------------ (a) the reference is the convolution
@pytest.mark.parametrize('kind', [(3, 3, 1, 1, 1), (1, 7, 0, 3, 1), (7, 1, 3, 0, 1), (5, 5, 2, 2, 1), (1, 1, 0, 0, 1),
                                  (3, 3, 0, 0, 1), (3, 3, 0, 0, 2), (4, 4, 1, 1, 2)])
def test_forward_geometries_equal_conv2d(kind):
    KH, KW, ph, pw, s = kind
    N, H, W, Cin, Cout = 2, 11, 9, 6, 5
    x, w = draw(N, H, W, Cin, Cout, KH * KW, 1)
    taps, OH, OW = S.fwd(KH, KW, ph, pw, H, W, s)
    g = R.geom(N, H, W, Cin, OH, OW, Cout, taps, sy=s)
    want = F.conv2d(nchw(x), oihw(w, KH, KW), None, s, (ph, pw))
    got = R.contract(x, w, g)
    assert got.shape == (N, OH, OW, Cout)
    assert float((nchw(got) - want).abs().max()) <= 1e-13
    # the same launch on a channel slice of a wider tensor whose other channels are NaN
    xw = torch.full((N, H, W, Cin + 7), NAN, dtype=torch.float64)
    xw[..., 3:3 + Cin] = x
    gs = R.geom(N, H, W, Cin, OH, OW, Cout, taps, sy=s, xcs=Cin + 7, xco=3)
    assert torch.equal(R.contract(xw, w, gs), got)
    # A is the contraction of the absolute values
    r = R.launch(x, w, g)
    assert float((nchw(r.A) - F.conv2d(nchw(x.abs()), oihw(w.abs(), KH, KW), None, s, (ph, pw))).abs().max()) <= 1e-12
    assert bool((r.A >= r.acc.abs() - 1e-12).all())


def test_upsampled_input_equals_conv2d_of_the_upsampled_tensor():
    N, H, W, Cin, Cout = 2, 5, 4, 6, 5
    x, w = draw(N, H, W, Cin, Cout, 9, 2)
    g = R.geom(N, H, W, Cin, 2 * H, 2 * W, Cout, R.window_taps(3, 3, 1, 1), ups=1)
    up = nchw(x).repeat_interleave(2, 2).repeat_interleave(2, 3)
    assert float((nchw(R.contract(x, w, g)) - F.conv2d(up, oihw(w, 3, 3), None, 1, 1)).abs().max()) <= 1e-13


@pytest.mark.parametrize('pad', [0, 1])
def test_stride1_data_gradient_equals_conv_transpose2d(pad):
    N, H, W, I, O = 2, 7, 6, 5, 4                       # dy is [N, H, W, O], the conv was I -> O
    wf = fill.unit((O, I, 3, 3), 3).double() / 7
    dy = fill.unit((N, H, W, O), 4).double()
    taps, OH, OW = S.dgrad1(3, 3, pad, pad, H, W)
    wd = wf.permute(1, 2, 3, 0).reshape(I, 9, O).contiguous()        # [Cout = I][tap = kh * 3 + kw][Cin = O]
    g = R.geom(N, H, W, O, OH, OW, I, taps)
    want = F.conv_transpose2d(nchw(dy), wf, None, 1, pad)
    assert float((nchw(R.contract(dy, wd, g)) - want).abs().max()) <= 1e-13


def test_stride2_parity_classes_equal_conv_transpose2d():
    """case 7: four sub-grid launches (osy = 2, ooy / oox = the class) fill the input gradient of a stride-2 conv"""
    N, S_, I, O = 2, 17, 5, 6
    OH = (S_ - 3) // 2 + 1
    wf = fill.unit((O, I, 3, 3), 5).double() / 7
    dy = fill.unit((N, OH, OH, O), 6).double()
    want = F.conv_transpose2d(nchw(dy), wf, None, 2, 0)
    assert want.shape[-1] == S_
    dx = torch.full((N, S_, S_, I + 4), NAN, dtype=torch.float64)
    for cls in range(4):
        py, px = cls // 2, cls % 2
        sel, taps = S.s2_class_taps(3, 3, py, px)
        wd = torch.stack([wf[:, :, kh, kw].t() for kh, kw in sel], 1).contiguous()      # [I][taps][O]
        g = R.geom(N, OH, OH, O, S_, S_, I, taps, OHs=(S_ - py + 1) // 2, OWs=(S_ - px + 1) // 2, osy=2, ooy=py, oox=px,
                   ycs=I + 4, yco=2)
        R.window(dx, g)[...] = R.contract(dy, wd, g)
    assert bool(torch.isnan(dx[..., :2]).all()) and bool(torch.isnan(dx[..., 2 + I:]).all())
    assert float((nchw(dx[..., 2:2 + I]) - want).abs().max()) <= 1e-13
    # the class tables of the GPU cases are these
    for cls, c in enumerate(S.DGRAD_S2):
        assert c.taps == S.s2_class_taps(3, 3, cls // 2, cls % 2)[1] and (c.osy, c.ooy, c.oox) == (2, cls // 2, cls % 2)


def test_epilogue_order_and_weight_gradient():
    N, H, W, Cin, Cout = 2, 5, 4, 6, 5
    x, w = draw(N, H, W, Cin, Cout, 9, 7)
    bias = fill.unit((Cout,), 8).double()
    add = fill.unit((N, H, W, Cout + 6), 9).double()
    mask = fill.unit((N, H, W, Cout + 6), 10).double()
    mask.view(-1)[::3] = 0.0
    mask.view(-1)[1::7] = -0.0
    g = R.geom(N, H, W, Cin, H, W, Cout, R.window_taps(3, 3, 1, 1), relu=1, ycs=Cout + 6, yco=4)
    r = R.launch(x, w, g, bias, add, mask)
    conv = F.conv2d(nchw(x), oihw(w, 3, 3), bias, 1, 1).permute(0, 2, 3, 1)
    m = mask[..., 4:4 + Cout]
    want = (conv.clamp(min=0) + add[..., 4:4 + Cout]) * (m > 0)
    assert float((r.ref - want).abs().max()) <= 1e-13
    assert torch.equal(r.zero, ~(m > 0)) and bool(r.zero[m == 0].all()) and r.add
    assert float((r.pre - conv.clamp(min=0)).abs().max()) <= 1e-13
    assert float((r.A - (R.contract(x.abs(), w.abs(), g) + bias.abs())).abs().max()) == 0.0
    # weight gradient against autograd
    xr, wr = nchw(x).requires_grad_(True), oihw(w, 3, 3).requires_grad_(True)
    dy = fill.unit((N, H, W, Cout), 11).double()
    (gw,) = torch.autograd.grad(F.conv2d(xr, wr, None, 1, 1), [wr], nchw(dy))
    gd = R.geom(N, H, W, Cin, H, W, Cout, R.window_taps(3, 3, 1, 1))
    dw, A = R.wgrad(x, dy, gd)
    assert float((oihw(dw, 3, 3) - gw).abs().max()) <= 1e-12
    assert bool((A >= dw.abs() - 1e-12).all())


# ------------------------------------------------------------------ (b) a correct implementation passes everywhere
def emulate(c, o, g):
    """what a correct kernel of mode c.mode stores: float32 accumulation of the rounded operands, bias / ReLU in
    float32, one rounding to the output type; an addend is added to the ROUNDED value and the sum rounded again
    (float32 outputs: added in float32)"""
    so = S.MODES[c.mode][2]
    acc = R.contract(o.x.float(), o.w.float(), g)
    pre = acc if o.bias is None else acc + o.bias.float()
    if g.relu:
        pre = pre.clamp(min=0)
    out = pre.to(so)
    if o.add is not None:
        out = (out.float() + R.window(o.add, g)).to(so)
        out = torch.where(R.window(o.mask, g) > 0, out, torch.zeros_like(out))
    return acc, out


ALL_CASES = S.PLAN_CASES + S.GROUP_ITEMS
_SEEN = {}


@pytest.mark.parametrize('c', ALL_CASES, ids=[c.id for c in ALL_CASES])
def test_a_correct_low_precision_implementation_is_inside_the_bounds(c):
    key = S.ref_key(c)
    if key in _SEEN:                        # (the forced-tile variants of a case share their geometry and reference)
        return
    o, r = S.reference(c)
    g = S.geom_of(c)
    u = S.MODES[c.mode][4]
    acc, out = emulate(c, o, g)
    facc = float(((acc.double() - r.acc).abs() / r.A.clamp(min=1e-30)).max())
    ratio = R.worst(out, r, u)
    _SEEN[key] = (c.mode, o.add is not None, ratio, R.worst(out, r, u / 2) if c.mode != 'f32' else None,
                  R.worst(out, r, u, two_roundings=False))
    print('%-24s float32 accumulation %.2e A, emulation at %.3f of the bound' % (c.id, facc, ratio))
    assert facc <= R.C_ACC / 10, 'float32 accumulation is a tenth of c at most'
    assert ratio <= 1.0
    s = R.stats(r)
    a32 = acc.reshape(-1, c.Cout)
    assert float(((a32.sum(0).double() - s.sum).abs() / s.sum_abs.clamp(min=1e-30)).max()) <= R.C_ACC
    assert float((((a32 * a32).sum(0).double() - s.sumsq).abs() / s.sumsq_abs.clamp(min=1e-30)).max()) <= R.C_ACC


def test_the_bounds_are_not_slack():
    """over the cases above: with half the unit roundoff some bf16 case fails (u = 2^-8 is needed), and behind an addend
    the single-rounding bound fails (the u |pre| term is needed)"""
    for c in ALL_CASES:
        if S.ref_key(c) not in _SEEN:
            test_a_correct_low_precision_implementation_is_inside_the_bounds(c)
    rows = list(_SEEN.values())
    bf = [v for v in rows if v[0] == 'bf16']
    assert max(v[2] for v in bf) > 0.5 and max(v[3] for v in bf) > 1.0
    assert all(v[3] > 1.0 for v in bf if not v[1]), 'every bf16 case without an addend needs more than u / 2'
    assert all(v[4] > 1.0 for v in bf if v[1]), 'every bf16 case with an addend needs the second rounding term'


# ------------------------------------------------------------------ (c) injected errors are rejected
def rejected(got, r, u, **kw):
    try:
        return R.worst(got, r, u, **kw) > 1.0
    except AssertionError:
        return True


@pytest.fixture(scope='module')
def victim():
    """case 2 (1 x 7, 128 -> 44, addend + mask) on its sliced output layout, addend and mask tensors filled with OTHER
    values outside the window, and the correct emulated output"""
    c = [k for k in S.SINGLE if k.id == '2-t0'][0]
    o, _ = S.reference(c)
    sl = S.slices(c)
    g = S.geom_of(c, (0, 0) + sl[2:])
    ycs, yco = sl[2], sl[3]
    shape = (c.N, c.OH, c.OW, ycs)
    addw = S.stored(fill.unit(shape, 71), torch.bfloat16)
    maskw = S.stored(fill.unit(shape, 72), torch.bfloat16)
    addw[..., yco:yco + c.Cout] = o.add
    maskw[..., yco:yco + c.Cout] = o.mask
    r = R.launch(o.x, o.w, g, None, addw, maskw)

    def emu(gg, addw=addw, maskw=maskw, ge=False):
        out = R.contract(o.x.float(), o.w.float(), gg).to(torch.bfloat16)
        out = (out.float() + R.window(addw, gg)).to(torch.bfloat16)
        m = R.window(maskw, gg)
        return torch.where((m >= 0) if ge else (m > 0), out, torch.zeros_like(out)).double()
    good = emu(g)
    assert not rejected(good, r, R.U_BF16)
    return NS(c=c, o=o, g=g, r=r, good=good, emu=emu, yco=yco)


def test_one_dropped_k_term_is_rejected(victim):
    v = victim
    n, oy, ox, co = 1, 5, 9, 17
    assert not bool(v.r.zero[n, oy, ox, co])
    terms = torch.cat([p[n, oy, ox].double() * v.o.w[co, t].double() for t, p in enumerate(R.patches(v.o.x, v.g))])
    assert abs(float(terms.sum() - v.r.acc[n, oy, ox, co])) <= 1e-12
    drop = float(terms[terms.abs().argmax()])          # the largest of the 896 products of this element
    got = v.good.clone()
    pre = v.r.pre[n, oy, ox, co] - drop
    got[n, oy, ox, co] = float((pre.to(torch.bfloat16).float() + v.o.add[n, oy, ox, co]).to(torch.bfloat16))
    assert rejected(got, v.r, R.U_BF16)
    assert not rejected(v.good, v.r, R.U_BF16)


def test_a_missing_output_row_is_rejected(victim):
    v = victim
    for leftover in (NAN, 0.0):
        got = v.good.clone()
        got[1, 7, :, :] = leftover
        assert rejected(got, v.r, R.U_BF16)
    got = v.good.clone()
    got[1, 7] = got[1, 8]                   # the row of the pixel below
    assert rejected(got, v.r, R.U_BF16)


def test_a_shift_by_eight_channels_is_rejected(victim):
    assert rejected(torch.roll(victim.good, 8, -1), victim.r, R.U_BF16)
    assert rejected(torch.roll(victim.good, -8, -1), victim.r, R.U_BF16)


def test_addend_or_mask_read_without_the_channel_offset_is_rejected(victim):
    v = victim
    g0 = R.geom(**dict((k, getattr(v.g, k)) for k in ('N', 'IH', 'IW', 'Cin', 'OH', 'OW', 'Cout')), taps=v.c.taps,
                ycs=v.g.y_cstride, yco=0)
    # the window the faulty kernel would read: channels [0, Cout) of the same tensors
    addw = S.stored(fill.unit((v.c.N, v.c.OH, v.c.OW, v.g.y_cstride), 71), torch.bfloat16)
    addw[..., v.yco:v.yco + v.c.Cout] = v.o.add
    maskw = S.stored(fill.unit(addw.shape, 72), torch.bfloat16)
    maskw[..., v.yco:v.yco + v.c.Cout] = v.o.mask
    right_add = torch.zeros_like(addw)
    right_add[..., :v.c.Cout] = v.o.add
    right_mask = torch.zeros_like(maskw)
    right_mask[..., :v.c.Cout] = v.o.mask
    assert not rejected(v.emu(g0, right_add, right_mask), v.r, R.U_BF16)        # (the harness itself is right)
    assert rejected(v.emu(g0, addw, right_mask), v.r, R.U_BF16), 'addend read at y_coff = 0'
    assert rejected(v.emu(g0, right_add, maskw), v.r, R.U_BF16), 'mask read at y_coff = 0'


def test_a_mask_taken_as_greater_or_equal_is_rejected(victim):
    v = victim
    assert bool((v.o.mask == 0).any()) and bool((torch.signbit(v.o.mask) & (v.o.mask == 0)).any())
    assert rejected(v.emu(v.g, ge=True), v.r, R.U_BF16)


def test_a_single_rounding_bound_rejects_the_two_roundings(victim):
    """the epilogue rounds twice behind an addend: a bound that assumes one rounding (no u |pre| term) must not pass a
    correct kernel, and the two-rounding bound must not pass an output that is off by one more rounding of |pre|"""
    v = victim
    assert rejected(v.good, v.r, R.U_BF16, two_roundings=False)
    keep = ~v.r.zero
    off = v.good + torch.where(keep, 2.5 * R.U_BF16 * (v.r.pre.abs() + v.r.ref.abs()), torch.zeros_like(v.good))
    assert rejected(off, v.r, R.U_BF16)
