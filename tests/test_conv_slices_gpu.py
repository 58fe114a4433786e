"""The forward / data-gradient convolution kernels of csrc/igemm.hip on CHANNEL SLICES of wider NHWC tensors and in
GROUPED launches, called directly through the C ABI (sbagan._lib), compared element by element with the float64
reference of tests/conv_ref.py evaluated on the kernel's own (storage-rounded) operands.

M = N * OHs * OWs rows, nslabs = ntaps * Cin / 32 (bf16) or / 16 (f32).  Case numbers are the ids of SINGLE below;
tests/test_conv_slices_plan_cpu.py asks sba_conv_igemm_plan, without a device, for the (family, tile, splits) written
beside every case, so the "covered by" column cannot go stale.

kernel / branch                     host condition that selects it                          covered by
----------------------------------  ------------------------------------------------------  ----------------------------
igemm_dma2_kernel (family 1)        bf16, Cin % 64 == 0, tile != 11, not a halo geometry    1, 2, 5, 6, 11; G1, G3
  rule tile                         g.tile = 0: M <= 2048 -> row 1 of the tile table        1, 2-t0, 5-rule, 6, 11
  forced tile                       g.tile = 3 / 7 / 12 / 14, g.ksplit = 1                  2-t3 .. 2-t14
  split-K + splitk_finish_kernel    workspace >= 4 M Cout bytes, nslabs >= 16, Cout % 4     5-rule-full (9 splits),
                                    == 0 (rule), or g.tile + g.ksplit > 1                   5-t1k3-full (3 splits)
  workspace too small               4 M Cout > workspace_bytes: one split                   5-*-small (== no workspace)
igemm_dma_kernel (family 2)         bf16, Cin % 64 == 32, tile != 11                        3 (rule, 1, 5, 9), 7; G2
igemm_kernel (family 3)             bf16: g.tile = 11;  f32: always                         4;  8a, 8b (18 splits)
tile_epilogue, 16-byte row stores   bf16 / binary16 output, chunk inside Cout               every bf16 case
  scalar ragged-Cout tail           Cout % 8 != 0 (needs y_cstride: dense is refused)       2 (Cout = 44)
  f32 direct stores                 f32                                                     8a, 8b (no split)
  statistics                        stats != NULL                                           4, 5, 8, 9, 11
  binary16 output                   SBA_BF16_YH (sba_conv_igemm)                            11
splitk_finish_kernel                behind every split launch; bias / ReLU / addend / mask  5 (bf16), 8b (f32)
sub-grid store (osy = 2, ooy, oox)  geometry                                                7 (four parity classes), G1
stride-2 gather                     g.sy = 2                                                6, G1 item 3x3s2
conv3x3_halo_kernel (family 0)      bf16, 3x3 same, Cin 64 / 128, Cout % 64 == 0, OH % 8    9-64-u0-l0, 9-64-u1-l0
                                    == 0, OW % 32 == 0, >= 128 tiles; w_layout 0; ups 0 / 1
conv3x3_halo3_kernel (family 0)     the same with w_layout = 1 (fragment-major weights)     9-64-u0-l1, 9-64-u1-l1,
                                                                                            9-128-u0-l1 (two chunks)
conv3x3_halo3g_kernel (family 4)    w_layout = 1, any stride-1 3x3 window, Cin % 32 == 0,   10a <32,1>, 10b <64,2>,
  <CIN, TN>                         Cout % 32 == 0, >= 128 tiles; CIN = 64 when Cin % 64    10c <32,2>, 10d <32,1>,
                                    == 0 else 32; TN = 2 when Cout % 64 == 0 else 1         10e <64,2>, 10f <64,1>
igemm_dma2_group_kernel             sba_conv_igemm_group, every Cin % 64 == 0; tile 0 (= 1), G1: n = 2, 5, 8;
                                    1, 3, 5, 7                                              heterogeneous items
igemm_dma_group_kernel              some member Cin % 64 == 32: gen-1 form of row `group`   G2: tiles 1, 3, 5, 7 (as 5)
grouped split-K +                   sba_conv_igemm_group_splitk, ksplit > 1, workspace      G3: ksplit 2, 3, 8; unequal
splitk_finish_group_kernel          >= sum 4 M Cout, every Cin % 64 == 0                    (M, Cout): grid by max_m / max_co
  fallbacks to one split            workspace too small; a member with Cin = 96             G3
every SBA_E_ARG condition           --                                                      test_slices_refusals

Conventions.  Operands come from oracle.fill, rounded to the storage type; weights are scaled by 1 / sqrt(ntaps Cin).
x lives in a wider tensor (bf16: x_cstride = Cin + 24, x_coff = 8; f32: Cin + 12, 4) whose other channels, and
PAD_ROWS pixel rows behind the last pixel, are NaN.  y lives in a wider and longer tensor prefilled with NaN: after
the launch every element the launch does not own -- other channels, the pad rows, the pixels of another parity class --
must hold its prefill BIT FOR BIT, every element it owns must be finite and inside the bound.  The dense twin
(x_cstride = y_cstride = 0) must give the same bits (a bf16 Cout that is no multiple of 8 has no dense form: the twin
then keeps the narrowest legal y_cstride and the refusal of 0 is asserted).  Masks hold positive and negative values,
+0 and -0.  An addend is given once as a tensor of its own and once in place (addend == y, the window prefilled with
it), which is how the Inception trunk's data gradients call the kernels; both must give the same bits.

Bounds (tests/conv_ref.py; tests/test_conv_ref_cpu.py shows that a correct implementation meets them at every element
of every case here and that they reject the errors they are there for).  With ref the float64 result on the rounded
operands, pre its value before the addend, A the same contraction on absolute values (+ |bias|), u the unit roundoff
of the output type (2^-8 bf16, 2^-11 binary16, 2^-24 f32) and c = 1e-5 for the f32 accumulation (the MFMA chains and
the split-K atomics measure below 1e-7 A):
    |got - ref| <= u |ref| + c A                one rounding of the f32 accumulator
    |got - ref| <= u |pre| + u |ref| + c A      16-bit output with an addend: tile_epilogue rounds the accumulator to
                                                bf16 and add_bf16x2 rounds the sum again (splitk_finish_kernel adds in
                                                f32 and rounds once: inside the same bound)
    got == +-0                                  where !(mask > 0)
    statistics: |got - ref| <= c sum |acc| and c sum acc^2 per channel (sums of the f32 accumulators, before the bias)
Largest observed err / bound on an MI355X: 0.984 (bf16: the rounding itself; the emulation of test_conv_ref_cpu.py
gives the same figures to three digits), 0.013 for the f32 outputs, 0.024 for the statistics.

A launch with S > 1 K splits adds its S partial tiles with f32 atomics in arrival order: every add rounds a partial sum
of magnitude <= A, so the f32 sums of two runs differ by up to 2 S 2^-24 A before the epilogue rounds them.  Where a
twin or an in-place run is compared with a split run the two may therefore differ by 2 S 2^-24 A + 2 u max(|a|, |b|)
(neighbours in the output type; + 2 u |pre| behind a 16-bit addend, whose first rounding may fall either way), never
more; without a split the bits must be equal.

Grouped launches without a K split are compared with a single sba_conv_igemm_bias launch of each item forced to the
same row of the tile table: same body, same K order, so the bits must be equal.  One legitimate exception, read off the
two call sites (group_dispatch / launch_igemm): when some member has Cin % 64 == 32 the WHOLE group runs the gen-1 body
(32-channel slabs), while a member with Cin % 64 == 0 launched alone takes the gen-2 body (64-channel slabs, four MFMA
steps per stage against two): the products are the same and meet in the same K order, but the bodies are different
instantiations, so for those members one bf16 unit in the last place is allowed instead of bit equality.
"""
import ctypes
import zlib
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_ref as R  # noqa: E402
from oracle import fill  # noqa: E402

NAN = float('nan')
PAD_ROWS = 3                    # NaN pixel rows behind the last pixel of every activation tensor
PAD = 64                        # NaN elements behind flat f32 buffers
E_ARG = -1
# mode -> (dtype code, operand storage, output storage, elements per 16-byte vector, unit roundoff of the output)
MODES = {'f32': (0, torch.float32, torch.float32, 4, R.U_F32), 'bf16': (1, torch.bfloat16, torch.bfloat16, 8, R.U_BF16),
         'yh': (2, torch.bfloat16, torch.float16, 8, R.U_F16)}


# ------------------------------------------------------------------ case tables (plain data: the CPU tests read them)
def fwd(KH, KW, ph, pw, IH, IW, s=1):
    """(taps, OH, OW) of a KH x KW window, padding (ph, pw), stride s"""
    return R.window_taps(KH, KW, ph, pw), (IH + 2 * ph - KH) // s + 1, (IW + 2 * pw - KW) // s + 1


def dgrad1(KH, KW, ph, pw, IH, IW):
    """(taps, OH, OW) of the data gradient of a stride-1 KH x KW conv with padding (ph, pw): IH x IW is dy's map"""
    return [(ph - t // KW, pw - t % KW) for t in range(KH * KW)], IH + KH - 1 - 2 * ph, IW + KW - 1 - 2 * pw


def case(id, mode, N, IH, IW, Cin, Cout, tow, plan=None, s=1, ups=0, sub=None, tile=0, ksplit=0, epi='none',
         stats=False, ws='none', layout=0):
    """tow = (taps, OH, OW); sub = (OHs, OWs, osy, ooy, oox) of a sub-grid launch; epi: 'none' | 'bias_relu' |
    'add_mask'; ws: split-K workspace 'none' | 'full' (4 M Cout bytes) | 'small' (16 bytes short);
    plan = what sba_conv_igemm_plan must answer: (family, tile id or configuration, K splits)"""
    taps, OH, OW = tow
    OHs, OWs, osy, ooy, oox = sub if sub else (OH, OW, 1, 0, 0)
    return NS(id=id, mode=mode, N=N, IH=IH, IW=IW, Cin=Cin, Cout=Cout, taps=taps, OH=OH, OW=OW, OHs=OHs, OWs=OWs, s=s,
              osy=osy, ooy=ooy, oox=oox, ups=ups, tile=tile, ksplit=ksplit, epi=epi, stats=stats, ws=ws, layout=layout,
              plan=plan)


def _single_cases():
    C = []
    m17 = fwd(3, 3, 1, 1, 17, 17)
    C.append(case('1', 'bf16', 2, 17, 17, 64, 96, m17, (1, 1, 1), epi='bias_relu'))
    for t in (0, 3, 7, 12, 14):
        C.append(case('2-t%d' % t, 'bf16', 2, 17, 17, 128, 44, fwd(1, 7, 0, 3, 17, 17), (1, t or 1, 1), tile=t,
                      ksplit=1 if t else 0, epi='add_mask'))
    for t in (0, 1, 5, 9):
        for epi in ('bias_relu', 'add_mask'):
            C.append(case('3-t%d-%s' % (t, epi), 'bf16', 2, 17, 17, 96, 72, m17, (2, t or 1, 1), tile=t,
                          ksplit=1 if t else 0, epi=epi))
    C.append(case('4', 'bf16', 2, 17, 17, 96, 136, m17, (3, 4, 1), tile=11, ksplit=1, epi='add_mask', stats=True))
    for name, t, k, ws, split in (('rule-full', 0, 0, 'full', 9), ('t1k3-full', 1, 3, 'full', 3),
                                  ('rule-small', 0, 0, 'small', 1), ('t1k3-small', 1, 3, 'small', 1)):
        for epi in ('bias_relu', 'add_mask'):
            C.append(case('5-%s-%s' % (name, epi), 'bf16', 2, 8, 8, 256, 72, fwd(3, 3, 1, 1, 8, 8), (1, 1, split),
                          tile=t, ksplit=k, epi=epi, stats=True, ws=ws))
    C.append(case('6', 'bf16', 2, 35, 35, 64, 96, fwd(3, 3, 0, 0, 35, 35, 2), (1, 1, 1), s=2, epi='bias_relu'))
    C.append(case('8a', 'f32', 2, 9, 9, 48, 44, fwd(3, 3, 1, 1, 9, 9), (3, 3, 1), epi='add_mask', stats=True))
    C.append(case('8b', 'f32', 2, 8, 8, 256, 72, fwd(3, 3, 1, 1, 8, 8), (3, 3, 18), epi='add_mask', stats=True,
                  ws='full'))
    for Cin, ups, lay in ((64, 0, 0), (64, 0, 1), (64, 1, 0), (64, 1, 1), (128, 0, 1)):
        S = 32 if ups else 64
        C.append(case('9-%d-u%d-l%d' % (Cin, ups, lay), 'bf16', 8, S, S, Cin, 64, (R.window_taps(3, 3, 1, 1), 64, 64),
                      (0, ups, 1), ups=ups, epi='add_mask', stats=True, layout=lay))
    C.append(case('10a', 'bf16', 13, 35, 35, 32, 32, fwd(3, 3, 0, 0, 35, 35), (4, 32, 1), epi='bias_relu', layout=1))
    C.append(case('10b', 'bf16', 13, 35, 35, 64, 128, fwd(3, 3, 1, 1, 35, 35), (4, 64, 1), epi='bias_relu', layout=1))
    C.append(case('10c', 'bf16', 13, 35, 35, 96, 64, fwd(3, 3, 1, 1, 35, 35), (4, 32, 1), epi='bias_relu', layout=1))
    C.append(case('10d', 'bf16', 13, 33, 33, 32, 32, dgrad1(3, 3, 0, 0, 33, 33), (4, 32, 1), epi='add_mask', layout=1))
    C.append(case('10e', 'bf16', 13, 35, 35, 128, 64, dgrad1(3, 3, 1, 1, 35, 35), (4, 64, 1), epi='add_mask', layout=1))
    C.append(case('10f', 'bf16', 13, 35, 35, 64, 96, dgrad1(3, 3, 1, 1, 35, 35), (4, 64, 1), epi='add_mask', layout=1))
    C.append(case('11', 'yh', 2, 17, 17, 64, 96, m17, (1, 1, 1), stats=True))
    return C


def s2_class_taps(KH, KW, py, px):
    """parity class (py, px) of the data gradient of a stride-2 unpadded KH x KW conv: the kernel cells it uses and the
    taps into dy (input pixel (2 a + py, 2 b + px) collects dy[a + ty][b + tx] * w[kh][kw] with 2 ty = py - kh)"""
    sel = [(kh, kw) for kh in range(KH) if (kh - py) % 2 == 0 for kw in range(KW) if (kw - px) % 2 == 0]
    return sel, [((py - kh) // 2, (px - kw) // 2) for kh, kw in sel]


def _dgrad_s2_cases():
    """case 7: data gradient of the 3x3 stride-2 unpadded conv 64 -> 96 on 17 x 17 (output 8 x 8): dy [2, 8, 8, 96] ->
    dx, a 64-channel slice of a [2, 17, 17, .] tensor, as four parity classes with an in-place addend and a mask"""
    C = []
    for cls in range(4):
        py, px = cls // 2, cls % 2
        _, taps = s2_class_taps(3, 3, py, px)
        C.append(case('7-c%d' % cls, 'bf16', 2, 8, 8, 96, 64, (taps, 17, 17), (2, 1, 1),
                      sub=((17 - py + 1) // 2, (17 - px + 1) // 2, 2, py, px), epi='add_mask'))
    return C


SINGLE = _single_cases()
DGRAD_S2 = _dgrad_s2_cases()
PLAN_CASES = SINGLE + DGRAD_S2


def item(id, N, IH, IW, Cin, Cout, KH, KW, ph, pw, epi, xb, xco, yb, yco, s=1, sub=None, inplace=False):
    """one member of a grouped launch: a bf16 case bound to channel slices of named tensors; sub = (OH, OW, osy, ooy,
    oox): the member writes its (whole) output as a sub-grid of an OH x OW map"""
    taps, oh, ow = fwd(KH, KW, ph, pw, IH, IW, s)
    if sub:
        c = case(id, 'bf16', N, IH, IW, Cin, Cout, (taps, sub[0], sub[1]), s=s, sub=(oh, ow) + tuple(sub[2:]), epi=epi)
    else:
        c = case(id, 'bf16', N, IH, IW, Cin, Cout, (taps, oh, ow), s=s, epi=epi)
    c.xb, c.xco, c.yb, c.yco, c.inplace = xb, xco, yb, yco, inplace
    return c


# name -> (N, H, W, channel stride, [valid channel range of an input tensor])
G1_BUFS = {'X': (2, 17, 17, 216, (8, 200)), 'Y': (2, 17, 17, 416, None), 'X5': (3, 9, 9, 88, (8, 72)),
           'Y5': (3, 9, 9, 104, None)}
G1 = [
    item('1x1', 2, 17, 17, 128, 64, 1, 1, 0, 0, 'bias_relu', 'X', 8, 'Y', 8),
    item('1x7', 2, 17, 17, 128, 96, 1, 7, 0, 3, 'add_mask', 'X', 8, 'Y', 72),
    item('7x1', 2, 17, 17, 64, 40, 7, 1, 3, 0, 'none', 'X', 136, 'Y', 168),
    item('3x3s2', 2, 17, 17, 64, 96, 3, 3, 0, 0, 'bias_relu', 'X', 136, 'Y', 208, s=2, sub=(17, 17, 2, 1, 0)),   # M = 128
    item('5x5', 3, 9, 9, 64, 72, 5, 5, 2, 2, 'add_mask', 'X5', 8, 'Y5', 16, inplace=True),
    item('1x1-b', 2, 17, 17, 64, 32, 1, 1, 0, 0, 'none', 'X', 136, 'Y', 304),
    item('1x1-c', 2, 17, 17, 64, 32, 1, 1, 0, 0, 'add_mask', 'X', 136, 'Y', 336, inplace=True),
    item('1x1-d', 2, 17, 17, 64, 32, 1, 1, 0, 0, 'bias_relu', 'X', 136, 'Y', 368),
]
# G2: the 7x1 member reads 96 channels: the whole group falls back to the gen-1 body
G2 = G1[:2] + [item('7x1-96', 2, 17, 17, 96, 40, 7, 1, 3, 0, 'none', 'X', 104, 'Y', 168)] + G1[3:5]
G3_BUFS = {'XP': (2, 4, 4, 280, (8, 264)), 'YP': (2, 4, 4, 104, None), 'XQ': (2, 8, 8, 152, (8, 136)),
           'YQ': (2, 8, 8, 168, None), 'XR': (2, 6, 6, 120, (8, 104)), 'YR': (2, 6, 6, 72, None)}
G3 = [      # (M, Cout) = (32, 72), (128, 136), (72, 40); 36, 18 and 9 slabs of 64 channels
    item('g3-256', 2, 4, 4, 256, 72, 3, 3, 1, 1, 'bias_relu', 'XP', 8, 'YP', 16),
    item('g3-128', 2, 8, 8, 128, 136, 3, 3, 1, 1, 'add_mask', 'XQ', 8, 'YQ', 16, inplace=True),
    item('g3-64', 2, 6, 6, 64, 40, 3, 3, 1, 1, 'none', 'XR', 8, 'YR', 16),
]
G3_96 = G3[:2] + [item('g3-96', 2, 6, 6, 96, 40, 3, 3, 1, 1, 'add_mask', 'XR', 8, 'YR', 16)]
GROUP_ITEMS = G1 + G2[2:3] + G3 + G3_96[2:3]


# ------------------------------------------------------------------ operands and references (CPU; computed once)
def slices(c, sliced=True):
    """(x_cstride, x_coff, y_cstride, y_coff) of the sliced run, or of the dense twin"""
    V = MODES[c.mode][3]
    if sliced:
        return c.Cin + 3 * V, V, (c.Cout + V - 1) // V * V + 5 * V, 2 * V
    return 0, 0, (0 if c.Cout % V == 0 else (c.Cout + V - 1) // V * V), 0


def geom_of(c, sl=(0, 0, 0, 0)):
    return R.geom(c.N, c.IH, c.IW, c.Cin, c.OH, c.OW, c.Cout, c.taps, sy=c.s, OHs=c.OHs, OWs=c.OWs, osy=c.osy,
                  ooy=c.ooy, oox=c.oox, ups=c.ups, xcs=sl[0], xco=sl[1], ycs=sl[2], yco=sl[3],
                  relu=1 if c.epi == 'bias_relu' else 0, tile=c.tile, ksplit=c.ksplit, w_layout=c.layout)


def ref_key(c):
    return (c.mode, c.N, c.IH, c.IW, c.Cin, c.Cout, tuple(c.taps), c.OH, c.OW, c.OHs, c.OWs, c.s, c.osy, c.ooy, c.oox,
            c.ups, c.epi)


def stored(t, dt):
    """t rounded to storage type dt, as float32"""
    return t.to(dt).float()


def operands(c, x=None, w=None):
    """dense CPU operands of a case, already rounded to their storage types (float32 tensors): x [N, IH, IW, Cin],
    w [Cout][ntaps][Cin], bias [Cout] | None, add / mask [N, OH, OW, Cout] | None (values at EVERY pixel: a sub-grid
    launch uses its own)"""
    _, st, so, _, _ = MODES[c.mode]
    tag = zlib.crc32(repr(ref_key(c)).encode()) & 0xFFFFF
    nt = len(c.taps)
    if x is None:
        x = stored(fill.unit((c.N, c.IH, c.IW, c.Cin), tag), st)
    if w is None:
        w = stored(fill.unit((c.Cout, nt, c.Cin), tag + 1) / float(np.sqrt(nt * c.Cin)), st)
    o = NS(x=x, w=w, bias=None, add=None, mask=None)
    if c.epi == 'bias_relu':
        o.bias = 0.1 * fill.uniform((c.Cout,), tag + 2)
    if c.epi == 'add_mask':
        shape = (c.N, c.OH, c.OW, c.Cout)
        o.add = stored(fill.unit(shape, tag + 3), so)
        m = stored(fill.unit(shape, tag + 4), so).flatten()
        i = torch.arange(m.numel())
        m[i % 5 == 1] = 0.0
        m[i % 5 == 3] = -0.0
        o.mask = m.view(shape)
    return o


_REF = {}


def reference(c, o=None, key=None):
    """conv_ref.launch of the dense operands of a case, computed once per distinct (geometry, epilogue)"""
    key = key or ref_key(c)
    if key not in _REF:
        o = o or operands(c)
        _REF[key] = (o, R.launch(o.x, o.w, geom_of(c), o.bias, o.add, o.mask))
    return _REF[key]


# ------------------------------------------------------------------ device side
@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def L():
    from sbagan import _lib
    return _lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def p(t):
    return None if t is None else t.data_ptr()


def cgeom(g):
    cg = L().ConvGeom()
    for name, _ in cg._fields_:
        if name not in ('ty', 'tx'):
            setattr(cg, name, getattr(g, name))
    for t in range(g.ntaps):
        cg.ty[t], cg.tx[t] = g.ty[t], g.tx[t]
    return cg


def wide(val, cs, co, dt, fill_value=NAN):
    """[N, H, W, C] values at channels [co, co + C) of a [N * H * W + PAD_ROWS][cs] CPU tensor of type dt"""
    N, H, W, C = val.shape
    buf = torch.full((N * H * W + PAD_ROWS, cs), fill_value, dtype=torch.float32)
    buf[:N * H * W, co:co + C] = val.reshape(-1, C)
    return buf.to(dt)


def owned_only(val, g):
    """val [N, OH, OW, Cout] with everything the launch of geometry g does not own replaced by NaN"""
    gd = NS(**vars(g))
    gd.y_coff = 0
    out = torch.full(val.shape, NAN)
    R.window(out, gd)[...] = R.window(val, gd)
    return out


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def frag_major(w, dev):
    """the fragment-major copy (sba_pack_frag_multi) of a packed bf16 device weight [R][taps][K]"""
    from sbagan import ops
    Rr, taps, K = w.shape
    dst = torch.zeros((Rr + 63) // 64 * 64 * taps * K, dtype=w.dtype, device=dev)
    ops._pack_frag([(w, dst, Rr, taps, K)], dev)
    return dst


def check_window(got_buf, y0_buf, g, r, u, name):
    """NaN / prefill guard and the elementwise bound of one launch's output tensor; returns the window's bits"""
    rows = g.N * g.OH * g.OW
    cs = g.y_cstride or g.Cout
    got, y0 = got_buf.detach().cpu().view(-1, cs), y0_buf.detach().cpu().view(-1, cs)
    own = torch.zeros(got.shape, dtype=torch.bool)
    R.window(own[:rows].view(g.N, g.OH, g.OW, cs), g)[...] = True
    assert torch.equal(bits(got)[~own], bits(y0)[~own]), '%s: wrote outside what the launch owns' % name
    win = R.window(got[:rows].view(g.N, g.OH, g.OW, cs), g)
    ratio = R.worst(win, r, u)
    print('%-34s y      err / bound = %.3f' % (name, ratio))
    assert ratio <= 1.0, '%s: worst err / bound = %.3f' % (name, ratio)
    return bits(win)


def check_stats(buf, Cout, r, name):
    s = buf.detach().cpu().double()
    n = L().lib.sba_bn_stat_slots() * 2 * Cout
    assert bool(torch.isnan(s[n:]).all()), '%s: statistics written past their end' % name
    assert bool(torch.isfinite(s[:n]).all()), name
    s = s[:n].view(-1, 2 * Cout).sum(0)
    want = R.stats(r)
    a = float(((s[:Cout] - want.sum).abs() / want.sum_abs.clamp(min=1e-30)).max())
    b = float(((s[Cout:] - want.sumsq).abs() / want.sumsq_abs.clamp(min=1e-30)).max())
    print('%-34s stats  err / bound = %.3f (sum), %.3f (sumsq)' % (name, a / R.C_ACC, b / R.C_ACC))
    assert a <= R.C_ACC and b <= R.C_ACC, '%s: statistics %.3e / %.3e of the absolute sums' % (name, a, b)


def same_or_neighbour(a, b, dt, exact, name, r=None, splits=0):
    """two results of the same launch: equal bits, or neighbours (module docstring).  r, splits: the launch adds
    `splits` partial tiles of reference r with f32 atomics in arrival order"""
    if exact:
        assert torch.equal(a, b), '%s: bits differ' % name
        return
    fa, fb = a.view(dt).double(), b.view(dt).double()
    u = {torch.bfloat16: R.U_BF16, torch.float16: R.U_F16, torch.float32: R.U_F32}[dt]
    tol = 2 * u * torch.maximum(fa.abs(), fb.abs())
    if r is not None:
        tol = tol + 2 * splits * R.U_F32 * r.A + (2 * u * r.pre.abs() if r.add and u > R.U_F32 else 0.0)
    assert bool(((fa - fb).abs() <= tol).all()), '%s: more than the order of the last sums apart' % name


def tensors(c, o, sl, dev, inplace):
    """device tensors of one launch: x (wide), w, bias, the CPU prefill of y, addend and mask laid out like y"""
    _, st, so, _, _ = MODES[c.mode]
    g = geom_of(c, sl)
    t = NS(g=g, x=wide(o.x, sl[0] or c.Cin, sl[1], st).to(dev), w=o.w.to(st).to(dev).contiguous(),
           bias=None if o.bias is None else o.bias.to(dev), add=None, mask=None)
    ycs = sl[2] or c.Cout
    t.y0 = torch.full((c.N * c.OH * c.OW + PAD_ROWS, ycs), NAN, dtype=so)
    if o.add is not None:
        if inplace:
            t.y0 = wide(o.add, ycs, sl[3], so)
        else:
            t.add = wide(owned_only(o.add, g), ycs, sl[3], so).to(dev)
        t.mask = wide(owned_only(o.mask, g), ycs, sl[3], so).to(dev)
    return t


def launch_single(c, t, dev, y, ws_mode=None):
    """one sba_conv_igemm(_bias) launch of case c on tensors t into y; returns the statistics buffer (or None)"""
    lib = L().lib
    code = MODES[c.mode][0]
    M = c.N * c.OHs * c.OWs
    ws_mode = ws_mode or c.ws
    ws = None if ws_mode == 'none' else torch.zeros(M * c.Cout, dtype=torch.float32, device=dev)
    ws_bytes = 0 if ws is None else (4 * M * c.Cout - (16 if ws_mode == 'small' else 0))
    stats = None
    if c.stats:
        stats = torch.full((lib.sba_bn_stat_slots() * 2 * c.Cout + PAD,), NAN, dtype=torch.float32, device=dev)
        stats[:-PAD] = 0
    w = frag_major(t.w, dev) if c.layout == 1 else t.w
    cg = cgeom(t.g)
    add = y if (t.add is None and c.epi == 'add_mask') else t.add
    if c.mode == 'yh':
        rc = lib.sba_conv_igemm(code, p(t.x), p(w), p(y), None, p(stats), ctypes.byref(cg), p(ws), ws_bytes, stream())
    else:
        rc = lib.sba_conv_igemm_bias(code, p(t.x), p(w), p(y), p(add), p(stats), p(t.bias), p(t.mask), ctypes.byref(cg),
                                     p(ws), ws_bytes, stream())
    torch.cuda.synchronize()
    assert rc == 0, '%s: status %d' % (c.id, rc)
    if ws is not None:
        assert int(ws.count_nonzero()) == 0, '%s: the split-K workspace is not left zero-filled' % c.id
    return stats


def run_single(c, dev, sliced=True, inplace=False, ws_mode=None, tag=''):
    o, r = reference(c)
    sl = slices(c, sliced)
    t = tensors(c, o, sl, dev, inplace)
    y = t.y0.to(dev)
    stats = launch_single(c, t, dev, y, ws_mode)
    name = 'case %s%s' % (c.id, tag)
    b = check_window(y, t.y0, t.g, r, MODES[c.mode][4], name)
    if stats is not None:
        check_stats(stats, c.Cout, r, name)
    return b



@pytest.mark.parametrize('c', SINGLE, ids=[c.id for c in SINGLE])
def test_slices_single_launch(dev, c):
    so = MODES[c.mode][2]
    exact = c.plan[2] == 1                  # no K split: no atomics, the same sums in the same order
    a = run_single(c, dev)
    V = MODES[c.mode][3]
    if c.Cout % V:                          # no dense form: y_cstride = 0 means Cout, which is no whole vector
        cg = cgeom(geom_of(c, (0, 0, 0, 0)))
        plan = (ctypes.c_int * 3)()
        assert L().lib.sba_conv_igemm_plan(MODES[c.mode][0], ctypes.byref(cg), 0, plan) == E_ARG
    d = run_single(c, dev, sliced=False, tag=' dense')
    r = reference(c)[1]
    same_or_neighbour(a, d, so, exact, 'case %s: sliced against dense' % c.id, r, c.plan[2])
    if c.epi == 'add_mask':
        b = run_single(c, dev, inplace=True, tag=' in place')
        same_or_neighbour(a, b, so, exact, 'case %s: addend in place against a separate addend' % c.id, r, c.plan[2])
    if c.ws == 'small':                     # the too-small workspace must behave exactly like no workspace
        n = run_single(c, dev, ws_mode='none', tag=' no ws')
        same_or_neighbour(a, n, so, True, 'case %s: workspace too small against none' % c.id)


def test_slices_stride2_dgrad_classes(dev):
    """case 7: the four parity classes of a stride-2 data gradient written into ONE 64-channel slice, operands packed
    by inception_hip._Conv, the addend in place (and once separate), the mask of the tensor the gradient completes"""
    from sbagan.inception_hip import _Conv
    dt = torch.bfloat16
    conv = torch.nn.Conv2d(64, 96, 3, stride=2, padding=0, bias=False)
    bn = torch.nn.BatchNorm2d(96, eps=1e-3).eval()
    with torch.no_grad():
        conv.weight.copy_(fill.unit((96, 64, 3, 3), 11) / 24.0)
        bn.weight.copy_(1.0 + 0.2 * fill.uniform((96,), 12))
        bn.bias.copy_(0.1 * fill.uniform((96,), 13))
        bn.running_mean.copy_(0.1 * fill.uniform((96,), 14))
        bn.running_var.copy_(1.0 + 0.3 * fill.uniform((96,), 15))
    Lc = _Conv(conv.to(dev), bn.to(dev), dt, relu=True)
    assert (Lc.Ip, Lc.Op) == (64, 96)
    dy = stored(fill.unit((2, 8, 8, 96), 16), dt)
    base = operands(DGRAD_S2[0])            # the addend and the mask of the whole 17 x 17 x 64 tensor
    results = {}
    for sliced, inplace in ((True, True), (True, False), (False, False)):
        y = y0 = None
        for cls, c in enumerate(DGRAD_S2):
            assert [tuple(a) for a in Lc.dtaps[cls]] == [tuple(a) for a in c.taps]
            o = operands(c, x=dy, w=Lc.w_dgrad[cls].float().cpu())
            o.add, o.mask = base.add, base.mask
            _, r = reference(c, o, key=('7', cls))
            t = tensors(c, o, slices(c, sliced), dev, inplace)
            if y is None:
                y0, y = t.y0, t.y0.to(dev)
            before = y.clone()
            launch_single(c, t, dev, y)
            name = 'case %s%s%s' % (c.id, '' if sliced else ' dense', ' in place' if inplace else '')
            results[(sliced, inplace, cls)] = check_window(y, before, t.g, r, R.U_BF16, name)
        g = t.g
        cs = g.y_cstride or g.Cout
        full = y.cpu().view(-1, cs)[:2 * 17 * 17, g.y_coff:g.y_coff + 64]
        assert bool(torch.isfinite(full.float()).all()), 'the four classes together cover the slice'
    for cls in range(4):
        assert torch.equal(results[(True, True, cls)], results[(True, False, cls)]), 'in place against separate'
        assert torch.equal(results[(True, False, cls)], results[(False, False, cls)]), 'sliced against dense'


# ------------------------------------------------------------------ grouped launches
def group_operands(items, bufs):
    """per item: its operands (x cut from the shared input tensors) and its reference"""
    xs = {}
    out = []
    for c in items:
        if c.xb not in xs:
            N, H, W, cs, _ = bufs[c.xb]
            xs[c.xb] = stored(fill.unit((N, H, W, cs), zlib.crc32(c.xb.encode()) & 0xFFFF), torch.bfloat16)
        o = operands(c, x=xs[c.xb][..., c.xco:c.xco + c.Cin].contiguous())
        out.append(reference(c, o, key=('group', c.id, c.xb, c.xco)))
    return xs, out


def group_tensors(items, bufs, dev):
    """device tensors of a grouped launch: the shared inputs (NaN outside their valid channels), the CPU prefill of
    every output tensor, per item the weights, bias, addend and mask"""
    dt = torch.bfloat16
    xs, refs = group_operands(items, bufs)
    T = NS(x={}, y0={}, it=[], refs=refs)
    for name, xv in xs.items():
        lo, hi = bufs[name][4]
        v = torch.full(xv.shape, NAN)
        v[..., lo:hi] = xv[..., lo:hi]
        T.x[name] = wide(v, xv.shape[-1], 0, dt).to(dev)
    for c in items:
        N, H, W, cs, _ = bufs[c.yb]
        assert (N, H, W) == (c.N, c.OH, c.OW)
        if c.yb not in T.y0:
            T.y0[c.yb] = torch.full((N * H * W + PAD_ROWS, cs), NAN, dtype=dt)
    for c, (o, r) in zip(items, refs):
        cs = bufs[c.yb][3]
        g = geom_of(c, (bufs[c.xb][3], c.xco, cs, c.yco))
        e = NS(c=c, g=g, w=o.w.to(dt).to(dev).contiguous(), bias=None if o.bias is None else o.bias.to(dev), add=None,
               mask=None, inplace=False)
        if o.add is not None:
            if c.inplace:
                rows = c.N * c.OH * c.OW
                T.y0[c.yb][:rows, c.yco:c.yco + c.Cout] = o.add.reshape(rows, c.Cout).to(dt)
                e.inplace = True
            else:
                e.add = wide(owned_only(o.add, g), cs, c.yco, dt).to(dev)
            e.mask = wide(owned_only(o.mask, g), cs, c.yco, dt).to(dev)
        T.it.append(e)
    return T


def run_group(dev, items, bufs, tile, name, ksplit=None, ws_mode='full', single=None):
    """one grouped launch, every item checked.  single = (tile id, exact(item) -> bool): also compare every item with a
    single sba_conv_igemm_bias launch forced to that tile id, bit for bit where exact(item).  Returns {item id: bits}."""
    lib = L().lib
    T = group_tensors(items, bufs, dev)
    ys = dict((k, v.to(dev)) for k, v in T.y0.items())
    arr = (L().ConvGroupItem * len(items))()
    keep = []
    for a, e in zip(arr, T.it):
        cg = cgeom(e.g)
        keep.append(cg)
        y = ys[e.c.yb]
        a.x, a.w, a.y = p(T.x[e.c.xb]), p(e.w), p(y)
        a.addend = p(y) if e.inplace else p(e.add)
        a.bias, a.relu_mask = p(e.bias), p(e.mask)
        a.g = ctypes.pointer(cg)
    if ksplit is None:
        rc = lib.sba_conv_igemm_group(1, len(items), arr, tile, stream())
    else:
        need = sum(c.N * c.OHs * c.OWs * c.Cout for c in items)
        ws = None if ws_mode == 'none' else torch.zeros(need, dtype=torch.float32, device=dev)
        ws_bytes = 0 if ws is None else 4 * need - (16 if ws_mode == 'small' else 0)
        rc = lib.sba_conv_igemm_group_splitk(1, len(items), arr, tile, ksplit, p(ws), ws_bytes, stream())
    torch.cuda.synchronize()
    assert rc == 0, '%s: status %d' % (name, rc)
    if ksplit is not None and ws is not None:
        assert int(ws.count_nonzero()) == 0, '%s: the split-K workspace is not left zero-filled' % name
    # nothing outside the union of the items' windows changed (no item writes into a neighbour's slice: each window
    # is then checked against its own reference)
    for yb, y in ys.items():
        N, H, W, cs, _ = bufs[yb]
        own = torch.zeros((N * H * W + PAD_ROWS, cs), dtype=torch.bool)
        for e in T.it:
            if e.c.yb == yb:
                R.window(own[:N * H * W].view(N, H, W, cs), e.g)[...] = True
        assert torch.equal(bits(y)[~own], bits(T.y0[yb])[~own]), '%s: wrote outside the items\' windows of %s' % (name, yb)
    out = {}
    for e, (o, r) in zip(T.it, T.refs):
        N, H, W, cs, _ = bufs[e.c.yb]
        win = R.window(ys[e.c.yb].cpu()[:N * H * W].view(N, H, W, cs), e.g)
        ratio = R.worst(win, r, R.U_BF16)
        print('%-34s y      err / bound = %.3f' % ('%s item %s' % (name, e.c.id), ratio))
        assert ratio <= 1.0, '%s item %s: worst err / bound = %.3f' % (name, e.c.id, ratio)
        out[e.c.id] = bits(win)
    if single:
        stile, exact = single
        for e in T.it:
            y = T.y0[e.c.yb].to(dev)
            g = NS(**vars(e.g))
            g.tile, g.ksplit = stile, 1
            cg = cgeom(g)
            rc = lib.sba_conv_igemm_bias(1, p(T.x[e.c.xb]), p(e.w), p(y), p(y) if e.inplace else p(e.add), None, p(e.bias),
                                         p(e.mask), ctypes.byref(cg), None, 0, stream())
            torch.cuda.synchronize()
            assert rc == 0
            N, H, W, cs, _ = bufs[e.c.yb]
            alone = bits(R.window(y.cpu()[:N * H * W].view(N, H, W, cs), e.g))
            same_or_neighbour(out[e.c.id], alone, torch.bfloat16, exact(e.c),
                              '%s item %s: grouped against a single launch, tile %d' % (name, e.c.id, stile))
    return out


@pytest.mark.parametrize('tile', [0, 1, 3, 5, 7])
def test_slices_group_gen2(dev, tile):
    """G1: five heterogeneous members, every Cin % 64 == 0: igemm_dma2_group_kernel"""
    run_group(dev, G1[:5], G1_BUFS, tile, 'G1 tile %d' % tile, single=(tile or 1, lambda c: True))


@pytest.mark.parametrize('n', [2, 8])
def test_slices_group_member_counts(dev, n):
    run_group(dev, G1[:n], G1_BUFS, 1, 'G1 n = %d' % n, single=(1, lambda c: True))


@pytest.mark.parametrize('tile', [1, 3, 5, 7])
def test_slices_group_gen1_fallback(dev, tile):
    """G2: one member with Cin = 96: igemm_dma_group_kernel for the whole group; tile 7 runs as 5 (no 128-wide gen-1
    group).  A member with Cin % 64 == 0 launched alone takes the gen-2 body: one ulp (module docstring)."""
    run_group(dev, G2, G1_BUFS, tile, 'G2 tile %d' % tile, single=(5 if tile == 7 else tile, lambda c: c.Cin % 64 != 0))


def test_slices_group_splitk_unequal_items(dev):
    """G3: sba_conv_igemm_group_splitk with (M, Cout) = (32, 72), (128, 136), (72, 40) and 36 / 18 / 9 slabs: the
    finishing grid is sized by the largest M and Cout, the shortest member has no slab in the upper splits"""
    one = run_group(dev, G3, G3_BUFS, 1, 'G3 ksplit 1', ksplit=1, single=(1, lambda c: True))
    for ks in (2, 3, 8):
        run_group(dev, G3, G3_BUFS, 1, 'G3 ksplit %d' % ks, ksplit=ks)
    run_group(dev, G3, G3_BUFS, 5, 'G3 tile 5 ksplit 3', ksplit=3)
    small = run_group(dev, G3, G3_BUFS, 1, 'G3 ksplit 3 small ws', ksplit=3, ws_mode='small')
    none = run_group(dev, G3, G3_BUFS, 1, 'G3 ksplit 3 no ws', ksplit=3, ws_mode='none')
    for k in one:                           # both fall back to one split: the bits of the unsplit launch
        assert torch.equal(small[k], one[k]) and torch.equal(none[k], one[k]), k
    run_group(dev, G3_96, G3_BUFS, 1, 'G3 Cin 96 ksplit 3', ksplit=3, single=(1, lambda c: c.Cin % 64 != 0))


# ------------------------------------------------------------------ refusals
def test_slices_refusals(dev):
    """every SBA_E_ARG condition of the slice fields and of the grouped entry points; nothing is written"""
    lib = L().lib
    bf, f32 = torch.bfloat16, torch.float32
    taps = R.window_taps(3, 3, 1, 1)

    def tens(dt, n=1 << 16):
        return torch.full((n,), NAN, dtype=dt, device=dev)

    def untouched(t, what):
        torch.cuda.synchronize()
        assert bool(torch.isnan(t).all()), '%s: wrote before refusing' % what

    for code, dt, V in ((1, bf, 8), (0, f32, 4)):
        Cin, Cout = 64, 64
        x, w, y = torch.zeros(1 << 16, dtype=dt, device=dev), torch.zeros(Cout * 9 * Cin, dtype=dt, device=dev), tens(dt)

        def rc_of(**kw):
            g = R.geom(2, 4, 4, Cin, 4, 4, Cout, taps, **kw)
            return lib.sba_conv_igemm_bias(code, p(x), p(w), p(y), None, None, None, None, ctypes.byref(cgeom(g)), None, 0,
                                           stream())
        bad = [dict(xcs=Cin + 2 * V, xco=3 * V), dict(ycs=Cout + 2 * V, yco=3 * V), dict(xcs=Cin + V + 1, xco=V),
               dict(xcs=Cin + 2 * V, xco=V - 1), dict(ycs=Cout + V + 2, yco=V), dict(ycs=Cout + 2 * V, yco=V // 2),
               dict(xcs=Cin - V), dict(ycs=Cout - V), dict(xco=-V, xcs=Cin + V), dict(yco=-V, ycs=Cout + V)]
        for kw in bad:
            assert rc_of(**kw) == E_ARG, (code, kw)
            untouched(y, kw)
        # sba_conv_wgrad: no slice field
        dw = tens(f32)
        g = R.geom(2, 4, 4, Cin, 4, 4, Cout, taps)
        plan = (ctypes.c_int * L().WGRAD_PLAN_INTS)()
        assert lib.sba_conv_wgrad_plan(code, ctypes.byref(cgeom(g)), 1, 0, plan) == 0
        for kw in (dict(xcs=Cin + V), dict(xcs=Cin + V, xco=V), dict(ycs=Cout + V), dict(ycs=Cout + V, yco=V),
                   dict(xcs=Cin), dict(ycs=Cout)):
            g = R.geom(2, 4, 4, Cin, 4, 4, Cout, taps, **kw)
            assert lib.sba_conv_wgrad(code, p(x), p(x), p(dw), ctypes.byref(cgeom(g)), 1, stream()) == E_ARG, (code, kw)
            untouched(dw, kw)
    # sba_conv_igemm_glu: dense output only
    x, w, y = torch.zeros(1 << 16, dtype=bf, device=dev), torch.zeros(64 * 9 * 64, dtype=bf, device=dev), tens(bf)
    bias = torch.zeros(64, dtype=f32, device=dev)
    plan = (ctypes.c_int * 3)()
    g = R.geom(2, 4, 4, 64, 4, 4, 64, taps)
    assert lib.sba_conv_igemm_glu_plan(1, ctypes.byref(cgeom(g)), 32, plan) == 0
    for kw in (dict(ycs=40), dict(ycs=40, yco=8), dict(ycs=32)):
        cg = cgeom(R.geom(2, 4, 4, 64, 4, 4, 64, taps, **kw))
        assert lib.sba_conv_igemm_glu_plan(1, ctypes.byref(cg), 32, plan) == E_ARG, kw
        assert lib.sba_conv_igemm_glu(1, p(x), p(w), p(bias), p(y), 32, ctypes.byref(cg), stream()) == E_ARG, kw
        untouched(y, kw)
    # binary16 output: whole 16-byte chunks only
    cg = cgeom(R.geom(2, 4, 4, 64, 4, 4, 44, taps, ycs=48))
    assert lib.sba_conv_igemm_plan(1, ctypes.byref(cg), 0, plan) == 0                # (the bf16 form is accepted)
    assert lib.sba_conv_igemm(2, p(x), p(w), p(y), None, None, ctypes.byref(cg), None, 0, stream()) == E_ARG
    untouched(y, 'SBA_BF16_YH, Cout = 44')
    # groups: n = 0, n = 9, f32, a tile id without a grouped form
    cgs = [cgeom(R.geom(2, 4, 4, 64, 4, 4, 64, taps, ycs=64 * 9, yco=64 * i)) for i in range(9)]
    arr = (L().ConvGroupItem * 9)()
    for a, cg in zip(arr, cgs):
        a.x, a.w, a.y, a.g = p(x), p(w), p(y), ctypes.pointer(cg)
    ws = torch.zeros(9 * 32 * 64, dtype=f32, device=dev)
    for dtc, n, tile in ((1, 0, 1), (1, 9, 1), (0, 2, 1), (1, 2, 2), (1, 2, 4), (1, 2, 9), (1, 2, 11), (1, 2, 19), (1, 2, -1)):
        assert lib.sba_conv_igemm_group(dtc, n, arr, tile, stream()) == E_ARG, (dtc, n, tile)
        assert lib.sba_conv_igemm_group_splitk(dtc, n, arr, tile, 2, p(ws), ws.numel() * 4, stream()) == E_ARG, (dtc, n, tile)
        untouched(y, (dtc, n, tile))
    assert int(ws.count_nonzero()) == 0
