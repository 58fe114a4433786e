"""float64 reference of ONE sba_conv_geom launch (include/sbagan_hip.h), written from the header's definition on NHWC
tensors with channel strides and offsets, and the per-element error bounds the convolution tests hold the kernels to.
Needs no device and does not import the library under test.

Definition.  Output pixel (oy, ox) of the OHs x OWs sub-grid of image n reads, for tap t, pixel (oy * sy + ty[t],
ox * sx + tx[t]) of the LOGICAL input -- the physical IH x IW tensor, or its nearest-neighbour x2 upsampling when ups
is set -- zero outside it; channels [x_coff, x_coff + Cin) of rows x_cstride wide:
    acc[n][oy][ox][co] = sum_t sum_ci x[n][iy][ix][x_coff + ci] * w[co][t][ci]
    pre = acc + bias[co];  pre = max(pre, 0) when relu;  ref = pre + addend;  ref = 0 where !(mask > 0)
stored at pixel (oy * osy + ooy, ox * osx + oox) of the OH x OW output, channels [y_coff, y_coff + Cout) of rows
y_cstride wide; addend and mask are indexed exactly like the output.  A is the same contraction on absolute values,
A = sum |x| |w| + |bias|: the scale of the partial sums every accumulation-order error is proportional to.

Bounds (derived, not fitted; checked against an emulated correct implementation and against injected errors by
tests/test_conv_ref_cpu.py).  u = unit roundoff of the output's storage type under round-to-nearest: 2^-8 bf16, 2^-11
binary16, 2^-24 f32.  c = C_ACC = 1e-5 bounds the f32 accumulation of the partial sums, relative to A (the project's
figure for f32 partial sums, tests/test_norm_kernels_gpu.py; the float32 contraction of these shapes measures 6e-8).
    no addend:  |got - ref| <= u |ref| + c A                    one rounding of the f32 accumulator
    addend:     |got - ref| <= u |pre| + u |ref| + c A          16-bit outputs: the epilogue rounds the accumulator to the
                                                                storage type and rounds the sum again (add_bf16x2);
                                                                f32 outputs add in f32: one rounding, u |ref| + c A
    masked:     got == +-0 exactly
    sums (statistics, weight gradients; f32): |got - ref| <= c x (the float64 sum of the ABSOLUTE summands)
"""
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

C_ACC = 1e-5
U_BF16, U_F16, U_F32 = 2.0 ** -8, 2.0 ** -11, 2.0 ** -24


def geom(N, IH, IW, Cin, OH, OW, Cout, taps, sy=1, sx=None, OHs=None, OWs=None, osy=1, osx=None, ooy=0, oox=0, ups=0,
         xcs=0, xco=0, ycs=0, yco=0, relu=0, tile=0, ksplit=0, w_layout=0):
    """the fields of sba_conv_geom as a plain object (same names; ty / tx as lists)"""
    return NS(N=N, IH=IH, IW=IW, Cin=Cin, OH=OH, OW=OW, Cout=Cout, OHs=OH if OHs is None else OHs,
              OWs=OW if OWs is None else OWs, sy=sy, sx=sy if sx is None else sx, osy=osy, osx=osy if osx is None else osx,
              ooy=ooy, oox=oox, ups=ups, ntaps=len(taps), ty=[int(a) for a, _ in taps], tx=[int(b) for _, b in taps],
              x_cstride=xcs, x_coff=xco, y_cstride=ycs, y_coff=yco, relu=relu, tile=tile, ksplit=ksplit, first_write=0,
              w_layout=w_layout)


def window_taps(KH, KW, ph, pw):
    """taps of a KH x KW window with padding (ph, pw), in the [kh][kw] order of a packed weight"""
    return [(t // KW - ph, t % KW - pw) for t in range(KH * KW)]


def patches(x, g):
    """the gathered input of every tap: generator of [N, OHs, OWs, Cin] tensors (dtype of x); x: [N, IH, IW, xcs]"""
    xs = x[..., g.x_coff:g.x_coff + g.Cin]
    assert xs.shape == (g.N, g.IH, g.IW, g.Cin), (tuple(xs.shape), (g.N, g.IH, g.IW, g.Cin))
    if g.ups:
        xs = xs.repeat_interleave(2, 1).repeat_interleave(2, 2)
    LH, LW = xs.shape[1], xs.shape[2]
    ty, tx = g.ty[:g.ntaps], g.tx[:g.ntaps]
    ey, ex = (g.OHs - 1) * g.sy, (g.OWs - 1) * g.sx
    top, left = max(0, -min(ty)), max(0, -min(tx))
    bottom, right = max(0, ey + max(ty) - (LH - 1)), max(0, ex + max(tx) - (LW - 1))
    xp = F.pad(xs, (0, 0, left, right, top, bottom))                 # zero outside the logical input
    for t in range(g.ntaps):
        y0, x0 = top + ty[t], left + tx[t]
        yield xp[:, y0:y0 + ey + 1:g.sy, x0:x0 + ex + 1:g.sx, :]


def contract(x, w, g):
    """acc[N, OHs, OWs, Cout] in the dtype of x; w: [Cout][ntaps][Cin]"""
    assert tuple(w.shape) == (g.Cout, g.ntaps, g.Cin), (tuple(w.shape), (g.Cout, g.ntaps, g.Cin))
    acc = torch.zeros((g.N, g.OHs, g.OWs, g.Cout), dtype=x.dtype)
    for t, p in enumerate(patches(x, g)):
        acc += p.reshape(-1, g.Cin).matmul(w[:, t, :].t()).view(acc.shape)
    return acc


def window(t, g):
    """what a launch owns of a tensor laid out like its output ([N, OH, OW, ycs]): a [N, OHs, OWs, Cout] VIEW"""
    v = t[:, g.ooy::g.osy, g.oox::g.osx][:, :g.OHs, :g.OWs, g.y_coff:g.y_coff + g.Cout]
    assert v.shape == (g.N, g.OHs, g.OWs, g.Cout), tuple(v.shape)
    return v


def launch(x, w, g, bias=None, addend=None, mask=None):
    """float64 result of one launch.  x [N, IH, IW, xcs], w [Cout][ntaps][Cin], bias [Cout]; addend / mask laid out
    like the output tensor [N, OH, OW, ycs].  Returns acc, pre (before the addend), ref, A, zero (the elements the mask
    clears; all False without a mask), add (an addend was given) -- all [N, OHs, OWs, Cout]."""
    x, w = x.double(), w.double()
    acc, A = contract(x, w, g), contract(x.abs(), w.abs(), g)
    pre = acc.clone()
    if bias is not None:
        pre = pre + bias.double()
        A = A + bias.double().abs()
    if g.relu:
        pre = pre.clamp(min=0)
    ref = pre.clone()
    if addend is not None:
        ref = ref + window(addend.double(), g)
    zero = torch.zeros(ref.shape, dtype=torch.bool)
    if mask is not None:
        zero = ~(window(mask.double(), g) > 0)
        ref = torch.where(zero, torch.zeros_like(ref), ref)
    return NS(acc=acc, pre=pre, ref=ref, A=A, zero=zero, add=addend is not None)


def bound(r, u, two_roundings=None, c=C_ACC):
    """per-element bound of launch() result r for an output stored with unit roundoff u; two_roundings: the epilogue
    rounds before it adds the addend (default: every 16-bit output with an addend)"""
    if two_roundings is None:
        two_roundings = r.add and u > U_F32
    b = u * r.ref.abs() + c * r.A
    if two_roundings:
        b = b + u * r.pre.abs()
    return torch.where(r.zero, torch.zeros_like(b), b)


def worst(got, r, u, two_roundings=None, c=C_ACC):
    """largest |got - ref| / bound over the elements that are not masked (0.0 when all are); got: [N, OHs, OWs, Cout].
    Raises when an element is not finite or a masked element is not exactly +-0."""
    got = got.double()
    assert got.shape == r.ref.shape, (tuple(got.shape), tuple(r.ref.shape))
    assert bool(torch.isfinite(got).all()), 'non-finite or unwritten values inside the window'
    assert bool((got[r.zero] == 0).all()), 'a masked element is not exactly zero'
    keep = ~r.zero
    if not bool(keep.any()):
        return 0.0
    b = bound(r, u, two_roundings, c)[keep]
    err = (got - r.ref).abs()[keep]
    return float((err / b.clamp(min=1e-300)).max())


def stats(r):
    """per-channel statistics of the accumulators (before bias / ReLU / addend): (sum, sumsq) and the sums of the
    absolute summands (sum |acc|, sum acc^2) that bound their f32 summation error"""
    a = r.acc.reshape(-1, r.acc.shape[-1])
    return NS(sum=a.sum(0), sumsq=(a * a).sum(0), sum_abs=a.abs().sum(0), sumsq_abs=(a * a).sum(0))


def wgrad(x, dy, g):
    """dw[co][t][ci] = sum_pixel dy[pixel][co] * x[gather(pixel, t)][ci] in float64, and the same on absolute values;
    x [N, IH, IW, Cin], dy [N, OHs, OWs, Cout] (dense: sba_conv_wgrad refuses slices)"""
    x, dy = x.double(), dy.double()
    d, da = dy.reshape(-1, g.Cout).t(), dy.abs().reshape(-1, g.Cout).t()
    dw = torch.stack([d.matmul(p.reshape(-1, g.Cin)) for p in patches(x, g)], 1)
    A = torch.stack([da.matmul(p.reshape(-1, g.Cin)) for p in patches(x.abs(), g)], 1)
    return dw, A
