"""Float64 reference of the DAMSM loss family (miscc/losses.py:20-132 with func_attention, GlobalAttention.py:31-69) and
of its derivative, as the 13 entry points of csrc/damsm.hip and csrc/damsm_mfma.hip define the operation -- written from
the formulas, not from the kernels, on the CPU only.  tests/test_damsm_ref_cpu.py ties the forward to
oracle.sbagan_oracle.words_loss / sent_loss and the hand-written backward to float64 autograd;
tests/test_damsm_kernels_gpu.py judges the kernels by them.

Per (image j, caption i) pair, T = clamp(cap_lens[i], 1, L), every tensor below indexed [j][i][t][.]:

    S[t][r]    = sum_c f_j[c][r] q_i[c][t]
    a1[t][r]   = softmax over t < T of S[.][r]                (attn1)
    A[t][r]    = softmax over r of gamma1 a1[t][.]            (attn)
    w[t][c]    = sum_r f_j[c][r] A[t][r]                      (wctx)
    cos[t]     = <q_t, w_t> / max(|q_t| |w_t|, 1e-8)
    sim[j][i]  = log sum_{t<T} exp(gamma2 cos[t])

    dcos[t]    = dsim gamma2 exp(gamma2 cos[t]) / exp(sim)
    dw[t][c]   = ka q - kb w,  direct[t][c] = ka w - kc q     ka = dcos / max(den, 1e-8); kb = dcos cos / |w|^2 and
                                                              kc = dcos cos / |q|^2, both 0 where the clamp is active
    dA[t][r]   = sum_c dw[t][c] f[c][r];  dot[t] = <A[t], dA[t]>;  dz = A (dA - dot);  da1 = gamma1 dz
    dS[t][r]   = a1 (da1 - sum_t a1 da1)
    dfeat[j]   = sum_{i,t} (dw (x) A + q (x) dS)              dwords[i] = sum_j (direct + f . dS)

Words t >= T take no part: a1, A, w, dw, dS are 0 there in the results (the kernels leave attn / attn1 / wctx unwritten).
The sentence scores are gamma3 cos(cnn_j, rnn_i) with the clamp eps; ce_pair is the two cross entropies over a B x B
matrix (rows / columns, labels arange(B), masked entries -inf) with their gradients d0 / d1 w.r.t. the UNSCALED scores;
ce_direct is lam (loss0 + loss1) with dscore = lam (d0 + d1); combine2 is ga a + gb b.

Every argument is converted to float64 and every result is float64.  Every summed output comes with the sum of its
ABSOLUTE summands (`*_abs`), and every output behind a softmax with `*_cond`: the absolute summands together with the
first-order effect of a relative error c in every product in front of them, per unit of c (the convention of
tests/attn_ref.py).  A cancelling sum cannot normalise its own error, and dS = a1 (da1 - <a1, da1>) is one.  The chain:
|dS| <= c S_abs;  |d a1| <= c a1 sg1, sg1 = S_abs + <a1, S_abs>;  z = gamma1 a1: zg = z (1 + sg1);  |d A| <= c A ag,
ag = zg + <A, zg>;  w: sum |f| A (1 + ag);  cos: the error of w through the quotient, plus its own sums;  dcos through
the softmax of gamma2 cos;  ka / kb / kc, dw, direct by the product rule;  dA, dot, dz, da1, dS likewise
(words_backward spells every line out).

The second half holds what the CPU test and the GPU test share: the bounds as functions that return error / bound, an
emulation of each kernel family's STATED arithmetic in float32 torch (with the mutations the CPU test must see fail),
the deterministic inputs and the case lists.

Inputs (oracle.fill by tag).  Features and words are unit x sqrt(1.5) / nef^(1/4): the scores S have standard
deviation SCORE_STD = 1.5 whatever nef is, so the softmax over the words is neither flat nor one-hot, and gamma1 a1
spreads over [0, gamma1], so the softmax over the regions is not flat either.  Over the word cases below the largest
attn1 entry (captions of more than one word) is 0.989 (0.9994 in the two-word captions of LDS_CASES) and the flattest softmax over the words has a maximum of 0.085;
the largest attn entry is 0.61 at R = 17 and 0.17 at R = 289, against 1 / R = 0.06 and 0.0035 for a flat one
(test_damsm_ref_cpu.test_inputs_and_case_lists prints and holds these).  The `peak` cases multiply the words by
PEAK = 27: scores of standard deviation 40, differences down to -238, exp(S - max) below the smallest normal float32
(e^-87.3) in more than 30 % of the entries and exactly 0 (below e^-104) in some -- this exercises the max-subtraction
of the first softmax.  The second softmax of the matrix-core forward has none by design: gamma1 a1 <= gamma1.

The matrix-core bound.  Every product of the bf16 arms is x y ~ xh yh + xl yh + xh yl with xh = bf16(x), xl = bf16(x -
xh): the split leaves 2^-17 |x| (two 8-bit significands; the sign of lo buys the 17th bit), the dropped xl yl is at most
2^-18 |x y|, sums are float32.  So the unit is 2^-17 x the conditioned sum, and the multiple is MEASURED, not chosen: over
every matrix-core case of this file the emulation of that arithmetic (bf16 hi + lo operands, three products per term,
float32 sums, attention and the pass-1 -> pass-2 fragments rounded to hi + lo) needs at most 0.234 x 2^-17 x the
conditioned sum (attn1 of the peaked case: the scores' error through a near one-hot softmax; wctx 0.21, the gradients
below 0.03 -- their conditioned sums are worst-case over a long chain); MFMA_K = 1 is the smallest whole multiple that
leaves it at or below one half (tests/test_damsm_ref_cpu.py::test_mfma_multiple derives it and fails when it changes),
and hi-only features are then at 34 x the bound or more in attn1 at every case with lo parts.

Prefilled outputs.  Where a kernel ADDS to a buffer (dfeat / dwords of the f32 backward, dwords and dfeat with
accumulate = 1 of the matrix-core one, dcnn / drnn of sba_damsm_sent_bwd) the tests prefill it with values around 0.5,
compare stored - prefill, and allow one float32 ulp of the prefill on top of the bound of the sum.
"""
import functools
from collections import namedtuple
from types import SimpleNamespace as NS

import numpy as np
import torch

from oracle import fill

INF = float('inf')
NAN = float('nan')
CLAMP = 1e-8                    # the clamp of the word cosine (cosine_similarity's eps; the kernels hard-code it)
GAMMAS = ((4.0, 5.0, 10.0), (5.0, 5.0, 10.0))       # (gamma1, gamma2, gamma3) of the configs
TINY = 1e-300


def _d(t):
    return None if t is None else t.detach().double()


def lengths(lens, L):
    """T = clamp(cap_lens, 1, L)"""
    return torch.as_tensor(lens).long().clamp(1, L)


def live_words(lens, L):
    """[B][L] bool: word t of caption i takes part (t < T_i)"""
    return torch.arange(L)[None, :] < lengths(lens, L)[:, None]


# ------------------------------------------------------------------ the words loss in float64
def words_forward(feat, words, lens, g1, g2):
    """feat [B][nef][R], words [B][nef][L], lens [B] -> sim [j][i]; attn1, attn [j][i][t][r]; wctx [j][i][t][c]; cos"""
    f, q = _d(feat), _d(words)
    L = q.shape[2]
    live = live_words(lens, L)
    lv = live[None, :, :, None]
    S = torch.einsum('jcr,ict->jitr', f, q)
    S_abs = torch.einsum('jcr,ict->jitr', f.abs(), q.abs())
    a1 = torch.softmax(S.masked_fill(~lv, -INF), 2)
    sg1 = S_abs + (a1 * S_abs).sum(2, keepdim=True)
    z = g1 * a1
    A = torch.softmax(z, 3) * lv
    zg = z * (1 + sg1)
    ag = zg + (A * zg).sum(3, keepdim=True)
    w = torch.einsum('jcr,jitr->jitc', f, A)
    r = NS(live=live, S=S, S_abs=S_abs, attn1=a1, sg1=sg1, attn=A, ag=ag, wctx=w)
    r.attn1_cond, r.attn_cond = a1 * (1 + sg1), A * (1 + ag)
    r.wctx_abs = torch.einsum('jcr,jitr->jitc', f.abs(), A)
    r.wctx_cond = torch.einsum('jcr,jitr->jitc', f.abs(), A * (1 + ag))
    qt = q.permute(0, 2, 1)[None]                           # [1][i][t][c]
    r.w12, r.n1, r.n2 = (qt * w).sum(3), (qt ** 2).sum(3), (w ** 2).sum(3)
    r.den = r.n1.sqrt() * r.n2.sqrt()
    dc = r.den.clamp(min=CLAMP)
    r.cos = r.w12 / dc
    r.den_rel = 1 + (w.abs() * r.wctx_cond).sum(3) / r.n2.clamp(min=TINY)
    r.cos_gain = ((qt.abs() * r.wctx_cond).sum(3) + (qt * w).abs().sum(3)) / dc + r.cos.abs() * (1 + r.den_rel)
    e = torch.exp(g2 * r.cos) * live[None]
    r.sim = torch.log(e.sum(2))
    r.p = e / e.sum(2, keepdim=True)
    r.sim_cond = (r.p * g2 * r.cos_gain).sum(2) + r.sim.abs()
    return r


def words_backward(feat, words, lens, g1, g2, dsim, fwd=None, chained=False):
    """dsim [j][i] -> dfeat [B][nef][R], dwords [B][nef][L] with *_abs / *_cond, and every stage in between.
    chained = False: sim, attn, attn1 and wctx reach the backward EXACT (the float64 values rounded to float32: 2^-24 of
    each, far inside one product's share), so the conditioned sums hold the gains of the backward's own products only;
    chained = True: they are the forward kernel's, and carry the forward's gains (sg1, ag, wctx_cond) with them."""
    F0 = fwd or words_forward(feat, words, lens, g1, g2)
    f, q, g = _d(feat), _d(words), _d(dsim)
    qt = q.permute(0, 2, 1)[None]
    a1, A, w = F0.attn1, F0.attn, F0.wctx
    r = NS(fwd=F0)
    F = NS(**vars(F0))
    if not chained:
        F.sg1, F.ag, F.wctx_cond = torch.zeros_like(F0.sg1), torch.zeros_like(F0.ag), torch.zeros_like(F0.wctx_cond)
        F.den_rel = torch.ones_like(F0.den_rel)
        F.cos_gain = (qt * w).abs().sum(3) / F0.den.clamp(min=CLAMP) + 2 * F0.cos.abs()
    # d cos, through the softmax of gamma2 cos; exp(sim) is formed from the stored (float32) sim
    dcos = g[:, :, None] * g2 * F.p
    dcos_gain = dcos.abs() * (1 + g2 * F.cos_gain + (F.p * g2 * F.cos_gain).sum(2, keepdim=True) + F.sim.abs()[:, :, None])
    dc, clamped = F.den.clamp(min=CLAMP), F.den < CLAMP
    n1c, n2c = F.n1.clamp(min=TINY), F.n2.clamp(min=TINY)
    zero = torch.zeros_like(dcos)
    ka = dcos / dc
    kb = torch.where(clamped, zero, dcos * F.cos / n2c)
    kc = torch.where(clamped, zero, dcos * F.cos / n1c)
    kn = dcos_gain * F.cos.abs() + dcos.abs() * F.cos_gain
    ka_gain = dcos_gain / dc + ka.abs() * (1 + F.den_rel)
    kb_gain = torch.where(clamped, zero, kn / n2c + kb.abs() * (1 + 2 * F.den_rel))
    kc_gain = torch.where(clamped, zero, kn / n1c + 3 * kc.abs())
    u = lambda x: x[:, :, :, None]                                                   # noqa: E731
    # dcos -> dwctx and the direct d(words) term
    r.dcos, r.ka, r.kb, r.kc = dcos, ka, kb, kc
    r.dwctx = u(ka) * qt - u(kb) * w
    dw_gain = u(ka_gain) * qt.abs() + u(kb_gain) * w.abs() + u(kb.abs()) * F.wctx_cond + (u(ka) * qt).abs() + (u(kb) * w).abs()
    r.direct = u(ka) * w - u(kc) * qt
    direct_gain = u(ka_gain) * w.abs() + u(ka.abs()) * F.wctx_cond + u(kc_gain) * qt.abs() + (u(ka) * w).abs() + (u(kc) * qt).abs()
    # dA and <A, dA>
    r.dA = torch.einsum('jitc,jcr->jitr', r.dwctx, f)
    dA_abs = torch.einsum('jitc,jcr->jitr', r.dwctx.abs(), f.abs())
    dA_gain = torch.einsum('jitc,jcr->jitr', dw_gain, f.abs()) + dA_abs
    r.dot = (A * r.dA).sum(3, keepdim=True)
    dot_gain = (A * (F.ag * r.dA.abs() + dA_gain)).sum(3, keepdim=True)
    # the two softmax backward passes
    r.dz = A * (r.dA - r.dot)
    dz_gain = r.dz.abs() + A * (F.ag * (r.dA - r.dot).abs() + dA_gain + dot_gain)
    r.da1 = g1 * r.dz
    da1_gain = g1 * dz_gain + r.da1.abs()
    r.dot1 = (a1 * r.da1).sum(2, keepdim=True)
    dot1_gain = (a1 * (F.sg1 * r.da1.abs() + da1_gain)).sum(2, keepdim=True)
    r.dS = a1 * (r.da1 - r.dot1)
    r.dS_gain = r.dS.abs() + a1 * (F.sg1 * (r.da1 - r.dot1).abs() + da1_gain + dot1_gain)
    # d(features) and d(words)
    r.dfeat = torch.einsum('jitc,jitr->jcr', r.dwctx, A) + torch.einsum('ict,jitr->jcr', q, r.dS)
    r.dfeat_abs = torch.einsum('jitc,jitr->jcr', r.dwctx.abs(), A) + torch.einsum('ict,jitr->jcr', q.abs(), r.dS.abs())
    r.dfeat_cond = (torch.einsum('jitc,jitr->jcr', dw_gain + r.dwctx.abs(), A)
                    + torch.einsum('jitc,jitr->jcr', r.dwctx.abs(), A * F.ag)
                    + torch.einsum('ict,jitr->jcr', q.abs(), r.dS_gain + r.dS.abs()))
    r.dwords = r.direct.sum(0).permute(0, 2, 1) + torch.einsum('jcr,jitr->ict', f, r.dS)
    r.dwords_abs = r.direct.abs().sum(0).permute(0, 2, 1) + torch.einsum('jcr,jitr->ict', f.abs(), r.dS.abs())
    r.dwords_cond = ((direct_gain + r.direct.abs()).sum(0).permute(0, 2, 1)
                     + torch.einsum('jcr,jitr->ict', f.abs(), r.dS_gain + r.dS.abs()))
    return r


# ------------------------------------------------------------------ sentence scores, cross entropies, combine2
def sent_forward(cnn, rnn, g3, eps):
    """s[j][i] = gamma3 <cnn_j, rnn_i> / max(|cnn_j| |rnn_i|, eps); s_cond: sum of the absolute products, and the norms"""
    a, b = _d(cnn), _d(rnn)
    n0, n1 = (a ** 2).sum(1)[:, None], (b ** 2).sum(1)[None, :]
    den = n0.sqrt() * n1.sqrt()
    dc = den.clamp(min=eps)
    w12 = a @ b.t()
    s = g3 * w12 / dc
    return NS(s=s, w12=w12, n0=n0, n1=n1, den=den, s_cond=g3 * (a.abs() @ b.abs().t()) / dc + 3 * s.abs())


def sent_backward(cnn, rnn, ds, g3, eps, ds_gain=None):
    """ds [j][i] = d loss / d s -> dcnn [B][nef], drnn [B][nef] with *_abs (and *_cond where ds carries an error ds_gain)"""
    a, b, ds = _d(cnn), _d(rnn), _d(ds)
    F = sent_forward(a, b, 1.0, eps)
    g = ds * g3
    clamped = F.den < eps
    zero = torch.zeros_like(g)
    k0 = g / F.den.clamp(min=eps)
    cosv = F.w12 / F.den.clamp(min=TINY)
    ka = torch.where(clamped, zero, g * cosv / F.n0.clamp(min=TINY))
    kb = torch.where(clamped, zero, g * cosv / F.n1.clamp(min=TINY))
    r = NS(k0=k0, ka=ka, kb=kb)
    r.dcnn = k0 @ b - ka.sum(1, keepdim=True) * a
    r.drnn = k0.t() @ a - kb.sum(0)[:, None] * b
    r.dcnn_abs = k0.abs() @ b.abs() + ka.abs().sum(1, keepdim=True) * a.abs()
    r.drnn_abs = k0.abs().t() @ a.abs() + kb.abs().sum(0)[:, None] * b.abs()
    if ds_gain is not None:
        rel = _d(ds_gain) / ds.abs().clamp(min=TINY)        # the relative error of every ds, per unit of c
        r.dcnn_cond = (k0.abs() * (3 + rel)) @ b.abs() + (ka.abs() * (4 + rel)).sum(1, keepdim=True) * a.abs()
    return r


def ce_pair(score, mask, scale, s_cond=None):
    """-> loss0 (rows), loss1 (columns), d0, d1 = d loss / d score (unscaled); d_gain: the first-order error of d0 + d1
    per unit of relative error in the scaled scores' products (s_cond; default |s|)"""
    x = _d(score) * scale
    B = x.shape[0]
    if mask is not None:
        x = x.masked_fill(mask.bool(), -INF)
    eye = torch.eye(B, dtype=torch.float64)
    lse0, lse1 = torch.logsumexp(x, 1), torch.logsumexp(x, 0)
    diag = torch.diagonal(x)
    p0, p1 = torch.exp(x - lse0[:, None]), torch.exp(x - lse1[None, :])
    r = NS(loss0=(lse0 - diag).mean(), loss1=(lse1 - diag).mean(), p0=p0, p1=p1)
    r.d0, r.d1 = (p0 - eye) / B * scale, (p1 - eye) / B * scale
    sa = (x.abs() if s_cond is None else _d(s_cond) * scale).masked_fill(torch.isinf(x), 0.0)
    r.d_gain = (p0 * (sa + (p0 * sa).sum(1, keepdim=True)) + p1 * (sa + (p1 * sa).sum(0, keepdim=True))) / B * scale \
        + r.d0.abs() + r.d1.abs()
    return r


def ce_direct(score, mask, scale, lam, s_cond=None):
    c = ce_pair(score, mask, scale, s_cond)
    return NS(loss=lam * (c.loss0 + c.loss1), dscore=lam * (c.d0 + c.d1), dscore_gain=lam * c.d_gain, pair=c)


def combine2(a, ga, b, gb):
    return float(ga) * _d(a) + float(gb) * _d(b)


def sent_direct(cnn, rnn, mask, g3, eps, lam):
    """the whole sentence loss: lam (loss0 + loss1) over the scores and its gradient w.r.t. cnn"""
    F = sent_forward(cnn, rnn, g3, eps)
    c = ce_direct(F.s, mask, 1.0, lam, F.s_cond)
    b = sent_backward(cnn, rnn, c.dscore, g3, eps, c.dscore_gain)
    return NS(loss=c.loss, ds=c.dscore, dcnn=b.dcnn, dcnn_abs=b.dcnn_abs, dcnn_cond=b.dcnn_cond, s=F.s)


# ====================================================================================================================
# Bounds.  Each function returns the worst error / bound over the elements (inf when an element is not finite); the
# CPU test states how far inside the emulations are and that the mutations are outside, the GPU test asserts <= 1.
# RTOL / ATOL / C_SUM are the project's (tests/test_norm_kernels_gpu.py: elem_close, sums_close).
# ====================================================================================================================
RTOL, ATOL = 2e-4, 2e-5         # elementwise float32 values
C_SUM = 1e-5                    # float32 sums: |error| <= C_SUM x the float64 sum of the absolute summands
U_MFMA = 2.0 ** -17             # the unit of the matrix-core bound (see the docstring)
MFMA_K = 1.0                    # its multiple; derived by tests/test_damsm_ref_cpu.py::test_mfma_multiple
ULP32 = 2.0 ** -23


def _flat(*ts):
    out = [t.detach().double().cpu().flatten() for t in ts]
    assert all(t.shape == out[0].shape for t in out), [t.shape for t in out]
    return out


def _worst(err, bound):
    if not bool(torch.isfinite(err).all()):
        return INF
    return float((err / bound.clamp(min=TINY)).max()) if err.numel() else 0.0


def elem_ratio(got, ref):
    got, ref = _flat(got, ref)
    return _worst((got - ref).abs(), ATOL + RTOL * ref.abs())


def sums_ratio(got, ref, ref_abs, pre=None):
    """C_SUM x the (conditioned) sum of absolute summands, plus one float32 ulp of the prefill the kernel adds to"""
    got, ref, ref_abs = _flat(got, ref, ref_abs)
    bound = C_SUM * ref_abs.clamp(min=1e-30)
    if pre is not None:
        bound = bound + ULP32 * _flat(pre)[0].abs()
    return _worst((got - ref).abs(), bound)


def mfma_ratio(got, ref, cond, pre=None, k=None):
    got, ref, cond = _flat(got, ref, cond)
    bound = (MFMA_K if k is None else k) * U_MFMA * cond.clamp(min=1e-30)
    if pre is not None:
        bound = bound + ULP32 * _flat(pre)[0].abs()
    return _worst((got - ref).abs(), bound)


def _unwritten(x, dead):
    """every element of a word t >= T still holds the NaN prefill"""
    return 0.0 if bool(torch.isnan(x[dead]).all()) else INF


def words_fwd_ratios(fam, out, ref, k=None):
    """out: sim [j][i], attn1 / attn [j][i][t][r], wctx [j][i][t][c] as the kernel left its NaN-prefilled buffers.
    f32: elementwise; mfma: MFMA_K x 2^-17 x the conditioned sums."""
    B = ref.sim.shape[0]
    lv = ref.live[None].expand(B, -1, -1)
    res = {}
    for name in ('attn1', 'attn', 'wctx'):
        x = getattr(out, name).detach().double().cpu()
        res[name + ' unwritten at t >= T'] = _unwritten(x, ~lv)
        if fam == 'f32':
            res[name] = elem_ratio(x[lv], getattr(ref, name)[lv])
        else:
            res[name] = mfma_ratio(x[lv], getattr(ref, name)[lv], getattr(ref, name + '_cond')[lv], k=k)
    res['sim'] = elem_ratio(out.sim, ref.sim) if fam == 'f32' else mfma_ratio(out.sim, ref.sim, ref.sim_cond, k=k)
    return res


def words_bwd_ratios(fam, dfeat_added, dwords_added, ref, pre_feat=None, pre_words=None, k=None):
    """dfeat_added / dwords_added = stored - prefill (dfeat with accumulate = 0: the stored value, pre_feat None)"""
    ratio = sums_ratio if fam == 'f32' else functools.partial(mfma_ratio, k=k)
    res = {'dfeat': ratio(dfeat_added, ref.dfeat, ref.dfeat_cond, pre_feat)}
    if dwords_added is not None:
        res['dwords'] = ratio(dwords_added, ref.dwords, ref.dwords_cond, pre_words)
        dead = ~ref.fwd.live[:, None, :].expand_as(ref.dwords)
        added = dwords_added.detach().double().cpu()
        if pre_words is not None:       # a word t >= T gets nothing added: at most the rounding of prefill + 0 - prefill
            res['dwords at t >= T'] = _worst(added[dead].abs(), ULP32 * pre_words.double().reshape(added.shape)[dead].abs())
    return res


def ce_ratios(out, ref):
    """out / ref: loss0, loss1, d0, d1 (sba_ce_pair) or loss, dscore (sba_ce_pair_direct): elementwise float32"""
    return {k: elem_ratio(torch.as_tensor(getattr(out, k)), torch.as_tensor(getattr(ref, k)))
            for k in ('loss0', 'loss1', 'd0', 'd1', 'loss', 'dscore') if hasattr(out, k)}


def sent_bwd_ratios(dcnn_added, drnn_added, ref, pre_cnn=None, pre_rnn=None):
    res = {}
    if dcnn_added is not None:
        res['dcnn'] = sums_ratio(dcnn_added, ref.dcnn, ref.dcnn_abs, pre_cnn)
    if drnn_added is not None:
        res['drnn'] = sums_ratio(drnn_added, ref.drnn, ref.drnn_abs, pre_rnn)
    return res


def sent_direct_ratios(loss, dcnn, ref):
    """the loss elementwise; dcnn (stored, or None) at C_SUM x its conditioned sum: ds carries the error of the scores
    through the two softmaxes"""
    res = {'loss': elem_ratio(torch.as_tensor(loss).reshape(1), ref.loss.reshape(1))}
    if dcnn is not None:
        res['dcnn'] = sums_ratio(dcnn, ref.dcnn, ref.dcnn_cond)
    return res


def agree_ratio(x, y, bx, by):
    """two arms against each other: |x - y| <= the sum of their two bounds"""
    x, y, bx, by = _flat(x, y, bx, by)
    return _worst((x - y).abs(), bx + by)


# ====================================================================================================================
# Emulations of the kernels' stated arithmetic (the comments of csrc/damsm.hip and csrc/damsm_mfma.hip), float32 torch.
#   'f32'   float32 products and sums throughout
#   'mfma'  features, words, the attention, dwctx and dS enter the matrix cores as bf16 hi + lo pairs, three products
#           per term (the lo x lo one left out), float32 sums; softmaxes, cosine, log-sum-exp in float32 on the float32
#           words; the second softmax without max-subtraction
# `mut`: a set of mutations -- what tests/test_damsm_ref_cpu.py must see fall outside a bound.
# ====================================================================================================================
def _bf(x):
    return x.to(torch.bfloat16).float()


def _hi_lo(x):
    hi = _bf(x)
    return hi, _bf(x - hi)


def _mm(fam, eq, x, y, xlo=True, ylo=True):
    if fam == 'f32':
        return torch.einsum(eq, x, y)
    (xh, xl), (yh, yl) = _hi_lo(x), _hi_lo(y)
    out = torch.einsum(eq, xh, yh)
    if xlo:
        out = out + torch.einsum(eq, xl, yh)
    if ylo:
        out = out + torch.einsum(eq, xh, yl)
    return out


def _mut_inputs(feat, words, lens, mut):
    f, q = feat.detach().float().clone(), words.detach().float().clone()
    L = q.shape[2]
    T = lengths(lens, L)
    if 'T+1' in mut:
        T = (T + 1).clamp(max=L)
    if 'T-1' in mut:
        T = (T - 1).clamp(min=1)
    if 'ctile' in mut:                                      # the last 32-channel tile contributes nothing
        f[:, -32:], q[:, -32:] = 0, 0
    return f, q, T


def emulate_words_fwd(fam, feat, words, lens, g1, g2, mut=()):
    """-> sim, attn1, attn, wctx in float32, NaN (the prefill) at t >= T"""
    f, q, T = _mut_inputs(feat, words, lens, mut)
    if 'region' in mut:                                     # the last region takes no part
        o = emulate_words_fwd(fam, f[:, :, :-1], q, T, g1, g2, set(mut) - {'region', 'T+1', 'T-1', 'ctile'})
        pad = lambda x: torch.cat([x, torch.zeros_like(x[..., :1])], -1)            # noqa: E731
        return NS(sim=o.sim, attn1=pad(o.attn1), attn=pad(o.attn), wctx=o.wctx)
    L = q.shape[2]
    live = torch.arange(L)[None, :] < T[:, None]
    lv = live[None, :, :, None]
    flo = 'hi' not in mut
    if 'gamma1' in mut:
        g1 = 1.0
    S = _mm(fam, 'ict,jcr->jitr', q, f, True, flo)
    if 'axis' in mut:                                       # the softmaxes over each other's axis
        a1 = torch.softmax(S, 3) * lv
        A = torch.softmax((g1 * a1).masked_fill(~lv, -INF), 2)
    else:
        a1 = torch.softmax(S.masked_fill(~lv, -INF), 2)
        if fam == 'f32':
            A = torch.softmax(g1 * a1, 3) * lv
        else:
            e2 = torch.exp(g1 * a1)
            A = e2 / e2.sum(3, keepdim=True) * lv
    w = _mm(fam, 'jcr,jitr->jitc', f, A, flo, True)
    qt = q.permute(0, 2, 1)[None]
    w12, n1, n2 = (qt * w).sum(3), (qt * qt).sum(3), (w * w).sum(3)
    cos = w12 / (n1.sqrt() * n2.sqrt()).clamp(min=CLAMP)
    sim = torch.log((torch.exp(g2 * cos) * live[None]).sum(2))
    nan = torch.full((), NAN)
    o = NS(sim=sim, attn1=torch.where(lv, a1, nan), attn=torch.where(lv, A, nan), wctx=torch.where(lv, w, nan))
    if 'pair' in mut:                                       # results stored at [i][j]
        o = NS(sim=o.sim.t().contiguous(), attn1=o.attn1.transpose(0, 1), attn=o.attn.transpose(0, 1), wctx=o.wctx.transpose(0, 1))
    return o


def emulate_words_bwd(fam, feat, words, lens, g1, g2, dsim, saved, pre_feat, accumulate, pre_words, mut=()):
    """saved: sim / attn / attn1 / wctx as handed to the kernel (float32, NaN at t >= T).  pre_feat / pre_words: the
    float32 contents of dfeat / dwords before the call (pre_words None: dwords = NULL).  The f32 arm always adds to dfeat;
    the matrix-core arm adds with accumulate = 1 and stores with 0.  -> the stored dfeat, dwords"""
    f, q, T = _mut_inputs(feat, words, lens, mut)
    L = q.shape[2]
    live = torch.arange(L)[None, :] < T[:, None]
    lv = live[None, :, :, None]
    flo = 'hi' not in mut
    if 'gamma1' in mut:
        g1 = 1.0
    zero = torch.zeros(())
    g, sim = dsim.float(), saved.sim.float()
    A, a1, w = (torch.where(lv, x.float(), zero) for x in (saved.attn, saved.attn1, saved.wctx))
    if 'pair' in mut:
        g, sim = g.t(), sim.t()
    if 'region' in mut:
        A, a1 = A.clone(), a1.clone()
        A[..., -1], a1[..., -1] = 0, 0
    qt = q.permute(0, 2, 1)[None]
    w12, n1, n2 = (qt * w).sum(3), (qt * qt).sum(3), (w * w).sum(3)
    den = n1.sqrt() * n2.sqrt()
    clamped = den < CLAMP
    cos = w12 / den.clamp(min=CLAMP)
    dcos = g[:, :, None] * g2 * torch.exp(g2 * cos) / torch.exp(sim)[:, :, None] * live[None]
    ka = dcos / den.clamp(min=CLAMP)
    kb, kc = dcos * cos / n2, dcos * cos / n1
    if 'clampflag' not in mut:
        kb, kc = torch.where(clamped, zero, kb), torch.where(clamped, zero, kc)
    u = lambda x: x[:, :, :, None]                                                   # noqa: E731
    dw = (u(ka) * qt - u(kb) * w) * lv
    direct = (u(ka) * w - u(kc) * qt) * lv
    dA = _mm(fam, 'jitc,jcr->jitr', dw, f, True, flo)
    if 'axis' in mut:
        dz = A * (dA - (A * dA).sum(2, keepdim=True))
        da1 = g1 * dz
        dS = a1 * (da1 - (a1 * da1).sum(3, keepdim=True))
    else:
        dz = A * (dA - (A * dA).sum(3, keepdim=True))
        da1 = g1 * dz
        dS = a1 * (da1 - (a1 * da1).sum(2, keepdim=True))
    wl = live if 'w16' not in mut else live & (torch.arange(L)[None, :] < 16)       # the words d(features) sums over
    wv = wl[None, :, :, None]
    dfeat = _mm(fam, 'jitc,jitr->jcr', dw * wv, A) + _mm(fam, 'ict,jitr->jcr', q, dS * wv)
    if fam == 'f32':
        add = 'acc' not in mut
    else:
        add = bool(accumulate) != ('acc' in mut)
    dfeat = pre_feat.float().reshape(dfeat.shape) + dfeat if add else dfeat
    dwords = None
    if pre_words is not None:
        dwords = pre_words.float().reshape(q.shape) + direct.sum(0).permute(0, 2, 1) + _mm(fam, 'jcr,jitr->ict', f, dS, flo, True)
    return NS(dfeat=dfeat, dwords=dwords)


def emulate_sent_fwd(cnn, rnn, g3, eps, mut=()):
    a, b = cnn.float(), rnn.float()
    n0, n1 = (a * a).sum(1)[:, None], (b * b).sum(1)[None, :]
    s = (a @ b.t()) / (n0.sqrt() * n1.sqrt()).clamp(min=eps) * g3
    return s.t().contiguous() if 'pair' in mut else s


def emulate_sent_bwd(cnn, rnn, ds, g3, eps, pre_cnn, pre_rnn, mut=()):
    """-> the stored dcnn, drnn (prefill + gradient; None where the buffer is NULL)"""
    a, b, g = cnn.float(), rnn.float(), ds.float() * g3
    if 'pair' in mut:
        g = g.t()
    n0, n1 = (a * a).sum(1)[:, None], (b * b).sum(1)[None, :]
    den = n0.sqrt() * n1.sqrt()
    w12 = a @ b.t()
    k0 = g / den.clamp(min=eps)
    ka, kb = g * (w12 / den) / n0, g * (w12 / den) / n1
    if 'clampflag' not in mut:
        ka, kb = torch.where(den < eps, torch.zeros(()), ka), torch.where(den < eps, torch.zeros(()), kb)
    dcnn = k0 @ b - ka.sum(1, keepdim=True) * a
    drnn = k0.t() @ a - kb.sum(0)[:, None] * b
    add = 'acc' not in mut
    return NS(dcnn=None if pre_cnn is None else (pre_cnn.float().reshape(a.shape) if add else 0) + dcnn,
              drnn=None if pre_rnn is None else (pre_rnn.float().reshape(b.shape) if add else 0) + drnn)


def emulate_ce_pair(score, mask, scale, mut=()):
    x = score.float() * scale
    B = x.shape[0]
    if mask is not None:
        m = mask.bool()
        x = x.masked_fill(m.t() if 'maskT' in mut else m, -INF)
    eye = torch.eye(B)
    lse0, lse1 = torch.logsumexp(x, 1), torch.logsumexp(x, 0)
    diag = torch.diagonal(x)
    d0 = (torch.exp(x - lse0[:, None]) - eye) / B * scale
    d1 = (torch.exp(x - lse1[None, :]) - eye) / B * scale
    l0, l1 = (lse0 - diag).sum() / B, (lse1 - diag).sum() / B
    if 'colrow' in mut:                                     # the column cross entropy replaced by the row one
        d1, l1 = d0, l0
    return NS(loss0=l0, loss1=l1, d0=d0, d1=d1)


def emulate_ce_direct(score, mask, scale, lam, mut=()):
    c = emulate_ce_pair(score, mask, scale, mut)
    return NS(loss=(c.loss0 + c.loss1) * lam, dscore=lam * c.d0 + lam * c.d1)


def emulate_sent_direct(cnn, rnn, mask, g3, eps, lam, mut=()):
    s = emulate_sent_fwd(cnn, rnn, g3, eps, mut)
    c = emulate_ce_direct(s, mask, 1.0, lam, mut)
    b = emulate_sent_bwd(cnn, rnn, c.dscore, g3, eps, torch.zeros_like(cnn), None, set(mut) - {'acc'})
    return NS(loss=c.loss, dcnn=b.dcnn)


# ====================================================================================================================
# Inputs
# ====================================================================================================================
TAG_F, TAG_Q, TAG_DSIM, TAG_DFEAT, TAG_DWORDS = 301, 302, 303, 304, 305
TAG_CNN, TAG_RNN, TAG_DS, TAG_DCNN, TAG_DRNN, TAG_SCORE, TAG_MASK = 311, 312, 313, 314, 315, 316, 317
SCORE_STD = 1.5
PEAK = 27.0
ZERO_WORD = (0, 2)              # (caption, word) of the all-zero word of the `zero` cases; inside that caption's length


def prefill(n, tag):
    """the non-zero float32 values a buffer holds before a kernel adds to it (test_norm_kernels_gpu.prefilled(n, tag))"""
    return 0.5 + 0.25 * fill.unit((n,), tag)


@functools.lru_cache(maxsize=64)
def words_inputs(c):
    """-> feat [B][nef][R], words [B][nef][L] float32, lens int64 [B] (as given: the kernels clamp), dsim [B][B]"""
    s = float(np.sqrt(SCORE_STD) / c.nef ** 0.25)
    feat = fill.unit((c.B, c.nef, c.R), TAG_F) * s
    words = fill.unit((c.B, c.nef, c.L), TAG_Q) * (s * (PEAK if c.peak else 1.0))
    if not c.flo:
        feat = _bf(feat)                                    # exactly bf16: no lo part
    if c.zero:
        words[ZERO_WORD[0], :, ZERO_WORD[1]] = 0
    assert len(c.lens) == c.B
    return NS(feat=feat, words=words, lens=torch.tensor(c.lens, dtype=torch.int64), dsim=fill.unit((c.B, c.B), TAG_DSIM))


def gammas(c):
    return GAMMAS[c.g]


@functools.lru_cache(maxsize=64)
def words_ref(c, chained=False):
    """the float64 forward and backward of a case, computed once and shared"""
    i, (g1, g2, _) = words_inputs(c), gammas(c)
    f = words_ref(c).fwd if chained else words_forward(i.feat, i.words, i.lens, g1, g2)
    return words_backward(i.feat, i.words, i.lens, g1, g2, i.dsim, f, chained)


def saved_for_backward(F):
    """sim / attn / attn1 / wctx of the float64 forward rounded to float32, NaN at t >= T: what the isolated backward
    tests hand to the kernel in place of its own forward's outputs"""
    B = F.sim.shape[0]
    lv = F.live[None, :, :, None].expand(B, -1, -1, 1)
    nan = torch.full((), NAN)
    return NS(sim=F.sim.float(), attn=torch.where(lv, F.attn.float(), nan), attn1=torch.where(lv, F.attn1.float(), nan),
              wctx=torch.where(lv, F.wctx.float(), nan))


def sent_inputs(B, nef, zero=None):
    """zero: 'cnn' / 'rnn' -- vector 1 (0 at B = 1) of that side is all zero (the clamp)"""
    cnn, rnn = fill.unit((B, nef), TAG_CNN), fill.unit((B, nef), TAG_RNN)
    if zero == 'cnn':
        cnn[min(1, B - 1)] = 0
    if zero == 'rnn':
        rnn[min(1, B - 1)] = 0
    return NS(cnn=cnn, rnn=rnn, ds=fill.unit((B, B), TAG_DS) / B)


def ce_mask(B, kind):
    """None; 'class': the same-class mask of repeated ids (symmetric, i // 3 -- ids in runs of three); 'all': every
    off-diagonal entry; 'asym': an arbitrary mask that differs from its transpose (the entry points take any uint8[B][B])"""
    if kind is None:
        return None
    if kind == 'class':
        ids = torch.arange(B) // 3
        m = ids[:, None] == ids[None, :]
    elif kind == 'all':
        m = torch.ones((B, B), dtype=torch.bool)
    else:
        m = fill.uniform((B, B), TAG_MASK, 0.0, 1.0) < 0.3
    m = m.clone()
    m[torch.arange(B), torch.arange(B)] = False
    return m


def ce_scores(B):
    """scores like sim: log-sum-exp values around 2, spread 1"""
    return 2.0 + fill.unit((B, B), TAG_SCORE)


# ====================================================================================================================
# Cases.  Shapes are (B, nef, R, L) with lens; each is the smallest that reaches what its comment names.
# g: index into GAMMAS; flo: features carry lo parts (0: exactly bf16); peak: scores x 27; zero: an all-zero word
# ====================================================================================================================
W = namedtuple('W', 'B nef R L lens g flo peak zero')


def _w(B, nef, R, L, lens, g=0, flo=1, peak=0, zero=0):
    return W(B, nef, R, L, tuple(lens), g, flo, peak, zero)


F32_CASES = [
    _w(1, 32, 1, 1, (1,)),                      # B = 1, one region, one word, one channel tile (four idle waves)
    _w(3, 96, 17, 20, (0, 20, 23)),             # LP = 20 at its edge; nine K-pairs (chunk of 8 + 1); tiles < waves; lens 0, L, L + 3
    _w(3, 192, 289, 21, (21, 1, 13)),           # LP = 32 at its edge; odd R; tiles (6) > waves (5); lens 1
    _w(2, 256, 320, 32, (32, 17)),              # R = NT and L = TMAX: the limits
    _w(3, 64, 33, 9, (9, 5, 7), g=1),           # gamma1 = 5
    _w(2, 64, 33, 18, (18, 11), peak=1),        # exp underflows in the first softmax
    _w(2, 32, 17, 5, (5, 4), zero=1),           # an all-zero word inside caption 0: the clamp
]
MFMA_CASES = [
    _w(1, 64, 1, 1, (1,)),                      # B = 1: bwd2's prefetch with one caption; one region tile, three idle waves
    _w(2, 64, 33, 16, (16, 1)),                 # two region tiles; T = 16: bwd2 skips the second k-step of both captions
    _w(3, 128, 160, 17, (17, 16, 1), flo=0),    # exactly-bf16 features; five region tiles; T = 17 | 16 | 1
    _w(3, 320, 289, 32, (32, 17, 35)),          # ten tiles of either kind: bwd2's last workgroup has two live waves; lens L + 3
    _w(2, 64, 384, 32, (0, 16)),                # twelve region tiles = 4 waves x MAX_RT; lens 0
    _w(3, 128, 289, 18, (18, 9, 12), g=1, flo=0),   # the training shape's R and L, gamma1 = 5, bf16 features
    _w(2, 64, 33, 18, (18, 11), peak=1),        # peaked scores
    _w(2, 64, 17, 5, (5, 4), zero=1),           # the clamp
]
BOTH_ARMS = [c for c in MFMA_CASES if c.R <= 320]           # shapes both families accept (nef % 64 == 0, R <= 320)
# (nef, R) around the LDS limit of the matrix-core arm, 128 (nef + RP) + 4096 <= 160 KB with RP = R rounded up to 32: each
# pair is the last shape that fits and the first that does not; (1024, 384) is the corner the other limits allow
LDS_SHAPES = [(960, 288), (960, 289), (896, 352), (896, 353), (1024, 224), (1024, 225), (1024, 384), (64, 384)]


def lds_fits(nef, Rn):
    return 128 * (nef + (Rn + 31) // 32 * 32) + 4096 <= 160 * 1024


def lds_case(nef, Rn):
    """one image, one caption of two words: what runs at a shape of LDS_SHAPES that fits"""
    return _w(1, nef, Rn, 2, (2,))


LDS_CASES = [lds_case(nef, Rn) for nef, Rn in LDS_SHAPES if lds_fits(nef, Rn)]
SENT_CASES = [(1, 1, None), (2, 63, None), (5, 64, 'cnn'), (5, 65, 'rnn'), (2, 256, None)]      # (B, nef, zero side)
# (B, mask kind, scale, lam)
CE_CASES = [(1, None, 10.0, 5.0), (2, 'all', 10.0, 1.0), (2, None, 1.0, 5.0), (17, 'class', 10.0, 5.0), (17, 'asym', 1.0, 1.0),
            (17, 'all', 1.0, 5.0), (96, 'class', 10.0, 5.0), (96, None, 1.0, 1.0)]
SENT_DIRECT_CASES = [(1, 64, None, None), (2, 65, 'all', None), (17, 63, 'class', 'rnn'), (17, 256, 'asym', None),
                     (96, 64, 'class', None)]               # (B, nef, mask kind, zero side); B = 96: LDS above 64 KB
COMBINE_NS = (1, 255, 256, 257)
SENT_EPS = 1e-8


def case_id(c):
    return 'B%d-nef%d-R%d-L%d-lens%s-g%d%s%s%s' % (c.B, c.nef, c.R, c.L, '.'.join(map(str, c.lens)), c.g,
                                                   '' if c.flo else '-bf16feat', '-peak' if c.peak else '', '-zero' if c.zero else '')
