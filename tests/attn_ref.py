"""Float64 reference of the generator's word-level attention (GlobalAttentionGeneral.forward, GlobalAttention.py:82-121)
and of its derivative, as the three entry points of csrc/attention.hip define the operation -- written from the
formulas, not from the kernels, on the CPU only.  tests/test_attn_ref_cpu.py ties the forward to
oracle.sbagan_oracle.word_attention and the backward to float64 autograd; tests/test_attention_kernels_gpu.py judges the
kernels by them.

    s[b][q][l]   = sum_c h[b][q][c] src[b][c][l]        -inf where word l is masked for query (b, q)
    a            = softmax over l                         (att[b][l][q] = a[b][q][l])
    ctx[b][q][c] = sum_l a[b][q][l] src[b][c][l]
    dA = dctx . src     dS = a (dA - <a, dA>)     dh = dS . src^T
    dsrc[b][c][l] = sum_q (h[b][q][c] dS[b][q][l] + dctx[b][q][c] a[b][q][l])

mask_mode 0 masks row r = b * Q + q of the (B * Q) x L score matrix with mask[r % B] (the reference's
mask.repeat(Q, 1)); mask_mode 1 masks it with mask[b].  A query all of whose words are masked has a NaN softmax, in the
reference as here.

Every argument is converted to float64 and every result is float64.  The summed outputs come with the sum of the
ABSOLUTE summands of every element (`*_abs`) and with the root of the sum of their squares (`*_rss`): the normalisers of
the error bounds (a cancelling sum cannot provide its own).  ctx and dh, which lie behind the softmax, also come with
`*_cond`: the absolute summands together with the first-order effect of a relative error in every product in front of
them (the scores, dA, <a, dA>) -- see ulp_ratio.

The second half holds what the CPU test and the GPU test share: the bounds as functions that return error / bound,
an emulation of each kernel family's STATED arithmetic in float32 torch, the deterministic inputs and the case lists.
"""
import functools
from collections import namedtuple
from types import SimpleNamespace as NS

import numpy as np
import torch

from helpers import rel_l2
from oracle import fill

INF = float('inf')


def _d(t):
    return None if t is None else t.detach().double()


# ------------------------------------------------------------------ the operation in float64
def mask_rows(B, Q, mask_mode):
    """[B][Q]: the row of `mask` that query (b, q) is masked with"""
    if mask_mode == 0:
        return torch.arange(B * Q).view(B, Q) % B
    return torch.arange(B).view(B, 1).expand(B, Q)


def dead_words(B, Q, L, mask, mask_mode):
    """[B][Q][L] bool: word l takes no part in the softmax of query (b, q)"""
    if mask is None:
        return torch.zeros((B, Q, L), dtype=torch.bool)
    assert tuple(mask.shape) == (B, L), (mask.shape, B, L)
    return mask.bool()[mask_rows(B, Q, mask_mode)]


def forward(h, src, mask, mask_mode):
    """h [B][Q][idf] (already rounded to its storage type), src [B][idf][L], mask [B][L] or None ->
    ctx [B][Q][idf], att [B][L][Q]; also a = att^T [B][Q][L] and ctx_abs"""
    h, src = _d(h), _d(src)
    B, Q, _ = h.shape
    L = src.shape[2]
    s = torch.einsum('bqc,bcl->bql', h, src).masked_fill(dead_words(B, Q, L, mask, mask_mode), -INF)
    a = torch.softmax(s, 2)
    sg = _softmax_gain(a, torch.einsum('bqc,bcl->bql', h.abs(), src.abs()))
    return NS(ctx=torch.einsum('bql,bcl->bqc', a, src), att=a.transpose(1, 2), a=a, sg=sg,
              ctx_abs=torch.einsum('bql,bcl->bqc', a, src.abs()),
              ctx_cond=torch.einsum('bql,bcl->bqc', a * (1 + sg), src.abs()))


def _softmax_gain(a, s_abs):
    """first-order error of a probability per unit of relative error c in every product of the scores:
    da[l] = a[l] (ds[l] - sum_l' a[l'] ds[l']), |ds[l]| <= c s_abs[l]  =>  |da[l]| <= c a[l] (s_abs[l] + <a, s_abs>)"""
    return s_abs + (a * s_abs).sum(2, keepdim=True)


def backward(h, src, mask, mask_mode, dctx):
    """dctx [B][Q][idf] -> dh [B][Q][idf], dsrc [B][idf][L], with dh_abs / dh_rss / dsrc_abs / dsrc_rss; also a and dS"""
    f = forward(h, src, mask, mask_mode)
    h, src, dctx, a = _d(h), _d(src), _d(dctx), f.a
    dA = torch.einsum('bqc,bcl->bql', dctx, src)
    dot = (a * dA).sum(2, keepdim=True)
    dS = a * (dA - dot)
    r = NS(a=a, dS=dS)
    # |d dS[l]| / c, to first order: the product's own rounding, the error of a[l], of dA[l] and of <a, dA>
    dA_abs = torch.einsum('bqc,bcl->bql', dctx.abs(), src.abs())
    dot_gain = (a * (f.sg * dA.abs() + dA_abs)).sum(2, keepdim=True)
    dS_gain = dS.abs() + a * (f.sg * (dA - dot).abs() + dA_abs + dot_gain)
    r.dh_cond = torch.einsum('bql,bcl->bqc', dS_gain, src.abs())
    r.dh = torch.einsum('bql,bcl->bqc', dS, src)
    r.dh_abs = torch.einsum('bql,bcl->bqc', dS.abs(), src.abs())
    r.dh_rss = torch.einsum('bql,bcl->bqc', dS ** 2, src ** 2).sqrt()
    r.dsrc = torch.einsum('bqc,bql->bcl', h, dS) + torch.einsum('bqc,bql->bcl', dctx, a)
    r.dsrc_abs = torch.einsum('bqc,bql->bcl', h.abs(), dS.abs()) + torch.einsum('bqc,bql->bcl', dctx.abs(), a.abs())
    r.dsrc_rss = (torch.einsum('bqc,bql->bcl', h ** 2, dS ** 2) + torch.einsum('bqc,bql->bcl', dctx ** 2, a ** 2)).sqrt()
    return r


# ====================================================================================================================
# Bounds.  Each function returns the worst error / bound over the elements (inf when an element is not finite), so
# that the CPU test can state how far inside the emulations are and that the mutations are outside; the GPU test
# asserts <= 1.  RTOL / ATOL / C_SUM and the bf16 relative-L2 floor are the project's (tests/test_norm_kernels_gpu.py:
# elem_close, sums_close, low_close), ATT_ABS is test_kernels_gpu.test_word_attention_matrix_core_forward's.
# ====================================================================================================================
RTOL, ATOL = 2e-4, 2e-5         # elementwise float32 outputs
C_SUM = 1e-5                    # float32 sums: |error| <= C_SUM x the float64 sum of the absolute summands
ATT_ABS = 3e-5                  # probabilities of the bf16 matrix-core kernels (keys carried as hi + lo bf16 pairs)
U_BF16 = 2.0 ** -9              # the unit of the bf16 dsrc bound: half the unit roundoff of bf16 (8 significant bits: 2^-8)
# bf16 dsrc: the summands h dS and dctx a enter the contraction with dS and a rounded to bf16, each summand off by up
# to 2 U_BF16 of itself, independently: |error| <= DSRC16_K x U_BF16 x root-sum-of-squares + C_SUM x sum of absolutes.
# DSRC16_K is derived in tests/test_attn_ref_cpu.py (test_dsrc16_multiple): over the bf16 cases the emulations need at
# most 4.23 x U_BF16 x rss (1 x for one summand at the bottom of its binade is 2; the worst of 327,680 sums of 522
# summands is 4.2 of their standard deviation); 9 is the smallest whole multiple that leaves them a factor 2, and a
# single dropped query -- one of 16,389 at the largest shape -- still fails up to a multiple of 17.9.
DSRC16_K = 9.0


def _flat(*ts):
    out = [t.detach().double().cpu().flatten() for t in ts]
    assert all(t.shape == out[0].shape for t in out), [t.shape for t in out]
    return out


def _worst(err, bound):
    if not bool(torch.isfinite(err).all()):
        return INF
    return float((err / bound.clamp(min=1e-300)).max()) if err.numel() else 0.0


def elem_ratio(got, ref):
    got, ref = _flat(got, ref)
    return _worst((got - ref).abs(), ATOL + RTOL * ref.abs())


def sums_ratio(got, ref, ref_abs):
    got, ref, ref_abs = _flat(got, ref, ref_abs)
    return _worst((got - ref).abs(), C_SUM * ref_abs.clamp(min=1e-30))


def abs_ratio(got, ref, bound=ATT_ABS):
    got, ref = _flat(got, ref)
    return _worst((got - ref).abs(), torch.full_like(ref, bound))


def bf16_ulp(x):
    """distance between the two bf16 values around x (8 significant bits): 2^(floor(log2 |x|) - 7); 0 at 0"""
    x = x.detach().double()
    _, e = torch.frexp(x)                                   # |x| = m 2^e, m in [0.5, 1)
    return torch.where(x == 0, torch.zeros_like(x), torch.ldexp(torch.ones_like(x), e - 8))


def ulp_ratio(got, ref, ref_abs):
    """a bf16 output element by element: one bf16 ulp of the float64 value plus the dot-product bound, C_SUM x ref_abs.
    For ctx and dh, which lie BEHIND the softmax, ref_abs is `*_cond`: the summands' absolute values with the first-order
    effect of the same relative error in every product in front of them (scores, dA, <a, dA>) -- forward() / backward().
    The plain sum over |a src| or |dS src| knows nothing of the cancellation in dA - <a, dA> or of a sharp softmax: a
    float32 evaluation is up to 58 x outside it (dh at B = 512), and inside this one by a factor 4."""
    got, ref, ref_abs = _flat(got, ref, ref_abs)
    return _worst((got - ref).abs(), bf16_ulp(ref) + C_SUM * ref_abs)


def low_ratio(got, ref):
    """low_close: relative L2 against twice the one-rounding floor"""
    got, ref = _flat(got, ref)
    if not bool(torch.isfinite(got).all()):
        return INF
    floor = rel_l2(ref.to(torch.bfloat16).double(), ref)
    return rel_l2(got, ref) / max(2 * floor, 1e-300) if float(ref.abs().max()) > 0 else float(got.abs().max() > 0) * INF


def dsrc16_ratio(got, ref, ref_abs, ref_rss, k=DSRC16_K):
    got, ref, ref_abs, ref_rss = _flat(got, ref, ref_abs, ref_rss)
    return _worst((got - ref).abs(), k * U_BF16 * ref_rss + C_SUM * ref_abs)


def store_abs(Q, pre, ref_abs):
    """dsrc is ADDED to a float32 buffer that holds `pre`: every addition into the stored value rounds it, by up to 2^-24
    of |pre| + |sum so far|, whatever the size of the sum -- and a probability, hence a whole sum, can be 1e-6 of |pre|.
    The kernels add at most once per 32-query tile.  Allowed: one float32 ulp of the prefill, 2^-23 |pre|, per tile (a
    rounding takes half of it), which the 1e-5 of the sum's own summands cannot provide.  -> the sum of the absolute
    summands plus that, in units of C_SUM (0.012 |pre| per tile): what the bounds of dsrc are formed with.  The share of the
    summands in a rounding of the stored value is 2^-24 of them, far inside C_SUM."""
    return ref_abs + (-(-Q // 32)) * 2.0 ** -23 / C_SUM * pre.double().abs().reshape(ref_abs.shape)


def _nan_placement(got, ref):
    """NaN exactly where float64 has it (a query without a live word), and the mask of the elements to compare"""
    where = torch.isnan(ref)
    return (0.0 if torch.equal(torch.isnan(got), where) else INF), ~where


def fwd_ratios(family, ctx, att, ref):
    """every bound of the forward outputs of one case: {name: worst error / bound}.  ctx [B][Q][idf], att [B][L][Q] or
    None, ref = forward(...).  f32: elementwise; bf16: relative L2 against twice the one-rounding floor AND every element
    within one bf16 ulp + the dot-product bound; att of the matrix-core kernels: ATT_ABS, of the others elementwise."""
    ctx = ctx.detach().double().cpu()
    out = {}
    out['ctx NaN placement'], ok = _nan_placement(ctx, ref.ctx)
    g, r, ab = ctx[ok], ref.ctx[ok], ref.ctx_cond[ok]
    if family == 'f32':
        out['ctx elem'] = elem_ratio(g, r)
    else:
        out['ctx low'], out['ctx ulp'] = low_ratio(g, r), ulp_ratio(g, r, ab)
    if att is not None:
        att = att.detach().double().cpu()
        out['att NaN placement'], ok = _nan_placement(att, ref.att)
        out['att abs' if family == 'mfma16' else 'att elem'] = (abs_ratio if family == 'mfma16' else elem_ratio)(att[ok], ref.att[ok])
    return out


def bwd_ratios(family, dh, dsrc_added, ref, pre, prev=None):
    """dh [B][Q][idf] as stored (prev + the gradient where the kernel accumulates), dsrc_added = stored - pre with pre the
    prefill of dsrc, ref = backward(...).  f32: dh elementwise, dsrc at C_SUM x sum |summands|; bf16: dh as ctx, dsrc at
    DSRC16_K x U_BF16 x rss + C_SUM x sum |summands|."""
    want, want_cond = ref.dh, ref.dh_cond
    if prev is not None:
        want, want_cond = want + prev.double(), want_cond + prev.double().abs()
    dsrc_abs = store_abs(ref.a.shape[1], pre, ref.dsrc_abs)
    out = {}
    if family == 'f32':
        out['dh elem'] = elem_ratio(dh, want)
        out['dsrc sums'] = sums_ratio(dsrc_added, ref.dsrc, dsrc_abs)
    else:
        out['dh low'], out['dh ulp'] = low_ratio(dh, want), ulp_ratio(dh, want, want_cond)
        out['dsrc bf16'] = dsrc16_ratio(dsrc_added, ref.dsrc, dsrc_abs, ref.dsrc_rss)
    return out


# ====================================================================================================================
# Emulations of the kernels' stated arithmetic (the comments of csrc/attention.hip), in float32 torch on the CPU.
#   'f32'     the VALU kernels on float32 tensors: float32 accumulation throughout
#   'valu16'  the VALU kernels on bf16 tensors: the same in float32, outputs rounded to bf16 once; the backward puts
#             dS and a into its LDS tiles as bf16, so the dsrc contraction (alone) sees them rounded
#   'mfma16'  the bf16 matrix-core kernels: src and the probabilities (dS in the backward's dh) enter the matrix cores
#             as hi + lo bf16 pairs -- x = hi + lo + O(2^-17 x), the lo x lo product is left out -- float32
#             accumulation; dS and a rounded to bf16 for the dsrc contraction only
# ====================================================================================================================
FAMILY_T = {'f32': torch.float32, 'valu16': torch.bfloat16, 'mfma16': torch.bfloat16}


def _bf(x):
    return x.to(torch.bfloat16).float()


def _hi_lo(x):
    hi = _bf(x)
    return hi, _bf(x - hi)


def _probabilities(family, h, src, dead):
    if family == 'mfma16':
        hi, lo = _hi_lo(src)
        s = torch.einsum('bqc,bcl->bql', h, hi) + torch.einsum('bqc,bcl->bql', h, lo)
    else:
        s = torch.einsum('bqc,bcl->bql', h, src)
    return torch.softmax(s.masked_fill(dead, -INF), 2)


def _times_src(family, x, src):
    """sum_l x[b][q][l] src[b][c][l]"""
    if family != 'mfma16':
        return torch.einsum('bql,bcl->bqc', x, src)
    (xh, xl), (sh, sl) = _hi_lo(x), _hi_lo(src)
    return torch.einsum('bql,bcl->bqc', xh, sh) + torch.einsum('bql,bcl->bqc', xl, sh) + torch.einsum('bql,bcl->bqc', xh, sl)


def emulate_fwd(family, h, src, mask, mask_mode):
    """-> ctx in the storage type, att in float32"""
    h, src = h.float(), src.float()
    B, Q, _ = h.shape
    a = _probabilities(family, h, src, dead_words(B, Q, src.shape[2], mask, mask_mode))
    return NS(ctx=_times_src(family, a, src).to(FAMILY_T[family]), att=a.transpose(1, 2).contiguous())


def emulate_bwd(family, h, src, mask, mask_mode, dctx, prev, dsrc0):
    """prev: the dh the kernel adds to (accumulate = 1) or None; dsrc0: the float32 prefill dsrc is added to.
    -> dh in the storage type, dsrc the stored float32 tensor"""
    h, src, dctx = h.float(), src.float(), dctx.float()
    B, Q, _ = h.shape
    a = _probabilities(family, h, src, dead_words(B, Q, src.shape[2], mask, mask_mode))
    if family == 'mfma16':
        hi, lo = _hi_lo(src)
        dA = torch.einsum('bqc,bcl->bql', dctx, hi) + torch.einsum('bqc,bcl->bql', dctx, lo)
    else:
        dA = torch.einsum('bqc,bcl->bql', dctx, src)
    dS = a * (dA - (a * dA).sum(2, keepdim=True))
    dh = _times_src(family, dS, src)
    if prev is not None:
        dh = dh + prev.float()
    ys, ya = (dS, a) if family == 'f32' else (_bf(dS), _bf(a))
    dsrc = torch.einsum('bqc,bql->bcl', h, ys) + torch.einsum('bqc,bql->bcl', dctx, ya)
    return NS(dh=dh.to(FAMILY_T[family]), dsrc=dsrc0.float() + dsrc)


# ====================================================================================================================
# Inputs: oracle.fill by tag, h / dctx / prev rounded to the storage type, src in float32 with scores of standard
# deviation 2 (src = unit x 2 / sqrt(idf)), about 30 % of the words masked and word 0 never.
# ====================================================================================================================
TAG_H, TAG_SRC, TAG_MASK, TAG_DCTX, TAG_PREV, TAG_DSRC = 201, 202, 203, 204, 205, 206
SRC_SCORE_STD = 2.0
DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16}


def make_mask(B, L, full_row=None):
    m = fill.uniform((B, L), TAG_MASK, 0.0, 1.0) < 0.3
    m[:, 0] = False
    if full_row is not None:
        m[full_row] = True
    return m


@functools.lru_cache(maxsize=3)
def inputs(B, Q, idf, L, dt, full_row=None):
    """-> h, dctx, prev [B][Q][idf] in storage type dt; src [B][idf][L] float32; mask [B][L] bool (pass it or None)"""
    T = DTYPES[dt]
    return NS(h=fill.unit((B, Q, idf), TAG_H).to(T), src=fill.unit((B, idf, L), TAG_SRC) * float(SRC_SCORE_STD / np.sqrt(idf)),
              mask=make_mask(B, L, full_row), dctx=fill.unit((B, Q, idf), TAG_DCTX).to(T), prev=fill.unit((B, Q, idf), TAG_PREV).to(T))


def dsrc_prefill(n):
    """the non-zero float32 values dsrc holds before the kernels add to it (test_norm_kernels_gpu.prefilled(n, TAG_DSRC))"""
    return 0.5 + 0.25 * fill.unit((n,), TAG_DSRC)


def fp8_inputs(B, Q, idf, L, mask_mode, dead_row=None):
    """the exact-layout inputs of test_kernels_gpu.test_word_attention_fp8: h integers in [-2, 2], src multiples of 1/4 in
    [-1, 1] (e4m3 holds both times their power-of-two scales exactly), ONE live word per mask row -- (3 row) % L -- so that
    the probability is exactly 1 and ctx is the selected key column bit for bit.  dead_row: that mask row has no live word.
    -> h (bf16), src, mask, and word [B][Q]: the live word of every query (-1: none, the query is NaN)"""
    g = torch.Generator().manual_seed(1000 * idf + L)
    h = torch.randint(-2, 3, (B, Q, idf), generator=g).float().to(torch.bfloat16)
    src = torch.randint(-4, 5, (B, idf, L), generator=g).float() * 0.25
    live = (3 * torch.arange(B)) % L
    mask = torch.ones((B, L), dtype=torch.bool)
    mask[torch.arange(B), live] = False
    if dead_row is not None:
        mask[dead_row] = True
        live[dead_row] = -1
    return NS(h=h, src=src, mask=mask, word=live[mask_rows(B, Q, mask_mode)])


# ====================================================================================================================
# Cases.  Each is the smallest shape that reaches its arm of the host dispatch (launch_fwd, launch_fwd_mfma, launch_bwd).
# mask: 'm0' / 'm1' = a mask in mask_mode 0 / 1, 'n0' / 'n1' = mask = NULL in mask_mode 0 / 1.
# ====================================================================================================================
Fwd = namedtuple('Fwd', 'dt idf B Q L mask att sliced')     # att: the map is asked for; sliced: ocs = 2 idf, oco = idf
Bwd = namedtuple('Bwd', 'dt idf B Q L mask acc sliced')     # acc: accumulate; sliced: dcs = 2 idf, dco = idf

LS = (1, 3, 16, 17, 32)         # L < 4, the lane's own 16 words | the partner half-wave's, the shift edge of the dead bits
QS = (1, 31, 32, 33, 261)       # one query, one short of a 32-query tile, a tile, a tile + 1, 8 tiles + 5 (> 256)
B_SMALL = 5                     # odd, divides none of QS: r % B and b differ
MASKS = ('m0', 'm1', 'n0', 'm0', 'm1', 'n1')
FWD_ARMS = (('f32', 32), ('f32', 64), ('f32', 128), ('bf16', 32), ('bf16', 64), ('bf16', 128))
BWD_ARMS = (('f32', 32), ('f32', 64), ('bf16', 64), ('bf16', 32))


def _ragged(arms, make):
    """a pairwise-covering selection, five cases per arm k: L = LS[i] with Q = QS[(i + k) % 5], i < 5, so every arm meets
    every L and every Q; the mask kind, the att / accumulate flag and the channel slice cycle with other periods, so every
    arm meets both mask modes, a NULL mask, both values of the flag and both slices (test_attn_ref_cpu.test_case_lists)"""
    return [make(dt, idf, B_SMALL, QS[(i + k) % 5], LS[i], MASKS[(i + 2 * k) % 6], (i + k // 2) % 2, (i // 2 + k) % 2)
            for k, (dt, idf) in enumerate(arms) for i in range(5)]


FWD_SMALL = _ragged(FWD_ARMS, Fwd)
BWD_SMALL = _ragged(BWD_ARMS, Bwd)
# tiles per wave (launch_fwd_mfma, the matrix-core arm of launch_bwd): tiles = ceil(261 / 32) = 9;  512 x 9 = 4608 >= 4096:
# tpw = 2, two workgroups per image, the second with ONE live tile in one wave;  2048 x 9 = 18432 >= 16384: tpw = 4, one
# workgroup, the third wave breaks after one tile, the fourth does nothing.  B = 2048 in mask_mode 0: mask rows >= 1024 lie
# beyond the kernels' LDS table of dead-word bits.
TPW_L = 5
FWD_TPW = [Fwd('bf16', 32, 512, 261, TPW_L, 'm1', 1, 0), Fwd('bf16', 32, 2048, 261, TPW_L, 'm0', 1, 0)]
BWD_TPW = [Bwd('bf16', 32, 512, 261, TPW_L, 'm1', 0, 0), Bwd('bf16', 32, 2048, 261, TPW_L, 'm0', 1, 0)]
# chunks of word_attn_bwd_kernel (NT = 128 queries per chunk in float32, 256 in bf16): Q = 4101 -> chunks = 2, Q = 16389 ->
# chunks = 4; both leave 5 queries to a last workgroup whose later chunks are entirely dead
BWD_CHUNKS = [Bwd(dt, idf, B, Q, 7, mk, acc, 0)
              for (dt, idf) in BWD_ARMS[:3] for (B, Q, mk, acc) in ((1, 4101, 'm1', 0), (2, 16389, 'm0', 1))]
# deterministic mode (det_part + sba_det_fold): more than one workgroup per image in either backward kernel
BWD_DET = [Bwd('bf16', 32, B_SMALL, 261, 17, 'm0', 1, 1), Bwd('f32', 64, B_SMALL, 261, 17, 'm1', 0, 1),
           Bwd('bf16', 64, B_SMALL, 261, 3, 'm0', 1, 0)]
# a fully masked row (forward only): mask row 1 has no live word; Q = 33 spans two tiles
FULL_ROW = 1
FWD_FULL = [Fwd(dt, idf, B_SMALL, 33, 3, mk, 1, 0) for (dt, idf) in (('f32', 32), ('bf16', 32), ('bf16', 64), ('bf16', 128))
            for mk in ('m0', 'm1')]
# (idf, B, Q, L, mask_mode) of the exact FP8 layout cases: MT = 2 at a ragged Q, tpw = 2 at idf 64, tpw = 4 with B > 1024
FP8_EXACT = [(64, B_SMALL, 261, 9, 1), (64, B_SMALL, 33, 32, 0), (64, 512, 261, TPW_L, 1), (32, 2048, 261, TPW_L, 0)]
FP8_FULL = [(32, B_SMALL, 33, 3, 0), (64, B_SMALL, 33, 3, 1)]


def family_of(case):
    """which kernel family the host dispatch selects for a case (see the table of test_attention_kernels_gpu.py)"""
    if case.dt == 'f32':
        return 'f32'
    if isinstance(case, Fwd):
        return 'mfma16' if case.idf <= 64 else 'valu16'
    return 'mfma16' if case.idf == 32 else 'valu16'


def case_id(c):
    return '%s-idf%d-B%d-Q%d-L%d-%s-%s%d-sl%d' % (c.dt, c.idf, c.B, c.Q, c.L, c.mask, 'att' if isinstance(c, Fwd) else 'acc', c[6], c.sliced)


def case_inputs(c, full_row=None):
    """the inputs of a case and its (mask or None, mask_mode)"""
    i = inputs(c.B, c.Q, c.idf, c.L, c.dt, full_row)
    return i, (i.mask if c.mask[0] == 'm' else None), int(c.mask[1])
