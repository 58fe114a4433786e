"""tests/damsm_ref.py checked without a GPU, before a kernel of csrc/damsm.hip or csrc/damsm_mfma.hip is judged by it.

(1) At EVERY case of tests/test_damsm_kernels_gpu.py -- the clamped lengths, the masks, the all-zero word and the zero
    vectors included -- the float64 forward equals oracle.sbagan_oracle.words_loss / sent_loss (tied to the reference's
    golden vectors by tests/test_oracle_golden.py), and the backward written out stage by stage equals float64 autograd
    of the oracle's forward.  The conditioned sums hold the plain ones and bound the first-order effect of a relative
    error in every product of the scores and of dA.
(2) At every case an emulation of the kernel family's stated arithmetic (float32 torch; bf16 hi + lo operands with three
    products per term on the matrix-core arms) is inside every bound the GPU test applies, by a factor 2 -- so a failure
    on the GPU is the kernel's, not the bound's or the inputs' -- and every mutation below is OUTSIDE a bound at the case
    meant to catch it, so the bounds are not vacuous.  Each case prints its ratios.
(3) The multiple of the matrix-core bound is derived here from the emulation (test_mfma_multiple).

Mutations (each judged by the same functions as the GPU outputs):
    pair        (i, j) transposed in the pair index: results stored at / upstream gradient read from [i][j].  B = 3
    T+1 / T-1   the caption length off by one in either direction; a caption with 1 < T < L
    region      the last region takes no part
    ctile       the last 32-channel tile contributes nothing
    axis        the two softmaxes over each other's axis
    gamma1      gamma1 left out
    w16         words 16 .. 31 dropped from d(features); a caption with T > 16
    hi          the hi part only of the features (matrix-core arms; through the forward -- the gradient bounds, whose
                conditioned sums are worst-case, cannot tell a 2^-9 error of one factor)
    maskT       the mask transposed; an asymmetric mask (a same-class mask is symmetric and cannot tell)
    acc         `accumulate` ignored, either way; the f32 arms store where they should add
    clampflag   the cosine clamp's flag ignored: 0 / 0 at the all-zero word / vector
    colrow      the column cross entropy replaced by the row one
"""
import pytest
import torch
import torch.nn.functional as F

import damsm_ref as R
from oracle import fill
from oracle import sbagan_oracle as O

TOL = 1e-10
SPARE = 0.5                     # the emulations stay below SPARE x bound
WORD_CASES = list(dict.fromkeys(R.F32_CASES + R.MFMA_CASES + R.LDS_CASES))
FAM_CASES = [('f32', c) for c in R.F32_CASES] + [('mfma', c) for c in R.MFMA_CASES + R.LDS_CASES]
fam_id = lambda fc: fc if isinstance(fc, str) else R.case_id(fc)       # noqa: E731


def same(got, ref, name='', tol=TOL):
    got, ref = got.detach().double(), ref.detach().double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = float((got - ref).abs().max())
    assert err <= tol * max(1.0, float(ref.abs().max())), '%s: max err %.3e' % (name, err)


def show(name, ratios):
    print('%-60s %s' % (name, '  '.join('%s %.3g' % kv for kv in sorted(ratios.items()))))
    return ratios


def inside(name, ratios):
    for k, v in show(name, ratios).items():
        assert v <= SPARE, '%s: the emulation is at %.3f of the bound on %s' % (name, v, k)


def outside(name, ratios):
    assert max(show(name, ratios).values()) > 1.0, '%s: the mutation is inside every bound' % name


# ------------------------------------------------------------------ (1) the reference
def class_ids(B):
    return (torch.arange(B) // 3).numpy()


@pytest.mark.parametrize('c', WORD_CASES, ids=R.case_id)
def test_words_reference_is_the_oracle_and_autograd(c):
    i, (g1, g2, g3) = R.words_inputs(c), R.gammas(c)
    ref = R.words_ref(c)
    T = R.lengths(i.lens, c.L)
    labels = torch.arange(c.B)
    f, q = i.feat.double().requires_grad_(True), i.words.double().requires_grad_(True)
    sim = O.words_similarity(f.view(c.B, c.nef, c.R, 1), q, T, g1, g2)
    same(ref.fwd.sim, sim, 'sim')
    assert bool(torch.isfinite(ref.fwd.sim).all())
    gf, gq = torch.autograd.grad(sim, [f, q], i.dsim.double())
    same(ref.dfeat, gf, 'dfeat'); same(ref.dwords, gq, 'dwords')
    dead = ~ref.fwd.live[:, None, :].expand_as(ref.dwords)
    assert float(ref.dwords[dead].abs().max() if bool(dead.any()) else 0.0) == 0.0
    for ids in (None, class_ids(c.B)):
        l0, l1 = O.words_loss(i.feat.double().view(c.B, c.nef, c.R, 1), i.words.double(), labels, T, ids, c.B, g1, g2, g3)
        ce = R.ce_pair(ref.fwd.sim, O.class_mask(ids, c.B), g3)
        same(ce.loss0, l0, 'loss0'); same(ce.loss1, l1, 'loss1')
    # the stages against func_attention of one pair
    j, k = c.B - 1, 0
    wctx, att = O.func_attention(i.words.double()[k:k + 1, :, :int(T[k])], i.feat.double()[j:j + 1].view(1, c.nef, c.R, 1), g1)
    same(ref.fwd.wctx[j, k, :int(T[k])], wctx[0].t(), 'wctx'); same(ref.fwd.attn[j, k, :int(T[k])], att.view(int(T[k]), c.R), 'attn')
    for name in ('wctx', 'dfeat', 'dwords'):
        src = ref.fwd if name == 'wctx' else ref
        assert bool((getattr(src, name + '_cond') >= getattr(src, name + '_abs') * (1 - 1e-12)).all()), name
        assert bool((getattr(src, name + '_abs') >= getattr(src, name).abs() * (1 - 1e-9) - 1e-300).all()), name
    if c.zero:                                              # the clamp: cos = 0 at the zero word, everything finite
        zi, zt = R.ZERO_WORD
        assert float(ref.fwd.cos[:, zi, zt].abs().max()) == 0.0 and float(ref.fwd.den[:, zi, zt].max()) == 0.0
        assert float(ref.dwords[zi, :, zt].abs().max()) > 1e6        # w dcos / 1e-8: autograd of w12 / max(|q| |w|, 1e-8)


def test_conditioned_sums_bound_a_perturbation():
    """a relative error c = 1e-6 of one random sign in every product of S, of wctx and of dA moves every output by at most
    1.01 c x its conditioned sum (chained: the forward's error reaches the backward)"""
    c = R._w(2, 8, 5, 4, (4, 3))
    i, (g1, g2, _) = R.words_inputs(c), R.GAMMAS[0]
    f, q, g = i.feat.double(), i.words.double(), i.dsim.double()
    ref = R.words_backward(f, q, i.lens, g1, g2, g, chained=True)
    Fw = ref.fwd
    e = 1e-6
    sgn = lambda shape, tag: 1 + e * torch.sign(fill.unit(shape, tag).double())      # noqa: E731
    lv = Fw.live[None, :, :, None]
    S = (torch.einsum('jcr,ict->jitrc', f, q) * sgn((2, 2, 4, 5, 8), 331)).sum(4)
    a1 = torch.softmax(S.masked_fill(~lv, -R.INF), 2)
    A = torch.softmax(g1 * a1, 3) * lv
    w = (torch.einsum('jcr,jitr->jitcr', f, A) * sgn((2, 2, 4, 8, 5), 332)).sum(4)
    assert bool(((a1 - Fw.attn1).abs() <= 1.01 * e * Fw.attn1_cond).all())
    assert bool(((A - Fw.attn).abs() <= 1.01 * e * Fw.attn_cond).all())
    assert bool(((w - Fw.wctx).abs() <= 1.01 * e * Fw.wctx_cond).all())
    qt = q.permute(0, 2, 1)[None]
    n1, n2 = (qt ** 2).sum(3), (w ** 2).sum(3)
    den, n2 = (n1.sqrt() * n2.sqrt()).clamp(min=R.CLAMP), n2.clamp(min=R.TINY)      # (dead words: 0 / 0 otherwise)
    cos = (qt * w).sum(3) / den
    ex = torch.exp(g2 * cos) * Fw.live[None]
    sim = torch.log(ex.sum(2))
    assert bool(((sim - Fw.sim).abs() <= 1.01 * e * Fw.sim_cond).all())
    dcos = g[:, :, None] * g2 * ex / ex.sum(2, keepdim=True)
    u = lambda x: x[:, :, :, None]                                                   # noqa: E731
    dw = u(dcos / den) * qt - u(dcos * cos / n2) * w
    direct = u(dcos / den) * w - u(dcos * cos / n1) * qt
    dA = (torch.einsum('jitc,jcr->jitrc', dw, f) * sgn((2, 2, 4, 5, 8), 333)).sum(4)
    da1 = g1 * A * (dA - (A * dA).sum(3, keepdim=True))
    dS = a1 * (da1 - (a1 * da1).sum(2, keepdim=True))
    dfeat = torch.einsum('jitc,jitr->jcr', dw, A) + torch.einsum('ict,jitr->jcr', q, dS)
    dwords = direct.sum(0).permute(0, 2, 1) + torch.einsum('jcr,jitr->ict', f, dS)
    assert bool(((dS - ref.dS).abs() <= 1.01 * e * ref.dS_gain).all())
    assert bool(((dfeat - ref.dfeat).abs() <= 1.01 * e * ref.dfeat_cond).all())
    assert bool(((dwords - ref.dwords).abs() <= 1.01 * e * ref.dwords_cond).all())


@pytest.mark.parametrize('B,kind,scale,lam', R.CE_CASES, ids=lambda v: str(v))
def test_cross_entropies_are_torch(B, kind, scale, lam):
    score, mask = R.ce_scores(B).double().requires_grad_(True), R.ce_mask(B, kind)
    x = score * scale
    if mask is not None:
        x = x.masked_fill(mask, -R.INF)
    labels = torch.arange(B)
    l0, l1 = F.cross_entropy(x, labels), F.cross_entropy(x.t(), labels)
    ref = R.ce_direct(score, mask, scale, lam)
    same(ref.pair.loss0, l0, 'loss0'); same(ref.pair.loss1, l1, 'loss1')
    same(ref.pair.d0, torch.autograd.grad(l0, score, retain_graph=True)[0], 'd0')
    same(ref.pair.d1, torch.autograd.grad(l1, score, retain_graph=True)[0], 'd1')
    same(ref.dscore, torch.autograd.grad(lam * (l0 + l1), score)[0], 'dscore'); same(ref.loss, lam * (l0 + l1), 'loss')
    same(R.combine2(ref.pair.d0, lam, ref.pair.d1, 0.5), lam * ref.pair.d0 + 0.5 * ref.pair.d1, 'combine2')
    if kind == 'all' or B == 1:                             # every off-diagonal entry hidden: nothing to tell apart
        assert float(ref.loss) == 0.0 and float(ref.dscore.abs().max()) == 0.0
    if kind == 'asym':
        assert not torch.equal(mask, mask.t())
    if kind == 'class':
        assert torch.equal(mask, O.class_mask(class_ids(B), B)) and bool(mask.any())


@pytest.mark.parametrize('B,nef,kind,zero', R.SENT_DIRECT_CASES + [(b, n, None, z) for b, n, z in R.SENT_CASES], ids=lambda v: str(v))
def test_sentence_reference_is_the_oracle_and_autograd(B, nef, kind, zero):
    i, mask = R.sent_inputs(B, nef, zero), R.ce_mask(B, kind)
    g3, lam = R.GAMMAS[0][2], 5.0
    cnn, rnn = i.cnn.double().requires_grad_(True), i.rnn.double().requires_grad_(True)
    labels = torch.arange(B)
    if kind in (None, 'class'):
        l0, l1 = O.sent_loss(cnn, rnn, labels, None if kind is None else class_ids(B), B, g3, R.SENT_EPS)
    else:                                                   # the oracle's formula with an arbitrary mask
        n0, n1 = cnn.norm(2, dim=1, keepdim=True), rnn.norm(2, dim=1, keepdim=True)
        s = (cnn @ rnn.t() / (n0 @ n1.t()).clamp(min=R.SENT_EPS) * g3).masked_fill(mask, -R.INF)
        l0, l1 = F.cross_entropy(s, labels), F.cross_entropy(s.t(), labels)
    d = R.sent_direct(i.cnn, i.rnn, mask, g3, R.SENT_EPS, lam)
    same(d.loss, lam * (l0 + l1), 'loss')
    gc, gr = torch.autograd.grad(lam * (l0 + l1), [cnn, rnn])
    b = R.sent_backward(i.cnn, i.rnn, d.ds, g3, R.SENT_EPS)
    same(d.dcnn, gc, 'dcnn'); same(b.dcnn, gc, 'dcnn'); same(b.drnn, gr, 'drnn')
    assert bool((d.dcnn_cond >= d.dcnn_abs * (1 - 1e-12)).all()) and bool(torch.isfinite(d.dcnn).all())
    s = R.sent_forward(i.cnn, i.rnn, g3, R.SENT_EPS).s
    if zero:
        z = min(1, B - 1)
        assert float((s[z] if zero == 'cnn' else s[:, z]).abs().max()) == 0.0


def test_inputs_and_case_lists():
    """what the docstring of damsm_ref.py states about the inputs, and what the GPU test's coverage table relies on"""
    a1max, a1flat, amax17, amax289 = 0.0, 1.0, 0.0, 0.0
    for c in WORD_CASES:
        Fw = R.words_ref(c).fwd
        multi = (R.lengths(c.lens, c.L) > 1)[None, :, None, None].expand_as(Fw.attn1)
        lv = Fw.live[None, :, :, None]
        dS = (Fw.S - Fw.S.masked_fill(~lv, -R.INF).max(2, keepdim=True)[0]).masked_fill(~lv, 0.0)
        if c.peak:
            assert float(dS.min()) < -104, 'no exp underflows to zero in float32'
            assert float((dS < -87.4).double().mean()) > 0.3
        elif bool(multi.any()):
            assert float(dS.min()) > -20
            a1max = max(a1max, float(Fw.attn1[multi].max()))
            a1flat = min(a1flat, float(Fw.attn1.masked_fill(~multi, 1.0).max(2)[0].min()))
            if c.R == 17:
                amax17 = max(amax17, float(Fw.attn.max()))
            if c.R == 289:
                amax289 = max(amax289, float(Fw.attn.max()))
    print('largest attn1 %.4f, flattest softmax over the words: max %.3f; largest attn at R = 17: %.3f, at R = 289: %.3f'
          % (a1max, a1flat, amax17, amax289))
    assert 0.9 < a1max < 0.9999 and a1flat < 0.2 and 3 / 17 < amax17 < 0.9 and 10 / 289 < amax289 < 0.9
    f32, mf = R.F32_CASES, R.MFMA_CASES
    assert {c.L for c in f32} >= {1, 20, 21, 32} and {c.R for c in f32} >= {1, 17, 289, 320}
    assert {c.nef for c in f32} >= {32, 96, 192, 256} and {c.B for c in f32} >= {1, 3}
    assert {c.R for c in mf} >= {1, 33, 160, 289, 384} and {c.nef for c in mf} >= {64, 128, 320}
    assert {c.L for c in mf} >= {1, 16, 17, 32} and {c.B for c in mf} == {1, 2, 3} and {c.flo for c in mf} == {0, 1}
    assert {t for c in mf for t in c.lens} >= {0, 1, 16, 17, 32, 35}
    assert any(0 in c.lens and c.L + 3 in c.lens and c.L in c.lens for c in f32)
    assert {g for c in f32 + mf for g in (c.g,)} == {0, 1}
    for c in f32 + mf:
        assert c.B * c.B * c.L * max(c.R, c.nef) <= 9 * 32 * 384
        if c.zero:
            assert R.ZERO_WORD[1] < c.lens[R.ZERO_WORD[0]]
    assert all(c.nef % 64 == 0 and c.R <= 320 for c in R.BOTH_ARMS) and len(R.BOTH_ARMS) >= 5


# ------------------------------------------------------------------ (2) emulations inside, mutations outside
def emulated_fwd(fam, c, mut=(), k=None):
    i, (g1, g2, _) = R.words_inputs(c), R.gammas(c)
    o = R.emulate_words_fwd(fam, i.feat, i.words, i.lens, g1, g2, mut)
    return o, R.words_fwd_ratios(fam, o, R.words_ref(c).fwd, k)


def emulated_bwd(fam, c, mut=(), acc=1, with_words=True, chained=False, k=None):
    i, (g1, g2, _) = R.words_inputs(c), R.gammas(c)
    ref = R.words_ref(c, chained)
    saved = emulated_fwd(fam, c)[0] if chained else R.saved_for_backward(ref.fwd)
    adds = fam == 'f32' or acc
    pf = R.prefill(c.B * c.nef * c.R, R.TAG_DFEAT) if adds else torch.full((c.B * c.nef * c.R,), R.NAN)
    pw = R.prefill(c.B * c.nef * c.L, R.TAG_DWORDS) if with_words else None
    o = R.emulate_words_bwd(fam, i.feat, i.words, i.lens, g1, g2, i.dsim, saved, pf, acc, pw, mut)
    dfeat = o.dfeat.double() - pf.double().view_as(o.dfeat) if adds else o.dfeat
    dwords = None if pw is None else o.dwords.double() - pw.double().view_as(o.dwords)
    return R.words_bwd_ratios(fam, dfeat, dwords, ref, pf if adds else None, pw, k)


@pytest.mark.parametrize('fam,c', FAM_CASES, ids=fam_id)
def test_words_emulations_are_inside(fam, c):
    name = '%s %s' % (fam, R.case_id(c))
    inside(name + ' fwd', emulated_fwd(fam, c)[1])
    inside(name + ' bwd', emulated_bwd(fam, c, acc=1))
    inside(name + ' bwd, dwords NULL, accumulate 0', emulated_bwd(fam, c, acc=0, with_words=False))
    inside(name + ' bwd chained', emulated_bwd(fam, c, chained=True))


def test_mfma_multiple():
    """MFMA_K: the smallest whole multiple of 2^-17 x the conditioned sum that leaves the emulation of the matrix-core
    arithmetic at or below one half at every case and output; hi-only features stay outside it"""
    need, where = 0.0, None
    for c in R.MFMA_CASES + R.LDS_CASES:
        for what, ratios in (('fwd', emulated_fwd('mfma', c, k=1.0)[1]), ('bwd', emulated_bwd('mfma', c, k=1.0)),
                             ('bwd chained', emulated_bwd('mfma', c, chained=True, k=1.0))):
            for key, v in ratios.items():
                if 'unwritten' not in key and 't >= T' not in key and v > need:
                    need, where = v, '%s %s of %s' % (what, key, R.case_id(c))
    k = float(max(1, -(-need // SPARE)))                    # the smallest whole k with need / k <= 1 / 2
    print('the emulation needs %.3f x 2^-17 x the conditioned sum (%s): MFMA_K = %g' % (need, where, k))
    assert k == R.MFMA_K, 'damsm_ref.MFMA_K = %g, derived %g' % (R.MFMA_K, k)
    hi = min(max(v for key, v in emulated_fwd('mfma', c, {'hi'})[1].items()) for c in R.MFMA_CASES if c.flo and c.L > 1)
    print('hi-only features: at least %.1f x the bound at every case with lo parts and more than one word' % hi)
    assert hi > 2.0


F32_B3, F32_T, F32_16, F32_Z = R.F32_CASES[1], R.F32_CASES[2], R.F32_CASES[3], R.F32_CASES[6]
MF_B3, MF_T, MF_CT, MF_Z = R.MFMA_CASES[3], R.MFMA_CASES[1], R.MFMA_CASES[2], R.MFMA_CASES[7]
FWD_MUTATIONS = [('pair', F32_B3, MF_B3), ('T+1', F32_T, MF_B3), ('T-1', F32_T, MF_B3), ('region', F32_B3, MF_T),
                 ('ctile', F32_B3, MF_CT), ('axis', F32_B3, MF_T), ('gamma1', F32_B3, MF_T), ('hi', None, MF_T)]
BWD_MUTATIONS = FWD_MUTATIONS[:7] + [('w16', F32_16, MF_B3), ('hi', None, None), ('acc', F32_B3, MF_T), ('clampflag', F32_Z, MF_Z)]


@pytest.mark.parametrize('mut,cf,cm', FWD_MUTATIONS, ids=lambda v: v if isinstance(v, str) else '')
def test_forward_mutations_are_outside(mut, cf, cm):
    for fam, c in (('f32', cf), ('mfma', cm)):
        if c is not None:
            outside('%s fwd %s at %s' % (fam, mut, R.case_id(c)), emulated_fwd(fam, c, {mut})[1])


@pytest.mark.parametrize('mut,cf,cm', BWD_MUTATIONS, ids=lambda v: v if isinstance(v, str) else '')
def test_backward_mutations_are_outside(mut, cf, cm):
    for fam, c in (('f32', cf), ('mfma', cm)):
        if c is None:
            continue
        if mut in ('T+1', 'T-1', 'w16'):
            assert any((1 < t < c.L) if mut != 'w16' else t > 16 for t in R.lengths(c.lens, c.L).tolist())
        for acc in ((0, 1) if (mut == 'acc' and fam == 'mfma') else (1,)):
            r = emulated_bwd(fam, c, {mut}, acc=acc)
            outside('%s bwd %s at %s, accumulate %d' % (fam, mut, R.case_id(c), acc), r)
            if mut in ('w16', 'acc'):                       # d(features) must fail on its own
                assert r['dfeat'] > 1.0


def sent_emulated(B, nef, zero, mut=()):
    i = R.sent_inputs(B, nef, zero)
    g3 = R.GAMMAS[0][2]
    ref = R.sent_backward(i.cnn, i.rnn, i.ds, g3, R.SENT_EPS)
    pc, pr = R.prefill(B * nef, R.TAG_DCNN), R.prefill(B * nef, R.TAG_DRNN)
    o = R.emulate_sent_bwd(i.cnn, i.rnn, i.ds, g3, R.SENT_EPS, pc, pr, mut)
    res = R.sent_bwd_ratios(o.dcnn.double() - pc.double().view(B, nef), o.drnn.double() - pr.double().view(B, nef), ref, pc, pr)
    res['s'] = R.elem_ratio(R.emulate_sent_fwd(i.cnn, i.rnn, g3, R.SENT_EPS, mut), R.sent_forward(i.cnn, i.rnn, g3, R.SENT_EPS).s)
    return res


@pytest.mark.parametrize('B,nef,zero', R.SENT_CASES, ids=lambda v: str(v))
def test_sentence_emulations_are_inside(B, nef, zero):
    inside('sent B%d nef%d zero=%s' % (B, nef, zero), sent_emulated(B, nef, zero))


@pytest.mark.parametrize('B,nef,kind,zero', R.SENT_DIRECT_CASES, ids=lambda v: str(v))
def test_sent_direct_emulation_is_inside(B, nef, kind, zero):
    i, mask = R.sent_inputs(B, nef, zero), R.ce_mask(B, kind)
    g3, lam = R.GAMMAS[0][2], 5.0
    ref = R.sent_direct(i.cnn, i.rnn, mask, g3, R.SENT_EPS, lam)
    o = R.emulate_sent_direct(i.cnn, i.rnn, mask, g3, R.SENT_EPS, lam)
    inside('sent_direct B%d nef%d %s' % (B, nef, kind), R.sent_direct_ratios(o.loss, o.dcnn, ref))
    if kind == 'asym':
        m = R.emulate_sent_direct(i.cnn, i.rnn, mask, g3, R.SENT_EPS, lam, {'maskT'})
        outside('sent_direct maskT', R.sent_direct_ratios(m.loss, m.dcnn, ref))
    if B == 17:
        # (a transposed score matrix under a SYMMETRIC mask swaps loss0 and loss1 and nothing else: only 'asym' can tell)
        for mut in ('colrow',) + (('pair',) if kind == 'asym' else ()) + (('clampflag',) if zero else ()):
            m = R.emulate_sent_direct(i.cnn, i.rnn, mask, g3, R.SENT_EPS, lam, {mut})
            outside('sent_direct ' + mut, R.sent_direct_ratios(m.loss, m.dcnn, ref))


@pytest.mark.parametrize('mut,case', [('pair', R.SENT_CASES[2]), ('clampflag', R.SENT_CASES[2]), ('clampflag', R.SENT_CASES[3]),
                                      ('acc', R.SENT_CASES[1])], ids=lambda v: str(v))
def test_sentence_mutations_are_outside(mut, case):
    outside('sent %s at %s' % (mut, case), sent_emulated(*case, mut={mut}))


@pytest.mark.parametrize('B,kind,scale,lam', R.CE_CASES, ids=lambda v: str(v))
def test_cross_entropy_emulations(B, kind, scale, lam):
    score, mask = R.ce_scores(B), R.ce_mask(B, kind)
    ref = R.ce_direct(score, mask, scale, lam)
    name = 'ce B%d %s scale %g lam %g' % (B, kind, scale, lam)
    inside(name, R.ce_ratios(R.emulate_ce_pair(score, mask, scale), ref.pair))
    inside(name + ' direct', R.ce_ratios(R.emulate_ce_direct(score, mask, scale, lam), ref))
    if kind == 'asym':
        outside(name + ' maskT', R.ce_ratios(R.emulate_ce_pair(score, mask, scale, {'maskT'}), ref.pair))
        outside(name + ' direct maskT', R.ce_ratios(R.emulate_ce_direct(score, mask, scale, lam, {'maskT'}), ref))
    if B > 1 and kind != 'all':
        outside(name + ' colrow', R.ce_ratios(R.emulate_ce_pair(score, mask, scale, {'colrow'}), ref.pair))
        outside(name + ' direct colrow', R.ce_ratios(R.emulate_ce_direct(score, mask, scale, lam, {'colrow'}), ref))
