"""The 13 entry points of csrc/damsm.hip and csrc/damsm_mfma.hip called directly through the C ABI (sbagan._lib), at the
smallest shape that reaches each kernel template and each arm of the host dispatch, element by element against the
float64 reference of tests/damsm_ref.py.  Word shapes are (B, nef, R, L) with lens (the cap_lens as given; the kernels
clamp them to [1, L]).

kernel                             host condition that selects it                         covered by
---------------------------------  -----------------------------------------------------  -----------------------------------
damsm_words_fwd_kernel<20>         sba_damsm_words_fwd, L <= 20                           test_words_forward[f32]: (1, 32, 1, 1),
                                                                                          (3, 96, 17, 20) lens 0 / 20 / 23,
                                                                                          (3, 64, 33, 9) gamma1 = 5, the peaked
                                                                                          and the zero-word case
damsm_words_fwd_kernel<32>         sba_damsm_words_fwd, L > 20                            (3, 192, 289, 21) lens 21 / 1 / 13,
                                                                                          (2, 256, 320, 32): R = NT, L = TMAX
damsm_words_bwd_kernel<20> / <32>  sba_damsm_words_bwd, the same switch                   test_words_backward[f32] at the same
  dwords NULL / given                                                                     cases, dwords given and NULL, saved
                                                                                          tensors from float64 (NaN at t >= T);
                                                                                          test_words_chained[f32]
  det_feat / det_words + fold      deterministic mode                                     test_words_backward_deterministic[f32]
damsm_sent_fwd_kernel              sba_damsm_sent_fwd (always)                            test_sentence: nef 1 / 63 / 64 / 65 /
damsm_sent_bwd_kernel              sba_damsm_sent_bwd, plain                              256, B 1 / 2 / 5, dcnn NULL, drnn NULL,
damsm_sent_bwd_det_kernel          sba_damsm_sent_bwd, deterministic mode                 a zero vector on either side; both modes
ce_pair_kernel                     sba_ce_pair (always)                                   test_cross_entropies: B 1 / 2 / 17 / 96,
ce_pair_direct_kernel              sba_ce_pair_direct (always)                            mask NULL / class / all / asymmetric,
                                                                                          scale 1 / 10, lam 1 / 5
combine2_kernel                    sba_combine2 (always)                                  test_combine2: n 1 / 255 / 256 / 257
damsm_prep_kernel                  sba_damsm_prep: flag_mode 1 / tmode 0 (words), then    every matrix-core test; the flag word:
                                   flag_mode 2 / tmode 1 (features)                       test_words_forward[mfma]
damsm_words_fwd_mfma_kernel        sba_damsm_words_fwd_mfma                               test_words_forward[mfma]: R 1 / 33 /
  body<true>  (FLO)                the flag the prep pass wrote: some lo part != 0        160 / 289 / 384 (1, 2, 5, 10, 12 region
  body<false>                      every feature exactly bf16                             tiles), nef 64 / 128 / 320, L 1 / 16 /
                                                                                          17 / 32, B 1 / 2 / 3; bf16 features at
                                                                                          (3, 128, 160, 17) and (3, 128, 289, 18)
damsm_words_bwd1_mfma_kernel       sba_damsm_words_bwd_mfma (always); the same flag       test_words_backward[mfma], dwords given
  need_words false / atomics /     dwords NULL / given / deterministic mode               / NULL; _deterministic[mfma];
  det_words                                                                               test_words_chained[mfma]
damsm_words_bwd2_mfma_kernel       sba_damsm_words_bwd_mfma (always)                      the same; lens 16 | 1 (second k-step
  accumulate 0 / 1                                                                        skipped), 17 (taken); nef 320 (a
                                                                                          workgroup with two live waves);
                                                                                          accumulate 0 on NaN, 1 on a prefill
damsm_sent_direct_kernel           sba_damsm_sent_direct; LDS above 64 KB at B = 96       test_sent_direct: B 1 / 2 / 17 / 96,
                                                                                          dcnn NULL and given
every SBA_E_ARG condition          --                                                     test_refusals (sba_det_alloc running out
                                                                                          of scratch left out: 2 GiB ring)
LDS limit of the matrix-core arm   mf_ok: 128 (nef + RP) + 4096 <= 160 KB                 test_prep_bytes_promises_acceptance:
                                                                                          (960, 288) runs AT the limit, (960, 289)
                                                                                          and (1024, 384) are refused by all
sba_det_alloc returning NULL        deterministic mode and the scratch ring exhausted      not reachable here: the ring is 2 GiB,
  (words_bwd, words_bwd_mfma)                                                             the largest request of this file 7 MB
These are the 15 kernels of the two files (the two LP and the two FLO templates counted once each); none of their arms
is unreachable through the C ABI.  No environment switch selects a kernel here (ops.DAMSM_MFMA picks between the two
families above the C ABI).

Bounds (tests/damsm_ref.py; tests/test_damsm_ref_cpu.py shows, at every case of this file, that an emulation of the
kernel family's stated arithmetic is inside each by a factor 2 and that thirteen mutations are outside).
  f32 stored values      attn1, attn, wctx, sim, sentence scores, losses, d0 / d1 / dscore, combine2: elementwise rtol
                         2e-4 / atol 2e-5 (elem_close)
  f32 gradients          1e-5 x the conditioned sum of the absolute summands (sums_close), + one float32 ulp of the
                         prefill where the kernel adds to one; compared as stored - prefill
  matrix-core arms       MFMA_K x 2^-17 x the conditioned sum, MFMA_K = 1 derived from the emulation on the CPU
  both arms              |f32 - matrix-core| <= the sum of their two bounds at the shapes both accept
attn, attn1 and wctx at t >= T are not written by either forward (still NaN afterwards) and not read by either backward
(handed over as NaN, the gradients are finite).  Isolated backward tests get sim / attn / attn1 / wctx from the float64
reference rounded to float32; the chained ones from the kernel's own forward.

entry point                  worst measured error / bound (MI355X)
---------------------------  -----------------------------------------------------------------------------------------
sba_damsm_words_fwd          attn1 0.090, attn 0.098, wctx 0.133 at the peaked case (2, 64, 33, 18), at most 0.013 elsewhere;
                             sim 0.005
sba_damsm_words_bwd          dfeat 0.0085 ((2, 256, 320, 32)), dwords 0.027 (peaked); deterministic mode 0.0050 / 0.0005;
                             chained 4e-5 (the conditioned sums then carry the forward's gains too)
sba_damsm_prep +             attn1 0.235 at the peaked case (the emulation: 0.234) and 0.215 at (2, 64, 384, 32), attn 0.096,
sba_damsm_words_fwd_mfma     wctx 0.206 (peaked), sim 0.0003; AT the LDS limit (1, 960, 288, 2): attn1 0.041
sba_damsm_words_bwd_mfma     dfeat 0.0038 ((3, 320, 289, 32), accumulate 1), dwords 0.035 (peaked); deterministic mode the
                             same; chained 2e-5; dfeat bit-equal run to run in plain mode
f32 against matrix cores     attn1 0.095, attn 0.037, wctx 0.030, dfeat 0.0032, dwords 0.0012, sim 0.0003
sba_damsm_sent_fwd           0.002
sba_damsm_sent_bwd           dcnn 0.223 ((2, 256)), drnn 0.326 ((5, 64), a zero cnn vector); deterministic mode the same
sba_ce_pair                  d0 0.023, d1 0.007, losses 0.0013
sba_ce_pair_direct           dscore 0.016, loss 0.0012; dscore bit-equal with sba_ce_pair + sba_combine2 at every case
sba_combine2                 0.001
sba_damsm_sent_direct        dcnn 0.0052 (B = 96), loss 0.0004; dcnn bit-equal with sent_fwd + ce_pair + combine2 +
                             sent_bwd (deterministic mode) at every case
The gradients sit at 1e-3 .. 1e-2 of their bounds: the conditioned sums are worst-case first-order bounds through two
softmaxes, and float32 rounding errors add up like a random walk.  What the gradient bounds are for is shown on the CPU:
every mutation of the backward is at 20 x its bound or more.

Every output buffer is PAD elements longer than documented and prefilled with NaN -- the ones the kernels add to with
non-zero values in front of a NaN tail; the tail must still be NaN afterwards and everything in front finite.
"""
from types import SimpleNamespace as NS

import pytest
import torch

pytestmark = pytest.mark.gpu

import damsm_ref as R  # noqa: E402
from test_kernels_gpu import _reset_cfg, dev  # noqa: E402,F401
from test_norm_kernels_gpu import (BIG, PAD, _refuse, deterministic, elem_close, front, lib, nans, p, prefilled, same_bits,  # noqa: E402
                                   stream, sums_close, twice)

F32 = torch.float32
FAMS = [('f32', c) for c in R.F32_CASES] + [('mfma', c) for c in R.MFMA_CASES]
fam_id = lambda v: v if isinstance(v, str) else R.case_id(v)       # noqa: E731
LAM = 5.0


def report(name, ratios):
    print('%-72s %s' % (name, '  '.join('%s %.3g' % kv for kv in sorted(ratios.items()))))
    for k, v in ratios.items():
        assert v <= 1.0, '%s: %s is at %.3f of its bound' % (name, k, v)


@pytest.fixture(scope='module', autouse=True)
def _leave_the_process_as_found():
    yield
    import gc
    from sbagan import ops
    for f in (R.words_inputs, R.words_ref):
        f.cache_clear()
    ops.set_deterministic(False)
    ops._DET_SCRATCH[0] = None                              # (set_deterministic(True) allocates the ring again when asked)
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def guarded(t, dev):
    """a flat device copy of t in front of PAD NaNs"""
    b = nans(t.numel() + PAD, F32, dev)
    b[:t.numel()] = t.float().flatten().to(dev)
    return b


def tail_is_nan(buf, n, name):
    assert bool(torch.isnan(buf[n:]).all()), '%s: wrote past its end' % name


# ------------------------------------------------------------------ the words loss: runners
def make_prep(dev, c, d):
    """sba_damsm_prep into an exactly sized scratch; checks the flag word behind the operands"""
    nbytes = int(lib().lib.sba_damsm_prep_bytes(c.B, c.nef, c.R, c.L))
    assert nbytes > 0
    prep = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
    lib().call('sba_damsm_prep', p(d.feat), p(d.words), p(d.lens), p(prep), nbytes, c.B, c.nef, c.R, c.L, stream())
    torch.cuda.synchronize()
    return prep


def lo_flag(prep):
    return int(prep[-256:-252].cpu().view(torch.int32)[0])


def on_device(dev, c):
    i = R.words_inputs(c)
    return NS(feat=i.feat.to(dev).contiguous(), words=i.words.to(dev).contiguous(), lens=i.lens.to(dev), dsim=i.dsim.to(dev).contiguous())


def run_fwd(fam, dev, c, d=None, prep=None):
    d = d or on_device(dev, c)
    g1, g2, _ = R.gammas(c)
    B, nef, Rn, L = c.B, c.nef, c.R, c.L
    o = NS(d=d, prep=prep, sim=nans(B * B + PAD, F32, dev), attn=nans(B * B * L * Rn + PAD, F32, dev),
           attn1=nans(B * B * L * Rn + PAD, F32, dev), wctx=nans(B * B * L * nef + PAD, F32, dev))
    if fam == 'f32':
        lib().call('sba_damsm_words_fwd', p(d.feat), p(d.words), p(d.lens), p(o.sim), p(o.attn), p(o.attn1), p(o.wctx), B, nef, Rn, L,
                   g1, g2, stream())
    else:
        o.prep = prep if prep is not None else make_prep(dev, c, d)
        lib().call('sba_damsm_words_fwd_mfma', p(o.prep), p(d.words), p(d.lens), p(o.sim), p(o.attn), p(o.attn1), p(o.wctx), B, nef,
                   Rn, L, g1, g2, stream())
    torch.cuda.synchronize()
    return o


def fwd_views(o, c, name):
    B, nef, Rn, L = c.B, c.nef, c.R, c.L
    tail_is_nan(o.attn, B * B * L * Rn, name + ' attn'); tail_is_nan(o.attn1, B * B * L * Rn, name + ' attn1')
    tail_is_nan(o.wctx, B * B * L * nef, name + ' wctx')
    return NS(sim=front(o.sim, B * B, name + ' sim').view(B, B), attn=o.attn[:B * B * L * Rn].cpu().view(B, B, L, Rn),
              attn1=o.attn1[:B * B * L * Rn].cpu().view(B, B, L, Rn), wctx=o.wctx[:B * B * L * nef].cpu().view(B, B, L, nef))


def check_fwd(fam, o, c, name):
    ref = R.words_ref(c).fwd
    v = fwd_views(o, c, name)
    report(name, R.words_fwd_ratios(fam, v, ref))
    if fam == 'f32':                                        # the project's own helper, where the issue names it
        lv = ref.live[None].expand(c.B, -1, -1)
        for k in ('attn1', 'attn', 'wctx'):
            elem_close(getattr(v, k)[lv], getattr(ref, k)[lv], name + ' ' + k)
        elem_close(v.sim, ref.sim, name + ' sim')
    return v


def run_bwd(fam, dev, c, saved, acc=1, with_words=True, d=None, prep=None):
    """saved: sim / attn / attn1 / wctx as guarded device buffers (NaN at t >= T and behind the end)"""
    d = d or on_device(dev, c)
    g1, g2, _ = R.gammas(c)
    B, nef, Rn, L = c.B, c.nef, c.R, c.L
    o = NS(adds=fam == 'f32' or bool(acc), pre_feat=None, pre_words=None, dwords=None)
    if o.adds:
        o.dfeat, o.pre_feat = prefilled(B * nef * Rn, R.TAG_DFEAT, dev)
    else:
        o.dfeat = nans(B * nef * Rn + PAD, F32, dev)
    if with_words:
        o.dwords, o.pre_words = prefilled(B * nef * L, R.TAG_DWORDS, dev)
    if fam == 'f32':
        lib().call('sba_damsm_words_bwd', p(d.feat), p(d.words), p(d.lens), p(saved.sim), p(saved.attn), p(saved.attn1), p(saved.wctx),
                   p(d.dsim), p(o.dfeat), p(o.dwords), B, nef, Rn, L, g1, g2, stream())
    else:
        prep = prep if prep is not None else make_prep(dev, c, d)
        nbytes = int(lib().lib.sba_damsm_bwd_bytes(B, nef, Rn, L))
        assert nbytes > 0
        scratch = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)        # "any contents": bf16 NaNs
        lib().call('sba_damsm_words_bwd_mfma', p(prep), p(d.words), p(d.lens), p(saved.sim), p(saved.attn), p(saved.attn1),
                   p(saved.wctx), p(d.dsim), p(scratch), nbytes, p(o.dfeat), int(acc), p(o.dwords), B, nef, Rn, L, g1, g2, stream())
    torch.cuda.synchronize()
    return o


def saved_from_reference(dev, c):
    s = R.saved_for_backward(R.words_ref(c).fwd)
    return NS(sim=guarded(s.sim, dev), attn=guarded(s.attn, dev), attn1=guarded(s.attn1, dev), wctx=guarded(s.wctx, dev))


def bwd_views(o, c, name):
    B, nef, Rn, L = c.B, c.nef, c.R, c.L
    dfeat = front(o.dfeat, B * nef * Rn, name + ' dfeat')
    if o.adds:
        dfeat = dfeat - o.pre_feat
    dwords = None
    if o.dwords is not None:
        dwords = (front(o.dwords, B * nef * L, name + ' dwords') - o.pre_words).view(B, nef, L)
    return dfeat.view(B, nef, Rn), dwords


def check_bwd(fam, o, c, name, chained=False):
    ref = R.words_ref(c, chained)
    dfeat, dwords = bwd_views(o, c, name)
    report(name, R.words_bwd_ratios(fam, dfeat, dwords, ref, o.pre_feat, o.pre_words))
    if fam == 'f32':
        unit = R.ULP32 / R.C_SUM
        sums_close(dfeat, ref.dfeat, ref.dfeat_cond + unit * o.pre_feat.abs().view_as(ref.dfeat), name + ' dfeat')
        if dwords is not None:
            sums_close(dwords, ref.dwords, ref.dwords_cond + unit * o.pre_words.abs().view_as(ref.dwords), name + ' dwords')
    return dfeat, dwords


# ------------------------------------------------------------------ the words loss: tests
@pytest.mark.parametrize('fam,c', FAMS, ids=fam_id)
def test_words_forward(dev, fam, c):
    """sim, attn1, attn, wctx within bound where t < T, still NaN where t >= T; the flag word of the prep pass"""
    o = run_fwd(fam, dev, c)
    check_fwd(fam, o, c, '%s fwd %s' % (fam, R.case_id(c)))
    if fam == 'mfma':
        assert lo_flag(o.prep) == c.flo, 'the lo flag is %d for features %s lo parts' % (lo_flag(o.prep), 'with' if c.flo else 'without')


@pytest.mark.parametrize('fam,c', FAMS, ids=fam_id)
def test_words_backward(dev, fam, c):
    """the backward alone, on the float64 forward rounded to float32 with NaN at t >= T: dwords given (dfeat added to a
    prefill / accumulate = 1) and dwords NULL (matrix cores: accumulate = 0 on a NaN-filled dfeat)"""
    saved, d = saved_from_reference(dev, c), on_device(dev, c)
    prep = make_prep(dev, c, d) if fam == 'mfma' else None
    name = '%s bwd %s' % (fam, R.case_id(c))
    o = run_bwd(fam, dev, c, saved, 1, True, d, prep)
    check_bwd(fam, o, c, name + ', dwords given, accumulate 1')
    o2 = run_bwd(fam, dev, c, saved, 0, False, d, prep)
    check_bwd(fam, o2, c, name + ', dwords NULL, accumulate 0')
    if fam == 'mfma':                                       # one owner per element, no atomics: the same bits again
        o3 = run_bwd(fam, dev, c, saved, 0, False, d, prep)
        same_bits(o2.dfeat[:c.B * c.nef * c.R], o3.dfeat[:c.B * c.nef * c.R], 'dfeat, matrix cores, plain mode')


@pytest.mark.parametrize('fam,c', [('f32', R.F32_CASES[1]), ('f32', R.F32_CASES[3]), ('mfma', R.MFMA_CASES[1]), ('mfma', R.MFMA_CASES[3])],
                         ids=fam_id)
def test_words_backward_deterministic(dev, fam, c):
    """det_feat / det_words + sba_det_fold: within the same bounds, still ADDED onto the prefill (the fold adds as the
    atomics do), and two runs bit-equal"""
    saved, d = saved_from_reference(dev, c), on_device(dev, c)
    prep = make_prep(dev, c, d) if fam == 'mfma' else None
    with deterministic(dev) as ops:
        o1, o2 = twice(ops, lambda: run_bwd(fam, dev, c, saved, 1, True, d, prep))
    check_bwd(fam, o1, c, '%s bwd, deterministic, %s' % (fam, R.case_id(c)))
    same_bits(o1.dfeat, o2.dfeat, 'dfeat'); same_bits(o1.dwords, o2.dwords, 'dwords')


@pytest.mark.parametrize('fam,c', [('f32', R.F32_CASES[1]), ('f32', R.F32_CASES[2]), ('mfma', R.MFMA_CASES[2]), ('mfma', R.MFMA_CASES[3])],
                         ids=fam_id)
def test_words_chained(dev, fam, c):
    """forward -> backward on the kernel's own sim / attn / attn1 / wctx (both LP templates; both FLO templates)"""
    o = run_fwd(fam, dev, c)
    b = run_bwd(fam, dev, c, o, 1, True, o.d, o.prep)
    check_bwd(fam, b, c, '%s chained %s' % (fam, R.case_id(c)), chained=True)


@pytest.mark.parametrize('c', R.BOTH_ARMS, ids=R.case_id)
def test_both_arms_agree(dev, c):
    """the f32 and the matrix-core kernels against each other, within the sum of their two bounds"""
    ref = R.words_ref(c)
    Fw = ref.fwd
    lv = Fw.live[None].expand(c.B, -1, -1)
    d = on_device(dev, c)
    vf = fwd_views(run_fwd('f32', dev, c, d), c, 'f32')
    vm = fwd_views(run_fwd('mfma', dev, c, d), c, 'mfma')
    k = R.MFMA_K * R.U_MFMA
    res = {}
    for n in ('attn1', 'attn', 'wctx'):
        r = getattr(Fw, n)[lv]
        res[n] = R.agree_ratio(getattr(vf, n)[lv], getattr(vm, n)[lv], R.ATOL + R.RTOL * r.abs(), k * getattr(Fw, n + '_cond')[lv])
    res['sim'] = R.agree_ratio(vf.sim, vm.sim, R.ATOL + R.RTOL * Fw.sim.abs(), k * Fw.sim_cond)
    saved = saved_from_reference(dev, c)
    bf, bm = run_bwd('f32', dev, c, saved, 1, True, d), run_bwd('mfma', dev, c, saved, 1, True, d)
    (ff, wf), (fm, wm) = bwd_views(bf, c, 'f32'), bwd_views(bm, c, 'mfma')
    ulp_f, ulp_w = R.ULP32 * bf.pre_feat.abs().view_as(ff), R.ULP32 * bf.pre_words.abs().view_as(wf)
    res['dfeat'] = R.agree_ratio(ff, fm, R.C_SUM * ref.dfeat_cond + ulp_f, k * ref.dfeat_cond + ulp_f)
    res['dwords'] = R.agree_ratio(wf, wm, R.C_SUM * ref.dwords_cond + ulp_w, k * ref.dwords_cond + ulp_w)
    report('f32 against matrix cores, ' + R.case_id(c), res)


# ------------------------------------------------------------------ sentence scores
def run_sent(dev, B, nef, zero, with_cnn=True, with_rnn=True):
    i = R.sent_inputs(B, nef, zero)
    g3 = R.GAMMAS[0][2]
    cnn, rnn, ds = i.cnn.to(dev), i.rnn.to(dev), i.ds.to(dev).contiguous()
    o = NS(i=i, s=nans(B * B + PAD, F32, dev), dcnn=None, drnn=None, pc=None, pr=None)
    lib().call('sba_damsm_sent_fwd', p(cnn), p(rnn), p(o.s), B, nef, g3, R.SENT_EPS, stream())
    if with_cnn:
        o.dcnn, o.pc = prefilled(B * nef, R.TAG_DCNN, dev)
    if with_rnn:
        o.drnn, o.pr = prefilled(B * nef, R.TAG_DRNN, dev)
    lib().call('sba_damsm_sent_bwd', p(cnn), p(rnn), p(ds), p(o.dcnn), p(o.drnn), B, nef, g3, R.SENT_EPS, stream())
    torch.cuda.synchronize()
    return o


def check_sent(o, B, nef, name):
    g3 = R.GAMMAS[0][2]
    elem_close(front(o.s, B * B, name + ' s'), R.sent_forward(o.i.cnn, o.i.rnn, g3, R.SENT_EPS).s, name + ' s')
    ref = R.sent_backward(o.i.cnn, o.i.rnn, o.i.ds, g3, R.SENT_EPS)
    dc = None if o.dcnn is None else (front(o.dcnn, B * nef, name + ' dcnn') - o.pc).view(B, nef)
    dr = None if o.drnn is None else (front(o.drnn, B * nef, name + ' drnn') - o.pr).view(B, nef)
    report(name, R.sent_bwd_ratios(dc, dr, ref, o.pc, o.pr))


@pytest.mark.parametrize('B,nef,zero', R.SENT_CASES, ids=lambda v: str(v))
def test_sentence(dev, B, nef, zero):
    """scores elementwise; dcnn / drnn ADDED onto their prefill, both given and each NULL in turn; plain and deterministic
    (bit-equal twice)"""
    name = 'sent B%d nef%d zero=%s' % (B, nef, zero)
    for wc, wr in ((True, True), (False, True), (True, False)):
        check_sent(run_sent(dev, B, nef, zero, wc, wr), B, nef, '%s dcnn %d drnn %d' % (name, wc, wr))
    with deterministic(dev) as ops:
        for wc, wr in ((True, True), (False, True), (True, False)):
            o1, o2 = twice(ops, lambda: run_sent(dev, B, nef, zero, wc, wr))
            check_sent(o1, B, nef, '%s deterministic dcnn %d drnn %d' % (name, wc, wr))
            for a, b in ((o1.dcnn, o2.dcnn), (o1.drnn, o2.drnn)):
                if a is not None:
                    same_bits(a, b, name)


# ------------------------------------------------------------------ cross entropies, combine2, the direct kernels
def mask8(mask, dev):
    return None if mask is None else mask.to(torch.uint8).contiguous().to(dev)


def run_ce(dev, score, m8, scale, lam, B):
    o = NS(loss=nans(2 + PAD, F32, dev), d0=nans(B * B + PAD, F32, dev), d1=nans(B * B + PAD, F32, dev),
           loss_d=nans(1 + PAD, F32, dev), dscore=nans(B * B + PAD, F32, dev))
    lib().call('sba_ce_pair', p(score), p(m8), scale, p(o.loss), p(o.d0), p(o.d1), B, stream())
    lib().call('sba_ce_pair_direct', p(score), p(m8), scale, lam, p(o.loss_d), p(o.dscore), B, stream())
    torch.cuda.synchronize()
    return o


def run_combine2(dev, a, ga, b, gb, n):
    out = nans(n + PAD, F32, dev)
    lib().call('sba_combine2', p(out), p(a), p(ga), p(b), p(gb), n, stream())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('B,kind,scale,lam', R.CE_CASES, ids=lambda v: str(v))
def test_cross_entropies(dev, B, kind, scale, lam):
    """sba_ce_pair and sba_ce_pair_direct elementwise against float64; the direct kernel equals ce_pair + combine2 bit for
    bit in dscore; with every off-diagonal entry hidden both losses and every gradient are exactly 0"""
    score, mask = R.ce_scores(B), R.ce_mask(B, kind)
    ref = R.ce_direct(score, mask, scale, lam)
    sd = score.to(dev).contiguous()
    o = run_ce(dev, sd, mask8(mask, dev), scale, lam, B)
    name = 'ce B%d %s scale %g lam %g' % (B, kind, scale, lam)
    loss = front(o.loss, 2, name + ' loss')
    got = NS(loss0=loss[0], loss1=loss[1], d0=front(o.d0, B * B, name + ' d0').view(B, B), d1=front(o.d1, B * B, name + ' d1').view(B, B))
    report(name, R.ce_ratios(got, ref.pair))
    gd = NS(loss=front(o.loss_d, 1, name + ' loss_out')[0], dscore=front(o.dscore, B * B, name + ' dscore').view(B, B))
    report(name + ' direct', R.ce_ratios(gd, ref))
    for k in ('d0', 'd1'):
        elem_close(getattr(got, k), getattr(ref.pair, k), name + ' ' + k)
    elem_close(gd.dscore, ref.dscore, name + ' dscore')
    g = torch.full((1,), lam, dtype=F32, device=dev)
    comb = run_combine2(dev, o.d0, g, o.d1, g, B * B)
    assert torch.equal(front(comb, B * B, 'combine2'), gd.dscore.flatten()), 'sba_ce_pair_direct differs from sba_ce_pair + sba_combine2'
    if kind == 'all' or B == 1:
        assert float(loss.abs().max()) == 0.0 and float(gd.loss) == 0.0
        assert float(got.d0.abs().max()) == 0.0 and float(got.d1.abs().max()) == 0.0 and float(gd.dscore.abs().max()) == 0.0


@pytest.mark.parametrize('n', R.COMBINE_NS)
def test_combine2(dev, n):
    a, b = R.prefill(n, 321), R.prefill(n, 322) - 0.7
    ga, gb = torch.tensor([1.25]), torch.tensor([-3.5])
    out = run_combine2(dev, a.to(dev), ga.to(dev), b.to(dev), gb.to(dev), n)
    elem_close(front(out, n, 'combine2'), R.combine2(a, ga, b, gb), 'combine2 n=%d' % n)


@pytest.mark.parametrize('B,nef,kind,zero', R.SENT_DIRECT_CASES, ids=lambda v: str(v))
def test_sent_direct(dev, B, nef, kind, zero):
    """the one-launch sentence loss against float64, dcnn given (STORED over a NaN prefill) and NULL; and bit-equal with
    sent_fwd + ce_pair + combine2 + sent_bwd in deterministic mode on a cleared dcnn"""
    i, mask = R.sent_inputs(B, nef, zero), R.ce_mask(B, kind)
    g3 = R.GAMMAS[0][2]
    ref = R.sent_direct(i.cnn, i.rnn, mask, g3, R.SENT_EPS, LAM)
    cnn, rnn, m8 = i.cnn.to(dev), i.rnn.to(dev), mask8(mask, dev)
    name = 'sent_direct B%d nef%d %s' % (B, nef, kind)
    loss, dcnn = nans(1 + PAD, F32, dev), nans(B * nef + PAD, F32, dev)
    lib().call('sba_damsm_sent_direct', p(cnn), p(rnn), p(m8), g3, R.SENT_EPS, LAM, p(loss), p(dcnn), B, nef, stream())
    loss0 = nans(1 + PAD, F32, dev)
    lib().call('sba_damsm_sent_direct', p(cnn), p(rnn), p(m8), g3, R.SENT_EPS, LAM, p(loss0), None, B, nef, stream())
    torch.cuda.synchronize()
    got = front(dcnn, B * nef, name + ' dcnn')
    report(name, R.sent_direct_ratios(front(loss, 1, name + ' loss'), got.view(B, nef), ref))
    same_bits(loss, loss0, 'the loss with dcnn NULL')
    if kind == 'all' or B == 1:
        assert float(front(loss, 1, 'loss')[0]) == 0.0 and float(got.abs().max()) == 0.0
    # the chain the direct kernel replaces
    s, l2, d0, d1 = (nans(n + PAD, F32, dev) for n in (B * B, 2, B * B, B * B))
    lam = torch.full((1,), LAM, dtype=F32, device=dev)
    with deterministic(dev) as ops:
        ops.det_reset()
        lib().call('sba_damsm_sent_fwd', p(cnn), p(rnn), p(s), B, nef, g3, R.SENT_EPS, stream())
        lib().call('sba_ce_pair', p(s), p(m8), 1.0, p(l2), p(d0), p(d1), B, stream())
        ds = run_combine2(dev, d0, lam, d1, lam, B * B)
        chain = nans(B * nef + PAD, F32, dev)
        chain[:B * nef] = 0
        lib().call('sba_damsm_sent_bwd', p(cnn), p(rnn), p(ds), p(chain), None, B, nef, g3, R.SENT_EPS, stream())
        torch.cuda.synchronize()
    assert torch.equal(front(chain, B * nef, 'chain dcnn'), got), \
        'sba_damsm_sent_direct differs from sent_fwd + ce_pair + combine2 + sent_bwd: max %g' % float((front(chain, B * nef, 'c') - got).abs().max())
    elem_close(front(s, B * B, 's'), ref.s, name + ' chain scores')


# ------------------------------------------------------------------ refusals
MF_BAD = [('nef = 32 (not a multiple of 64)', dict(nef=32)), ('nef = 1088', dict(nef=1088)), ('nef = 0', dict(nef=0)),
          ('R = 385', dict(R=385)), ('R = 0', dict(R=0)), ('L = 33', dict(L=33)), ('L = 0', dict(L=0)), ('B = 0', dict(B=0)),
          ('B = 1025', dict(B=1025)), ('LDS above 160 KB (nef 960, R 289)', dict(nef=960, R=289)),
          ('LDS above 160 KB (nef 1024, R 384)', dict(nef=1024, R=384))]
F32_BAD = [('nef = 48 (not a multiple of 32)', dict(nef=48)), ('nef = 0', dict(nef=0)), ('R = 321', dict(R=321)), ('R = 0', dict(R=0)),
           ('L = 33', dict(L=33)), ('L = 0', dict(L=0)), ('B = 0', dict(B=0)), ('B = 1025', dict(B=1025)),
           ('LDS above 160 KB (nef 1024, R 320, L 32)', dict(nef=1024, R=320, L=32))]


def _nulls(*keys):
    return [('%s = NULL' % k, {k: None}) for k in keys]


def test_refusals(dev):
    """every SBA_E_ARG condition of the 13 entry points: the call comes back refused and no output is written"""
    st = stream()
    L = lib().lib
    ins = lambda dt=F32: torch.ones(BIG, dtype=dt, device=dev)                     # noqa: E731
    outs = lambda: nans(BIG, F32, dev)                                                # noqa: E731
    B, nef, Rn, Lw = 2, 64, 40, 5
    lens = ins(torch.int64)
    shape = dict(B=B, nef=nef, R=Rn, L=Lw, g1=4.0, g2=5.0, st=st)
    order = ['feat', 'words', 'lens', 'sim', 'attn', 'attn1', 'wctx', 'B', 'nef', 'R', 'L', 'g1', 'g2', 'st']
    b = dict(feat=ins(), words=ins(), lens=lens, sim=outs(), attn=outs(), attn1=outs(), wctx=outs(), **shape)
    _refuse('sba_damsm_words_fwd', order, b, F32_BAD + _nulls('feat', 'words', 'lens', 'sim', 'attn', 'attn1', 'wctx'),
            ['sim', 'attn', 'attn1', 'wctx'])
    order = ['feat', 'words', 'lens', 'sim', 'attn', 'attn1', 'wctx', 'dsim', 'dfeat', 'dwords', 'B', 'nef', 'R', 'L', 'g1', 'g2', 'st']
    b = dict(feat=ins(), words=ins(), lens=lens, sim=ins(), attn=ins(), attn1=ins(), wctx=ins(), dsim=ins(), dfeat=outs(), dwords=outs(),
             **shape)
    _refuse('sba_damsm_words_bwd', order, b, F32_BAD + _nulls('feat', 'words', 'lens', 'sim', 'attn', 'attn1', 'wctx', 'dsim', 'dfeat'),
            ['dfeat', 'dwords'])
    # the matrix-core entry points and the two size queries
    for what, delta in MF_BAD:
        a = dict(shape); a.update(delta)
        assert L.sba_damsm_prep_bytes(a['B'], a['nef'], a['R'], a['L']) == -1, 'sba_damsm_prep_bytes accepted "%s"' % what
        assert L.sba_damsm_bwd_bytes(a['B'], a['nef'], a['R'], a['L']) == -1, 'sba_damsm_bwd_bytes accepted "%s"' % what
    nprep, nbwd = int(L.sba_damsm_prep_bytes(B, nef, Rn, Lw)), int(L.sba_damsm_bwd_bytes(B, nef, Rn, Lw))
    assert 0 < nprep <= 4 * BIG - 16 and 0 < nbwd <= 4 * BIG - 16
    prep = outs()
    order = ['feat', 'words', 'lens', 'prep', 'nprep', 'B', 'nef', 'R', 'L', 'st']
    b = dict(feat=ins(), words=ins(), lens=lens, prep=prep, nprep=nprep, B=B, nef=nef, R=Rn, L=Lw, st=st)
    _refuse('sba_damsm_prep', order, b, MF_BAD + _nulls('feat', 'words', 'lens', 'prep')
            + [('prep_bytes one short', dict(nprep=nprep - 1)), ('prep not 16-byte aligned', dict(prep=prep[2:]))], ['prep'])
    order = ['prep', 'words', 'lens', 'sim', 'attn', 'attn1', 'wctx', 'B', 'nef', 'R', 'L', 'g1', 'g2', 'st']
    b = dict(prep=prep, words=ins(), lens=lens, sim=outs(), attn=outs(), attn1=outs(), wctx=outs(), **shape)
    _refuse('sba_damsm_words_fwd_mfma', order, b, MF_BAD + _nulls('prep', 'words', 'lens', 'sim', 'attn', 'attn1', 'wctx'),
            ['sim', 'attn', 'attn1', 'wctx'])
    scratch = outs()
    order = ['prep', 'words', 'lens', 'sim', 'attn', 'attn1', 'wctx', 'dsim', 'scratch', 'nbwd', 'dfeat', 'acc', 'dwords', 'B', 'nef', 'R',
             'L', 'g1', 'g2', 'st']
    b = dict(prep=prep, words=ins(), lens=lens, sim=ins(), attn=ins(), attn1=ins(), wctx=ins(), dsim=ins(), scratch=scratch, nbwd=nbwd,
             dfeat=outs(), acc=0, dwords=outs(), **shape)
    _refuse('sba_damsm_words_bwd_mfma', order, b,
            MF_BAD + _nulls('prep', 'words', 'lens', 'sim', 'attn', 'attn1', 'wctx', 'dsim', 'scratch', 'dfeat')
            + [('scratch_bytes one short', dict(nbwd=nbwd - 1)), ('scratch not 16-byte aligned', dict(scratch=scratch[2:]))],
            ['dfeat', 'dwords', 'scratch'])
    # sentence scores, cross entropies, combine2
    bad_b = lambda top: [('B = 0', dict(B=0)), ('B = %d' % (top + 1), dict(B=top + 1)), ('B = -1', dict(B=-1))]       # noqa: E731
    order = ['cnn', 'rnn', 's', 'B', 'nef', 'g3', 'eps', 'st']
    b = dict(cnn=ins(), rnn=ins(), s=outs(), B=5, nef=65, g3=10.0, eps=1e-8, st=st)
    _refuse('sba_damsm_sent_fwd', order, b, bad_b(1024) + [('nef = 0', dict(nef=0))] + _nulls('cnn', 'rnn', 's'), ['s'])
    order = ['cnn', 'rnn', 'ds', 'dcnn', 'drnn', 'B', 'nef', 'g3', 'eps', 'st']
    b = dict(cnn=ins(), rnn=ins(), ds=ins(), dcnn=outs(), drnn=outs(), B=5, nef=65, g3=10.0, eps=1e-8, st=st)
    _refuse('sba_damsm_sent_bwd', order, b, bad_b(1024) + [('nef = 0', dict(nef=0))] + _nulls('cnn', 'rnn', 'ds'), ['dcnn', 'drnn'])
    m8 = torch.zeros(BIG, dtype=torch.uint8, device=dev)
    order = ['score', 'mask', 'scale', 'loss', 'd0', 'd1', 'B', 'st']
    b = dict(score=ins(), mask=m8, scale=10.0, loss=outs(), d0=outs(), d1=outs(), B=17, st=st)
    _refuse('sba_ce_pair', order, b, bad_b(96) + _nulls('score', 'loss', 'd0', 'd1'), ['loss', 'd0', 'd1'])
    order = ['score', 'mask', 'scale', 'lam', 'loss', 'dscore', 'B', 'st']
    b = dict(score=ins(), mask=m8, scale=10.0, lam=5.0, loss=outs(), dscore=outs(), B=17, st=st)
    _refuse('sba_ce_pair_direct', order, b, bad_b(96) + _nulls('score', 'loss', 'dscore'), ['loss', 'dscore'])
    order = ['cnn', 'rnn', 'mask', 'g3', 'eps', 'lam', 'loss', 'dcnn', 'B', 'nef', 'st']
    b = dict(cnn=ins(), rnn=ins(), mask=m8, g3=10.0, eps=1e-8, lam=5.0, loss=outs(), dcnn=outs(), B=17, nef=65, st=st)
    _refuse('sba_damsm_sent_direct', order, b, bad_b(96) + [('nef = 0', dict(nef=0))] + _nulls('cnn', 'rnn', 'loss'), ['loss', 'dcnn'])
    order = ['out', 'a', 'ga', 'b', 'gb', 'n', 'st']
    b = dict(out=outs(), a=ins(), ga=ins(), b=ins(), gb=ins(), n=257, st=st)
    _refuse('sba_combine2', order, b, [('n = 0', dict(n=0)), ('n = -1', dict(n=-1))] + _nulls('out', 'a', 'ga', 'b', 'gb'), ['out'])


@pytest.mark.parametrize('nef,Rn', R.LDS_SHAPES, ids=lambda v: str(v))
def test_prep_bytes_promises_acceptance(dev, nef, Rn):
    """a positive sba_damsm_prep_bytes promises that prep, forward and backward accept the shape -- also where the
    per-pair LDS, 128 (nef + RP) + 4096 bytes, decides; (960, 288) then runs AT the 160 KB limit and is held to the
    bounds like every other case"""
    c = R.lds_case(nef, Rn)
    nbytes = int(lib().lib.sba_damsm_prep_bytes(c.B, nef, Rn, c.L))
    fits = R.lds_fits(nef, Rn)
    assert (nbytes > 0) == fits, 'sba_damsm_prep_bytes(%d, %d) = %d, LDS fits: %s' % (nef, Rn, nbytes, fits)
    assert (int(lib().lib.sba_damsm_bwd_bytes(c.B, nef, Rn, c.L)) > 0) == fits
    if nbytes <= 0:
        return
    o = run_fwd('mfma', dev, c)                             # (lib().call raises on a refusal)
    check_fwd('mfma', o, c, 'mfma fwd ' + R.case_id(c))
    check_bwd('mfma', run_bwd('mfma', dev, c, o, 0, True, o.d, o.prep), c, 'mfma chained ' + R.case_id(c), chained=True)
