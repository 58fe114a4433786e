"""Every entry point of csrc/text.hip and csrc/bert.hip called directly through the C ABI (sbagan._lib), at the smallest
shapes that reach each kernel and each arm, against the float64 references of tests/text_ref.py evaluated on the kernel's
own (f32 or storage-rounded) inputs.  The case lists, with the arm each case reaches, are in text_ref.py.

kernel                         host condition that selects it                          covered by
-----------------------------  ------------------------------------------------------  ------------------------------------
lstm_xproj_kernel              sba_lstm_bidir_fwd (always); 8 (caption, step) rows     test_lstm_bidir_fwd: B*T = 15 (partial
                               per workgroup, ceil(4H / 256) gate blocks per           tile), 16 and 8; ninput 4, 300, 2048 (64
                               direction, 8 * ninput * 4 bytes of dynamic LDS          KB of LDS: accepted, runs); one gate block
                                                                                       (H = 64), two (H = 128); token ids -1
                                                                                       and ntoken (read row 0)
lstm_recur_kernel<64 / 128>    sba_lstm_bidir_fwd: H                                   test_lstm_bidir_fwd: B = 1 and 3, Lout =
                                                                                       T, Lout = len < T, Lout < len, len 0,
                                                                                       len > T (clamped), state NULL / non-zero
lstm_recur_train_kernel        sba_lstm_recur_train: H                                 test_lstm_recur_train_and_bwd: both H, B
  <64 / 128>                                                                           = 1 and 5, lengths 1, T, middle, 0, -3,
                                                                                       T + 4, Lout = T, Lout = max(lens) < T,
                                                                                       Lout < len, state NULL / non-zero
lstm_recur_bwd_kernel          sba_lstm_recur_bwd: H                                   the same cases, on the tensors the
  <64 / 128>                                                                           training kernel just saved
the three GEMMs around them    ops.LstmBidirTrainFn                                    test_lstm_train_fn_end_to_end
bert_embed_ln_kernel<T, 0>     sba_bert_embed_ln; one wave per row, 4 rows per         test_embed_ln: rows 1, 5, 21, 8; per =
                               workgroup, per = C / 64 values per lane                 1, 12, 16; B >= 2 (position wraps);
                                                                                       tokens out of range; f32 and bf16
bert_add_ln_kernel<T, 0>       sba_bert_add_ln; the same geometry                      test_add_ln: the same rows and widths;
                                                                                       rows at mean 4 x std; a constant row
bert_attention_kernel<T, 0>    sba_bert_attention; grid (B, heads), L <= 32            test_attention: L = 1, 7, 20, 32; heads 1,
                                                                                       2, 12; logits +-50 and +-100
bert_gelu_kernel               sba_bert_gelu; min(ceil(n / 256), 4096) workgroups      test_gelu: n = 1, 255, 257, 4096 * 256 + 3
                                                                                       (the grid-stride loop wraps); in place
bert_tanh_t_kernel             sba_bert_tanh_transpose; the same grid                  test_tanh_transpose: up to (8, 32, 4100)
                                                                                       (wraps)
bert_words_head_bwd_kernel     sba_bert_words_head_bwd; nef / 64 workgroups            test_words_head_bwd: L = 1, 7, 32, 12
bert_sent_fc_bwd_kernel +      sba_bert_sent_head_bwd (two launches)                   test_sent_head_bwd: B = 1, 3, 64, 5
bert_sent_pooler_bwd_kernel
<T, 1> (dropout) kernels       the _train entry points                                 not repeated here: test_bert_train_gpu.
                                                                                       test_dropout_generator_masks pins them bit
                                                                                       for bit to the entry points above at p = 0
every SBA_E_ARG condition      --                                                      test_refusals

No environment switch selects a kernel: H, the dtype code and the entry point do.

Bounds (the project's own, tests/test_norm_kernels_gpu.py).  Elementwise f32 outputs (words, sent, gates, cs, hs, dG, hprev,
the LayerNorm outputs, ctx, GELU, tanh-transpose, dpre, dpooled): rtol 2e-4 / atol 2e-5.  Dot-product outputs and outputs
that are added to (gx, dbias, dW_fc, db_fc, dW_pool, db_pool; dx, dw_ih, dw_hh, db of the end-to-end test): |error| <= 1e-5
x the float64 sum of the ABSOLUTE summands of that element; the outputs the kernels ADD to are checked as (stored -
prefill).  bf16 outputs: relative L2 at most twice the one-rounding floor.  tests/test_text_ref_cpu.py holds a plain f32
evaluation of every case 5 x inside these bounds and every wrong variant listed in text_ref.py 10 x outside them.
Every LSTM entry point is run twice on identical inputs and must give identical bits.  words / sent of the training kernel
against those of sba_lstm_bidir_fwd on the same gx: inside the elementwise bound (asserted); whether they are bit-equal
is printed, not asserted.

Every output buffer is longer than the kernel should write and is prefilled with NaN -- the outputs the kernels add to with
non-zero values in front of a NaN tail; gates / cs / hs / dG / hprev are NaN all over: their rows t >= len are the caller's
to clear and must still be NaN afterwards, the rows t < len finite.

entry point              worst measured error / bound (MI355X)
-----------------------  --------------------------------------------------------------------------------------------
sba_lstm_bidir_fwd       gx 0.013 (1.32e-7 of sum |summands|, ninput = 4); words 0.004, sent 0.003
sba_lstm_recur_train     cs 0.013, words 0.009, hs 0.009, gates 0.008 (all at H = 128, w_hh x 1.7), sent 0.007; against
                         sba_lstm_bidir_fwd on the same gx: words 0.003, sent 0.002 -- NOT bit-equal at any of the four cases
sba_lstm_recur_bwd       dG 0.004, hprev 0.000 (a copy)
ops.LstmBidirTrainFn     dw_ih 0.394 (3.94e-6), dw_hh 0.339, db 0.125, dx 0.016, all at (3, 6, 300, 128); words, sent 0.013
sba_bert_embed_ln        f32 0.003;  bf16: rel L2 1.000 x the one-rounding floor = 0.50 of the bound
sba_bert_add_ln          f32 0.020 (the rows at mean 4 x std; 0.002 elsewhere); the constant row = beta exactly;  bf16 0.50
sba_bert_attention       f32 0.077 (logits +-50; 0.015 at unit q, k; 0.007 at logits +-100);  bf16 0.50
sba_bert_gelu            f32 0.004;  bf16 0.50
sba_bert_tanh_transpose  0.001
sba_bert_words_head_bwd  dpre f32 0.001, bf16 0.50;  dbias 0.011 (1.06e-7: (1, 1, 64), ONE term added to the prefill)
sba_bert_sent_head_bwd   dpooled 0.089 (B = 64);  dw_pool 0.130, dw_fc 0.020, db_pool 0.018 (all three at B = 1: single
                         products added to the prefill), db_fc 0.013
"""
from types import SimpleNamespace as NS

import pytest
import torch

pytestmark = pytest.mark.gpu

import text_ref as R  # noqa: E402
from test_dense_kernels_gpu import added_close, name_of  # noqa: E402
from test_kernels_gpu import _reset_cfg, dev  # noqa: E402,F401
from test_norm_kernels_gpu import (BIG, PAD, _refuse, elem_close, front, lib, low_close, nans, p, prefilled, same_bits,  # noqa: E402
                                   stream, sums_close, twice)

F32, BF16 = torch.float32, torch.bfloat16
MODES = {'f32': (0, F32), 'bf16': (1, BF16)}
cid = R.case_id


def on(dev, t):
    return None if t is None else t.to(dev).contiguous()


def out_close(got, ref, T, name):
    if T == F32:
        elem_close(got, ref, name)
    else:
        low_close(got.flatten(), ref.flatten(), name)


# ------------------------------------------------------------------ the LSTM entry points
def rows_of(buf, n_rows, width, written, name):
    """a [2][B*T][width] buffer prefilled with NaN: the rows t < len finite, every other row and the tail still NaN;
    returns the written rows"""
    b = buf.detach().float().cpu()
    assert bool(torch.isnan(b[2 * n_rows * width:]).all()), '%s: wrote past its end' % name
    v = b[:2 * n_rows * width].view(2, n_rows, width)
    assert bool(torch.isfinite(v[written]).all()), '%s: non-finite or unwritten values in a row t < len' % name
    assert bool(torch.isnan(v[~written]).all()), '%s: wrote a row t >= len (the caller clears those)' % name
    return v[written].double()


def run_train(dev, c, i, gx):
    """sba_lstm_recur_train on the device tensor gx [2][B*T][4H]"""
    B, T, Lout, H = c.B, c.T, c.Lout, c.H
    r = NS(c=c, i=i, w_hh=on(dev, i.w_hh), lens=on(dev, i.lens))
    r.h0, r.c0 = (None, None) if i.state is None else (on(dev, i.state[0]), on(dev, i.state[1]))
    r.words, r.sent = nans(B * 2 * H * Lout + PAD, F32, dev), nans(B * 2 * H + PAD, F32, dev)
    r.gates = nans(2 * B * T * 4 * H + PAD, F32, dev)
    r.cs, r.hs = nans(2 * B * T * H + PAD, F32, dev), nans(2 * B * T * H + PAD, F32, dev)
    lib().call('sba_lstm_recur_train', p(gx), p(r.lens), p(r.w_hh), p(r.h0), p(r.c0), p(r.words), p(r.sent), p(r.gates),
               p(r.cs), p(r.hs), B, T, Lout, H, stream())
    torch.cuda.synchronize()
    return r


def check_words_sent(words, sent, ref, c, name):
    B, H, Lout = c.B, c.H, c.Lout
    w = front(words, B * 2 * H * Lout, name + ' words').view(B, 2 * H, Lout)      # every element written, the tail NaN
    elem_close(w, ref.words, name + ' words')
    elem_close(front(sent, B * 2 * H, name + ' sent'), ref.sent, name + ' sent')
    for b, n in enumerate(R.clamp_lens(c.lens, c.T)):
        assert n >= Lout or bool((w[b, :, n:] == 0).all()), '%s: words past len = %d are not exact zeros' % (name, n)


def check_train(r, gx_cpu, name):
    c, i = r.c, r.i
    ref = R.lstm_recur(gx_cpu, i.w_hh, i.lens, i.state, c.T, c.Lout)
    check_words_sent(r.words, r.sent, ref, c, name)
    for k, width in (('gates', 4 * c.H), ('cs', c.H), ('hs', c.H)):
        elem_close(rows_of(getattr(r, k), c.B * c.T, width, ref.written, name + ' ' + k), getattr(ref, k)[ref.written], name + ' ' + k)
    return ref


def run_bwd(dev, tr):
    """sba_lstm_recur_bwd on the tensors the training kernel just saved (their rows t >= len still NaN)"""
    c, i = tr.c, tr.i
    B, T, Lout, H = c.B, c.T, c.Lout, c.H
    b = NS(tr=tr, dwords=on(dev, i.dwords), dsent=on(dev, i.dsent))
    b.dG, b.hprev = nans(2 * B * T * 4 * H + PAD, F32, dev), nans(2 * B * T * H + PAD, F32, dev)
    lib().call('sba_lstm_recur_bwd', p(tr.lens), p(tr.w_hh), p(tr.h0), p(tr.c0), p(tr.gates), p(tr.cs), p(tr.hs), p(b.dwords),
               p(b.dsent), p(b.dG), p(b.hprev), B, T, Lout, H, stream())
    torch.cuda.synchronize()
    return b


def check_bwd(b, written, name):
    c, i, tr = b.tr.c, b.tr.i, b.tr
    n = c.B * c.T
    saved = [getattr(tr, k)[:2 * n * w].cpu().view(2, n, w) for k, w in (('gates', 4 * c.H), ('cs', c.H), ('hs', c.H))]
    ref = R.lstm_bptt(*saved, i.w_hh, i.lens, i.state, i.dwords, i.dsent, c.T, c.Lout)
    elem_close(rows_of(b.dG, n, 4 * c.H, written, name + ' dG'), ref.dG[written], name + ' dG')
    elem_close(rows_of(b.hprev, n, c.H, written, name + ' hprev'), ref.hprev[written], name + ' hprev')


@pytest.mark.parametrize('c', R.RECUR_CASES, ids=cid)
def test_lstm_recur_train_and_bwd(dev, c):
    from sbagan import ops
    i = R.recur_inputs(c)
    gx = on(dev, i.gx)
    tr, tr2 = twice(ops, lambda: run_train(dev, c, i, gx))
    ref = check_train(tr, i.gx, 'recur_train %s' % cid(c))
    for k in ('words', 'sent', 'gates', 'cs', 'hs'):
        same_bits(getattr(tr, k), getattr(tr2, k), 'sba_lstm_recur_train ' + k)
    b, b2 = twice(ops, lambda: run_bwd(dev, tr))
    check_bwd(b, ref.written, 'recur_bwd %s' % cid(c))
    same_bits(b.dG, b2.dG, 'sba_lstm_recur_bwd dG'); same_bits(b.hprev, b2.hprev, 'sba_lstm_recur_bwd hprev')


def run_fwd(dev, c, i):
    B, T, Lout, H = c.B, c.T, c.Lout, c.H
    t = NS(**{k: on(dev, getattr(i, k)) for k in ('captions', 'lens', 'emb', 'w_ih', 'w_hh', 'b_ih', 'b_hh')})
    h0, c0 = (None, None) if i.state is None else (on(dev, i.state[0]), on(dev, i.state[1]))
    r = NS(gx=nans(2 * B * T * 4 * H + PAD, F32, dev), words=nans(B * 2 * H * Lout + PAD, F32, dev), sent=nans(B * 2 * H + PAD, F32, dev))
    lib().call('sba_lstm_bidir_fwd', p(t.captions), p(t.lens), p(t.emb), p(t.w_ih), p(t.w_hh), p(t.b_ih), p(t.b_hh), p(h0), p(c0),
               p(r.gx), p(r.words), p(r.sent), B, T, Lout, c.ntoken, c.ninput, H, stream())
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize('c', R.FWD_CASES, ids=cid)
def test_lstm_bidir_fwd(dev, c):
    from sbagan import ops
    i = R.fwd_inputs(c)
    name = 'bidir_fwd %s' % cid(c)
    r, r2 = twice(ops, lambda: run_fwd(dev, c, i))
    n = 2 * c.B * c.T * 4 * c.H
    xp = R.lstm_xproj(i.captions, i.emb, i.w_ih, i.b_ih, i.b_hh)
    gx = front(r.gx, n, name + ' gx')
    sums_close(gx, xp.gx, xp.gx_abs, name + ' gx')
    gx = gx.view(2, c.B * c.T, 4 * c.H)                     # the recurrence is judged on the gx the projection gave it
    check_words_sent(r.words, r.sent, R.lstm_recur(gx, i.w_hh, i.lens, i.state, c.T, c.Lout), c, name)
    for k in ('gx', 'words', 'sent'):
        same_bits(getattr(r, k), getattr(r2, k), 'sba_lstm_bidir_fwd ' + k)
    # the training kernel on the same gx
    tr = run_train(dev, c, i, r.gx)
    check_train(tr, gx, name + ' -> recur_train')
    m = c.B * 2 * c.H
    elem_close(tr.words[:m * c.Lout], r.words[:m * c.Lout].double().cpu(), name + ' words: training kernel against forward kernel')
    elem_close(tr.sent[:m], r.sent[:m].double().cpu(), name + ' sent: training kernel against forward kernel')
    print('%s: training kernel bit-equal to the forward kernel: words %s, sent %s'
          % (name, torch.equal(tr.words[:m * c.Lout], r.words[:m * c.Lout]), torch.equal(tr.sent[:m], r.sent[:m])))


@pytest.mark.parametrize('c', R.E2E_CASES, ids=cid)
def test_lstm_train_fn_end_to_end(dev, c):
    """ops.LstmBidirTrainFn (projection GEMM, recurrence, BPTT, the three GEMMs) with a non-zero state against float64
    autograd of torch.nn.LSTM over packed sequences: per element, at the sums bound with the absolute summands of the
    float64 dG"""
    from sbagan import ops
    i, f, g = R.e2e_reference(c)
    t = R.torch_lstm(i.x, i.w_ih, i.w_hh, i.b_ih, i.b_hh, i.lens, i.state, c.T)
    a = R.torch_lstm_grads(t, i.gw, i.gs)
    x, w_ih, w_hh, b_ih, b_hh = (on(dev, v).requires_grad_(True) for v in (i.x, i.w_ih, i.w_hh, i.b_ih, i.b_hh))
    words, sent = ops.LstmBidirTrainFn.apply(x, on(dev, i.lens), w_ih, w_hh, b_ih, b_hh, on(dev, i.state[0]), on(dev, i.state[1]), c.T)
    ((words * on(dev, i.gw)).sum() + (sent * on(dev, i.gs)).sum()).backward()
    torch.cuda.synchronize()
    name = 'LstmBidirTrainFn %s ' % cid(c)
    elem_close(words.detach(), t.words.detach(), name + 'words'); elem_close(sent.detach(), t.sent.detach(), name + 'sent')
    sums_close(x.grad, a.dx, g.dx_abs, name + 'dx')
    sums_close(w_ih.grad, a.dw_ih, g.dw_ih_abs, name + 'dw_ih')
    sums_close(w_hh.grad, a.dw_hh, g.dw_hh_abs, name + 'dw_hh')
    sums_close(b_ih.grad, a.db, g.db_abs, name + 'db (b_ih)')
    sums_close(b_hh.grad, a.db_hh, g.db_abs, name + 'db (b_hh)')


# ------------------------------------------------------------------ the BERT entry points
@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('case', R.EMBED_CASES, ids=cid)
def test_embed_ln(dev, case, mode):
    (B, L, C), _ = case
    code, T = MODES[mode]
    i = R.embed_inputs(B, L, C)
    t = [on(dev, v) for v in (i.tok, i.we, i.pe, i.te, i.gamma, i.beta)]
    out = nans(B * L * C + PAD, T, dev)
    lib().call('sba_bert_embed_ln', code, *[p(v) for v in t], p(out), B, L, C, i.ntoken, R.LN_EPS, stream())
    torch.cuda.synchronize()
    ref = R.embed_ln(i.tok, i.we, i.pe, i.te, i.gamma, i.beta, L)
    out_close(front(out, B * L * C, 'out'), ref, T, name_of('embed_ln', (B, L, C), mode))


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('case', R.ADD_LN_CASES, ids=cid)
def test_add_ln(dev, case, mode):
    (rows, C, kind), _ = case
    code, T = MODES[mode]
    i = R.add_ln_inputs(rows, C, kind, T)
    x, res, gamma, beta = (on(dev, v) for v in (i.x, i.res, i.gamma, i.beta))
    out = nans(rows * C + PAD, T, dev)
    lib().call('sba_bert_add_ln', code, p(x), p(res), p(gamma), p(beta), p(out), rows, C, R.LN_EPS, stream())
    torch.cuda.synchronize()
    got = front(out, rows * C, 'out')
    out_close(got, R.add_ln(i.x, i.res, i.gamma, i.beta), T, name_of('add_ln', (rows, C, kind), mode))
    if kind == 'const' and T == F32:
        assert torch.equal(got.view(rows, C)[2], i.beta.double()), 'x + res exactly constant: the output is beta exactly'


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('case', R.ATTN_CASES, ids=cid)
def test_attention(dev, case, mode):
    (B, L, heads, top), _ = case
    code, T = MODES[mode]
    C = 64 * heads
    qkv = R.attn_inputs(B, L, heads, top, T)
    q = on(dev, qkv)
    ctx = nans(B * L * C + PAD, T, dev)
    lib().call('sba_bert_attention', code, p(q), p(ctx), B, L, C, heads, stream())
    torch.cuda.synchronize()
    out_close(front(ctx, B * L * C, 'ctx'), R.attention(qkv, B, L, heads), T, name_of('attention', (B, L, heads, top), mode))


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('case', R.GELU_CASES, ids=cid)
def test_gelu(dev, case, mode):
    n, _ = case
    code, T = MODES[mode]
    xin = R.gelu_inputs(n, T)
    x = nans(n + PAD, T, dev)
    x[:n] = xin.to(dev)
    lib().call('sba_bert_gelu', code, p(x), n, stream())    # in place
    torch.cuda.synchronize()
    out_close(front(x, n, 'x'), R.gelu(xin), T, name_of('gelu', (n,), mode))


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('case', R.TANH_T_CASES, ids=cid)
def test_tanh_transpose(dev, case, mode):
    (B, L, C), _ = case
    code, T = MODES[mode]
    xin = R.tanh_t_inputs(B, L, C, T)
    x = on(dev, xin)
    y = nans(B * C * L + PAD, F32, dev)
    lib().call('sba_bert_tanh_transpose', code, p(x), p(y), B, L, C, stream())
    torch.cuda.synchronize()
    elem_close(front(y, B * C * L, 'y'), R.tanh_t(xin, B, L, C), name_of('tanh_transpose', (B, L, C), mode))


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('case', R.WORDS_BWD_CASES, ids=cid)
def test_words_head_bwd(dev, case, mode):
    (B, L, nef), _ = case
    code, T = MODES[mode]
    i = R.words_bwd_inputs(B, L, nef)
    dwords, y = on(dev, i.dwords), on(dev, i.y)
    dpre = nans(B * L * nef + PAD, T, dev)
    dbias, pre = prefilled(nef, R.TAG_DBIAS, dev)           # the kernel ADDS to dbias
    lib().call('sba_bert_words_head_bwd', code, p(dwords), p(y), p(dpre), p(dbias), B, L, nef, stream())
    torch.cuda.synchronize()
    ref = R.words_head_bwd(i.dwords, i.y)
    out_close(front(dpre, B * L * nef, 'dpre'), ref.dpre, T, name_of('words_head_bwd', (B, L, nef), mode + ' dpre'))
    added_close(dbias, nef, pre, ref.dbias, ref.dbias_abs, name_of('words_head_bwd', (B, L, nef), mode + ' dbias'))


@pytest.mark.parametrize('case', R.SENT_BWD_CASES, ids=cid)
def test_sent_head_bwd(dev, case):
    (B, C, nef), _ = case
    i = R.sent_bwd_inputs(B, C, nef)
    t = [on(dev, v) for v in (i.dsent, i.sent, i.pooled, i.cls, i.w_fc)]
    dpooled = nans(B * C + PAD, F32, dev)
    outs = {k: prefilled(n, tag, dev) for k, n, tag in (('dw_fc', nef * C, R.TAG_DWFC), ('db_fc', nef, R.TAG_DBFC),
                                                        ('dw_pool', C * C, R.TAG_DWP), ('db_pool', C, R.TAG_DBP))}
    lib().call('sba_bert_sent_head_bwd', *[p(v) for v in t], p(dpooled), *[p(outs[k][0]) for k in ('dw_fc', 'db_fc', 'dw_pool', 'db_pool')],
               B, C, nef, stream())
    torch.cuda.synchronize()
    got = front(dpooled, B * C, 'dpooled')
    # the second launch reads the dpooled the first one stored: its sums are judged on that
    ref = R.sent_head_bwd(i.dsent, i.sent, i.pooled, i.cls, i.w_fc, dpooled=got.view(B, C))
    elem_close(got, ref.dpooled, name_of('sent_head_bwd', (B, C, nef), 'dpooled'))
    for k, (buf, pre) in outs.items():
        added_close(buf, pre.numel(), pre, getattr(ref, k), getattr(ref, k + '_abs'), name_of('sent_head_bwd', (B, C, nef), k))


# ------------------------------------------------------------------ refusals
def test_refusals(dev):
    """every SBA_E_ARG condition of the two files: the call comes back refused and no output is written"""
    st = stream()
    i64 = torch.int64

    def ins(dt=F32):
        return torch.ones(BIG, dtype=dt, device=dev)

    def outs(dt=F32):
        return nans(BIG, dt, dev)

    def nulls(*keys):
        return [('%s = NULL' % k, {k: None}) for k in keys]

    def dims(*keys):
        return [('%s = 0' % k, {k: 0}) for k in keys] + [('%s = -1' % k, {k: -1}) for k in keys]
    lstm = [('Lout > T', dict(Lout=5)), ('H = 32', dict(H=32)), ('H = 96', dict(H=96)), ('H = 256', dict(H=256))]

    order = ['cap', 'lens', 'emb', 'w_ih', 'w_hh', 'b_ih', 'b_hh', 'h0', 'c0', 'gx', 'words', 'sent', 'B', 'T', 'Lout', 'ntoken',
             'ninput', 'H', 'st']
    for state in (False, True):
        b = dict(cap=torch.zeros(BIG, dtype=i64, device=dev), lens=torch.full((BIG,), 2, dtype=i64, device=dev), emb=ins(),
                 w_ih=ins(), w_hh=ins(), b_ih=ins(), b_hh=ins(), h0=ins() if state else None, c0=ins() if state else None,
                 gx=outs(), words=outs(), sent=outs(), B=2, T=4, Lout=4, ntoken=5, ninput=8, H=64, st=st)
        one = [('c0 = NULL, h0 given', dict(c0=None)), ('h0 = NULL, c0 given', dict(h0=None))] if state else \
            [('h0 without c0', dict(h0=b['emb'])), ('c0 without h0', dict(c0=b['emb']))]
        _refuse('sba_lstm_bidir_fwd', order, b, nulls('cap', 'lens', 'emb', 'w_ih', 'w_hh', 'b_ih', 'b_hh', 'gx', 'words', 'sent')
                + dims('B', 'T', 'Lout', 'ntoken', 'ninput') + lstm + one + [
                    ('ninput % 4 != 0', dict(ninput=6)), ('ninput = 2052: 8 rows x ninput x 4 bytes > 64 KB of LDS', dict(ninput=2052))],
                ['gx', 'words', 'sent'])

    order = ['gx', 'lens', 'w_hh', 'h0', 'c0', 'words', 'sent', 'gates', 'cs', 'hs', 'B', 'T', 'Lout', 'H', 'st']
    b = dict(gx=ins(), lens=torch.full((BIG,), 2, dtype=i64, device=dev), w_hh=ins(), h0=None, c0=None, words=outs(), sent=outs(),
             gates=outs(), cs=outs(), hs=outs(), B=2, T=4, Lout=4, H=128, st=st)
    _refuse('sba_lstm_recur_train', order, b, nulls('gx', 'lens', 'w_hh', 'words', 'sent', 'gates', 'cs', 'hs') + dims('B', 'T', 'Lout')
            + lstm + [('h0 without c0', dict(h0=b['gx'])), ('c0 without h0', dict(c0=b['gx']))], ['words', 'sent', 'gates', 'cs', 'hs'])

    order = ['lens', 'w_hh', 'h0', 'c0', 'gates', 'cs', 'hs', 'dwords', 'dsent', 'dG', 'hprev', 'B', 'T', 'Lout', 'H', 'st']
    b = dict(lens=torch.full((BIG,), 2, dtype=i64, device=dev), w_hh=ins(), h0=ins(), c0=ins(), gates=ins(), cs=ins(), hs=ins(),
             dwords=ins(), dsent=ins(), dG=outs(), hprev=outs(), B=2, T=4, Lout=4, H=64, st=st)
    _refuse('sba_lstm_recur_bwd', order, b, nulls('lens', 'w_hh', 'gates', 'cs', 'hs', 'dwords', 'dsent', 'dG', 'hprev')
            + dims('B', 'T', 'Lout') + lstm + [('c0 = NULL, h0 given', dict(c0=None)), ('h0 = NULL, c0 given', dict(h0=None))],
            ['dG', 'hprev'])

    bad_dt = [('unknown dtype', dict(dt=7)), ('binary16 y has no meaning here', dict(dt=2))]
    width = [('C % 64 != 0', dict(C=96)), ('C % 64 != 0', dict(C=32)), ('C > 1024', dict(C=1088))]
    for code, T in MODES.values():
        order = ['dt', 'tok', 'we', 'pe', 'te', 'gamma', 'beta', 'out', 'B', 'L', 'C', 'ntoken', 'eps', 'st']
        b = dict(dt=code, tok=torch.zeros(BIG, dtype=i64, device=dev), we=ins(), pe=ins(), te=ins(), gamma=ins(), beta=ins(),
                 out=outs(T), B=2, L=3, C=64, ntoken=5, eps=R.LN_EPS, st=st)
        _refuse('sba_bert_embed_ln', order, b, nulls('tok', 'we', 'pe', 'te', 'gamma', 'beta', 'out') + dims('B', 'L', 'C', 'ntoken')
                + width + bad_dt, ['out'])
        order = ['dt', 'x', 'res', 'gamma', 'beta', 'out', 'rows', 'C', 'eps', 'st']
        b = dict(dt=code, x=ins(T), res=ins(T), gamma=ins(), beta=ins(), out=outs(T), rows=5, C=64, eps=R.LN_EPS, st=st)
        _refuse('sba_bert_add_ln', order, b, nulls('x', 'res', 'gamma', 'beta', 'out') + dims('rows', 'C') + width + bad_dt, ['out'])
        order = ['dt', 'qkv', 'ctx', 'B', 'L', 'C', 'heads', 'st']
        b = dict(dt=code, qkv=ins(T), ctx=outs(T), B=2, L=3, C=128, heads=2, st=st)
        _refuse('sba_bert_attention', order, b, nulls('qkv', 'ctx') + dims('B', 'L', 'heads') + bad_dt + [
            ('L > 32', dict(L=33)), ('C != heads * 64', dict(C=64)), ('C != heads * 64', dict(C=192)), ('C != heads * 64', dict(heads=3))],
            ['ctx'])
        b = dict(dt=code, x=outs(T), n=100, st=st)          # in place: the buffer is the output
        _refuse('sba_bert_gelu', ['dt', 'x', 'n', 'st'], b, nulls('x') + dims('n') + bad_dt, ['x'])
        b = dict(dt=code, x=ins(T), y=outs(), B=2, L=3, C=5, st=st)
        _refuse('sba_bert_tanh_transpose', ['dt', 'x', 'y', 'B', 'L', 'C', 'st'], b, nulls('x', 'y') + dims('B', 'L', 'C') + bad_dt, ['y'])
        order = ['dt', 'dwords', 'words', 'dpre', 'dbias', 'B', 'L', 'nef', 'st']
        b = dict(dt=code, dwords=ins(), words=ins(), dpre=outs(T), dbias=outs(), B=2, L=3, nef=64, st=st)
        _refuse('sba_bert_words_head_bwd', order, b, nulls('dwords', 'words', 'dpre', 'dbias') + dims('B', 'L', 'nef') + bad_dt + [
            ('L > 32', dict(L=33)), ('nef % 64 != 0', dict(nef=96)), ('nef % 64 != 0', dict(nef=32))], ['dpre', 'dbias'])

    order = ['dsent', 'sent', 'pooled', 'cls', 'w_fc', 'dpooled', 'dw_fc', 'db_fc', 'dw_pool', 'db_pool', 'B', 'C', 'nef', 'st']
    b = dict(dsent=ins(), sent=ins(), pooled=ins(), cls=ins(), w_fc=ins(), dpooled=outs(), dw_fc=outs(), db_fc=outs(), dw_pool=outs(),
             db_pool=outs(), B=3, C=64, nef=128, st=st)
    _refuse('sba_bert_sent_head_bwd', order, b, nulls(*order[:10]) + dims('B', 'C', 'nef') + [
        ('B > 64', dict(B=65)), ('C % 64 != 0', dict(C=96)), ('nef % 64 != 0', dict(nef=96))], order[5:10])
