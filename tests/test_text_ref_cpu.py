"""tests/text_ref.py checked without a GPU, before a kernel of csrc/text.hip or csrc/bert.hip is judged by it.

(1) Every reference equals PyTorch in float64, to 1e-12 relative: the recurrence against torch.nn.LSTM(bidirectional=True)
    over pack_padded_sequence (gx is fed through an identity input projection, one block per direction, so that x.grad IS
    dG), the projection + recurrence against oracle/text_encoder.py, back-propagation through time composed with the three
    GEMMs of ops.LstmBidirTrainFn.backward against autograd of the module on (words * gw).sum() + (sent * gs).sum() with a
    non-zero (h0, c0); LayerNorm, attention, GELU, tanh-transpose against torch.nn.functional; both heads' backward against
    autograd of tanh(x W^T + b) and tanh(fc(tanh(pooler(cls)))).  Captions of (clamped) length 0, which PyTorch refuses,
    are held to the definition: words all zero, sent = h0, no saved row, no gradient.
(2) On every case of tests/test_text_kernels_gpu.py a plain float32 evaluation of the same formulas (text_ref with
    dtype = float32) stays at least 5 x inside the bound the GPU test uses for that output (INSIDE), so a failure on the GPU
    is the kernel's, not the bound's or the inputs'.  The GPU's own expf / tanhf / erff are not emulated.  A bf16 output is
    the f32 value rounded once: it sits AT the one-rounding floor, half of its bound (twice the floor), by construction --
    asserted as that, not as 5 x inside.
(3) Every wrong variant listed in text_ref's docstring exceeds the same bound by at least 10 x (OUTSIDE) on at least one
    case of its list: the bounds are not vacuous.
(4) The case lists reach every arm named in the GPU test's table.
"""
import pytest
import torch
import torch.nn.functional as F

import text_ref as R
from helpers import rel_l2
from oracle import text_encoder as TE

F64, F32, BF16 = R.F64, R.F32, R.BF16
TOL = 1e-12
INSIDE, OUTSIDE = 0.2, 10.0
cid = R.case_id


def same(got, ref, name=''):
    got, ref = got.detach().double(), ref.detach().double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    assert err <= TOL * max(1.0, float(ref.abs().max())), '%s: max err %.3e' % (name, err)


def show(name, ratios):
    print('%-72s %s' % (name, '  '.join('%s %.3g' % kv for kv in ratios.items())))
    return ratios


def inside(name, ratios, spare=INSIDE):
    for k, v in show(name, ratios).items():
        assert v <= spare, '%s: the float32 evaluation is at %.3f of the bound on %s' % (name, v, k)


def low_ratio(got32, ref):
    """a bf16 output: relative L2 over the bound of test_norm_kernels_gpu.low_close (twice the one-rounding floor)"""
    r, floor = rel_l2(got32.to(BF16).double(), ref), rel_l2(ref.to(BF16).double(), ref)
    return r / (2 * floor) if floor > 0 else (0.0 if r == 0 else float('inf'))       # (L = 1: ctx = v, already bf16)


# ------------------------------------------------------------------ (1) LSTM references against PyTorch
def block_identity(H, dtype=F64):
    """w_ih [2][4H][8H]: direction d reads columns [4H d, 4H (d + 1)) of x = gx[0] | gx[1]"""
    w = torch.zeros((2, 4 * H, 8 * H), dtype=dtype)
    w[0, :, :4 * H], w[1, :, 4 * H:] = torch.eye(4 * H, dtype=dtype), torch.eye(4 * H, dtype=dtype)
    return w


@pytest.mark.parametrize('c', R.RECUR_CASES, ids=cid)
def test_recurrence_and_bptt_are_torch_lstm(c):
    i = R.recur_inputs(c)
    B, T, H, Lout = c.B, c.T, c.H, c.Lout
    lens = R.clamp_lens(c.lens, T)
    f = R.lstm_recur(i.gx, i.w_hh, i.lens, i.state, T, Lout)
    g = R.lstm_bptt(f.gates, f.cs, f.hs, i.w_hh, i.lens, i.state, i.dwords, i.dsent, T, Lout)
    keep = [b for b in range(B) if lens[b] >= 1]
    x = torch.cat((i.gx[0], i.gx[1]), 1).view(B, T, 8 * H)[keep]
    zero = torch.zeros((2, 4 * H), dtype=F64)
    state = None if i.state is None else (i.state[0][:, keep], i.state[1][:, keep])
    t = R.torch_lstm(x, block_identity(H), i.w_hh.double(), zero, zero, [lens[b] for b in keep], state, Lout)
    same(f.words[keep], t.words, 'words'); same(f.sent[keep], t.sent, 'sent')
    a = R.torch_lstm_grads(t, i.dwords[keep], i.dsent[keep])
    rows = lambda v: v.view(2, B, T, -1)[:, keep]           # noqa: E731
    same(rows(g.dG), torch.stack((a.dx[:, :, :4 * H], a.dx[:, :, 4 * H:])), 'dG')
    same(rows(g.dG).reshape(2, -1, 4 * H).transpose(1, 2) @ rows(g.hprev).reshape(2, -1, H), a.dw_hh, 'dG^T hprev')
    same(rows(g.dG).sum((1, 2)), a.db_hh, 'sum dG')
    for b in range(B):                                      # the definition past (and at) a caption's end
        n = lens[b]
        assert float(f.words[b, :, n:].abs().max() if n < Lout else 0) == 0
        for d in range(2):
            past = slice(b * T + n, (b + 1) * T)
            assert not bool(f.written[d, past].any()) and bool(f.written[d, b * T:b * T + n].all())
            assert float(g.dG[d, past].abs().sum() + g.hprev[d, past].abs().sum() + f.gates[d, past].abs().sum()) == 0
            if n == 0:
                h0 = torch.zeros(H, dtype=F64) if i.state is None else i.state[0][d, b].double()
                assert torch.equal(f.sent[b, d * H:(d + 1) * H], h0)


@pytest.mark.parametrize('c', R.FWD_CASES, ids=cid)
def test_projection_and_recurrence_are_the_oracle(c):
    i = R.fwd_inputs(c)
    BT = c.B * c.T
    xp = R.lstm_xproj(i.captions, i.emb, i.w_ih, i.b_ih, i.b_hh)
    tok = i.captions.flatten().clone()
    assert int((tok < 0).sum()) == 1 and int((tok >= c.ntoken).sum()) == 1
    tok[(tok < 0) | (tok >= c.ntoken)] = 0
    x = F.embedding(tok, i.emb.double())
    for d in range(2):
        same(xp.gx[d], F.linear(x, i.w_ih[d].double(), (i.b_ih[d].double() + i.b_hh[d].double())), 'gx')
    for r, j in ((0, 0), (BT - 1, 4 * c.H - 1), (1, 5)):    # the sums of absolute summands, term by term
        want = sum(abs(float(x[r, k]) * float(i.w_ih[1, j, k])) for k in range(c.ninput)) + abs(float(i.b_ih[1, j])) + abs(float(i.b_hh[1, j]))
        assert abs(float(xp.gx_abs[1, r, j]) - want) <= 1e-12 * want
    assert bool((xp.gx_abs >= xp.gx.abs() - 1e-12).all())
    f = R.lstm_recur(xp.gx, i.w_hh, i.lens, None, c.T, c.Lout)
    P = {'encoder.weight': i.emb.numpy()}
    for d, suf in enumerate(('', '_reverse')):
        P.update({'rnn.weight_ih_l0' + suf: i.w_ih[d].numpy(), 'rnn.weight_hh_l0' + suf: i.w_hh[d].numpy(),
                  'rnn.bias_ih_l0' + suf: i.b_ih[d].numpy(), 'rnn.bias_hh_l0' + suf: i.b_hh[d].numpy()})
    ow, osent = TE.rnn_encoder_forward(P, tok.view(c.B, c.T).numpy(), R.clamp_lens(c.lens, c.T), max_len=c.Lout)
    same(f.words, torch.from_numpy(ow), 'words'); same(f.sent, torch.from_numpy(osent), 'sent')


@pytest.mark.parametrize('c', R.E2E_CASES, ids=cid)
def test_bptt_with_the_three_gemms_is_autograd(c):
    i, f, p = R.e2e_reference(c)
    t = R.torch_lstm(i.x, i.w_ih, i.w_hh, i.b_ih, i.b_hh, i.lens, i.state, c.T)
    same(f.words, t.words, 'words'); same(f.sent, t.sent, 'sent')
    a = R.torch_lstm_grads(t, i.gw, i.gs)
    same(p.dx, a.dx.view(c.B * c.T, c.ninput), 'dx'); same(p.dw_ih, a.dw_ih, 'dw_ih'); same(p.dw_hh, a.dw_hh, 'dw_hh')
    same(p.db, a.db, 'db (b_ih)'); same(p.db, a.db_hh, 'db (b_hh)')
    for k in ('dx', 'dw_ih', 'dw_hh', 'db'):
        assert bool((getattr(p, k + '_abs') >= getattr(p, k).abs() - 1e-12).all())
    # float32 autograd of the same module against the bound of the GPU's end-to-end test
    t32 = R.torch_lstm(i.x, i.w_ih, i.w_hh, i.b_ih, i.b_hh, i.lens, i.state, c.T, dtype=F32)
    a32 = R.torch_lstm_grads(t32, i.gw, i.gs)
    inside('LstmBidirTrainFn %s' % cid(c), {
        'dx': R.sums_ratio(a32.dx.view(c.B * c.T, c.ninput), p.dx, p.dx_abs), 'dw_ih': R.sums_ratio(a32.dw_ih, p.dw_ih, p.dw_ih_abs),
        'dw_hh': R.sums_ratio(a32.dw_hh, p.dw_hh, p.dw_hh_abs), 'db': R.sums_ratio(a32.db, p.db, p.db_abs)})


# ------------------------------------------------------------------ (1) BERT references against PyTorch
def test_layer_norms_are_torch():
    for (B, L, C), _ in R.EMBED_CASES:
        i = R.embed_inputs(B, L, C)
        tok = i.tok.clone()
        tok[(tok < 0) | (tok >= i.ntoken)] = 0
        pos = torch.arange(B * L) % L
        v = F.embedding(tok, i.we.double()) + F.embedding(pos, i.pe.double()) + i.te[0].double()
        want = F.layer_norm(v, (C,), i.gamma.double(), i.beta.double(), R.LN_EPS)
        same(R.embed_ln(i.tok, i.we, i.pe, i.te, i.gamma, i.beta, L), want, 'embed_ln')
        if B >= 2:
            assert int(pos[L]) == 0 and not torch.equal(pos, torch.arange(B * L) // L)
    for (rows, C, kind), _ in R.ADD_LN_CASES:
        i = R.add_ln_inputs(rows, C, kind)
        want = F.layer_norm(i.x.double() + i.res.double(), (C,), i.gamma.double(), i.beta.double(), R.LN_EPS)
        got = R.add_ln(i.x, i.res, i.gamma, i.beta)
        if kind == 'const':                                 # (F.layer_norm's own rounding decides row 2 there)
            assert torch.equal(got[2], i.beta.double())
            keep = [0, 1, 3, 4]
            got, want = got[keep], want[keep]
        same(got, want, 'add_ln')
        if kind == 'offset':
            s = i.x.double() + i.res.double()
            assert 3.0 < float((s.mean(1) / s.std(1)).min())


def test_attention_is_softmax_and_matmul():
    for (B, L, heads, big), _ in R.ATTN_CASES:
        qkv = R.attn_inputs(B, L, heads, big).double()
        C = 64 * heads
        want = torch.empty((B * L, C), dtype=F64)
        top, low = 0.0, 0.0
        for b in range(B):
            for h in range(heads):
                q, k, v = (qkv[b * L:(b + 1) * L, j * C + h * 64:j * C + (h + 1) * 64] for j in range(3))
                s = q @ k.t() / 8
                top, low = max(top, float(s.max())), min(low, float(s.min()))
                want[b * L:(b + 1) * L, h * 64:(h + 1) * 64] = torch.softmax(s, 1) @ v
        same(R.attention(qkv, B, L, heads), want, 'ctx')
        if big:
            assert abs(top - big) < 1e-3 * big and low < -0.6 * big


def test_gelu_and_tanh_transpose_are_torch():
    for n, _ in R.GELU_CASES[:3]:
        x = R.gelu_inputs(n)
        same(R.gelu(x), F.gelu(x.double()), 'gelu')
    x = R.gelu_inputs(257)
    assert [float(v) for v in x[3:7]] == [0.0, -0.0, 10.0, -10.0] and bool(torch.signbit(x[4]))
    B, L, C = 2, 7, 5
    x = R.tanh_t_inputs(B, L, C)
    y = R.tanh_t(x, B, L, C)
    assert y.shape == (B, C, L)
    for b, c, l in ((0, 0, 0), (1, 4, 6), (1, 2, 3)):
        assert float(y[b, c, l]) == float(torch.tanh(x[b * L + l, c].double()))


def test_heads_backward_is_autograd():
    B, L, nef, C = 3, 7, 64, 128
    x = R.fill.unit((B * L, C), 1).double()
    w = (R.fill.unit((nef, C), 2) / C ** 0.5).double().requires_grad_(True)
    b = (0.1 * R.fill.unit((nef,), 3)).double().requires_grad_(True)
    pre = F.linear(x, w, b).requires_grad_(True)
    pre.retain_grad()
    words = torch.tanh(pre).view(B, L, nef).permute(0, 2, 1)            # [B][nef][L]
    dwords = R.fill.unit((B, nef, L), 4).double()
    (words * dwords).sum().backward()
    r = R.words_head_bwd(dwords, words)
    same(r.dpre, pre.grad, 'dpre'); same(r.dbias, b.grad, 'dbias')
    same(r.dbias_abs, (dwords * (1 - words.detach() ** 2)).abs().sum((0, 2)), 'dbias_abs')
    c = R.sent_head_chain(B, C, nef)
    leaves = [t.clone().requires_grad_(True) for t in (c.w_pool, c.b_pool, c.w_fc, c.b_fc)]
    pooled = torch.tanh(F.linear(c.cls, leaves[0], leaves[1]))
    pooled.retain_grad()
    sent = torch.tanh(F.linear(pooled, leaves[2], leaves[3]))
    (sent * c.dsent).sum().backward()
    r = R.sent_head_bwd(c.dsent, sent, pooled, c.cls, c.w_fc)
    same(r.dpooled, pooled.grad, 'dpooled'); same(r.dw_pool, leaves[0].grad, 'dw_pool'); same(r.db_pool, leaves[1].grad, 'db_pool')
    same(r.dw_fc, leaves[2].grad, 'dw_fc'); same(r.db_fc, leaves[3].grad, 'db_fc')
    same(R.sent_head_bwd(c.dsent, sent, pooled, c.cls, c.w_fc, dpooled=r.dpooled).dw_pool, r.dw_pool, 'dw_pool on a given dpooled')
    g = (c.dsent * (1 - sent.detach() ** 2)).abs()
    h = (r.dpooled * (1 - pooled.detach() ** 2)).abs()
    same(r.dw_fc_abs, g.t() @ pooled.detach().abs(), 'dw_fc_abs'); same(r.db_fc_abs, g.sum(0), 'db_fc_abs')
    same(r.dw_pool_abs, h.t() @ c.cls.abs(), 'dw_pool_abs'); same(r.db_pool_abs, h.sum(0), 'db_pool_abs')


# ------------------------------------------------------------------ (2) + (3) LSTM: float32 inside, wrong variants outside
def recur_ratios(got, ref):
    w = ref.written
    r = {k: R.elem_ratio(getattr(got, k), getattr(ref, k)) for k in ('words', 'sent')}
    r.update({k: R.elem_ratio(getattr(got, k)[w], getattr(ref, k)[w]) for k in ('gates', 'cs', 'hs')})
    # a row written that should not be (or the reverse) counts as far outside
    r['rows'] = 0.0 if torch.equal(got.written, w) else 1e9
    return r


def bptt_ratios(got, ref):
    return {k: R.elem_ratio(getattr(got, k), getattr(ref, k)) for k in ('dG', 'hprev')}


def emulate_recur(i, c, mut=()):
    f32 = R.lstm_recur(i.gx, i.w_hh, i.lens, i.state, c.T, c.Lout, dtype=F32, mut=mut)
    return f32, recur_ratios(f32, R.lstm_recur(i.gx, i.w_hh, i.lens, i.state, c.T, c.Lout))


def emulate_bptt(i, c, mut=()):
    """on the tensors the float32 forward saved, as the GPU test runs the kernel on what the training kernel saved"""
    s = R.lstm_recur(i.gx, i.w_hh, i.lens, i.state, c.T, c.Lout, dtype=F32)
    args = (s.gates, s.cs, s.hs, i.w_hh, i.lens, i.state, i.dwords, i.dsent, c.T, c.Lout)
    return bptt_ratios(R.lstm_bptt(*args, dtype=F32, mut=mut), R.lstm_bptt(*args))


@pytest.mark.parametrize('c', R.RECUR_CASES, ids=cid)
def test_float32_recurrence_and_bptt_are_inside(c):
    i = R.recur_inputs(c)
    inside('recurrence %s' % cid(c), emulate_recur(i, c)[1])
    inside('BPTT %s' % cid(c), emulate_bptt(i, c))


@pytest.mark.parametrize('c', R.FWD_CASES, ids=cid)
def test_float32_forward_is_inside(c):
    i = R.fwd_inputs(c)
    ref = R.lstm_xproj(i.captions, i.emb, i.w_ih, i.b_ih, i.b_hh)
    gx32 = R.lstm_xproj(i.captions, i.emb, i.w_ih, i.b_ih, i.b_hh, dtype=F32).gx
    inside('projection %s' % cid(c), {'gx': R.sums_ratio(gx32, ref.gx, ref.gx_abs)})
    i.gx = gx32                                             # the recurrence is judged on the gx it was given
    inside('recurrence %s' % cid(c), emulate_recur(i, c)[1])


def worst_over(cases, ratios_of):
    worst = {}
    for c in cases:
        for k, v in ratios_of(c).items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


LOUT_CASES = [c for c in R.RECUR_CASES if c.Lout < max(R.clamp_lens(c.lens, c.T))]
STATE_CASES = [c for c in R.RECUR_CASES if c.state]
LSTM_MUTATIONS = [('no_dsent', 'bptt', R.RECUR_CASES), ('rev_tp', 'bptt', R.RECUR_CASES), ('drop_term', 'bptt', R.RECUR_CASES),
                  ('no_state', 'bptt', STATE_CASES), ('dwords_past', 'bptt', LOUT_CASES), ('stop_lout', 'recur', LOUT_CASES),
                  ('sent_rev', 'recur', R.RECUR_CASES)]


@pytest.mark.parametrize('mut,which,cases', LSTM_MUTATIONS, ids=lambda v: v if isinstance(v, str) and v not in ('bptt', 'recur') else '')
def test_lstm_mutations_are_outside(mut, which, cases):
    assert cases
    fn = (lambda c: emulate_bptt(R.recur_inputs(c), c, {mut})) if which == 'bptt' else (lambda c: emulate_recur(R.recur_inputs(c), c, {mut})[1])
    worst = show('%s: worst over its %d cases' % (mut, len(cases)), worst_over(cases, fn))
    assert max(worst.values()) >= OUTSIDE, mut


def test_projection_mutation_is_outside():
    def ratios(c):
        i = R.fwd_inputs(c)
        ref = R.lstm_xproj(i.captions, i.emb, i.w_ih, i.b_ih, i.b_hh)
        return {'gx': R.sums_ratio(R.lstm_xproj(i.captions, i.emb, i.w_ih, i.b_ih, i.b_hh, dtype=F32, mut={'drop_k'}).gx, ref.gx, ref.gx_abs)}
    for c in R.FWD_CASES:                                   # at EVERY ninput, 2048 included
        assert show('drop_k %s' % cid(c), ratios(c))['gx'] >= OUTSIDE


# ------------------------------------------------------------------ (2) + (3) BERT
def out_ratio(got32, ref, T):
    return R.elem_ratio(got32, ref) if T == F32 else low_ratio(got32, ref)


def spare_of(T):
    return INSIDE if T == F32 else 0.55                     # bf16: one rounding of the f32 value = the floor = half the bound


@pytest.mark.parametrize('T', [F32, BF16], ids=['f32', 'bf16'])
def test_float32_bert_forward_is_inside(T):
    for (B, L, C), _ in R.EMBED_CASES:
        i = R.embed_inputs(B, L, C)
        args = (i.tok, i.we, i.pe, i.te, i.gamma, i.beta, L)
        inside('embed_ln %s' % ((B, L, C),), {'out': out_ratio(R.embed_ln(*args, dtype=F32), R.embed_ln(*args), T)}, spare_of(T))
    for (rows, C, kind), _ in R.ADD_LN_CASES:
        i = R.add_ln_inputs(rows, C, kind, T)
        args = (i.x, i.res, i.gamma, i.beta)
        got = R.add_ln(*args, dtype=F32)
        inside('add_ln %s' % ((rows, C, kind),), {'out': out_ratio(got, R.add_ln(*args), T)}, spare_of(T))
        if kind == 'const' and T == F32:
            assert torch.equal(got[2], i.beta), 'x + res exactly constant: float32 gives beta exactly'
    for (B, L, heads, big), _ in R.ATTN_CASES:
        qkv = R.attn_inputs(B, L, heads, big, T)
        inside('attention %s' % ((B, L, heads, big),),
               {'ctx': out_ratio(R.attention(qkv, B, L, heads, dtype=F32), R.attention(qkv, B, L, heads), T)}, spare_of(T))
    for n, _ in R.GELU_CASES:
        x = R.gelu_inputs(n, T)
        inside('gelu %d' % n, {'y': out_ratio(R.gelu(x, dtype=F32), R.gelu(x), T)}, spare_of(T))
    for (B, L, C), _ in R.TANH_T_CASES:
        x = R.tanh_t_inputs(B, L, C, T)                     # (the output is f32 for either input type)
        inside('tanh_t %s' % ((B, L, C),), {'y': R.elem_ratio(R.tanh_t(x, B, L, C, dtype=F32), R.tanh_t(x, B, L, C))})


def added(n, tag, s32):
    """(stored - prefill) of an f32 output the kernel adds its sum to, as the GPU test forms it"""
    from test_norm_kernels_gpu import prefilled
    buf, pre = prefilled(n, tag, torch.device('cpu'))
    return (buf[:n] + s32.flatten()).double() - pre


def test_float32_heads_backward_is_inside():
    for (B, L, nef), _ in R.WORDS_BWD_CASES:
        i = R.words_bwd_inputs(B, L, nef)
        ref, e = R.words_head_bwd(i.dwords, i.y), R.words_head_bwd(i.dwords, i.y, dtype=F32)
        inside('words head %s' % ((B, L, nef),), {'dpre': R.elem_ratio(e.dpre, ref.dpre),
                                                  'dbias': R.sums_ratio(added(nef, R.TAG_DBIAS, e.dbias), ref.dbias, ref.dbias_abs)})
        inside('words head %s bf16' % ((B, L, nef),), {'dpre': low_ratio(e.dpre, ref.dpre)}, 0.55)
    for (B, C, nef), _ in R.SENT_BWD_CASES:
        i = R.sent_bwd_inputs(B, C, nef)
        args = (i.dsent, i.sent, i.pooled, i.cls, i.w_fc)
        e = R.sent_head_bwd(*args, dtype=F32)
        ref = R.sent_head_bwd(*args, dpooled=e.dpooled)     # the second stage on the dpooled the first one stored
        r = {'dpooled': R.elem_ratio(e.dpooled, ref.dpooled)}
        for k, tag in (('dw_fc', R.TAG_DWFC), ('db_fc', R.TAG_DBFC), ('dw_pool', R.TAG_DWP), ('db_pool', R.TAG_DBP)):
            r[k] = R.sums_ratio(added(getattr(ref, k).numel(), tag, getattr(e, k)), getattr(ref, k), getattr(ref, k + '_abs'))
        inside('sentence head %s' % ((B, C, nef),), r)


def test_bert_mutations_are_outside():
    def worst(name, ratios):
        v = max(ratios)
        print('%-12s worst over its %d cases: %.3g x the bound' % (name, len(ratios), v))
        assert v >= OUTSIDE, name
    r = []
    for (B, L, C), _ in R.EMBED_CASES:
        i = R.embed_inputs(B, L, C)
        args = (i.tok, i.we, i.pe, i.te, i.gamma, i.beta, L)
        r.append((R.elem_ratio(R.embed_ln(*args, dtype=F32, mut={'var_c1'}), R.embed_ln(*args)),
                  R.elem_ratio(R.embed_ln(*args, dtype=F32, mut={'pos_div'}), R.embed_ln(*args))))
    worst('var_c1', [a for a, _ in r]); worst('pos_div', [b for _, b in r])
    # var_c1 is 1 / (2C) of the value: outside at EVERY width, barely so at C = 1024
    assert all(a > 1.0 for a, _ in r)
    worst('var_c1 add_ln', [R.elem_ratio(R.add_ln(i.x, i.res, i.gamma, i.beta, dtype=F32, mut={'var_c1'}), R.add_ln(i.x, i.res, i.gamma, i.beta))
                            for i in (R.add_ln_inputs(rows, C, kind) for (rows, C, kind), _ in R.ADD_LN_CASES)])
    worst('no_scale', [R.elem_ratio(R.attention(q, B, L, h, dtype=F32, mut={'no_scale'}), R.attention(q, B, L, h))
                       for (B, L, h, big), _ in R.ATTN_CASES if L > 1 for q in [R.attn_inputs(B, L, h, big)]])
    worst('tanh', [R.elem_ratio(R.gelu(x, dtype=F32, mut={'tanh'}), R.gelu(x)) for n, _ in R.GELU_CASES for x in [R.gelu_inputs(n)]])
    rr = []
    for (B, L, nef), _ in R.WORDS_BWD_CASES:
        i = R.words_bwd_inputs(B, L, nef)
        ref = R.words_head_bwd(i.dwords, i.y)
        rr.append(R.sums_ratio(R.words_head_bwd(i.dwords, i.y, dtype=F32, mut={'miss_last'}).dbias, ref.dbias, ref.dbias_abs))
    worst('miss_last', rr)
    assert min(rr) >= OUTSIDE                               # at every case: one of at most 384 terms of a sum of like terms
    # a softmax without the max subtraction, in f32: still finite at logits of 50 (exp(50) = 5e21), inf / inf at 100
    for top, finite in ((50.0, True), (100.0, False)):
        assert ((2, 7, 2, top) in [s for s, _ in R.ATTN_CASES])
        qkv = R.attn_inputs(2, 7, 2, top)
        q, k = (t.permute(0, 2, 1, 3) for t in qkv.view(2, 7, 3, 2, 64).unbind(2)[:2])
        e = torch.exp(q @ k.transpose(2, 3) * 0.125)
        assert bool(torch.isfinite(e / e.sum(-1, keepdim=True)).all()) == finite


# ------------------------------------------------------------------ (4) the case lists reach every arm
def test_case_lists_reach_every_arm():
    rc = R.RECUR_CASES
    lens = lambda c: R.clamp_lens(c.lens, c.T)              # noqa: E731
    assert all(c.T <= 18 and len(c.lens) == c.B for c in rc)
    for H in (64, 128):
        mine = [c for c in rc if c.H == H]
        assert {1, 5} <= {c.B for c in mine}
        assert any(c.state for c in mine) and any(not c.state for c in mine)
        assert any(c.Lout == c.T for c in mine)
        assert any(c.Lout < max(lens(c)) for c in mine), 'Lout below a caption length at H = %d' % H
        assert any(c.Lout < max(lens(c)) and c.state for c in rc)
    assert any(c.Lout == max(lens(c)) < c.T for c in rc)
    raw = [n for c in rc for n in c.lens]
    assert {1, 0, -3} <= set(raw) and any(n == c.T for c in rc for n in c.lens) and any(n == c.T + 4 for c in rc for n in c.lens)
    assert any(1 < n < c.T for c in rc for n in c.lens)
    fc = R.FWD_CASES
    assert {c.ninput for c in fc} == {4, 300, 2048} and all(c.ninput % 4 == 0 and 8 * c.ninput * 4 <= 64 * 1024 for c in fc)
    assert any(c.B * c.T == 15 for c in fc) and any(c.B * c.T % 8 == 0 for c in fc) and any(c.B == 1 for c in fc)
    assert {-(-4 * c.H // 256) for c in fc} == {1, 2}
    assert any(c.Lout < max(lens(c)) for c in fc) and any(0 in lens(c) for c in fc) and any(c.state for c in fc)
    assert [(c.B, c.T, c.ninput, c.H) for c in R.E2E_CASES] == [(4, 9, 12, 64), (3, 6, 300, 128)]
    for cases in (R.EMBED_CASES, R.ADD_LN_CASES):
        shapes = [s for s, _ in cases]
        rows = [s[0] * s[1] if cases is R.EMBED_CASES else s[0] for s in shapes]
        assert {1, 5, 21} <= set(rows) and any(r % 4 == 0 for r in rows) and any(r % 4 for r in rows)
        assert {s[2] if cases is R.EMBED_CASES else s[1] for s in shapes} == {64, 768, 1024}          # per = 1, 12, 16
    assert any(B >= 2 and L > 1 for (B, L, C), _ in R.EMBED_CASES)
    assert {'offset', 'const'} <= {k for (_, _, k), _ in R.ADD_LN_CASES}
    assert [s[:3] for s, _ in R.ATTN_CASES if not s[3]] == [(1, 1, 1), (2, 7, 2), (3, 20, 12), (1, 32, 12)] and {50.0, 100.0} <= {s[3] for s, _ in R.ATTN_CASES}
    assert [n for n, _ in R.GELU_CASES] == [1, 255, 257, 4096 * 256 + 3]
    assert [s for s, _ in R.TANH_T_CASES] == [(1, 1, 1), (2, 7, 5), (3, 20, 256), (8, 32, 4100)] and 8 * 32 * 4100 > 4096 * 256
    assert [s for s, _ in R.WORDS_BWD_CASES] == [(1, 1, 64), (3, 7, 128), (2, 32, 256), (32, 12, 256)]
    assert [s for s, _ in R.SENT_BWD_CASES] == [(1, 64, 64), (3, 128, 64), (64, 64, 128), (5, 768, 256)]
    for cases in (rc, fc, R.EMBED_CASES, R.ADD_LN_CASES, R.ATTN_CASES, R.GELU_CASES, R.TANH_T_CASES, R.WORDS_BWD_CASES, R.SENT_BWD_CASES):
        assert all(isinstance(c[-1], str) and c[-1] for c in cases), 'every case names the arm it reaches'
