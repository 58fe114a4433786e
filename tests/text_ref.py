"""Float64 references of the text-encoder entry points of csrc/text.hip (the bidirectional LSTM of RNN_ENCODER, model.py:75-159,
forward and back-propagation through time) and csrc/bert.hip (the pieces between BertEncoder's dense layers,
model_bert.py:161-189, and the backward of its two heads), written from the formulas of the layers (torch.nn.LSTM's
published cell equations over packed sequences, LayerNorm, softmax attention, erf GELU, tanh), not from the kernels.
tests/test_text_ref_cpu.py checks every function against float64 PyTorch; tests/test_text_kernels_gpu.py judges the kernels
by them.

The LSTM references are per kernel -- the input projection, the recurrence on a GIVEN gx, back-propagation through time on
GIVEN saved gates / cs / hs -- so that each kernel is judged on its own f32 inputs and no error is carried from the kernel
before it.  Every argument is converted to `dtype` (float64; float32 gives the plain f32 evaluation of the same formulas
that test_text_ref_cpu.py holds against the bounds); every result has that type.  Dot-product results come with the sum
of the ABSOLUTE summands of every element (`*_abs`).  For 16-bit storage the caller passes the rounded inputs.

`mut` names a deliberately WRONG variant of a reference (test_text_ref_cpu.py: each is outside the bounds):
    no_dsent     BPTT: d sent is not added at the last processed step
    rev_tp       BPTT: the reverse direction takes t - 1, not t + 1, as the step processed before
    drop_term    BPTT: the last term of W_hh^T . dgates is left out
    no_state     BPTT: h0 / c0 ignored in the first step's cp / hp
    dwords_past  BPTT: d words read at t >= Lout (the flat index runs into the next channel's row)
    stop_lout    recurrence: stops at min(len, Lout), not at len
    sent_rev     recurrence: sent of the reverse direction taken at t = len - 1 (its FIRST processed step)
    drop_k       projection: the last 4 columns of ninput take no part
    var_c1       LayerNorm: variance over C - 1
    pos_div      embedding: position index row / L
    no_scale     attention: no 1 / 8
    tanh         GELU: the tanh approximation
    miss_last    words head: dbias misses l = L - 1

The second half of the file holds the cases of the GPU tests, each with the arm it reaches named beside it, and their
inputs: closed-form (oracle.fill), no random state.
"""
import math
from collections import namedtuple
from types import SimpleNamespace as NS

import torch

from oracle import fill

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
RTOL, ATOL = 2e-4, 2e-5         # elementwise f32 outputs (test_kernels_gpu.tol(torch.float32))
C_SUM = 1e-5                    # sums: |error| <= C_SUM x the float64 sum of the absolute summands
LN_EPS = 1e-12                  # BertLayerNorm
OFFSET = 4.0                    # |mean| / std of the offset rows (test_norm_kernels_gpu.OFFSET)


def _c(t, dt):
    return None if t is None else t.detach().to(dt)


def clamp_lens(lens, T):
    """the kernels' contract: a length below 0 counts as 0, one above T as T"""
    return [min(max(int(n), 0), T) for n in lens]


def elem_ratio(got, ref):
    """worst |error| / (ATOL + RTOL |ref|): what test_norm_kernels_gpu.elem_close asserts to be <= 1"""
    got, ref = got.detach().double().flatten(), ref.detach().double().flatten()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(((got - ref).abs() / (ATOL + RTOL * ref.abs())).max()) if ref.numel() else 0.0


def sums_ratio(got, ref, ref_abs):
    """worst |error| / (C_SUM x sum |summands|): what test_norm_kernels_gpu.sums_close asserts to be <= 1"""
    got, ref, ref_abs = (t.detach().double().flatten() for t in (got, ref, ref_abs))
    assert got.shape == ref.shape == ref_abs.shape, (got.shape, ref.shape)
    return float(((got - ref).abs() / (C_SUM * ref_abs.clamp(min=1e-30))).max())


# ------------------------------------------------------------------ LSTM: input projection
def lstm_xproj(captions, emb, w_ih, b_ih, b_hh, dtype=F64, mut=()):
    """captions [B][T] int64, emb [ntoken][ninput], w_ih [2][4H][ninput], b_ih / b_hh [2][4H] ->
    gx [2][B*T][4H] = W_ih[dir] . emb[token] + b_ih[dir] + b_hh[dir] and gx_abs; a token id outside [0, ntoken) reads row 0
    (the kernel's stated contract; nn.Embedding would raise).  x [B*T][ninput] = the gathered rows."""
    emb, w_ih, b_ih, b_hh = (_c(t, dtype) for t in (emb, w_ih, b_ih, b_hh))
    ntoken, ninput = emb.shape
    tok = captions.detach().flatten().clone().long()
    tok[(tok < 0) | (tok >= ntoken)] = 0
    x = emb[tok]
    K = ninput - 4 if 'drop_k' in mut else ninput
    gx = torch.einsum('rk,djk->drj', x[:, :K], w_ih[:, :, :K]) + (b_ih + b_hh)[:, None, :]
    gx_abs = torch.einsum('rk,djk->drj', x[:, :K].abs(), w_ih[:, :, :K].abs()) + (b_ih.abs() + b_hh.abs())[:, None, :]
    return NS(gx=gx, gx_abs=gx_abs, x=x)


# ------------------------------------------------------------------ LSTM: recurrence over packed sequences
def lstm_recur(gx, w_hh, cap_lens, state, T, Lout, dtype=F64, mut=()):
    """gx [2][B*T][4H] (gate order i | f | g | o), w_hh [2][4H][H], cap_lens [B] (clamped to [0, T]), state = None or
    (h0, c0) [2][B][H].  The forward direction runs t = 0 .. len - 1, the reverse direction t = len - 1 .. 0.
    Returns words [B][2H][Lout] (exact zeros past len, written for t < Lout only), sent [B][2H] (the state after the last
    processed step; h0 at len = 0), gates [2][B*T][4H] (AFTER the nonlinearities), cs, hs [2][B*T][H] and
    written [2][B*T] (bool: the rows t < len; the others are zero here and not the kernels' to write)."""
    gx, w_hh = _c(gx, dtype), _c(w_hh, dtype)
    H = w_hh.shape[2]
    B = gx.shape[1] // T
    lens = clamp_lens(cap_lens, T)
    words, sent = torch.zeros((B, 2 * H, Lout), dtype=dtype), torch.zeros((B, 2 * H), dtype=dtype)
    gates = torch.zeros((2, B * T, 4 * H), dtype=dtype)
    cs, hs = torch.zeros((2, B * T, H), dtype=dtype), torch.zeros((2, B * T, H), dtype=dtype)
    written = torch.zeros((2, B * T), dtype=torch.bool)
    for d in range(2):
        for b in range(B):
            n = min(lens[b], Lout) if 'stop_lout' in mut else lens[b]
            h = torch.zeros(H, dtype=dtype) if state is None else _c(state[0][d, b], dtype)
            c = torch.zeros(H, dtype=dtype) if state is None else _c(state[1][d, b], dtype)
            first = h
            for s in range(n):
                t = s if d == 0 else n - 1 - s
                a = gx[d, b * T + t] + w_hh[d] @ h
                i, f = torch.sigmoid(a[:H]), torch.sigmoid(a[H:2 * H])
                g, o = torch.tanh(a[2 * H:3 * H]), torch.sigmoid(a[3 * H:])
                c = f * c + i * g
                h = o * torch.tanh(c)
                gates[d, b * T + t], cs[d, b * T + t], hs[d, b * T + t] = torch.cat((i, f, g, o)), c, h
                written[d, b * T + t] = True
                if t < Lout:
                    words[b, d * H:(d + 1) * H, t] = h
                if s == 0:
                    first = h
            sent[b, d * H:(d + 1) * H] = first if ('sent_rev' in mut and d == 1) else h
    return NS(words=words, sent=sent, gates=gates, cs=cs, hs=hs, written=written)


# ------------------------------------------------------------------ LSTM: back-propagation through time
def lstm_bptt(gates, cs, hs, w_hh, cap_lens, state, dwords, dsent, T, Lout, dtype=F64, mut=()):
    """From the SAVED gates [2][B*T][4H], cs, hs [2][B*T][H] (rows t >= len are never read), d words [B][2H][Lout] and
    d sent [B][2H]: dG [2][B*T][4H], the gradient at the gate PRE-activations, and hprev [2][B*T][H], the hidden state
    each step started from; rows t >= len are zero here (the caller of the kernel clears them; the kernel leaves them).
        dh_t = d words[:, t] (t < Lout) + d sent (last processed step) + W_hh^T . dgates(the step processed AFTER t)
        dc_t = dh_t o (1 - tanh(c_t)^2) + dc(after) f(after)
        di = dc g i (1 - i),  df = dc c_before f (1 - f),  dg = dc i (1 - g^2),  do = dh tanh(c) o (1 - o)"""
    gates, cs, hs, w_hh, dwords, dsent = (_c(t, dtype) for t in (gates, cs, hs, w_hh, dwords, dsent))
    H = w_hh.shape[2]
    B = gates.shape[1] // T
    lens = clamp_lens(cap_lens, T)
    dG, hprev = torch.zeros((2, B * T, 4 * H), dtype=dtype), torch.zeros((2, B * T, H), dtype=dtype)
    flat = dwords.flatten()
    use_state = state is not None and 'no_state' not in mut
    for d in range(2):
        for b in range(B):
            n = lens[b]
            dh_rec, dc_next = torch.zeros(H, dtype=dtype), torch.zeros(H, dtype=dtype)
            for s in range(n - 1, -1, -1):
                t = s if d == 0 else n - 1 - s
                tp = t - 1 if (d == 0 or 'rev_tp' in mut) else t + 1         # the step processed before this one
                dh = dh_rec.clone()
                if t < Lout:
                    dh = dh + dwords[b, d * H:(d + 1) * H, t]
                elif 'dwords_past' in mut:
                    idx = ((b * 2 * H + d * H + torch.arange(H)) * Lout + t) % flat.numel()
                    dh = dh + flat[idx]
                if s == n - 1 and 'no_dsent' not in mut:
                    dh = dh + dsent[b, d * H:(d + 1) * H]
                r = b * T + t
                i, f, g, o = gates[d, r, :H], gates[d, r, H:2 * H], gates[d, r, 2 * H:3 * H], gates[d, r, 3 * H:]
                if s == 0:
                    cp = _c(state[1][d, b], dtype) if use_state else torch.zeros(H, dtype=dtype)
                    hp = _c(state[0][d, b], dtype) if use_state else torch.zeros(H, dtype=dtype)
                else:
                    cp, hp = cs[d, b * T + tp], hs[d, b * T + tp]
                tc = torch.tanh(cs[d, r])
                dc = dh * o * (1 - tc * tc) + dc_next
                dgate = torch.cat((dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)))
                dG[d, r], hprev[d, r] = dgate, hp
                dc_next = dc * f
                dh_rec = w_hh[d][:-1].t() @ dgate[:-1] if 'drop_term' in mut else w_hh[d].t() @ dgate
    return NS(dG=dG, hprev=hprev)


def lstm_param_grads(dG, hprev, x, w_ih):
    """the three GEMMs (and the bias sum) of ops.LstmBidirTrainFn.backward, and the sums of their absolute summands:
    dw_ih [2][4H][ninput] = dG^T x, dw_hh [2][4H][H] = dG^T hprev, db [2][4H] = sum dG, dx [B*T][ninput] = sum_dir dG W_ih"""
    dG, hprev, x, w_ih = (_c(t, F64) for t in (dG, hprev, x, w_ih))
    dGt, aGt = dG.transpose(1, 2), dG.abs().transpose(1, 2)
    return NS(dw_ih=dGt @ x, dw_hh=dGt @ hprev, db=dG.sum(1), dx=(dG @ w_ih).sum(0),
              dw_ih_abs=aGt @ x.abs(), dw_hh_abs=aGt @ hprev.abs(), db_abs=dG.abs().sum(1), dx_abs=(dG.abs() @ w_ih.abs()).sum(0))


def torch_lstm(x, w_ih, w_hh, b_ih, b_hh, cap_lens, state, Lout, dtype=F64):
    """torch.nn.LSTM(bidirectional=True) over pack_padded_sequence, as RNN_ENCODER.forward runs it (model.py:139-158);
    lengths in [1, T].  x [B][T][ninput].  Returns words [B][2H][Lout], sent [B][2H], the leaf x and the module."""
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    B, T, ninput = x.shape
    H = w_hh.shape[2]
    m = torch.nn.LSTM(ninput, H, batch_first=True, bidirectional=True).to(dtype)
    with torch.no_grad():
        for d, suf in enumerate(('', '_reverse')):
            getattr(m, 'weight_ih_l0' + suf).copy_(w_ih[d])
            getattr(m, 'weight_hh_l0' + suf).copy_(w_hh[d])
            getattr(m, 'bias_ih_l0' + suf).copy_(b_ih[d])
            getattr(m, 'bias_hh_l0' + suf).copy_(b_hh[d])
    xl = x.detach().to(dtype).clone().requires_grad_(True)
    lens = torch.tensor(clamp_lens(cap_lens, T), dtype=torch.int64)
    assert int(lens.min()) >= 1
    hx = None if state is None else (_c(state[0], dtype).contiguous(), _c(state[1], dtype).contiguous())
    out, (hn, _) = m(pack_padded_sequence(xl, lens, batch_first=True, enforce_sorted=False), hx)
    out, _ = pad_packed_sequence(out, batch_first=True, total_length=T)
    return NS(words=out.transpose(1, 2)[:, :, :Lout], sent=hn.transpose(0, 1).reshape(B, 2 * H), x=xl, m=m)


def torch_lstm_grads(t, gw, gs):
    """autograd of (words * gw).sum() + (sent * gs).sum() through torch_lstm's module, stacked as the project stacks them"""
    ((t.words * gw.to(t.words.dtype)).sum() + (t.sent * gs.to(t.sent.dtype)).sum()).backward()
    m = t.m
    pair = lambda k: torch.stack((getattr(m, k).grad, getattr(m, k + '_reverse').grad))     # noqa: E731
    return NS(dx=t.x.grad, dw_ih=pair('weight_ih_l0'), dw_hh=pair('weight_hh_l0'), db=pair('bias_ih_l0'), db_hh=pair('bias_hh_l0'))


# ------------------------------------------------------------------ BERT: forward pieces
def layer_norm(v, gamma, beta, eps=LN_EPS, mut=()):
    """over the last axis, biased variance; a constant row gives beta exactly"""
    C = v.shape[-1]
    d = v - v.mean(-1, keepdim=True)
    var = (d * d).sum(-1, keepdim=True) / (C - 1 if 'var_c1' in mut else C)
    return d / torch.sqrt(var + eps) * gamma + beta


def embed_ln(tokens, we, pe, te, gamma, beta, L, eps=LN_EPS, dtype=F64, mut=()):
    """tokens [B*L] int64 -> LayerNorm(we[token] + pe[row % L] + te[0]) [B*L][C]; a token outside [0, ntoken) reads row 0"""
    we, pe, te, gamma, beta = (_c(t, dtype) for t in (we, pe, te, gamma, beta))
    tok = tokens.detach().flatten().clone().long()
    tok[(tok < 0) | (tok >= we.shape[0])] = 0
    row = torch.arange(tok.numel())
    pos = row // L if 'pos_div' in mut else row % L
    return layer_norm(we[tok] + pe[pos] + te[0], gamma, beta, eps, mut)


def add_ln(x, res, gamma, beta, eps=LN_EPS, dtype=F64, mut=()):
    return layer_norm(_c(x, dtype) + _c(res, dtype), _c(gamma, dtype), _c(beta, dtype), eps, mut)


def attention(qkv, B, L, heads, dtype=F64, mut=()):
    """qkv [B*L][3C] = q | k | v, C = 64 heads -> ctx [B*L][C] = softmax(q k^T / 8) v per (caption, head), no mask"""
    q, k, v = (t.permute(0, 2, 1, 3) for t in _c(qkv, dtype).view(B, L, 3, heads, 64).unbind(2))        # [B][heads][L][64]
    s = q @ k.transpose(2, 3) * (1.0 if 'no_scale' in mut else 0.125)
    return (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(B * L, heads * 64)


def gelu(x, dtype=F64, mut=()):
    x = _c(x, dtype)
    if 'tanh' in mut:
        return 0.5 * x * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))
    return 0.5 * x * (1 + torch.erf(x * math.sqrt(0.5)))


def tanh_t(x, B, L, C, dtype=F64):
    """x [B*L][C] -> y [B][C][L] = tanh(x[b*L + l][c])"""
    return torch.tanh(_c(x, dtype)).view(B, L, C).permute(0, 2, 1).contiguous()


# ------------------------------------------------------------------ BERT: the heads' backward
def words_head_bwd(dwords, y, dtype=F64, mut=()):
    """words = y = tanh(pre) as [B][nef][L]: dpre [B*L][nef] = (dwords (1 - y^2)) transposed, dbias [nef] = its sum over
    (b, l), and dbias_abs"""
    dwords, y = _c(dwords, dtype), _c(y, dtype)
    B, nef, L = y.shape
    g = dwords * (1 - y * y)
    gs = g[:, :, :L - 1] if 'miss_last' in mut else g
    return NS(dpre=g.permute(0, 2, 1).reshape(B * L, nef), dbias=gs.sum((0, 2)), dbias_abs=gs.abs().sum((0, 2)))


def sent_head_bwd(dsent, sent, pooled, cls, w_fc, dpooled=None, dtype=F64):
    """sent = tanh(fc(pooled)) [B][nef], pooled = tanh(pooler(cls)) [B][C]:
        g = dsent (1 - sent^2);  dw_fc [nef][C] = g^T pooled;  db_fc = sum_b g;  dpooled [B][C] = g w_fc
        h = dpooled (1 - pooled^2);  dw_pool [C][C] = h^T cls;  db_pool = sum_b h
    with the sums of absolute summands.  dpooled given: the second stage is evaluated on it (the second launch reads what
    the first one stored)."""
    dsent, sent, pooled, cls, w_fc = (_c(t, dtype) for t in (dsent, sent, pooled, cls, w_fc))
    g = dsent * (1 - sent * sent)
    r = NS(dpooled=g @ w_fc, dw_fc=g.t() @ pooled, db_fc=g.sum(0), dw_fc_abs=g.abs().t() @ pooled.abs(), db_fc_abs=g.abs().sum(0))
    h = (r.dpooled if dpooled is None else _c(dpooled, dtype)) * (1 - pooled * pooled)
    r.dw_pool, r.db_pool, r.dw_pool_abs, r.db_pool_abs = h.t() @ cls, h.sum(0), h.abs().t() @ cls.abs(), h.abs().sum(0)
    return r


# ====================================================================================================================
# The GPU cases (tests/test_text_kernels_gpu.py), each with the arm it reaches, and their inputs: float32 tensors on
# the CPU from oracle.fill.  Each shape is the smallest that reaches its arm.
# ====================================================================================================================
RC = namedtuple('RC', 'B T Lout H lens state wscale gscale arm')
# sba_lstm_recur_train / sba_lstm_recur_bwd: the recurrence and BPTT on a given gx
RECUR_CASES = [
    RC(1, 5, 5, 64, (5,), None, 1.0, 1.0, 'H = 64, B = 1, Lout = T = len'),
    RC(5, 18, 18, 64, (1, 18, 7, 0, -3), 'state', 1.0, 1.0, 'H = 64, B = 5, Lout = T, lengths 1, T, middle, 0 and -3, state'),
    RC(5, 18, 18, 128, (22, 12, 1, 0, 5), None, 1.0, 1.0, 'H = 128, B = 5, Lout = T, lengths T + 4 (clamped), 1 and 0'),
    RC(5, 18, 12, 128, (12, 1, 7, 3, 12), 'state', 1.0, 1.0, 'H = 128, Lout = max(lens) < T, state'),
    RC(5, 18, 6, 64, (18, 6, 7, 1, 22), 'state', 1.0, 2.0, 'H = 64, Lout < len (captions 0, 2 and 4), state, gx x 2'),
    RC(5, 18, 6, 128, (18, 6, 7, 1, 0), None, 1.7, 1.0, 'H = 128, Lout < len, w_hh x 1.7'),
    RC(1, 9, 9, 128, (4,), 'state', 1.0, 1.0, 'H = 128, B = 1, len < Lout = T, state'),
    RC(5, 18, 18, 64, (18, 12, 7, 7, 1), None, 1.0, 1.0, 'H = 64, sorted lengths in [1, T] (torch.nn.LSTM)'),
    RC(4, 9, 9, 128, (9, 6, 2, 1), 'state', 1.0, 1.0, 'H = 128, sorted lengths in [1, T] (torch.nn.LSTM), state'),
]
FC = namedtuple('FC', 'B T Lout ninput H ntoken lens state arm')
# sba_lstm_bidir_fwd: projection (8 rows per workgroup, ceil(4H / 256) gate blocks per direction) + recurrence
FWD_CASES = [
    FC(3, 5, 5, 4, 64, 11, (5, 1, 3), None, 'B*T = 15 (partial 8-row tile), ninput = 4, one gate block (H = 64)'),
    FC(3, 5, 4, 300, 128, 11, (9, 0, 2), 'state', 'B*T = 15, ninput = 300, two gate blocks (H = 128), Lout < len, len 0, state'),
    FC(2, 8, 8, 2048, 64, 7, (8, 3), None, 'B*T = 16 (whole tiles), ninput = 2048: 64 KB of LDS, the accepted edge'),
    FC(1, 8, 5, 300, 128, 11, (5,), 'state', 'B = 1, B*T = 8, two gate blocks, Lout = len < T, state'),
]
E2E = namedtuple('E2E', 'B T ninput H lens')
# ops.LstmBidirTrainFn end to end, non-zero state, L = T
E2E_CASES = [E2E(4, 9, 12, 64, (9, 4, 1, 6)), E2E(3, 6, 300, 128, (3, 6, 1))]


def case_id(c):
    """a pytest id: the case's numbers, without the name of its arm"""
    if isinstance(c, str):
        return c
    c = c[:-1] if isinstance(c[-1], str) else c
    c = c[0] if len(c) == 1 and isinstance(c[0], tuple) else c
    return '-'.join(str(v).replace(' ', '') for v in c)


def state_of(B, H, tag=203):
    """non-zero initial state, values in +-0.3"""
    return 0.3 * fill.uniform((2, B, H), tag), 0.3 * fill.uniform((2, B, H), tag + 1)


def recur_inputs(c):
    B, T, H = c.B, c.T, c.H
    return NS(gx=c.gscale * fill.unit((2, B * T, 4 * H), 201), w_hh=fill.unit((2, 4 * H, H), 202) * (c.wscale / math.sqrt(H)),
              lens=torch.tensor(c.lens, dtype=torch.int64), state=state_of(B, H) if c.state else None,
              dwords=fill.unit((B, 2 * H, c.Lout), 205), dsent=fill.unit((B, 2 * H), 206))


def lstm_weights(ninput, H):
    return NS(w_ih=fill.unit((2, 4 * H, ninput), 213) / math.sqrt(ninput), w_hh=fill.unit((2, 4 * H, H), 202) / math.sqrt(H),
              b_ih=0.1 * fill.unit((2, 4 * H), 214), b_hh=0.1 * fill.unit((2, 4 * H), 215))


def fwd_inputs(c):
    """token ids in [0, ntoken) with -1 and ntoken planted among them (both must read row 0)"""
    i = lstm_weights(c.ninput, c.H)
    cap = fill.uniform((c.B, c.T), 211, 0, c.ntoken).floor().long().clamp(0, c.ntoken - 1)
    cap.view(-1)[1], cap.view(-1)[-2] = -1, c.ntoken
    i.captions, i.emb = cap, fill.unit((c.ntoken, c.ninput), 212)
    i.lens, i.state = torch.tensor(c.lens, dtype=torch.int64), state_of(c.B, c.H) if c.state else None
    return i


def e2e_inputs(c):
    i = lstm_weights(c.ninput, c.H)
    i.x, i.lens, i.state = fill.unit((c.B, c.T, c.ninput), 221), torch.tensor(c.lens, dtype=torch.int64), state_of(c.B, c.H)
    i.gw, i.gs = fill.unit((c.B, 2 * c.H, c.T), 222), fill.unit((c.B, 2 * c.H), 223)
    return i


def e2e_reference(c):
    """the projection GEMM, the recurrence, BPTT and the three GEMMs, all float64 references: (inputs, forward, the
    parameter gradients with their sums of absolute summands from the float64 dG)"""
    i = e2e_inputs(c)
    x2 = i.x.double().view(c.B * c.T, c.ninput)
    gx = torch.einsum('rk,djk->drj', x2, i.w_ih.double()) + (i.b_ih.double() + i.b_hh.double())[:, None, :]
    f = lstm_recur(gx, i.w_hh, i.lens, i.state, c.T, c.T)
    g = lstm_bptt(f.gates, f.cs, f.hs, i.w_hh, i.lens, i.state, i.gw, i.gs, c.T, c.T)
    return i, f, lstm_param_grads(g.dG, g.hprev, x2, i.w_ih)


# ---- BERT.  One wave per row, 4 rows per workgroup, per = C / 64 values per lane (1 .. 16); attention tiles of L <= 32
# (B, L, C): rows = B * L
EMBED_CASES = [((1, 1, 64), 'rows = 1, per = 1'), ((1, 5, 768), 'rows = 5 (rows % 4 = 1), per = 12'),
               ((3, 7, 1024), 'rows = 21, per = 16, position index wraps, tokens out of range'),
               ((2, 4, 768), 'rows = 8 (whole workgroups), position index wraps'), ((3, 7, 64), 'rows = 21, per = 1, wraps')]
# (rows, C, kind)
ADD_LN_CASES = [((1, 64, ''), 'rows = 1, per = 1'), ((5, 768, ''), 'rows = 5, per = 12'), ((21, 1024, ''), 'rows = 21, per = 16'),
                ((8, 768, ''), 'rows = 8 (whole workgroups)'), ((21, 64, ''), 'rows = 21, per = 1'),
                ((5, 768, 'offset'), 'rows with mean = 4 x std'), ((5, 64, 'const'), 'row 2: x + res exactly constant -> beta')]
# (B, L, heads, top): top = 0: unit q and k (|logit| up to about 4); else q and k scaled so that the largest logit is top
ATTN_CASES = [((1, 1, 1, 0.0), 'L = 1'), ((2, 7, 2, 0.0), 'L = 7, two heads'), ((3, 20, 12, 0.0), 'the workload width'),
              ((1, 32, 12, 0.0), 'L = 32: the LDS tile edge'), ((2, 7, 2, 50.0), 'logits about +-50'),
              # exp(50) = 5e21 is still an f32 number, so a softmax without its max subtraction would pass at 50: at 100
              # (exp(88.8) overflows f32) it gives inf / inf.  v > 0 there: no ctx element is what is left of a cancellation
              ((2, 7, 2, 100.0), 'logits about +-100: exp() overflows f32 without the max subtraction')]
GELU_CASES = [(1, 'n = 1'), (255, 'one partial workgroup'), (257, 'two workgroups'), (4096 * 256 + 3, 'the grid-stride loop wraps')]
# (B, L, C)
TANH_T_CASES = [((1, 1, 1), 'one element'), ((2, 7, 5), 'odd sizes'), ((3, 20, 256), 'the workload shape'),
                ((8, 32, 4100), 'more than 4096 * 256 elements: the grid-stride loop wraps')]
# (B, L, nef)
WORDS_BWD_CASES = [((1, 1, 64), 'one (b, l) term'), ((3, 7, 128), 'two workgroups, odd L'), ((2, 32, 256), 'L = 32: the LDS tile edge'),
                   ((32, 12, 256), 'the workload shape')]
# (B, C, nef)
SENT_BWD_CASES = [((1, 64, 64), 'B = 1: single products'), ((3, 128, 64), 'C != nef'), ((64, 64, 128), 'B = 64: the accepted edge'),
                  ((5, 768, 256), 'the workload widths')]
# fill tags of the non-zero prefills of the outputs the kernels add to (test_norm_kernels_gpu.prefilled)
TAG_DBIAS, TAG_DWFC, TAG_DBFC, TAG_DWP, TAG_DBP = 271, 281, 282, 283, 284


def ln_params(C, tag):
    return 1 + 0.3 * fill.unit((C,), tag), 0.2 * fill.unit((C,), tag + 1)


def away(shape, tag, lo, hi):
    """values of either sign with lo <= |v| < hi: no summand of a short sum is small against a prefill of about 0.5"""
    return fill.uniform(shape, tag, lo, hi) * torch.where(fill.uniform(shape, tag + 50) < 0, -1.0, 1.0)


def embed_inputs(B, L, C, ntoken=13):
    rows = B * L
    tok = fill.uniform((rows,), 231, 0, ntoken).floor().long().clamp(0, ntoken - 1)
    if rows >= 5:
        tok[1], tok[rows - 2] = -1, ntoken
    gamma, beta = ln_params(C, 235)
    # (the position table has max(L, B) rows so that the wrong index row / L of the `pos_div` variant stays inside it)
    return NS(tok=tok, we=fill.unit((ntoken, C), 232), pe=0.5 * fill.unit((max(L, B), C), 233), te=0.5 * fill.unit((2, C), 234),
              gamma=gamma, beta=beta, ntoken=ntoken)


def add_ln_inputs(rows, C, kind, T=F32):
    """x and residual in storage type T.  'offset': every row at mean 4 x std.  'const': row 2 has x + res = 1.5 exactly
    (multiples of 1 / 16, exact in bf16 too, and every partial sum of up to 1024 of them is exact in f32)."""
    x = ((OFFSET if kind == 'offset' else 0.0) + fill.unit((rows, C), 241)).to(T)
    res = (0.5 * fill.unit((rows, C), 242)).to(T)
    if kind == 'const':
        x[2] = ((fill.unit((C,), 243) * 16).round() / 16).to(T)
        res[2] = (1.5 - x[2].float()).to(T)
        assert bool((x[2].float() + res[2].float() == 1.5).all())
    gamma, beta = ln_params(C, 245)
    return NS(x=x, res=res, gamma=gamma, beta=beta)


def attn_inputs(B, L, heads, top, T=F32):
    """qkv [B*L][3C] in storage type T; top > 0: q and k scaled so that the largest logit is +top (before the rounding to T;
    the smallest is about -top); top >= 100: v in [0.5, 1.5)"""
    C = 64 * heads
    qkv = fill.unit((B * L, 3 * C), 251)
    if top:
        q, k = (t.permute(0, 2, 1, 3).double() for t in qkv.view(B, L, 3, heads, 64).unbind(2)[:2])
        qkv[:, :2 * C] *= math.sqrt(top / float((q @ k.transpose(2, 3) * 0.125).max()))
    if top >= 100:
        qkv[:, 2 * C:] = fill.uniform((B * L, C), 252, 0.5, 1.5)
    return qkv.to(T)


def gelu_inputs(n, T=F32):
    """3 x unit (|x| < 5.2), with 0, -0.0, 10 and -10 planted where there is room"""
    x = 3 * fill.unit((n,), 261)
    if n >= 255:
        x[3], x[4], x[5], x[6] = 0.0, -0.0, 10.0, -10.0
    return x.to(T)


def tanh_t_inputs(B, L, C, T=F32):
    return (1.5 * fill.unit((B * L, C), 265)).to(T)


def words_bwd_inputs(B, L, nef):
    """d words with 4 <= |.| < 8 and words = tanh(.) with 0.2 <= |y| < 0.8"""
    return NS(dwords=away((B, nef, L), 272, 4.0, 8.0), y=away((B, nef, L), 273, 0.2, 0.8))


def sent_bwd_inputs(B, C, nef):
    return NS(dsent=away((B, nef), 285, 4.0, 8.0), sent=away((B, nef), 286, 0.2, 0.8), pooled=away((B, C), 287, 0.2, 0.8),
              cls=away((B, C), 288, 0.5, 1.5), w_fc=fill.unit((nef, C), 289) / math.sqrt(C))


def sent_head_chain(B, C, nef, dtype=F64):
    """the forward chain itself (test_text_ref_cpu.py: autograd): cls, W_pool, b_pool, W_fc, b_fc"""
    return NS(cls=fill.unit((B, C), 291).to(dtype), w_pool=(fill.unit((C, C), 292) / math.sqrt(C)).to(dtype),
              b_pool=(0.1 * fill.unit((C,), 293)).to(dtype), w_fc=(fill.unit((nef, C), 294) / math.sqrt(C)).to(dtype),
              b_fc=(0.1 * fill.unit((nef,), 295)).to(dtype), dsent=fill.unit((B, nef), 296).to(dtype))
