"""tests/attn_ref.py checked without a GPU, before a kernel of csrc/attention.hip is judged by it.

(1) The float64 forward equals oracle.sbagan_oracle.word_attention (tied to the reference's golden vectors by
    tests/test_oracle_golden.py) in mask_mode 0, the backward equals float64 autograd in both mask modes, and the sums of
    absolute / squared summands equal a term-by-term evaluation.
(2) At EVERY case of tests/test_attention_kernels_gpu.py an emulation of the kernel family's stated arithmetic (float32
    torch; hi + lo bf16 pairs; bf16-rounded dS and a) is inside every bound the GPU test applies, by a factor 2 -- so a
    failure on the GPU is the kernel's, not the bound's or the inputs' -- and every applicable mutation of the reference
    is OUTSIDE, so the bounds are not vacuous.  Each case prints its ratios.

The one bound that cannot have a factor 2 to spare is the project's low_close (relative L2 at most twice the floor of ONE
bf16 rounding): a correct kernel rounds once, so it sits AT the floor, 0.5 of the bound, by construction; a rounding that
float32 noise tips the other way adds a few 1e-4 of that.  The emulations are held to 0.5 x 1.01 there.

Mutations (each judged by the same functions as the GPU outputs):
    query / tile    one query, or one 32-query tile, takes no part: its ctx / att / dh elements keep their NaN prefill
                    (accumulate = 1: the previous dh), and dsrc, a sum over the queries, misses its summands -- dsrc
                    must fail ON ITS OWN, the only output in which a skipped query of the backward is a number
    word            word 0 (never masked) is left out of the softmax and of both contractions; L >= 2
    channel         one channel contributes nothing: src, h and dctx are zero there
    mask            mask[b] where mask[r % B] belongs and the reverse; where a mask is given and the two differ
    hi-only         the keys rounded to bf16 (no lo part).  Applies to the forward of the matrix-core kernels at L >= 2,
                    through the probabilities (ATT_ABS); at L = 1 the only probability is 1 and ctx = bf16(src) either
                    way.  It does NOT apply to the backward: dh (one bf16 ulp) and dsrc (bf16-rounded dS and a by
                    design) carry errors of the same 2^-9 order as a bf16 key -- no bound on them can tell.
    accumulate      dh does not add the previous gradient although asked to / adds the (NaN) buffer although not
"""
import functools

import numpy as np
import pytest
import torch

import attn_ref as R
from oracle import fill
from oracle import sbagan_oracle as O

TOL = 1e-10
SPARE = 0.5                     # the emulations stay below SPARE x bound ...
SPARE_LOW = 0.5 * 1.01          # ... and at the one-rounding floor of low_close (see above)
FWD_CASES = R.FWD_SMALL + R.FWD_TPW
BWD_CASES = R.BWD_SMALL + R.BWD_TPW + R.BWD_CHUNKS + R.BWD_DET


def same(got, ref, name=''):
    got, ref = got.detach().double(), ref.detach().double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = float((got - ref).abs().max())
    assert err <= TOL * max(1.0, float(ref.abs().max())), '%s: max err %.3e' % (name, err)


# ------------------------------------------------------------------ (1) the reference
def torch_forward(h, src, mask, mask_mode):
    """GlobalAttention.py:103-117 on [B][Q][idf] queries with torch.bmm, differentiable"""
    B, Q, _ = h.shape
    s = torch.bmm(h, src)
    if mask is not None:
        s = s.masked_fill(mask[R.mask_rows(B, Q, mask_mode)], -float('inf'))
    a = torch.softmax(s, 2)
    return torch.bmm(a, src.transpose(1, 2)), a.transpose(1, 2)


@pytest.mark.parametrize('shape', [(3, 8, 2, 5, 4), (5, 32, 3, 7, 6)], ids=lambda s: 'x'.join(map(str, s)))
def test_forward_is_the_oracle(shape):
    """mask_mode 0 against oracle.sbagan_oracle.word_attention; B divides Q in neither shape (3 / 10, 5 / 21), and the
    mask rows differ, so mask[r % B] and mask[b] give different results"""
    B, idf, ih, iw, L = shape
    Q, cdf = ih * iw, 6
    assert Q % B != 0
    h, words = fill.unit((B, idf, ih, iw), 211).double(), fill.unit((B, cdf, L), 212).double()
    w = fill.unit((idf, cdf, 1, 1), 213).double() / float(np.sqrt(cdf))
    mask = R.make_mask(B, L)
    assert not torch.equal(R.dead_words(B, Q, L, mask, 0), R.dead_words(B, Q, L, mask, 1))
    src = torch.einsum('ic,bcl->bil', w.view(idf, cdf), words)
    hq = h.reshape(B, idf, Q).transpose(1, 2)
    for m in (mask, None):
        cref, aref = O.word_attention(h, words, w, m)
        f = R.forward(hq, src, m, 0)
        same(f.ctx.transpose(1, 2).reshape(B, idf, ih, iw), cref, 'ctx')
        same(f.att.reshape(B, L, ih, iw), aref, 'att')
        same(f.a, f.att.transpose(1, 2), 'a')
    f0, f1 = R.forward(hq, src, mask, 0), R.forward(hq, src, mask, 1)
    assert float((f0.att - f1.att).abs().max()) > 1e-2, 'the two mask modes agree: the case cannot tell them apart'
    c1, a1 = torch_forward(hq, src, mask, 1)
    same(f1.ctx, c1, 'ctx, mask_mode 1'); same(f1.att, a1, 'att, mask_mode 1')


@pytest.mark.parametrize('mask_mode', [0, 1])
@pytest.mark.parametrize('with_mask', [True, False])
def test_backward_is_autograd(mask_mode, with_mask):
    B, Q, idf, L = 3, 10, 8, 4
    i = R.inputs(B, Q, idf, L, 'f32')
    mask = i.mask if with_mask else None
    h, src = i.h.double().requires_grad_(True), i.src.double().requires_grad_(True)
    ctx, att = torch_forward(h, src, mask, mask_mode)
    gh, gs = torch.autograd.grad(ctx, [h, src], i.dctx.double())
    r = R.backward(i.h, i.src, mask, mask_mode, i.dctx)
    same(r.dh, gh, 'dh'); same(r.dsrc, gs, 'dsrc')
    same(R.forward(i.h, i.src, mask, mask_mode).ctx, ctx, 'ctx')
    # the sums over absolute and squared summands, term by term
    hd, sd, dd, a, dS = i.h.double(), i.src.double(), i.dctx.double(), r.a, r.dS
    for b in range(B):
        for c in range(idf):
            for l in range(L):
                terms = [float(hd[b, q, c] * dS[b, q, l]) for q in range(Q)] + [float(dd[b, q, c] * a[b, q, l]) for q in range(Q)]
                assert abs(sum(abs(t) for t in terms) - float(r.dsrc_abs[b, c, l])) <= TOL
                assert abs(sum(t * t for t in terms) ** 0.5 - float(r.dsrc_rss[b, c, l])) <= TOL
    for b in range(B):
        for q in range(Q):
            for c in range(idf):
                terms = [float(dS[b, q, l] * sd[b, c, l]) for l in range(L)]
                assert abs(sum(abs(t) for t in terms) - float(r.dh_abs[b, q, c])) <= TOL
                assert abs(sum(t * t for t in terms) ** 0.5 - float(r.dh_rss[b, q, c])) <= TOL
    f = R.forward(i.h, i.src, mask, mask_mode)
    same(f.ctx_abs, torch.einsum('bql,bcl->bqc', f.a, sd.abs()), 'ctx_abs')
    # the conditioned sums hold the plain ones, and the first-order effect of a relative error c in every product of the
    # scores and of dA stays below c x them (c = 1e-6, one draw of signs; the second-order rest is c^2)
    assert bool((f.ctx_cond >= f.ctx_abs).all()) and bool((r.dh_cond >= r.dh_abs).all())
    c = 1e-6
    sgn = lambda tag: 1 + c * torch.sign(fill.unit((B, Q, idf, L), tag).double())      # noqa: E731
    dead = R.dead_words(B, Q, L, mask, mask_mode)
    a2 = torch.softmax((hd[:, :, :, None] * sd[:, None, :, :] * sgn(221)).sum(2).masked_fill(dead, -float('inf')), 2)
    dA2 = (dd[:, :, :, None] * sd[:, None, :, :] * sgn(222)).sum(2)
    dS2 = a2 * (dA2 - (a2 * dA2).sum(2, keepdim=True))
    assert bool(((torch.einsum('bql,bcl->bqc', a2, sd) - f.ctx).abs() <= 1.01 * c * f.ctx_cond).all())
    assert bool(((torch.einsum('bql,bcl->bqc', dS2, sd) - r.dh).abs() <= 1.01 * c * r.dh_cond).all())


def test_a_query_without_a_live_word_is_nan():
    """float64 softmax over an all -inf row is NaN: the placement the GPU test holds the kernels to"""
    c = R.FWD_FULL[0]
    i = R.inputs(c.B, c.Q, c.idf, c.L, c.dt, R.FULL_ROW)
    for mode in (0, 1):
        f = R.forward(i.h, i.src, i.mask, mode)
        nan_q = R.mask_rows(c.B, c.Q, mode) == R.FULL_ROW
        assert 0 < int(nan_q.sum()) < c.B * c.Q
        assert torch.equal(torch.isnan(f.ctx), nan_q[:, :, None].expand_as(f.ctx))
        assert torch.equal(torch.isnan(f.att), nan_q[:, None, :].expand_as(f.att))


def test_bf16_ulp():
    x = torch.tensor([1.0, 1.5, 1.999, 2.0, -3.0, 0.75, 0.0, 2.0 ** -20])
    want = torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6, 2.0 ** -8, 0.0, 2.0 ** -27]).double()
    assert torch.equal(R.bf16_ulp(x), want)
    y = fill.unit((4096,), 9).double()                      # one rounding is half an ulp at most
    assert bool(((y.to(torch.bfloat16).double() - y).abs() <= 0.5 * R.bf16_ulp(y)).all())


def test_the_bounds_are_the_projects():
    from test_kernels_gpu import tol
    t = tol(torch.float32)
    assert (t['rtol'], t['atol']) == (R.RTOL, R.ATOL)
    import inspect
    import test_norm_kernels_gpu as N
    assert 'worst <= 1e-5' in inspect.getsource(N.sums_close) and R.C_SUM == 1e-5
    assert 'factor=2.0' in inspect.getsource(N.low_close)
    assert torch.equal(N.prefilled(40, R.TAG_DSRC, torch.device('cpu'))[1].float(), R.dsrc_prefill(40))


# ------------------------------------------------------------------ the case lists reach what they claim
def tiles_per_wave(B, Q):
    tiles = -(-Q // 32) * B
    return 4 if tiles >= 16384 else (2 if tiles >= 4096 else 1)


def chunks(Q):
    return 4 if Q >= 16384 else (2 if Q >= 4096 else 1)


def test_case_lists():
    for arms, cases in ((R.FWD_ARMS, R.FWD_SMALL), (R.BWD_ARMS, R.BWD_SMALL)):
        for dt, idf in arms:
            mine = [c for c in cases if (c.dt, c.idf) == (dt, idf)]
            assert sorted(c.L for c in mine) == sorted(R.LS) and sorted(c.Q for c in mine) == sorted(R.QS)
            kinds = set(c.mask for c in mine)
            assert {'m0', 'm1'} <= kinds and kinds & {'n0', 'n1'}
            assert set(c[6] for c in mine) == {0, 1} and set(c.sliced for c in mine) == {0, 1}
            assert all(c.B == R.B_SMALL and c.Q % c.B for c in mine)
            assert all(tiles_per_wave(c.B, c.Q) == 1 and chunks(c.Q) == 1 for c in mine)
    assert [R.family_of(c) for c in R.FWD_SMALL[::5]] == ['f32', 'f32', 'f32', 'mfma16', 'mfma16', 'valu16']
    assert [R.family_of(c) for c in R.BWD_SMALL[::5]] == ['f32', 'f32', 'valu16', 'mfma16']
    assert [tiles_per_wave(c.B, c.Q) for c in R.FWD_TPW + R.BWD_TPW] == [2, 4, 2, 4]
    assert [tiles_per_wave(B, Q) for _, B, Q, _, _ in R.FP8_EXACT] == [1, 1, 2, 4]
    for c in R.FWD_TPW + R.BWD_TPW:
        assert R.family_of(c) == 'mfma16' and -(-c.Q // 32) == 9
        if c.B > 1024:                                      # rows beyond the LDS table, and different from the rows below
            m = R.make_mask(c.B, c.L)
            assert c.mask == 'm0' and not torch.equal(m[1024:], m[:c.B - 1024]) and not torch.equal(m[1024:2048], m[:1024])
    assert sorted(set((R.family_of(c), c.idf, chunks(c.Q)) for c in R.BWD_CHUNKS)) == sorted(
        (f, idf, k) for f, idf in (('f32', 32), ('f32', 64), ('valu16', 64)) for k in (2, 4))
    for c in R.BWD_CHUNKS:                                  # a last workgroup with 5 live queries and dead later chunks
        per_wg = (128 if c.dt == 'f32' else 256) * chunks(c.Q)
        assert c.Q % per_wg == 5 and c.B in (1, 2)
    for c in R.BWD_DET:                                     # more than one workgroup per image
        per_wg = 128 if R.family_of(c) != 'f32' and c.idf == 32 else (128 if c.dt == 'f32' else 256)
        assert -(-c.Q // per_wg) > 1
    biggest = max(c.B * c.Q * c.idf * (2 if c.dt == 'bf16' else 4) * (2 if c.sliced else 1)
                  for c in R.FWD_SMALL + R.FWD_TPW + R.FWD_FULL + BWD_CASES)
    assert biggest <= 40 << 20, biggest


# ------------------------------------------------------------------ (2) emulations inside, mutations outside
def _show(title, ratios):
    print('%-74s %s' % (title, '  '.join('%s %.3g' % kv for kv in sorted(ratios.items()))))


def _inside(ratios, title):
    _show(title, ratios)
    for k, v in ratios.items():
        assert v <= (SPARE_LOW if k.endswith(' low') else SPARE), '%s: the emulation is at %.3f of the bound "%s"' % (title, v, k)


def _outside(ratios, title, only=None):
    _show(title, ratios)
    worst = max(v for k, v in ratios.items() if only is None or k.startswith(only))
    assert worst > 1.0, '%s: the mutation passes every bound (worst %.3f)' % (title, worst)
    return worst


def _unwritten(x, b, qs, axis):
    x = x.clone()
    if axis == 1:
        x[b, qs] = float('nan')
    else:
        x[b, :, qs] = float('nan')
    return x


def _tile(Q):
    """the last full 32-query tile (the whole map where it is shorter)"""
    q0 = max(0, (Q // 32 - 1) * 32)
    return torch.arange(q0, min(Q, q0 + 32))


def _zero_channel(x, c, axis):
    x = x.clone()
    x.select(axis, c).zero_()
    return x


@pytest.mark.parametrize('case', FWD_CASES, ids=R.case_id)
def test_forward_bounds(case):
    fam = R.family_of(case)
    i, mask, mode = R.case_inputs(case)
    B, Q, L = case.B, case.Q, case.L
    ref = R.forward(i.h, i.src, mask, mode)
    e = R.emulate_fwd(fam, i.h, i.src, mask, mode)
    _inside(R.fwd_ratios(fam, e.ctx, e.att, ref), 'emulation ' + R.case_id(case))
    b = B - 1
    for name, qs in (('query', torch.tensor([Q - 1])), ('tile', _tile(Q))):
        _outside(R.fwd_ratios(fam, _unwritten(ref.ctx, b, qs, 1), _unwritten(ref.att, b, qs, 2), ref), name + ' dropped')
    if L >= 2:
        m = R.forward(i.h, i.src[:, :, 1:], None if mask is None else mask[:, 1:], mode)
        att = torch.cat((torch.full((B, 1, Q), float('nan'), dtype=torch.float64), m.att), 1)
        _outside(R.fwd_ratios(fam, m.ctx, None, ref), 'word dropped', only='ctx')
        _outside(R.fwd_ratios(fam, m.ctx, att, ref), 'word dropped', only='att')
    c0 = case.idf - 1
    m = R.forward(_zero_channel(i.h, c0, 2), _zero_channel(i.src, c0, 1), mask, mode)
    _outside(R.fwd_ratios(fam, m.ctx, m.att, ref), 'channel dropped', only='ctx')
    if mask is not None and not torch.equal(R.dead_words(B, Q, L, mask, 0), R.dead_words(B, Q, L, mask, 1)):
        m = R.forward(i.h, i.src, mask, 1 - mode)
        _outside(R.fwd_ratios(fam, m.ctx, None, ref), 'mask of the other mode', only='ctx')
        _outside(R.fwd_ratios(fam, m.ctx, m.att, ref), 'mask of the other mode', only='att')
    if fam == 'mfma16' and L >= 2:
        m = R.forward(i.h, i.src.to(torch.bfloat16), mask, mode)
        _outside(R.fwd_ratios(fam, m.ctx, m.att, ref), 'hi-only keys', only='att abs')


@pytest.mark.parametrize('case', R.FWD_FULL, ids=R.case_id)
def test_forward_bounds_with_a_fully_masked_row(case):
    fam = R.family_of(case)
    i, mask, mode = R.case_inputs(case, R.FULL_ROW)
    ref = R.forward(i.h, i.src, mask, mode)
    e = R.emulate_fwd(fam, i.h, i.src, mask, mode)
    assert bool(torch.isnan(ref.ctx).any()) and not bool(torch.isnan(ref.ctx).all())
    _inside(R.fwd_ratios(fam, e.ctx, e.att, ref), 'emulation ' + R.case_id(case))
    m = R.forward(i.h, i.src, mask, 1 - mode)               # NaN at the other mode's queries
    assert _outside(R.fwd_ratios(fam, m.ctx, m.att, ref), 'mask of the other mode', only='ctx NaN') == R.INF
    zero = torch.where(torch.isnan(ref.ctx), torch.zeros_like(ref.ctx), ref.ctx)
    assert _outside(R.fwd_ratios(fam, zero, ref.att, ref), '0 in place of NaN', only='ctx NaN') == R.INF


def _dsrc_without(ref, i, b, qs):
    """dsrc when the queries qs of image b take no part in the sum"""
    out = ref.dsrc.clone()
    out[b] -= (torch.einsum('qc,ql->cl', i.h[b, qs].double(), ref.dS[b, qs])
               + torch.einsum('qc,ql->cl', i.dctx[b, qs].double(), ref.a[b, qs]))
    return out


def _needed_k(got, ref, pre):
    """the smallest multiple of U_BF16 x rss at which dsrc `got` passes (the C_SUM term as it is)"""
    over = (got - ref.dsrc).abs() - R.C_SUM * R.store_abs(ref.a.shape[1], pre, ref.dsrc_abs)
    return float((over / (R.U_BF16 * ref.dsrc_rss).clamp(min=1e-300)).max())


@functools.lru_cache(maxsize=None)
def backward_report(case):
    """everything test_backward_bounds and test_dsrc16_multiple need of a case, as numbers"""
    fam = R.family_of(case)
    i, mask, mode = R.case_inputs(case)
    B, Q, L, idf = case.B, case.Q, case.L, case.idf
    ref = R.backward(i.h, i.src, mask, mode, i.dctx)
    prev = i.prev if case.acc else None
    pre = R.dsrc_prefill(B * idf * L).view(B, idf, L)
    e = R.emulate_bwd(fam, i.h, i.src, mask, mode, i.dctx, prev, pre)
    added = e.dsrc.double() - pre.double()
    rep = dict(emulation=R.bwd_ratios(fam, e.dh, added, ref, pre, prev), k_emulation=_needed_k(added, ref, pre), k_mutation={})
    stored = ref.dh + (prev.double() if case.acc else 0)

    def judge(name, dh, dsrc):
        rep[name] = R.bwd_ratios(fam, dh, dsrc, ref, pre, prev)
    b = B - 1
    for name, qs in (('query dropped', torch.tensor([Q - 1])), ('tile dropped', _tile(Q))):
        dh = stored.clone()
        dh[b, qs] = prev[b, qs].double() if case.acc else float('nan')
        dsrc = _dsrc_without(ref, i, b, qs)
        judge(name, dh, dsrc)
        rep['k_mutation'][name] = _needed_k(dsrc, ref, pre)
    if L >= 2:
        m = R.backward(i.h, i.src[:, :, 1:], None if mask is None else mask[:, 1:], mode, i.dctx)
        judge('word dropped', m.dh + (prev.double() if case.acc else 0), torch.cat((torch.zeros(B, idf, 1).double(), m.dsrc), 2))
    c0 = idf - 1
    m = R.backward(_zero_channel(i.h, c0, 2), _zero_channel(i.src, c0, 1), mask, mode, _zero_channel(i.dctx, c0, 2))
    judge('channel dropped', m.dh + (prev.double() if case.acc else 0), m.dsrc)
    if mask is not None and not torch.equal(R.dead_words(B, Q, L, mask, 0), R.dead_words(B, Q, L, mask, 1)):
        m = R.backward(i.h, i.src, mask, 1 - mode, i.dctx)
        judge('mask of the other mode', m.dh + (prev.double() if case.acc else 0), m.dsrc)
    judge('accumulate ignored', ref.dh if case.acc else ref.dh + float('nan'), ref.dsrc)
    judge('dsrc overwritten, not added to', stored, ref.dsrc - pre.double())
    return rep


@pytest.mark.parametrize('case', BWD_CASES, ids=R.case_id)
def test_backward_bounds(case):
    rep = backward_report(case)
    _inside(rep['emulation'], 'emulation ' + R.case_id(case))
    for name, ratios in rep.items():
        if name in ('emulation', 'k_emulation', 'k_mutation'):
            continue
        if name in ('query dropped', 'tile dropped', 'dsrc overwritten, not added to'):
            _outside(ratios, name, only='dsrc')
        elif name == 'accumulate ignored':
            _outside(ratios, name, only='dh')
        elif case.L == 1 and name == 'channel dropped':     # dS = 0 at L = 1: dh is 0 either way
            _outside(ratios, name, only='dsrc')
        else:
            _outside(ratios, name, only='dh'), _outside(ratios, name, only='dsrc')


def test_dsrc16_multiple():
    """DSRC16_K: over the bf16 cases, the smallest multiple of U_BF16 x rss that leaves the emulations a factor 2, rounded
    up to a whole number -- and below the smallest multiple at which a dropped query or tile would pass"""
    cases = [c for c in BWD_CASES if c.dt == 'bf16']
    reps = [backward_report(c) for c in cases]
    need = max(r['k_emulation'] for r in reps)
    pass_at = min(min(r['k_mutation'].values()) for r in reps)
    worst = max(r['emulation']['dsrc bf16'] for r in reps)
    print('bf16 dsrc: the emulations need %.3f x U_BF16 x rss, a dropped query passes from %.3f on; at DSRC16_K = %g the '
          'emulations are at %.3f of the bound' % (need, pass_at, R.DSRC16_K, worst))
    assert R.DSRC16_K == float(np.ceil(2 * need)), (need, R.DSRC16_K)
    assert R.DSRC16_K < pass_at and worst <= SPARE


# ------------------------------------------------------------------ the exact FP8 inputs
@pytest.mark.parametrize('shape', R.FP8_EXACT + R.FP8_FULL, ids=lambda s: 'x'.join(map(str, s)))
def test_fp8_inputs_are_exact(shape):
    """h integers in [-2, 2] and src multiples of 1/4 in [-1, 1]: three significant bits at most, so e4m3 holds them times
    any power-of-two scale up to 448 / max; one live word per query: the probability is exactly 1 (256 x 1 is an e4m3
    value) and ctx is that key column, itself a bf16 value -- no tolerance"""
    idf, B, Q, L, mode = shape
    dead_row = R.FULL_ROW if shape in R.FP8_FULL else None
    i = R.fp8_inputs(B, Q, idf, L, mode, dead_row)
    for x, step in ((i.h.float(), 1.0), (i.src, 0.25)):
        assert torch.equal(x, (x / step).round() * step) and float((x / step).abs().max()) <= 4
    assert torch.equal(i.src.to(torch.bfloat16).float(), i.src)
    live = ~R.dead_words(B, Q, L, i.mask, mode)
    assert torch.equal(live.sum(2), (i.word >= 0).long())
    ok = i.word >= 0
    assert torch.equal(live[ok].float().argmax(1), i.word[ok])
    assert bool(ok.all()) == (dead_row is None) and bool(ok.any())
    f = R.forward(i.h, i.src, i.mask, mode)
    want = i.src.transpose(1, 2)[torch.arange(B)[:, None], i.word.clamp(min=0)].double()
    assert torch.equal(f.ctx[ok], want[ok]) and bool(torch.isnan(f.ctx[~ok]).all())
    if B > 1024:
        assert not torch.equal(i.mask[1024:2048], i.mask[:1024])
