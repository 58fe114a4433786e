"""The three entry points of csrc/attention.hip called directly through the C ABI (sbagan._lib), at the smallest shape
that reaches each kernel template and each arm of the host dispatch, element by element against the float64 reference of
tests/attn_ref.py evaluated on the kernel's own (storage-rounded) inputs.  Shapes are (B, Q, idf, L).

kernel                             host condition that selects it                         covered by
---------------------------------  -----------------------------------------------------  -----------------------------------
word_attn_fwd_kernel<float, IDF>   sba_word_attn_fwd, f32: always (launch_fwd);           test_forward: R.FWD_SMALL, five cases
  IDF = 32 / 64 / 128              grid = ceil(Q / 256) x B                               per IDF -- every L of {1, 3, 16, 17,
                                                                                          32} and every Q of {1, 31, 32, 33, 261}
                                                                                          (261: two workgroups), both mask
                                                                                          modes, mask = NULL, att given / NULL,
                                                                                          ctx at oco = 0 and in the upper half
                                                                                          of a 2 idf slice; test_fully_masked_row
word_attn_fwd_kernel<bf16, 128>    sba_word_attn_fwd, bf16, idf = 128                     the same five-case row of R.FWD_SMALL;
                                                                                          test_fully_masked_row
word_attn_fwd_kernel<bf16, 32>     bf16 and idf <= 64 needs ocs % 4 or oco % 4 != 0,      not reachable, not tested
word_attn_fwd_kernel<bf16, 64>     which the entry point refuses (V = 8)
word_attn_fwd_mfma_kernel<IDF, 0>  sba_word_attn_fwd, bf16, idf = 32 / 64                 R.FWD_SMALL rows (bf16, 32), (bf16, 64);
  tiles_per_wave = 1               ceil(Q / 32) x B < 4096                                test_fully_masked_row
  tiles_per_wave = 2               ceil(Q / 32) x B >= 4096                               test_forward: (512, 261, 32, 5): second
                                                                                          workgroup with ONE live tile
  tiles_per_wave = 4               ceil(Q / 32) x B >= 16384                              test_forward: (2048, 261, 32, 5): third
                                                                                          wave breaks after one tile, fourth idle
  mrow >= NDEAD (global mask read)   mask_mode 0 and B > 1024                             the same case: mask_mode 0, rows >= 1024
                                                                                          differ from rows < 1024
word_attn_fwd_mfma_kernel<IDF, 1>  sba_word_attn_fwd_fp8, idf = 32 / 64                   test_fp8_exact: (5, 261, 64, 9) and (5,
  (FP8, MT = IDF / 32)                                                                    33, 64, 32) (MT = 2), (512, 261, 64, 5)
                                                                                          (tpw = 2), (2048, 261, 32, 5) (tpw = 4,
                                                                                          mask_mode 0); test_fp8_fully_masked_row;
                                                                                          random inputs: test_kernels_gpu.
                                                                                          test_word_attention_fp8 (kept)
word_attn_bwd_mfma_kernel<32>      sba_word_attn_bwd, bf16, idf = 32 (dcs % 8 and         test_backward: R.BWD_SMALL row (bf16,
  tiles_per_wave = 1 / 2 / 4       dco % 8 == 0 always hold: V = 8); thresholds as        32): every L, every Q, both modes, NULL
                                   in the forward                                         mask, dctx slice, accumulate 0 / 1;
                                                                                          R.BWD_TPW: (512, 261, 32, 5) and (2048,
                                                                                          261, 32, 5) in mask_mode 0
  det_part + sba_det_fold          deterministic mode                                     test_backward_deterministic (3 workgroups
                                                                                          per image)
word_attn_bwd_kernel<bf16, 32>     bf16 and idf = 32 always takes the matrix-core arm     not reachable, not tested
word_attn_bwd_kernel<bf16, 64>     sba_word_attn_bwd, bf16, idf = 64 (ds_read_tr16_b64    test_backward: R.BWD_SMALL row (bf16,
  chunks = 1 / 2 / 4               fragments, CT = 2); chunks by Q >= 4096 / 16384        64); R.BWD_CHUNKS: (1, 4101, 64, 7) and
                                                                                          (2, 16389, 64, 7): the last workgroup
                                                                                          has 5 live queries, its later chunks none
word_attn_bwd_kernel<float, 32>    sba_word_attn_bwd, f32, idf = 32 / 64                  R.BWD_SMALL rows (f32, 32), (f32, 64);
word_attn_bwd_kernel<float, 64>                                                           R.BWD_CHUNKS at both Q, both idf
  det_part + sba_det_fold          deterministic mode                                     test_backward_deterministic: <float, 64>
                                                                                          (3 workgroups), <bf16, 64> (2)
every SBA_E_ARG condition          --                                                     test_refusals (B > 65535 left out: it
                                                                                          needs buffers beyond BIG)

No environment switch selects a kernel: the dtype, idf, the shape and the deterministic mode do.

Bounds (tests/attn_ref.py; tests/test_attn_ref_cpu.py shows, at every case of this file, that an emulation of the kernel
family's stated arithmetic is inside each by a factor 2 and that a dropped query, tile, word or channel, the mask of the
other mode, hi-only keys and an ignored accumulate flag are outside).
  f32 ctx, att, dh       elementwise rtol 2e-4 / atol 2e-5 (elem_close); att of the bf16 VALU kernel likewise
  bf16 ctx, dh           relative L2 at most twice the one-rounding floor (low_close), AND every element within one bf16
                         ulp of the float64 value + 1e-5 x the sum of the absolute summands, the summands taken with the
                         first-order effect of the same relative error in the scores / dA / <a, dA> in front of them
  att, matrix-core       3e-5 absolute (keys as hi + lo bf16 pairs)
  dsrc, f32              1e-5 x the sum of the absolute summands (sums_close), on stored - prefill
  dsrc, bf16             9 x 2^-9 x root-sum-of-squares of the summands + the f32 term (dS and a are rounded to bf16 by
                         design).  Derived on the CPU: the emulations need 4.23 x 2^-9 x rss at the worst case, 9 is the
                         smallest whole multiple with a factor 2 to spare (emulations at 0.47 of the bound), and one query
                         dropped of 16,389 still fails up to a multiple of 17.9.
  dsrc, both             the stored value is prefill + sum: one f32 ulp of the prefill per 32-query tile on top
  FP8, exact inputs      no tolerance
A query without a live word is NaN in att and ctx exactly where float64 has it.

entry point            worst measured error / bound (MI355X)
---------------------  ----------------------------------------------------------------------------------------------
sba_word_attn_fwd      f32: ctx 0.023 ((5, 261, 64, 17), mask = NULL), att 0.011 ((5, 261, 128, 16))
                       bf16 VALU (idf 128): att 0.007; ctx as below
                       bf16 matrix cores: att 0.314 (9.4e-6 absolute, (512, 261, 32, 5)); ctx within 0.493 of one ulp +
                       dot-product bound (a rounding is half an ulp), rel L2 1.000 x the floor = 0.50 of the bound
sba_word_attn_fwd_fp8  exact (no tolerance), NaN exactly at the queries without a live word
sba_word_attn_bwd      f32: dh 0.033 ((2, 16389, 64, 7)); dsrc 0.464 at (5, 1, 64, 32) -- ONE query: the rounding of
                       prefill + sum against one f32 ulp of the prefill -- and 2.0e-8 of sum |summands| = 0.002 at
                       Q = 16389, 1.8e-7 in deterministic mode at Q = 261
                       bf16: dh within 0.499 of one ulp + bound, rel L2 1.000 x the floor; dsrc 0.473 of 9 x 2^-9 x
                       rss ((2048, 261, 32, 5), matrix cores; the emulation: 0.473), 0.27 on the VALU arm at Q = 16389

Every output buffer is longer (and, with a channel stride, wider) than the kernel should write and is prefilled with
NaN -- dsrc, which the kernels add to, and dh with accumulate = 1 with non-zero values in front of a NaN tail; dctx is
read from a slice whose other half holds NaN.  Everything outside the written range must still be NaN afterwards and
everything inside finite.
"""
import functools
from types import SimpleNamespace as NS

import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_ref as R  # noqa: E402
from test_kernels_gpu import _reset_cfg, dev  # noqa: E402,F401
from test_norm_kernels_gpu import (BIG, PAD, _refuse, deterministic, elem_close, front, lib, low_close, nans, p, prefilled,  # noqa: E402
                                   same_bits, stream, sums_close, twice, window)

F32 = torch.float32
CODE = {'f32': 0, 'bf16': 1}


def mask8(mask, dev):
    return None if mask is None else mask.to(torch.uint8).contiguous().to(dev)


def report(name, ratios):
    print('%-72s %s' % (name, '  '.join('%s %.3g' % kv for kv in sorted(ratios.items()))))
    for k, v in ratios.items():
        assert v <= 1.0, '%s: %s is at %.3f of its bound' % (name, k, v)


@pytest.fixture(scope='module', autouse=True)
def _free_the_references():
    """the float64 references of the two B = 2048 cases are some hundred MB each: shared while this file runs, gone after.
    The file leaves the process as it found it: no reference kept, and the 34 MB device blocks of the B = 2048 cases handed
    back, so that the tests behind it meet the allocator they meet without this file."""
    yield
    import gc
    from sbagan import ops
    for f in (forward_ref, backward_ref, R.inputs):
        f.cache_clear()
    ops.set_deterministic(False)
    ops._DET_SCRATCH[0] = None                              # (set_deterministic(True) allocates the ring again when asked)
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=2)
def forward_ref(case, full_row=None):
    i, mask, mode = R.case_inputs(case, full_row)
    return R.forward(i.h, i.src, mask, mode)


@functools.lru_cache(maxsize=2)
def backward_ref(case):
    i, mask, mode = R.case_inputs(case)
    return R.backward(i.h, i.src, mask, mode, i.dctx)


# ------------------------------------------------------------------ sba_word_attn_fwd
def run_forward(dev, case, full_row=None):
    i, mask, mode = R.case_inputs(case, full_row)
    B, Q, idf, L = case.B, case.Q, case.idf, case.L
    T = R.DTYPES[case.dt]
    ocs, oco = (2 * idf, idf) if case.sliced else (idf, 0)
    h, src, m8 = i.h.to(dev), i.src.to(dev), mask8(mask, dev)
    out = nans((B * Q + 3) * ocs, T, dev)
    att = nans(B * L * Q + PAD, F32, dev)
    lib().call('sba_word_attn_fwd', CODE[case.dt], p(h), p(src), p(m8), p(out), p(att) if case.att else None, B, Q, idf, L,
               mode, ocs, oco, stream())
    torch.cuda.synchronize()
    return NS(out=out, att=att, ocs=ocs, oco=oco)


def check_forward(r, case, ref, name):
    """NaN guards first (window / front refuse a write outside the slice, past the end, or a skipped element), then the
    bounds; where float64 has NaN queries the guards' finiteness check is replaced by the NaN placement of R.fwd_ratios"""
    B, Q, idf, L = case.B, case.Q, case.idf, case.L
    fam = R.family_of(case)
    nan_q = torch.isnan(ref.ctx[:, :, 0])                   # [B][Q]: float64 says NaN
    v = r.out.detach().float().cpu().view(-1, r.ocs)
    inside = v[:B * Q, r.oco:r.oco + idf].double().view(B, Q, idf)
    if not bool(nan_q.any()):
        window(r.out, B * Q, r.ocs, r.oco, idf, name + ' ctx')
    else:
        outside = torch.ones(v.shape, dtype=torch.bool)
        outside[:B * Q, r.oco:r.oco + idf] = False
        assert bool(torch.isnan(v[outside]).all()), '%s ctx: wrote outside its channel window / past the last row' % name
    att = None
    if case.att:
        a = r.att.detach().cpu()
        assert bool(torch.isnan(a[B * L * Q:]).all()), '%s att: wrote past its end' % name
        att = a[:B * L * Q].double().view(B, L, Q)
        if not bool(nan_q.any()):
            front(r.att, B * L * Q, name + ' att')
    else:
        assert bool(torch.isnan(r.att).all()), '%s: att = NULL, yet its buffer was written' % name
    report(name, R.fwd_ratios(fam, inside, att, ref))
    if bool(nan_q.any()):
        return
    if fam == 'f32':                                        # the project's own helpers, where the issue names them
        elem_close(inside, ref.ctx, name + ' ctx')
        if att is not None:
            elem_close(att, ref.att, name + ' att')
    else:
        low_close(inside.flatten(), ref.ctx.flatten(), name + ' ctx')
        if att is not None and fam == 'valu16':
            elem_close(att, ref.att, name + ' att')


@pytest.mark.parametrize('case', R.FWD_SMALL + R.FWD_TPW, ids=R.case_id)
def test_forward(dev, case):
    check_forward(run_forward(dev, case), case, forward_ref(case), 'fwd ' + R.case_id(case))


@pytest.mark.parametrize('case', R.FWD_FULL, ids=R.case_id)
def test_fully_masked_row(dev, case):
    """mask row 1 has no live word: att and ctx are NaN at exactly the queries float64 says (mask_mode 1: image 1;
    mask_mode 0: the rows r with r % B == 1), finite and within bound everywhere else"""
    ref = forward_ref(case, R.FULL_ROW)
    assert bool(torch.isnan(ref.ctx).any()) and not bool(torch.isnan(ref.ctx).all())
    check_forward(run_forward(dev, case, R.FULL_ROW), case, ref, 'fwd, row without a live word, ' + R.case_id(case))


# ------------------------------------------------------------------ sba_word_attn_fwd_fp8
def run_fp8(dev, shape, dead_row=None, with_att=True):
    idf, B, Q, L, mode = shape
    i = R.fp8_inputs(B, Q, idf, L, mode, dead_row)
    h, src, m8 = i.h.to(dev), i.src.to(dev), mask8(i.mask, dev)
    out = nans(B * Q * idf + PAD, torch.bfloat16, dev)
    att = nans(B * L * Q + PAD, F32, dev)
    lib().call('sba_word_attn_fwd_fp8', p(h), p(src), p(m8), p(out), p(att) if with_att else None, B, Q, idf, L, mode, idf, 0,
               stream())
    torch.cuda.synchronize()
    o, a = out.detach().float().cpu(), att.detach().cpu()
    assert bool(torch.isnan(o[B * Q * idf:]).all()) and bool(torch.isnan(a[B * L * Q:]).all()), 'wrote past the end'
    return i, o[:B * Q * idf].view(B, Q, idf), a[:B * L * Q].view(B, L, Q)


def check_fp8(i, ctx, att, with_att=True):
    """bit equality with the selected key column and with the probabilities 1 / 0; NaN where no word is live"""
    B, Q, idf = ctx.shape
    ok = i.word >= 0
    want = i.src.transpose(1, 2)[torch.arange(B)[:, None], i.word.clamp(min=0)]      # [B][Q][idf]
    assert torch.equal(torch.isnan(ctx), (~ok)[:, :, None].expand_as(ctx)), 'ctx: NaN placement'
    assert torch.equal(ctx[ok], want[ok]), 'ctx differs from the selected key column: max %g' % float((ctx[ok] - want[ok]).abs().max())
    if not with_att:
        assert bool(torch.isnan(att).all()), 'att = NULL, yet its buffer was written'
        return
    a = att.transpose(1, 2)                                 # [B][Q][L]
    one_hot = torch.nn.functional.one_hot(i.word.clamp(min=0), a.shape[2]).float()
    assert torch.equal(torch.isnan(a), (~ok)[:, :, None].expand_as(a)), 'att: NaN placement'
    assert torch.equal(a[ok], one_hot[ok]), 'att is not exactly 1 at the live word and 0 elsewhere'


@pytest.mark.parametrize('shape', R.FP8_EXACT, ids=lambda s: 'idf%d-B%d-Q%d-L%d-m%d' % s)
def test_fp8_exact(dev, shape):
    """the exact-layout check of test_kernels_gpu.test_word_attention_fp8 at idf = 64 (two context tiles) and at the
    tiles-per-wave shapes: e4m3-exact inputs, one live word per query, no tolerance"""
    check_fp8(*run_fp8(dev, shape))
    if shape[1] == R.B_SMALL:
        check_fp8(*run_fp8(dev, shape, with_att=False), with_att=False)


@pytest.mark.parametrize('shape', R.FP8_FULL, ids=lambda s: 'idf%d-B%d-Q%d-L%d-m%d' % s)
def test_fp8_fully_masked_row(dev, shape):
    check_fp8(*run_fp8(dev, shape, dead_row=R.FULL_ROW))


# ------------------------------------------------------------------ sba_word_attn_bwd
def run_backward(dev, case):
    i, mask, mode = R.case_inputs(case)
    B, Q, idf, L = case.B, case.Q, case.idf, case.L
    T = R.DTYPES[case.dt]
    dcs, dco = (2 * idf, idf) if case.sliced else (idf, 0)
    h, src, m8 = i.h.to(dev), i.src.to(dev), mask8(mask, dev)
    dfull = nans((B * Q + 3) * dcs, T, dev)                 # dctx in its slice; the other half and the tail hold NaN
    dfull.view(-1, dcs)[:B * Q, dco:dco + idf] = i.dctx.to(dev).view(B * Q, idf)
    dh = nans(B * Q * idf + PAD, T, dev)
    if case.acc:
        dh[:B * Q * idf] = i.prev.to(dev).flatten()
    dsrc, pre = prefilled(B * idf * L, R.TAG_DSRC, dev)
    lib().call('sba_word_attn_bwd', CODE[case.dt], p(h), p(src), p(m8), p(dfull), p(dh), p(dsrc), B, Q, idf, L, mode, dcs, dco,
               case.acc, stream())
    torch.cuda.synchronize()
    return NS(dh=dh, dsrc=dsrc, pre=pre)


def check_backward(r, case, ref, name):
    i, _, _ = R.case_inputs(case)
    B, Q, idf, L = case.B, case.Q, case.idf, case.L
    fam = R.family_of(case)
    prev = i.prev if case.acc else None
    dh = front(r.dh, B * Q * idf, name + ' dh').view(B, Q, idf)
    added = (front(r.dsrc, B * idf * L, name + ' dsrc') - r.pre).view(B, idf, L)
    report(name, R.bwd_ratios(fam, dh, added, ref, r.pre, prev))
    want = ref.dh + (prev.double() if case.acc else 0)
    if fam == 'f32':
        elem_close(dh, want, name + ' dh')
        sums_close(added, ref.dsrc, R.store_abs(Q, r.pre, ref.dsrc_abs), name + ' dsrc')
    else:
        low_close(dh.flatten(), want.flatten(), name + ' dh')


@pytest.mark.parametrize('case', R.BWD_SMALL + R.BWD_TPW + R.BWD_CHUNKS, ids=R.case_id)
def test_backward(dev, case):
    check_backward(run_backward(dev, case), case, backward_ref(case), 'bwd ' + R.case_id(case))


@pytest.mark.parametrize('case', R.BWD_DET, ids=R.case_id)
def test_backward_deterministic(dev, case):
    """det_part + sba_det_fold, more than one workgroup per image: the same bounds, dsrc still ADDED onto its prefill
    (the fold adds as the atomics do), and two runs bit-equal"""
    with deterministic(dev) as ops:
        r1, r2 = twice(ops, lambda: run_backward(dev, case))
    check_backward(r1, case, backward_ref(case), 'bwd, deterministic, ' + R.case_id(case))
    same_bits(r1.dh, r2.dh, 'dh'); same_bits(r1.dsrc, r2.dsrc, 'dsrc')


# ------------------------------------------------------------------ refusals
def _changes(V, idf, cs, co):
    return [('L = 0', dict(L=0)), ('L = 33', dict(L=33)), ('idf = 48', {'idf': 48, cs: 96}), ('mask_mode = 2', dict(mode=2)),
            ('mask_mode = -1', dict(mode=-1)), ('B = 0', dict(B=0)), ('Q = 0', dict(Q=0)), ('B = -1', dict(B=-1)),
            ('stride below idf + offset', {cs: idf, co: V}), ('stride not a multiple of V', {cs: idf + V + 1}),
            ('offset not a multiple of V', {cs: 2 * idf, co: 1}), ('unaligned offset, bytes', {cs: 2 * idf, co: V // 2})]


def test_refusals(dev):
    """every SBA_E_ARG condition of the three entry points: the call comes back refused and no output is written"""
    st = stream()
    idf = 32

    def ins(dt=F32):
        return torch.ones(BIG, dtype=dt, device=dev)

    def outs(dt=F32):
        return nans(BIG, dt, dev)

    def nulls(*keys):
        return [('%s = NULL' % k, {k: None}) for k in keys]
    m8 = torch.zeros(BIG, dtype=torch.uint8, device=dev)
    for dt, T, V in ((0, F32, 4), (1, torch.bfloat16, 8)):
        order = ['dt', 'h', 'src', 'mask', 'ctx', 'att', 'B', 'Q', 'idf', 'L', 'mode', 'cs', 'co', 'st']
        b = dict(dt=dt, h=ins(T), src=ins(), mask=m8, ctx=outs(T), att=outs(), B=2, Q=40, idf=idf, L=5, mode=1, cs=idf, co=0, st=st)
        _refuse('sba_word_attn_fwd', order, b, _changes(V, idf, 'cs', 'co') + nulls('h', 'src', 'ctx')
                + [('unknown dtype', dict(dt=7)), ('binary16 has no meaning here', dict(dt=2))], ['ctx', 'att'])
        order = ['dt', 'h', 'src', 'mask', 'dctx', 'dh', 'dsrc', 'B', 'Q', 'idf', 'L', 'mode', 'cs', 'co', 'acc', 'st']
        b = dict(dt=dt, h=ins(T), src=ins(), mask=m8, dctx=ins(T), dh=outs(T), dsrc=outs(), B=2, Q=40, idf=idf, L=5, mode=1,
                 cs=idf, co=0, acc=0, st=st)
        _refuse('sba_word_attn_bwd', order, b, _changes(V, idf, 'cs', 'co') + nulls('h', 'src', 'dctx', 'dh', 'dsrc')
                + [('idf = 128', dict(idf=128, cs=128)), ('unknown dtype', dict(dt=7)), ('binary16 has no meaning here', dict(dt=2))],
                ['dh', 'dsrc'])
    order = ['h', 'src', 'mask', 'ctx', 'att', 'B', 'Q', 'idf', 'L', 'mode', 'cs', 'co', 'st']
    b = dict(h=ins(torch.bfloat16), src=ins(), mask=m8, ctx=outs(torch.bfloat16), att=outs(), B=2, Q=40, idf=idf, L=5, mode=1,
             cs=idf, co=0, st=st)
    _refuse('sba_word_attn_fwd_fp8', order, b, _changes(8, idf, 'cs', 'co') + nulls('h', 'src', 'ctx')
            + [('idf = 128', dict(idf=128, cs=128))], ['ctx', 'att'])
