"""Every entry point of csrc/linear.hip called directly through the C ABI (sbagan._lib), at the smallest shape that
reaches each kernel and each arm of the host dispatch, against the float64 references of tests/dense_ref.py evaluated
on the kernel's own f32 inputs.  Shapes are (B, K, N), (B, C), (B, idf, cdf, L) and (B, K, F2).

kernel                         host condition that selects it                          covered by
-----------------------------  ------------------------------------------------------  ------------------------------------
linear_fwd_mfma_kernel         sba_linear_fwd: B <= 32 and K % 4 == 0                  test_linear_fwd: (1, 4, 1), (32, 36, 33)
                                                                                       (partial 8-vector group, last tile
                                                                                       one column), (20, 100, 400), (31,
                                                                                       256, 31); bias and bias = NULL
linear_fwd_kernel              sba_linear_fwd otherwise (B * K * 4 <= 64 KB)           test_linear_fwd: (33, 64, 37), (20,
                                                                                       102, 40) (K % 4), (33, 8, 8200) (grid-
                                                                                       stride wrap), (64, 256, 5) (64 KB LDS)
linear_bwd_xw_mfma_kernel      sba_linear_bwd: B <= 32, N % 4 == 0, N <= 2048,         test_linear_bwd_small: (20, 100, 400),
                               dx and dw                                               (32, 33, 36), (1, 4, 4); dbias = NULL
linear_bwd_w_mfma_kernel       same shapes, dw without dx; N > 2048 and N % 32 == 0    test_linear_bwd_small (dw + dbias call),
                                                                                       test_linear_bwd_wide
linear_bwd_x_mfma_kernel
  one slice, plain stores      same shapes, dx without dw                              test_linear_bwd_small (dx-only call):
                                                                                       bit-equal to the combined launch
  128-column slices, atomics   N > 2048, N % 32 == 0, default mode                     test_linear_bwd_wide: (3, 40, 2080)
                                                                                       (last slice 32 columns), and dx-only
  one slice, N > 2048          the same, deterministic mode                            test_linear_bwd_wide_deterministic
  512-column slices, fallback  fallback arm and dx && B <= 32 && N % 32 == 0:          not reachable, not tested
                               needs N / 32 > 65535, N >= 2,097,152
linear_bwd_w_kernel            sba_linear_bwd otherwise (fallback), dw                 test_linear_bwd_fallback
linear_bwd_x_kernel            fallback, dx; nper = 4 / 16 / 64 by N                   test_linear_bwd_fallback: (33, 16, 7),
                                                                                       (33, 16, 516), (33, 16, 4100); (20, 100,
                                                                                       402) (N % 4), (4, 16, 2052) (N > 2048,
                                                                                       N % 32); dx-only and dw-only calls
  nper = N (one workgroup)     fallback, deterministic mode                            test_linear_bwd_fallback_deterministic
ca_fwd_kernel                  sba_ca_fwd (always)                                     test_ca: (1, 1), (3, 100), (5, 257)
ca_bwd_kernel                  sba_ca_bwd; dc / dmu / dlogvar each optional            test_ca: all three, each NULL in turn
ctx_proj_fwd_mfma_kernel       sba_ctx_proj_fwd: cdf % 4 == 0                          test_ctx_proj_fwd: (1, 32, 4, 1), (3, 48,
                                                                                       100, 7), (2, 64, 256, 18), (5, 32, 256, 32)
ctx_proj_fwd_kernel            sba_ctx_proj_fwd: cdf % 4 != 0                          test_ctx_proj_fwd: (2, 5, 6, 3)
ctx_proj_fwd_fp8_kernel        sba_ctx_proj_fwd_fp8 (cdf % 16 == 0)                    test_ctx_proj_fwd_fp8_exact: (1, 32, 16,
  amax = 0 -> scale 1          an all-zero 32-row tile of the words or of W            1), (3, 48, 48, 7), (2, 64, 256, 18); the
                                                                                       last with a zero tile of either operand
ctx_proj_bwd_w_mfma_kernel     sba_ctx_proj_bwd: dwords = NULL                         test_ctx_proj_bwd: the four matrix-core
                                                                                       forward shapes (P = 1, 21, 36, 160)
ctx_proj_bwd_kernel            sba_ctx_proj_bwd: dwords given                          test_ctx_proj_bwd: (2, 5, 6, 3), (3, 32,
                                                                                       256, 7)
linear_glu_mfma_kernel<T, 1>   sba_linear_glu_fwd: K % 4 == 0; T = f32 / bf16          test_linear_glu: (1, 4, 16), (33, 100, 48)
                                                                                       (two batch tiles, 1.5 feature tiles,
                                                                                       partial 4-vector group; f32 and bf16)
linear_glu_mfma_kernel<T, 0>   sba_linear_glu_fwd: K % 4 != 0                          test_linear_glu: (20, 102, 32)
every SBA_E_ARG condition      --                                                      test_refusals

No environment switch selects a kernel: the shape, the NULL outputs and the deterministic mode do.

Bounds (the project's own, tests/test_norm_kernels_gpu.py).  Dot-product outputs (y, dx, dw, db, src, dW, dwords):
|error| <= 1e-5 x the float64 sum of the ABSOLUTE summands of that element (one dropped term of a 16384-term sum is
about 6e-5 of it, a dropped 4-element K tail at K = 100 about 4e-2; plain f32 is at most 3e-7: test_dense_ref_cpu).
Elementwise f32 outputs (ca_*, the f32 GLU output): rtol 2e-4 / atol 2e-5.  The bf16 GLU output: relative L2 at most
twice the one-rounding floor.  The FP8 projection on integers in [-2, 2]: equal to the f32 kernel and to float64, no
tolerance.  For N <= 2048 the split dx-only / dw-only calls of ops.LinearFn are bit-equal to the combined launch.

entry point            worst measured error / bound (MI355X)
---------------------  ----------------------------------------------------------------------------------------------
sba_linear_fwd         0.018  (1.84e-7 of sum |summands|: y at (20, 100, 400) without bias)
sba_linear_bwd         0.115  (1.15e-6: dw at (3, 40, 2080), B = 3 terms added to the prefill); dx 0.017, db 0.012
sba_ca_fwd             0.005  (c at (5, 257))
sba_ca_bwd             0.002
sba_ctx_proj_fwd       0.022  (2.23e-7: src at (5, 32, 256, 32))
sba_ctx_proj_bwd       0.194  (1.94e-6: dW at (1, 32, 4, 1), ONE product added to the prefill); dwords 0.015
sba_ctx_proj_fwd_fp8   exact  (no tolerance)
sba_linear_glu_fwd     0.008  (f32, (33, 100, 48));  bf16: rel L2 1.000 x the one-rounding floor = 0.50 of the bound

Every output buffer is longer than the kernel should write and is prefilled with NaN -- dw, dbias and dW, which the
kernels add to, with non-zero values in front of a NaN tail; everything outside the written range must still be NaN
afterwards and everything inside finite.  An output passed as NULL has a buffer of its own that must be untouched.
"""
from types import SimpleNamespace as NS

import pytest
import torch

pytestmark = pytest.mark.gpu

import dense_ref as R  # noqa: E402
from test_kernels_gpu import _reset_cfg, dev  # noqa: E402,F401
from test_norm_kernels_gpu import (BIG, PAD, _refuse, deterministic, elem_close, front, lib, low_close, nans, p, prefilled,  # noqa: E402
                                   same_bits, stream, sums_close, twice)

F32 = torch.float32


def name_of(entry, shape, what):
    return '%s %s %s' % (entry, 'x'.join(map(str, shape)), what)


def untouched_nan(buf, name):
    assert bool(torch.isnan(buf).all()), '%s = NULL, yet its buffer was written' % name


def added_close(buf, n, pre, ref, ref_abs, name):
    """an output the kernel ADDS its sum to, prefilled with `pre`: (stored - pre) against the sum, at the dot-product
    bound of the sum alone.  (The stored f32 value pre + sum is rounded once more than the sum, by up to 3e-8 at |pre|
    about 0.5; test_dense_ref_cpu shows that on these prefills and inputs f32 stays 5 x inside the bound even where a
    sum is a single small product, B = 1 or P = 1.)"""
    sums_close(front(buf, n, name) - pre, ref, ref_abs, name)


# ------------------------------------------------------------------ sba_linear_fwd
@pytest.mark.parametrize('with_bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('shape', R.LINEAR_FWD_MFMA + R.LINEAR_FWD_ROWS, ids=lambda s: '%dx%dx%d' % s)
def test_linear_fwd(dev, shape, with_bias):
    B, K, N = shape
    i = R.linear_inputs(B, K, N)
    x, w = i.x.to(dev), i.w.to(dev)
    bias = i.bias.to(dev) if with_bias else None
    y = nans(B * N + PAD, F32, dev)
    lib().call('sba_linear_fwd', p(x), p(w), p(bias), p(y), B, K, N, stream())
    torch.cuda.synchronize()
    ref = R.linear_fwd(i.x, i.w, i.bias if with_bias else None)
    sums_close(front(y, B * N, 'y'), ref.y, ref.y_abs, name_of('linear_fwd', shape, 'y'))


# ------------------------------------------------------------------ sba_linear_bwd
def run_linear_bwd(dev, shape, want=('dx', 'dw', 'db')):
    """one sba_linear_bwd call with the outputs in `want`; the others are passed as NULL and keep a buffer of their own"""
    B, K, N = shape
    i = R.linear_inputs(B, K, N)
    r = NS(shape=shape, want=want, i=i)
    x, w, dy = i.x.to(dev), i.w.to(dev), i.dy.to(dev)
    r.dx = nans(B * K + PAD, F32, dev)
    r.dw, r.dw0 = prefilled(N * K, R.TAG_DW, dev)
    r.db, r.db0 = prefilled(N, R.TAG_DB, dev)
    lib().call('sba_linear_bwd', p(x), p(w), p(dy), p(r.dx) if 'dx' in want else None, p(r.dw) if 'dw' in want else None,
               p(r.db) if 'db' in want else None, B, K, N, stream())
    torch.cuda.synchronize()
    return r


def check_linear_bwd(r, what=''):
    B, K, N = r.shape
    ref = R.linear_bwd(r.i.x, r.i.w, r.i.dy)
    if 'dx' in r.want:
        sums_close(front(r.dx, B * K, 'dx'), ref.dx, ref.dx_abs, name_of('linear_bwd', r.shape, what + 'dx'))
    else:
        untouched_nan(r.dx, 'dx')
    for k, n, g, g_abs in (('dw', N * K, ref.dw, ref.dw_abs), ('db', N, ref.db, ref.db_abs)):
        if k in r.want:                                     # the kernels ADD to dw / dbias
            added_close(getattr(r, k), n, getattr(r, k + '0'), g, g_abs, name_of('linear_bwd', r.shape, what + k))
        else:
            assert torch.equal(front(getattr(r, k), n, k), getattr(r, k + '0')), '%s = NULL, yet its buffer was written' % k


@pytest.mark.parametrize('shape', R.LINEAR_BWD_SMALL, ids=lambda s: '%dx%dx%d' % s)
def test_linear_bwd_small(dev, shape):
    """N <= 2048: the combined launch, the combined launch without dbias, and the two calls ops.LinearFn issues when
    the weight gradient goes to the companion stream -- the same device functions, one slice, no atomics: bit-equal"""
    both = run_linear_bwd(dev, shape)
    check_linear_bwd(both, 'combined ')
    check_linear_bwd(run_linear_bwd(dev, shape, ('dx', 'dw')), 'combined, dbias = NULL ')
    only_x = run_linear_bwd(dev, shape, ('dx',))            # dx, prefilled with NaN, is overwritten
    check_linear_bwd(only_x, 'dx-only ')
    only_w = run_linear_bwd(dev, shape, ('dw', 'db'))
    check_linear_bwd(only_w, 'dw-only ')
    check_linear_bwd(run_linear_bwd(dev, shape, ('dw',)), 'dw-only, dbias = NULL ')
    same_bits(only_x.dx, both.dx, 'dx: split call against the combined launch')
    same_bits(only_w.dw, both.dw, 'dw: split call against the combined launch')
    same_bits(only_w.db, both.db, 'dbias: split call against the combined launch')


def test_linear_bwd_wide(dev):
    """N > 2048, N % 32 == 0: dW on the matrix cores, dx over 128-column slices (17 of them, the last 32 columns wide)
    with f32 atomics into a dx the entry point clears itself"""
    shape = R.LINEAR_BWD_WIDE
    check_linear_bwd(run_linear_bwd(dev, shape), 'wide ')
    check_linear_bwd(run_linear_bwd(dev, shape, ('dx',)), 'wide dx-only ')
    check_linear_bwd(run_linear_bwd(dev, shape, ('dw', 'db')), 'wide dw-only ')


def _bits_of(r1, r2):
    for k in ('dx', 'dw', 'db'):
        same_bits(getattr(r1, k), getattr(r2, k), k)


def test_linear_bwd_wide_deterministic(dev):
    with deterministic(dev) as ops:                         # one slice over all 2080 columns, plain stores
        r1, r2 = twice(ops, lambda: run_linear_bwd(dev, R.LINEAR_BWD_WIDE))
    check_linear_bwd(r1, 'wide, deterministic ')
    _bits_of(r1, r2)


@pytest.mark.parametrize('shape', R.LINEAR_BWD_FALLBACK, ids=lambda s: '%dx%dx%d' % s)
def test_linear_bwd_fallback(dev, shape):
    check_linear_bwd(run_linear_bwd(dev, shape), 'fallback ')
    check_linear_bwd(run_linear_bwd(dev, shape, ('dx',)), 'fallback dx-only ')
    check_linear_bwd(run_linear_bwd(dev, shape, ('dw', 'db')), 'fallback dw-only ')
    check_linear_bwd(run_linear_bwd(dev, shape, ('dx', 'dw')), 'fallback, dbias = NULL ')


def test_linear_bwd_fallback_deterministic(dev):
    with deterministic(dev) as ops:                         # linear_bwd_x_kernel as ONE workgroup
        r1, r2 = twice(ops, lambda: run_linear_bwd(dev, R.LINEAR_BWD_FALLBACK_DET))
    check_linear_bwd(r1, 'fallback, deterministic ')
    _bits_of(r1, r2)


# ------------------------------------------------------------------ sba_ca_fwd / sba_ca_bwd
@pytest.mark.parametrize('shape', R.CA, ids=lambda s: '%dx%d' % s)
def test_ca(dev, shape):
    B, C = shape
    i = R.ca_inputs(B, C)
    h, eps = i.h.to(dev), i.eps.to(dev)
    c, mu, logvar = (nans(B * C + PAD, F32, dev) for _ in range(3))
    lib().call('sba_ca_fwd', p(h), p(eps), p(c), p(mu), p(logvar), B, C, stream())
    torch.cuda.synchronize()
    ref = R.ca_fwd(i.h, i.eps)
    for k, buf in (('c', c), ('mu', mu), ('logvar', logvar)):
        elem_close(front(buf, B * C, k), getattr(ref, k), name_of('ca_fwd', shape, k))
    grads = dict(dc=i.dc, dmu=i.dmu, dlogvar=i.dlogvar)
    for absent in (None, 'dc', 'dmu', 'dlogvar'):
        given = {k: (None if k == absent else v) for k, v in grads.items()}
        on_dev = {k: (None if v is None else v.to(dev)) for k, v in given.items()}
        dh = nans(B * 4 * C + PAD, F32, dev)
        lib().call('sba_ca_bwd', p(h), p(eps), p(on_dev['dc']), p(on_dev['dmu']), p(on_dev['dlogvar']), p(dh), B, C, stream())
        torch.cuda.synchronize()
        elem_close(front(dh, B * 4 * C, 'dh'), R.ca_bwd(i.h, i.eps, **given),
                   name_of('ca_bwd', shape, 'dh, %s = NULL' % absent if absent else 'dh'))


# ------------------------------------------------------------------ sba_ctx_proj_fwd / _bwd
@pytest.mark.parametrize('shape', R.CTX_FWD_MFMA + [R.CTX_VALU], ids=lambda s: '%dx%dx%dx%d' % s)
def test_ctx_proj_fwd(dev, shape):
    B, idf, cdf, L = shape
    i = R.ctx_inputs(*shape)
    words, W = i.words.to(dev), i.W.to(dev)
    src = nans(B * idf * L + PAD, F32, dev)
    lib().call('sba_ctx_proj_fwd', p(words), p(W), p(src), B, idf, cdf, L, stream())
    torch.cuda.synchronize()
    ref = R.ctx_proj_fwd(i.words, i.W)
    sums_close(front(src, B * idf * L, 'src'), ref.src, ref.src_abs, name_of('ctx_proj_fwd', shape, 'src'))


@pytest.mark.parametrize('shape,with_dwords', [(s, False) for s in R.CTX_FWD_MFMA] + [(s, True) for s in R.CTX_BWD_DWORDS],
                         ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else 'dwords%d' % v)
def test_ctx_proj_bwd(dev, shape, with_dwords):
    B, idf, cdf, L = shape
    i = R.ctx_inputs(*shape)
    words, W, dsrc = i.words.to(dev), i.W.to(dev), i.dsrc.to(dev)
    dW, dW0 = prefilled(idf * cdf, R.TAG_CTX_DW, dev)                 # the kernels ADD to dW
    dwords = nans(B * cdf * L + PAD, F32, dev)
    lib().call('sba_ctx_proj_bwd', p(words), p(W), p(dsrc), p(dW), p(dwords) if with_dwords else None, B, idf, cdf, L, stream())
    torch.cuda.synchronize()
    ref = R.ctx_proj_bwd(i.words, i.W, i.dsrc)
    added_close(dW, idf * cdf, dW0, ref.dW, ref.dW_abs, name_of('ctx_proj_bwd', shape, 'dW'))
    if with_dwords:
        sums_close(front(dwords, B * cdf * L, 'dwords'), ref.dwords, ref.dwords_abs, name_of('ctx_proj_bwd', shape, 'dwords'))
    else:
        untouched_nan(dwords, 'dwords')


# ------------------------------------------------------------------ sba_ctx_proj_fwd_fp8
@pytest.mark.parametrize('shape,zero', [(s, None) for s in R.CTX_FP8] + [(R.CTX_FP8_ZERO, 'words'), (R.CTX_FP8_ZERO, 'W')],
                         ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_ctx_proj_fwd_fp8_exact(dev, shape, zero):
    """integers in [-2, 2] (test_attention_key_projection_fp8): e4m3 holds them times the tile's power-of-two scale
    exactly, so the FP8 kernel equals the f32 kernel and the float64 einsum -- no tolerance.  zero: one whole 32-row
    tile of the words, or of W, is zero (amax = 0 -> scale 1)."""
    B, idf, cdf, L = shape
    i = R.ctx_fp8_inputs(*shape, zero=zero)
    words, W = i.words.to(dev), i.W.to(dev)
    n = B * idf * L
    got, f32 = nans(n + PAD, F32, dev), nans(n + PAD, F32, dev)
    lib().call('sba_ctx_proj_fwd', p(words), p(W), p(f32), B, idf, cdf, L, stream())
    lib().call('sba_ctx_proj_fwd_fp8', p(words), p(W), p(got), B, idf, cdf, L, stream())
    torch.cuda.synchronize()
    ref = R.ctx_proj_fwd(i.words, i.W).src.flatten()
    assert torch.equal(front(f32, n, 'src (f32 kernel)'), ref), 'the f32 kernel differs from float64 on integer data'
    g = front(got, n, 'src (fp8 kernel)')
    assert torch.equal(g, ref), 'fp8 %s zero=%s: max difference %g' % (shape, zero, float((g - ref).abs().max()))


# ------------------------------------------------------------------ sba_linear_glu_fwd
@pytest.mark.parametrize('shape,mode', [(s, 'f32') for s in R.GLU] + [(R.GLU_BF16, 'bf16')],
                         ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else v)
def test_linear_glu(dev, shape, mode):
    """operands packed by sba_fold_bn_pack(glu = 1) as sbagan.infer._fold does: 64 * ceil(F2 / 32) rows, value and gate
    granules interleaved, rows of features >= F2 zero"""
    B, K, F2 = shape
    code, T = (0, F32) if mode == 'f32' else (1, torch.bfloat16)
    i = R.glu_inputs(B, K, F2)
    x, w, gamma, beta, rm, rv = (t.to(dev) for t in (i.x, i.w, i.gamma, i.beta, i.rm, i.rv))
    rows = 64 * ((F2 + 31) // 32)
    wp, bias = nans(rows * K + PAD, F32, dev), nans(rows + PAD, F32, dev)
    lib().call('sba_fold_bn_pack', 0, p(w), p(gamma), p(beta), p(rm), p(rv), R.EPS, p(wp), p(bias), 2 * F2, 1, K, 1, stream())
    out = nans(B * F2 + PAD, T, dev)
    lib().call('sba_linear_glu_fwd', code, p(x), p(wp), p(bias), p(out), B, K, F2, stream())
    torch.cuda.synchronize()
    front(wp, rows * K, 'packed weights'); front(bias, rows, 'packed bias')
    ref = R.fc_bn_glu_eval(i.x, i.w, i.gamma, i.beta, i.rm, i.rv)
    got = front(out, B * F2, 'out')
    if mode == 'f32':
        elem_close(got, ref, name_of('linear_glu_fwd', shape, 'out (NHWC)'))
    else:
        low_close(got, ref.flatten(), name_of('linear_glu_fwd', shape, 'out (NHWC)'))


# ------------------------------------------------------------------ refusals
def test_refusals(dev):
    """every SBA_E_ARG condition of the eight entry points: the call comes back refused and no output is written"""
    st = stream()

    def ins():
        return torch.ones(BIG, dtype=F32, device=dev)

    def outs(dt=F32):
        return nans(BIG, dt, dev)

    def nulls(*keys):
        return [('%s = NULL' % k, {k: None}) for k in keys]

    def dims(*keys):
        return [('%s = 0' % k, {k: 0}) for k in keys] + [('%s = -1' % k, {k: -1}) for k in keys]
    lds = [('B * K * 4 > 64 KB in the wave-per-row arm', dict(B=65, K=256, N=4))]

    b = dict(x=ins(), w=ins(), bias=ins(), y=outs(), B=4, K=8, N=8, st=st)
    _refuse('sba_linear_fwd', ['x', 'w', 'bias', 'y', 'B', 'K', 'N', 'st'], b, nulls('x', 'w', 'y') + dims('B', 'K', 'N') + lds, ['y'])

    order = ['x', 'w', 'dy', 'dx', 'dw', 'db', 'B', 'K', 'N', 'st']
    for shape in (dict(B=4, K=8, N=8), dict(B=33, K=8, N=8)):            # a matrix-core shape and a fallback shape
        b = dict(x=ins(), w=ins(), dy=ins(), dx=outs(), dw=outs(), db=outs(), st=st, **shape)
        _refuse('sba_linear_bwd', order, b, nulls('x', 'w', 'dy') + dims('B', 'K', 'N') + lds + [
            ('dbias without dw (dbias is summed by the dw kernels)', dict(dw=None)),
            ('dbias alone', dict(dw=None, dx=None))], ['dx', 'dw', 'db'])

    b = dict(h=ins(), eps=ins(), c=outs(), mu=outs(), lv=outs(), B=3, C=5, st=st)
    _refuse('sba_ca_fwd', ['h', 'eps', 'c', 'mu', 'lv', 'B', 'C', 'st'], b, nulls('h', 'eps', 'c', 'mu', 'lv') + dims('B', 'C'),
            ['c', 'mu', 'lv'])
    b = dict(h=ins(), eps=ins(), dc=ins(), dmu=ins(), dlv=ins(), dh=outs(), B=3, C=5, st=st)
    _refuse('sba_ca_bwd', ['h', 'eps', 'dc', 'dmu', 'dlv', 'dh', 'B', 'C', 'st'], b, nulls('h', 'eps', 'dh') + dims('B', 'C'), ['dh'])

    order = ['words', 'W', 'src', 'B', 'idf', 'cdf', 'L', 'st']
    for cdf in (16, 6):                                     # the matrix-core arm and the VALU arm
        b = dict(words=ins(), W=ins(), src=outs(), B=2, idf=5, cdf=cdf, L=3, st=st)
        _refuse('sba_ctx_proj_fwd', order, b, nulls('words', 'W', 'src') + dims('B', 'idf', 'cdf', 'L'), ['src'])
    b = dict(words=ins(), W=ins(), src=outs(), B=2, idf=5, cdf=16, L=3, st=st)
    _refuse('sba_ctx_proj_fwd_fp8', order, b, nulls('words', 'W', 'src') + dims('B', 'idf', 'cdf', 'L') + [
        ('cdf % 16 != 0', dict(cdf=24)), ('cdf % 16 != 0', dict(cdf=8))], ['src'])
    order = ['words', 'W', 'dsrc', 'dW', 'dwords', 'B', 'idf', 'cdf', 'L', 'st']
    for with_dwords in (True, False):
        b = dict(words=ins(), W=ins(), dsrc=ins(), dW=outs(), dwords=outs() if with_dwords else None, B=2, idf=5, cdf=16, L=3, st=st)
        _refuse('sba_ctx_proj_bwd', order, b, nulls('words', 'W', 'dsrc', 'dW') + dims('B', 'idf', 'cdf', 'L'),
                ['dW', 'dwords'] if with_dwords else ['dW'])

    order = ['dt', 'x', 'wp', 'bias', 'out', 'B', 'K', 'F2', 'st']
    for code, T, K in ((0, F32, 8), (1, torch.bfloat16, 8), (0, F32, 6)):
        b = dict(dt=code, x=ins(), wp=ins(), bias=ins(), out=outs(T), B=3, K=K, F2=32, st=st)
        _refuse('sba_linear_glu_fwd', order, b, nulls('x', 'wp', 'bias', 'out') + dims('B', 'K', 'F2') + [
            ('F2 % 16 != 0', dict(F2=24)), ('F2 % 16 != 0', dict(F2=40)), ('unknown dtype', dict(dt=7)),
            ('binary16 y has no meaning here', dict(dt=2)), ('more than 65535 batch tiles', dict(B=65535 * 32 + 1))], ['out'])
