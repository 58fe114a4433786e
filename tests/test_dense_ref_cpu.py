"""(1) The float64 references of tests/dense_ref.py against float64 autograd through torch.nn.functional, to 1e-10:
the reference is trusted before a kernel is judged by it.  (2) Every case of tests/test_dense_kernels_gpu.py evaluated
with plain float32 torch on the CPU, against the bound the GPU test uses: the chosen inputs, not the kernel, keep a
float32 evaluation inside the bound (dot products: measured at most 2.5e-7 x the sum of the absolute summands, 40 x
inside 1e-5).  No GPU needed."""
import pytest
import torch
import torch.nn.functional as F

import dense_ref as R
from helpers import rel_l2
from oracle import fill

TOL = 1e-10
C_SUM = 1e-5                    # dot products: |error| <= C_SUM x the float64 sum of the absolute summands
RTOL, ATOL = 2e-4, 2e-5         # elementwise float32 outputs (test_kernels_gpu.tol(torch.float32))


def same(got, ref, name=''):
    got, ref = got.detach().double(), ref.detach().double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = float((got - ref).abs().max())
    assert err <= TOL * max(1.0, float(ref.abs().max())), '%s: max err %.3e' % (name, err)


def by_hand(fn, shape):
    """a tensor of `shape` filled element by element from a Python function of the index"""
    out = torch.empty(shape, dtype=torch.float64)
    for idx in torch.cartesian_prod(*[torch.arange(s) for s in shape]).reshape(-1, len(shape)).tolist():
        out[tuple(idx)] = fn(*idx)
    return out


# ------------------------------------------------------------------ (1) references against float64 autograd
@pytest.mark.parametrize('with_bias', [True, False])
def test_linear(with_bias):
    i = R.linear_inputs(5, 7, 6)
    x, w, b = (t.double().requires_grad_(True) for t in (i.x, i.w, i.bias))
    y = F.linear(x, w, b if with_bias else None)
    f = R.linear_fwd(i.x, i.w, i.bias if with_bias else None)
    same(f.y, y, 'y')
    y.backward(i.dy.double())
    r = R.linear_bwd(i.x, i.w, i.dy)
    same(r.dx, x.grad, 'dx'); same(r.dw, w.grad, 'dw')
    if with_bias:
        same(r.db, b.grad, 'db')
    # the sums of absolute summands, term by term
    xd, wd, dyd = i.x.double(), i.w.double(), i.dy.double()
    same(f.y_abs, by_hand(lambda bb, n: sum(abs(float(xd[bb, k] * wd[n, k])) for k in range(7))
                          + (abs(float(i.bias[n])) if with_bias else 0.0), (5, 6)), 'y_abs')
    same(r.dx_abs, by_hand(lambda bb, k: sum(abs(float(dyd[bb, n] * wd[n, k])) for n in range(6)), (5, 7)), 'dx_abs')
    same(r.dw_abs, by_hand(lambda n, k: sum(abs(float(dyd[bb, n] * xd[bb, k])) for bb in range(5)), (6, 7)), 'dw_abs')
    same(r.db_abs, dyd.abs().sum(0), 'db_abs')
    assert bool((f.y_abs >= f.y.abs() - 1e-12).all()) and bool((r.dw_abs >= r.dw.abs() - 1e-12).all())


def _ca_torch(h, eps):
    """model.py:281-294"""
    C = h.shape[1] // 4
    x = F.glu(h, 1)
    mu, logvar = x[:, :C], x[:, C:]
    return eps * torch.exp(0.5 * logvar) + mu, mu, logvar


@pytest.mark.parametrize('given', [(1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 0, 0)])
def test_ca(given):
    i = R.ca_inputs(3, 5)
    h = i.h.double().requires_grad_(True)
    c, mu, logvar = _ca_torch(h, i.eps.double())
    f = R.ca_fwd(i.h, i.eps)
    same(f.c, c, 'c'); same(f.mu, mu, 'mu'); same(f.logvar, logvar, 'logvar')
    grads = [g if on else None for g, on in zip((i.dc, i.dmu, i.dlogvar), given)]
    loss = sum((o * g.double()).sum() for o, g in zip((c, mu, logvar), grads) if g is not None)
    loss.backward()
    same(R.ca_bwd(i.h, i.eps, *grads), h.grad, 'dh')


def test_ctx_proj():
    i = R.ctx_inputs(2, 5, 6, 3)
    words, W = i.words.double().requires_grad_(True), i.W.double().requires_grad_(True)
    src = F.conv1d(words, W[:, :, None])                    # conv1x1 (GlobalAttention.py:75) on [B][cdf][L]
    f = R.ctx_proj_fwd(i.words, i.W)
    same(f.src, src, 'src')
    src.backward(i.dsrc.double())
    r = R.ctx_proj_bwd(i.words, i.W, i.dsrc)
    same(r.dW, W.grad, 'dW'); same(r.dwords, words.grad, 'dwords')
    wd, Wd, dd = i.words.double(), i.W.double(), i.dsrc.double()
    same(f.src_abs, by_hand(lambda b, o, l: sum(abs(float(Wd[o, c] * wd[b, c, l])) for c in range(6)), (2, 5, 3)), 'src_abs')
    same(r.dW_abs, by_hand(lambda o, c: sum(abs(float(dd[b, o, l] * wd[b, c, l])) for b in range(2) for l in range(3)),
                           (5, 6)), 'dW_abs')
    same(r.dwords_abs, by_hand(lambda b, c, l: sum(abs(float(Wd[o, c] * dd[b, o, l])) for o in range(5)), (2, 6, 3)),
         'dwords_abs')


def test_fc_bn_glu_eval():
    B, K, F2 = 3, 6, 32
    i = R.glu_inputs(B, K, F2)
    z = F.batch_norm(F.linear(i.x.double(), i.w.double()), i.rm.double(), i.rv.double(), i.gamma.double(), i.beta.double(),
                     False, 0.1, 1e-5)
    out = F.glu(z, 1).view(B, F2 // 16, 4, 4)               # INIT_STAGE_G: fc + view (model.py:353-356,372-373)
    same(R.fc_bn_glu_eval(i.x, i.w, i.gamma, i.beta, i.rm, i.rv), out.permute(0, 2, 3, 1).reshape(B, 16, F2 // 16), 'out')
    flat = F.glu(z, 1)
    got = R.fc_bn_glu_eval(i.x, i.w, i.gamma, i.beta, i.rm, i.rv)
    for f in (0, 15, 16, 31):                               # value feature f = channel f // 16, pixel f % 16
        same(got[:, f % 16, f // 16], flat[:, f], 'feature %d' % f)


# ------------------------------------------------------------------ (2) float32 on the CPU against the GPU bounds
def sums_inside(got, ref, ref_abs, name):
    worst = float(((got.double() - ref).abs() / ref_abs.clamp(min=1e-30)).max())
    print('%-40s float32 torch: worst |err| / sum|summands| = %.2e' % (name, worst))
    assert worst <= C_SUM, (name, worst)
    return worst


def elem_inside(got, ref, name):
    worst = float(((got.double() - ref).abs() / (ATOL + RTOL * ref.abs())).max())
    print('%-40s float32 torch: worst error / bound = %.3f' % (name, worst))
    assert worst <= 1.0, (name, worst)


@pytest.mark.parametrize('shape', sorted(set(R.LINEAR_FWD_MFMA + R.LINEAR_FWD_ROWS + R.LINEAR_BWD_SMALL + [R.LINEAR_BWD_WIDE]
                                             + R.LINEAR_BWD_FALLBACK + [(20, 200, 16384), (64, 256, 8200)])),
                         ids=lambda s: '%dx%dx%d' % s)
def test_float32_linear_is_inside_the_bound(shape):
    """every sba_linear_fwd / sba_linear_bwd shape of the GPU file, and the two large shapes the bound was measured on"""
    i = R.linear_inputs(*shape)
    f, r = R.linear_fwd(i.x, i.w, i.bias), R.linear_bwd(i.x, i.w, i.dy)
    worst = [sums_inside(F.linear(i.x, i.w, i.bias), f.y, f.y_abs, 'y'), sums_inside(i.dy @ i.w, r.dx, r.dx_abs, 'dx'),
             sums_inside(i.dy.t() @ i.x, r.dw, r.dw_abs, 'dw'), sums_inside(i.dy.sum(0), r.db, r.db_abs, 'db')]
    assert max(worst) <= C_SUM / 10, worst                  # an order of magnitude of room for another summation order


def test_float32_sum_added_to_the_prefill_is_inside_the_bound():
    """dw, dbias and dW are ADDED to a non-zero prefill; the GPU tests judge (stored - prefill) by the bound of the sum
    alone, although the stored float32 value is rounded once more (up to 3e-8 at a prefill of about 0.5).  On the prefills
    and inputs of every such case, the single-product sums of B = 1 and P = 1 included, float32 stays inside the bound:
    measured at most 1.9e-6 (sba_ctx_proj_bwd at (1, 32, 4, 1)), 5 x inside."""
    from test_norm_kernels_gpu import prefilled
    cpu = torch.device('cpu')

    def inside(n, tag, s, ref, ref_abs, name):
        buf, pre = prefilled(n, tag, cpu)
        stored = (buf[:n] + s.flatten()).double()
        return sums_inside(stored - pre, ref.flatten(), ref_abs.flatten(), name)
    worst = []
    for shape in R.LINEAR_BWD_SMALL + [R.LINEAR_BWD_WIDE] + R.LINEAR_BWD_FALLBACK:
        i = R.linear_inputs(*shape)
        r = R.linear_bwd(i.x, i.w, i.dy)
        worst.append(inside(r.dw.numel(), R.TAG_DW, i.dy.t() @ i.x, r.dw, r.dw_abs, 'dw %s' % (shape,)))
        worst.append(inside(r.db.numel(), R.TAG_DB, i.dy.sum(0), r.db, r.db_abs, 'db %s' % (shape,)))
    for shape in R.CTX_FWD_MFMA + R.CTX_BWD_DWORDS:
        i = R.ctx_inputs(*shape)
        r = R.ctx_proj_bwd(i.words, i.W, i.dsrc)
        worst.append(inside(r.dW.numel(), R.TAG_CTX_DW, torch.einsum('bil,bcl->ic', i.dsrc, i.words), r.dW, r.dW_abs,
                            'dW %s' % (shape,)))
    assert max(worst) <= C_SUM / 4, max(worst)


@pytest.mark.parametrize('shape', R.CA, ids=lambda s: '%dx%d' % s)
def test_float32_ca_is_inside_the_bound(shape):
    i = R.ca_inputs(*shape)
    f = R.ca_fwd(i.h, i.eps)
    c, mu, logvar = _ca_torch(i.h, i.eps)
    elem_inside(c, f.c, 'c'); elem_inside(mu, f.mu, 'mu'); elem_inside(logvar, f.logvar, 'logvar')
    h = i.h.clone().requires_grad_(True)
    c, mu, logvar = _ca_torch(h, i.eps)
    ((c * i.dc).sum() + (mu * i.dmu).sum() + (logvar * i.dlogvar).sum()).backward()
    elem_inside(h.grad, R.ca_bwd(i.h, i.eps, i.dc, i.dmu, i.dlogvar), 'dh')


@pytest.mark.parametrize('shape', sorted(set(R.CTX_FWD_MFMA + [R.CTX_VALU] + R.CTX_BWD_DWORDS)), ids=lambda s: '%dx%dx%dx%d' % s)
def test_float32_ctx_proj_is_inside_the_bound(shape):
    i = R.ctx_inputs(*shape)
    f, r = R.ctx_proj_fwd(i.words, i.W), R.ctx_proj_bwd(i.words, i.W, i.dsrc)
    sums_inside(torch.einsum('ic,bcl->bil', i.W, i.words), f.src, f.src_abs, 'src')
    sums_inside(torch.einsum('bil,bcl->ic', i.dsrc, i.words), r.dW, r.dW_abs, 'dW')
    sums_inside(torch.einsum('ic,bil->bcl', i.W, i.dsrc), r.dwords, r.dwords_abs, 'dwords')


@pytest.mark.parametrize('shape,zero', [(s, None) for s in R.CTX_FP8] + [(R.CTX_FP8_ZERO, 'words'), (R.CTX_FP8_ZERO, 'W')],
                         ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_fp8_inputs_are_exact(shape, zero):
    """integers in [-2, 2]: every product and every partial sum is an integer far below 2^24, so float32 in any order equals
    float64 -- the GPU test needs no tolerance; and e4m3 (4 exponent bits, 3 mantissa bits, largest value 448) holds every
    value times the tile's power-of-two scale (2 x 128 = 1 x 256 = 256)"""
    i = R.ctx_fp8_inputs(*shape, zero=zero)
    assert float(i.words.abs().max()) <= 2 and float(i.W.abs().max()) <= 2
    assert torch.equal(i.words, i.words.round()) and torch.equal(i.W, i.W.round())
    f = R.ctx_proj_fwd(i.words, i.W)
    assert torch.equal(torch.einsum('ic,bcl->bil', i.W, i.words).double(), f.src)
    assert float(f.src_abs.max()) < 2 ** 24
    B, idf, cdf, L = shape
    if zero == 'words':
        assert float(i.words.permute(0, 2, 1).reshape(B * L, cdf)[:32].abs().max()) == 0
        assert float(i.words.permute(0, 2, 1).reshape(B * L, cdf)[32:].abs().max()) > 0
    if zero == 'W':
        assert float(i.W[32:64].abs().max()) == 0 and float(i.W[:32].abs().max()) > 0


def fold_f32(i, eps=1e-5):
    """sba_fold_bn_pack in float32: w' = w * s, bias = beta - mean * s, s = gamma / sqrt(var + eps)"""
    s = i.gamma / torch.sqrt(i.rv + eps)
    return i.w * s[:, None], i.beta - i.rm * s


@pytest.mark.parametrize('shape', R.GLU, ids=lambda s: '%dx%dx%d' % s)
def test_float32_fc_bn_glu_is_inside_the_bound(shape):
    from norm_ref import to_nhwc16
    i = R.glu_inputs(*shape)
    ref = R.fc_bn_glu_eval(i.x, i.w, i.gamma, i.beta, i.rm, i.rv)
    w, b = fold_f32(i)
    out = to_nhwc16(F.glu(F.linear(i.x, w, b), 1))
    elem_inside(out, ref, 'glu out, f32')
    if shape == R.GLU_BF16:                                 # one rounding of the float32 value: at the floor, bound 2 x
        floor = rel_l2(ref.to(torch.bfloat16).double(), ref)
        r = rel_l2(out.to(torch.bfloat16).double(), ref)
        print('glu out, bf16: rel L2 %.3e, one-rounding floor %.3e' % (r, floor))
        assert r <= 2 * floor
