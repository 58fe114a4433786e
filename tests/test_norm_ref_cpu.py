"""The float64 references of tests/norm_ref.py against float64 autograd through torch.nn.functional,
to 1e-10: the reference is trusted before a kernel is judged by it.  No GPU needed."""
import pytest
import torch
import torch.nn.functional as F

import norm_ref as R
from oracle import fill

TOL = 1e-10


def same(got, ref, name=''):
    got, ref = (t.detach().double() if torch.is_tensor(t) else torch.tensor(t, dtype=torch.float64) for t in (got, ref))
    err = float((got - ref).abs().max())
    assert err <= TOL * max(1.0, float(ref.abs().max())), '%s: max err %.3e' % (name, err)


def _inputs(G, rows, C, Co, tag=1, offset=0.0):
    y = (offset + fill.unit((G, rows, C), tag)).double()
    dout = fill.unit((G, rows, Co), tag + 1).double()
    gamma = (1 + 0.3 * fill.unit((C,), tag + 2)).double()
    beta = (0.2 * fill.unit((C,), tag + 3)).double()
    return y, dout, gamma, beta


def _torch_act(z, act):
    """z NCHW-like [R][C]"""
    if act == R.ACT_GLU:
        return F.glu(z, 1)
    if act == R.ACT_LRELU:
        return F.leaky_relu(z, 0.2)
    if act == R.ACT_RELU:
        return F.relu(z)
    return z


def test_bn_stats():
    y = fill.unit((2, 37, 12), 3).double()
    r = R.bn_stats(y)
    for g in range(2):
        for c in range(12):
            same(r.sums[g, 0, c], sum(float(v) for v in y[g, :, c]), 'sum')
            same(r.sums[g, 1, c], sum(float(v) ** 2 for v in y[g, :, c]), 'sumsq')
    assert bool((r.sums_abs[:, 0] >= r.sums[:, 0].abs()).all())


@pytest.mark.parametrize('act,residual', [(R.ACT_NONE, False), (R.ACT_NONE, True), (R.ACT_GLU, False),
                                          (R.ACT_LRELU, False), (R.ACT_LRELU, True), (R.ACT_RELU, False)])
@pytest.mark.parametrize('G', [1, 2])
def test_bn_act_forward_backward_train(act, G, residual):
    rows, C = 53, 16
    Co = C // 2 if act == R.ACT_GLU else C
    y, dout, gamma, beta = _inputs(G, rows, C, Co, offset=0.7)
    res = fill.unit((G, rows, Co), 9).double() if residual else None
    rm0, rv0 = (0.1 * fill.unit((C,), 7)).double(), (1 + 0.2 * fill.unit((C,), 8)).double()
    got = R.bn_act_fwd(y, gamma, beta, rm0, rv0, 5, act, residual=res)
    # torch: G consecutive module calls
    yt, gt, bt = y.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm, rv = rm0.clone(), rv0.clone()
    outs = []
    for g in range(G):
        z = F.batch_norm(yt[g], rm, rv, gt, bt, True, 0.1, 1e-5)
        o = _torch_act(z, act)
        outs.append(o + res[g] if residual else o)
    out = torch.stack(outs)
    same(got.out, out, 'out'); same(got.running_mean, rm, 'running_mean'); same(got.running_var, rv, 'running_var')
    assert got.nbt == 5 + G
    for g in range(G):
        mean, var = y[g].mean(0), y[g].var(0, unbiased=False)
        same(got.aux[g, 2], mean, 'mean'); same(got.aux[g, 3], (var + 1e-5).rsqrt(), 'rstd')
        same(y[g] * got.aux[g, 0] + got.aux[g, 1], F.batch_norm(y[g], None, None, gamma, beta, True, 0.1, 1e-5), 'scale/shift')
    if act == R.ACT_RELU:
        return      # (no backward entry point for ReLU: the Inception trunk's backward masks with sba_relu_bwd first)
    out.backward(dout)
    b = R.bn_act_bwd(y, dout, got.aux, gamma, beta, act)
    same(b.dy, yt.grad, 'dy'); same(b.dgamma, gt.grad, 'dgamma'); same(b.dbeta, bt.grad, 'dbeta')
    assert bool((b.red_abs >= b.red.abs()).all())
    same(b.red[:, 1].sum(0), gt.grad, 'red1'); same(b.red[:, 0].sum(0), bt.grad, 'red0')
    if act == R.ACT_LRELU:      # the branch taken, passed in explicitly, gives the same result
        pos = (out - (res if residual else 0)) > 0
        same(R.bn_act_bwd(y, dout, got.aux, gamma, beta, act, positive=pos).dy, yt.grad, 'dy (explicit mask)')


@pytest.mark.parametrize('act', [R.ACT_NONE, R.ACT_GLU, R.ACT_LRELU, R.ACT_RELU])
def test_bn_act_forward_eval(act):
    rows, C = 29, 16
    y, _, gamma, beta = _inputs(1, rows, C, C, tag=20)
    rm0, rv0 = (0.3 * fill.unit((C,), 7)).double(), (1 + 0.2 * fill.unit((C,), 8)).double()
    got = R.bn_act_fwd(y, gamma, beta, rm0, rv0, 4, act, training=False)
    same(got.out[0], _torch_act(F.batch_norm(y[0], rm0, rv0, gamma, beta, False, 0.1, 1e-5), act), 'out')
    same(got.running_mean, rm0); same(got.running_var, rv0)
    assert got.nbt == 4
    same(got.aux[0, 2], rm0); same(got.aux[0, 3], (rv0 + 1e-5).rsqrt())


@pytest.mark.parametrize('B', [2, 20, 33])
def test_bn1d_glu(B):
    Fdim = 64
    y = fill.unit((B, Fdim), 30).double().requires_grad_(True)
    gamma = (1 + 0.3 * fill.unit((Fdim,), 31)).double().requires_grad_(True)
    beta = (0.2 * fill.unit((Fdim,), 32)).double().requires_grad_(True)
    rm, rv = torch.zeros(Fdim).double(), torch.ones(Fdim).double()
    got = R.bn1d_glu_fwd(y, gamma, beta, rm, rv, 0)
    out = F.glu(F.batch_norm(y, rm, rv, gamma, beta, True, 0.1, 1e-5), 1).view(B, Fdim // 32, 4, 4)   # INIT_STAGE_G.fc + view
    nhwc = out.permute(0, 2, 3, 1).reshape(B, 16, Fdim // 32)
    same(got.out, nhwc, 'out'); same(got.running_mean, rm); same(got.running_var, rv)
    assert got.nbt == 1
    dnhwc = fill.unit((B, 16, Fdim // 32), 33).double()
    nhwc.backward(dnhwc)
    b = R.bn1d_glu_bwd(y, dnhwc, gamma, beta, got.mean, got.rstd)
    same(b.dy, y.grad, 'dy'); same(b.dgamma, gamma.grad, 'dgamma'); same(b.dbeta, beta.grad, 'dbeta')


def test_instnorm_and_adain():
    N, HW, C = 3, 45, 8
    h = (0.5 + fill.unit((N, HW, C), 40)).double().requires_grad_(True)
    style = (0.5 * fill.unit((N, 2 * C), 41)).double().requires_grad_(True)
    dout = fill.unit((N, HW, C), 42).double()
    st = R.instnorm_stats(h)
    same(st.mean, h.mean(1)); same(st.rstd, (h.var(1, unbiased=False) + 1e-5).rsqrt())
    nchw = h.transpose(1, 2).reshape(N, C, HW, 1)
    xhat = F.instance_norm(nchw, eps=1e-5).reshape(N, C, HW).transpose(1, 2)
    out = (1 + style[:, None, :C]) * xhat + style[:, None, C:]          # model.py:324-339
    same(R.adain_fwd(h, st.mean, st.rstd, style), out, 'adain')
    out.backward(dout)
    b = R.adain_bwd(h, dout, st.mean, st.rstd, style)
    same(b.dh, h.grad, 'dh'); same(b.dstyle, style.grad, 'dstyle')
    same(b.red[..., 0], style.grad[:, :C]); same(b.red[..., 1], style.grad[:, C:])
    assert bool((b.red_abs >= b.red.abs()).all()) and bool((b.dstyle_abs >= b.dstyle.abs()).all())


def test_single_pass_variance_in_float32_at_the_offset_the_gpu_tests_use():
    """The kernels evaluate the variance as E[x^2] - mean^2 in float32.  The GPU tests pin it at |mean| / std = 4
    (tests/test_norm_kernels_gpu.py: OFFSET); that choice is only fair if plain float32 arithmetic at this ratio stays
    inside the float32 bound those tests use (rtol 2e-4): measured 2e-6.  Ratio 30 is printed, not asserted (7e-5 with
    numpy's pairwise sums; the GPU tests print what the kernels' own summation order gives there)."""
    e4 = max(R.f32_single_pass_rstd_error(4.0, n, tag) for n in (331, 1296, 4096) for tag in (1, 2, 3))
    e30 = max(R.f32_single_pass_rstd_error(30.0, n, tag) for n in (331, 1296, 4096) for tag in (1, 2, 3))
    print('float32 single-pass rstd error: ratio 4: %.2e   ratio 30: %.2e' % (e4, e30))
    assert e4 <= 2e-4 / 4, e4          # a quarter of the bound: the kernels' summation order may differ from numpy's
