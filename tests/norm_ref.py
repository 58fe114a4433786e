"""Float64 references of the normalisation entry points of csrc/norm_act.hip, written from the
formulas of the layers (BatchNorm2d / BatchNorm1d / InstanceNorm2d, GLU, LeakyReLU 0.2, ReLU,
AdaIN), not from the kernels.  tests/test_norm_ref_cpu.py checks every function against float64
autograd through torch.nn.functional; tests/test_norm_kernels_gpu.py judges the kernels by them.

Layout: activations are NHWC flattened to [groups][rows][C] (BatchNorm: one BatchNorm batch per
group) or [N][HW][C] (InstanceNorm / AdaIN).  Every argument is converted to float64; every result
is float64.  Per-channel sums come with the sum of the ABSOLUTE summands (`*_abs`): the
normaliser of a sum's error bound, which a cancelling sum cannot provide itself.
"""
from types import SimpleNamespace as NS

import torch

ACT_NONE, ACT_GLU, ACT_LRELU, ACT_RELU = 0, 1, 2, 3
EPS, MOMENTUM, SLOPE = 1e-5, 0.1, 0.2


def _d(t):
    return None if t is None else t.detach().double()


# ------------------------------------------------------------------ BatchNorm2d (+ activation)
def bn_stats(y):
    """y [G][R][C] -> sums [G][2][C] = (sum, sum of squares) and the sums of absolute summands."""
    y = _d(y)
    return NS(sums=torch.stack((y.sum(1), (y * y).sum(1)), 1),
              sums_abs=torch.stack((y.abs().sum(1), (y * y).sum(1)), 1))


def activation(z, act):
    """z [..., C] -> [..., Co]"""
    if act == ACT_NONE:
        return z
    if act == ACT_GLU:
        Co = z.shape[-1] // 2
        return z[..., :Co] * torch.sigmoid(z[..., Co:])
    if act == ACT_LRELU:
        return torch.where(z > 0, z, SLOPE * z)
    if act == ACT_RELU:
        return z.clamp(min=0)
    raise ValueError(act)


def bn_act_fwd(y, gamma, beta, running_mean, running_var, nbt, act, residual=None, training=True,
               eps=EPS, momentum=MOMENTUM):
    """`groups` consecutive module calls of BatchNorm + activation (+ residual [G][R][Co]).
    Returns out [G][R][Co], aux [G][4][C] = (scale, shift, mean, rstd) with out = act(y * scale + shift),
    and the running statistics / num_batches_tracked after the last call."""
    y, gamma, beta, residual = _d(y), _d(gamma), _d(beta), _d(residual)
    rm, rv, nbt = _d(running_mean).clone(), _d(running_var).clone(), int(nbt)
    G, R, C = y.shape
    outs, aux = [], []
    for g in range(G):
        if training:
            mean = y[g].mean(0)
            var = ((y[g] - mean) ** 2).mean(0)                       # biased: what normalises
            unb = var * R / (R - 1) if R > 1 else var               # unbiased: what is tracked
            rm = (1 - momentum) * rm + momentum * mean
            rv = (1 - momentum) * rv + momentum * unb
            nbt += 1
        else:
            mean, var = rm, rv
        rstd = (var + eps) ** -0.5
        z = (y[g] - mean) * rstd * gamma + beta
        o = activation(z, act)
        if residual is not None:
            o = o + residual[g]
        outs.append(o)
        aux.append(torch.stack((gamma * rstd, beta - mean * gamma * rstd, mean, rstd)))
    return NS(out=torch.stack(outs), aux=torch.stack(aux), running_mean=rm, running_var=rv, nbt=nbt)


def bn_act_bwd(y, dout, aux, gamma, beta, act, positive=None):
    """Backward of training-mode BatchNorm + activation.  aux [G][4][C] supplies mean and rstd.
    positive: optional bool [G][R][C], the LeakyReLU branch taken per element (from the sign of a forward value);
    default: the sign of the float64 pre-activation.
    Returns dy and dz (the gradient at the BatchNorm output) [G][R][C], red [G][2][C] = (sum dz, sum dz * xhat) per
    group, dgamma / dbeta [C] summed over the groups,
    and red_abs / dgamma_abs / dbeta_abs, the same sums over absolute summands."""
    y, dout, aux, gamma, beta = _d(y), _d(dout), _d(aux), _d(gamma), _d(beta)
    G, R, C = y.shape
    mean, rstd = aux[:, 2][:, None, :], aux[:, 3][:, None, :]
    xhat = (y - mean) * rstd
    z = xhat * gamma + beta
    if act == ACT_NONE:
        dz = dout
    elif act == ACT_LRELU:
        pos = (z > 0) if positive is None else positive
        dz = torch.where(pos, dout, SLOPE * dout)
    elif act == ACT_GLU:
        Co = C // 2
        a, s = z[..., :Co], torch.sigmoid(z[..., Co:])
        dz = torch.cat((dout * s, dout * a * s * (1 - s)), -1)
    else:
        raise ValueError(act)
    t = dz * xhat
    red = torch.stack((dz.sum(1), t.sum(1)), 1)
    red_abs = torch.stack((dz.abs().sum(1), t.abs().sum(1)), 1)
    dy = gamma * rstd * (dz - dz.mean(1, keepdim=True) - xhat * t.mean(1, keepdim=True))
    return NS(dy=dy, dz=dz, red=red, red_abs=red_abs, dgamma=red[:, 1].sum(0), dbeta=red[:, 0].sum(0),
              dgamma_abs=red_abs[:, 1].sum(0), dbeta_abs=red_abs[:, 0].sum(0))


# ------------------------------------------------------------------ BatchNorm1d + GLU + view(B, F/32, 4, 4) as NHWC
def to_nhwc16(v):
    """[B][F/2] in the order of view(B, F/32, 4, 4) (feature = c * 16 + s) -> NHWC [B][16][F/32]"""
    B, fh = v.shape
    return v.reshape(B, fh // 16, 16).transpose(1, 2).contiguous()


def from_nhwc16(v):
    B, s, Cg = v.shape
    return v.transpose(1, 2).reshape(B, Cg * 16)


def bn1d_glu_fwd(y, gamma, beta, running_mean, running_var, nbt, eps=EPS, momentum=MOMENTUM):
    """y [B][F] -> out NHWC [B][16][F/32], mean / rstd [F], updated running statistics."""
    y, gamma, beta = _d(y), _d(gamma), _d(beta)
    B = y.shape[0]
    mean = y.mean(0)
    var = ((y - mean) ** 2).mean(0)
    rstd = (var + eps) ** -0.5
    z = (y - mean) * rstd * gamma + beta
    unb = var * B / (B - 1) if B > 1 else var
    return NS(out=to_nhwc16(activation(z, ACT_GLU)), mean=mean, rstd=rstd,
              running_mean=(1 - momentum) * _d(running_mean) + momentum * mean,
              running_var=(1 - momentum) * _d(running_var) + momentum * unb, nbt=int(nbt) + 1)


def bn1d_glu_bwd(y, dout, gamma, beta, mean, rstd):
    """dout NHWC [B][16][F/32] -> dy [B][F], dgamma / dbeta [F] (+ sums of absolute summands)."""
    y = _d(y)
    aux = torch.stack((torch.zeros_like(_d(mean)), torch.zeros_like(_d(mean)), _d(mean), _d(rstd)))[None]
    r = bn_act_bwd(y[None], from_nhwc16(_d(dout))[None], aux, gamma, beta, ACT_GLU)
    return NS(dy=r.dy[0], dz=r.dz[0], dgamma=r.dgamma, dbeta=r.dbeta, dgamma_abs=r.dgamma_abs, dbeta_abs=r.dbeta_abs)


# ------------------------------------------------------------------ InstanceNorm / AdaIN
def instnorm_stats(h, eps=EPS):
    """h [N][HW][C] -> mean, rstd [N][C] (biased variance)."""
    h = _d(h)
    mean = h.mean(1)
    var = ((h - mean[:, None]) ** 2).mean(1)
    return NS(mean=mean, rstd=(var + eps) ** -0.5)


def adain_fwd(h, mean, rstd, style):
    """style [N][2C] = (scale, shift): out = (1 + scale) * xhat + shift"""
    h, style = _d(h), _d(style)
    C = h.shape[-1]
    xhat = (h - _d(mean)[:, None]) * _d(rstd)[:, None]
    return (1 + style[:, None, :C]) * xhat + style[:, None, C:]


def adain_bwd(h, dout, mean, rstd, style):
    """Returns dh [N][HW][C], dstyle [N][2C], red [N][C][2] = (sum dout * xhat, sum dout) and red_abs."""
    h, dout, style = _d(h), _d(dout), _d(style)
    C = h.shape[-1]
    rstd = _d(rstd)[:, None]
    xhat = (h - _d(mean)[:, None]) * rstd
    t = dout * xhat
    red = torch.stack((t.sum(1), dout.sum(1)), -1)
    red_abs = torch.stack((t.abs().sum(1), dout.abs().sum(1)), -1)
    dh = (1 + style[:, None, :C]) * rstd * (dout - dout.mean(1, keepdim=True) - xhat * t.mean(1, keepdim=True))
    return NS(dh=dh, dstyle=torch.cat((red[..., 0], red[..., 1]), 1), red=red, red_abs=red_abs,
              dstyle_abs=torch.cat((red_abs[..., 0], red_abs[..., 1]), 1))


# ------------------------------------------------------------------ single-pass variance in float32
def f32_single_pass_rstd_error(ratio, n=4096, tag=77, eps=EPS):
    """Relative error of rstd when the variance of n samples `ratio + unit` is evaluated as E[x^2] - mean^2 with
    float32 sums (numpy's pairwise summation: the accuracy class of the kernels' tree of partial sums), against float64."""
    import numpy as np
    from oracle import fill
    x = (ratio + fill.unit((n,), tag)).numpy().astype(np.float32)
    m = np.float32(x.sum(dtype=np.float32) / np.float32(n))
    var = np.float32((x * x).sum(dtype=np.float32) / np.float32(n)) - m * m
    got = 1.0 / np.sqrt(np.float64(max(var, np.float32(0))) + eps)
    xd = x.astype(np.float64)
    ref = 1.0 / np.sqrt(xd.var() + eps)
    return abs(got - ref) / ref
