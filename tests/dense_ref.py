"""Float64 references of the dense conditioning-path entry points of csrc/linear.hip, written from the formulas of
the layers (nn.Linear, CA_NET's tail model.py:281-294, the attention key projection GlobalAttention.py:75,95-97,
INIT_STAGE_G.fc + BatchNorm1d(eval) + GLU + view), not from the kernels.  tests/test_dense_ref_cpu.py checks every
function against float64 autograd through torch.nn.functional; tests/test_dense_kernels_gpu.py judges the kernels
by them.

Every argument is converted to float64; every result is float64.  Dot-product results come with the sum of the
ABSOLUTE summands of every element (`*_abs`): the normaliser of a sum's error bound, which a cancelling sum cannot
provide itself.

The second half of the file holds the shapes and the inputs of the GPU cases, so that test_dense_ref_cpu.py can
show on the same numbers that plain float32 arithmetic stays inside the bounds the GPU tests use.
"""
from types import SimpleNamespace as NS

import numpy as np
import torch

from norm_ref import EPS, to_nhwc16
from oracle import fill


def _d(t):
    return None if t is None else t.detach().double()


# ------------------------------------------------------------------ nn.Linear
def linear_fwd(x, w, bias=None):
    """x [B][K], w [N][K], bias [N] or None -> y [B][N] and y_abs"""
    x, w, bias = _d(x), _d(w), _d(bias)
    y, y_abs = x @ w.t(), x.abs() @ w.abs().t()
    if bias is not None:
        y, y_abs = y + bias, y_abs + bias.abs()
    return NS(y=y, y_abs=y_abs)


def linear_bwd(x, w, dy):
    """dx [B][K] = dy w, dw [N][K] = dy^T x, db [N] = sum_b dy, and the same sums over absolute summands"""
    x, w, dy = _d(x), _d(w), _d(dy)
    return NS(dx=dy @ w, dw=dy.t() @ x, db=dy.sum(0),
              dx_abs=dy.abs() @ w.abs(), dw_abs=dy.abs().t() @ x.abs(), db_abs=dy.abs().sum(0))


# ------------------------------------------------------------------ CA_NET tail
def ca_fwd(h, eps):
    """h [B][4C], eps [B][C]: GLU, split into mu | logvar, c = eps * exp(0.5 logvar) + mu"""
    h, eps = _d(h), _d(eps)
    C = h.shape[1] // 4
    x = h[:, :2 * C] * torch.sigmoid(h[:, 2 * C:])
    mu, logvar = x[:, :C], x[:, C:]
    return NS(c=eps * torch.exp(0.5 * logvar) + mu, mu=mu, logvar=logvar)


def ca_bwd(h, eps, dc=None, dmu=None, dlogvar=None):
    """dh [B][4C] from the gradients at c, mu and logvar (None: zero)"""
    h, eps = _d(h), _d(eps)
    C = h.shape[1] // 4
    zero = torch.zeros_like(eps)
    dc, dmu, dlogvar = (zero if g is None else _d(g) for g in (dc, dmu, dlogvar))
    a, s = h[:, :2 * C], torch.sigmoid(h[:, 2 * C:])
    logvar = (a * s)[:, C:]
    gx = torch.cat((dc + dmu, dc * eps * 0.5 * torch.exp(0.5 * logvar) + dlogvar), 1)      # at the GLU output
    return torch.cat((gx * s, gx * a * s * (1 - s)), 1)


# ------------------------------------------------------------------ attention key projection (a 1x1 convolution)
def ctx_proj_fwd(words, W):
    """words [B][cdf][L], W [idf][cdf] -> src [B][idf][L] and src_abs"""
    words, W = _d(words), _d(W)
    return NS(src=torch.einsum('ic,bcl->bil', W, words), src_abs=torch.einsum('ic,bcl->bil', W.abs(), words.abs()))


def ctx_proj_bwd(words, W, dsrc):
    """dW [idf][cdf], dwords [B][cdf][L] and the same sums over absolute summands"""
    words, W, dsrc = _d(words), _d(W), _d(dsrc)
    return NS(dW=torch.einsum('bil,bcl->ic', dsrc, words), dwords=torch.einsum('ic,bil->bcl', W, dsrc),
              dW_abs=torch.einsum('bil,bcl->ic', dsrc.abs(), words.abs()),
              dwords_abs=torch.einsum('ic,bil->bcl', W.abs(), dsrc.abs()))


# ------------------------------------------------------------------ inference INIT_STAGE_G.fc
def fc_bn_glu_eval(x, w, gamma, beta, running_mean, running_var, eps=EPS):
    """x [B][K], w [2 F2][K] (no bias), BatchNorm1d(2 F2) in eval mode, GLU, view(B, F2 / 16, 4, 4) as NHWC
    [B][16][F2 / 16]: value feature f = channel f // 16, pixel f % 16"""
    x, w, gamma, beta, rm, rv = (_d(t) for t in (x, w, gamma, beta, running_mean, running_var))
    z = (x @ w.t() - rm) / torch.sqrt(rv + eps) * gamma + beta
    F2 = z.shape[1] // 2
    return to_nhwc16(z[:, :F2] * torch.sigmoid(z[:, F2:]))


# ====================================================================================================================
# The GPU cases (tests/test_dense_kernels_gpu.py) and their inputs: float32 tensors on the CPU from oracle.fill,
# weights divided by sqrt(K).  Each shape is the smallest that reaches its branch of the host dispatch.
# ====================================================================================================================
# (B, K, N)
LINEAR_FWD_MFMA = [(1, 4, 1), (32, 36, 33), (20, 100, 400), (31, 256, 31)]
LINEAR_FWD_ROWS = [(33, 64, 37), (20, 102, 40), (33, 8, 8200), (64, 256, 5)]
LINEAR_BWD_SMALL = [(20, 100, 400), (32, 33, 36), (1, 4, 4)]
LINEAR_BWD_WIDE = (3, 40, 2080)
LINEAR_BWD_FALLBACK = [(33, 16, 7), (33, 16, 516), (33, 16, 4100), (20, 100, 402), (4, 16, 2052)]
LINEAR_BWD_FALLBACK_DET = (33, 16, 516)
# (B, C)
CA = [(1, 1), (3, 100), (5, 257)]
# (B, idf, cdf, L)
CTX_FWD_MFMA = [(1, 32, 4, 1), (3, 48, 100, 7), (2, 64, 256, 18), (5, 32, 256, 32)]
CTX_VALU = (2, 5, 6, 3)
CTX_BWD_DWORDS = [(2, 5, 6, 3), (3, 32, 256, 7)]
CTX_FP8 = [(1, 32, 16, 1), (3, 48, 48, 7), (2, 64, 256, 18)]
CTX_FP8_ZERO = (2, 64, 256, 18)
# (B, K, F2)
GLU = [(1, 4, 16), (33, 100, 48), (20, 102, 32)]
GLU_BF16 = (33, 100, 48)
# fill tags of the non-zero prefills of the outputs the kernels add to (test_norm_kernels_gpu.prefilled)
TAG_DW, TAG_DB, TAG_CTX_DW = 75, 76, 94


def linear_inputs(B, K, N):
    return NS(x=fill.unit((B, K), 71), w=fill.unit((N, K), 72) / float(np.sqrt(K)), bias=fill.unit((N,), 73),
              dy=fill.unit((B, N), 74))


def ca_inputs(B, C):
    return NS(h=fill.unit((B, 4 * C), 81), eps=fill.unit((B, C), 82), dc=fill.unit((B, C), 83),
              dmu=fill.unit((B, C), 84), dlogvar=fill.unit((B, C), 85))


def ctx_inputs(B, idf, cdf, L):
    return NS(words=fill.unit((B, cdf, L), 91), W=fill.unit((idf, cdf), 92) / float(np.sqrt(cdf)),
              dsrc=fill.unit((B, idf, L), 93))


def ctx_fp8_inputs(B, idf, cdf, L, zero=None):
    """integers in [-2, 2]: e4m3 holds them (and their power-of-two multiples up to 256) exactly.
    zero = 'words': the first 32-position tile of the words is all zero; zero = 'W': rows 32 .. 63 of W are."""
    g = torch.Generator().manual_seed(1000 * cdf + L)
    words = torch.randint(-2, 3, (B, cdf, L), generator=g).float()
    W = torch.randint(-2, 3, (idf, cdf), generator=g).float()
    if zero == 'words':
        assert B * L > 32
        flat = words.permute(0, 2, 1).reshape(B * L, cdf).clone()          # row = position (b, l)
        flat[:32] = 0
        words = flat.reshape(B, L, cdf).permute(0, 2, 1).contiguous()
    elif zero == 'W':
        assert idf >= 64
        W[32:64] = 0
    return NS(words=words, W=W)


def glu_inputs(B, K, F2):
    O = 2 * F2
    return NS(x=fill.unit((B, K), 101), w=fill.unit((O, K), 102) / float(np.sqrt(K)),
              gamma=fill.uniform((O,), 103, 0.5, 1.5), beta=0.2 * fill.unit((O,), 104),
              rm=0.1 * fill.unit((O,), 105), rv=fill.uniform((O,), 106, 0.5, 1.5))
