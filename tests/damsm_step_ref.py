"""Float64 numpy references for the kernels of the recorded DAMSM update (csrc/damsm_step.hip), written from their
definitions in include/sbagan_hip.h.  Pure numpy: importable without a GPU and without the library."""
import numpy as np


def embed_dropout_fwd(ids, W, keep, scale):
    """out[i][c] = keep[i][c] ? W[ids[i]][c] * scale : 0 in float64; an id outside [0, ntoken) gives a zero row"""
    ids = np.asarray(ids, dtype=np.int64)
    W = np.asarray(W, dtype=np.float64)
    keep = np.asarray(keep) != 0
    out = np.zeros((len(ids), W.shape[1]), dtype=np.float64)
    for i, t in enumerate(ids):
        if 0 <= t < W.shape[0]:
            out[i] = np.where(keep[i], W[t] * float(scale), 0.0)
    return out


def embed_dropout_bwd(ids, keep, scale, dout, ntoken, dW0=None):
    """(dW, abs_terms, count): dW[id][c] = dW0[id][c] + sum_{j: ids[j] == id} keep[j][c] * dout[j][c] * scale in float64;
    abs_terms = the same sum over absolute values (|dW0| included), count[id] = how many positions hold id -- what the
    first-order bound of an f32 sum of `count` multiply-adds is made of.  Out-of-range ids add nothing."""
    ids = np.asarray(ids, dtype=np.int64)
    keep = np.asarray(keep) != 0
    dout = np.asarray(dout, dtype=np.float64)
    ninput = dout.shape[1]
    dW = np.zeros((ntoken, ninput), dtype=np.float64) if dW0 is None else np.asarray(dW0, dtype=np.float64).copy()
    mag = np.abs(dW)
    count = np.zeros(ntoken, dtype=np.int64)
    for j, t in enumerate(ids):
        if 0 <= t < ntoken:
            term = np.where(keep[j], dout[j] * float(scale), 0.0)
            dW[t] += term
            mag[t] += np.abs(term)
            count[t] += 1
    return dW, mag, count


def norm_and_coef(g, max_norm):
    """(norm, coef) of torch.nn.utils.clip_grad_norm_: the 2-norm of g in float64 and min(1, max_norm / (norm + 1e-6)).
    Everything in float64.  (The kernel squares in f32: one rounding of 2^-24 relative per term, so at most 2^-24 on the
    sum and 2^-25 on its root; with the f32 rounding of the result, 2^-24, that stays inside 2^-22.)"""
    g = np.asarray(g, dtype=np.float64).reshape(-1)
    norm = float(np.sqrt(np.sum(g * g)))
    return norm, min(1.0, float(max_norm) / (norm + 1e-6))


def adam_step_size(lr, beta1, t):
    """lr / (1 - beta1^t), float64"""
    return float(lr) / (1.0 - float(beta1) ** int(t))
