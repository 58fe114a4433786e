"""Reference of --diffaug_p / --ada (numpy, no GPU, no library): the per-image flags of the gated augmentation, the gated
transform built from tests/diffaug_ref.py image by image, and the controller -- Python integers for the counts,
numpy.float32 for r_t and p, in the operation order include/sbagan_hip_ext.h states."""
import numpy as np

import diffaug_ref as R

F = np.float32


def gate_bits(gates, p):
    """g_n per image: bit b set iff gates[n][b] < p, strictly, compared in float32; a NaN p sets nothing"""
    gates, p = np.asarray(gates, dtype=F), F(p)
    with np.errstate(invalid='ignore'):
        on = gates[:, :3] < p
    return (on[:, 0] * 1 + on[:, 1] * 2 + on[:, 2] * 4).astype(np.int32)


def applied(gates, p, flags):
    return (gate_bits(gates, p) & np.int32(flags)).astype(np.int32)


def forward(x, params, gates, p, flags, fn=R.chain_forward):
    """image n = fn(x[n], params[n], flags & g_n); f_n = 0: the image itself.  Returns (out, applied)."""
    f = applied(gates, p, flags)
    out = np.array(x, copy=True)
    for n in range(x.shape[0]):
        if f[n]:
            out[n] = fn(x[n:n + 1], params[n:n + 1], int(f[n]))[0]
    return out, f


def backward(dout, params, f, flags, fn=R.chain_backward):
    """dx for the output gradient dout with the per-image flags f & flags (any int32 in f: only its low bits count)"""
    f = np.asarray(f, dtype=np.int64) & int(flags)
    dx = np.array(dout, copy=True)
    for n in range(dout.shape[0]):
        if f[n]:
            dx[n] = fn(dout[n:n + 1], params[n:n + 1], int(f[n]))[0]
    return dx


class Controller(object):
    """the state of sba_ada_count / sba_ada_adjust for nD discriminators"""

    def __init__(self, nD, p0=0.0):
        self.p = np.full(nD, p0, dtype=F)
        self.rt = np.zeros(nD, dtype=F)
        self.counters = [[0, 0, 0, 0] for _ in range(nD)]        # pos, neg, cnt, calls: Python ints

    def count(self, row, prob):
        prob = np.asarray(prob, dtype=F)
        c = self.counters[row]
        with np.errstate(invalid='ignore'):
            c[0] += int((prob > F(0.5)).sum())
            c[1] += int((prob < F(0.5)).sum())
        c[2] += int(prob.size)
        c[3] += 1

    def adjust(self, interval, target, adjust, p_max):
        target, adjust, p_max = F(target), F(adjust), F(p_max)
        for r, c in enumerate(self.counters):
            if c[3] < interval:
                continue
            rt = F(0)
            if c[2] != 0:
                rt = F(F(c[0] - c[1]) / F(c[2]))                 # one float32 division of two exactly converted ints
                v = self.p[r]
                if rt > target:
                    v = F(v + adjust)
                elif rt < target:
                    v = F(v - adjust)
                self.p[r] = min(max(v, F(0)), p_max)
            self.rt[r] = rt
            c[:] = [0, 0, 0, 0]
