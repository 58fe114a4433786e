"""A numpy restatement of the two truncation kernels' definitions (include/sbagan_hip_ext.h: sba_style_mean,
sba_style_truncate), written from the contract: a plain helper module like ada_ref.py.

The mean is an explicit row loop in float64 in the stated order (every sum starts from +0.0); the lerp is three np.float32
operations, each rounded on its own."""
import numpy as np

CHUNK = 256


def style_mean(w):
    """(mean64 [D] float64, mean32 [D] float32) of w [n][D] float32: P_c = rows 256 c .. of the chunk in ascending row
    order, T = the P_c in ascending c, mean64 = T / n (one division), mean32 its rounding to nearest"""
    w = np.asarray(w)
    assert w.dtype == np.float32 and w.ndim == 2 and w.shape[0] >= 1
    n, D = w.shape
    total = np.zeros(D, dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        for lo in range(0, n, CHUNK):
            part = np.zeros(D, dtype=np.float64)
            for r in range(lo, min(lo + CHUNK, n)):
                part = part + w[r].astype(np.float64)
            total = total + part
        mean64 = total / np.float64(n)
        return mean64, mean64.astype(np.float32)


def style_truncate(w, w_avg, psi, copy_at_one=True):
    """w_avg + psi (w - w_avg) over the rows of w [n][D] float32, as subtract, multiply, add in float32; psi == 1: the
    bits of w (copy_at_one False: the formula there too, to show that it is NOT the identity)"""
    w, w_avg, psi = np.asarray(w), np.asarray(w_avg), np.float32(psi)
    assert w.dtype == np.float32 and w_avg.dtype == np.float32 and w.ndim == 2 and w_avg.shape == (w.shape[1],)
    if copy_at_one and psi == np.float32(1.0):
        return w.copy()
    with np.errstate(invalid='ignore', over='ignore'):
        diff = (w - w_avg[None, :]).astype(np.float32)
        scaled = (psi * diff).astype(np.float32)
        return (w_avg[None, :] + scaled).astype(np.float32)
