"""Float64 numpy reference of the Kernel Inception Distance (sbagan/kid.py), written from the definition:

    k(x, y) = (x . y / D + 1)^3
    mmd2    = Sxx / (m (m - 1)) + Syy / (m (m - 1)) - 2 Sxy / (m m)      per subset of m rows a side
    kid     = mean of mmd2 over the subsets, kid_std = their population standard deviation

Sxx and Syy leave the diagonal out BY POSITION within the subset (a row drawn twice, or two equal rows, still pair with
each other); nothing is ever subtracted.  A row number outside [0, n) stands for a zero row that is left out of the sum
with every pair it belongs to, as the kernel's contract has it (include/sbagan_hip.h)."""
import numpy as np


def gather(x, idx):
    """(rows [m][D] float64, valid [m] bool): the rows of x at idx, zero rows where idx is outside [0, n)"""
    x, idx = np.asarray(x, dtype=np.float64), np.asarray(idx, dtype=np.int64)
    valid = (idx >= 0) & (idx < x.shape[0])
    rows = np.zeros((idx.shape[0], x.shape[1]))
    rows[valid] = x[idx[valid]]
    return rows, valid


def kernel_sum(a, b, idx_a=None, idx_b=None, exclude_diag=False):
    """float: sum of k over the position pairs (i, j) of ONE subset; idx None = every row in order"""
    a, b = np.asarray(a), np.asarray(b)
    D = a.shape[1]
    ra, va = gather(a, np.arange(a.shape[0]) if idx_a is None else idx_a)
    rb, vb = gather(b, np.arange(b.shape[0]) if idx_b is None else idx_b)
    t = ra @ rb.T / float(D) + 1.0
    k = (t * t) * t
    on = va[:, None] & vb[None, :]
    if exclude_diag:
        assert ra.shape[0] == rb.shape[0]
        on &= ~np.eye(ra.shape[0], dtype=bool)
    return float(k[on].sum())


def kernel_sums(a, b, idx_a=None, idx_b=None, exclude_diag=False):
    """[subsets] float64: kernel_sum per row of the index matrices [subsets][m] (None: one subset of every row)"""
    if idx_a is None and idx_b is None:
        return np.array([kernel_sum(a, b, None, None, exclude_diag)])
    S = len(idx_a) if idx_a is not None else len(idx_b)
    return np.array([kernel_sum(a, b, None if idx_a is None else idx_a[s], None if idx_b is None else idx_b[s],
                                exclude_diag) for s in range(S)])


def mmd2(x, y):
    """the unbiased estimate on two sets of m rows each"""
    m = len(x)
    assert len(y) == m and m >= 2
    return (kernel_sum(x, x, exclude_diag=True) / (m * (m - 1.0)) + kernel_sum(y, y, exclude_diag=True) / (m * (m - 1.0))
            - 2.0 * kernel_sum(x, y) / (float(m) * m))


def kid(real, fake, idx_real, idx_fake):
    """{'kid', 'kid_std'} over the subsets idx_real / idx_fake [S][m]"""
    real, fake = np.asarray(real), np.asarray(fake)
    v = np.array([mmd2(real[ir], fake[jf]) for ir, jf in zip(idx_real, idx_fake)])
    return {'kid': float(v.mean()), 'kid_std': float(v.std())}
