#!/usr/bin/env python3
"""One SHA-256 per output buffer of every entry point of csrc/fid.hip, csrc/prdc.hip, csrc/kid.hip, csrc/msssim.hip and csrc/swd.hip over a fixed list
of seeded real-valued inputs, through the C ABI.  Run it once per build of the library, each in a fresh process, and
diff the two listings -- the summation orders of these kernels are fixed, so a refactor must leave every line equal:

    python tools/eval_bytes.py > branch.txt
    SBA_LIB_PATH=tools/_ab/parent/libsbagan_hip.so python tools/eval_bytes.py > parent.txt
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'sba-gan_amd')):
    sys.path.insert(0, p)
import torch  # noqa: E402

from sbagan import _lib  # noqa: E402

DEV = torch.device('cuda:0')
SPLITS = (0, 1, 2, 3)


def rows(seed, n, D, ld=None):
    """f32 [n][D] feature-like rows (non-negative, a scale per feature) on the device, with row stride ld"""
    rng = np.random.RandomState(seed)
    x = (np.abs(rng.randn(n, D)) * rng.uniform(0.1, 1.0, D)).astype(np.float32)
    if ld is None:
        return torch.from_numpy(x).to(DEV)
    wide = torch.full((n, ld), float('nan'), dtype=torch.float32, device=DEV)
    wide[:, :D] = torch.from_numpy(x).to(DEV)
    return wide[:, :D]


def emit(entry, case, **bufs):
    torch.cuda.synchronize()
    for name, t in bufs.items():
        h = hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()
        print('%-22s %-46s %-8s %-12s %s' % (entry, case, name, 'x'.join(str(v) for v in t.shape), h))


def stream():
    return torch.cuda.current_stream().cuda_stream


def p(t):
    return t.data_ptr() if t is not None else 0


def f64(*shape):
    return torch.zeros(shape, dtype=torch.float64, device=DEV)


def nans(*shape):
    return torch.full(shape, float('nan'), dtype=torch.float64, device=DEV)


def workspace(nbytes):
    assert nbytes >= 0
    return nans(max(nbytes, 8) // 8)


def fid():
    def accumulate(x, sum, gram):
        _lib.call('sba_fid_accumulate', p(x), x.shape[0], x.shape[1], x.stride(0) if x.shape[0] > 1 else x.shape[1],
                  p(sum), p(gram), stream())

    def finalize(case, sum, gram, n, D):
        mu, sigma, trace = nans(D), nans(D, D), nans(1)
        _lib.call('sba_fid_finalize', p(sum), p(gram), n, D, p(mu), p(sigma), p(trace), stream())
        emit('sba_fid_finalize', case, mu=mu, sigma=sigma, trace=trace)

    for D in (64, 192):
        for n in (1, 5, 33, 300):
            sum, gram = f64(D), f64(D, D)
            accumulate(rows(n, n, D), sum, gram)
            emit('sba_fid_accumulate', 'D%d-n%d' % (D, n), sum=sum, gram=gram)
            if n >= 2:
                finalize('D%d-n%d' % (D, n), sum, gram, n, D)
        sum, gram = f64(D), f64(D, D)
        accumulate(rows(7, 33, D, ld=D + 68), sum, gram)
        emit('sba_fid_accumulate', 'D%d-n33-strided' % D, sum=sum, gram=gram)
        accumulate(rows(8, 300, D), sum, gram)                  # a second call adds to the first one's moments
        emit('sba_fid_accumulate', 'D%d-n33+300' % D, sum=sum, gram=gram)
        finalize('D%d-n33+300' % D, sum, gram, 333, D)


def knn(x, k, splits):
    n, D = x.shape
    nbytes = int(_lib.lib.sba_prdc_workspace_bytes(n, n, splits))
    ws, radius2 = workspace(nbytes), nans(n)
    _lib.call('sba_prdc_knn_radius', p(x), n, D, x.stride(0), k, splits, p(radius2), p(ws), nbytes, stream())
    return radius2


def prdc():
    for D in (64, 192):
        for n in (9, 63, 64, 65, 130):
            x = rows(100 + n, n, D)
            for k in (1, 5, 8):
                for splits in SPLITS:
                    emit('sba_prdc_knn_radius', 'D%d-n%d-k%d-s%d' % (D, n, k, splits), radius2=knn(x, k, splits))
        for na, nb in ((65, 130), (130, 63)):
            a, b = rows(200 + na, na, D), rows(300 + nb, nb, D)
            ra, rb = knn(a, 5, 0), knn(b, 5, 0)
            for which, (qa, qb) in (('a', (ra, None)), ('b', (None, rb)), ('ab', (ra, rb))):
                for splits in SPLITS:
                    nbytes = int(_lib.lib.sba_prdc_workspace_bytes(na, nb, splits))
                    ws = workspace(nbytes)
                    in_b = torch.full((na,), -7, dtype=torch.int32, device=DEV)
                    in_own = torch.full((na,), -7, dtype=torch.int32, device=DEV)
                    _lib.call('sba_prdc_ball_counts', p(a), na, D, p(b), nb, D, D, p(qa), p(qb), splits, p(in_b), p(in_own),
                              p(ws), nbytes, stream())
                    emit('sba_prdc_ball_counts', 'D%d-%dx%d-r%s-s%d' % (D, na, nb, which, splits), in_b=in_b, in_own=in_own)


def kid_sums(a, b, ia, ib, ma, mb, subsets, diag, splits):
    D = a.shape[1]
    nbytes = int(_lib.lib.sba_kid_workspace_bytes(ma, mb, subsets, splits))
    ws, sums = workspace(nbytes), nans(subsets)
    _lib.call('sba_kid_kernel_sums', p(a), a.shape[0], a.stride(0), p(ia), ma, p(b), b.shape[0], b.stride(0), p(ib), mb, D,
              subsets, diag, splits, p(sums), p(ws), nbytes, stream())
    return sums


def kid():
    def indices(seed, S, m, n):
        return torch.from_numpy(np.random.RandomState(seed).randint(0, n, (S, m)).astype(np.int32)).to(DEV)

    for D in (64, 192, 2048):
        for m in (2, 63, 65, 130):
            plain_a, plain_b = rows(400 + m, m, D), rows(500 + m, m, D)
            pool_a, pool_b = rows(600 + m, m + 7, D), rows(700 + m, m + 5, D)
            for diag in (0, 1):
                for splits in SPLITS:
                    emit('sba_kid_kernel_sums', 'D%d-m%d-rows-diag%d-s%d' % (D, m, diag, splits),
                         sums=kid_sums(plain_a, plain_b, None, None, m, m, 1, diag, splits))
                    for S in (1, 3):
                        ia, ib = indices(10 * m + S, S, m, m + 7), indices(10 * m + S + 5, S, m, m + 5)
                        emit('sba_kid_kernel_sums', 'D%d-m%d-S%d-idx-diag%d-s%d' % (D, m, S, diag, splits),
                             sums=kid_sums(pool_a, pool_b, ia, ib, m, m, S, diag, splits))
    # row numbers outside [0, n) (the Python operator refuses them; the kernel reads such a row as absent)
    D, m, S = 192, 65, 3
    a, b = rows(801, m + 7, D), rows(802, m + 5, D)
    ia, ib = indices(803, S, m, m + 7), indices(804, S, m, m + 5)
    ia[0, 3], ia[1, 64], ia[2, 0], ib[0, 10], ib[2, 64] = -1, m + 7, 1 << 30, -(1 << 31), m + 5
    for diag in (0, 1):
        for splits in SPLITS:
            emit('sba_kid_kernel_sums', 'D%d-m%d-S%d-idx-out-of-range-diag%d-s%d' % (D, m, S, diag, splits),
                 sums=kid_sums(a, b, ia, ib, m, m, S, diag, splits))


def msssim():
    def images(seed, n, H, W):
        """uint8 [n][3][H][W]: a smooth pattern per image plus noise"""
        rng = np.random.RandomState(seed)
        yy, xx = np.mgrid[0:H, 0:W]
        x = np.stack([[127.5 + 90.0 * np.sin(xx / (5.0 + i + c)) * np.cos(yy / (7.0 + c)) for c in range(3)] for i in range(n)])
        return torch.from_numpy(np.clip(x + rng.normal(0.0, 20.0, x.shape), 0, 255).astype(np.uint8)).to(DEV)

    def means(imgs, pairs, scales):
        n, _, H, W = imgs.shape
        P = pairs.shape[0]
        nbytes = int(_lib.lib.sba_msssim_workspace_bytes(H, W, P, scales))
        ws, out = workspace(nbytes), nans(P, 3, scales, 2)
        _lib.call('sba_msssim_pairs', p(imgs), n, H, W, p(pairs), P, scales, p(out), p(ws), nbytes, stream())
        return out

    for H, W, scales in ((11, 11, 1), (12, 27, 1), (22, 23, 2), (45, 47, 3), (176, 176, 5), (177, 208, 5), (256, 256, 5)):
        imgs = images(900 + H, 6, H, W)
        pairs = torch.tensor([(0, 1), (2, 3), (4, 4), (5, 0), (1, 0)], dtype=torch.int32, device=DEV)
        for s in range(1, scales + 1):
            emit('sba_msssim_pairs', '%dx%d-S%d' % (H, W, s), out=means(imgs, pairs, s))
        # image numbers outside [0, n) (such a pair reads nothing and gives NaN)
        pairs[1, 1], pairs[3, 0] = 6, -1
        emit('sba_msssim_pairs', '%dx%d-S%d-out-of-range' % (H, W, scales), out=means(imgs, pairs, scales))


def swd():
    from sbagan import ops
    for S, n, P in ((32, 1, 1), (64, 3, 5), (256, 2, 128)):
        rng = np.random.RandomState(700 + S)
        imgs = torch.from_numpy(rng.randint(0, 256, (n, 3, S, S)).astype(np.uint8)).to(DEV)
        dirs = torch.from_numpy(rng.randn(147, 130)).to(DEV)
        for level in range(ops.swd_levels(S)):
            Sl = S >> level
            centres = rng.randint(3, Sl - 3, (n * P, 2)).astype(np.int32)
            desc, stats = ops.swd_descriptors(imgs, level, centres)
            emit('sba_swd_descriptors', '%dpx-n%d-P%d-L%d' % (S, n, P, level), desc=desc, stats=stats)
            proj = ops.swd_project(desc, stats, dirs)
            emit('sba_swd_project', '%dpx-n%d-P%d-L%d' % (S, n, P, level), out=proj)
    for m in (1, 2047, 2048, 2049, 6161):
        x = torch.from_numpy(np.random.RandomState(m).randn(130, m)).to(DEV)
        y = torch.from_numpy(np.random.RandomState(m + 1).randn(130, m)).to(DEV)
        emit('sba_swd_sort_columns', 'm%d' % m, data=ops.swd_sort_columns(x))
        emit('sba_swd_abs_mean', 'm%d' % m, out=ops.swd_abs_mean(x, ops.swd_sort_columns(y)))


def main():
    if not torch.cuda.is_available():
        raise SystemExit('eval_bytes.py runs the kernels: no device visible')
    print('# library: %s' % _lib.LIB_PATH)
    fid()
    prdc()
    kid()
    msssim()
    swd()


if __name__ == '__main__':
    main()
