"""Precision / recall / density / coverage on the GPU: the float64 distance-and-selection kernels through
ops.prdc_knn_radius / ops.prdc_ball_counts -- exactly equal to the numpy reference (tests/prdc_ref.py) on integer-valued
features, within a derived bound (radii) and exactly (counts) on real-valued ones -- invariance under the column split,
symmetry and self-exclusion, a padded row stride, the refusals, the PRDC class with a stub feature callable, and
sampling() with --prdc through both trainers."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import prdc_ref
import sampling_harness as sh

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
U = 2.0 ** -53                  # unit roundoff of float64


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def int_features(n, D, seed):
    """integer values in [-8, 8] (as test_fid_gpu.int_features): every squared distance is an exact integer"""
    return np.random.RandomState(seed).randint(-8, 9, size=(n, D)).astype(np.float32)


def dev(x):
    return torch.tensor(np.asarray(x), device=DEV)


def host(t):
    return None if t is None else t.cpu().numpy()


def gpu_counts(a, b, ra=None, rb=None, splits=0):
    from sbagan import ops
    in_b, in_own = ops.prdc_ball_counts(dev(a), dev(b), None if ra is None else dev(ra), None if rb is None else dev(rb),
                                        splits=splits)
    for t in (in_b, in_own):
        assert t is None or (t.dtype == torch.int32 and tuple(t.shape) == (a.shape[0],))
    return host(in_b), host(in_own)


# ------------------------------------------------------------------ exactness on integer-valued features
# n = k + 1: the fewest rows a radius exists for; 63, 64, 65: one below, on and one above the tile edge; 130: three row
# blocks and three column tiles, the last of 2 rows.  D = 64: two staged chunks; 128, 192: more; 2048: the real width.
# The companion set of the count launches has another row count, so na != nb in every case.
EXACT = [(D, n, k) for D in (64, 128, 192) for k in (1, 3, 8) for n in (k + 1, 63, 64, 65, 130)]
EXACT += [(2048, 20, k) for k in (1, 3, 8)]
OTHER = {63: 130, 64: 65, 65: 130, 130: 63, 20: 9}


@pytest.mark.parametrize('D,n,k', EXACT)
def test_integer_features_are_exact(D, n, k):
    from sbagan import ops
    m = OTHER.get(n, 65)
    X, Y = int_features(n, D, 1000 * D + 10 * n + k), int_features(m, D, 77 * D + n + k)
    Y[0] = X[n - 1]                                             # a distance of exactly 0 across the sets
    rx = ops.prdc_knn_radius(dev(X), k)
    assert rx.dtype == torch.float64 and tuple(rx.shape) == (n,)
    rx = host(rx)
    want = prdc_ref.knn_radius(X, k)
    assert np.array_equal(bits(rx), bits(want))
    ry = prdc_ref.knn_radius(Y, min(k, m - 1))
    # ties are certain: a radius is itself one of the integer distances, and radii this small sit among the d2 values
    for a, b, ra, rb in ((X, Y, want, ry), (Y, X, ry, want)):
        in_b, in_own = gpu_counts(a, b, ra, rb)
        ref_b, ref_own = prdc_ref.ball_counts(a, b, ra, rb)
        assert np.array_equal(in_b, ref_b) and np.array_equal(in_own, ref_own)
    # a radius equal to a cross-set distance exactly: `<=` counts it, `<` would not
    d2 = prdc_ref.dist2(X, Y)
    in_b, in_own = gpu_counts(X, Y, d2[:, m - 1].copy(), d2[n - 1].copy())
    ref_b, ref_own = prdc_ref.ball_counts(X, Y, d2[:, m - 1], d2[n - 1])
    assert np.array_equal(in_b, ref_b) and np.array_equal(in_own, ref_own)
    assert (in_own >= 1).all() and in_b[n - 1] == m


@pytest.mark.parametrize('na,nb', [(65, 130), (130, 63)])
def test_either_radius_vector_may_be_left_out(na, nb):
    A, B = int_features(na, 128, na), int_features(nb, 128, 1000 + nb)
    ra, rb = prdc_ref.knn_radius(A, 3) * 1.2, prdc_ref.knn_radius(B, 3) * 1.2
    ref_b, ref_own = prdc_ref.ball_counts(A, B, ra, rb)
    assert ref_b.max() > 0 and ref_own.max() > 0 and ref_b.min() < nb
    for splits in (1, 2):
        in_b, in_own = gpu_counts(A, B, ra, None, splits)
        assert in_b is None and np.array_equal(in_own, ref_own)
        in_b, in_own = gpu_counts(A, B, None, rb, splits)
        assert in_own is None and np.array_equal(in_b, ref_b)


# ------------------------------------------------------------------ real-valued features against float64 numpy
# The bound on |d2_kernel - d2_reference| (derived, not measured), to first order in U, with A = |a|^2 + |b|^2:
#   kernel: a squared norm is D exact products and at most D additions: error <= D U |a|^2, both norms D U A; the dot
#     product likewise D U sum|a_d b_d| <= D U A / 2, doubled without rounding: D U A; the addition of the norms U A and
#     the subtraction U d2 <= 2 U A (d2 <= 2 A).  Together (2 D + 3) U A.
#   reference: each difference carries U, its square 3 U in all, the sum of D squares D U more: (D + 3) U d2
#     <= (2 D + 6) U A.
# Sum: (4 D + 9) U A.  A radius is an order statistic of such values, so it moves by at most the largest bound of its row.
REAL = [(70, 50, 64, 3, 0.15), (200, 150, 64, 5, 0.2), (130, 97, 192, 5, 0.08)]
SEED = {70: 0, 200: 3, 130: 7}      # per case (by nr): draws at which precision, recall (and coverage, where the case
#                                     allows it: at D = 192 every draw tried covers every real row) lie inside (0, 1)


def d2_bound_rel(D):
    return (4 * D + 9) * U


@functools.lru_cache(maxsize=None)
def real_case(nr, nf, D, k, shift):
    """(R, F, reference): the fixtures and everything numpy knows about them, computed once per case"""
    rng = np.random.RandomState(SEED[nr])
    R = rng.randn(nr, D)
    F = 0.9 * rng.randn(nf, D) + shift
    R, F = R.astype(np.float32), F.astype(np.float32)
    ref = {'r_real': prdc_ref.knn_radius(R, k), 'r_fake': prdc_ref.knn_radius(F, k),
           'd_fr': prdc_ref.dist2(F, R), 'd_rf': prdc_ref.dist2(R, F),
           'n_real': (R.astype(np.float64) ** 2).sum(1), 'n_fake': (F.astype(np.float64) ** 2).sum(1)}
    ref['counts'] = prdc_ref.counts(R, F, k)
    ref['prdc'] = prdc_ref.prdc(R, F, k)
    for v in (R, F) + tuple(ref['counts']) + tuple(v for v in ref.values() if isinstance(v, np.ndarray)):
        v.setflags(write=False)
    return R, F, ref


def smallest_gap(ref):
    """the smallest |d2 - radius| over every comparison the metrics make, relative to |a|^2 + |b|^2 of the pair"""
    nr, nf = ref['n_real'], ref['n_fake']
    fr = np.abs(ref['d_fr'] - ref['r_real'][None, :]) / (nf[:, None] + nr[None, :])      # fake in a real ball
    rf = np.abs(ref['d_rf'] - ref['r_fake'][None, :]) / (nr[:, None] + nf[None, :])      # real in a fake ball
    ro = np.abs(ref['d_rf'] - ref['r_real'][:, None]) / (nr[:, None] + nf[None, :])      # fake in a real's own ball
    return min(fr.min(), rf.min(), ro.min())


@pytest.mark.parametrize('nr,nf,D,k,shift', REAL)
def test_real_features_radii_within_the_bound_and_counts_equal(nr, nf, D, k, shift):
    from sbagan import ops
    R, F, ref = real_case(nr, nf, D, k, shift)
    m = ref['prdc']
    print('reference: precision %.4f recall %.4f density %.4f coverage %.4f'
          % (m['precision'], m['recall'], m['density'], m['coverage']))
    # neither branch of any comparison is idle on these fixtures: every count vector holds a row that some ball misses
    # and a row that some ball contains, and the rates that can lie strictly inside (0, 1) do
    assert 0.0 < m['precision'] < 1.0 and 0.0 < m['recall'] < 1.0 and (m['coverage'] < 1.0 or D == 192)
    for cnt, other in zip(ref['counts'], (nr, nf, nf)):
        assert cnt.max() > 0 and cnt.min() < other

    bound = d2_bound_rel(D)
    for X, norms, want in ((R, ref['n_real'], ref['r_real']), (F, ref['n_fake'], ref['r_fake'])):
        got = host(ops.prdc_knn_radius(dev(X), k))
        tol = bound * (norms + norms.max())
        print('radius error / bound %.3g' % (np.abs(got - want) / tol).max())
        assert (np.abs(got - want) <= tol).all()

    # the counts must be EQUAL: every d2 stays on its side of its radius when both move by their error bounds.  The
    # radius's own error is the bound at the norms of ITS pair, at most 2 max|x|^2 <= 5 (|a|^2 + |b|^2) when the norms of
    # a case lie within a factor 5 of each other; 1 + 5 bounds fit into the factor ten below.
    allnorms = np.concatenate([ref['n_real'], ref['n_fake']])
    assert allnorms.max() <= 5.0 * allnorms.min()
    gap = smallest_gap(ref)
    print('smallest relative gap %.3g against the bound %.3g' % (gap, bound))
    assert gap > 10.0 * bound
    r_real, r_fake = ops.prdc_knn_radius(dev(R), k), ops.prdc_knn_radius(dev(F), k)
    fake_in_real, _ = ops.prdc_ball_counts(dev(F), dev(R), radius_b=r_real)
    real_in_fake, real_own = ops.prdc_ball_counts(dev(R), dev(F), radius_a=r_real, radius_b=r_fake)
    for got, want in zip((fake_in_real, real_in_fake, real_own), ref['counts']):
        assert np.array_equal(host(got), want)


# ------------------------------------------------------------------ split invariance, determinism, symmetry
def test_splits_and_repeated_launches_are_bit_identical():
    from sbagan import ops
    R, F, ref = real_case(130, 97, 192, 5, 0.08)
    x, f = dev(R), dev(F)                                       # n = 130: three column tiles
    runs = []
    for splits in (1, 2, 3, 1, 0, 32):                          # (32 is capped at the three tiles there are)
        r = ops.prdc_knn_radius(x, 5, splits=splits)
        in_b, in_own = ops.prdc_ball_counts(f, x, radius_a=ops.prdc_knn_radius(f, 5, splits=splits), radius_b=r,
                                            splits=splits)
        runs.append((host(r), host(in_b), host(in_own)))
    assert runs[0][1].max() > 0 and runs[0][2].max() > 0
    for r, in_b, in_own in runs[1:]:
        assert np.array_equal(bits(r), bits(runs[0][0]))
        assert np.array_equal(in_b, runs[0][1]) and np.array_equal(in_own, runs[0][2])


def test_distances_are_bitwise_symmetric():
    """with k = 1 and mutual nearest neighbours i <-> j, radius2[i] is d2(i, j) and radius2[j] is d2(j, i): computed in
    different workgroups (rows 3 and 100) from swapped operands, they must agree in every bit"""
    from sbagan import ops
    rng = np.random.RandomState(5)
    X = rng.randn(130, 128).astype(np.float32)
    X[100] = X[3] + (0.01 * rng.randn(128)).astype(np.float32)
    want = prdc_ref.knn_radius(X, 1)
    assert want[3] == want[100] and want[3] > 0.0
    got = host(ops.prdc_knn_radius(dev(X), 1))
    assert bits(got[3]) == bits(got[100]) and got[3] > 0.0


def test_twins_get_radius_zero_and_self_is_excluded_by_index():
    from sbagan import ops
    X = int_features(70, 64, 11)
    X[66] = X[2]                                                # twins in different row blocks
    want = prdc_ref.knn_radius(X, 1)
    got = host(ops.prdc_knn_radius(dev(X), 1))
    assert np.array_equal(bits(got), bits(want))
    assert got[2] == 0.0 and got[66] == 0.0
    others = np.delete(got, [2, 66])
    assert (others > 0.0).all()                                 # it would be 0 if a row counted itself


def test_a_copy_of_the_real_set_scores_one():
    from sbagan.prdc import PRDC
    R, _, _ = real_case(70, 50, 64, 3, 0.15)
    ev = PRDC(lambda x: x, D=64, k=3, dtype='float32')
    ev.update('real', dev(R))
    ev.update('fake', dev(R).clone())
    res = ev.result()
    print(res)
    assert res['precision'] == 1.0 and res['recall'] == 1.0 and res['coverage'] == 1.0
    assert res['density'] >= 1.0 / 3


def test_row_stride_larger_than_the_width():
    from sbagan import ops
    X, Y = int_features(65, 192, 7), int_features(21, 192, 8)
    wide_x = torch.full((65, 200), 1e30, device=DEV)            # ld = 200: the 8 extra columns must never be read
    wide_y = torch.full((21, 196), 1e30, device=DEV)
    wide_x[:, :192] = dev(X)
    wide_y[:, :192] = dev(Y)
    rx, ry = prdc_ref.knn_radius(X, 2), prdc_ref.knn_radius(Y, 2)
    got = host(ops.prdc_knn_radius(wide_x[:, :192], 2))
    assert np.array_equal(bits(got), bits(rx))
    for splits in (1, 2):
        in_b, in_own = ops.prdc_ball_counts(wide_x[:, :192], wide_y[:, :192], dev(rx), dev(ry), splits=splits)
        ref_b, ref_own = prdc_ref.ball_counts(X, Y, rx, ry)
        assert np.array_equal(host(in_b), ref_b) and np.array_equal(host(in_own), ref_own)


# ------------------------------------------------------------------ refusals, all before any launch
def test_wrapper_refusals():
    from sbagan import ops
    x = torch.ones(8, 64, device=DEV)
    r8 = torch.ones(8, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError):
        ops.prdc_knn_radius(torch.ones(8, 100, device=DEV), 2)                      # D = 100
    with pytest.raises(ValueError):
        ops.prdc_knn_radius(x[:3], 3)                                               # n = k
    with pytest.raises(ValueError):
        ops.prdc_knn_radius(x, 0)
    with pytest.raises(ValueError):
        ops.prdc_knn_radius(x, 9)
    with pytest.raises(ValueError):
        ops.prdc_knn_radius(x, 2, splits=33)
    with pytest.raises(ValueError):
        ops.prdc_knn_radius(x, 2, splits=-1)
    with pytest.raises(TypeError):
        ops.prdc_knn_radius(x.double(), 2)
    with pytest.raises(RuntimeError):
        ops.prdc_knn_radius(x.cpu(), 2)
    with pytest.raises(ValueError):
        ops.prdc_knn_radius(torch.ones(8, 64, 1, device=DEV), 2)                    # 3-D
    with pytest.raises(ValueError):
        ops.prdc_knn_radius(torch.ones(64, 8, device=DEV).t(), 2)                   # column stride != 1
    with pytest.raises(ValueError):
        ops.prdc_knn_radius(torch.ones(8, 66, device=DEV)[:, :64], 2)               # row stride 66
    with pytest.raises(ValueError):
        ops.prdc_knn_radius(torch.ones(8, 68, device=DEV)[:, 1:65], 2)              # misaligned
    with pytest.raises(ValueError):
        ops.prdc_ball_counts(x, x)                                                  # no radius at all
    with pytest.raises(ValueError):
        ops.prdc_ball_counts(x, torch.ones(8, 128, device=DEV), radius_a=r8)        # widths differ
    with pytest.raises(ValueError):
        ops.prdc_ball_counts(x, x[:5], radius_b=r8)                                 # radius_b is per row of b
    with pytest.raises(TypeError):
        ops.prdc_ball_counts(x, x, radius_a=r8.float())
    with pytest.raises(RuntimeError):
        ops.prdc_ball_counts(x, x, radius_a=r8.cpu())
    with pytest.raises(TypeError):
        ops.prdc_ball_counts(x, x.double(), radius_a=r8)
    with pytest.raises(ValueError):
        ops.prdc_ball_counts(x, x, radius_a=r8, splits=40)


def test_c_abi_refusals():
    from sbagan import _lib
    E_ARG = -1
    x = torch.ones(200, 128, device=DEV)
    rad = torch.full((200,), -7.0, dtype=torch.float64, device=DEV)
    cnt = torch.full((400,), -7, dtype=torch.int32, device=DEV)
    ws = torch.zeros(4 * 200 * 8, dtype=torch.float64, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    knn, cnts, size = _lib.lib.sba_prdc_knn_radius, _lib.lib.sba_prdc_ball_counts, _lib.lib.sba_prdc_workspace_bytes
    X, R, W, B, O = x.data_ptr(), rad.data_ptr(), ws.data_ptr(), cnt.data_ptr(), cnt.data_ptr() + 800
    assert size(200, 200, 1) == 0 and size(200, 200, 2) == 2 * 200 * 64 and size(200, 200, 32) == 4 * 200 * 64
    assert size(0, 200, 1) == -1 and size(200, 200, 33) == -1 and size(200, 200, -1) == -1
    full = ws.numel() * 8
    assert knn(None, 200, 128, 128, 5, 1, R, W, full, st) == E_ARG
    assert knn(X, 200, 128, 128, 5, 1, None, W, full, st) == E_ARG
    assert knn(X + 4, 100, 128, 128, 5, 1, R, W, full, st) == E_ARG                 # misaligned rows
    assert knn(X, 200, 128, 128, 5, 1, R + 4, W, full, st) == E_ARG                 # misaligned radius
    assert knn(X, 200, 100, 128, 5, 1, R, W, full, st) == E_ARG                     # D % 64
    assert knn(X, 200, 0, 128, 5, 1, R, W, full, st) == E_ARG
    assert knn(X, 100, 128, 64, 5, 1, R, W, full, st) == E_ARG                      # ld < D
    assert knn(X, 100, 128, 130, 5, 1, R, W, full, st) == E_ARG                     # ld % 4
    assert knn(X, 200, 128, 128, 0, 1, R, W, full, st) == E_ARG                     # k
    assert knn(X, 200, 128, 128, 9, 1, R, W, full, st) == E_ARG
    assert knn(X, 5, 128, 128, 5, 1, R, W, full, st) == E_ARG                       # n = k
    assert knn(X, 200, 128, 128, 5, 33, R, W, full, st) == E_ARG                    # splits
    assert knn(X, 200, 128, 128, 5, -1, R, W, full, st) == E_ARG
    assert knn(X, 200, 128, 128, 5, 2, R, None, full, st) == E_ARG                  # two parts need a workspace
    assert knn(X, 200, 128, 128, 5, 2, R, W, size(200, 200, 2) - 1, st) == E_ARG    # ... of the full size
    assert knn(X, 200, 128, 128, 5, 2, R, W + 4, full, st) == E_ARG
    assert cnts(None, 200, 128, X, 200, 128, 128, R, R, 1, B, O, W, full, st) == E_ARG
    assert cnts(X, 200, 128, None, 200, 128, 128, R, R, 1, B, O, W, full, st) == E_ARG
    assert cnts(X, 200, 128, X, 200, 128, 128, None, None, 1, B, O, W, full, st) == E_ARG       # no radius
    assert cnts(X, 200, 128, X, 200, 128, 128, R, R, 1, None, O, W, full, st) == E_ARG          # radius_b, no in_b
    assert cnts(X, 200, 128, X, 200, 128, 128, R, R, 1, B, None, W, full, st) == E_ARG
    assert cnts(X, 200, 128, X, 0, 128, 128, R, R, 1, B, O, W, full, st) == E_ARG               # nb = 0
    assert cnts(X, 200, 128, X, 200, 128, 192, R, R, 1, B, O, W, full, st) == E_ARG             # D > ld
    assert cnts(X, 200, 128, X, 200, 128, 128, R, R, 2, B, O, None, 0, st) == E_ARG
    assert cnts(X, 200, 128, X, 200, 128, 128, R, R, 2, B, O, W, size(200, 200, 2) - 8, st) == E_ARG
    assert cnts(X, 200, 128, X, 200, 128, 128, R + 4, R, 1, B, O, W, full, st) == E_ARG
    assert cnts(X, 200, 128, X, 200, 128, 128, R, R, 1, B + 2, O, W, full, st) == E_ARG
    torch.cuda.synchronize()
    assert (rad.cpu().numpy() == -7.0).all() and (cnt.cpu().numpy() == -7).all() and (ws.cpu().numpy() == 0).all()


# ------------------------------------------------------------------ the PRDC class with a stub feature callable
def _feed(ev, side, x, update_features=False):
    """rows of x in batches of 20, 20, 7, 1, 20, ... rows"""
    lo, b = 0, 0
    while lo < x.shape[0]:
        rows = min((20, 20, 7, 1)[b % 4], x.shape[0] - lo)
        if update_features:
            ev.update_features(side, x[lo:lo + rows])
        else:
            ev.update(side, x[lo:lo + rows])
        lo, b = lo + rows, b + 1


def test_prdc_class_with_stub_features():
    from sbagan.prdc import FIELDS, PRDC
    nr, nf, D, k, shift = REAL[1]
    R, F, ref = real_case(*REAL[1])
    calls = []

    def features(images):           # the stub "trunk": the images are the feature rows
        calls.append(images.shape[0])
        return images

    ev = PRDC(features, D=D, k=k, dtype='float32', capacity=16)     # 16 -> 32 -> ... -> 256 rows: four growths a side
    _feed(ev, 'real', dev(R))
    _feed(ev, 'fake', dev(F), update_features=True)
    assert sum(calls) == nr and ev.count('real') == nr and ev.count('fake') == nf
    assert np.array_equal(host(ev.rows('real')), R) and np.array_equal(host(ev.rows('fake')), F)
    res = ev.result()
    print(res)
    assert sorted(res) == sorted(FIELDS)
    for key in ('precision', 'recall', 'density', 'coverage'):
        assert res[key] == ref['prdc'][key]
    assert (res['k'], res['n_real'], res['n_fake'], res['dtype']) == (k, nr, nf, 'float32')
    assert json.loads(json.dumps(res)) == res
    with pytest.raises(TypeError):
        ev.update('fake', dev(F).double())
    with pytest.raises(ValueError):
        ev.update('fake', torch.zeros(3, 128, device=DEV))
    with pytest.raises(ValueError):
        ev.update('both', dev(F))

    few = PRDC(features, D=D, k=k)
    few.update('real', dev(R))
    with pytest.raises(RuntimeError, match='fake side holds 0 rows'):
        few.result()
    few.update('fake', dev(F[:k]))
    with pytest.raises(RuntimeError, match='fake side holds %d rows' % k):
        few.result()
    few.update('fake', dev(F[k:k + 1]))                             # k + 1 rows: the fewest that have a k-th neighbour
    assert few.result()['n_fake'] == k + 1


# ------------------------------------------------------------------ sampling() with the flag
def _check_result(algo, files, n_images, k):
    res = json.loads(files['prdc.json'].decode())
    print('prdc.json:', res)
    assert res == algo.prdc_result
    assert sorted(res) == ['coverage', 'density', 'dtype', 'k', 'n_fake', 'n_real', 'precision', 'recall']
    assert res['n_real'] == n_images and res['n_fake'] == n_images and res['k'] == k and res['dtype'] == 'bfloat16'
    for key in ('precision', 'recall', 'coverage'):
        assert math.isfinite(res[key]) and 0.0 <= res[key] <= 1.0
    assert math.isfinite(res['density']) and 0.0 <= res['density'] <= n_images / float(k)
    return res


def test_sampling_without_and_with_the_flag(tmp_path):
    from miscc.config import reset_cfg
    make, loader, ds, ckpts = sh.setup(tmp_path, ('without', 'with'))
    algo0, files0, states0, calls0 = sh.sample(make, loader, ds, ckpts[0])
    algo1, files1, states1, calls1 = sh.sample(make, loader, ds, ckpts[1], prdc=2)
    assert algo0.prdc_result is None and calls0 == 0 and len(files0) == 6 and all(k.endswith('.png') for k in files0)
    # the same image files, byte for byte, and prdc.json beside them
    assert sorted(files1) == sorted(list(files0) + ['prdc.json']) and sh.images(files1) == files0
    # the flag consumes none of the randomness the data path and the noise draw from
    assert sh.same_states(states1, states0)
    _check_result(algo1, files1, 6, 2)
    assert calls1 == 3 + 3                          # one trunk forward per generated and per real batch
    reset_cfg()


def test_sampling_with_fid_and_r_precision_shares_the_forwards(tmp_path):
    from miscc.config import reset_cfg
    make, loader, ds, ckpts = sh.setup(tmp_path, ('two', 'three', 'cached'))
    stats = str(tmp_path / 'real.npz')
    algo0, files0, states0, calls0 = sh.sample(make, loader, ds, ckpts[0], fid=True, fid_stats=stats, r_precision=4)
    algo1, files1, states1, calls1 = sh.sample(make, loader, ds, ckpts[1], prdc=2, fid=True, r_precision=4)
    assert calls0 == 3 + 3 and os.path.exists(stats)
    assert calls1 == 3 + 3                          # each batch goes through the trunk ONCE for all three evaluators
    assert sorted(files1) == sorted(list(files0) + ['prdc.json']) and sh.images(files1) == sh.images(files0)
    for name in ('fid.json', 'r_precision.json'):
        assert json.loads(files1[name].decode()) == json.loads(files0[name].decode())
    assert sh.same_states(states1, states0)
    res1 = _check_result(algo1, files1, 6, 2)
    # cached real FID statistics: FID skips its real pass, the real batches are encoded for PRDC alone
    algo2, files2, states2, calls2 = sh.sample(make, loader, ds, ckpts[2], prdc=2, fid=True, fid_stats=stats, r_precision=4)
    assert calls2 == 3 + 3
    assert _check_result(algo2, files2, 6, 2) == res1
    assert json.loads(files2['fid.json'].decode()) == json.loads(files0['fid.json'].decode())
    assert sh.images(files2) == sh.images(files0) and sh.same_states(states2, states0)
    reset_cfg()


def test_sampling_with_prdc_through_the_bert_trainer(tmp_path):
    from miscc.config import reset_cfg
    make, loader, ds, (ckpt,) = sh.setup(tmp_path, ('out',), bert=True)
    algo, files, _, calls = sh.sample(make, loader, ds, ckpt, prdc=2)
    assert len(files) == 7 and calls == 6
    _check_result(algo, files, 6, 2)
    reset_cfg()
