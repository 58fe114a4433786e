"""Image-caption retrieval without a GPU: the numpy reference (tests/retrieval_ref.py) against brute force on hand-made
cases (an example ranked by hand, ties, NaN and zero rows, the class mask), summarize, the command-line options, the
binding, the evaluator's refusals, and the derivation of the score bound the GPU tests use, shown to hold for an
emulation of the kernel's summation order."""
import ctypes
import math

import numpy as np
import pytest
import torch

import retrieval_ref as ref

U = 2.0 ** -53


def rows(values, D=64):
    """f32 rows whose first features are `values` and the rest 0"""
    out = np.zeros((len(values), D), dtype=np.float32)
    for i, v in enumerate(values):
        out[i, :len(v)] = v
    return out


def brute(X, Y, owner, cls, eps=1e-8):
    """the definitions, one pair at a time in python floats"""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    ni, nt = len(X), len(Y)

    def s(i, t):
        g = nx = ny = 0.0
        for d in range(X.shape[1]):
            g += X[i, d] * Y[t, d]
            nx += X[i, d] * X[i, d]
            ny += Y[t, d] * Y[t, d]
        den = math.sqrt(nx * ny) if nx * ny == nx * ny else float('nan')
        den = eps if not den >= eps else den           # max(den, eps), a NaN giving way to eps
        return g / den

    with np.errstate(all='ignore'):                     # (inf * 0 and inf / inf are meant)
        S = [[float(s(i, t)) for t in range(nt)] for i in range(ni)]
    out = {k: [] for k in ('i2t_instance', 'i2t_class_masked', 't2i_instance', 't2i_class_masked')}
    for i in range(ni):
        own = [S[i][t] for t in range(nt) if owner[t] == i]
        best = float('-inf')
        for v in own:
            best = float('nan') if (v != v or best != best) else max(best, v)
        cand = [t for t in range(nt) if owner[t] != i and not S[i][t] < best]
        out['i2t_instance'].append(len(cand))
        out['i2t_class_masked'].append(len([t for t in cand if cls[owner[t]] != cls[i]]))
    for t in range(nt):
        thr = S[owner[t]][t]
        cand = [i for i in range(ni) if i != owner[t] and not S[i][t] < thr]
        out['t2i_instance'].append(len(cand))
        out['t2i_class_masked'].append(len([i for i in cand if cls[i] != cls[owner[t]]]))
    return out, S


def check(X, Y, owner, cls):
    want, _ = brute(X, Y, owner, cls)
    got = ref.all_ranks(X, Y, owner, cls)
    for k, v in want.items():
        assert got[k].tolist() == v, (k, got[k].tolist(), v)
    return got


# ------------------------------------------------------------------ the reference against the definitions
def test_three_images_six_captions_by_hand():
    """unit vectors in the plane spanned by features 0 and 1; the scores are cosines that can be read off:
        images    x0 = (1, 0)   x1 = (0, 1)   x2 = (1, 1) / sqrt 2 direction (3, 3)
        captions  y0 = (1, 0)  y1 = (4, 3)   | y2 = (0, 2)  y3 = (3, 4)   | y4 = (1, 1)  y5 = (1, 0)
        owner       0     0        1     1        2     2
    s(0, .) = 1, .8, 0, .6, .707, 1      best_0 = 1    others not below 1: y5 (an exact tie)           rank 1
    s(1, .) = 0, .6, 1, .8, .707, 0      best_1 = 1    none                                            rank 0
    s(2, .) = .707, .990, .707, .990, 1, .707  best_2 = 1  none                                        rank 0
    text to image: y0: thr 1, x2 .707 -> 0;  y1: thr .8, x2 .990 -> 1;  y2: thr 1 -> 0;  y3: thr .8, x2 .990 -> 1;
                   y4: thr 1 -> 0;  y5: thr .707, x0 scores 1 -> 1."""
    X = rows([(1, 0), (0, 1), (3, 3)])
    Y = rows([(1, 0), (4, 3), (0, 2), (3, 4), (1, 1), (1, 0)])
    owner, cls = [0, 0, 1, 1, 2, 2], [5, 6, 7]
    got = check(X, Y, owner, cls)
    assert got['i2t_instance'].tolist() == [1, 0, 0]
    assert got['t2i_instance'].tolist() == [0, 1, 0, 1, 0, 1]
    assert got['i2t_class_masked'].tolist() == [1, 0, 0]            # every image is a class of its own
    assert got['best'].tolist() == [1.0, 1.0, 1.0]
    f = ref.figures(got['t2i_instance'])
    assert f['r_at_1'] == 0.5 and f['r_at_5'] == 1.0 and f['median_rank'] == 1.5 and f['mean_rank'] == 1.5


def test_a_duplicate_row_is_a_tie_that_counts():
    X = rows([(1, 2, 3), (3, 2, 1), (1, 2, 3)])             # image 2 is image 0 again
    Y = rows([(1, 2, 2), (3, 1, 1), (1, 2, 2)])             # and caption 2 is caption 0 again
    got = check(X, Y, [0, 1, 2], [1, 2, 3])
    assert got['i2t_instance'].tolist() == [1, 0, 1]        # the twin caption ties with the own one
    assert got['t2i_instance'].tolist() == [1, 0, 1]        # and the twin image with the own one


def test_a_nan_row_has_the_worst_rank_in_every_pair_it_is_in():
    X = rows([(1, 0), (0, 1), (1, 1)])
    Y = rows([(1, 0), (0, 1), (float('nan'), 1)])
    got = check(X, Y, [0, 1, 2], [1, 2, 3])
    # the NaN caption counts against images 0 and 1; image 2's own caption is NaN: every other caption counts
    assert got['i2t_instance'].tolist() == [1, 1, 2]
    assert got['t2i_instance'].tolist() == [0, 0, 2] and np.isnan(got['best'][2])
    X[1, 0] = float('inf')                                  # an infinite row scores NaN everywhere as well
    got = check(X, Y, [0, 1, 2], [1, 2, 3])
    assert got['i2t_instance'].tolist() == [1, 2, 2] and got['t2i_instance'].tolist() == [1, 2, 2]


def test_a_zero_row_scores_zero():
    X = rows([(1, 0), (0, 0), (-1, 1)])
    Y = rows([(1, 0), (0, 1), (0, 0)])
    S = ref.scores(X, Y)
    assert S[1].tolist() == [0.0, 0.0, 0.0] and S[:, 2].tolist() == [0.0, 0.0, 0.0]
    assert not np.signbit(S[1]).any()
    got = check(X, Y, [0, 1, 2], [1, 2, 3])
    # image 1 (zero): own score 0, captions 0 and 2 score 0 too (ties) -> rank 2; image 2: own 0, caption 1 above,
    # caption 0 below -> rank 1
    assert got['i2t_instance'].tolist() == [0, 2, 1]


def test_the_class_mask_removes_the_same_class_candidates_that_are_not_own():
    rng = np.random.RandomState(3)
    X = rng.randint(-3, 4, (7, 64)).astype(np.float32)
    Y = rng.randint(-3, 4, (14, 64)).astype(np.float32)
    owner = np.arange(14) // 2
    cls = np.array([1, 1, 2, 2, 2, 3, 1])
    got = check(X, Y, owner, cls)
    S = got['scores']
    for i in range(7):
        dropped = [t for t in range(14) if owner[t] != i and cls[owner[t]] == cls[i] and not S[i, t] < got['best'][i]]
        assert got['i2t_instance'][i] - got['i2t_class_masked'][i] == len(dropped)
    assert (got['i2t_instance'] != got['i2t_class_masked']).any()
    assert (got['t2i_instance'] != got['t2i_class_masked']).any()
    # one class for everything: nothing but the query's own is left, every masked rank is 0
    one = ref.all_ranks(X, Y, owner, np.zeros(7, dtype=np.int64))
    assert not one['i2t_class_masked'].any() and not one['t2i_class_masked'].any()


def test_an_image_without_a_caption_gets_minus_infinity_and_every_candidate():
    S = ref.scores(rows([(1, 0), (0, 1)]), rows([(1, 0), (1, 1), (0, 1)]))
    best = ref.own_best(S, [0, 7], [0, 0, 1])
    assert best[0] == 1.0 and best[1] == -np.inf
    above, masked = ref.counts(S, [0, 7], [0, 0, 1], best)
    assert above.tolist() == [0, 3] and masked is None


# ------------------------------------------------------------------ summarize
def test_summarize_fields_and_medians():
    from sbagan.retrieval import FIGURES, summarize
    odd = summarize(np.array([0, 9, 4, 30, 2], dtype=np.int32))
    assert sorted(odd) == sorted(FIGURES)
    assert odd == {'r_at_1': 0.2, 'r_at_5': 0.6, 'r_at_10': 0.8, 'median_rank': 5.0, 'mean_rank': 10.0}
    even = summarize([0, 1, 3, 12])
    assert even == {'r_at_1': 0.25, 'r_at_5': 0.75, 'r_at_10': 0.75, 'median_rank': 3.0, 'mean_rank': 5.0}
    for r in ([0], [5, 5], list(range(17)), [3, 0, 0, 2 ** 31 - 1]):
        assert summarize(r) == ref.figures(r)
    with pytest.raises(ValueError):
        summarize([])


def test_format_line():
    from sbagan.retrieval import RANKS, format_line, summarize
    res = {name: summarize([0, 1, 7]) for name in RANKS}
    line = format_line(3, res)
    assert line.startswith('| end epoch   3 | retrieval i2t 0.333 0.667 1.000 2 | t2i 0.333 0.667 1.000 2 | class-masked ')
    assert line.endswith('|') and '\n' not in line


# ------------------------------------------------------------------ the command line
def test_cli_options():
    from miscc import cli
    a = cli.options('x', 'cfg/DAMSM/bird.yml', [])
    assert a.retrieval == 0 and a.retrieval_only is False
    a = cli.options('x', 'cfg/DAMSM/bird.yml', ['--retrieval', '5', '--retrieval_only'], bert=True)
    assert a.retrieval == 5 and a.retrieval_only is True
    with pytest.raises(SystemExit):
        cli.options('x', 'cfg/DAMSM/bird.yml', ['--retrieval', '-1'])
    with pytest.raises(SystemExit):
        cli.options('x', 'cfg/DAMSM/bird.yml', ['--retrieval'])
    assert '--retrieval E' in cli.__doc__ and '--retrieval_only' in cli.__doc__


@pytest.mark.parametrize('module', ['main', 'main_bert', 'pretrain_DAMSM', 'pretrain_DAMSM_bert'])
def test_every_entry_point_parses_the_options(module):
    import importlib
    m = importlib.import_module(module)
    a = m.parse_args(['--retrieval', '2'])
    assert a.retrieval == 2 and a.retrieval_only is False and a.swd == 0
    assert m.parse_args([]).retrieval == 0


# ------------------------------------------------------------------ the binding
def test_header_declares_what_the_binding_binds():
    from sbagan import _lib
    decls = {name: (d.ret, ['%s %s' % (ctext, arg) for ctext, arg, _ in d.params])
             for name, d in _lib.DECLS.items() if name.startswith('sba_retrieval_')}
    assert sorted(decls) == ['sba_retrieval_counts', 'sba_retrieval_own_best', 'sba_retrieval_workspace_bytes']
    ret, args = decls.pop('sba_retrieval_workspace_bytes')
    fn = _lib.lib.sba_retrieval_workspace_bytes
    assert ret == 'int64_t' and fn.restype is ctypes.c_int64 and fn.argtypes == [ctypes.c_int] * len(args) and len(args) == 3
    for name, (ret, args) in decls.items():
        sig = _lib.SIGNATURES[name]
        assert ret == 'int' and len(sig) == len(args), name
        for ctype, arg in zip(sig, args):
            want = ctypes.c_void_p if '*' in arg else ctypes.c_int64 if 'int64_t' in arg else \
                ctypes.c_double if 'double' in arg else ctypes.c_int
            assert ctype is want, (name, arg)


def test_workspace_sizes_and_the_refusals_that_need_no_device():
    from sbagan import _lib
    ws = _lib.lib.sba_retrieval_workspace_bytes
    assert ws(64, 64, 0) == 0 and ws(1, 1, 3) == 0              # one B tile: one part
    assert ws(100, 200, 1) == 0
    assert ws(100, 200, 3) == 3 * 100 * 8 and ws(100, 200, 4) == 4 * 100 * 8 and ws(100, 200, 9) == 4 * 100 * 8
    assert ws(2933, 29330, 0) == 12 * 2933 * 8                  # 46 row blocks: 12 parts for 512 workgroups
    assert ws(40504, 202520, 0) == 0                            # 633 row blocks fill the chip on their own
    for bad in ((0, 1, 0), (1, 0, 0), (1, 1, -1), (1, 1, 33)):
        assert ws(*bad) == -1
    p = 1 << 20     # never dereferenced: every call below is refused before a launch
    best = _lib.lib.sba_retrieval_own_best
    assert best(None, 1, 64, p, 1, 64, 64, p, p, 1e-8, 0, p, None, 0, None) == -1
    for D in (0, 63, 65):
        assert best(p, 1, 128, p, 1, 128, D, p, p, 1e-8, 0, p, None, 0, None) == -1
    assert best(p + 4, 1, 64, p, 1, 64, 64, p, p, 1e-8, 0, p, None, 0, None) == -1
    assert best(p, 2, 60, p, 1, 64, 64, p, p, 1e-8, 0, p, None, 0, None) == -1
    assert best(p, 1, 64, p, 1, 64, 64, p, p, 0.0, 0, p, None, 0, None) == -1
    assert best(p, 1, 64, p, 200, 64, 64, p, p, 1e-8, 2, p, p, 15, None) == -1
    cnt = _lib.lib.sba_retrieval_counts
    assert cnt(p, 1, 64, p, 1, 64, 64, p, p, p, None, p, 1e-8, 0, p, p, None, 0, None) == -1    # classes in part
    assert cnt(p, 1, 64, p, 1, 64, 64, p, p, None, None, p, 1e-8, 0, p, p, None, 0, None) == -1
    assert cnt(p, 1, 64, p, 1, 64, 64, p, p, None, None, None, 1e-8, 0, p, None, None, 0, None) == -1


def test_the_evaluator_refuses_before_any_device_call(monkeypatch):
    from sbagan import _lib, retrieval

    def no_call(name, *a):
        raise AssertionError('a refusal reached %s' % name)
    monkeypatch.setattr(_lib, 'call', no_call)
    monkeypatch.setattr(retrieval.ops, 'call', no_call)
    x, y = torch.zeros(3, 64), torch.zeros(6, 64)
    own, cls = np.arange(6) // 2, np.array([1, 2, 3])
    retrieval.Retrieval(x, y, own, cls)                                 # (fine, and launches nothing by itself)
    for args, what in (((x, torch.zeros(6, 128), own, cls), 'wide'),
                       ((x, y, np.array([0, 0, 1, 1, 1, 1]), cls), 'image 2 has no caption'),
                       ((x, y, np.array([0, 0, 1, 1, 2, 3]), cls), 'outside'),
                       ((x, y, np.array([0, 0, 1, 1, 2, -1]), cls), 'outside'),
                       ((x, y, own[:5], cls), 'owners'),
                       ((x, y, own, cls[:2]), 'classes'),
                       ((x, y, own.astype(np.float64), cls), 'integers'),
                       ((x.double(), y, own, cls), 'float32'),
                       ((x, y[0], own, cls), '2-D')):
        with pytest.raises(ValueError, match=what):
            retrieval.Retrieval(*args)
    with pytest.raises(ValueError, match='eps'):
        retrieval.Retrieval(x, y, own, cls, eps=0.0)


# ------------------------------------------------------------------ the score bound of the GPU tests
# Derivation, to first order in U = 2^-53, for a pair whose norm product is above eps^2.  P = |x| |y| and c = x.y / P, the
# exact cosine, |c| <= 1.  The products of widened f32 values are exact in f64 (48 significant bits), so only additions,
# the product of the norms, the square root and the division round.
#   kernel (csrc/retrieval.hip):
#     g: D exact products added in ascending feature order from 0; the first addition is exact, D - 1 round:
#        |g - x.y| <= (D - 1) U sum|x_d y_d| <= (D - 1) U P                                  (Cauchy-Schwarz)
#     |x|^2: 8 partial sums (features 4 p .. 4 p + 3 of every 32-feature chunk, D / 8 terms each, D / 8 - 1 roundings),
#        then ((p0 + p1) + p2) ... + p7, at most 7 more; all terms are >= 0, so the error is relative: (D / 8 + 6) U
#     nx * ny: (D / 4 + 12) U from the norms and U of its own; the square root halves that and adds U:
#        (D / 8 + 7.5) U; the division adds U.
#     |s_kernel - c| <= (D - 1) U + |c| (D / 8 + 8.5) U <= (D + D / 8 + 7.5) U
#   reference (retrieval_ref.scores(exact=True)): every sum is math.fsum of exact products, correctly rounded:
#     g carries U |x.y|, each norm U, their product 3 U, its root 2.5 U, the quotient (1 + 2.5 + 1) U = 4.5 U |c|
# Sum: (D + D / 8 + 12) U = retrieval_ref.score_bound(D).
def emulated_scores(X, Y, eps=1e-8):
    """the kernel's arithmetic in python floats: ascending dot product, the norm in 8 interleaved partials"""
    X, Y = np.asarray(X, dtype=np.float32).astype(np.float64), np.asarray(Y, dtype=np.float32).astype(np.float64)

    def norm(v):
        part = [0.0] * 8
        for d0 in range(0, len(v), 32):
            for p in range(8):
                for d in range(d0 + 4 * p, d0 + 4 * p + 4):
                    part[p] += float(v[d]) * float(v[d])
        total = part[0]
        for p in range(1, 8):
            total += part[p]
        return total

    nx, ny = [norm(v) for v in X], [norm(v) for v in Y]
    out = np.zeros((len(X), len(Y)))
    for i, x in enumerate(X):
        for j, y in enumerate(Y):
            g = 0.0
            for d in range(len(x)):
                g += float(x[d]) * float(y[d])
            out[i, j] = g / max(math.sqrt(nx[i] * ny[j]), eps)
    return out


def bound_cases(D):
    rng = np.random.RandomState(D)
    gauss = rng.randn(6, D)
    positive = np.abs(rng.randn(6, D)) + 1.0                    # every rounding of a sum can fall the same way
    decaying = rng.randn(6, D) * (0.7 ** np.arange(D))          # the large terms first
    growing = decaying[:, ::-1]
    return [(a, b) for a in (gauss, positive, decaying, growing) for b in (gauss, positive)]


@pytest.mark.parametrize('D', [64, 256])
def test_the_score_bound_holds_for_the_kernel_order(D):
    assert ref.score_bound(D) == (D + D / 8.0 + 12.0) * U
    worst = 0.0
    for A, B in bound_cases(D):
        A, B = A.astype(np.float32), B.astype(np.float32)
        err = np.abs(emulated_scores(A, B) - ref.scores(A, B, exact=True)).max()
        worst = max(worst, err / ref.score_bound(D))
        # what the bound catches: one f32 rounding of the dot product is far outside it
        g32 = np.abs((A @ B.T).astype(np.float64) - A.astype(np.float64) @ B.astype(np.float64).T)
        assert g32.max() > 0
    print('D = %d: the worst emulated error is %.3f of the bound' % (D, worst))
    assert worst <= 1.0
    # a score taken with f32 inputs rounded once more (the dot product kept in f32) misses the bound by orders
    A, B = bound_cases(D)[0]
    A, B = A.astype(np.float32), B.astype(np.float32)
    s32 = (A @ B.T).astype(np.float64) / np.sqrt((A.astype(np.float64) ** 2).sum(1)[:, None]
                                                  * (B.astype(np.float64) ** 2).sum(1)[None, :])
    assert np.abs(s32 - ref.scores(A, B, exact=True)).max() > 100 * ref.score_bound(D)


def test_integer_features_make_the_reference_exact():
    """small integers: dot products, norms and their product are integers below 2^53 in any order, and the correctly
    rounded square root and quotient are the same everywhere -- both summation orders agree bit for bit"""
    rng = np.random.RandomState(5)
    A, B = (rng.randint(-8, 9, (9, 256)).astype(np.float32) for _ in range(2))
    a, b, c = ref.scores(A, B), ref.scores(A, B, exact=True), emulated_scores(A, B)
    assert np.array_equal(a.view(np.int64), b.view(np.int64)) and np.array_equal(a.view(np.int64), c.view(np.int64))
    assert np.array_equal(ref.scores(B, A).T.view(np.int64), a.view(np.int64))      # either side may be the query
