"""R-precision on the GPU: the rank kernel through ops.rprec_rank against the float64 reference of
tests/test_rprecision_cpu.py (scores within the f32 summation bound, ranks exactly), constructed ties / NaNs / zero rows,
determinism, the wrapper's refusals, the evaluator with a stub image encoder, and sampling() with the flag through both
trainers."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import sampling_harness as sh

pytestmark = pytest.mark.gpu

from test_rprecision_cpu import ref_scores_ranks  # noqa: E402

DEV = 'cuda:0'

# (B, M, nef, P)
CASES = [(1, 0, 4, 1), (1, 1, 4, 2), (3, 2, 8, 5), (5, 7, 252, 9),
         (20, 99, 256, 300),        # the product shape
         (2, 100, 260, 64),         # a row that is not a whole number of 64-lane float4 passes
         (2, 3, 1024, 4),           # the widest row
         (65, 5, 256, 6),           # more images than a small grid; heavy index reuse
         (3, 257, 256, 300)]        # a candidate count that is not a multiple of the waves per workgroup


def score_tol(nef):
    """|s_f32 - s_f64| bound: sequential-summation n u on each of the three reductions (u = 2^-24), the cosine's
    absolute-sum ratio <= 1 by Cauchy-Schwarz, slack for the square root and the division"""
    return 4.0 * nef * 2.0 ** -24


def _inputs(case, seed):
    B, M, nef, P = case
    rng = np.random.RandomState(seed)
    cnn, true_emb, pool = (rng.randn(n, nef).astype(np.float32) for n in (B, B, P))
    idx = rng.randint(0, P, size=(B, M)).astype(np.int32)
    return cnn, true_emb, pool, idx


def _min_margin(s):
    """smallest |s_m - s_0| over the finite, not exactly tied candidates (inf when there is none)"""
    d = np.abs(s[:, 1:] - s[:, :1])
    d = d[np.isfinite(d) & (d != 0)]
    return d.min() if d.size else np.inf


@functools.lru_cache(maxsize=None)
def _case(case):
    """inputs and float64 reference of the first seed in 0..49 whose margins all exceed twice the score tolerance
    (ranks are then decided by the reference alone), computed once per case"""
    for seed in range(50):
        x = _inputs(case, seed)
        s, r = ref_scores_ranks(*x)
        if np.abs(s[:, 1:] - s[:, :1]).min(initial=np.inf) > 2 * score_tol(case[2]):
            return seed, x, s, r
    return None


def _dev(x):
    return [torch.from_numpy(t).to(DEV) for t in x]


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'B%d-M%d-nef%d-P%d' % c)
def test_kernel_vs_float64_reference(case):
    from sbagan import ops
    found = _case(case)
    assert found is not None, 'no seed in 0..49 with every margin above 2 x tolerance'
    seed, x, s64, r64 = found
    cnn, true_emb, pool, idx = _dev(x)
    rank, scores = ops.rprec_rank(cnn, true_emb, pool, idx, want_scores=True)
    assert rank.dtype == torch.int32 and rank.shape == (case[0],) and scores.shape == (case[0], case[1] + 1)
    err = np.abs(scores.cpu().numpy().astype(np.float64) - s64).max()
    print('case %s seed %d: max score error %.3e (bound %.3e)' % (case, seed, err, score_tol(case[2])))
    assert err <= score_tol(case[2])
    assert rank.cpu().numpy().tolist() == r64.tolist()
    # without the score output (scores = NULL in the C ABI), and with the indices handed over from the host
    assert torch.equal(ops.rprec_rank(cnn, true_emb, pool, idx), rank)
    assert torch.equal(ops.rprec_rank(cnn, true_emb, pool, x[3]), rank)


# ------------------------------------------------------------------ constructed cases at (3, 4, 256, 8)
def _constructed(seed=1):
    return list(_inputs((3, 4, 256, 8), seed))


def _run_exact(x):
    from sbagan import ops
    s64, r64 = ref_scores_ranks(*x)
    assert _min_margin(s64) > 2 * score_tol(256)          # everything but the constructed ties / NaNs is clear-cut
    rank = ops.rprec_rank(*_dev(x)).cpu().numpy()
    assert rank.tolist() == r64.tolist()
    return rank


def test_duplicate_of_the_true_caption_is_an_exact_tie():
    x = _constructed()
    cnn, true_emb, pool, idx = x
    true_emb[1] *= 1e3                                     # (magnitudes within the contract's 1e-3 .. 1e3)
    pool[5] = true_emb[1]
    idx[1] = [0, 5, 2, 3]
    cnn[1] = true_emb[1] * 1e-3 + 0.05 * cnn[1]            # the true caption clearly beats rows 0, 2, 3
    rank = _run_exact(x)
    assert rank[1] == 1


def test_repeated_index_contributes_twice():
    x = _constructed()
    cnn, true_emb, pool, idx = x
    cnn[2] = pool[6] + 0.5 * true_emb[2] + 0.05 * cnn[2]   # row 6 beats the true caption, which beats the random rows
    idx[2] = [6, 1, 0, 3]
    assert _run_exact(x)[2] == 1
    idx[2] = [6, 1, 6, 3]
    assert _run_exact(x)[2] == 2


def test_zero_image_row_ranks_last():
    x = _constructed()
    x[0][0] = 0
    assert _run_exact(x)[0] == 4


def test_nan_in_a_gathered_row_counts_against_the_image():
    x = _constructed()
    cnn, true_emb, pool, idx = x
    cnn[0] = true_emb[0] + 0.05 * cnn[0]                   # alone, the true caption would win: rank 0
    idx[:] = [[1, 2, 3, 4], [1, 2, 3, 4], [1, 2, 3, 4]]
    assert _run_exact(x)[0] == 0
    pool[3, 77] = np.nan
    assert _run_exact(x).tolist()[0] == 1


def test_nan_in_the_true_caption_ranks_last():
    x = _constructed()
    x[1][2, 255] = np.nan
    assert _run_exact(x)[2] == 4


def test_two_launches_are_bit_identical():
    from sbagan import ops
    x = _dev(_inputs((20, 99, 256, 300), 0))
    r1, s1 = ops.rprec_rank(*x, want_scores=True)
    r2, s2 = ops.rprec_rank(*x, want_scores=True)
    assert torch.equal(r1, r2) and torch.equal(s1, s2)


# ------------------------------------------------------------------ contract
def test_wrapper_refuses_before_any_launch(monkeypatch):
    from sbagan import ops
    launched = []
    monkeypatch.setattr(ops, 'call', lambda *a: launched.append(a[0]))

    def t(*shape):
        return torch.zeros(*shape, device=DEV)

    def i32(B, M):
        return torch.zeros(B, M, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        ops.rprec_rank(t(2, 6), t(2, 6), t(3, 6), i32(2, 1))                     # nef % 4
    with pytest.raises(ValueError):
        ops.rprec_rank(t(2, 1028), t(2, 1028), t(3, 1028), i32(2, 1))            # nef > 1024
    with pytest.raises(ValueError):
        ops.rprec_rank(t(2, 16)[:, ::2], t(2, 8), t(3, 8), i32(2, 1))            # not contiguous
    with pytest.raises(ValueError):
        ops.rprec_rank(t(2, 8), t(2, 8), t(6, 8)[::2], i32(2, 1))
    with pytest.raises(TypeError):
        ops.rprec_rank(t(2, 8), t(2, 8), t(3, 8), i32(2, 1).long())              # int64 idx
    with pytest.raises(TypeError):
        ops.rprec_rank(t(2, 8).double(), t(2, 8), t(3, 8), i32(2, 1))
    with pytest.raises(ValueError):
        ops.rprec_rank(t(2, 8), t(2, 8), t(3, 8), i32(2, 1) + 3)                 # idx == P
    with pytest.raises(ValueError):
        ops.rprec_rank(t(2, 8), t(2, 8), t(3, 8), np.array([[0], [-1]], dtype=np.int32))
    with pytest.raises(ValueError):
        ops.rprec_rank(t(2, 8), t(3, 8), t(3, 8), i32(2, 1))                     # true_emb rows != B
    with pytest.raises(ValueError):
        ops.rprec_rank(t(2, 8), t(2, 8), t(3, 8), i32(3, 1))                     # idx rows != B
    assert launched == []


def test_c_abi_rejects_misaligned_rows_and_bad_sizes():
    from sbagan import _lib
    buf = torch.zeros(64, device=DEV)
    rank = torch.zeros(2, dtype=torch.int32, device=DEV)
    idx = torch.zeros(2, dtype=torch.int32, device=DEV)
    p, st = buf.data_ptr(), torch.cuda.current_stream().cuda_stream

    def rc(cnn, B, M, nef, P):
        return _lib.lib.sba_rprec_rank(cnn, p, p, idx.data_ptr(), 1e-8, rank.data_ptr(), None, B, M, nef, P, st)
    assert rc(p + 4, 2, 1, 8, 1) == -1                     # a row pointer that is not 16-byte aligned
    for B, M, nef, P in ((0, 1, 8, 1), (2, -1, 8, 1), (2, 1, 8, 0), (2, 1, 6, 1), (2, 1, 0, 1), (2, 1, 1028, 1)):
        assert rc(p, B, M, nef, P) == -1, (B, M, nef, P)
    assert rc(p, 2, 1, 8, 1) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the evaluator with a stub image encoder
def _stub_setup():
    rng = np.random.RandomState(4)
    pool = torch.from_numpy(rng.randn(40, 256).astype(np.float32)).to(DEV)
    pool_class = np.repeat(np.arange(10), 4)
    true_emb = torch.from_numpy(rng.randn(6, 256).astype(np.float32)).to(DEV)
    class_ids = np.array([0, 3, 3, 9, 5, 1])
    return pool, pool_class, true_emb, class_ids


def test_evaluator_code_equal_to_the_true_caption():
    from sbagan.rprecision import RPrecision
    pool, pool_class, true_emb, class_ids = _stub_setup()
    ev = RPrecision(lambda images: (None, images), pool, pool_class, R=8, seed=5)
    ev.update(true_emb[:4].clone(), true_emb[:4], class_ids[:4])
    ev.update(true_emb[4:].clone(), true_emb[4:], class_ids[4:])
    assert ev.ranks().tolist() == [0] * 6
    res = ev.result()
    assert res['n'] == 6 and res['R'] == 8 and res['seed'] == 5 and res['splits'] == 1
    assert res['r_at_1'] == 1.0 and res['r_at_5'] == 1.0 and res['r_at_1_splits_mean'] == 1.0


def test_evaluator_code_equal_to_a_mismatched_candidate():
    from sbagan.rprecision import RPrecision, draw_mismatched
    pool, pool_class, true_emb, class_ids = _stub_setup()
    idx = draw_mismatched(np.random.default_rng(5), class_ids, pool_class, 7)     # what the evaluator will draw
    code = pool[torch.from_numpy(idx[:, 2].astype(np.int64)).to(DEV)].clone()
    ev = RPrecision(lambda images: (None, images), pool, pool_class, R=8, seed=5)
    ev.update(code, true_emb, class_ids)
    ranks = ev.ranks()
    assert (ranks >= 1).all() and (ranks <= 7).all()
    assert ev.result()['r_at_1'] == 0.0


# ------------------------------------------------------------------ sampling() with the flag
def _sample(make, loader, ds, ckpt, R):
    """sampling_harness.sample as these tests read it: (trainer, output directory, sorted file names, states after)"""
    algo, files, states, _ = sh.sample(make, loader, ds, ckpt, r_precision=R)
    return algo, os.path.join(ckpt[:-len('.pth')], 'valid'), sorted(files), states


def _check_result(algo, out_dir, R):
    with open(os.path.join(out_dir, 'r_precision.json')) as f:
        res = json.load(f)
    assert res == algo.r_precision_result
    ranks = algo.r_precision_evaluator.ranks()
    assert res['n'] == 6 and len(ranks) == 6 and res['R'] == R and res['splits'] == 1
    assert ranks.min() >= 0 and ranks.max() <= R - 1
    for k in (1, 5, 10):
        assert 0.0 <= res['r_at_%d' % k] <= 1.0 and res['r_at_%d' % k] == pytest.approx((ranks < k).mean())
    assert res['r_at_1_splits_mean'] == pytest.approx(res['r_at_1']) and res['r_at_1_splits_std'] == 0.0
    assert res['r_at_5'] == 1.0                            # R = 4: every rank is below 5


def test_sampling_with_and_without_the_flag(tmp_path):
    from miscc.config import reset_cfg
    make, loader, ds, ckpts = sh.setup(tmp_path, ('with', 'without'))
    algo, out_dir, files, states = _sample(make, loader, ds, ckpts[0], 4)
    algo0, out_dir0, files0, states0 = _sample(make, loader, ds, ckpts[1], 0)
    assert algo0.r_precision_result is None and 'r_precision.json' not in files0
    assert len(files0) == 6 and files == sorted(files0 + ['r_precision.json'])
    _check_result(algo, out_dir, 4)
    # the flag consumes none of the randomness the data path and the noise draw from
    assert states[0][0] == states0[0][0] and np.array_equal(states[0][1], states0[0][1]) \
        and states[0][2:] == states0[0][2:]
    assert torch.equal(states[1], states0[1]) and torch.equal(states[2], states0[2])
    reset_cfg()


def test_sampling_with_the_flag_through_the_bert_trainer(tmp_path):
    """the pool is encoded through the trainer's _encode hook: trainer_bert's BertEncoder (a random 2-layer trunk)"""
    from miscc.config import reset_cfg
    make, loader, ds, (ckpt,) = sh.setup(tmp_path, ('out',), bert=True)
    algo, out_dir, files, _ = _sample(make, loader, ds, ckpt, 4)
    assert len(files) == 7 and 'r_precision.json' in files
    _check_result(algo, out_dir, 4)
    assert algo.r_precision_evaluator.pool.shape == (12, 256)
    reset_cfg()
