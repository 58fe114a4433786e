"""CPU checks of the R-precision evaluation (sbagan/rprecision.py): the candidate drawing, the measure itself as a
float64 reference on hand-made cases with known ranks, the arithmetic of the result, the command-line flag, and the
refusal of CPU tensors."""
import numpy as np
import pytest
import torch


def ref_scores_ranks(cnn, true_emb, pool, idx, eps=1e-8):
    """float64 reference of the measure: scores [B][M + 1] (column 0 = the true caption) with the clamped cosine
    dot / max(|a| |c|, eps), and rank = #{ m : NOT (s_m < s_0) }."""
    cnn, true_emb, pool = (np.asarray(t, dtype=np.float64) for t in (cnn, true_emb, pool))
    idx = np.asarray(idx).reshape(cnn.shape[0], -1)
    cand = np.concatenate([true_emb[:, None, :], pool[idx]], 1)                  # [B][M + 1][nef]
    with np.errstate(invalid='ignore'):
        dot = np.einsum('bn,bmn->bm', cnn, cand)
        den = np.sqrt((cnn * cnn).sum(1))[:, None] * np.sqrt((cand * cand).sum(2))
        s = dot / np.maximum(den, eps)          # (a NaN row makes dot NaN, whatever the clamp does with a NaN norm)
        rank = (~(s[:, 1:] < s[:, :1])).sum(1)
    return s, rank.astype(np.int64)


# ------------------------------------------------------------------ draw_mismatched
def _classes():
    pool_class = np.repeat(np.arange(1, 8), 3)          # 7 classes x 3 captions = 21 pool rows
    image_class = np.array([1, 4, 4, 7, 2])
    return image_class, pool_class


def test_draw_in_range_distinct_and_never_the_images_class():
    from sbagan.rprecision import draw_mismatched
    image_class, pool_class = _classes()
    for M in (1, 5, 18):                                # 18 = every eligible row
        idx = draw_mismatched(np.random.default_rng(3), image_class, pool_class, M)
        assert idx.shape == (5, M) and idx.dtype == np.int32
        assert idx.min() >= 0 and idx.max() < len(pool_class)
        for b in range(5):
            assert len(set(idx[b].tolist())) == M
            assert (pool_class[idx[b]] != image_class[b]).all()


def test_draw_is_seeded_by_its_generator_alone():
    from sbagan.rprecision import draw_mismatched
    image_class, pool_class = _classes()
    a = draw_mismatched(np.random.default_rng(11), image_class, pool_class, 6)
    b = draw_mismatched(np.random.default_rng(11), image_class, pool_class, 6)
    c = draw_mismatched(np.random.default_rng(12), image_class, pool_class, 6)
    assert np.array_equal(a, b) and not np.array_equal(a, c)


def test_draw_leaves_the_global_generator_alone():
    from sbagan.rprecision import draw_mismatched
    image_class, pool_class = _classes()
    np.random.seed(5)
    before = np.random.get_state()
    draw_mismatched(np.random.default_rng(0), image_class, pool_class, 6)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]


def test_draw_too_few_eligible_rows_and_m_zero():
    from sbagan.rprecision import draw_mismatched
    image_class, pool_class = _classes()
    with pytest.raises(ValueError):
        draw_mismatched(np.random.default_rng(0), image_class, pool_class, 19)      # 18 eligible rows per image
    idx = draw_mismatched(np.random.default_rng(0), image_class, pool_class, 0)
    assert idx.shape == (5, 0) and idx.dtype == np.int32


# ------------------------------------------------------------------ the measure, on cases with known ranks
def test_reference_measure_on_hand_made_cases():
    e = np.eye(4)
    nan = np.full(4, np.nan)
    pool = np.stack([e[1], e[0] + e[1], 2 * e[0], -e[0], nan])      # cosines with e0: 0, 0.707, 1, -1, NaN
    idx = np.array([[0, 1, 3]])
    # a clear win: the true caption is the image's own direction
    s, r = ref_scores_ranks(e[:1], e[:1], pool, idx)
    assert r.tolist() == [0] and np.allclose(s[0], [1, 0, np.sqrt(0.5), -1])
    # a clear loss: the true caption is opposite, every candidate beats it
    s, r = ref_scores_ranks(e[:1], -e[:1], pool, idx)
    assert r.tolist() == [3]
    # an exact tie (a candidate with the true caption's direction) counts against the image
    s, r = ref_scores_ranks(e[:1], e[:1], pool, np.array([[0, 2, 3]]))
    assert s[0, 2] == s[0, 0] and r.tolist() == [1]
    # a NaN candidate counts against the image
    s, r = ref_scores_ranks(e[:1], e[:1], pool, np.array([[0, 4, 3]]))
    assert np.isnan(s[0, 2]) and r.tolist() == [1]
    # a NaN true score: nothing is below it
    s, r = ref_scores_ranks(e[:1], nan[None], pool, idx)
    assert np.isnan(s[0, 0]) and r.tolist() == [3]
    # a zero image vector: every score is 0 / eps = 0, every candidate ties
    s, r = ref_scores_ranks(np.zeros((1, 4)), e[:1], pool, idx)
    assert (s == 0).all() and r.tolist() == [3]


# ------------------------------------------------------------------ encode_pool (host logic, a stand-in text encoder)
class _ToyCaptions(object):
    """5 images x 2 captions; get_caption draws from numpy's global generator like datasets.TextDataset's does"""
    number_example, embeddings_num = 5, 2
    class_id = [3, 3, 8, 1, 8]

    def get_caption(self, i):
        np.random.randint(0, 10)                            # (the word-subset draw of an over-long caption)
        n = 1 + (7 * i) % 5
        col = np.zeros((6, 1), dtype='int64')
        col[:n, 0] = 100 + i
        return col, n


def test_encode_pool_order_chunks_and_global_state():
    from sbagan.rprecision import encode_pool
    seen = []

    def encode(captions, cap_lens):
        assert captions.dim() == 2 and (cap_lens[:-1] >= cap_lens[1:]).all()         # sorted, descending
        assert ((captions != 0).sum(1) == cap_lens).all()
        seen.append(len(cap_lens))
        sent = torch.stack([captions[:, 0].float(), cap_lens.float()], 1)
        return None, sent
    np.random.seed(9)
    before = np.random.get_state()
    pool, pool_class = encode_pool(_ToyCaptions(), encode, 4, seed=100, device=torch.device('cpu'))
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert seen == [4, 4, 2] and pool.dtype == torch.float32 and pool.shape == (10, 2)
    assert pool[:, 0].tolist() == [100 + i for i in range(10)]                        # un-permuted: row i = caption i
    assert pool[:, 1].tolist() == [1 + (7 * i) % 5 for i in range(10)]
    assert pool_class.tolist() == [3, 3, 3, 3, 8, 8, 1, 1, 8, 8]


# ------------------------------------------------------------------ result() arithmetic
def _evaluator(ranks, R=20):
    from sbagan.rprecision import RPrecision
    ev = RPrecision(None, torch.zeros(3, 4), np.array([1, 2, 3]), R=R, seed=7)
    ev._ranks = [torch.tensor(ranks[:5], dtype=torch.int32), torch.tensor(ranks[5:], dtype=torch.int32)]
    return ev


def test_result_arithmetic_with_a_dropped_remainder():
    # 23 images, 10 splits of 2, the last 3 left out of the split figures only
    ranks = [0, 1, 0, 0, 4, 9, 0, 12, 5, 0, 0, 0, 3, 10, 0, 2, 0, 0, 1, 0, 0, 0, 7]
    res = _evaluator(ranks).result()
    r = np.array(ranks)
    assert res['n'] == 23 and res['R'] == 20 and res['seed'] == 7 and res['splits'] == 10
    assert res['r_at_1'] == pytest.approx((r < 1).mean())
    assert res['r_at_5'] == pytest.approx((r < 5).mean())
    assert res['r_at_10'] == pytest.approx((r < 10).mean())
    per_split = [0.5, 1.0, 0.0, 0.5, 0.5, 1.0, 0.0, 0.5, 1.0, 0.5]
    assert (r[:20] < 1).reshape(10, 2).mean(1).tolist() == per_split
    assert res['r_at_1_splits_mean'] == pytest.approx(np.mean(per_split))
    assert res['r_at_1_splits_std'] == pytest.approx(np.std(per_split, ddof=0))
    assert set(res) == {'n', 'R', 'r_at_1', 'r_at_5', 'r_at_10', 'r_at_1_splits_mean', 'r_at_1_splits_std', 'splits',
                        'seed'}
    assert _evaluator(ranks).result(splits=4)['splits'] == 4


def test_result_with_fewer_images_than_splits():
    res = _evaluator([0, 3, 0, 0, 6, 1]).result()
    assert res['n'] == 6 and res['splits'] == 1
    assert res['r_at_1'] == pytest.approx(0.5) and res['r_at_5'] == pytest.approx(5 / 6) and res['r_at_10'] == 1.0
    assert res['r_at_1_splits_mean'] == pytest.approx(0.5) and res['r_at_1_splits_std'] == 0.0


# ------------------------------------------------------------------ the flag, the refusal
def test_r_precision_flag_in_all_four_entry_points():
    import main
    import main_bert
    import pretrain_DAMSM
    import pretrain_DAMSM_bert
    for mod in (main, main_bert, pretrain_DAMSM, pretrain_DAMSM_bert):
        assert mod.parse_args([]).r_precision == 0
        assert mod.parse_args(['--r_precision', '100']).r_precision == 100
    with pytest.raises(SystemExit):
        main.parse_args(['--r_precision', '1'])
    from trainer import condGANTrainer
    assert condGANTrainer.r_precision == 0


def test_rprec_rank_refuses_cpu_tensors():
    from sbagan import ops
    with pytest.raises(RuntimeError):
        ops.rprec_rank(torch.zeros(2, 8), torch.zeros(2, 8), torch.zeros(3, 8), torch.zeros(2, 1, dtype=torch.int32))
