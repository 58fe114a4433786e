"""FID on the host: fid_from_stats against the textbook scipy sqrtm form on full-rank covariances, its behaviour on
rank-deficient ones, hand-checked cases, the result fields, the key check of cached real statistics and the command-line
flags.  (The moment kernels are tested on the GPU in tests/test_fid_gpu.py.)"""
import json

import numpy as np
import pytest
import torch


def features(D, n, seed, shift=0.0):
    """n correlated feature rows of width D, rounded through f32 as the trunk's features are"""
    rng = np.random.RandomState(seed)
    mix = rng.randn(D, D) / np.sqrt(D) + np.diag(rng.uniform(0.5, 1.5, D))
    return (np.abs(rng.randn(n, D) @ mix + shift)).astype(np.float32).astype(np.float64)


def moments(X):
    return X.mean(0), np.cov(X, rowvar=False)


def fid_sqrtm(mu1, S1, mu2, S2):
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrtm(S1 S2): the textbook form"""
    from scipy.linalg import sqrtm
    d = mu1 - mu2
    return float(d @ d + np.trace(S1) + np.trace(S2) - 2.0 * np.trace(sqrtm(S1 @ S2).real))


@pytest.mark.parametrize('D,n', [(64, 500), (128, 400), (256, 1000)])
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_fid_from_stats_against_sqrtm_on_full_rank_cases(D, n, seed):
    from sbagan.fid import fid_from_stats
    mu1, S1 = moments(features(D, n, 10 * seed + 1))
    mu2, S2 = moments(features(D, n, 10 * seed + 2, shift=0.25))
    assert np.linalg.matrix_rank(S1) == D and np.linalg.matrix_rank(S2) == D
    got, ref = fid_from_stats(mu1, S1, mu2, S2), fid_sqrtm(mu1, S1, mu2, S2)
    scale = np.trace(S1) + np.trace(S2)
    print('D %d n %d seed %d: fid %.12g, sqrtm form %.12g, difference %.3g of the traces'
          % (D, n, seed, got, ref, abs(got - ref) / scale))
    assert got > 0.0
    assert abs(got - ref) <= 1e-10 * scale


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_rank_deficient_identical_sets(seed):
    """n < D: the covariance has rank n - 1; sqrtm is no reference there, FID(X, X) must still vanish"""
    from sbagan.fid import fid_from_stats
    mu, S = moments(features(128, 100, seed))
    assert np.linalg.matrix_rank(S) < 128
    got = fid_from_stats(mu, S, mu, S)
    print('seed %d: FID(X, X) = %.3g at tr S = %.4g' % (seed, got, np.trace(S)))
    assert abs(got) <= 1e-6 * np.trace(S)


def test_hand_checked_shifted_mean_and_diagonal_covariances():
    from sbagan.fid import fid_from_stats
    mu, S = moments(features(64, 300, 3))
    d = np.linspace(-1.0, 1.0, 64)
    # equal covariances: the trace terms cancel, |d|^2 is left
    assert fid_from_stats(mu, S, mu + d, S) == pytest.approx(d @ d, abs=1e-10 * 2 * np.trace(S))
    # diagonal covariances commute: sum_i (sqrt a_i - sqrt b_i)^2; a zero variance on either side is allowed
    a = np.array([4.0, 9.0, 0.0, 1.0] * 16)
    b = np.array([1.0, 9.0, 16.0, 0.0] * 16)
    want = ((np.sqrt(a) - np.sqrt(b)) ** 2).sum()
    assert want == 16 * (1.0 + 0.0 + 16.0 + 1.0)
    assert fid_from_stats(mu, np.diag(a), mu, np.diag(b)) == pytest.approx(want, abs=1e-10 * (a.sum() + b.sum()))
    assert fid_from_stats(mu, np.diag(a), mu + d, np.diag(b)) == pytest.approx(want + d @ d, abs=1e-10 * (a.sum() + b.sum()))
    # 1-D textbook case: N(0, 1) against N(3, 4) is 9 + 1 + 4 - 2 * 2
    one = np.zeros((1, 1))
    assert fid_from_stats([0.0], one + 1.0, [3.0], one + 4.0) == pytest.approx(10.0, abs=1e-12)
    with pytest.raises(ValueError):
        fid_from_stats(mu, S, mu[:32], S)


def test_the_value_is_not_clipped():
    """a tiny negative number for identical sets is reported as it is: no max(., 0) and no abs in the way"""
    from sbagan.fid import fid_from_stats
    vals = []
    for seed in range(6):
        mu, S = moments(features(128, 100, seed))
        vals.append(fid_from_stats(mu, S, mu, S))
    assert any(v != 0.0 for v in vals)
    assert fid_from_stats([0.0, 0.0], np.eye(2), [0.0, 0.0], np.eye(2) * (1 + 1e-15)) == pytest.approx(0.0, abs=1e-14)


def test_summarize_fields_and_json():
    from sbagan.fid import FIELDS, fid_from_stats, summarize
    mu1, S1 = moments(features(64, 300, 5))
    mu2, S2 = moments(features(64, 200, 6, shift=0.5))
    res = summarize((300, mu1, S1, np.trace(S1)), (200, mu2, S2, np.trace(S2)), 'bfloat16')
    assert sorted(res) == sorted(FIELDS)
    assert sorted(FIELDS) == sorted(['fid', 'n_real', 'n_fake', 'trace_real', 'trace_fake', 'mean_term', 'dtype'])
    assert res['n_real'] == 300 and res['n_fake'] == 200 and res['dtype'] == 'bfloat16'
    assert res['fid'] == fid_from_stats(mu1, S1, mu2, S2)
    assert res['trace_real'] == np.trace(S1) and res['trace_fake'] == np.trace(S2)
    assert res['mean_term'] == pytest.approx(((mu1 - mu2) ** 2).sum(), rel=1e-14)
    assert res['fid'] < res['mean_term'] + res['trace_real'] + res['trace_fake']
    assert json.loads(json.dumps(res)) == res                  # plain Python numbers and strings only


def test_real_statistics_file_round_trip_and_key_mismatch(tmp_path):
    from sbagan.fid import FID, stats_key
    key = stats_key('../DAMSMencoders/bird/image_encoder200.pth', 'bfloat16', 'test', 256)
    for other in (stats_key('../DAMSMencoders/bird/image_encoder100.pth', 'bfloat16', 'test', 256),
                  stats_key('../DAMSMencoders/bird/image_encoder200.pth', 'float32', 'test', 256),
                  stats_key('../DAMSMencoders/bird/image_encoder200.pth', 'bfloat16', 'train', 256),
                  stats_key('../DAMSMencoders/bird/image_encoder200.pth', 'bfloat16', 'test', 128)):
        assert other != key
    mu, S = moments(features(64, 300, 7))
    path = str(tmp_path / 'real.npz')
    np.savez(path, n=np.int64(300), mu=mu, sigma=S, trace=np.float64(np.trace(S)), key=np.str_(key))
    ev = FID(None, D=64, key=key, dtype='bfloat16')
    assert not ev.is_loaded('real')
    ev.load_real(path)
    assert ev.is_loaded('real') and not ev.is_loaded('fake')
    n, mu_l, S_l = ev.stats('real')
    assert n == 300 and np.array_equal(mu_l, mu) and np.array_equal(S_l, S)
    with pytest.raises(RuntimeError):                           # a loaded side takes no rows
        ev.update_features('real', torch.zeros(2, 64))
    again = str(tmp_path / 'again.npz')
    ev.save_real(again)
    with np.load(again) as z:
        assert sorted(z.files) == ['key', 'mu', 'n', 'sigma', 'trace']
        assert str(z['key']) == key and int(z['n']) == 300
        assert np.array_equal(z['mu'], mu) and np.array_equal(z['sigma'], S) and float(z['trace']) == np.trace(S)
    with pytest.raises(ValueError, match='image_encoder200'):
        FID(None, D=64, key=key.replace('bfloat16', 'float32'), dtype='float32').load_real(path)
    with pytest.raises(ValueError):
        FID(None, D=128, key=key).load_real(path)               # the right key, another width
    with pytest.raises(ValueError):
        ev.stats('both')
    with pytest.raises(RuntimeError):
        ev.stats('fake')                                        # no rows yet


def test_fid_flags_in_all_four_entry_points():
    import main
    import main_bert
    import pretrain_DAMSM
    import pretrain_DAMSM_bert
    for mod in (main, main_bert, pretrain_DAMSM, pretrain_DAMSM_bert):
        args = mod.parse_args([])
        assert args.fid is False and args.fid_stats is None
        args = mod.parse_args(['--fid', '--fid_stats', 'real.npz'])
        assert args.fid is True and args.fid_stats == 'real.npz'
    from trainer import condGANTrainer
    import trainer_bert
    for cls in (condGANTrainer, trainer_bert.condGANTrainer):
        assert cls.fid is False and cls.fid_stats is None and cls.fid_result is None


def test_fid_operators_refuse_cpu_tensors():
    from sbagan import ops
    with pytest.raises(RuntimeError):
        ops.fid_accumulate(torch.zeros(4, 64), torch.zeros(64, dtype=torch.float64),
                           torch.zeros(64, 64, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        ops.fid_finalize(torch.zeros(64, dtype=torch.float64), torch.zeros(64, 64, dtype=torch.float64), 4)
