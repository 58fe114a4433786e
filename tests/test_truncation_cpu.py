"""--truncation / --truncation_sweep without a GPU: the two entry points in the second header and the Makefile, the flags
and their refusals on every entry point, the numpy reference (tests/truncation_ref.py) against itself, and the schemas of
truncation.json / truncation_sweep.json."""
import os

import numpy as np
import pytest

import truncation_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {'sba_style_mean': [('const float*', 'w'), ('int', 'n'), ('int', 'D'), ('double*', 'mean64'), ('float*', 'mean32'),
                          ('void*', 'workspace'), ('void*', 'stream')],
       'sba_style_truncate': [('const float*', 'w'), ('const float*', 'w_avg'), ('float', 'psi'), ('float*', 'out'),
                              ('int', 'n'), ('int', 'D'), ('void*', 'stream')]}


def test_the_two_entry_points_are_declared_in_the_second_header_and_built():
    from sbagan import abi
    for name, params in NEW.items():
        assert name in abi.EXT_DECLS and name not in abi.DECLS
        assert abi.EXT_DECLS[name].ret == 'int' and [p[:2] for p in abi.EXT_DECLS[name].params] == params
    with open(os.path.join(ROOT, 'sba-gan_amd', 'csrc', 'Makefile')) as fh:
        assert 'truncation.hip' in fh.read()
    assert os.path.isfile(os.path.join(ROOT, 'sba-gan_amd', 'csrc', 'truncation.hip'))


def test_refusals_come_back_before_any_launch():
    """the argument checks need no device"""
    from sbagan import _lib
    lib, bad = _lib.lib, _lib.CONSTANTS['SBA_E_ARG']
    x = 4096            # any non-NULL, 16-byte aligned address: refused before it is used
    ok = (x, 300, 8, x, x, x)
    for i, v in ((0, None), (3, None), (4, None), (5, None), (1, 0), (1, (1 << 20) + 1), (2, 0), (2, 4097), (0, x + 2),
                 (3, x + 4), (4, x + 1), (5, x + 4)):
        args = list(ok)
        args[i] = v
        assert lib.sba_style_mean(*args, None) == bad, (i, v)
    ok = (x, x, 0.5, x, 3, 8)
    for i, v in ((0, None), (1, None), (3, None), (0, x + 1), (1, x + 2), (3, x + 3), (2, float('nan')), (2, float('inf')),
                 (2, float('-inf')), (4, 0), (4, (1 << 20) + 1), (5, 0), (5, 4097)):
        args = list(ok)
        args[i] = v
        assert lib.sba_style_truncate(*args, None) == bad, (i, v)


# ------------------------------------------------------------------ the flags
def test_the_parser_refuses_and_accepts(capsys):
    import main
    for bad in (['--truncation', '1.5'], ['--truncation', '-0.1'], ['--truncation', 'a'], ['--truncation', '0.5,0.5,0.5'],
                ['--truncation', 'nan'], ['--truncation_n', '0'], ['--truncation_n', str((1 << 20) + 1)],
                ['--kid', '--truncation_sweep', '0.5,1.5'], ['--kid', '--truncation_sweep', '0.5,x'],
                ['--kid', '--truncation_sweep', '0.5,1,0.5'], ['--kid', '--truncation_sweep', '1,1.0'],
                ['--kid', '--truncation_sweep', ''], ['--kid', '--truncation_sweep', '0.5,'],
                ['--kid', '--truncation_sweep', '0.5', '--truncation_sweep_n', '-1']):
        with pytest.raises(SystemExit):
            main.parse_args(bad)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        main.parse_args(['--truncation_sweep', '1,0.5', '--ms_ssim', '2'])
    err = capsys.readouterr().err
    assert err.count('--truncation_sweep needs at least one of --fid, --kid, --prdc K, --r_precision R') == 1
    a = main.parse_args(['--truncation', '0.7,1.0', '--truncation_sweep', '1,0.7,0.5', '--prdc', '2'])
    assert a.truncation == (0.7, 1.0) and a.truncation_sweep == (1.0, 0.7, 0.5) and a.prdc == 2
    assert (a.truncation_n, a.truncation_sweep_n) == (16384, 0)
    assert main.parse_args(['--truncation', '0']).truncation == 0.0            # a given value turns it on
    assert main.parse_args(['--truncation', '1']).truncation == 1.0
    for one in (['--fid'], ['--kid'], ['--prdc', '2'], ['--r_precision', '3']):
        assert main.parse_args(['--truncation_sweep', '0.5'] + one).truncation_sweep == (0.5,)


@pytest.mark.parametrize('module', ['main', 'main_bert', 'pretrain_DAMSM', 'pretrain_DAMSM_bert'])
def test_flags_parse_on_every_entry_point(module):
    import importlib
    m = importlib.import_module(module)
    a = m.parse_args([])
    assert a.truncation is None and a.truncation_sweep is None and (a.truncation_n, a.truncation_sweep_n) == (16384, 0)
    a = m.parse_args(['--truncation', '0.7', '--truncation_n', '600', '--truncation_sweep', '1,0.5', '--kid',
                      '--truncation_sweep_n', '4'])
    assert (a.truncation, a.truncation_n, a.truncation_sweep, a.truncation_sweep_n) == (0.7, 600, (1.0, 0.5), 4)
    with pytest.raises(SystemExit):
        m.parse_args(['--truncation', '1.5'])


def test_the_lines_of_the_entry_points():
    import main
    from sbagan import truncation
    a = main.parse_args(['--truncation_sweep', '1,0.5', '--kid', '--ms_ssim', '2', '--swd', '8', '--nearest', '1'])
    assert truncation.not_swept_line(a) == \
        '--truncation_sweep: --ms_ssim, --swd, --nearest are not swept (the normal run only)'
    assert truncation.not_swept_line(main.parse_args(['--truncation_sweep', '1', '--kid', '--swd', '8'])) == \
        '--truncation_sweep: --swd is not swept (the normal run only)'
    assert truncation.not_swept_line(main.parse_args(['--truncation_sweep', '1', '--kid'])) is None
    m = {'kid': {'kid': 0.25}, 'prdc': {'precision': 1.0, 'recall': 0.5, 'density': 0.75, 'coverage': 0.25},
         'r_precision': {'r_at_1': 0.5}}
    assert truncation.format_line(0.7, m, 1.25) == \
        '| psi 0.7 | track kid 0.25 prdc 1.0000 0.5000 0.7500 0.2500 | r@1 0.5000 | 1.2 s |'


def test_trainer_defaults_are_off_and_the_generators_carry_none():
    import trainer
    import trainer_bert
    from sbagan import nets
    for cls in (trainer.condGANTrainer, trainer_bert.condGANTrainer):
        assert cls.truncation is None and cls.truncation_sweep is None
        assert (cls.truncation_n, cls.truncation_sweep_n) == (16384, 0)
    assert nets._GBase.truncation is None
    for cls in (nets.G_NET, nets.G_NET_BERT, nets.G_NET_MIX):
        assert 'truncation' not in cls.__dict__


def test_psi_is_held_against_the_stages():
    from sbagan.truncation import stage_psi
    assert stage_psi(0.7, 2) == (0.7, 0.7) and stage_psi(0.7, 3) == (0.7, 0.7) and stage_psi((1.0, 0.0), 3) == (1.0, 0.0)
    for psi, branches in ((1.5, 3), (-0.1, 3), (float('nan'), 3), ((0.5, 1.5), 3), ((0.5, 0.5), 2), (0.5, 1),
                          ((0.1, 0.2, 0.3), 3)):
        with pytest.raises(ValueError):
            stage_psi(psi, branches)


# ------------------------------------------------------------------ the reference against itself
def test_the_formula_at_psi_1_is_not_a_copy_which_is_why_the_kernel_copies():
    rng = np.random.RandomState(3)
    w = rng.standard_normal((64, 32)).astype(np.float32)
    w_avg = (0.1 * rng.standard_normal(32)).astype(np.float32)
    by_formula = R.style_truncate(w, w_avg, 1.0, copy_at_one=False)
    assert not np.array_equal(by_formula.view(np.int32), w.view(np.int32))
    assert np.allclose(by_formula, w, rtol=0, atol=2.0 ** -22 * np.abs(w).max())      # (a few ulps, not more)
    assert np.array_equal(R.style_truncate(w, w_avg, 1.0).view(np.int32), w.view(np.int32))


def test_psi_0_gives_w_avg_plus_zero_times_the_difference():
    rng = np.random.RandomState(4)
    w = rng.standard_normal((5, 7)).astype(np.float32)
    w_avg = rng.standard_normal(7).astype(np.float32)
    got = R.style_truncate(w, w_avg, 0.0)
    assert np.array_equal(got, np.broadcast_to(w_avg, w.shape))
    w[2, 3] = np.inf                    # 0 * inf: the formula's NaN, not w_avg
    w[1, 0] = np.nan
    got = R.style_truncate(w, w_avg, 0.0)
    assert np.isnan(got[2, 3]) and np.isnan(got[1, 0]) and np.isfinite(got).sum() == got.size - 2


@pytest.mark.parametrize('n,D', [(1, 1), (255, 3), (256, 5), (257, 4), (600, 9)])
def test_the_ordered_mean_is_within_its_bound_of_numpy(n, D):
    rng = np.random.RandomState(n + D)
    w = (rng.standard_normal((n, D)) * 3 + 1).astype(np.float32)
    mean64, mean32 = R.style_mean(w)
    assert mean64.dtype == np.float64 and mean32.dtype == np.float32
    want = np.mean(w.astype(np.float64), axis=0)
    assert np.abs(mean64 - want).max() <= n * 2.0 ** -53 * np.abs(w).max()
    assert np.array_equal(mean32, mean64.astype(np.float32))
    # the order is the contract: the stated chunking, restated with numpy's cumulative sum (sequential in float64)
    parts = [np.cumsum(w[lo:lo + 256].astype(np.float64), axis=0)[-1] for lo in range(0, n, 256)]
    total = np.cumsum(np.stack(parts), axis=0)[-1]
    assert np.array_equal((total / n).view(np.int64), mean64.view(np.int64))


def test_a_nan_or_inf_in_a_column_reaches_that_column_only():
    rng = np.random.RandomState(9)
    w = rng.standard_normal((300, 4)).astype(np.float32)
    clean = R.style_mean(w)[0]
    w[7, 1], w[290, 3] = np.nan, np.inf
    got = R.style_mean(w)[0]
    assert np.isnan(got[1]) and np.isposinf(got[3]) and np.array_equal(got[[0, 2]], clean[[0, 2]])


# ------------------------------------------------------------------ the two JSON files
def test_the_schema_of_truncation_json():
    from sbagan.truncation import check_record
    good = {'psi': [0.5, 0.5], 'n': 600, 'seed': 100, 'w_avg_norm': 1.25, 'w_rms_distance': 3.5, 'w_rows': 6}
    assert check_record(dict(good)) == good
    assert check_record(dict(good, w_rms_distance=None, w_rows=0))['w_rms_distance'] is None
    for bad in (dict(good, psi=[0.5]), dict(good, psi=[0.5, 1.5]), dict(good, psi=0.5), dict(good, n=0),
                dict(good, n=(1 << 20) + 1), dict(good, n=1.5), dict(good, seed=-1), dict(good, w_avg_norm=-1.0),
                dict(good, w_avg_norm='1'), dict(good, w_rms_distance=-2.0), dict(good, extra=1),
                {k: v for k, v in good.items() if k != 'seed'}, [good]):
        with pytest.raises(ValueError):
            check_record(bad)


def test_the_schema_of_truncation_sweep_json():
    from sbagan.truncation import check_sweep
    rec = {'psi': 1.0, 'seconds': 0.5, 'metrics': {'kid': {'kid': 0.1}, 'prdc': {'precision': 1.0}}}
    good = [rec, dict(rec, psi=0.5)]
    assert check_sweep(good) is good
    for bad in ([], rec, [dict(rec, psi=1.5)], [rec, dict(rec)], [dict(rec, seconds=-1)], [dict(rec, metrics={})],
                [dict(rec, metrics={'swd': {}})], [dict(rec, metrics={'kid': 0.1})], [dict(rec, epoch=3)],
                [{k: v for k, v in rec.items() if k != 'seconds'}]):
        with pytest.raises(ValueError):
            check_sweep(bad)
