"""--track on the host: the schedule, the flags and their refusals, the jsonl writer, the best-so-far logic, and that
importing sbagan.track loads no device library."""
import json
import math
import subprocess
import sys

import pytest


def _modules():
    import main
    import main_bert
    import pretrain_DAMSM
    import pretrain_DAMSM_bert
    return main, main_bert, pretrain_DAMSM, pretrain_DAMSM_bert


# ------------------------------------------------------------------ the schedule
@pytest.mark.parametrize('every', [1, 2, 3, 7])
@pytest.mark.parametrize('start', [0, 1, 5, 14])
def test_due_names_the_multiples_of_the_interval(every, start):
    from sbagan.track import due
    last = start + 15
    got = [e for e in range(start, last) if due(e, every)]
    assert got == [e for e in range(start, last) if e % every == 0]
    assert got and all(b - a == every for a, b in zip(got, got[1:]))
    assert got[0] - start < every and (last - 1) - got[-1] < every          # none missed at either end
    assert due(last - 1, every) == ((last - 1) % every == 0)                # the last epoch is an epoch like any other


def test_due_is_off_at_zero_and_refuses_a_negative_interval():
    from sbagan.track import due
    assert not any(due(e, 0) for e in range(20))
    assert due(0, 5) and due(10, 5) and not due(9, 5)
    with pytest.raises(ValueError):
        due(3, -1)


# ------------------------------------------------------------------ flags
def test_defaults_and_values_on_the_gan_entry_points():
    main, main_bert = _modules()[:2]
    for mod in (main, main_bert):
        a = mod.parse_args([])
        assert (a.track, a.track_split, a.track_n, a.track_captions, a.track_best) == (0, 'test', 0, 1, None)
        a = mod.parse_args(['--track', '3', '--track_split', 'train', '--track_n', '64', '--track_captions', '2',
                            '--track_best', 'prdc.coverage', '--prdc', '5'])
        assert (a.track, a.track_split, a.track_n, a.track_captions, a.track_best) == (3, 'train', 64, 2, 'prdc.coverage')


@pytest.mark.parametrize('argv, why', [
    (['--track', '-1', '--kid'], 'argument --track: E must be 0 (off) or an interval in epochs'),
    (['--track', 'x', '--kid'], 'argument --track: invalid'),
    (['--track', '1.5', '--kid'], 'argument --track: invalid'),
    (['--track', '1', '--kid', '--track_n', '-1'], 'argument --track_n: N must be 0 (the whole split) or a number'),
    (['--track', '1', '--kid', '--track_captions', '0'], 'argument --track_captions: C must be a number of captions'),
    (['--track', '1', '--kid', '--track_best', 'kid'], "argument --track_best: unknown key 'kid'; valid keys are fid.fid,"),
    (['--track', '1', '--kid', '--track_best', 'kid.kid_std'], "argument --track_best: unknown key 'kid.kid_std'"),
    (['--track', '1', '--kid', '--track_best', 'ms_ssim.ms_ssim_fake'], "argument --track_best: unknown key"),
    (['--track', '1', '--kid', '--track_best', 'fid.fid'], 'error: --track_best fid.fid needs --fid'),    # not on
])
def test_flags_out_of_range_are_refused_at_parse_time(argv, why, capsys):
    for mod in _modules()[:2]:
        with pytest.raises(SystemExit):
            mod.parse_args(argv)
        err = capsys.readouterr().err
        assert why in err and 'unrecognized arguments' not in err, err


def test_best_table_and_its_directions():
    from sbagan import evaluation, track
    assert list(track.BEST_KEYS.items()) == [
        ('fid.fid', -1), ('kid.kid', -1), ('prdc.precision', 1), ('prdc.recall', 1), ('prdc.density', 1),
        ('prdc.coverage', 1), ('r_precision.r_at_1', 1)]
    stems = [rec.stem for rec in evaluation.EVALUATORS]
    assert sorted(track.TRACKED + track.NOT_TRACKED) == sorted(stems)
    assert {k.split('.')[0] for k in track.BEST_KEYS} == set(track.TRACKED)
    main = _modules()[0]
    on = {'fid': ['--fid'], 'kid': ['--kid'], 'prdc': ['--prdc', '3'], 'r_precision': ['--r_precision', '4']}
    for key in track.BEST_KEYS:
        assert main.parse_args(['--track', '1', '--track_best', key] + on[key.split('.')[0]]).track_best == key


def test_track_without_a_tracked_evaluator_is_refused_with_their_names(capsys):
    from sbagan import track
    for mod in _modules()[:2]:
        for extra in ([], ['--ms_ssim', '4'], ['--swd', '8', '--nearest', '2']):
            with pytest.raises(SystemExit):
                mod.parse_args(['--track', '1'] + extra)
            err = capsys.readouterr().err
            for flag in ('--fid', '--kid', '--prdc', '--r_precision'):
                assert flag in err
        for on in (['--fid'], ['--kid'], ['--prdc', '2'], ['--r_precision', '3']):
            assert mod.parse_args(['--track', '1'] + on).track == 1
        assert mod.parse_args(['--ms_ssim', '4']).track == 0         # (without --track nothing is asked)

    class Args(object):
        track, kid, track_best = 1, True, None
    assert track.check_flags(Args) is None
    Args.kid = False
    assert '--r_precision' in track.check_flags(Args)


def test_the_damsm_parsers_accept_and_ignore_the_flags():
    for mod in _modules()[2:]:
        a = mod.parse_args(['--track', '2', '--track_split', 'test', '--track_n', '8', '--track_captions', '1'])
        assert a.track == 2 and a.track_n == 8                       # no tracked evaluator on: not their business
        a = mod.parse_args(['--track', '1', '--kid', '--track_best', 'kid.kid'])
        assert a.track_best == 'kid.kid'
        assert mod.parse_args(['--track', '1', '--track_best', 'fid.fid']).track_best == 'fid.fid'      # (ignored whole)
        assert mod.parse_args([]).track == 0


def test_not_tracked_line_and_tracked_values():
    from sbagan import evaluation, track
    main = _modules()[0]
    a = main.parse_args(['--track', '1', '--kid'])
    assert track.not_tracked_line(a) is None
    a = main.parse_args(['--track', '1', '--kid', '--swd', '8'])
    assert track.not_tracked_line(a) == '--track: --swd is not tracked in training (sampling only)'
    a = main.parse_args(['--track', '1', '--kid', '--ms_ssim', '2', '--nearest', '3'])
    assert track.not_tracked_line(a) == '--track: --ms_ssim, --nearest are not tracked in training (sampling only)'
    values = {opt.name: opt.default for opt in evaluation.OPTIONS}
    values.update(kid=True, kid_subsets=7, prdc=3, ms_ssim=5, swd=9, nearest=2, nearest_show=3, nearest_stats='x.npz')
    got = track.tracked_values(values)
    assert got['kid'] is True and got['kid_subsets'] == 7 and got['prdc'] == 3
    assert (got['ms_ssim'], got['swd'], got['nearest'], got['nearest_stats'], got['nearest_show']) == (0, 0, 0, None, 16)
    assert values['swd'] == 9                                        # (a copy: the trainer's own values stay)


def test_trainer_attributes_default_to_off():
    import trainer
    import trainer_bert
    for cls in (trainer.condGANTrainer, trainer_bert.condGANTrainer):
        assert (cls.track, cls.track_split, cls.track_n, cls.track_captions, cls.track_best) == (0, 'test', 0, 1, None)
    assert 'track' not in trainer_bert.condGANTrainer.__dict__


# ------------------------------------------------------------------ the writer and the line
def test_jsonl_writer_appends(tmp_path):
    from sbagan import track
    path = str(tmp_path / 'track.jsonl')
    recs = [{'epoch': e, 'metrics': {'kid': {'kid': 0.5 / (e + 1), 'kid_std': float('nan')}}} for e in range(3)]
    for i, r in enumerate(recs):
        track.append_jsonl(path, r)
        lines = open(path).read().split('\n')
        assert len(lines) == i + 2 and lines[-1] == ''               # one line each, the earlier ones kept
    back = [json.loads(line) for line in open(path)]
    assert [r['epoch'] for r in back] == [0, 1, 2]
    assert back[1]['metrics']['kid']['kid'] == 0.25 and math.isnan(back[2]['metrics']['kid']['kid_std'])


def test_printed_line():
    from sbagan.track import format_line
    m = {'kid': {'kid': 0.0125}, 'fid': {'fid': 31.5}, 'r_precision': {'r_at_1': 0.25},
         'prdc': {'precision': 0.5, 'recall': 0.25, 'density': 1.5, 'coverage': 0.75}}
    assert format_line(7, m, 1.26) == ('| end epoch 7 | track kid 0.0125 fid 31.5 prdc 0.5000 0.2500 1.5000 0.7500 |'
                                      ' r@1 0.2500 | 1.3 s |')
    assert format_line(0, {'kid': m['kid']}, 0.04) == '| end epoch 0 | track kid 0.0125 | 0.0 s |'


# ------------------------------------------------------------------ best so far
def _run(best, figures):
    """offer a scripted sequence of (epoch, figure); returns the epochs that were taken"""
    return [e for e, v in figures if best.offer(v, e, 10 * e)]


def test_best_lower_is_better_with_ties_and_nan(tmp_path):
    from sbagan.track import Best
    nan = float('nan')
    best = Best('kid.kid', str(tmp_path))
    taken = _run(best, [(0, nan), (1, 0.5), (2, 0.7), (3, 0.5), (4, nan), (5, 0.25), (6, None), (7, 0.25), (8, 0.3)])
    assert taken == [1, 5]                                           # ties keep the earlier epoch, a NaN is never best
    held = json.load(open(str(tmp_path / 'best.json')))
    assert held == {'key': 'kid.kid', 'value': 0.25, 'epoch': 5, 'iteration': 50}


def test_best_higher_is_better(tmp_path):
    from sbagan.track import Best
    best = Best('prdc.coverage', str(tmp_path))
    taken = _run(best, [(0, 0.1), (1, 0.1), (2, 0.05), (3, float('nan')), (4, 0.4), (5, 0.4), (6, -1.0)])
    assert taken == [0, 4]
    assert json.load(open(str(tmp_path / 'best.json')))['epoch'] == 4
    assert not best.improves(float('nan')) and not best.improves(0.4) and best.improves(0.41)
    assert not best.improves(True) and not best.improves('0.9')


def test_nan_first_leaves_no_file(tmp_path):
    from sbagan.track import Best
    best = Best('fid.fid', str(tmp_path))
    assert _run(best, [(0, float('nan')), (1, float('nan'))]) == []
    assert not (tmp_path / 'best.json').exists() and best.value is None


def test_best_json_is_honoured_on_resume(tmp_path, capsys):
    from sbagan.track import Best
    old, new = tmp_path / 'old', tmp_path / 'new'
    old.mkdir(), new.mkdir()
    first = Best('kid.kid', str(old))
    assert _run(first, [(0, 0.5), (1, 0.2)]) == [0, 1]
    resumed = Best('kid.kid', str(new), resume_dir=str(old))
    assert resumed.value == 0.2 and resumed.epoch == 1
    assert _run(resumed, [(2, 0.3), (3, 0.2)]) == []                 # worse and equal: the earlier run's best stays
    assert not (new / 'best.json').exists()
    assert _run(resumed, [(4, 0.1)]) == [4]
    assert json.load(open(str(new / 'best.json')))['epoch'] == 4
    assert json.load(open(str(old / 'best.json')))['epoch'] == 1     # (the file resumed from is read, never written)
    other = Best('fid.fid', str(new), resume_dir=str(old))           # another key: nothing to honour
    assert other.value is None and _run(other, [(5, 9.0)]) == [5]
    assert Best('kid.kid', str(new), resume_dir=str(tmp_path / 'none')).value is None
    with pytest.raises(ValueError):
        Best('kid.kid_std', str(new))
    capsys.readouterr()


def test_first_images_view_forwards_and_survives_a_copy():
    import copy
    from sbagan.track import _First

    class DS(object):
        filenames = ['a', 'b', 'c']

        def __len__(self):
            return 3
    view = _First(DS(), 2)
    assert len(view) == 2 and view.filenames == ['a', 'b', 'c']
    with pytest.raises(AttributeError):
        view.nothing_of_the_kind
    assert len(copy.copy(view)) == 2 and len(copy.deepcopy(view)) == 2           # (no recursion through __getattr__)
    with pytest.raises(AttributeError):
        _First.__new__(_First).dataset


def test_fid_stats_are_read_once_and_handed_on(tmp_path, capsys):
    """the cache= route of evaluation.Suite: the first Suite reads --fid_stats and checks its key, later ones take the
    statistics from the caller's dict (the file is not opened again); another key is refused as in sampling()"""
    import os

    import numpy as np
    from miscc import cli
    from miscc.config import cfg, reset_cfg
    from sbagan import evaluation
    from sbagan.feature_rows import dtype_name
    from sbagan.fid import stats_key
    reset_cfg()
    cfg.TRAIN.NET_E = ''

    class Trunk(object):
        def pooled_features(self, images):
            raise AssertionError('no image goes through the trunk here')
    rng = np.random.RandomState(0)
    mu, a = rng.randn(2048), rng.randn(2048, 8)
    path = str(tmp_path / 'stats.npz')
    key = stats_key('', dtype_name(), 'test', cli.image_size())
    np.savez(path, n=np.int64(9), mu=mu, sigma=a @ a.T, trace=np.float64(np.trace(a @ a.T)), key=np.str_(key))
    values = {opt.name: opt.default for opt in evaluation.OPTIONS}
    values.update(fid=True, fid_stats=path)
    args = (values, 'test', None, Trunk, None, 2, 'cpu')
    cache = {}
    first = evaluation.Suite(*args, cache=cache)
    first.attach(None)
    assert capsys.readouterr().out.count('Load real FID statistics from:') == 1
    assert first.on['fid'].is_loaded('real') and first._real_rows == [] and sorted(cache) == ['fid_real']
    os.remove(path)
    second = evaluation.Suite(*args, cache=cache)
    second.attach(None)
    assert capsys.readouterr().out == ''
    fid = second.on['fid']
    assert fid is not first.on['fid'] and fid.is_loaded('real') and second._real_rows == []
    n, mu2, sigma2, trace2 = fid.real_stats()
    assert n == 9 and np.array_equal(mu2, mu) and np.array_equal(sigma2, a @ a.T) and trace2 == np.trace(a @ a.T)
    with pytest.raises(RuntimeError, match='takes no more rows'):
        fid.update_features('real', None)
    with pytest.raises(ValueError):
        fid.set_real((1, mu, a @ a.T, 0.0))
    # a file written under another key
    np.savez(path, n=np.int64(9), mu=mu, sigma=a @ a.T, trace=np.float64(1.0), key=np.str_(key + '|other'))
    with pytest.raises(ValueError, match='holds statistics for'):
        evaluation.Suite(*args, cache={}).attach(None)
    reset_cfg()


def test_figure_reads_a_record():
    from sbagan.track import BEST_KEYS, figure
    m = {'fid': {'fid': 1.0}, 'kid': {'kid': 2.0}, 'r_precision': {'r_at_1': 3.0},
         'prdc': {'precision': 4.0, 'recall': 5.0, 'density': 6.0, 'coverage': 7.0}}
    assert [figure(m, k) for k in BEST_KEYS] == [1.0, 2.0, 4.0, 5.0, 6.0, 7.0, 3.0]


# ------------------------------------------------------------------ the import
def test_importing_the_module_loads_no_device_library():
    import os
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'sba-gan_amd')
    code = ('import sys; sys.path.insert(0, %r); import sbagan.track, sbagan.evaluation; '
            'bad = [m for m in ("sbagan._lib", "sbagan.ops", "sbagan.trainer", "sbagan.inception_hip") if m in sys.modules]; '
            'assert not bad, bad' % pkg)
    subprocess.check_call([sys.executable, '-c', code])
