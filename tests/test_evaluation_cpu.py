"""sbagan.evaluation's table against what is generated from it or must agree with it: the trainers' class attributes, the
command line of the four entry points, and the integer bounds the parser and the suite each enforce."""
import pytest


def _modules():
    import main
    import main_bert
    import pretrain_DAMSM
    import pretrain_DAMSM_bert
    return main, main_bert, pretrain_DAMSM, pretrain_DAMSM_bert


def test_table_order_and_names():
    from sbagan import evaluation as ev
    assert [rec.stem for rec in ev.EVALUATORS] == ['r_precision', 'fid', 'prdc', 'kid', 'ms_ssim', 'swd', 'nearest']
    assert [opt.name for opt in ev.OPTIONS] == [
        'r_precision', 'r_precision_seed', 'fid', 'fid_stats', 'prdc', 'kid', 'kid_subsets', 'kid_subset_size',
        'kid_seed', 'ms_ssim', 'ms_ssim_seed', 'swd', 'swd_seed', 'nearest', 'nearest_stats', 'nearest_show']
    for rec in ev.EVALUATORS:
        assert rec.options[0].name == rec.stem and not rec.options[0].default      # the switch, off by default
        assert rec.line.count('%') - 2 * rec.line.count('%%') == len(rec.fields)
    from sbagan import ops
    assert ev.MAX_K == ops.PRDC_MAX_K == ops.KNN_MAX_K


def test_defaults_equal_the_class_attributes_of_both_trainers():
    import trainer
    import trainer_bert
    from sbagan import evaluation as ev
    want = dict(r_precision=0, r_precision_seed=100, fid=False, fid_stats=None, prdc=0, kid=False, kid_subsets=100,
                kid_subset_size=1000, kid_seed=100, ms_ssim=0, ms_ssim_seed=100, swd=0, swd_seed=100, nearest=0,
                nearest_stats=None, nearest_show=16)
    assert {opt.name: opt.default for opt in ev.OPTIONS} == want
    for cls in (trainer.condGANTrainer, trainer_bert.condGANTrainer):
        for opt in ev.OPTIONS:
            assert getattr(cls, opt.name) == opt.default and type(getattr(cls, opt.name)) is type(opt.default), opt.name
        for rec in ev.EVALUATORS:
            assert getattr(cls, rec.stem + '_result') is None and getattr(cls, rec.stem + '_evaluator') is None
        assert 'fid' not in trainer_bert.condGANTrainer.__dict__        # inherited, not restated


def test_defaults_equal_the_empty_command_line_of_all_four_entry_points():
    from sbagan import evaluation as ev
    flags = [opt for opt in ev.OPTIONS if opt.help is not None]
    assert [opt.name for opt in ev.OPTIONS if opt.help is None] == ['r_precision_seed', 'kid_seed', 'ms_ssim_seed',
                                                                   'swd_seed']
    for mod in _modules():
        args = mod.parse_args([])
        for opt in flags:
            assert getattr(args, opt.name) == opt.default and type(getattr(args, opt.name)) is type(opt.default)
        for opt in ev.OPTIONS:
            assert hasattr(args, opt.name) == (opt.help is not None)


def _suite(values):
    from sbagan import evaluation as ev
    full = {opt.name: opt.default for opt in ev.OPTIONS}
    full.update(values)
    return ev.Suite(full, 'test', None, None, None, 2, 'cpu')


def test_parser_and_suite_refuse_the_same_integers(capsys):
    """at lo - 1 and hi + 1 both refuse; at lo and hi the parser accepts and the suite's check passes (builders that
    would then run are kept out by leaving the evaluator's switch off, or are the check's own subject below)"""
    from sbagan import evaluation as ev
    main = _modules()[0]
    ranged = [(rec, opt) for rec in ev.EVALUATORS for opt in rec.options if opt.lo is not None]
    assert [opt.name for _, opt in ranged] == ['r_precision', 'prdc', 'kid_subsets', 'kid_subset_size', 'ms_ssim', 'swd',
                                               'nearest', 'nearest_show']
    assert [(opt.lo, opt.hi) for _, opt in ranged] == [(2, None), (1, 8), (1, 1024), (2, None), (1, None), (1, None),
                                                       (1, 8), (0, None)]
    for rec, opt in ranged:
        switch = rec.options[0]
        on = {} if opt is switch else {switch.name: True if switch.default is False else switch.lo}
        inside = [opt.lo] + ([opt.hi] if opt.hi is not None else [opt.lo + 1000])
        outside = [opt.lo - 1] + ([opt.hi + 1] if opt.hi is not None else [])
        for v in inside:
            assert getattr(main.parse_args(['--' + opt.name, str(v)]), opt.name) == v
            ev._int_option(opt.name, v, opt.lo, opt.hi, opt.what)
        for v in outside:
            if v != opt.default:            # (0 = off where the default is 0: the parser takes it, the suite skips it)
                with pytest.raises(SystemExit):
                    main.parse_args(['--' + opt.name, str(v)])
            if v or opt is not switch:
                with pytest.raises(ValueError, match=r'^%s must be .* \(got %d\)$' % (opt.name, v)):
                    _suite(dict(on, **{opt.name: v}))
        for v in (True, 2.0, '3'):          # not an integer at all
            with pytest.raises(ValueError, match='^%s must be ' % opt.name):
                _suite(dict(on, **{opt.name: v}))
        assert getattr(main.parse_args(['--' + opt.name, str(opt.default)]), opt.name) == opt.default
    capsys.readouterr()


def test_suite_messages_are_the_trainers_own():
    with pytest.raises(ValueError) as e:
        _suite({'prdc': 9})
    assert str(e.value) == 'prdc must be 0 (off) or a neighbour count from 1 to 8 (got 9)'
    with pytest.raises(ValueError) as e:
        _suite({'nearest': -1})
    assert str(e.value) == 'nearest must be 0 (off) or a neighbour count from 1 to 8 (got -1)'
    with pytest.raises(ValueError) as e:
        _suite({'r_precision': 1})
    assert str(e.value) == 'r_precision must be 0 (off) or >= 2 candidates per image (got 1)'
    with pytest.raises(ValueError) as e:
        _suite({'ms_ssim': -2})
    assert str(e.value) == 'ms_ssim must be 0 (off) or a number of pairs per class (got -2)'
    with pytest.raises(ValueError) as e:
        _suite({'swd': 2.5})
    assert str(e.value) == 'swd must be 0 (off) or a number of images per side (got 2.5)'


def test_a_suite_with_nothing_on_builds_nothing_and_routes_nothing(tmp_path):
    suite = _suite({})
    suite.attach(None)
    suite.update(None, None, None, None, None)
    assert suite.on == {} and suite.image_encoder is None and suite.finish(str(tmp_path)) == {}
    assert list(tmp_path.iterdir()) == []
