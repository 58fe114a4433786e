"""--geoaug without a GPU: the float64 reference (tests/geoaug_ref.py) against torch's grid_sample route and numpy's
permutations, its adjointness, its bounds against an f32 emulation of a correct kernel and of six broken ones, the
policy parser, the row layout, the command line, the C entry points' refusals (they come back before any launch) and
the trainer's defaults."""
import ctypes

import numpy as np
import pytest
import torch

import geoaug_ref as R

NEW = ('sba_geoaug_prepare', 'sba_geoaug_fwd', 'sba_geoaug_bwd')


def _torch_route(x, M):
    n, _, S, _ = x.shape
    theta = torch.zeros((n, 2, 3), dtype=torch.float64)
    theta[:, :, :2] = torch.from_numpy(np.asarray(M, dtype=np.float64).reshape(n, 2, 2))
    xt = torch.from_numpy(x).requires_grad_(True)
    grid = torch.nn.functional.affine_grid(theta, (n, 3, S, S), align_corners=True)
    return xt, torch.nn.functional.grid_sample(xt, grid, 'bilinear', 'zeros', align_corners=True)


@pytest.mark.parametrize('S', [8, 10, 20])
def test_reference_is_torchs_grid_sample_and_its_autograd(S):
    rng = np.random.RandomState(S)
    u = np.concatenate([rng.random_sample((3, 8)).astype(np.float32), R.edge_rows()])
    M, on = R.matrices(u, 15)
    assert on.tolist() == [15] * len(u)
    x, g = rng.standard_normal((len(u), 3, S, S)), rng.standard_normal((len(u), 3, S, S))
    xt, out = _torch_route(x, M)
    assert np.abs(out.detach().numpy() - R.forward(x, M)).max() < 5e-14
    out.backward(torch.from_numpy(g))
    assert np.abs(xt.grad.numpy() - R.backward(g, M)).max() < 5e-14
    # <fwd(x), g> == <x, bwd(g)>
    lhs, rhs = float((R.forward(x, M) * g).sum()), float((x * R.backward(g, M)).sum())
    assert abs(lhs - rhs) < 1e-11 * max(1.0, abs(lhs))


@pytest.mark.parametrize('S', [8, 10, 256])
def test_flip_and_rot90_are_numpys_permutations_bit_for_bit_in_f32(S):
    x = np.random.RandomState(S).standard_normal((1, 3, S, S)).astype(np.float32)
    for flipped in (False, True):
        for k in range(4):
            u = np.zeros((1, 8), dtype=np.float32)
            u[0, 0], u[0, 1] = (0.5 if flipped else 0.25), (k + 0.5) / 4
            M, _ = R.matrices(u, R.FLIP | R.ROT90)
            m32 = R.emulate_matrices(u, np.array([3], dtype=np.int32))
            assert np.array_equal(M, m32) and set(np.abs(M).ravel()) == {0.0, 1.0}
            want = np.rot90(x[:, :, :, ::-1] if flipped else x, k, axes=(2, 3))
            assert np.array_equal(R.forward(x, M), want)
            assert np.array_equal(R.emulate_forward(x, m32), want)
            # the adjoint of a permutation is its inverse
            assert np.array_equal(R.backward(want, M), x)
            if S <= 10:
                assert np.array_equal(R.emulate_backward(want, m32), x)
    ident, _ = R.matrices(np.zeros((1, 8), dtype=np.float32), 15, gates=np.ones((1, 4), np.float32), p=[0.5], rows_per_p=1)
    assert ident.tolist() == [[1.0, 0.0, 0.0, 1.0]] and np.array_equal(R.forward(x, ident), x)


def test_draws_and_gates():
    u = R.edge_rows()
    flipped, k, s, theta = R.draws(u)
    assert k[0] == 3 and s[1] == 1.0 and bool(flipped[2]) and not bool(flipped[7])
    assert abs(s[3] - R.S_MAX) < 1e-12 and abs(s[4] - 1 / R.S_MAX) < 1e-12
    assert theta[5] == -np.pi and np.pi - 1e-6 < theta[6] < np.pi
    assert (s >= 1 / R.S_MAX - 1e-12).all() and (s <= R.S_MAX + 1e-12).all()
    # the largest box the backward has to cover: 2 s sqrt 2 px
    assert 2 * R.S_MAX * np.sqrt(2) < 4.29 and R.WINDOW == 7
    gates = np.array([[0.1, 0.6, 0.4, 0.5]] * 4, dtype=np.float32)
    on = R.parts_on(15, 4, gates, [0.5, np.nan], 2)
    assert on.tolist() == [5, 5, 0, 0]
    assert R.parts_on(10, 4, gates, [1.0, 0.0], 2).tolist() == [10, 10, 0, 0]
    assert R.parts_on(7, 3).tolist() == [7, 7, 7]
    # a flip that is on but drawn "off" by u0 counts as applied and leaves the matrix alone
    u0 = np.zeros((1, 8), dtype=np.float32)
    M, on = R.matrices(u0, R.FLIP)
    assert on.tolist() == [1] and M.tolist() == [[1.0, 0.0, 0.0, 1.0]]


def test_the_constants_are_those_of_the_measurement():
    m, f, b = R.measure()
    print('measured: matrix %.3g, forward ratio %.3g, backward ratio %.3g' % (m, f, b))
    assert m <= R.MEASURED_MATRIX < 1.25 * m
    assert f <= R.MEASURED_FWD < 1.25 * f
    assert b <= R.MEASURED_BWD < 1.25 * b
    assert (R.MATRIX_BOUND, R.FWD_K, R.BWD_K) == (4 * R.MEASURED_MATRIX, 4 * R.MEASURED_FWD, 4 * R.MEASURED_BWD)


def test_matrix_bound_passes_the_emulation_and_fails_the_mutations():
    rng = np.random.RandomState(9)
    u = np.concatenate([rng.random_sample((2000, 8)).astype(np.float32), R.edge_rows()])
    for flags in range(1, 16):
        ref, on = R.matrices(u, flags)
        assert np.abs(R.emulate_matrices(u, on) - ref).max() <= R.MATRIX_BOUND, flags
    ref, on = R.matrices(u, 15)
    for mutate in ('theta', 'k', 's', 'flip_last'):
        err = np.abs(R.emulate_matrices(u, on, mutate) - ref).max(1)
        if mutate == 'flip_last':           # (the order matters on the flipped rows only)
            err = err[R.draws(u)[0]]
        assert (err > R.MATRIX_BOUND).mean() > 0.9, (mutate, (err > R.MATRIX_BOUND).mean())


@pytest.mark.parametrize('S,n', R.SHAPES)
def test_warp_bounds_pass_the_emulation_and_fail_the_mutations(S, n):
    mats, x, g = R.case_mats(n), R.case_images(n, S, 1), R.case_images(n, S, 2)
    out, dx = R.forward(x, mats), R.backward(g, mats)
    assert R.ratio(R.emulate_forward(x, mats), out, R.forward_bound(x, mats)) <= 1
    assert R.ratio(R.emulate_backward(g, mats), dx, R.backward_bound(g, mats)) <= 1
    assert R.ratio(R.emulate_forward(x, mats, 'axis'), out, R.forward_bound(x, mats)) > 100
    assert R.ratio(R.emulate_backward(g, mats, 'window'), dx, R.backward_bound(g, mats)) > 100
    if n > 1:       # the constant image: the interior exactly, the corners (45 degrees: outside the source) zero
        e = R.emulate_forward(x[1:2], R.case_mats(1))
        assert (e[0, :, S // 2 - 1:S // 2 + 1, S // 2 - 1:S // 2 + 1] == np.float32(0.75)).all()
        assert (e[0, :, [0, 0, -1, -1], [0, -1, 0, -1]] == 0).all()


def test_policy_parsing_and_row_layout():
    from sbagan import geoaug, ops
    assert geoaug.parse_policy('flip,rot90,scale,rotate') == 15 and geoaug.parse_policy(' rotate , flip') == 9
    assert (ops.GEOAUG_FLIP, ops.GEOAUG_ROT90, ops.GEOAUG_SCALE, ops.GEOAUG_ROTATE) == (1, 2, 4, 8)
    assert geoaug.POLICIES == R.NAMES
    for bad in ('', 'color', 'flip,', 'flip;rot90', 'Flip'):
        with pytest.raises(ValueError, match='--geoaug: unknown policy'):
            geoaug.parse_policy(bad)
    B, nD = 3, 2
    dev = torch.device('cpu')
    a = geoaug.GeoAugment('scale,flip', B, nD, dev)
    assert a.flags == 5 and not a.gated and a.gates is None and a.p is None
    assert tuple(a.uniforms.shape) == (nD * 3 * B, 8) and tuple(a.mats.shape) == (nD * 3 * B, 4)
    assert a.applied.dtype == torch.int32 and tuple(a.applied.shape) == (nD * 3 * B,)
    for i in range(nD):
        d, g = a.d_mats(i), a.g_mats(i)
        assert tuple(d.shape) == (2 * B, 4) and tuple(g.shape) == (B, 4)
        assert d.data_ptr() == a.mats.data_ptr() + 16 * (i * 3 * B)
        assert g.data_ptr() == a.mats.data_ptr() + 16 * (i * 3 * B + 2 * B)
        assert d.data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0 and d.is_contiguous() and g.is_contiguous()
    torch.manual_seed(1)
    a.draw()
    first = a.uniforms.clone()
    assert bool((first >= 0).all()) and bool((first < 1).all()) and bool(first.any())
    a.draw()
    assert not torch.equal(first, a.uniforms)
    with pytest.raises(RuntimeError, match='no CPU'):
        a.prepare()                         # the one launch: a HIP kernel, no CPU fall-back
    p = torch.zeros(nD)
    gated = geoaug.GeoAugment('rotate', B, nD, dev, p=p)
    assert gated.gated and gated.p is p and tuple(gated.gates.shape) == (nD * 3 * B, 4)
    gated.draw()
    assert bool(gated.gates.any())
    for bad in (torch.zeros(nD + 1), torch.zeros(nD, dtype=torch.float64)):
        with pytest.raises(ValueError, match='p must be'):
            geoaug.GeoAugment('rotate', B, nD, dev, p=bad)
    with pytest.raises(ValueError, match='positive'):
        geoaug.GeoAugment('rotate', 0, nD, dev)


def test_cli():
    from miscc import cli
    args = cli.options('t', 'cfg/bird_style.yml', ['--geoaug', 'flip, rot90'])
    assert args.geoaug == 'flip,rot90' and args.diffaug == ''
    assert cli.options('t', 'cfg/bird_style.yml', []).geoaug == ''
    args = cli.options('t', 'cfg/bird_style.yml', ['--diffaug', 'color', '--geoaug', 'flip,rot90,scale,rotate', '--ada',
                                                 '0.6'], bert=True)
    assert (args.geoaug, args.diffaug, args.ada) == ('flip,rot90,scale,rotate', 'color', 0.6)
    for argv in (['--geoaug', 'color'], ['--diffaug', 'color,flip'], ['--geoaug', 'flip', '--ada', '0.6'],
                 ['--geoaug', 'flip', '--diffaug_p', '0.5']):
        with pytest.raises(SystemExit):
            cli.options('t', 'cfg/bird_style.yml', argv)
    with open(cli.__file__) as f:
        assert '[--geoaug POLICY' in f.read().split('"""')[1]


def test_entry_points_are_declared_in_the_second_header_and_bound():
    from sbagan import _lib, abi
    for name in NEW:
        assert name in abi.EXT_DECLS and name not in abi.DECLS and abi.EXT_DECLS[name].ret == 'int'
        assert len(getattr(_lib.lib, name).argtypes) == len(abi.EXT_DECLS[name].params)
    d = abi.EXT_DECLS
    assert [p[1] for p in d['sba_geoaug_prepare'].params] == ['uniforms', 'gates', 'p_dev', 'rows_per_p', 'N', 'flags',
                                                             'mats', 'applied', 'stream']
    assert [p[1] for p in d['sba_geoaug_fwd'].params] == ['real', 'nr', 'fake', 'nf', 'mats', 'out', 'S', 'stream']
    assert [p[1] for p in d['sba_geoaug_bwd'].params] == ['dout', 'n', 'mats', 'dx', 'S', 'stream']


def test_refusals_come_back_before_any_launch():
    """host memory stands in for device memory: a refused call dereferences nothing and launches nothing"""
    from sbagan import _lib
    E = _lib.CONSTANTS['SBA_E_ARG']
    buf = (ctypes.c_float * 4096)()
    base = ctypes.addressof(buf)
    a16 = (base + 15) // 16 * 16
    lib = _lib.lib
    ok = dict(real=a16, nr=1, fake=a16 + 1024, nf=1, mats=a16 + 2048, out=a16 + 4096, S=8)

    def fwd(**kw):
        v = dict(ok, **kw)
        return lib.sba_geoaug_fwd(v['real'], v['nr'], v['fake'], v['nf'], v['mats'], v['out'], v['S'], None)

    for kw in (dict(S=6), dict(S=9), dict(S=4098), dict(nr=0, nf=0), dict(nr=-1), dict(nf=65536), dict(nr=40000, nf=40000),
               dict(real=None), dict(fake=None), dict(mats=None), dict(out=None), dict(real=a16 + 4), dict(fake=a16 + 8),
               dict(out=a16 + 4), dict(mats=a16 + 4)):
        assert fwd(**kw) == E, kw

    def bwd(dout=a16, n=1, mats=a16 + 2048, dx=a16 + 4096, S=8):
        return lib.sba_geoaug_bwd(dout, n, mats, dx, S, None)

    for kw in (dict(S=6), dict(S=11), dict(S=5000), dict(n=0), dict(n=65536), dict(dout=None), dict(mats=None),
               dict(dx=None), dict(dout=a16 + 4), dict(dx=a16 + 8), dict(mats=a16 + 12)):
        assert bwd(**kw) == E, kw

    def prepare(uniforms=a16, gates=None, p_dev=None, rows_per_p=1, N=4, flags=15, mats=a16 + 2048, applied=a16 + 4096):
        return lib.sba_geoaug_prepare(uniforms, gates, p_dev, rows_per_p, N, flags, mats, applied, None)

    for kw in (dict(N=0), dict(N=(1 << 20) + 1), dict(flags=0), dict(flags=16), dict(uniforms=None), dict(mats=None),
               dict(applied=None), dict(uniforms=a16 + 2), dict(mats=a16 + 4), dict(applied=a16 + 1),
               dict(gates=a16 + 512), dict(gates=a16 + 512, p_dev=a16 + 768, rows_per_p=0),
               dict(gates=a16 + 513, p_dev=a16 + 768), dict(gates=a16 + 512, p_dev=a16 + 770)):
        assert prepare(**kw) == E, kw
    assert not any(buf)


def test_trainer_defaults_are_off():
    import trainer
    from sbagan.trainer import GANStep
    assert GANStep.geo_augment is None and GANStep.augment is None
    assert trainer.condGANTrainer.geoaug == '' and trainer.condGANTrainer.diffaug == ''
    import inspect
    from miscc import losses
    for fn in (losses.discriminator_loss, losses.generator_d_term, losses.generator_loss):
        assert inspect.signature(fn).parameters['geo'].default is None


def test_step_refuses_the_two_pass_layouts_and_real_features():
    from miscc import losses
    from sbagan import geoaug
    from sbagan.trainer import GANStep
    geo = geoaug.GeoAugment('flip', 2, 1, torch.device('cpu'))

    class Warped(GANStep):
        geo_augment = geo

    class Overlapped(Warped):
        force_overlap_layout = True

    with pytest.raises(ValueError, match='--geoaug.*distributed'):
        Warped(None, None, None, 2, distributed=True)
    with pytest.raises(ValueError, match='--geoaug.*force_overlap_layout'):
        Overlapped(None, None, None, 2)
    x = torch.zeros((2, 3, 8, 8))
    with pytest.raises(ValueError, match='geo does not go with real_features'):
        losses.discriminator_loss(None, x, x, None, None, None, real_features=x, geo=geo.d_mats(0))
