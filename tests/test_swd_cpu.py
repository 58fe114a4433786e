"""The sliced Wasserstein distance without a GPU: the numpy reference (tests/swd_ref.py) against scipy and against its own
definition (exactness of the float64 pyramid, a distance of zero, symmetry, a case that can be checked by hand), the
recorded draw order, the command-line flag, the evaluator's refusals, the binding, and an emulation of the kernels'
arithmetic that shows what the bounds of tests/test_swd_gpu.py let through and what they catch."""
import ctypes
import hashlib
import math
import os

import numpy as np
import pytest
import torch

import swd_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K1 = np.array([1, 4, 6, 4, 1], dtype=np.int64)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


# ------------------------------------------------------------------ the pyramid is exact in float64
@pytest.mark.parametrize('size,levels', [(16, 2), (32, 2), (64, 3), (256, 5)])
def test_pyramid_equals_scipy_mirror_convolution_bit_for_bit(size, levels):
    from scipy import ndimage
    img = np.random.RandomState(size).randint(0, 256, (size, size)).astype(np.uint8)
    K = np.outer(swd_ref.K1, swd_ref.K1) / 256.0
    g, want = img.astype(np.float64), []
    for _ in range(levels - 1):
        nxt = ndimage.convolve(g, K, mode='mirror')[::2, ::2]
        z = np.zeros_like(g)
        z[::2, ::2] = nxt
        want.append(g - ndimage.convolve(z, 4.0 * K, mode='mirror'))
        g = nxt
    want.append(g)
    got = swd_ref.laplacian_pyramid(img, levels=levels)
    assert [v.shape for v in got] == [(size >> lv, size >> lv) for lv in range(levels)]
    for a, b in zip(got, want):
        assert np.array_equal(bits(a), bits(b))


def test_pyramid_is_bit_equal_under_the_reversed_tap_order_at_256_px():
    """every level is an integer over a power of two with at most 46 significant bits, so float64 adds the taps without
    rounding in any order; float32 does not"""
    img = np.random.RandomState(7).randint(0, 256, (3, 256, 256)).astype(np.uint8)
    fwd = swd_ref.laplacian_pyramid(img)
    rev = swd_ref.laplacian_pyramid(img, reverse=True)
    for lv, (a, b) in enumerate(zip(fwd, rev)):
        assert np.array_equal(bits(a), bits(b)), lv
        scaled = a * 2.0 ** (8 * lv + (14 if lv < 4 else 0))
        assert np.array_equal(scaled, np.round(scaled)) and np.abs(scaled).max() < 2.0 ** 46
    f32 = swd_ref.laplacian_pyramid(img, dtype=np.float32)
    assert max(np.abs(a - b).max() for a, b in zip(fwd, f32)) > 1e-6


# ------------------------------------------------------------------ the distance
def test_a_set_against_itself_with_the_same_positions_is_exactly_zero():
    imgs = swd_ref.make_images(64, 3, seed=1)
    drawn = [(cr, cr, dirs) for cr, _, dirs in swd_ref.draws(100, 64, 3)]
    assert (swd_ref.swd(imgs, imgs, drawn) == 0.0).all()


def test_the_distance_is_symmetric_in_its_sides():
    a, b = swd_ref.make_images(64, 2, seed=1), swd_ref.make_images(64, 2, seed=2)
    drawn = swd_ref.draws(100, 64, 2)
    swapped = [(cf, cr, dirs) for cr, cf, dirs in drawn]
    ab, ba = swd_ref.swd(a, b, drawn), swd_ref.swd(b, a, swapped)
    assert (ab > 0.0).all() and np.array_equal(bits(ab), bits(ba))


def test_an_image_against_its_inverse_can_be_checked_by_hand():
    """one image a side, the generated one 255 - real, the same positions: every Laplacian level changes its sign (the
    filters keep a constant), the last level becomes 255 - G; after the normalisation every descriptor is the negative
    of its partner, so the sorted projections of one side are the reversed negatives of the other's and the distance of
    a direction is mean_i |a_(i) + a_(m-1-i)| of the REAL side's sorted projections alone"""
    real = swd_ref.make_images(32, 1, seed=3)
    fake = 255 - real
    drawn = [(cr, cr, dirs) for cr, _, dirs in swd_ref.draws(100, 32, 1)]
    pr, pf = swd_ref.laplacian_pyramid(real), swd_ref.laplacian_pyramid(fake)
    assert np.array_equal(pf[0], -pr[0]) and np.array_equal(pf[1], 255.0 - pr[1])
    got = swd_ref.swd(real, fake, drawn)
    for lv, (cr, _, dirs) in enumerate(drawn):
        a = np.sort(swd_ref.project(swd_ref.gather(pr[lv], cr, 128), dirs), axis=1)
        by_hand = np.abs(a + a[:, ::-1]).mean(axis=1).mean()
        assert by_hand > 0.01 and abs(got[lv] - by_hand) <= 1e-12


def test_two_descriptor_case_with_a_closed_form():
    """descriptors +1 / -1 on every entry against the same with the third channel swapped: mean 0 and deviation 1 per
    channel, projections +-s and +-t with s = sum of the direction, t = s - 2 (sum over the third channel): the distance
    of a direction is | |s| - |t| |"""
    one = np.ones(147)
    flip = np.concatenate([np.ones(98), -np.ones(49)])
    dirs = swd_ref.draws(5, 32, 1)[0][2][:, :16]
    got = swd_ref.level_distance(np.stack([one, -one]), np.stack([flip, -flip]), dirs)
    s, t = dirs.sum(axis=0), dirs[:98].sum(axis=0) - dirs[98:].sum(axis=0)
    assert abs(got - np.abs(np.abs(s) - np.abs(t)).mean()) <= 1e-14


def test_the_draw_order_is_pinned_by_a_recorded_digest():
    from sbagan import swd
    drawn = swd_ref.draws(100, 64, 2)
    h = hashlib.sha256()
    for cr, cf, dirs in drawn:
        h.update(cr.astype(np.int64).tobytes())
        h.update(cf.astype(np.int64).tobytes())
        h.update(dirs.tobytes())
    assert h.hexdigest() == '4b47055fcdc4f58118d409161c2452630545294d6638cc21158288526bc0c1c5'
    assert drawn[0][0][:3].tolist() == [[11, 47], [27, 19], [6, 54]]
    # the evaluator draws the same, and touches no global generator
    np.random.seed(3)
    torch.manual_seed(3)
    before = (np.random.get_state()[1].copy(), torch.get_rng_state())
    mine = swd.draw(100, 64, 2)
    assert np.array_equal(np.random.get_state()[1], before[0]) and torch.equal(torch.get_rng_state(), before[1])
    assert len(mine) == len(drawn) == 3
    for (a, b, c), (x, y, z) in zip(mine, drawn):
        assert a.dtype == b.dtype == np.int32 and a.shape == (256, 2) and c.shape == (147, 512)
        assert np.array_equal(a, x) and np.array_equal(b, y) and np.array_equal(bits(c), bits(z))
        assert a.min() >= 3 and np.allclose((c * c).sum(axis=0), 1.0, rtol=0, atol=150 * 2.0 ** -53)
    assert max(v.max() for v in (mine[2][0], mine[2][1])) <= 16 - 4


# ------------------------------------------------------------------ the interface
def test_swd_flag_in_all_four_entry_points(capsys):
    import main
    import main_bert
    import pretrain_DAMSM
    import pretrain_DAMSM_bert
    for mod in (main, main_bert, pretrain_DAMSM, pretrain_DAMSM_bert):
        assert mod.parse_args([]).swd == 0
        assert mod.parse_args(['--swd', '16384']).swd == 16384
        assert mod.parse_args(['--swd', '0']).swd == 0
        for bad in ('-1', 'many', '1.5'):
            with pytest.raises(SystemExit):
                mod.parse_args(['--swd', bad])
    capsys.readouterr()
    from trainer import condGANTrainer
    import trainer_bert
    for cls in (condGANTrainer, trainer_bert.condGANTrainer):
        assert cls.swd == 0 and cls.swd_seed == 100 and cls.swd_result is None and cls.swd_evaluator is None
    assert '--swd N' in open(os.path.join(ROOT, 'sba-gan_amd', 'miscc', 'cli.py')).read().split('"""')[1]


def test_class_arguments_and_refusals():
    from sbagan import ops
    from sbagan.swd import FIELDS, SWD
    assert sorted(FIELDS) == ['dir_repeats', 'dirs_per_repeat', 'levels', 'n_images', 'patches_per_image', 'resolutions',
                              'seed', 'size', 'swd_avg_x1e3', 'swd_x1e3']
    assert [ops.swd_levels(s) for s in (32, 64, 128, 256)] == [2, 3, 4, 5]
    for bad in (dict(max_images=0, size=64), dict(max_images=2.0, size=64), dict(max_images=True, size=64),
                dict(max_images=4, size=16), dict(max_images=4, size=96), dict(max_images=4, size=512),
                dict(max_images=4, size=64.0), dict(max_images=4, size=64, capacity=0)):
        with pytest.raises(ValueError):
            SWD(**bad)
    ev = SWD(4, size=64)
    assert ev.count('real') == 0 and ev.count('fake') == 0 and ev.seed == 100 and ev.levels == 3
    with pytest.raises(ValueError):
        ev.count('both')
    with pytest.raises(RuntimeError):                           # CPU images are refused
        ev.update('real', torch.zeros(2, 3, 64, 64))
    with pytest.raises(ValueError):
        ev.update('real', torch.zeros(2, 3, 32, 32))
    with pytest.raises(RuntimeError, match='same number of images, at least one: 0 real, 0 generated'):
        ev.result()
    # unequal counts are refused before anything is launched (host buffers stand in for the device ones here)
    ev._held = {'real': [torch.zeros(4, 3, 64, 64, dtype=torch.uint8), 3],
                'fake': [torch.zeros(4, 3, 64, 64, dtype=torch.uint8), 2]}
    assert (ev.count('real'), ev.count('fake')) == (3, 2)
    with pytest.raises(RuntimeError, match='3 real, 2 generated'):
        ev.result()

    class Store(object):                # a shared store of another size is refused
        size = 128
    with pytest.raises(ValueError, match='128'):
        SWD(4, size=64, images=Store())


def test_operators_refuse_cpu_tensors_and_bad_arguments():
    from sbagan import ops
    imgs = torch.zeros(2, 3, 32, 32, dtype=torch.uint8)
    centres = np.full((2, 2), 5, dtype=np.int32)
    with pytest.raises(RuntimeError):
        ops.swd_descriptors(imgs, 0, centres)
    with pytest.raises(TypeError):
        ops.swd_descriptors(imgs.numpy(), 0, centres)
    for fn, args in ((ops.swd_project, (torch.zeros(2, 147, dtype=torch.float64), torch.zeros(6, dtype=torch.float64),
                                       torch.zeros(147, 4, dtype=torch.float64))),
                     (ops.swd_sort_columns, (torch.zeros(2, 5, dtype=torch.float64),)),
                     (ops.swd_abs_mean, (torch.zeros(2, 5, dtype=torch.float64), torch.zeros(2, 5, dtype=torch.float64)))):
        with pytest.raises(RuntimeError):
            fn(*args)


def test_entry_points_refuse_without_a_device():
    """validation comes before any launch or copy: these return SBA_E_ARG on a machine without a GPU"""
    from sbagan import _lib
    buf = (ctypes.c_double * 4096)()
    p = ctypes.addressof(buf)
    centres = (ctypes.c_int32 * 2)(5, 5)
    c = ctypes.addressof(centres)
    d = _lib.lib.sba_swd_descriptors
    assert d(p, 1, 48, 0, c, 1, p, p, p, 1 << 20, None) == -1           # a size outside the set
    assert d(p, 1, 32, 2, c, 1, p, p, p, 1 << 20, None) == -1           # 32 px has levels 0 and 1
    assert d(p, 0, 32, 0, c, 1, p, p, p, 1 << 20, None) == -1
    assert d(p, 1, 32, 0, c, 0, p, p, p, 1 << 20, None) == -1
    assert d(None, 1, 32, 0, c, 1, p, p, p, 1 << 20, None) == -1
    assert d(p, 1, 32, 0, c, 1, p + 4, p, p, 1 << 20, None) == -1
    assert d(p, 1, 32, 0, c, 1, p, p, p, 48 + 8 - 1, None) == -1        # the workspace one byte short
    for x, y, level in ((2, 5, 0), (5, 29, 0), (13, 5, 1), (5, -1, 1)):
        centres[0], centres[1] = x, y
        assert d(p, 1, 32, level, c, 1, p, p, p, 1 << 20, None) == -1, (x, y, level)
    assert _lib.lib.sba_swd_project(p, 0, p, p, 4, p, p, 1 << 20, None) == -1
    assert _lib.lib.sba_swd_project(p, 4, p, p, 0, p, p, 1 << 20, None) == -1
    assert _lib.lib.sba_swd_project(p, 4, p, p, 65536, p, p, 1 << 30, None) == -1
    assert _lib.lib.sba_swd_project(p, 4, p, p, 4, p, p, 8 * 148 * 4 - 1, None) == -1
    assert _lib.lib.sba_swd_sort_columns(None, None, 1, 1, None) == -1
    assert _lib.lib.sba_swd_sort_columns(p, None, 1, 2049, None) == -1  # longer than a tile: the second buffer is needed
    assert _lib.lib.sba_swd_sort_columns(p, p, 1, 2049, None) == -1
    assert _lib.lib.sba_swd_sort_columns(p, None, 0, 4, None) == -1
    assert _lib.lib.sba_swd_abs_mean(p, p, 1, 0, p, p, 8, None) == -1
    assert _lib.lib.sba_swd_abs_mean(p, p + 4, 1, 4, p, p, 8, None) == -1
    assert _lib.lib.sba_swd_abs_mean(p, p, 2, 4097, p, p, 8 * 2 * 2 - 1, None) == -1


def test_header_declares_what_the_binding_binds():
    from sbagan import _lib
    decls = {name: (d.ret, ['%s %s' % (ctext, arg) for ctext, arg, _ in d.params])
             for name, d in _lib.DECLS.items() if name.startswith('sba_swd_')}
    assert sorted(decls) == ['sba_swd_abs_mean', 'sba_swd_descriptors', 'sba_swd_project', 'sba_swd_sort_columns']
    for name, (ret, args) in decls.items():
        sig = _lib.SIGNATURES[name]
        assert ret == 'int' and len(sig) == len(args), name
        for ctype, arg in zip(sig, args):
            want = ctypes.c_void_p if '*' in arg else ctypes.c_int64 if 'int64_t' in arg else ctypes.c_int
            assert ctype is want, (name, arg)


# ------------------------------------------------------------------ what the GPU bounds let through and what they catch
def emulated_descriptors(images, level, centres, patches, boundary='reflect', order='cyx'):
    """the kernel's arithmetic: integer levels I_l = G_l 2^(8 l), Lap_l = (2^14 I_l - sum k_i k_j Z_{l+1}) / 2^(8 l + 14)"""
    S = images.shape[-1]
    levels = swd_ref.levels_of(S)
    pad = [(0, 0), (0, 0), (2, 2), (2, 2)]
    cur = images.astype(np.int64)
    for _ in range(level):
        cur = _int_filter(np.pad(cur, pad, mode=boundary), cur.shape[-1])[..., ::2, ::2]
    if level == levels - 1:
        lap = cur.astype(np.float64) / 2.0 ** (8 * level)
    else:
        n = cur.shape[-1]
        nxt = _int_filter(np.pad(cur, pad, mode=boundary), n)[..., ::2, ::2]
        z = np.zeros_like(cur)
        z[..., ::2, ::2] = nxt
        lap = (cur * 16384 - _int_filter(np.pad(z, pad, mode=boundary), n)).astype(np.float64) / 2.0 ** (8 * level + 14)
    return swd_ref.gather(lap, centres, patches, order)


def _int_filter(xp, n):
    out = np.zeros(xp.shape[:-2] + (n, n), dtype=np.int64)
    for i in reversed(range(5)):
        for j in reversed(range(5)):
            out += K1[i] * K1[j] * xp[..., i:i + n, j:j + n]
    return out


def emulated_project(desc, dirs, ddof=0):
    """sba_swd_project's formulation -- (d - mu) * (dir * (1 / sigma)), the statistics from compensated sums -- with the
    contraction in descending k"""
    m = desc.shape[0]
    N = m * 49.0
    d3 = desc.reshape(m, 3, 49)
    s1 = np.array([math.fsum(d3[::-1, c, ::-1].reshape(-1)) for c in range(3)])
    mu = s1 / N
    s2 = np.array([math.fsum(((d3[::-1, c, ::-1] - mu[c]) ** 2).reshape(-1)) for c in range(3)])
    inv = 1.0 / np.sqrt(s2 / (N - ddof))
    ch = np.repeat(np.arange(3), 49)
    w = dirs * inv[ch][:, None]
    out = np.zeros((m, dirs.shape[1]))
    for k in reversed(range(147)):
        out += (desc[:, k, None] - mu[ch[k]]) * w[None, k]
    return out.T, s1, s2


@pytest.fixture(scope='module')
def small_case():
    imgs = swd_ref.make_images(64, 3, seed=4)
    centres = np.random.RandomState(0).randint(3, 32 - 3, (15, 2))
    centres[:4] = [(3, 3), (28, 3), (3, 28), (28, 28)]
    desc = swd_ref.descriptors(imgs, 1, centres, 5)
    dirs = swd_ref.draws(9, 64, 1)[1][2][:, :130]
    return imgs, centres, desc, dirs


def test_an_emulated_correct_kernel_passes_every_bound(small_case):
    imgs, centres, desc, dirs = small_case
    for level, side in ((0, 64), (1, 32), (2, 16)):
        c = np.minimum(centres, side - 4)
        assert np.array_equal(bits(emulated_descriptors(imgs, level, c, 5)), bits(swd_ref.descriptors(imgs, level, c, 5)))
    got, s1, s2 = emulated_project(desc, dirs)
    d3 = desc.reshape(-1, 3, 49)
    for c in range(3):
        vals = d3[:, c].reshape(-1)
        assert abs(s1[c] - math.fsum(vals)) <= swd_ref.sum_bound(vals)
        dev = (vals - math.fsum(vals) / vals.size) ** 2
        assert abs(s2[c] - math.fsum(dev)) <= swd_ref.sum_bound(dev) + 4 * swd_ref.U * math.fsum(dev)
    err, bound = np.abs(got - swd_ref.project(desc, dirs)), swd_ref.projection_bound(desc, dirs)
    assert err.max() > 0.0 and (err <= bound).all() and bound.max() < 1e-11
    a, b = np.sort(got, axis=1), np.sort(got[::-1] * 1.25, axis=1)
    chunked = np.array([sum(np.abs(ra - rb)[::-1].tolist()) for ra, rb in zip(a, b)]) / a.shape[1]
    assert (np.abs(chunked - swd_ref.abs_mean(a, b)) <= swd_ref.abs_mean_bound(a, b)).all()
    # end to end: another summation order stays within 16 x the float64 / extended-precision difference
    real, fake = swd_ref.make_images(32, 2, seed=5), swd_ref.make_images(32, 2, seed=6)
    drawn = swd_ref.draws(100, 32, 2)
    ref, _, diff, bound = swd_ref.end_to_end_bound(real, fake, drawn)
    emu = []
    for lv, (cr, cf, dr) in enumerate(drawn):
        pa = np.sort(emulated_project(swd_ref.descriptors(real, lv, cr, 128), dr)[0], axis=1)
        pb = np.sort(emulated_project(swd_ref.descriptors(fake, lv, cf, 128), dr)[0], axis=1)
        emu.append(np.abs(pa - pb).mean(axis=1).mean())
    print('f64 against extended precision: %.3g, bound %.3g, emulation off by %.3g' % (diff, bound, np.abs(emu - ref).max()))
    assert 0.0 < diff < 1e-14 and (np.abs(emu - ref) <= bound).all()


@pytest.mark.parametrize('mutation', ['edge_repeated', 'ddof_1', 'order_yxc'])
def test_a_mutated_kernel_fails_the_bounds(small_case, mutation):
    imgs, centres, desc, dirs = small_case
    if mutation == 'ddof_1':
        got, _, _ = emulated_project(desc, dirs, ddof=1)
        assert (np.abs(got - swd_ref.project(desc, dirs)) > swd_ref.projection_bound(desc, dirs)).any()
        return
    kw = dict(boundary='symmetric') if mutation == 'edge_repeated' else dict(order='yxc')
    wrong = [not np.array_equal(emulated_descriptors(imgs, lv, np.minimum(centres, (64 >> lv) - 4), 5, **kw),
                                swd_ref.descriptors(imgs, lv, np.minimum(centres, (64 >> lv) - 4), 5))
             for lv in range(3)]
    assert all(wrong), wrong
    real, fake = swd_ref.make_images(32, 2, seed=5), swd_ref.make_images(32, 2, seed=6)
    drawn = swd_ref.draws(100, 32, 2)
    ref, _, _, bound = swd_ref.end_to_end_bound(real, fake, drawn)
    assert (np.abs(swd_ref.swd(real, fake, drawn, **kw) - ref) > bound).all()
