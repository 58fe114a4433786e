"""MS-SSIM evaluation on the host: the float64 numpy reference (tests/msssim_ref.py) on the cases with a known answer,
that the bound of the GPU test has teeth (two summation orders of the reference agree far below it, a float32 evaluation
misses it), draw_pairs, combine, quantize against trainer._to_uint8, the flag, the class's arguments, the operator's
refusal of CPU tensors, the workspace size and the header / binding agreement.  (The kernel is tested on the GPU in
tests/test_msssim_gpu.py.)"""
import ctypes
import random

import numpy as np
import pytest
import torch

import msssim_ref

C1, C2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2
H, W = 176, 208                     # five scales, the last one 11 x 13


@pytest.fixture(scope='module')
def six_kinds():
    """{kind: (x, y, reference means [3][5][2])}, computed once"""
    return {k: (x, y, msssim_ref.scale_means(x, y, 5)) for k, (x, y) in msssim_ref.kinds(H, W).items()}


# ------------------------------------------------------------------ the reference
def test_window_and_pooling():
    g = msssim_ref.window()
    assert g.shape == (11,) and abs(g.sum() - 1.0) < 1e-15 and np.array_equal(g, g[::-1]) and g.argmax() == 5
    assert abs(g[4] / g[5] - np.exp(-1.0 / 4.5)) < 1e-15
    a = np.arange(5 * 7, dtype=np.float64).reshape(5, 7)
    p = msssim_ref.pool(a)                                      # the odd row and the odd column are dropped
    assert p.shape == (2, 3) and p[0, 0] == (0 + 1 + 7 + 8) / 4.0 and p[1, 2] == (18 + 19 + 25 + 26) / 4.0
    # pooling s times is the mean of the 2^s x 2^s block of the original, at floor(H / 2^s) rows
    b = np.random.RandomState(0).randint(0, 256, (45, 47)).astype(np.float64)
    pp = msssim_ref.pool(msssim_ref.pool(msssim_ref.pool(b)))
    assert pp.shape == (45 >> 3, 47 >> 3)
    assert np.array_equal(pp, b[:40, :40].reshape(5, 8, 5, 8).mean(axis=(1, 3)))


def test_identical_images_give_exactly_one(six_kinds):
    x, y, ref = six_kinds['identical']
    assert np.array_equal(x, y) and ref.shape == (3, 5, 2) and (ref == 1.0).all()
    assert (msssim_ref.combine(ref[None]) == 1.0).all()


def test_swapping_a_pair_changes_nothing(six_kinds):
    for kind, (x, y, ref) in six_kinds.items():
        assert np.array_equal(msssim_ref.scale_means(y, x, 5), ref), kind


def test_two_constant_images():
    """mx = a, my = b and the variances vanish: cs = 1 and ssim = (2ab + C1) / (a^2 + b^2 + C1) at every scale (the
    window sums to 1 within rounding, so the variances vanish within a few ulp of 65025 over C2 = 58.5)"""
    for a, b in ((255, 254), (0, 255), (17, 17), (0, 0), (128, 3)):
        x, y = np.full((1, H, W), a, dtype=np.uint8), np.full((1, H, W), b, dtype=np.uint8)
        got = msssim_ref.scale_means(x, y, 5)
        want = (2.0 * a * b + C1) / (a * a + b * b + C1)
        assert np.abs(got[0, :, 1] - 1.0).max() < 1e-12 and np.abs(got[0, :, 0] - want).max() < 1e-12, (a, b)


def test_out_of_range_pairs_are_nan_in_the_reference():
    imgs, _ = msssim_ref.kind_stack(12, 13)
    out = msssim_ref.pair_means(imgs, [(0, 1), (0, 12), (-1, 2), (3, 3)], 1)
    assert out.shape == (4, 3, 1, 2) and np.isnan(out[1]).all() and np.isnan(out[2]).all()
    assert np.isfinite(out[0]).all() and (out[3] == 1.0).all()


def test_the_bound_has_teeth(six_kinds):
    """The GPU test holds every per-scale mean to 1e-10 of the reference.  Two summation orders of the float64
    definition agree within 1e-12 on all six kinds, and a float32 evaluation of the same lines misses the reference by
    more than 1e-8 on the noise and the flat kinds: the bound sits between them with decades on either side."""
    for kind, (x, y, ref) in six_kinds.items():
        other = msssim_ref.scale_means(x, y, 5, order='cols')
        f32 = msssim_ref.scale_means(x, y, 5, dtype=np.float32)
        assert f32.dtype == np.float32
        d_order, d_f32 = np.abs(other - ref).max(), np.abs(f32.astype(np.float64) - ref).max()
        print('%-10s two f64 orders differ by %.3g, f32 misses by %.3g' % (kind, d_order, d_f32))
        assert d_order <= 1e-12, kind
        if kind in ('noise', 'flat'):
            assert d_f32 > 1e-8, kind


def test_reference_factors_are_zero_or_well_away_from_zero():
    """what the 1e-8 bound on the final values assumes (v^0.0448 is steep at 0): at the five-scale shapes of the GPU
    test no factor of the reference lies within 1e-3 of 0 on either side"""
    imgs, pairs = msssim_ref.kind_stack(H, W, seed=H)
    out = msssim_ref.pair_means(imgs, pairs, 5)
    raw = np.concatenate([out[:, :, :4, 1], out[:, :, 4:, 0]], axis=2)
    assert np.abs(raw).min() >= 1e-3 and (raw < 0).any()
    v = msssim_ref.factors(out)
    assert ((v == 0.0) | (v >= 1e-3)).all() and (v == 0.0).any()


# ------------------------------------------------------------------ draw_pairs
def test_draw_pairs_counts_order_and_classes():
    from sbagan.msssim import draw_pairs
    ids = np.array([7, 3, 7, 7, 3, 9, 7, 3, 5, 7], dtype=np.int64)     # class 7: 5 images, 3: 3, 9 and 5: one each
    pairs, used, skipped = draw_pairs(ids, 100, with_counts=True)
    assert pairs.dtype == np.int32 and pairs.shape == (3 + 10, 2) and (used, skipped) == (2, 2)
    # ascending class id, then the lexicographic order of (i < j) within the class
    assert pairs[:3].tolist() == [[1, 4], [1, 7], [4, 7]]
    assert pairs[3:].tolist() == [[0, 2], [0, 3], [0, 6], [0, 9], [2, 3], [2, 6], [2, 9], [3, 6], [3, 9], [6, 9]]
    assert np.array_equal(draw_pairs(ids, 100), pairs)
    # capped: class 3 keeps its 3 pairs, class 7 gets 4 of its 10, sorted by pair number
    capped = draw_pairs(ids, 4, seed=100)
    assert capped.shape == (3 + 4, 2) and capped[:3].tolist() == pairs[:3].tolist()
    want = np.sort(np.random.RandomState(100).choice(10, 4, replace=False))
    assert capped[3:].tolist() == pairs[3:][want].tolist()
    for got in (pairs, capped):
        assert (got[:, 0] < got[:, 1]).all() and (ids[got[:, 0]] == ids[got[:, 1]]).all()      # no cross-class pair
        assert len({tuple(p) for p in got.tolist()}) == len(got)                                # no pair twice


def test_draw_pairs_one_generator_for_the_whole_call_and_private():
    from sbagan.msssim import draw_pairs
    ids = np.repeat(np.arange(4), 6)[np.random.RandomState(3).permutation(24)]         # 4 classes x 6 images: 15 pairs
    random.seed(7)
    np.random.seed(7)
    torch.manual_seed(7)
    before = (random.getstate(), np.random.get_state(), torch.get_rng_state())
    a, b, c = draw_pairs(ids, 5, seed=100), draw_pairs(ids, 5, seed=100), draw_pairs(ids, 5, seed=101)
    after = (random.getstate(), np.random.get_state(), torch.get_rng_state())
    assert before[0] == after[0] and torch.equal(before[2], after[2])
    assert before[1][0] == after[1][0] and np.array_equal(before[1][1], after[1][1]) and before[1][2:] == after[1][2:]
    assert a.shape == (20, 2) and np.array_equal(a, b) and not np.array_equal(a, c)
    rng = np.random.RandomState(100)                    # ONE RandomState: the classes draw from it one after the other
    i, j = np.triu_indices(6, 1)
    for k, cls in enumerate(range(4)):
        pos = np.flatnonzero(ids == cls)
        pick = np.sort(rng.choice(15, 5, replace=False))
        assert a[5 * k:5 * k + 5].tolist() == np.stack([pos[i[pick]], pos[j[pick]]], axis=1).tolist()
    assert len({tuple(p) for p in a.tolist()}) == 20
    # the default seed is 100
    assert np.array_equal(draw_pairs(ids, 5), a)


def test_draw_pairs_skipped_classes_and_bad_arguments():
    from sbagan.msssim import draw_pairs
    pairs, used, skipped = draw_pairs([4, 2, 9], 3, with_counts=True)
    assert pairs.shape == (0, 2) and pairs.dtype == np.int32 and (used, skipped) == (0, 3)
    pairs, used, skipped = draw_pairs([1, 1, 1, 2, 2, 3], 2, with_counts=True)
    assert len(pairs) == 2 + 1 and (used, skipped) == (2, 1) and pairs[2].tolist() == [3, 4]
    assert draw_pairs(np.zeros(0, dtype=np.int64), 1).shape == (0, 2)
    for bad in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            draw_pairs([1, 1], bad)


# ------------------------------------------------------------------ combine and quantize
def test_combine_against_a_hand_computation():
    from sbagan.msssim import WEIGHTS, combine
    assert WEIGHTS == (0.0448, 0.2856, 0.3001, 0.2363, 0.1333) == msssim_ref.WEIGHTS
    out = np.zeros((2, 3, 5, 2))
    out[..., 0] = 0.123                                          # the ssim of the scales 0 .. 3 is never used
    cs = [0.9, 0.8, 0.7, 0.6]
    for ch, last in enumerate((0.5, 0.25, 1.0)):
        out[0, ch, :4, 1], out[0, ch, 4, 0], out[0, ch, 4, 1] = cs, last, -3.0     # nor is the cs of the last scale
    base = 0.9 ** 0.0448 * 0.8 ** 0.2856 * 0.7 ** 0.3001 * 0.6 ** 0.2363
    want0 = base * (0.5 ** 0.1333 + 0.25 ** 0.1333 + 1.0) / 3.0
    # pair 1: a negative factor is clipped to 0 and zeroes its channel alone
    out[1, :, :4, 1], out[1, :, 4, 0] = cs, 0.5
    out[1, 1, 2, 1] = -0.2
    want1 = base * 0.5 ** 0.1333 * 2.0 / 3.0
    got = combine(out)
    assert got.shape == (2,) and abs(got[0] - want0) < 1e-15 and abs(got[1] - want1) < 1e-15
    assert np.abs(msssim_ref.combine(out) - got).max() < 1e-15
    # fewer scales: the first S weights
    small = np.zeros((1, 3, 2, 2))
    small[0, :, 0, 1], small[0, :, 1, 0] = 0.9, 0.5
    assert abs(combine(small)[0] - 0.9 ** 0.0448 * 0.5 ** 0.2856) < 1e-15
    for bad in (np.zeros((2, 3, 5)), np.zeros((2, 4, 5, 2)), np.zeros((2, 3, 6, 2)), np.zeros((2, 3, 5, 3))):
        with pytest.raises(ValueError):
            combine(bad)


def test_quantize_equals_to_uint8():
    from sbagan.msssim import quantize
    from trainer import _to_uint8
    rng = np.random.RandomState(0)
    k = np.arange(0, 257, dtype=np.float64)
    edges = np.concatenate([k / 127.5 - 1.0, (k + 0.5) / 127.5 - 1.0, [-1.0, 1.0, -1.5, 1.5, -100.0, 100.0, 0.0, -0.0]])
    edges = np.concatenate([edges, np.nextafter(edges.astype(np.float32), np.float32(2)).astype(np.float64),
                            np.nextafter(edges.astype(np.float32), np.float32(-2)).astype(np.float64)])
    vals = np.concatenate([edges, rng.uniform(-1.1, 1.1, 3 * 40 * 50 * 2 - edges.size)]).astype(np.float32)
    imgs = torch.from_numpy(vals.reshape(2, 3, 40, 50))
    for t in (imgs, imgs.to(torch.bfloat16), imgs.double()):
        q = quantize(t)
        assert q.dtype == torch.uint8 and q.shape == t.shape and q.device == t.device
        for b in range(2):
            assert np.array_equal(q[b].numpy().transpose(1, 2, 0), _to_uint8(t[b]))
    assert quantize(imgs).min() == 0 and quantize(imgs).max() == 255


# ------------------------------------------------------------------ the interface
def test_ms_ssim_flag_in_all_four_entry_points(capsys):
    import main
    import main_bert
    import pretrain_DAMSM
    import pretrain_DAMSM_bert
    for mod in (main, main_bert, pretrain_DAMSM, pretrain_DAMSM_bert):
        assert mod.parse_args([]).ms_ssim == 0
        assert mod.parse_args(['--ms_ssim', '100']).ms_ssim == 100
        assert mod.parse_args(['--ms_ssim', '0']).ms_ssim == 0
        for bad in ('-1', 'many', '1.5'):
            with pytest.raises(SystemExit):
                mod.parse_args(['--ms_ssim', bad])
    capsys.readouterr()
    from trainer import condGANTrainer
    import trainer_bert
    for cls in (condGANTrainer, trainer_bert.condGANTrainer):
        assert cls.ms_ssim == 0 and cls.ms_ssim_seed == 100
        assert cls.ms_ssim_result is None and cls.ms_ssim_evaluator is None


def test_class_arguments_and_cpu_images():
    from sbagan.msssim import FIELDS, MIN_SIZE, MSSSIM
    assert MIN_SIZE == 176 == 11 << 4
    assert sorted(FIELDS) == ['classes', 'classes_skipped', 'ms_ssim_fake', 'ms_ssim_fake_std', 'ms_ssim_real',
                              'ms_ssim_real_std', 'n_images', 'pairs', 'pairs_per_class', 'scales', 'seed', 'size']
    for bad in (dict(per_class=0), dict(per_class=2.0), dict(per_class=True), dict(per_class=2, size=175),
                dict(per_class=2, size=128), dict(per_class=2, size=1025), dict(per_class=2, capacity=0)):
        with pytest.raises(ValueError):
            MSSSIM(**bad)
    ev = MSSSIM(2, size=176)
    assert ev.count('real') == 0 and ev.count('fake') == 0 and ev.seed == 100 and ev.size == 176
    with pytest.raises(ValueError):
        ev.count('both')
    with pytest.raises(RuntimeError):                           # CPU images are refused
        ev.update('real', torch.zeros(2, 3, 176, 176), [1, 1])
    with pytest.raises(ValueError):
        ev.update('real', torch.zeros(2, 3, 128, 128), [1, 1])
    with pytest.raises(RuntimeError, match='no class holds two images'):
        ev.result()


def test_operator_refuses_cpu_tensors():
    from sbagan import ops
    imgs = torch.zeros(2, 3, 16, 16, dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        ops.msssim_pairs(imgs, np.zeros((1, 2), dtype=np.int32), 1)
    with pytest.raises(TypeError):
        ops.msssim_pairs(imgs.numpy(), np.zeros((1, 2), dtype=np.int32), 1)


def test_header_declares_what_the_binding_binds():
    from sbagan import _lib
    decls = {name: (d.ret, ['%s %s' % (ctext, arg) for ctext, arg, _ in d.params])
             for name, d in _lib.DECLS.items() if name.startswith('sba_msssim_')}
    assert sorted(decls) == ['sba_msssim_pairs', 'sba_msssim_workspace_bytes']
    ret, args = decls['sba_msssim_pairs']
    sig = _lib.SIGNATURES['sba_msssim_pairs']
    assert ret == 'int' and len(sig) == len(args) == 11
    for ctype, arg in zip(sig, args):                           # pointers to pointers, ints to ints, int64_t to int64
        want = ctypes.c_void_p if '*' in arg else ctypes.c_int64 if 'int64_t' in arg else ctypes.c_int
        assert ctype is want, arg
    assert _lib.lib.sba_msssim_pairs.restype is ctypes.c_int
    ret, args = decls['sba_msssim_workspace_bytes']
    size = _lib.lib.sba_msssim_workspace_bytes
    assert ret == 'int64_t' and size.restype is ctypes.c_int64 and list(size.argtypes) == [ctypes.c_int] * len(args)


def test_workspace_size_needs_no_device_and_does_not_grow_with_n():
    """one {ssim, cs} pair of f64 per (pair, channel, tile of 16 x 32 window positions of every scale); the image
    count is not even an argument"""
    from sbagan import _lib
    size = _lib.lib.sba_msssim_workspace_bytes

    def tiles(H, W, scales):
        return sum(-(-((H >> s) - 10) // 16) * -(-((W >> s) - 10) // 32) for s in range(scales))
    assert tiles(256, 256, 5) == 128 + 32 + 8 + 2 + 1
    for H, W, P, S in ((11, 11, 1, 1), (12, 27, 3, 1), (22, 23, 2, 2), (45, 47, 2, 3), (176, 176, 2, 5), (177, 208, 3, 5),
                       (256, 256, 4, 5), (256, 256, 5000, 5), (1024, 1024, 1000, 5), (176, 176, 1 << 20, 5)):
        assert size(H, W, P, S) == P * 3 * tiles(H, W, S) * 16, (H, W, P, S)
    for bad in ((10, 11, 1, 1), (11, 10, 1, 1), (175, 256, 1, 5), (256, 175, 1, 5), (21, 22, 1, 2), (1025, 256, 1, 1),
                (256, 1025, 1, 1), (256, 256, 0, 5), (256, 256, -1, 5), (256, 256, (1 << 20) + 1, 5), (256, 256, 1, 0),
                (256, 256, 1, 6), (0, 0, 1, 1), (1024, 1024, 1 << 20, 1)):       # (the last: a grid past 2^31)
        assert size(*bad) == -1, bad
