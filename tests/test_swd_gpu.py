"""The sliced Wasserstein distance on the GPU: the four entry points of csrc/swd.hip through the raw C ABI against the numpy
reference (tests/swd_ref.py, whose bounds tests/test_swd_cpu.py shows to have teeth) -- descriptors with ==, the
statistics, the projection, the sort with ==, the mean -- guard elements, refusals, the SWD class end to end, and the
flag through main.main() on a toy data set."""
import functools
import glob
import io
import json
import math
import os

import numpy as np
import pytest
import torch

import sampling_harness as sh
import swd_ref

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
E_ARG = -1
SENTINEL = -7.0
GUARD = 64                          # f64 elements on either side of every output and workspace
T = 2048                            # the sort's tile: what one workgroup sorts in LDS; longer columns take merge passes
CHUNK = 4096                        # values per partial sum of sba_swd_abs_mean


def stream():
    return torch.cuda.current_stream().cuda_stream


def guarded(n, dtype=torch.float64):
    """(whole buffer, the n elements between the guards)"""
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf, n):
    h = buf.cpu().numpy()
    return bool((h[:GUARD] == SENTINEL).all() and (h[GUARD + n:] == SENTINEL).all())


def as_float(u8):
    """float images in [-1, 1] whose quantisation is `u8`: the middle of each byte's interval"""
    return (torch.as_tensor(u8).to(DEV).float() + 0.5) / 127.5 - 1.0


# ------------------------------------------------------------------ descriptors
SHAPES = [(32, 1, 1), (64, 3, 5), (256, 2, 128)]       # (S, n, P)


def kind_image(kind, S, seed):
    """[3][S][S] uint8: 0 random, 1 checkerboard, 2 all 0, 3 all 255"""
    if kind == 0:
        return np.random.RandomState(seed).randint(0, 256, (3, S, S)).astype(np.uint8)
    if kind == 1:
        yy, xx = np.mgrid[0:S, 0:S]
        return np.broadcast_to((((yy + xx) & 1) * 255).astype(np.uint8), (3, S, S)).copy()
    return np.full((3, S, S), 0 if kind == 2 else 255, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def desc_case(S, n, P, rot):
    """(images [n][3][S][S], per level: (centres int32 [n P][2], reference descriptors [n P][147])); image i is of kind
    (i + rot) % 4; the first centres of every level are its four extreme corners (3, 3) .. (Sl - 4, Sl - 4), as far as
    P goes (P = 1: corner `rot`)"""
    imgs = np.stack([kind_image((i + rot) % 4, S, seed=S + i) for i in range(n)])
    pyr = swd_ref.laplacian_pyramid(imgs)
    rng = np.random.RandomState(S + rot)
    per_level = []
    for lv, lap in enumerate(pyr):
        Sl = S >> lv
        c = np.stack([rng.randint(3, Sl - 3, n * P), rng.randint(3, Sl - 3, n * P)], axis=1).astype(np.int32)
        corners = [(3, 3), (Sl - 4, 3), (3, Sl - 4), (Sl - 4, Sl - 4)]
        if P == 1:
            c[0] = corners[rot]
        else:
            c[:4] = corners
        ref = swd_ref.gather(lap, c, P)
        c.setflags(write=False)
        ref.setflags(write=False)
        per_level.append((c, ref))
    imgs.setflags(write=False)
    return imgs, per_level


def raw_descriptors(imgs_dev, S, level, centres, P):
    """the C entry point between guard elements: (return code, desc [n P][147], stats [6]) on the host"""
    from sbagan import _lib
    n = imgs_dev.shape[0]
    m = n * P
    nbytes = 48 * n + 8 * n * P
    dbuf, desc = guarded(m * 147)
    sbuf, stats = guarded(6)
    wbuf, ws = guarded(nbytes // 8)
    host = np.ascontiguousarray(centres, dtype=np.int32)
    rc = _lib.lib.sba_swd_descriptors(imgs_dev.data_ptr(), n, S, level, host.ctypes.data, P, desc.data_ptr(),
                                      stats.data_ptr(), ws.data_ptr(), nbytes, stream())
    torch.cuda.synchronize()
    assert guards_intact(dbuf, m * 147) and guards_intact(sbuf, 6) and guards_intact(wbuf, nbytes // 8)
    return rc, desc.cpu().numpy().reshape(m, 147), stats.cpu().numpy()


@pytest.mark.parametrize('rot', range(4))
@pytest.mark.parametrize('S,n,P', SHAPES)
def test_descriptors_equal_the_reference_bit_for_bit_at_every_level(S, n, P, rot):
    imgs, per_level = desc_case(S, n, P, rot)
    imgs_dev = torch.from_numpy(imgs.copy()).to(DEV)
    assert len(per_level) == swd_ref.levels_of(S)
    for lv, (centres, ref) in enumerate(per_level):
        rc, got, stats = raw_descriptors(imgs_dev, S, lv, centres, P)
        assert rc == 0
        assert np.array_equal(got, ref), (lv, np.abs(got - ref).max())
        d3 = ref.reshape(-1, 3, 49)
        for c in range(3):
            vals = d3[:, c].reshape(-1)
            total = math.fsum(vals)
            assert abs(stats[c] - total) <= swd_ref.sum_bound(vals), (lv, c)
            dev = (vals - total / vals.size) ** 2
            assert abs(stats[3 + c] - math.fsum(dev)) <= swd_ref.sum_bound(dev) + 4 * swd_ref.U * math.fsum(dev), (lv, c)


def test_descriptors_through_the_wrapper_are_the_same_launch():
    from sbagan import ops
    S, n, P = SHAPES[1]
    imgs, per_level = desc_case(S, n, P, 0)
    imgs_dev = torch.from_numpy(imgs.copy()).to(DEV)
    for lv, (centres, ref) in enumerate(per_level):
        for c in (centres, centres.astype(np.int64)):
            desc, stats = ops.swd_descriptors(imgs_dev, lv, c)
            assert desc.dtype == torch.float64 and tuple(desc.shape) == (n * P, 147) and tuple(stats.shape) == (6,)
            assert np.array_equal(desc.cpu().numpy(), ref)
        bad = centres.copy()
        bad[-1, 0] = (S >> lv) - 3
        with pytest.raises(ValueError, match='patch centres'):
            ops.swd_descriptors(imgs_dev, lv, bad)
    with pytest.raises(ValueError):
        ops.swd_descriptors(imgs_dev, 3, per_level[0][0])
    with pytest.raises(ValueError):
        ops.swd_descriptors(imgs_dev[:, :, :48, :48].contiguous(), 0, per_level[2][0])


# ------------------------------------------------------------------ projection
@functools.lru_cache(maxsize=None)
def proj_case(m, D):
    """descriptors with channel means 0, 5 and 127 and deviations 30, 2 and 50 (the last level has |mean| > deviation),
    unit directions, the statistics from math.fsum"""
    rng = np.random.RandomState(1000 * m + D)
    desc = (rng.randn(m, 3, 49) * np.array([30.0, 2.0, 50.0])[None, :, None]
            + np.array([0.0, 5.0, 127.0])[None, :, None]).reshape(m, 147)
    dirs = rng.randn(147, D)
    dirs = dirs / np.sqrt((dirs * dirs).sum(axis=0))
    d3 = desc.reshape(m, 3, 49)
    s1 = [math.fsum(d3[:, c].reshape(-1)) for c in range(3)]
    s2 = [math.fsum((d3[:, c].reshape(-1) - s1[c] / (m * 49.0)) ** 2) for c in range(3)]
    return desc, dirs, np.array(s1 + s2)


@pytest.mark.parametrize('D', [1, 128, 130])
@pytest.mark.parametrize('m', [1, 63, 64, 65, 200])
def test_projection_within_the_derived_bound(m, D):
    """the bound is swd_ref.projection_bound: (148 + 2) u sum_k |(d_k - mu_c) dir'_kj| for the contraction plus what the
    any-order error of the two statistics can move (derived there); ragged tiles on both axes, K padded 147 -> 148"""
    from sbagan import _lib
    desc, dirs, stats = proj_case(m, D)
    obuf, out = guarded(D * m)
    wbuf, ws = guarded(148 * D)
    a, b, c = (torch.from_numpy(v.copy()).to(DEV) for v in (desc, dirs, stats))
    rc = _lib.lib.sba_swd_project(a.data_ptr(), m, c.data_ptr(), b.data_ptr(), D, out.data_ptr(), ws.data_ptr(),
                                  8 * 148 * D, stream())
    torch.cuda.synchronize()
    assert rc == 0 and guards_intact(obuf, D * m) and guards_intact(wbuf, 148 * D)
    got = out.cpu().numpy().reshape(D, m)
    want, bound = swd_ref.project(desc, dirs), swd_ref.projection_bound(desc, dirs)
    err = np.abs(got - want)
    print('m %d, D %d: largest error %.3g, smallest bound %.3g, largest error / bound %.3g'
          % (m, D, err.max(), bound.min(), (err / bound).max()))
    assert np.isfinite(got).all() and (err <= bound).all()
    from sbagan import ops
    again = ops.swd_project(a, c, b)
    assert tuple(again.shape) == (D, m) and np.array_equal(again.cpu().numpy().view(np.int64), got.view(np.int64))


# ------------------------------------------------------------------ sort
def sort_columns_input(D, m):
    """[D][m]: column d is of kind d % 5: many duplicates, already sorted, reversed, negatives mixed with +-0, denormals"""
    rng = np.random.RandomState(D * 100003 + m)
    cols = []
    for d in range(D):
        kind = d % 5
        if kind == 0:
            v = rng.randint(0, 4, m).astype(np.float64)
        elif kind == 1:
            v = np.sort(rng.randn(m))
        elif kind == 2:
            v = np.sort(rng.randn(m))[::-1]
        elif kind == 3:
            v = -np.abs(rng.randn(m)) * rng.randint(0, 2, m)
            v[::3] = 0.0
        else:
            v = rng.randint(-5, 6, m) * 4.9e-324 * rng.randint(1, 1000, m)
        cols.append(v)
    return np.ascontiguousarray(np.stack(cols))


@pytest.mark.parametrize('D', [1, 130])
@pytest.mark.parametrize('m', [1, 2, T - 1, T, T + 1, 3 * T + 17])
def test_sorted_columns_equal_numpy_sort(m, D):
    from sbagan import _lib, ops
    assert ops.SWD_SORT_TILE == T
    x = sort_columns_input(D, m)
    dbuf, data = guarded(D * m)
    tbuf, tmp = guarded(D * m)
    data.copy_(torch.from_numpy(x).reshape(-1))
    rc = _lib.lib.sba_swd_sort_columns(data.data_ptr(), tmp.data_ptr() if m > T else None, D, m, stream())
    torch.cuda.synchronize()
    assert rc == 0 and guards_intact(dbuf, D * m) and guards_intact(tbuf, D * m)
    got = data.cpu().numpy().reshape(D, m)
    assert np.array_equal(got, np.sort(x, axis=1))              # values, not bits: -0 == +0
    # the wrapper (allocates the second buffer itself), on random values
    y = torch.from_numpy(np.random.RandomState(m).randn(D, m)).to(DEV)
    want = np.sort(y.cpu().numpy(), axis=1)
    assert ops.swd_sort_columns(y) is y and np.array_equal(y.cpu().numpy(), want)


# ------------------------------------------------------------------ the mean of |a - b|
@pytest.mark.parametrize('D', [1, 130])
@pytest.mark.parametrize('m', [1, 255, CHUNK, CHUNK + 1, 3 * CHUNK + 17])
def test_abs_mean_within_the_summation_bound(m, D):
    from sbagan import _lib, ops
    rng = np.random.RandomState(m + D)
    a, b = np.sort(rng.randn(D, m) * 3.0, axis=1), np.sort(rng.randn(D, m) + 0.5, axis=1)
    chunks = -(-m // CHUNK)
    obuf, out = guarded(D)
    wbuf, ws = guarded(D * chunks)
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    rc = _lib.lib.sba_swd_abs_mean(ta.data_ptr(), tb.data_ptr(), D, m, out.data_ptr(), ws.data_ptr(), 8 * D * chunks,
                                   stream())
    torch.cuda.synchronize()
    assert rc == 0 and guards_intact(obuf, D) and guards_intact(wbuf, D * chunks)
    got = out.cpu().numpy()
    err, bound = np.abs(got - swd_ref.abs_mean(a, b)), swd_ref.abs_mean_bound(a, b)
    print('m %d, D %d: largest error %.3g, smallest bound %.3g' % (m, D, err.max(), bound.min()))
    assert (err <= bound).all()
    assert np.array_equal(ops.swd_abs_mean(ta, tb).cpu().numpy().view(np.int64), got.view(np.int64))


# ------------------------------------------------------------------ refusals: SBA_E_ARG, nothing launched
def test_every_refusal_leaves_the_outputs_untouched():
    from sbagan import _lib
    L = _lib.lib
    S, n, P = 32, 2, 3
    imgs = torch.zeros((n, 3, S, S), dtype=torch.uint8, device=DEV)
    good = np.full((n * P, 2), 5, dtype=np.int32)
    dbuf, desc = guarded(n * P * 147)
    sbuf, stats = guarded(6)
    wbuf, ws = guarded(64)
    nbytes = 48 * n + 8 * n * P

    def d(imgs_p=imgs.data_ptr(), n_=n, S_=S, level=0, c=good, P_=P, desc_p=desc.data_ptr(), stats_p=stats.data_ptr(),
          ws_p=ws.data_ptr(), nb=nbytes):
        return L.sba_swd_descriptors(imgs_p, n_, S_, level, c.ctypes.data if c is not None else None, P_, desc_p, stats_p,
                                     ws_p, nb, stream())
    for S_ in (16, 48, 512, 0):
        assert d(S_=S_) == E_ARG
    for level in (-1, 2, 5):                                    # a 32 px image has levels 0 and 1
        assert d(level=level) == E_ARG
    assert d(n_=0) == E_ARG and d(P_=0) == E_ARG and d(P_=4097) == E_ARG and d(n_=1 << 31) == E_ARG
    assert d(imgs_p=None) == E_ARG and d(c=None) == E_ARG and d(desc_p=None) == E_ARG
    assert d(stats_p=None) == E_ARG and d(ws_p=None) == E_ARG
    assert d(desc_p=desc.data_ptr() + 4) == E_ARG and d(stats_p=stats.data_ptr() + 4) == E_ARG
    assert d(ws_p=ws.data_ptr() + 4) == E_ARG and d(nb=nbytes - 1) == E_ARG
    for level, lo_hi in ((0, (2, 29)), (1, (2, 13))):
        for v in lo_hi:
            for pos in ((0, 0), (n * P - 1, 1)):
                bad = good.copy()
                bad[pos] = v
                assert d(level=level, c=bad) == E_ARG, (level, v, pos)
    ok = good.copy()
    ok[0], ok[-1] = (3, 28), (28, 3)
    assert d(c=ok) == 0                                         # (the extremes themselves are fine)
    torch.cuda.synchronize()
    desc.fill_(SENTINEL)
    stats.fill_(SENTINEL)

    m, D = 5, 3
    x = torch.zeros(m * 147 + D * 147 + 6, dtype=torch.float64, device=DEV)
    obuf, out = guarded(D * m)

    def p(desc_p=x.data_ptr(), m_=m, stats_p=x.data_ptr(), dirs_p=x.data_ptr(), D_=D, out_p=out.data_ptr(),
          ws_p=ws.data_ptr(), nb=8 * 148 * D):
        return L.sba_swd_project(desc_p, m_, stats_p, dirs_p, D_, out_p, ws_p, nb, stream())
    assert p(m_=0) == E_ARG and p(D_=0) == E_ARG and p(D_=65536, nb=1 << 40) == E_ARG and p(m_=1 << 41) == E_ARG
    assert p(desc_p=None) == E_ARG and p(stats_p=None) == E_ARG and p(dirs_p=None) == E_ARG and p(out_p=None) == E_ARG
    assert p(ws_p=None) == E_ARG and p(out_p=out.data_ptr() + 4) == E_ARG and p(nb=8 * 148 * D - 1) == E_ARG

    def s(data_p=out.data_ptr(), tmp_p=None, D_=D, m_=m):
        return L.sba_swd_sort_columns(data_p, tmp_p, D_, m_, stream())
    assert s(data_p=None) == E_ARG and s(D_=0) == E_ARG and s(m_=0) == E_ARG and s(D_=65536) == E_ARG
    assert s(data_p=out.data_ptr() + 4) == E_ARG
    assert s(m_=T + 1) == E_ARG and s(m_=T + 1, tmp_p=out.data_ptr()) == E_ARG     # no second buffer / the same one

    def a(a_p=x.data_ptr(), b_p=x.data_ptr(), D_=D, m_=m, out_p=out.data_ptr(), ws_p=ws.data_ptr(), nb=8 * D):
        return L.sba_swd_abs_mean(a_p, b_p, D_, m_, out_p, ws_p, nb, stream())
    assert a(a_p=None) == E_ARG and a(b_p=None) == E_ARG and a(out_p=None) == E_ARG and a(ws_p=None) == E_ARG
    assert a(D_=0) == E_ARG and a(m_=0) == E_ARG and a(nb=8 * D - 1) == E_ARG and a(b_p=x.data_ptr() + 4) == E_ARG
    torch.cuda.synchronize()
    for buf, k in ((dbuf, n * P * 147), (sbuf, 6), (obuf, D * m)):
        assert (buf.cpu().numpy() == SENTINEL).all(), k


# ------------------------------------------------------------------ the evaluator, end to end
@functools.lru_cache(maxsize=None)
def end_to_end_case(S, n):
    real, fake = swd_ref.make_images(S, n, seed=1), swd_ref.make_images(S, n, seed=2)
    ref, _, diff, bound = swd_ref.end_to_end_bound(real, fake, swd_ref.draws(100, S, n))
    return real, fake, ref, diff, bound


def fed(ev, real, fake, batch=2):
    for side, stack in (('real', real), ('fake', fake)):
        for at in range(0, len(stack), batch):
            ev.update(side, as_float(stack[at:at + batch]))
    return ev


@pytest.mark.parametrize('S,n', [(64, 6), (256, 2)])
def test_result_against_the_reference_within_the_measured_bound(S, n):
    """The bound is 16 x the largest per-level difference between the float64 and the extended-precision evaluation of
    the reference at this shape (DESIGN.md 7k gives the figures measured on one MI355X)."""
    from sbagan.swd import FIELDS, SWD
    real, fake, ref, diff, bound = end_to_end_case(S, n)
    ev = fed(SWD(16384, size=S, capacity=1), real, fake)
    assert ev.count('real') == ev.count('fake') == n
    assert np.array_equal(ev.images('real').cpu().numpy(), real) and np.array_equal(ev.images('fake').cpu().numpy(), fake)
    res = ev.result()
    got = np.array(res['swd_x1e3'])
    err = np.abs(got - ref * 1e3)
    print('%d px, %d images: SWD x 1e3 %s; f64 against extended precision %.3g, bound %.3g, error %s (all x 1e3)'
          % (S, n, got, diff * 1e3, bound * 1e3, err))
    assert sorted(res) == sorted(FIELDS) and json.loads(json.dumps(res)) == res
    assert res['resolutions'] == [S >> lv for lv in range(len(ref))] and res['levels'] == len(ref) == len(got)
    assert (res['n_images'], res['patches_per_image'], res['dir_repeats'], res['dirs_per_repeat']) == (n, 128, 4, 128)
    assert (res['size'], res['seed']) == (S, 100) and res['swd_avg_x1e3'] == float(np.mean(got))
    assert (err <= bound * 1e3).all()
    assert ev.result() == res                                   # bit-identical, and the draws start from the seed
    assert fed(SWD(n, S, seed=101), real, fake).result() != res       # other draws, another figure


def test_shared_store_cap_and_zero_deviation():
    from sbagan.msssim import MSSSIM
    from sbagan.swd import SWD
    S, n = 256, 2
    real, fake, _, _, _ = end_to_end_case(S, n)
    own = fed(SWD(n, size=S), real, fake).result()
    ms = MSSSIM(2, size=S)
    for side, stack in (('real', real), ('fake', fake)):
        ms.update(side, as_float(stack), [1, 1])
    shared = SWD(n, size=S, images=ms)
    shared.update('fake', as_float(fake))                       # stores nothing
    assert shared._held == {} and shared.count('real') == n
    assert shared.images('fake').data_ptr() == ms.images('fake').data_ptr()
    assert shared.result() == own
    # the cap: the first max_images count, later ones are not stored
    more_real, more_fake = np.concatenate([real, fake[:1]]), np.concatenate([fake, real[:1]])
    capped = fed(SWD(n, size=S, capacity=1), more_real, more_fake)
    assert capped.count('real') == n and capped._held['real'][0].shape[0] == n and capped.result() == own
    assert SWD(1, size=S, images=ms).count('fake') == 1
    # a side without any variation cannot be normalised: named by side, level and channel
    flat = fed(SWD(n, size=S), real, np.zeros_like(fake))
    with pytest.raises(RuntimeError, match=r'the fake side has zero deviation at level 0 \(256 px\), channel 0'):
        flat.result()
    lone = SWD(4, size=S)
    lone.update('real', as_float(real))
    with pytest.raises(RuntimeError, match='2 real, 0 generated'):
        lone.result()


# ------------------------------------------------------------------ the flag through the entry points
def _toy_yml(tmp_path, root, net_g, base_size=64):
    import yaml
    yml = tmp_path / ('toy_%s.yml' % os.path.basename(os.path.dirname(net_g)))
    yml.write_text(yaml.safe_dump({
        'CONFIG_NAME': 'toy', 'DATASET_NAME': 'toy', 'DATA_DIR': root, 'GPU_ID': 0, 'WORKERS': 0,
        'B_VALIDATION': True, 'TREE': {'BRANCH_NUM': 2, 'BASE_SIZE': base_size},
        'TRAIN': {'FLAG': False, 'NET_G': net_g, 'NET_E': '', 'BATCH_SIZE': 2},
        'GAN': {'DF_DIM': 64, 'GF_DIM': 32, 'Z_DIM': 100, 'R_NUM': 2},
        'TEXT': {'EMBEDDING_DIM': 256, 'CAPTIONS_PER_IMAGE': 2, 'WORDS_NUM': 8}}))
    return str(yml)


def _files(root_dir):
    return {os.path.relpath(f, root_dir): open(f, 'rb').read()
            for f in glob.glob(os.path.join(root_dir, '**', '*'), recursive=True) if os.path.isfile(f)}


def test_main_with_and_without_the_flag(tmp_path, capsys):
    """main.main() sampling on a toy data set at 128 px (4 levels): --swd 8 writes swd.json and prints the line; the run
    without the flag writes the same PNG bytes and leaves the generators where the flagged run leaves them"""
    from test_host_cpu import _make_dataset
    from miscc.config import reset_cfg
    import main
    import model
    from miscc.utils import weights_init
    from sbagan import ops
    from trainer import condGANTrainer
    root = str(tmp_path / 'toy')
    _make_dataset(root, n_test=4)
    reset_cfg()
    from miscc.config import cfg
    cfg.GAN.GF_DIM, cfg.GAN.DF_DIM, cfg.TREE.BRANCH_NUM = 32, 64, 2
    torch.manual_seed(1)
    net = model.G_NET()
    net.apply(weights_init)
    sd = net.state_dict()
    seen = []

    def make_trainer(out, loader, n_words, ixtoword):
        seen.append(condGANTrainer(out, loader, n_words, ixtoword, allow_random_encoders=True))
        return seen[-1]
    runs = {}
    ops.set_deterministic(True, DEV)        # (the generator's default mode adds with f32 atomics: a few bytes differ)
    try:
        for flag in (True, False):
            ck = str(tmp_path / ('swd%d' % flag) / 'netG_epoch_1.pth')
            os.makedirs(os.path.dirname(ck))
            torch.save(sd, ck)
            reset_cfg()
            ops.set_compute_dtype(torch.bfloat16)
            capsys.readouterr()
            main.main(['--cfg', _toy_yml(tmp_path, root, ck), '--gpu', '0'] + (['--swd', '8'] if flag else []),
                      make_trainer=make_trainer)
            states = (np.random.get_state(), torch.cuda.get_rng_state(), torch.get_rng_state())
            runs[flag] = (seen[-1], _files(ck[:-4]), states, capsys.readouterr().out)
    finally:
        ops.set_deterministic(False)
        reset_cfg()
    (algo1, files1, states1, out1), (algo0, files0, states0, out0) = runs[True], runs[False]
    assert algo1.swd == 8 and algo0.swd == 0 and algo0.swd_result is None and algo0.swd_evaluator is None
    pngs0 = {k: v for k, v in files0.items() if k.endswith('.png')}
    assert len(pngs0) == 4 and pngs0 == files0
    swd_name = [k for k in files1 if k.endswith('swd.json')]
    assert len(swd_name) == 1 and {k: v for k, v in files1.items() if k != swd_name[0]} == files0
    assert sh.same_states(states1, states0)
    res = json.loads(files1[swd_name[0]].decode())
    print(out1)
    assert res == algo1.swd_result and res['levels'] == 4 == len(res['swd_x1e3']) and res['n_images'] == 4
    assert res['resolutions'] == [128, 64, 32, 16] and all(math.isfinite(v) and v > 0.0 for v in res['swd_x1e3'])
    line = [ln for ln in out1.splitlines() if ln.startswith('SWD x 1e3')]
    assert len(line) == 1 and '128 px' in line[0] and '16 px' in line[0] and 'average' in line[0]
    assert 'SWD' not in out0
    # the stored generated images are the pixels of the PNG files, and the figure is the reference's on them
    from PIL import Image
    ev = algo1.swd_evaluator
    fake, real = ev.images('fake').cpu().numpy(), ev.images('real').cpu().numpy()
    decoded = sorted(np.asarray(Image.open(io.BytesIO(v))).transpose(2, 0, 1).tobytes() for v in pngs0.values())
    assert sorted(im.tobytes() for im in fake) == decoded
    ref = swd_ref.swd(real, fake, swd_ref.draws(100, 128, 4)) * 1e3
    assert np.allclose(res['swd_x1e3'], ref, rtol=0, atol=1e-9)


def test_a_size_outside_the_set_is_refused_before_any_file_exists(tmp_path):
    from test_host_cpu import _make_dataset
    from miscc.config import reset_cfg
    import main
    from trainer import condGANTrainer
    root = str(tmp_path / 'toy')
    _make_dataset(root, n_test=2)
    ck = str(tmp_path / 'odd' / 'netG_epoch_1.pth')
    os.makedirs(os.path.dirname(ck))
    open(ck, 'wb').close()                  # (never read: the refusal comes first)

    def make_trainer(out, loader, n_words, ixtoword):
        return condGANTrainer(out, loader, n_words, ixtoword, allow_random_encoders=True)
    try:
        with pytest.raises(ValueError, match='side in'):
            main.main(['--cfg', _toy_yml(tmp_path, root, ck, base_size=48), '--gpu', '0', '--swd', '8'],
                      make_trainer=make_trainer)
    finally:
        reset_cfg()
    left = [os.path.join(d, f) for d, _, fs in os.walk(os.path.dirname(ck)) for f in fs]
    assert left == [ck] and not os.path.exists(ck[:-4])


def test_pretrain_damsm_parses_the_flag_and_ignores_it(tmp_path, monkeypatch):
    import yaml
    from test_host_cpu import _make_dataset
    from miscc.config import reset_cfg
    reset_cfg()
    root = str(tmp_path / 'toy')
    _make_dataset(root, n_train=4, n_test=4)
    yml = tmp_path / 'damsm_toy.yml'
    yml.write_text(yaml.safe_dump({
        'CONFIG_NAME': 'DAMSM', 'DATASET_NAME': 'toy', 'DATA_DIR': root, 'GPU_ID': 0, 'WORKERS': 0,
        'TREE': {'BRANCH_NUM': 1, 'BASE_SIZE': 128},
        'TRAIN': {'FLAG': True, 'NET_E': '', 'BATCH_SIZE': 4, 'MAX_EPOCH': 1, 'SNAPSHOT_INTERVAL': 1,
                  'ENCODER_LR': 0.002, 'RNN_GRAD_CLIP': 0.25,
                  'SMOOTH': {'GAMMA1': 4.0, 'GAMMA2': 5.0, 'GAMMA3': 10.0}},
        'TEXT': {'EMBEDDING_DIM': 256, 'CAPTIONS_PER_IMAGE': 2, 'WORDS_NUM': 8}}))
    monkeypatch.chdir(tmp_path / 'toy')
    import pretrain_DAMSM
    from sbagan import ops
    ops.set_compute_dtype(torch.bfloat16)
    try:
        model_dir = pretrain_DAMSM.main(['--cfg', str(yml), '--gpu', '0', '--manualSeed', '7', '--swd', '8'], max_steps=1)
        assert os.path.isfile(os.path.join(model_dir, 'text_encoder0.pth'))
        assert not glob.glob(os.path.join(os.path.dirname(model_dir), '**', 'swd.json'), recursive=True)
    finally:
        reset_cfg()
        ops.set_compute_dtype(torch.float32)
