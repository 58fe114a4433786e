"""MS-SSIM evaluation on the GPU: the float64 kernel through the raw C ABI and through ops.msssim_pairs against the numpy
reference (tests/msssim_ref.py) -- every per-scale mean within 1e-10, the combined values within 1e-8 -- guard bytes,
reproducibility, image numbers out of range, the refusals, the MSSSIM class with hand-fed batches, and sampling() with
ms_ssim on through both trainers at 256 px (and refused at 128 px)."""
import functools
import io
import json
import os

import numpy as np
import pytest
import torch

import msssim_ref
import sampling_harness as sh

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
E_ARG = -1
SENTINEL = -7.0
GUARD = 64                          # f64 elements on either side of `out` and of the workspace

# (H, W, scales, P): one window position; ragged tile edges, H != W; an odd column dropped, pooled to 11 x 11; odd at two
# levels; the floor (last scale 1 x 1 positions); odd and non-square; the workload's size
CASES = [(11, 11, 1, 1), (12, 27, 1, 3), (22, 23, 2, 2), (45, 47, 3, 2), (176, 176, 5, 2), (177, 208, 5, 3),
         (256, 256, 5, 4)]
# which pairs of msssim_ref.kind_stack a case takes: 0 noise, 1 smooth, 2 noisy copy, 3 flat 255 / 254, 4 identical,
# 5 inverted 0 / 255, 6 a pair (i, i), 7 images of two other pairs.  Together the cases cover every kind.
TAKES = {(11, 11): (0,), (12, 27): (1, 2, 3), (22, 23): (4, 5), (45, 47): (6, 7), (176, 176): (0, 5), (177, 208): (3, 7, 1),
         (256, 256): (0, 2, 6, 4)}
FIVE = [c for c in CASES if c[2] == 5]


def dev(x):
    return torch.tensor(np.asarray(x), device=DEV)


def host(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(H, W, S, P):
    """(imgs uint8 [12][3][H][W], pairs int32 [P][2], reference means [P][3][S][2]), computed once, read-only"""
    imgs, pairs = msssim_ref.kind_stack(H, W, seed=H)
    pairs = np.ascontiguousarray(pairs[list(TAKES[(H, W)])])
    assert len(pairs) == P
    ref = msssim_ref.pair_means(imgs, pairs, S)
    for v in (imgs, pairs, ref):
        v.setflags(write=False)
    return imgs, pairs, ref


def raw_pairs(imgs, pairs, S):
    """the C entry point itself, `out` and the workspace between guard elements: (return code, out [P][3][S][2] on the
    host); asserts that the guards are untouched"""
    from sbagan import _lib
    n, _, H, W = imgs.shape
    P = pairs.shape[0]
    nbytes = _lib.lib.sba_msssim_workspace_bytes(H, W, P, S)
    assert nbytes > 0 and nbytes % 16 == 0
    n_out, n_ws = P * 3 * S * 2, nbytes // 8
    out = torch.full((n_out + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=DEV)
    ws = torch.full((n_ws + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=DEV)
    rc = _lib.lib.sba_msssim_pairs(imgs.data_ptr(), n, H, W, pairs.data_ptr(), P, S, out[GUARD:].data_ptr(),
                                   ws[GUARD:].data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    out, ws = host(out), host(ws)
    for buf, m in ((out, n_out), (ws, n_ws)):
        assert (buf[:GUARD] == SENTINEL).all() and (buf[GUARD + m:] == SENTINEL).all()
    return rc, out[GUARD:GUARD + n_out].reshape(P, 3, S, 2)


def ops_pairs(imgs, pairs, S):
    from sbagan import ops
    out = ops.msssim_pairs(imgs, pairs, S)
    assert out.dtype == torch.float64 and tuple(out.shape) == (len(pairs), 3, S, 2) and out.device == imgs.device
    return host(out)


# ------------------------------------------------------------------ the per-scale means and the final values
@pytest.mark.parametrize('H,W,S,P', CASES)
def test_per_scale_means_within_1e_10_of_the_reference(H, W, S, P):
    """Largest error seen on one MI355X over all cases: 3.7e-13, on the flat 255 / 254 pair."""
    imgs, pairs, ref = case(H, W, S, P)
    rc, got = raw_pairs(dev(imgs), dev(pairs), S)
    assert rc == 0 and np.isfinite(got).all()
    err = np.abs(got - ref)
    print('%d x %d, %d scales, %d pairs: largest error %.3g (ssim %.3g, cs %.3g)'
          % (H, W, S, P, err.max(), err[..., 0].max(), err[..., 1].max()))
    assert (err <= 1e-10).all()
    # the wrapper makes the same launch: host pairs (int32 and int64) and device pairs
    for p in (pairs, pairs.astype(np.int64), torch.from_numpy(pairs.copy()), dev(pairs)):
        assert np.array_equal(ops_pairs(dev(imgs), p, S).view(np.int64), got.view(np.int64))


@pytest.mark.parametrize('H,W,S,P', FIVE)
def test_final_values_within_1e_8_of_the_reference(H, W, S, P):
    """v^0.0448 is steep at 0, so the bound is for inputs whose factors are 0 or at least 1e-3; here no factor of the
    reference lies within 1e-3 of 0 on EITHER side, so a clipped one is clipped in both"""
    from sbagan.msssim import combine
    imgs, pairs, ref = case(H, W, S, P)
    raw = np.concatenate([ref[:, :, :S - 1, 1], ref[:, :, S - 1:, 0]], axis=2)
    v = msssim_ref.factors(ref)
    assert np.abs(raw).min() >= 1e-3 and ((v == 0.0) | (v >= 1e-3)).all()
    got, want = combine(ops_pairs(dev(imgs), pairs, S)), msssim_ref.combine(ref)
    print('%d x %d: ms-ssim %s, reference %s, largest error %.3g' % (H, W, got, want, np.abs(got - want).max()))
    assert got.shape == (P,) and (np.abs(got - want) <= 1e-8).all()


def test_two_launches_are_bit_identical():
    H, W, S, P = CASES[5]
    imgs, pairs, _ = case(H, W, S, P)
    a, p = dev(imgs), dev(pairs)
    rc0, first = raw_pairs(a, p, S)
    rc1, again = raw_pairs(a, p, S)
    assert rc0 == 0 and rc1 == 0 and np.array_equal(first.view(np.int64), again.view(np.int64))
    assert np.array_equal(ops_pairs(a, pairs, S).view(np.int64), ops_pairs(a, pairs, S).view(np.int64))


def test_image_numbers_out_of_range_give_nan_for_that_pair_alone():
    """the 12 images lie in the middle of a buffer; pairs that name -1, n, n + 5 and the int32 extremes read nothing and
    give NaN, and their neighbours are bit for bit what they are in a launch of their own"""
    H, W, S = 45, 47, 3
    imgs, _, _ = case(*CASES[3])
    n = len(imgs)
    big = torch.zeros((n + 8, 3, H, W), dtype=torch.uint8, device=DEV)
    big[4:4 + n] = dev(imgs)
    a = big[4:4 + n]
    good = np.array([(0, 1), (2, 3), (11, 10), (5, 5)], dtype=np.int32)
    lim = np.iinfo(np.int32)
    mixed = np.array([(0, 1), (-1, 1), (2, 3), (2, n), (n + 5, 0), (11, 10), (lim.max, 3), (3, lim.min), (5, 5), (-1, -1)],
                     dtype=np.int32)
    ok = np.array([0, 2, 5, 8])
    rc, want = raw_pairs(a, dev(good), S)
    assert rc == 0 and np.isfinite(want).all()
    assert (np.abs(want - msssim_ref.pair_means(imgs, good, S)) <= 1e-10).all()
    rc, got = raw_pairs(a, dev(mixed), S)
    assert rc == 0
    bad = np.setdiff1d(np.arange(len(mixed)), ok)
    assert np.isnan(got[bad]).all() and np.array_equal(got[ok].view(np.int64), want.view(np.int64))
    # the wrapper passes such pairs on (int64 numbers beyond int32 included) and gives the same NaNs
    wide = mixed.astype(np.int64)
    wide[3, 1], wide[4, 0] = 1 << 40, -(1 << 35)
    via = ops_pairs(a, wide, S)
    assert np.isnan(via[bad]).all() and np.array_equal(via[ok].view(np.int64), want.view(np.int64))


# ------------------------------------------------------------------ refusals, all before any launch
def test_wrapper_refusals():
    from sbagan import ops
    imgs = torch.zeros(4, 3, 22, 23, dtype=torch.uint8, device=DEV)
    pairs = np.array([(0, 1)], dtype=np.int32)
    assert tuple(ops.msssim_pairs(imgs, pairs, 2).shape) == (1, 3, 2, 2)
    with pytest.raises(RuntimeError):
        ops.msssim_pairs(imgs.cpu(), pairs, 2)                              # a CPU tensor
    with pytest.raises(TypeError):
        ops.msssim_pairs(imgs.float(), pairs, 2)                            # wrong dtype
    with pytest.raises(TypeError):
        ops.msssim_pairs(imgs.to(torch.int8), pairs, 2)
    with pytest.raises(TypeError):
        ops.msssim_pairs(host(imgs), pairs, 2)                              # not a tensor
    with pytest.raises(ValueError):
        ops.msssim_pairs(imgs[0], pairs, 2)                                 # wrong rank
    with pytest.raises(ValueError):
        ops.msssim_pairs(imgs[None], pairs, 2)
    with pytest.raises(ValueError):
        ops.msssim_pairs(torch.zeros(4, 1, 22, 23, dtype=torch.uint8, device=DEV), pairs, 2)      # one channel
    with pytest.raises(ValueError):
        ops.msssim_pairs(torch.zeros(0, 3, 22, 23, dtype=torch.uint8, device=DEV), pairs, 2)      # no image
    with pytest.raises(ValueError):
        ops.msssim_pairs(torch.zeros(4, 3, 22, 46, dtype=torch.uint8, device=DEV)[:, :, :, ::2], pairs, 2)   # strided
    with pytest.raises(ValueError):
        ops.msssim_pairs(torch.zeros(4, 22, 23, 3, dtype=torch.uint8, device=DEV).permute(0, 3, 1, 2), pairs, 2)   # HWC
    for scales in (0, 6, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            ops.msssim_pairs(imgs, pairs, scales)
    with pytest.raises(ValueError):
        ops.msssim_pairs(imgs, pairs, 3)                                    # 22 >> 2 = 5 < 11
    with pytest.raises(ValueError):
        ops.msssim_pairs(torch.zeros(1, 3, 1025, 16, dtype=torch.uint8, device=DEV), pairs, 1)    # above 1024
    with pytest.raises(ValueError):
        ops.msssim_pairs(imgs, np.zeros((0, 2), dtype=np.int32), 2)         # no pair
    with pytest.raises(ValueError):
        ops.msssim_pairs(imgs, np.zeros((2,), dtype=np.int32), 2)           # pairs of the wrong rank
    with pytest.raises(ValueError):
        ops.msssim_pairs(imgs, np.zeros((2, 3), dtype=np.int32), 2)
    with pytest.raises(TypeError):
        ops.msssim_pairs(imgs, np.zeros((1, 2), dtype=np.float32), 2)
    with pytest.raises(TypeError):
        ops.msssim_pairs(imgs, torch.zeros(1, 2, dtype=torch.int64, device=DEV), 2)     # device pairs are int32
    with pytest.raises(ValueError):
        ops.msssim_pairs(imgs, torch.zeros(2, 4, dtype=torch.int32, device=DEV)[:, ::2], 2)             # strided


def test_c_abi_refusals():
    from sbagan import _lib
    fn, size = _lib.lib.sba_msssim_pairs, _lib.lib.sba_msssim_workspace_bytes
    H0, W0 = 45, 47
    imgs = torch.zeros(4 * 3 * 1024 * 64, dtype=torch.uint8, device=DEV)       # room for every shape tried below
    pairs = torch.zeros(2 * 8, dtype=torch.int32, device=DEV)
    out = torch.full((1024,), SENTINEL, dtype=torch.float64, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.float64, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    X, I, O, Wp, full = imgs.data_ptr(), pairs.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel() * 8
    need = size(H0, W0, 2, 3)
    assert need == 2 * 3 * (3 * 2 + 1 + 1) * 16 <= full

    def call(x=X, n=4, H=H0, W=W0, p=I, P=2, S=3, o=O, w=Wp, wbytes=full):
        return fn(x, n, H, W, p, P, S, o, w, wbytes, st)
    bad = [dict(x=None), dict(p=None), dict(o=None), dict(w=None),
           dict(p=I + 2), dict(p=I + 1), dict(o=O + 4), dict(w=Wp + 4),           # misaligned
           dict(S=4), dict(H=43), dict(W=43), dict(H=10, S=1), dict(W=10, S=1),   # min(H, W) >> (S - 1) < 11
           dict(S=0), dict(S=6), dict(S=-1),
           dict(H=1025, W=16, S=1), dict(H=16, W=1025, S=1), dict(H=0), dict(W=-5),
           dict(P=0), dict(P=-1), dict(P=(1 << 20) + 1), dict(n=0), dict(n=-2),
           dict(wbytes=need - 1), dict(wbytes=0), dict(wbytes=-8)]
    for kw in bad:
        assert call(**kw) == E_ARG, kw
    torch.cuda.synchronize()
    assert (host(out) == SENTINEL).all() and (host(ws) == 0).all()
    assert call() == 0 and call(wbytes=need) == 0 and call(x=X + 1) == 0         # the bytes need no alignment
    assert call(H=1024, W=16, S=1, P=1) == 0 and call(H=11, W=1024, S=1, P=1) == 0
    torch.cuda.synchronize()
    assert (host(out)[:2 * 3 * 3 * 2] != SENTINEL).all() and (host(out)[2 * 3 * 3 * 2:] == SENTINEL).all()


# ------------------------------------------------------------------ the MSSSIM class with hand-fed batches
def as_float(u8):
    """float images in [-1, 1] whose quantisation is `u8`: the middle of each byte's interval"""
    return (torch.as_tensor(u8).to(DEV).float() + 0.5) / 127.5 - 1.0


def reference_result(fake, real, ids, per_class, seed=100):
    """the result fields that depend on the pixels, from the reference on the stored uint8 images"""
    from sbagan.msssim import draw_pairs
    pairs = draw_pairs(ids, per_class, seed)
    f = msssim_ref.combine(msssim_ref.pair_means(fake, pairs, 5))
    r = msssim_ref.combine(msssim_ref.pair_means(real, pairs, 5))
    return {'ms_ssim_fake': f.mean(), 'ms_ssim_real': r.mean(), 'ms_ssim_fake_std': f.std(), 'ms_ssim_real_std': r.std(),
            'pairs': len(pairs)}


def check_against_reference(res, fake, real, ids, per_class):
    want = reference_result(fake, real, ids, per_class)
    assert res['pairs'] == want['pairs']
    for key in ('ms_ssim_fake', 'ms_ssim_real', 'ms_ssim_fake_std', 'ms_ssim_real_std'):
        print('%s %.12g (reference %.12g)' % (key, res[key], want[key]))
        assert np.isfinite(res[key]) and abs(res[key] - want[key]) <= 1e-8, key
    return want


def test_class_with_hand_fed_batches():
    from sbagan.msssim import FIELDS, MSSSIM
    imgs, _ = msssim_ref.kind_stack(176, 176, seed=176)
    fake, real = imgs[:8], imgs[4:12]
    ids = [5, 5, 2, 2, 5, 9, 2, 5]                  # class 5: 4 images, 6 pairs; class 2: 3 pairs; class 9 is skipped
    ev = MSSSIM(2, size=176, seed=100, capacity=2)  # batches of 3, 1, 4 images: the buffer doubles twice
    for side, stack in (('fake', fake), ('real', real)):
        at = 0
        for B in (3, 1, 4):
            ev.update(side, as_float(stack[at:at + B]), np.asarray(ids[at:at + B]))
            at += B
            assert ev.count(side) == at and np.array_equal(host(ev.images(side)), stack[:at])
        assert ev.images(side).dtype == torch.uint8 and ev.images(side).is_contiguous()
        assert ev._held[side][0].shape[0] == 8 and ev.class_ids(side).tolist() == ids
    res = ev.result()
    print(res)
    assert sorted(res) == sorted(FIELDS) and json.loads(json.dumps(res)) == res
    assert (res['pairs'], res['pairs_per_class'], res['classes'], res['classes_skipped']) == (4, 2, 2, 1)
    assert (res['n_images'], res['size'], res['scales'], res['seed']) == (8, 176, 5, 100)
    check_against_reference(res, fake, real, ids, 2)
    assert res['ms_ssim_fake'] != res['ms_ssim_real'] and res['ms_ssim_fake_std'] > 0.0
    assert ev.result() == res                       # the draws start from the seed every time

    # bf16 images (the compute dtype of a run) are quantised like the f32 ones they widen to
    half = MSSSIM(2, size=176, capacity=1)
    x = as_float(fake[:2]).to(torch.bfloat16)
    half.update('fake', x, [1, 1])
    from trainer import _to_uint8
    assert np.array_equal(host(half.images('fake'))[1].transpose(1, 2, 0), _to_uint8(x[1]))

    # the two sides must hold the same class-id sequence
    for other in ([5, 5, 2, 2, 5, 9, 2, 2], [5, 5, 2, 2, 5, 9, 2]):
        odd = MSSSIM(2, size=176)
        odd.update('fake', as_float(fake), ids)
        odd.update('real', as_float(real[:len(other)]), other)
        with pytest.raises(RuntimeError, match='same images in the same order: %d real, 8 generated' % len(other)):
            odd.result()
    # no class of two images: the counts are named
    lone = MSSSIM(2, size=176)
    for side in ('fake', 'real'):
        lone.update(side, as_float(fake[:3]), [4, 6, 5])
    with pytest.raises(RuntimeError, match=r'no class holds two images \(3 images, 3 classes\)'):
        lone.result()
    with pytest.raises(ValueError):
        ev.update('fake', as_float(fake[:2]), [1, 2, 3])                    # ids do not match the batch
    with pytest.raises(TypeError):
        ev.update('fake', dev(fake[:2]), [1, 2])                            # uint8: the class takes the float images
    with pytest.raises(ValueError):
        ev.update('both', as_float(fake[:2]), [1, 2])
    with pytest.raises(ValueError):
        ev.update('fake', as_float(fake[:2])[:, :, :, :100], [1, 2])


# ------------------------------------------------------------------ sampling() with the flag
CLASSES = [1, 1, 1, 2, 2, 3]        # of the 6 test images: 3 + 1 pairs, 2 drawn of the first class; class 3 is skipped
PER_CLASS = 2
SIZE = 256
OTHERS = dict(fid=True, r_precision=4, prdc=3, kid=True, kid_subsets=4, kid_subset_size=5)  # every other evaluator on


def _setup_256(tmp_path, names, bert=False):
    """the toy setup at 256 px (BRANCH_NUM 3) on a data dir of its own whose 6 test images have CLASSES"""
    return sh.setup(tmp_path, names, size=SIZE, bert=bert, classes=CLASSES)


def _decoded(files):
    """the PNG files of a run as a sorted list of CHW uint8 byte strings"""
    from PIL import Image
    return sorted(np.asarray(Image.open(io.BytesIO(v))).transpose(2, 0, 1).tobytes()
                  for k, v in files.items() if k.endswith('.png'))


def _check_result(algo, files):
    from sbagan.msssim import FIELDS
    res = json.loads(files['ms_ssim.json'].decode())
    print('ms_ssim.json:', res)
    assert res == algo.ms_ssim_result and sorted(res) == sorted(FIELDS)
    assert (res['pairs'], res['pairs_per_class'], res['classes'], res['classes_skipped']) == (3, PER_CLASS, 2, 1)
    assert (res['n_images'], res['size'], res['scales'], res['seed']) == (6, SIZE, 5, 100)
    ev = algo.ms_ssim_evaluator
    fake, real = host(ev.images('fake')), host(ev.images('real'))
    assert fake.shape == real.shape == (6, 3, SIZE, SIZE) and fake.dtype == np.uint8
    ids = ev.class_ids('fake')
    assert sorted(ids.tolist()) == CLASSES and np.array_equal(ids, ev.class_ids('real'))
    # the stored generated images are the pixels of the PNG files the run wrote
    assert sorted(im.tobytes() for im in fake) == _decoded(files)
    check_against_reference(res, fake, real, ids, PER_CLASS)
    assert 0.0 <= res['ms_ssim_fake'] <= 1.0 and 0.0 <= res['ms_ssim_real'] <= 1.0
    return res


def test_sampling_without_and_with_the_flag(tmp_path):
    from miscc.config import reset_cfg
    make, loader, ds, ckpts = _setup_256(tmp_path, ('without', 'with'))
    algo0, files0, states0, calls0 = sh.sample(make, loader, ds, ckpts[0])
    algo1, files1, states1, calls1 = sh.sample(make, loader, ds, ckpts[1], ms_ssim=PER_CLASS)
    assert algo0.ms_ssim_result is None and algo0.ms_ssim_evaluator is None
    assert calls0 == 0 and len(files0) == 6 and all(k.endswith('.png') for k in files0)
    # the same image files, byte for byte, and ms_ssim.json beside them
    assert sorted(files1) == sorted(list(files0) + ['ms_ssim.json']) and sh.images(files1) == files0
    # the flag consumes none of the randomness the data path and the noise draw from
    assert sh.same_states(states1, states0)
    assert calls1 == 0                              # no image encoder: the figure is on the pixels
    _check_result(algo1, files1)
    reset_cfg()


def test_sampling_with_every_other_evaluator_leaves_their_results_unchanged(tmp_path):
    from miscc.config import reset_cfg
    make, loader, ds, ckpts = _setup_256(tmp_path, ('four', 'five'))
    algo0, files0, states0, calls0 = sh.sample(make, loader, ds, ckpts[0], **OTHERS)
    algo1, files1, states1, calls1 = sh.sample(make, loader, ds, ckpts[1], ms_ssim=PER_CLASS, **OTHERS)
    assert calls0 == calls1 == 3 + 3
    assert sorted(files1) == sorted(list(files0) + ['ms_ssim.json']) and sh.images(files1) == sh.images(files0)
    for name in ('fid.json', 'prdc.json', 'kid.json', 'r_precision.json'):
        assert json.loads(files1[name].decode()) == json.loads(files0[name].decode()), name
    assert sh.same_states(states1, states0)
    _check_result(algo1, files1)
    reset_cfg()


def test_sampling_with_ms_ssim_through_the_bert_trainer(tmp_path):
    from miscc.config import reset_cfg
    make, loader, ds, ckpts = _setup_256(tmp_path, ('out',), bert=True)
    algo, files, _, calls = sh.sample(make, loader, ds, ckpts[0], ms_ssim=PER_CLASS)
    assert len(files) == 7 and calls == 0
    _check_result(algo, files)
    reset_cfg()


def test_a_128_px_configuration_is_refused_before_any_file_exists(tmp_path):
    from miscc.config import reset_cfg
    make, loader, ds, ckpts = sh.setup(tmp_path, ('small',))
    with pytest.raises(ValueError, match='176'):
        sh.sample(make, loader, ds, ckpts[0], ms_ssim=PER_CLASS)
    left = [os.path.join(d, f) for d, _, fs in os.walk(os.path.dirname(ckpts[0])) for f in fs]
    assert left == [ckpts[0]]
    assert not os.path.exists(ckpts[0][:-len('.pth')])          # not even the output directory
    reset_cfg()
