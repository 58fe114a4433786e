"""sba_batch_masks through the C ABI against numpy: word_mask = (captions == 0) (sbagan.trainer.build_mask), class_mask[i][j]
= (class_ids[j] == class_ids[i] and j != i) (miscc.losses.class_mask).  Bytes compared one for one, every byte 0 or 1, the
diagonal 0, 64 guard bytes around each output untouched, bad arguments refused before any launch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xAB
# one element; fewer elements than a wave; B * B far above B * L and the reverse; sizes that are no multiple of 64
SHAPES = [(1, 1), (2, 8), (3, 5), (20, 18), (64, 18), (65, 33)]


def _ids(kind, B):
    if kind == 'equal':
        return np.full(B, 41, dtype=np.int64)
    if kind == 'distinct':
        return (np.arange(B, dtype=np.int64) * 3 + 1)[::-1].copy()
    # pairs that differ only above bit 32: a 32-bit compare would call them equal
    return (7 + (np.arange(B, dtype=np.int64) % 3) * 2 ** 32 + (np.arange(B, dtype=np.int64) // 6)).astype(np.int64)


def _captions(kind, B, L):
    rng = np.random.RandomState(B * 100 + L)
    caps = rng.randint(1, 5000, (B, L)).astype(np.int64)
    if kind == 'start':
        caps[:, 0] = 0
        caps[::2, :min(L, 3)] = 0
    elif kind == 'middle':
        caps[:, L // 2] = 0
        for b in range(B):          # the usual shape too: zero padding behind row b's words
            caps[b, max(1, L - b % (L + 1)):] = 0
    return caps                     # 'nowhere': no zero at all


def _reference(caps, ids):
    B = len(ids)
    cm = np.zeros((B, B), dtype=np.uint8)
    for i in range(B):
        row = (ids == ids[i]).astype(np.uint8)
        row[i] = 0
        cm[i] = row
    return (caps == 0).astype(np.uint8), cm


def _guarded(n, dev):
    return torch.full((n + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)


def _entry(caps, ids, wm, cm, B, L):
    from sbagan import _lib
    ptr = lambda t, off=0: None if t is None else t.data_ptr() + off
    return _lib.lib.sba_batch_masks(ptr(caps), ptr(ids), ptr(wm, GUARD), ptr(cm, GUARD), B, L,
                                    torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize('zeros', ['start', 'middle', 'nowhere'])
@pytest.mark.parametrize('ids_kind', ['equal', 'distinct', 'high_bits'])
@pytest.mark.parametrize('B,L', SHAPES)
def test_masks_equal_numpy_byte_for_byte(B, L, ids_kind, zeros):
    dev = torch.device('cuda', 0)
    caps, ids = _captions(zeros, B, L), _ids(ids_kind, B)
    want_w, want_c = _reference(caps, ids)
    if ids_kind == 'high_bits' and B >= 2:
        assert (ids.astype(np.int32)[0] == ids.astype(np.int32)[1]) and ids[0] != ids[1]
    wm, cm = _guarded(B * L, dev), _guarded(B * B, dev)
    assert _entry(torch.from_numpy(caps).to(dev), torch.from_numpy(ids).to(dev), wm, cm, B, L) == 0
    wm, cm = wm.cpu().numpy(), cm.cpu().numpy()
    for got, want in ((wm, want_w), (cm, want_c)):
        body = got[GUARD:-GUARD].reshape(want.shape)
        assert set(np.unique(body).tolist()) <= {0, 1}
        assert np.array_equal(body, want)
        assert (got[:GUARD] == FILL).all() and (got[-GUARD:] == FILL).all()
    assert not np.diagonal(cm[GUARD:-GUARD].reshape(B, B)).any()


def test_bad_arguments_are_refused_and_write_nothing():
    dev = torch.device('cuda', 0)
    B, L = 3, 5
    caps = torch.from_numpy(_captions('middle', B, L)).to(dev)
    ids = torch.from_numpy(_ids('equal', B)).to(dev)
    wm, cm = _guarded(B * L, dev), _guarded(B * B, dev)
    from sbagan import _lib
    st = torch.cuda.current_stream().cuda_stream
    w, c = wm.data_ptr() + GUARD, cm.data_ptr() + GUARD
    bad = [(caps.data_ptr(), ids.data_ptr(), w, c, 0, L), (caps.data_ptr(), ids.data_ptr(), w, c, -1, L),
           (caps.data_ptr(), ids.data_ptr(), w, c, B, 0), (caps.data_ptr(), ids.data_ptr(), w, c, B, -4),
           (None, ids.data_ptr(), w, c, B, L), (caps.data_ptr(), None, w, c, B, L),
           (caps.data_ptr(), ids.data_ptr(), None, c, B, L), (caps.data_ptr(), ids.data_ptr(), w, None, B, L)]
    for a in bad:
        assert _lib.lib.sba_batch_masks(*a, st) != 0, a
    torch.cuda.synchronize()
    assert bool((wm == FILL).all()) and bool((cm == FILL).all())


def test_wrapper_writes_bool_mask_and_class_mask():
    """ops.batch_masks: the bool view the generator takes, the ClassMask the losses take, against the project's own
    build_mask / class_mask"""
    from miscc import losses
    from sbagan import ops
    from sbagan.trainer import build_mask
    dev = torch.device('cuda', 0)
    B, L = 5, 7
    caps = torch.from_numpy(_captions('middle', B, L)).to(dev)
    ids = np.array([3, 9, 3, 3, 9], dtype=np.int64)
    mask = torch.zeros((B, L), dtype=torch.bool, device=dev)
    cm = ops.ClassMask(torch.zeros((B, B), dtype=torch.uint8, device=dev))
    ops.batch_masks(caps, torch.from_numpy(ids).to(dev), mask, cm)
    assert torch.equal(mask, build_mask(caps, L))
    assert torch.equal(cm.tensor, losses.class_mask(ids, B, dev))
    assert losses.class_mask(cm, B, dev) is cm.tensor
    with pytest.raises(ValueError):
        losses.class_mask(cm, B + 1, dev)
    with pytest.raises(ValueError):
        ops.ClassMask(torch.zeros((B, L), dtype=torch.uint8, device=dev))
