"""--replay without a GPU: the flag on the four entry points, the declared kernel, the host side of the batch slot, and
losses.class_mask left as it was for host ids."""

import numpy as np
import pytest


@pytest.mark.parametrize('module', ['main', 'main_bert', 'pretrain_DAMSM', 'pretrain_DAMSM_bert'])
def test_replay_flag_parses_on_every_entry_point(module):
    import importlib
    m = importlib.import_module(module)
    assert m.parse_args([]).replay is False
    assert m.parse_args(['--replay']).replay is True
    assert m.parse_args(['--device_data', '--replay']).device_data is True


def test_trainer_defaults():
    import trainer
    import trainer_bert
    for cls in (trainer.condGANTrainer, trainer_bert.condGANTrainer):
        assert cls.replay is False and cls.replay_eager is False and cls.average_interval == 1000


def test_header_declares_batch_masks():
    from sbagan import _lib
    d = _lib.DECLS.get('sba_batch_masks')
    assert d and d.ret == 'int', 'sba_batch_masks is not declared'
    args = ['%s %s' % (ctext, arg) for ctext, arg, _ in d.params]
    assert len(args) == 7
    assert args[0].startswith('const int64_t*') and args[1].startswith('const int64_t*')
    assert args[2].startswith('uint8_t*') and args[3].startswith('uint8_t*') and args[6].startswith('void*')
    assert len(_lib.SIGNATURES['sba_batch_masks']) == 7


def test_blob_packing_round_trips():
    from sbagan.static_batch import blob_layout, pack_blob, unpack_blob
    rng = np.random.RandomState(3)
    for B, W, width in ((1, 1, 1), (4, 8, 8), (3, 7, 5), (20, 18, 18)):
        caps = rng.randint(0, 6000, (B, width)).astype(np.int64)
        lens = rng.randint(1, width + 1, B).astype(np.int64)
        ids = rng.randint(0, 200, B).astype(np.int64) + (np.arange(B, dtype=np.int64) % 2) * 2 ** 40
        params = rng.randint(0, 300, (B, 4)).astype(np.int32)
        blob = pack_blob(caps, lens, ids, B, W, params)
        assert blob.dtype == np.int64 and blob.shape == (blob_layout(B, W)[-1],) == (B * W + 4 * B,)
        c, n, k, p = unpack_blob(blob, B, W)
        assert np.array_equal(c[:, :width], caps) and not c[:, width:].any()     # a narrower batch is zero padded
        assert np.array_equal(n, lens) and np.array_equal(k, ids) and np.array_equal(p, params)
        assert k.dtype == np.int64 and p.dtype == np.int32
        # a WORDS_NUM x 1 column per caption (what the dataset hands out) packs the same; no params: zeros
        blob2 = pack_blob(caps.reshape(B, width, 1), lens, list(ids), B, W)
        c2, n2, k2, p2 = unpack_blob(blob2, B, W)
        assert np.array_equal(c2, c) and np.array_equal(n2, n) and np.array_equal(k2, k) and not p2.any()
    with pytest.raises(ValueError):
        pack_blob(np.zeros((3, 4)), np.zeros(3), np.zeros(3), 4, 4)          # another batch size
    with pytest.raises(ValueError):
        pack_blob(np.zeros((4, 5)), np.zeros(4), np.zeros(4), 4, 4)          # wider than the slot
    with pytest.raises(ValueError):
        pack_blob(np.zeros((4, 4)), np.zeros(4), np.zeros(4), 4, 4, np.zeros((3, 4), dtype=np.int32))


def test_slot_takes_a_host_batch_and_refuses_another_shape():
    """StaticBatch on the CPU device (no launch involved): load() of a batch whose integers are still on the host goes
    through pack_blob and one copy; the tensors keep their addresses; a batch of another size is refused in words"""
    import torch
    from sbagan.static_batch import StaticBatch
    B, W = 3, 6
    slot = StaticBatch(B, W, 2, 16, torch.device('cpu'), nef=8)
    assert [tuple(i.shape) for i in slot.imgs] == [(B, 3, 8, 8), (B, 3, 16, 16)]
    assert slot.mask.dtype == torch.bool and slot.class_mask.tensor.dtype == torch.uint8
    assert tuple(slot.words_embs.shape) == (B, 8, W) and tuple(slot.sent_emb.shape) == (B, 8)
    ptrs = [t.data_ptr() for t in (slot.captions, slot.cap_lens, slot.class_ids, slot.params)]
    rng = np.random.RandomState(1)
    for _ in range(2):
        imgs = [torch.from_numpy(rng.rand(B, 3, s, s).astype(np.float32)) for s in (8, 16)]
        caps = torch.from_numpy(rng.randint(0, 50, (B, W)).astype(np.int64))
        lens, ids = torch.tensor([6, 4, 2]), np.array([5, 5 + 2 ** 33, 5], dtype=np.int64)
        got = slot.load([imgs, caps, lens, ids, ['a', 'b', 'c']])
        assert got[1] is slot.captions and got[2] is slot.cap_lens and got[0] is slot.imgs and got[4] == ['a', 'b', 'c']
        assert torch.equal(slot.captions, caps) and slot.cap_lens.tolist() == [6, 4, 2]
        assert slot.class_ids.tolist() == ids.tolist()
        assert all(torch.equal(a, b) for a, b in zip(slot.imgs, imgs))
        assert slot.load(got) is got                        # already in the slot: passes through
    assert ptrs == [t.data_ptr() for t in (slot.captions, slot.cap_lens, slot.class_ids, slot.params)]
    small = [[i[:2] for i in imgs], caps[:2], lens[:2], ids[:2], ['a', 'b']]
    with pytest.raises(ValueError, match='drop the last'):
        slot.load(small)


def test_class_mask_from_host_ids_is_unchanged():
    import torch
    from miscc import losses
    for ids in ([5, 5, 2, 5], [1, 2, 3], [9], [4, 4, 4, 4, 4], [7, 7 + 2 ** 32, 7]):
        ids = np.asarray(ids, dtype=np.int64)
        B = len(ids)
        want = np.zeros((B, B), dtype=np.uint8)
        for i in range(B):
            for j in range(B):
                want[i, j] = 1 if (ids[j] == ids[i] and j != i) else 0
        losses._MASK_CACHE.clear()
        got = losses.class_mask(ids, B, torch.device('cpu'))
        assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), want)
        assert losses.class_mask(ids, B, torch.device('cpu')) is got          # the cache still serves repeated ids
        assert len(losses._MASK_CACHE) == 1
    assert losses.class_mask(None, 3, torch.device('cpu')) is None
