"""--device_data on the device: sba_batch_pyramid against the PIL path itself (miscc.transforms), bit for bit; the loader
end to end against batches rebuilt on the host from its draws; the trainers fed by it."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from pyramid_ref import pil_pyramid  # noqa: E402
from test_host_cpu import _make_dataset  # noqa: E402

# (H, W, saturated): 0-2 the 16 px sources (16 x 16 is an exact fit), 3-4 ragged tiles, 5 the DAMSM size, 6 the GAN size
SOURCES = ((19, 23, 0), (16, 16, 1), (40, 17, 0), (120, 131, 0), (110, 101, 1), (355, 400, 0), (304, 330, 0))


@pytest.fixture(scope='module')
def cache():
    from sbagan.device_data import DeviceImageCache
    rng = np.random.RandomState(7)
    arrays = [(rng.randint(0, 2, (h, w, 3)) * 255 if sat else rng.randint(0, 256, (h, w, 3))).astype(np.uint8)
              for h, w, sat in SOURCES]
    return arrays, DeviceImageCache.from_arrays(arrays, torch.device('cuda', 0))


def _check(cache, params, T, levels):
    from sbagan import ops
    arrays, dev_cache = cache
    params = np.asarray(params, dtype=np.int32)
    outs = ops.batch_pyramid(dev_cache, params, T, levels)
    refs = pil_pyramid(arrays, params, T, levels)
    assert len(outs) == levels
    for l, (out, ref) in enumerate(zip(outs, refs)):
        assert out.dtype == torch.float32 and tuple(out.shape) == (len(params), 3, T >> l, T >> l)
        got = out.cpu()
        assert torch.equal(got, ref), 'level %d: %d of %d values differ' % (l, int((got != ref).sum()), ref.numel())


# every corner of the 19 x 23 and 40 x 17 sources, flips mixed, image 0 twice in one batch
@pytest.mark.parametrize('params', [
    [[0, 0, 0, 0], [1, 0, 0, 1], [2, 1, 24, 1]],
    [[0, 7, 0, 1], [0, 0, 3, 0], [2, 1, 0, 0]],
    [[0, 7, 3, 0], [2, 0, 24, 1], [1, 0, 0, 0]],
])
def test_small_crops_in_every_corner(cache, params):
    _check(cache, params, 16, 3)


@pytest.mark.parametrize('T,levels,params', [
    (48, 3, [[3, 40, 33, 1], [4, 0, 62, 0], [3, 83, 72, 0], [4, 53, 0, 1]]),      # ragged 32 px tiles; strictly inside
    (100, 2, [[3, 17, 11, 1], [4, 1, 10, 0], [3, 31, 20, 0]]),
    (64, 2, [[3, 67, 56, 0], [4, 20, 30, 1]]),
    (299, 1, [[5, 101, 56, 1], [5, 0, 0, 0]]),                                    # T % 4 != 0: the scalar store path
    (256, 3, [[6, 37, 24, 1], [6, 74, 48, 0]]),
    (20, 1, [[3, 3, 0, 1]]),
    (36, 3, [[3, 5, 6, 1], [4, 65, 74, 0]]),                  # T % 32 == 4: a tile of halo only
])
def test_kernel_equals_pil(cache, T, levels, params):
    _check(cache, params, T, levels)


def test_bad_rows_write_nothing_and_bad_levels_are_refused(cache):
    """the raw C entry: a row whose index or window is out of range leaves its image's outputs untouched and the other
    rows right; levels = 4 comes back as SBA_E_ARG"""
    from sbagan import _lib
    from sbagan.device_data import pyramid_tables
    arrays, c = cache
    dev, T, levels, N = c.device, 16, 3, len(arrays)
    params = np.asarray([[0, 2, 1, 1], [N, 0, 0, 0], [2, 1, 5, 0], [0, 8, 0, 0], [-1, 0, 0, 0], [2, 0, 25, 1]],
                        dtype=np.int32)           # rows 1, 4: index; rows 3, 5: window one pixel out
    good = [0, 2]
    tab1, tab2, lut = pyramid_tables(T, levels, dev)
    sentinel = 12345.0
    outs = [torch.full((len(params), 3, T >> l, T >> l), sentinel, device=dev) for l in range(levels)]
    p_dev = torch.from_numpy(params).to(dev)
    st = torch.cuda.current_stream().cuda_stream

    def entry(lv):
        return _lib.lib.sba_batch_pyramid(c.data.data_ptr(), c.offset.data_ptr(), c.hw.data_ptr(), N, p_dev.data_ptr(),
                                          len(params), T, lv, tab1.data_ptr(), tab2.data_ptr(), lut.data_ptr(),
                                          outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), st)

    assert entry(4) == -1 and entry(0) == -1
    torch.cuda.synchronize()
    assert all(bool((o == sentinel).all()) for o in outs)            # refused before any launch
    assert entry(levels) == 0
    refs = pil_pyramid(arrays, params[good], T, levels)
    for out, ref in zip(outs, refs):
        got = out.cpu()
        assert torch.equal(got[good], ref)
        assert bool((got[[1, 3, 4, 5]] == sentinel).all())


def _toy_cfg(words=12):
    from miscc.config import cfg, reset_cfg
    reset_cfg()
    cfg.GAN.GF_DIM, cfg.GAN.DF_DIM, cfg.TREE.BRANCH_NUM = 32, 64, 2
    cfg.TEXT.CAPTIONS_PER_IMAGE, cfg.TEXT.WORDS_NUM, cfg.TEXT.EMBEDDING_DIM = 2, words, 256
    cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.MAX_EPOCH, cfg.TRAIN.SNAPSHOT_INTERVAL = 2, 1, 1
    cfg.TRAIN.NET_E, cfg.TRAIN.NET_G, cfg.TRAIN.FLAG, cfg.CUDA, cfg.GPU_ID = '', '', True, True, 0
    s = cfg.TRAIN.SMOOTH
    s.GAMMA1, s.GAMMA2, s.GAMMA3, s.LAMBDA = 4.0, 5.0, 10.0, 5.0
    return cfg


def test_loader_equals_the_pil_path_end_to_end(tmp_path):
    """one epoch on the toy directory; every batch rebuilt on the host from last_draws with the dataset's own functions"""
    from PIL import Image
    import datasets
    from miscc import transforms
    from miscc.config import reset_cfg
    from sbagan.device_data import DeviceBatchLoader, DeviceImageCache
    _toy_cfg()
    root = str(tmp_path / 'toy')
    _make_dataset(root, n_train=5)
    ds = datasets.TextDataset(root, 'train', base_size=64, transform=None)
    T, dev = 128, torch.device('cuda', 0)
    cache = DeviceImageCache(ds, int(T * 76 / 64), dev, max_bytes=1 << 30, workers=2)
    assert cache.hw_host.tolist() == [[152, 185]] * 5                # not square
    loader = DeviceBatchLoader(ds, cache, 2, T, 2, seed=3)
    assert len(loader) == 2
    seen = 0
    for batch in loader:
        imgs, captions, cap_lens, class_ids, keys = batch
        d = loader.last_draws
        assert isinstance(batch, list) and datasets.as_batch(batch) is batch
        want = [[], []]
        for j in range(2):
            i = int(d.index[j])
            img = datasets.load_image(ds.image_path(i), ds.image_box(i), int(T * 76 / 64))
            img = img.crop((int(d.x1[j]), int(d.y1[j]), int(d.x1[j]) + T, int(d.y1[j]) + T))
            if d.flip[j]:
                img = img.transpose(Image.FLIP_LEFT_RIGHT)
            want[0].append(ds.norm(transforms.Resize(ds.imsize[0])(img)))
            want[1].append(ds.norm(img))
        assert len(imgs) == 2
        for k in range(2):
            assert imgs[k].device == dev and imgs[k].dtype == torch.float32
            assert torch.equal(imgs[k].cpu(), torch.stack(want[k])), 'scale %d' % k
        caps = [ds.get_caption(int(s)) for s in d.caption_index]
        assert captions.dtype == torch.int64 and captions.device == dev and cap_lens.device == dev
        assert torch.equal(captions.cpu(), torch.from_numpy(np.stack([c.reshape(-1) for c, _ in caps])))
        assert cap_lens.cpu().tolist() == [n for _, n in caps] and cap_lens[0] >= cap_lens[1]
        assert isinstance(class_ids, np.ndarray) and class_ids.tolist() == [ds.class_id[int(i)] for i in d.index]
        assert keys == [ds.filenames[int(i)] for i in d.index]
        seen += 1
    assert seen == 2
    reset_cfg()


def test_gan_trainer_fed_by_the_device_loader(tmp_path, monkeypatch):
    import yaml
    import datasets
    import main
    from miscc.config import cfg, reset_cfg
    from sbagan import device_data, ops
    from trainer import condGANTrainer
    _toy_cfg(words=8)
    ops.set_compute_dtype(torch.bfloat16)
    root = str(tmp_path / 'toy')
    _make_dataset(root)
    ds = datasets.TextDataset(root, 'train', base_size=64, transform=None)
    loader = device_data.from_cfg(ds, 128, seed=3, gb=1.0)
    assert isinstance(loader, device_data.DeviceBatchLoader) and len(loader) == 2
    out_dir = str(tmp_path / 'out')
    torch.manual_seed(3)
    algo = condGANTrainer(out_dir, loader, ds.n_words, ds.ixtoword, allow_random_encoders=True)
    algo.train(max_steps=2)
    for name in ('netG_epoch_%d.pth' % cfg.TRAIN.MAX_EPOCH, 'netD0.pth', 'netD1.pth'):
        assert os.path.isfile(os.path.join(out_dir, 'Model', name)), name
    assert loader.last_draws is not None
    sd = torch.load(os.path.join(out_dir, 'Model', 'netG_epoch_%d.pth' % cfg.TRAIN.MAX_EPOCH), map_location='cpu')
    assert all(bool(torch.isfinite(v).all()) for v in sd.values() if v.is_floating_point())

    # the entry point: a torch DataLoader without the flag, the device loader with it
    yml = tmp_path / 'toy.yml'
    yml.write_text(yaml.safe_dump({
        'CONFIG_NAME': 'toy', 'DATASET_NAME': 'toy', 'DATA_DIR': root, 'GPU_ID': 0, 'WORKERS': 0,
        'TREE': {'BRANCH_NUM': 2, 'BASE_SIZE': 64},
        'TRAIN': {'FLAG': True, 'NET_E': '', 'NET_G': '', 'BATCH_SIZE': 2, 'MAX_EPOCH': 1, 'SNAPSHOT_INTERVAL': 1},
        'GAN': {'GF_DIM': 32, 'DF_DIM': 64},
        'TEXT': {'EMBEDDING_DIM': 256, 'CAPTIONS_PER_IMAGE': 2, 'WORDS_NUM': 8}}))
    monkeypatch.chdir(tmp_path / 'toy')
    handed = []

    class Stub(object):
        def __init__(self, output_dir, dataloader, n_words, ixtoword):
            handed.append(dataloader)

        def train(self):
            pass

    base = ['--cfg', str(yml), '--gpu', '0', '--manualSeed', '5']
    main.main(base, make_trainer=Stub)
    main.main(base + ['--device_data', '--device_data_gb', '1'], make_trainer=Stub)
    assert type(handed[0]) is torch.utils.data.DataLoader
    assert isinstance(handed[1], device_data.DeviceBatchLoader)
    assert handed[1].crop == 128 and handed[1].levels == 2 and handed[1].batch_size == 2
    assert handed[1].cache.nbytes == 4 * 152 * 185 * 3
    reset_cfg()


def test_pretrain_damsm_with_device_data(tmp_path, monkeypatch):
    import yaml
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
        'TEXT': {'EMBEDDING_DIM': 256, 'CAPTIONS_PER_IMAGE': 2, 'WORDS_NUM': 12}}))
    monkeypatch.chdir(tmp_path / 'toy')
    import pretrain_DAMSM
    from sbagan import ops
    ops.set_compute_dtype(torch.bfloat16)
    model_dir = pretrain_DAMSM.main(['--cfg', str(yml), '--gpu', '0', '--manualSeed', '7', '--device_data'], max_steps=2)
    for name in ('text_encoder0.pth', 'image_encoder0.pth'):
        assert os.path.isfile(os.path.join(model_dir, name)), name
    reset_cfg()
