"""Host side of --device_data (sbagan/device_data.py): the resampling tables against PIL itself, the byte -> float table
against miscc.transforms, the loader's draws on a toy CUB-shaped directory, the command-line options and the operator's
refusals.  Nothing here needs a device."""
import numpy as np
import pytest
import torch
from PIL import Image

from pyramid_ref import resize_emulated, sample_images
from test_host_cpu import _make_dataset

SIZES = (16, 24, 48, 64, 100, 256)


@pytest.mark.parametrize('T', SIZES)
def test_emulation_equals_pil_bilinear(T):
    """the two integer passes from the product's resample_table == Image.resize(BILINEAR), byte for byte; mirroring
    commutes with the resize; on noise the other pass order does not give PIL's bytes (so the order is observable)"""
    order_matters = 0
    for factor in (2, 4):
        out = T // factor
        for kind, img in sample_images(T, seed=T + factor).items():
            pil = np.asarray(Image.fromarray(img).resize((out, out), Image.BILINEAR))
            mine = resize_emulated(img, out)
            assert mine.shape == pil.shape == (out, out, 3)
            assert int((mine != pil).sum()) == 0, (T, factor, kind)
            flipped = np.ascontiguousarray(img[:, ::-1])
            pil_flipped = np.asarray(Image.fromarray(flipped).resize((out, out), Image.BILINEAR))
            assert np.array_equal(pil_flipped, pil[:, ::-1]), (T, factor, kind)
            assert np.array_equal(resize_emulated(flipped, out), mine[:, ::-1]), (T, factor, kind)
            if kind != 'ramp':
                order_matters += int((resize_emulated(img, out, vertical_first=True) != pil).sum())
    if T >= 48:
        assert order_matters > 0


def test_resample_table_rows():
    from sbagan.device_data import resample_table
    t2, t4 = resample_table(256, 128), resample_table(256, 64)
    assert t2.dtype == np.int32 and t2.shape == (128, 10) and t4.shape == (64, 10)
    assert t2[0].tolist() == [0, 3, 1797559, 1797559, 599186, 0, 0, 0, 0, 0]
    assert t4[0].tolist() == [0, 6, 748983, 1048576, 1048576, 748983, 449390, 149797, 0, 0]
    for o in range(1, 127):       # interior rows
        assert t2[o].tolist() == [2 * o - 1, 4] + [v << 19 for v in (1, 3, 3, 1)] + [0] * 4
    for o in range(1, 63):
        assert t4[o].tolist() == [4 * o - 2, 8] + [v << 17 for v in (1, 3, 5, 7, 7, 5, 3, 1)]
    # the far end mirrors the near end, and every window lies inside the crop
    assert t2[127].tolist() == [253, 3, 599186, 1797559, 1797559, 0, 0, 0, 0, 0]
    for T in SIZES:
        for f in (2, 4):
            t = resample_table(T, T // f)
            assert (t[:, 0] >= 0).all() and (t[:, 0] + t[:, 1] <= T).all() and (t[:, 1] >= 1).all()
            assert (t[:, 1] <= 8).all()
    with pytest.raises(ValueError):
        resample_table(256, 16)         # 17 taps: not a table the kernel takes


def test_lut_equals_totensor_normalize():
    from miscc import transforms
    from sbagan.device_data import normalize_lut
    norm = transforms.Compose([transforms.ToTensor(), transforms.Normalize((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))])
    img = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)
    ref = norm(Image.fromarray(img))
    lut = normalize_lut()
    assert lut.dtype == torch.float32 and lut.shape == (256,)
    for c in range(3):
        assert torch.equal(lut, ref[c].reshape(-1))
    u = torch.arange(256, dtype=torch.float32)
    assert int((u * (2.0 / 255.0) - 1.0 != lut).sum()) > 0      # the closed form is NOT the same floats


def _toy(tmp_path, n_train=7):
    from miscc.config import cfg, reset_cfg
    reset_cfg()
    cfg.TREE.BRANCH_NUM, cfg.TEXT.CAPTIONS_PER_IMAGE, cfg.TEXT.WORDS_NUM, cfg.CUDA = 2, 2, 12, False
    import datasets
    root = str(tmp_path / 'toy')
    _make_dataset(root, n_train=n_train)
    return datasets.TextDataset(root, 'train', base_size=64, transform=None)


def test_cache_holds_the_dataset_bytes(tmp_path):
    import datasets
    from miscc.config import cfg, reset_cfg
    from sbagan.device_data import DeviceImageCache
    ds = _toy(tmp_path, n_train=3)
    cache = DeviceImageCache(ds, 152, 'cpu', max_bytes=1 << 30, workers=0)
    assert len(cache) == 3 and cache.hw_host.tolist() == [[152, 185]] * 3         # 90 x 110 -> shorter side 152
    assert cache.offset_host.tolist() == [0, 152 * 185 * 3, 2 * 152 * 185 * 3] and cache.nbytes == 3 * 152 * 185 * 3
    assert torch.equal(cache.hw.cpu(), torch.from_numpy(cache.hw_host))
    for i in range(3):
        img = np.asarray(datasets.load_image(ds.image_path(i), ds.image_box(i), 152))
        assert datasets.loaded_size(ds.image_path(i), ds.image_box(i), 152) == img.shape[:2]
        got = cache.data[int(cache.offset_host[i]):][:img.size].reshape(img.shape)
        assert np.array_equal(got.numpy(), img)
    need = 2 * 152 * 185 * 3
    with pytest.raises(RuntimeError, match=str(need)):
        DeviceImageCache(ds, 152, 'cpu', max_bytes=need - 1, workers=0)
    cfg.GAN.B_DCGAN = True
    with pytest.raises(RuntimeError, match='B_DCGAN'):
        DeviceImageCache(ds, 152, 'cpu', max_bytes=1 << 30, workers=0)
    reset_cfg()


def test_get_imgs_is_unchanged(tmp_path):
    """get_imgs through load_image == the open / convert / transform / per-scale resize it always was"""
    import random
    import datasets
    from miscc import transforms
    from miscc.config import reset_cfg
    ds = _toy(tmp_path, n_train=2)
    tf = transforms.Compose([transforms.Resize(152), transforms.RandomCrop(128), transforms.RandomHorizontalFlip()])
    random.seed(5)
    got = datasets.get_imgs(ds.image_path(1), ds.imsize, None, tf, normalize=ds.norm)
    random.seed(5)
    img = tf(Image.open(ds.image_path(1)).convert('RGB'))
    want = [ds.norm(transforms.Resize(64)(img)), ds.norm(img)]
    assert len(got) == 2 and all(torch.equal(a, b) for a, b in zip(got, want))
    reset_cfg()


def test_loader_draws(tmp_path):
    from miscc.config import reset_cfg
    from sbagan.device_data import DeviceBatchLoader, DeviceImageCache
    ds = _toy(tmp_path, n_train=7)
    cache = DeviceImageCache(ds, 152, 'cpu', max_bytes=1 << 30, workers=0)
    T = 128

    def epoch(loader):
        return [loader.draw_batch(ix) for ix in loader.epoch_indices()]

    loader = DeviceBatchLoader(ds, cache, 3, T, 2, seed=11)
    assert len(loader) == 2                                          # drop_last
    assert len(DeviceBatchLoader(ds, cache, 3, T, 2, seed=11, drop_last=False)) == 3
    full = DeviceBatchLoader(ds, cache, 3, T, 2, seed=11, drop_last=False)
    for _ in range(2):                                               # every index exactly once per epoch
        batches = epoch(full)
        assert [len(d.index) for d in batches] == [3, 3, 1]
        assert sorted(int(i) for d in batches for i in d.index) == list(range(7))
    seen_x, seen_y, flips = set(), set(), set()
    for _ in range(8):
        for d in epoch(loader):
            assert len(d.index) == 3 and len(set(d.index.tolist())) == 3
            H, W = cache.hw_host[d.index, 0], cache.hw_host[d.index, 1]
            assert (d.x1 >= 0).all() and (d.y1 >= 0).all() and (d.x1 + T <= W).all() and (d.y1 + T <= H).all()
            assert (np.diff(d.lengths) <= 0).all()                   # descending
            assert (d.caption_index // ds.embeddings_num == d.index).all()
            for j in range(3):                                       # the rows travelled together
                cap, n = ds.get_caption(int(d.caption_index[j]))
                assert n == d.lengths[j] and np.array_equal(cap.reshape(-1), d.captions[j])
                assert d.keys[j] == ds.filenames[int(d.index[j])] and d.class_ids[j] == ds.class_id[int(d.index[j])]
            assert d.captions.shape == (3, 12) and d.captions.dtype == np.int64
            assert d.params().dtype == np.int32 and d.params().shape == (3, 4)
            seen_x.update(d.x1.tolist()); seen_y.update(d.y1.tolist()); flips.update(d.flip.tolist())
    assert max(seen_x) > 152 - T and max(seen_x) <= 185 - T          # the non-square side is used, never overrun
    assert max(seen_y) <= 152 - T and flips == {0, 1}
    # the same seed gives the same draws, another seed different ones
    a, b, c = (DeviceBatchLoader(ds, cache, 3, T, 2, seed=s) for s in (4, 4, 5))
    pa, pb, pc = (np.concatenate([d.params() for d in epoch(l)] + [d.params() for d in epoch(l)]) for l in (a, b, c))
    assert np.array_equal(pa, pb) and not np.array_equal(pa, pc)
    assert not np.array_equal(pa[:6], pa[6:])                        # and the second epoch is not the first
    no_shuffle = DeviceBatchLoader(ds, cache, 3, T, 2, seed=4, shuffle=False)
    assert sorted(np.concatenate(no_shuffle.epoch_indices()).tolist()) == list(range(6))
    with pytest.raises(ValueError):
        DeviceBatchLoader(ds, cache, 3, 160, 2, seed=1)              # a crop larger than the cached images
    reset_cfg()


def test_cli_options():
    from miscc import cli
    args = cli.options('x', 'cfg/bird_attn2.yml', [])
    assert args.device_data is False and args.device_data_gb == 64.0
    args = cli.options('x', 'cfg/bird_attn2.yml', ['--device_data', '--device_data_gb', '2.5'], bert=True)
    assert args.device_data is True and args.device_data_gb == 2.5


def test_batch_pyramid_refuses_before_the_device():
    """a CPU cache: every refusal below comes before the first device call (which a CPU cache could not survive)"""
    from sbagan import ops
    from sbagan.device_data import DeviceImageCache
    rng = np.random.RandomState(0)
    cache = DeviceImageCache.from_arrays([rng.randint(0, 256, (20, 30, 3)), rng.randint(0, 256, (40, 24, 3))], 'cpu')

    def params(*rows):
        return np.asarray(rows, dtype=np.int32)

    with pytest.raises(ValueError, match='window'):
        ops.batch_pyramid(cache, params([0, 0, 0, 0], [0, 15, 0, 1]), 16, 3)        # x1 + T = W + 1
    with pytest.raises(ValueError, match='window'):
        ops.batch_pyramid(cache, params([1, 8, 25, 0]), 16, 3)                      # y1 + T = H + 1
    with pytest.raises(ValueError, match='window'):
        ops.batch_pyramid(cache, params([1, -1, 0, 0]), 16, 3)
    with pytest.raises(ValueError, match='index'):
        ops.batch_pyramid(cache, params([2, 0, 0, 0]), 16, 3)                       # index == N
    with pytest.raises(ValueError, match='multiple'):
        ops.batch_pyramid(cache, params([0, 0, 0, 0]), 18, 3)
    with pytest.raises(ValueError, match='levels'):
        ops.batch_pyramid(cache, params([0, 0, 0, 0]), 16, 4)
    with pytest.raises(RuntimeError, match='no CPU'):                               # a valid call reaches the device check
        ops.batch_pyramid(cache, params([0, 14, 4, 0], [1, 8, 24, 1]), 16, 3)
