"""Training batches made on the device (--device_data).

The PIL data path decodes, crops and resizes every image of every batch on the host, every epoch.  What varies per
epoch is only the crop offset, the flip and the caption choice, so:

  * DeviceImageCache decodes the split ONCE, with the dataset's own code (datasets.load_image: open, RGB, bounding-box
    window, Resize), and keeps the uint8 HWC images back to back in one device buffer;
  * DeviceBatchLoader draws, per batch, the images, captions, crop offsets and flips on the host, uploads those few
    integers, and one sba_batch_pyramid launch gathers, crops, mirrors, resizes to every scale and normalises --
    bit-identical to what datasets.get_imgs yields for the same draws.  It yields what datasets.prepare_data returns.

The resampling coefficients (resample_table) and the byte -> float table (normalize_lut) are made on the host: the
first in Python doubles exactly as PIL computes them, the second by the torch operations of miscc.transforms."""
import numpy as np
import torch
import torch.utils.data as data

import datasets
from miscc.config import cfg

from . import ops

PRECISION_BITS = 22         # PIL's 8-bit resampling: 32 - 8 - 2
TABLE_TAPS = 8
UPLOAD_CHUNK = 64 << 20     # bytes of pinned staging per upload


def resample_table(T, out):
    """PIL's 8-bit BILINEAR coefficients for resizing T -> out pixels: int32 [out][10] = {xmin, n, k0..k7}, the
    window [xmin, xmin + n) clipped to [0, T), k = int(0.5 + w 2^22) of the normalised triangle weights."""
    T, out = int(T), int(out)
    if out < 1 or T < out:
        raise ValueError('resample_table: needs 1 <= out <= T (got T = %d, out = %d)' % (T, out))
    scale = T / out
    support = 1.0 * scale
    table = np.zeros((out, 2 + TABLE_TAPS), dtype=np.int32)
    for xx in range(out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), T)
        n = xmax - xmin
        if n > TABLE_TAPS:
            raise ValueError('resample_table: T = %d -> %d needs %d taps (at most %d)' % (T, out, n, TABLE_TAPS))
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * (1.0 / scale))) for x in range(n)]
        total = 0.0
        for v in w:
            total += v
        table[xx, 0], table[xx, 1] = xmin, n
        for x, v in enumerate(w):
            v = v / total if total != 0.0 else v
            table[xx, 2 + x] = int(0.5 + v * (1 << PRECISION_BITS))
    return table


def normalize_lut():
    """float32 [256]: Normalize((.5, .5, .5), (.5, .5, .5))(ToTensor(byte)), by the very torch operations of
    miscc.transforms (u * (2 / 255) - 1 differs from it in 111 of the 256 bytes)"""
    t = torch.arange(256, dtype=torch.uint8).float().div_(255.0)
    return (t - torch.tensor(0.5, dtype=torch.float32)) / torch.tensor(0.5, dtype=torch.float32)


class _DecodedImages(data.Dataset):
    """image i of `dataset` as load_image makes it: a uint8 HWC tensor"""

    def __init__(self, dataset, resize):
        self.dataset, self.resize = dataset, resize

    def __len__(self):
        return len(self.dataset)

    def __getitem__(self, index):
        img = datasets.load_image(self.dataset.image_path(index), self.dataset.image_box(index), self.resize)
        return torch.from_numpy(np.array(img, dtype=np.uint8))


class DeviceImageCache(object):
    """Every image of `dataset`, decoded once and kept on `device`:

        data    uint8, all images back to back, each HWC
        offset  int64 [N] byte offset of image i        (offset_host: the numpy copy)
        hw      int32 [N][2] = {H_i, W_i}               (hw_host)

    The sizes come from the files' headers first, so the buffer is allocated once and a split that needs more than
    `max_bytes` is refused before anything is decoded.  Images are decoded by `workers` DataLoader workers and uploaded
    in chunks."""

    def __init__(self, dataset, resize, device, max_bytes, workers=0):
        if cfg.GAN.B_DCGAN:
            raise RuntimeError('the device-resident image cache serves the multi-scale pyramid; GAN.B_DCGAN is not '
                               'supported')
        n = len(dataset)
        if n < 1:
            raise RuntimeError('DeviceImageCache: the dataset is empty')
        hw = np.zeros((n, 2), dtype=np.int32)
        offset = np.zeros(n, dtype=np.int64)
        total = 0
        for i in range(n):
            h, w = datasets.loaded_size(dataset.image_path(i), dataset.image_box(i), resize)
            hw[i] = (h, w)
            offset[i] = total
            total += h * w * 3
            if total > max_bytes:
                raise RuntimeError('DeviceImageCache: the first %d of %d images need %d bytes, more than the %d allowed'
                                   % (i + 1, n, total, max_bytes))
        self._set_tables(hw, offset, total, device)
        self.data = torch.empty(total, dtype=torch.uint8, device=self.device)
        loader = data.DataLoader(_DecodedImages(dataset, resize), batch_size=None, shuffle=False,
                                 num_workers=int(workers))
        self._fill(loader)

    @classmethod
    def from_arrays(cls, arrays, device):
        """a cache of the given uint8 [H][W][3] arrays"""
        arrays = [np.ascontiguousarray(a, dtype=np.uint8) for a in arrays]
        if not arrays or any(a.ndim != 3 or a.shape[2] != 3 or a.size == 0 for a in arrays):
            raise ValueError('DeviceImageCache.from_arrays: needs at least one non-empty uint8 [H][W][3] array')
        self = cls.__new__(cls)
        hw = np.array([a.shape[:2] for a in arrays], dtype=np.int32)
        sizes = np.array([a.size for a in arrays], dtype=np.int64)
        offset = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        self._set_tables(hw, offset, int(sizes.sum()), device)
        self.data = torch.empty(self.nbytes, dtype=torch.uint8, device=self.device)
        self._fill(torch.from_numpy(a) for a in arrays)
        return self

    def _set_tables(self, hw, offset, total, device):
        self.device = torch.device(device)
        self.hw_host, self.offset_host, self.nbytes = hw, offset, int(total)
        self.hw = torch.from_numpy(hw).to(self.device)
        self.offset = torch.from_numpy(offset).to(self.device)

    def __len__(self):
        return int(self.hw_host.shape[0])

    def _fill(self, images):
        """copy the images, in index order, into self.data through one staging buffer"""
        stage = torch.empty(min(UPLOAD_CHUNK, self.nbytes), dtype=torch.uint8)
        if self.device.type == 'cuda':
            stage = stage.pin_memory()
        start = used = 0          # self.data[start : start + used] is staged

        def flush():
            self.data[start:start + used].copy_(stage[:used])

        count = 0
        for i, img in enumerate(images):
            flat = img.reshape(-1)
            if tuple(img.shape) != (int(self.hw_host[i, 0]), int(self.hw_host[i, 1]), 3):
                raise RuntimeError('DeviceImageCache: image %d decoded as %s, its header promised %s'
                                   % (i, tuple(img.shape), tuple(self.hw_host[i])))
            done = 0
            while done < flat.numel():
                if used == stage.numel():
                    flush()
                    start, used = start + used, 0
                take = min(stage.numel() - used, flat.numel() - done)
                stage[used:used + take] = flat[done:done + take]
                used, done = used + take, done + take
            count += 1
        flush()
        if count != len(self) or start + used != self.nbytes:
            raise RuntimeError('DeviceImageCache: %d of %d images arrived' % (count, len(self)))


_TABLES = {}


def pyramid_tables(T, levels, device):
    """(tab1, tab2, lut) on `device` for sba_batch_pyramid: the resample tables of T -> T / 2 and T -> T / 4 (None for
    the levels not asked for) and the byte -> float table; made once per (T, levels, device)"""
    key = (int(T), int(levels), str(device))
    if key not in _TABLES:
        tabs = [torch.from_numpy(resample_table(T, T >> l)).to(device) if l < levels else None for l in (1, 2)]
        _TABLES[key] = (tabs[0], tabs[1], normalize_lut().to(device))
    return _TABLES[key]


class Draws(object):
    """the host side of one batch, in output (length-sorted) order"""

    def __init__(self, index, x1, y1, flip, caption_index, captions, lengths, class_ids, keys):
        self.index, self.x1, self.y1, self.flip, self.caption_index = index, x1, y1, flip, caption_index
        self.captions, self.lengths, self.class_ids, self.keys = captions, lengths, class_ids, keys

    def params(self):
        """int32 [B][4] = {index, x1, y1, flip}"""
        return np.stack([self.index, self.x1, self.y1, self.flip], axis=1).astype(np.int32)


class DeviceBatchLoader(object):
    """Iterates a dataset like DataLoader(dataset, batch_size, shuffle, drop_last) followed by datasets.prepare_data:
    every item is [images per scale (float32, device), captions B x T int64, caption lengths (descending), class ids
    (numpy), keys].  All draws -- the epoch's permutation, and per image the caption, the crop offset and the flip --
    come from the loader's own numpy Generator(PCG64(seed)); `last_draws` holds those of the latest batch.  (Only a
    caption longer than WORDS_NUM still draws its word subset on numpy's global generator, inside get_caption.)"""

    def __init__(self, dataset, cache, batch_size, crop, levels, seed, shuffle=True, drop_last=True):
        if len(cache) != len(dataset):
            raise ValueError('DeviceBatchLoader: the cache holds %d images, the dataset %d' % (len(cache), len(dataset)))
        if int(cache.hw_host.min()) < crop:
            raise ValueError('DeviceBatchLoader: a %d px crop does not fit the smallest cached side (%d)'
                             % (crop, int(cache.hw_host.min())))
        ops.check_pyramid_shape(crop, levels)
        self.dataset, self.cache = dataset, cache
        self.batch_size, self.crop, self.levels = int(batch_size), int(crop), int(levels)
        self.shuffle, self.drop_last = shuffle, drop_last
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.last_draws = None
        self.slot = None

    def __len__(self):
        n, b = len(self.dataset), self.batch_size
        return n // b if self.drop_last else (n + b - 1) // b

    def epoch_indices(self):
        """the image indices of one epoch, batch by batch"""
        n = len(self.dataset)
        order = self.rng.permutation(n) if self.shuffle else np.arange(n)
        return [order[i * self.batch_size:(i + 1) * self.batch_size] for i in range(len(self))]

    def draw_batch(self, indices):
        """the draws of one batch of images (host only): per image, in the given order, the caption, x1, y1 and the
        flip; then everything sorted by caption length, descending"""
        ds, T = self.dataset, self.crop
        n = len(indices)
        which = np.zeros(n, dtype=np.int64)
        x1, y1, flip = (np.zeros(n, dtype=np.int64) for _ in range(3))
        captions, lengths = [], np.zeros(n, dtype=np.int64)
        for j, i in enumerate(indices):
            which[j] = int(i) * ds.embeddings_num + int(self.rng.integers(0, ds.embeddings_num))
            caption, lengths[j] = ds.get_caption(int(which[j]))
            captions.append(np.asarray(caption, dtype=np.int64).reshape(-1))
            H, W = (int(v) for v in self.cache.hw_host[int(i)])
            x1[j] = self.rng.integers(0, W - T + 1)
            y1[j] = self.rng.integers(0, H - T + 1)
            flip[j] = 1 if self.rng.random() < 0.5 else 0
        order = np.argsort(-lengths, kind='stable')
        index = np.asarray(indices, dtype=np.int64)[order]
        return Draws(index, x1[order], y1[order], flip[order], which[order], np.stack(captions)[order], lengths[order],
                     np.asarray([ds.class_id[int(i)] for i in index]), [ds.filenames[int(i)] for i in index])

    def center_batch(self, indices):
        """float32 [n][3][crop][crop] on the device: the given images through the same sba_batch_pyramid launch, each
        with the window in the middle, ((W - crop) // 2, (H - crop) // 2), and not flipped (sbagan.retrieval).  It
        draws nothing, touches neither `last_draws` nor a bound slot, and returns fresh tensors."""
        index = np.asarray(list(indices), dtype=np.int64)
        hw = self.cache.hw_host[index].astype(np.int64)
        x1, y1 = (hw[:, 1] - self.crop) // 2, (hw[:, 0] - self.crop) // 2
        params = np.stack([index, x1, y1, np.zeros_like(index)], axis=1).astype(np.int32)
        return ops.batch_pyramid(self.cache, params, self.crop, 1)[0]

    def bind(self, slot):
        """Write every further batch straight into `slot` (sbagan.static_batch.StaticBatch; None: back to fresh
        tensors per batch): captions, lengths, CLASS IDS and params go up in the loader's single upload, into the
        slot's blob, and the pyramid launch writes the slot's image tensors.  The items keep their form; their device
        tensors are the slot's."""
        if slot is not None:
            if (slot.batch_size, slot.levels, slot.crop) != (self.batch_size, self.levels, self.crop) \
                    or slot.device != self.cache.device:
                raise ValueError('DeviceBatchLoader.bind: the slot holds batches of %d at %d px x %d scales on %s; the '
                                 'loader makes %d at %d px x %d on %s'
                                 % (slot.batch_size, slot.crop, slot.levels, slot.device, self.batch_size, self.crop,
                                    self.levels, self.cache.device))
            if not self.drop_last and len(self.dataset) % self.batch_size:
                raise ValueError('DeviceBatchLoader.bind: a batch slot needs drop_last (the last batch would be smaller)')
        self.slot = slot

    def _into_slot(self, d, params):
        from .static_batch import SlotBatch, pack_blob
        slot = self.slot
        slot.upload(pack_blob(d.captions, d.lengths, d.class_ids, slot.batch_size, slot.words_num, params))
        ops.batch_pyramid(self.cache, params, self.crop, self.levels, params_dev=slot.params, out=slot.imgs[::-1])
        batch = SlotBatch([slot.imgs, slot.captions, slot.cap_lens, d.class_ids, d.keys])
        batch.slot = slot
        return batch

    def __iter__(self):
        dev = self.cache.device
        for indices in self.epoch_indices():
            d = self.draw_batch(indices)
            self.last_draws = d
            params = d.params()
            if self.slot is not None:
                yield self._into_slot(d, params)
                continue
            # one pinned upload: captions and lengths (int64), then params (int32)
            head = np.concatenate([d.captions.reshape(-1), d.lengths])
            blob = np.concatenate([head.view(np.uint8), params.reshape(-1).view(np.uint8)])
            blob = torch.from_numpy(blob).pin_memory().to(dev, non_blocking=True)
            words = blob[:head.nbytes].view(torch.int64)
            n = len(indices)
            imgs = ops.batch_pyramid(self.cache, params, self.crop, self.levels,
                                     params_dev=blob[head.nbytes:].view(torch.int32).view(n, 4))
            yield datasets.PreparedBatch([imgs[::-1], words[:-n].view(n, -1), words[-n:], d.class_ids, d.keys])


def from_cfg(dataset, crop, seed, gb, **kw):
    """the cache (images resized as the entry points' transform does, crop * 76 / 64) and the loader the entry points
    hand to their training loops"""
    dev = torch.device('cuda', cfg.GPU_ID)
    cache = DeviceImageCache(dataset, int(crop * 76 / 64), dev, max_bytes=int(gb * (1 << 30)),
                             workers=int(cfg.WORKERS))
    print('device_data: %d images, %.1f MiB on %s' % (len(cache), cache.nbytes / float(1 << 20), dev))
    return DeviceBatchLoader(dataset, cache, cfg.TRAIN.BATCH_SIZE, crop, cfg.TREE.BRANCH_NUM, seed, **kw)
