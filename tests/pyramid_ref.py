"""Host references for the device-side batch pyramid (sbagan/device_data.py, sba_batch_pyramid).

  * resize_emulated: PIL's 8-bit BILINEAR resize of a square image as two integer passes in numpy, driven by the PRODUCT's
    resample_table -- horizontal first, the intermediate rounded to a byte, then vertical.  It is what the kernel
    computes; the CPU tests hold it against Image.resize itself.
  * pil_pyramid: the PIL path itself through miscc.transforms -- crop, FLIP_LEFT_RIGHT, Resize, ToTensor, Normalize: the
    reference of the GPU tests."""
import numpy as np
import torch
from PIL import Image


def _one_pass(a, table):
    """a [R][T][C] uint8 -> [R][out][C] uint8 along axis 1: byte = clip((2^21 + sum a k) >> 22, 0, 255) in int32"""
    out = np.empty((a.shape[0], table.shape[0], a.shape[2]), dtype=np.uint8)
    for o, row in enumerate(table):
        xmin, n = int(row[0]), int(row[1])
        acc = np.full((a.shape[0], a.shape[2]), 1 << 21, dtype=np.int32)
        for j in range(n):
            acc += a[:, xmin + j, :].astype(np.int32) * np.int32(row[2 + j])
        out[:, o, :] = np.clip(acc >> 22, 0, 255).astype(np.uint8)
    return out


def resize_emulated(img, out, vertical_first=False):
    """img [T][T][C] uint8 -> [out][out][C] uint8"""
    from sbagan.device_data import resample_table
    table = resample_table(img.shape[0], out)
    if vertical_first:
        return _one_pass(_one_pass(img.transpose(1, 0, 2), table).transpose(1, 0, 2), table)
    return _one_pass(_one_pass(img, table).transpose(1, 0, 2), table).transpose(1, 0, 2)


def sample_images(T, seed):
    """uniform noise, saturated 0 / 255 noise, and a ramp: [T][T][3] uint8 each"""
    rng = np.random.RandomState(seed)
    noise = rng.randint(0, 256, (T, T, 3)).astype(np.uint8)
    saturated = (rng.randint(0, 2, (T, T, 3)) * 255).astype(np.uint8)
    yy, xx = np.mgrid[0:T, 0:T]
    ramp = np.stack([(xx * 255) // (T - 1), (yy * 255) // (T - 1), ((xx + yy) * 255) // (2 * T - 2)], -1).astype(np.uint8)
    return {'noise': noise, 'saturated': saturated, 'ramp': ramp}


def pil_pyramid(arrays, params, T, levels):
    """[out_0 .. out_{levels-1}], out_l float32 [B][3][T >> l][T >> l], by the PIL path: arrays[index] cropped to the
    window at (x1, y1), mirrored when flip, resized from that crop to every smaller scale, normalised"""
    from miscc import transforms
    norm = transforms.Compose([transforms.ToTensor(), transforms.Normalize((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))])
    outs = [[] for _ in range(levels)]
    for index, x1, y1, flip in np.asarray(params).tolist():
        img = Image.fromarray(arrays[index]).crop((x1, y1, x1 + T, y1 + T))
        if flip:
            img = img.transpose(Image.FLIP_LEFT_RIGHT)
        for l in range(levels):
            outs[l].append(norm(img if l == 0 else transforms.Resize(T >> l)(img)))
    return [torch.stack(o) for o in outs]
