"""The static batch slot of the recorded training loop (--replay).

A recording of the training step (sbagan.trainer.ReplayedStep) re-issues launches whose ARGUMENTS are fixed: every
tensor the step reads must live at one address for the whole run.  StaticBatch owns those tensors for one batch:

    blob        int64, one allocation: captions [B][WORDS_NUM] | cap_lens [B] | class_ids [B] | loader params
                (int32 [B][4] = {index, x1, y1, flip}, used by the device loader only)
    mask        bool  [B][WORDS_NUM]      (captions == 0)         } made ON THE DEVICE from the blob by one recorded
    class_mask  uint8 [B][B], ops.ClassMask (same class, j != i)   } launch, ops.batch_masks
    words_embs  f32 [B][nef][WORDS_NUM], sent_emb f32 [B][nef]     the frozen text encoder's outputs (recorded too)
    imgs        f32 [B][3][S][S] per scale, smallest first          written eagerly: ops.batch_pyramid(out=) or copy_

Per batch the host packs the integers (pack_blob, pure numpy) and uploads them from pinned memory in ONE copy on the
current stream -- the stream the step is replayed from, so the copy is ordered behind the previous replay's reads.  Nothing
here synchronises with the device."""
import numpy as np
import torch

import datasets
from miscc.config import cfg

from . import ops


def blob_layout(batch_size, words_num):
    """element offsets (int64 units) of the blob's parts: (captions, cap_lens, class_ids, params, total)"""
    B, W = int(batch_size), int(words_num)
    return 0, B * W, B * W + B, B * W + 2 * B, B * W + 4 * B


def pack_blob(captions, cap_lens, class_ids, batch_size, words_num, params=None):
    """The host side of one batch as the slot's int64 blob (numpy).  captions: [B][<= WORDS_NUM] ids (a narrower
    array is zero padded), cap_lens and class_ids: [B]; params: the device loader's int32 [B][4], or None (zeros)."""
    B, W = int(batch_size), int(words_num)
    captions = np.asarray(captions, dtype=np.int64)
    captions = captions.reshape(captions.shape[0], -1)
    cap_lens = np.asarray(cap_lens, dtype=np.int64).reshape(-1)
    class_ids = np.asarray(class_ids, dtype=np.int64).reshape(-1)
    if captions.shape[0] != B or cap_lens.shape[0] != B or class_ids.shape[0] != B:
        raise ValueError('the batch slot holds %d rows; got %d captions, %d lengths, %d class ids (the loader must '
                         'drop the last, smaller batch)' % (B, captions.shape[0], cap_lens.shape[0], class_ids.shape[0]))
    if captions.shape[1] > W:
        raise ValueError('the batch slot holds captions of %d words; got %d' % (W, captions.shape[1]))
    o_cap, o_len, o_cls, o_par, total = blob_layout(B, W)
    blob = np.zeros(total, dtype=np.int64)
    blob[o_cap:o_len].reshape(B, W)[:, :captions.shape[1]] = captions
    blob[o_len:o_cls] = cap_lens
    blob[o_cls:o_par] = class_ids
    if params is not None:
        params = np.ascontiguousarray(params, dtype=np.int32)
        if params.shape != (B, 4):
            raise ValueError('the batch slot takes loader params int32 [%d][4]; got %s' % (B, params.shape))
        blob[o_par:].view(np.int32)[:] = params.reshape(-1)
    return blob


def unpack_blob(blob, batch_size, words_num):
    """(captions [B][WORDS_NUM], cap_lens [B], class_ids [B], params int32 [B][4]) views of a host blob"""
    B, W = int(batch_size), int(words_num)
    o_cap, o_len, o_cls, o_par, total = blob_layout(B, W)
    blob = np.asarray(blob)
    if blob.dtype != np.int64 or blob.shape != (total,):
        raise ValueError('unpack_blob: needs int64 [%d] (got %s %s)' % (total, blob.dtype, blob.shape))
    return (blob[o_cap:o_len].reshape(B, W), blob[o_len:o_cls], blob[o_cls:o_par],
            blob[o_par:].view(np.int32).reshape(B, 4))


class SlotBatch(datasets.PreparedBatch):
    """a prepared batch (datasets.as_batch form) whose device tensors ARE the slot's: StaticBatch.load passes it through"""
    slot = None


class StaticBatch(object):
    def __init__(self, batch_size, words_num, levels, crop, device, nef=None):
        B, W = int(batch_size), int(words_num)
        if B < 1 or W < 1:
            raise ValueError('StaticBatch: batch_size and words_num must be positive')
        ops.check_pyramid_shape(int(crop), int(levels))
        self.batch_size, self.words_num, self.levels, self.crop = B, W, int(levels), int(crop)
        self.device = dev = torch.device(device)
        nef = int(cfg.TEXT.EMBEDDING_DIM if nef is None else nef)
        o_cap, o_len, o_cls, o_par, total = blob_layout(B, W)
        self.blob = torch.zeros(total, dtype=torch.int64, device=dev)
        self.captions = self.blob[o_cap:o_len].view(B, W)
        self.cap_lens = self.blob[o_len:o_cls]
        self.class_ids = self.blob[o_cls:o_par]
        self.params = self.blob[o_par:].view(torch.int32).view(B, 4)
        self.mask = torch.zeros((B, W), dtype=torch.bool, device=dev)
        self.class_mask = ops.ClassMask(torch.zeros((B, B), dtype=torch.uint8, device=dev))
        self.words_embs = torch.zeros((B, nef, W), dtype=torch.float32, device=dev)
        self.sent_emb = torch.zeros((B, nef), dtype=torch.float32, device=dev)
        # smallest scale first, as the loaders yield them
        self.imgs = [torch.zeros((B, 3, self.crop >> l, self.crop >> l), dtype=torch.float32, device=dev)
                     for l in reversed(range(self.levels))]

    def upload(self, blob_host):
        """one pinned, non-blocking copy of a pack_blob array into the blob, on the current stream.  The staging
        buffer is a fresh pinned tensor per batch: torch's caching host allocator hands a pinned block out again only
        after the copy that read it has completed (it records an event on the copy's stream), so no staging buffer is
        rewritten under a copy in flight and nothing here waits for the device."""
        staged = torch.from_numpy(blob_host)
        if staged.dtype != torch.int64 or staged.numel() != self.blob.numel():
            raise ValueError('StaticBatch.upload: needs the int64 [%d] array of pack_blob' % self.blob.numel())
        if self.device.type == 'cuda':
            staged = staged.pin_memory()
        self.blob.copy_(staged, non_blocking=True)

    def load(self, batch):
        """Put one batch (what either loader yields, datasets.as_batch form) into the slot; returns the batch with
        the slot's tensors in it.  A batch the device loader has already written into this slot passes through.
        Integers that are still on the host are packed there and uploaded in one pinned copy; device tensors (a
        prepared batch of the torch DataLoader) are copied device to device, with the class ids uploaded beside
        them.  Images are copied with copy_."""
        if getattr(batch, 'slot', None) is self:
            return batch
        imgs, captions, cap_lens, class_ids, keys = batch
        B, W = self.batch_size, self.words_num
        if len(imgs) != self.levels or any(tuple(i.shape) != tuple(s.shape) for i, s in zip(imgs, self.imgs)):
            raise ValueError('the batch slot holds images %s; got %s (the loader must drop the last, smaller batch)'
                             % ([tuple(s.shape) for s in self.imgs], [tuple(i.shape) for i in imgs]))
        on_device = torch.is_tensor(captions) and captions.is_cuda
        if on_device:
            if captions.dim() != 2 or captions.size(0) != B or captions.size(1) > W or cap_lens.numel() != B:
                raise ValueError('the batch slot holds %d captions of %d words; got %s (the loader must drop the '
                                 'last, smaller batch)' % (B, W, tuple(captions.shape)))
            host = pack_blob(np.zeros((B, 0), dtype=np.int64), np.zeros(B, dtype=np.int64), class_ids, B, W)
            self.upload(host)
            if captions.size(1) < W:
                self.captions.zero_()
            self.captions[:, :captions.size(1)].copy_(captions)
            self.cap_lens.copy_(cap_lens.reshape(-1))
        else:
            to_np = lambda t: t.numpy() if torch.is_tensor(t) else np.asarray(t)
            self.upload(pack_blob(to_np(captions), to_np(cap_lens), class_ids, B, W))
        for dst, src in zip(self.imgs, imgs):
            dst.copy_(src, non_blocking=True)
        out = SlotBatch([self.imgs, self.captions, self.cap_lens, class_ids, keys])
        out.slot = self
        return out

    def prologue(self, text_encoder, encode=None):
        """The recorded prologue of the step (ReplayedStep(recorded_prologue=...)): ops.batch_masks into mask /
        class_mask, then the frozen text encoder's no-grad forward into words_embs / sent_emb -- deterministic
        launches that read and write the slot's tensors only.  encode(text_encoder, captions, cap_lens, out=(words_embs,
        sent_emb)): the trainers' static-output _encode hook; by default the bi-LSTM is called with
        max_len = WORDS_NUM and out=, any other encoder (BERT) as text_encoder(captions) followed by copy_."""
        if encode is None:
            if hasattr(text_encoder, 'init_hidden'):
                hidden = text_encoder.init_hidden(self.batch_size)

                def encode(enc, captions, cap_lens, out):
                    with torch.no_grad():
                        enc(captions, cap_lens, hidden, max_len=out[0].size(2), out=out)
            else:
                def encode(enc, captions, cap_lens, out):
                    with torch.no_grad():
                        w, s = enc(captions)
                    out[0].copy_(w)
                    out[1].copy_(s)
        outs = (self.words_embs, self.sent_emb)

        def run():
            ops.batch_masks(self.captions, self.class_ids, self.mask, self.class_mask)
            encode(text_encoder, self.captions, self.cap_lens, out=outs)
        return run


class SlotStep(object):
    """The training step over a StaticBatch, one call of train() per batch loaded into the slot:

        batch 0     ReplayedStep.warm_up: an eager step on the capture stream; then the step is RECORDED with
                    slot.prologue in front (capture executes nothing)
        batch 1     ReplayedStep.prioritize() -- one training step when priorities are on, else replay()
        batch 2..   ReplayedStep.replay()

    so every batch trains exactly once.  noise and the conditioning eps are the step's own static tensors and draws.
    eager=True, or a Python exception while the recording is constructed (one line is printed): the same slot, the
    same draws and the same prologue with the step launched eagerly (ReplayedStep._eager_step's form) -- capture is
    an optimisation, never a requirement.  This is no retry around a failing device step: only the construction is
    guarded, once."""

    def __init__(self, gan, slot, prologue, noise, eager=False):
        self.gan, self.slot, self.prologue, self.noise = gan, slot, prologue, noise
        self.args = (slot.imgs, slot.sent_emb, slot.words_embs, slot.mask, slot.cap_lens, slot.class_mask, noise)
        self.eager = bool(eager)
        self.recording = None
        self.eps = None
        self.batches = 0

    def _record(self, warm):
        from .trainer import ReplayedStep
        dev = self.gan.device
        rng = torch.cuda.get_rng_state(dev)      # (host-side state: the draws of a run do not depend on the launch mode)
        try:
            self.recording = ReplayedStep(self.gan, *self.args, recorded_prologue=self.prologue, warm=warm)
        except Exception as e:
            print('--replay: the step could not be recorded (%s: %s); training on with eager steps'
                  % (type(e).__name__, e))
            self.recording, self.eager = None, True
            torch.cuda.synchronize()
        torch.cuda.set_rng_state(rng, dev)

    def train(self):
        """train the batch in the slot; returns the dict of device scalars of GANStep.step"""
        from .trainer import ReplayedStep
        n, self.batches = self.batches, self.batches + 1
        if n == 0:
            warm = ReplayedStep.warm_up(self.gan, *self.args, recorded_prologue=self.prologue)
            self.eps = warm['eps']
            if not self.eager:
                self._record(warm)
            return warm['out']
        if self.recording is None:
            ops.weights_changed()
            self.noise.normal_(0, 1)
            self.eps.normal_(0, 1)
            if self.gan.augment is not None:
                self.gan.augment.draw()
            if self.gan.geo_augment is not None:
                self.gan.geo_augment.draw()
            self.prologue()
            return self.gan.step(*self.args, eps=self.eps)
        out = self.recording.prioritize() if n == 1 else None
        return self.recording.replay() if out is None else out

    def finish(self):
        self.gan.finish()

    def resync(self):
        """after parameters were edited behind the step's back (the EMA weights loaded for a dump or a checkpoint and
        put back): the recorded launches read packed copies of the weights, refreshed only where the capture did"""
        if self.recording is not None:
            self.recording.resync()
