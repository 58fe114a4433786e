"""One update of the DAMSM pre-training loop (AttnGAN2/code/pretrain_DAMSM.py:49-130): the text encoder and the two
embedding layers of the image encoder are trained with the words / sentence matching losses.

    words_features, sent_code = cnn_model(imgs[-1])          frozen Inception trunk (HIP implicit-GEMM kernels,
                                                             no tape) + emb_features / emb_cnn_code (trainable)
    words_emb, sent_emb = rnn_model(captions, cap_lens, h)   bi-LSTM with dropout, HIP recurrence + BPTT kernels
    loss = w_loss0 + w_loss1 + s_loss0 + s_loss1             fused all-pairs DAMSM kernels, gradients to both sides
    loss.backward(); clip_grad_norm(rnn params, RNN_GRAD_CLIP); Adam(lr, betas (0.5, 0.999)).step()

The two embedding layers are plain GEMMs (1x1 conv over 289 regions, Linear on the pooled code) and run through
the BLAS library; everything else on the path is a hand-written kernel.

With a BertEncoder as the text side (pretrain_DAMSM_bert.py) the trunk is frozen but runs in train mode (dropout) and
only its heads train: pooler.dense, fc and conv_text (model_bert.py:171-175).  The text forward is
sbagan.bert_hip.BertHIP.train_forward with a seed drawn from torch's generator when the step is built and a dropout
offset that advances once per step(); the clip norm covers exactly those head parameters."""
import torch
import torch.nn as nn

from miscc.config import cfg
from miscc.losses import sent_loss, words_loss

from . import ops
from ._lib import call
from .trainer import FlatParams, FusedAdam


class _Trainable(nn.Module):
    def __init__(self, text_encoder, image_encoder):
        super(_Trainable, self).__init__()
        self.text_encoder = text_encoder
        self.emb_features = image_encoder.emb_features
        self.emb_cnn_code = image_encoder.emb_cnn_code


class _BertHeads(nn.Module):
    """The trained part of a BertEncoder: pooler.dense, fc, conv_text (the trunk stays out of the flat buffers)."""

    def __init__(self, enc):
        super(_BertHeads, self).__init__()
        self.pooler = enc.model.pooler.dense
        self.fc = enc.fc
        self.conv_text = enc.conv_text


class DAMSMStep(object):
    def __init__(self, text_encoder, image_encoder, batch_size, lr=None, grad_clip=None):
        from .encoders import BertEncoder
        from .inception_hip import InceptionHIP
        self.text_encoder, self.image_encoder = text_encoder, image_encoder
        self.batch_size = batch_size
        self.device = next(text_encoder.parameters()).device
        self.trunk = InceptionHIP(image_encoder)
        self.bert = isinstance(text_encoder, BertEncoder)
        text_side = _BertHeads(text_encoder) if self.bert else text_encoder
        self.trainable = _Trainable(text_side, image_encoder)
        for p in self.trainable.parameters():
            p.requires_grad_(True)
        self.flat = FlatParams(self.trainable)
        self.grad_clip = cfg.TRAIN.RNN_GRAD_CLIP if grad_clip is None else grad_clip
        self.labels = torch.arange(batch_size, dtype=torch.int64, device=self.device)
        self.set_lr(cfg.TRAIN.ENCODER_LR if lr is None else lr)
        # clip_grad_norm_(text_encoder.parameters()): the frozen BERT trunk has no gradients, so the heads alone
        self._rnn_params = list(text_side.parameters())
        if self.bert:
            self.seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
            self.offset = 0

    def set_lr(self, lr):
        """pretrain_DAMSM.py:264: a NEW Adam every epoch (moments restart) with the decayed learning rate."""
        self.flat.m.zero_()
        self.flat.v.zero_()
        self.opt = FusedAdam(self.flat, lr, betas=(0.5, 0.999))

    def image_forward(self, img):
        """CNN_ENCODER.forward (model.py:207-267) with gradients only into emb_features / emb_cnn_code."""
        # (training mode = the reference's cnn_model.train(): BatchNorm with batch statistics, running statistics moved)
        f768, pooled = self.trunk.trunk_features(img, train=self.image_encoder.training)    # [B,17,17,768], [B,2048]
        B = f768.shape[0]
        w = self.image_encoder.emb_features.weight.view(-1, 768)           # [nef, 768]
        feat = torch.matmul(f768.view(B, 289, 768), w.t())                  # [B, 289, nef]
        words_features = feat.transpose(1, 2).reshape(B, -1, 17, 17)
        sent_code = torch.nn.functional.linear(pooled, self.image_encoder.emb_cnn_code.weight,
                                               self.image_encoder.emb_cnn_code.bias)
        return words_features, sent_code

    def losses(self, img, captions, cap_lens, class_ids):
        B = self.batch_size
        words_features, sent_code = self.image_forward(img)
        if not self.bert:
            hidden = self.text_encoder.init_hidden(B)
            words_emb, sent_emb = self.text_encoder(captions, cap_lens, hidden)
        elif torch.is_grad_enabled():
            p = None if self.text_encoder.training else 0.0
            words_emb, sent_emb = self.text_encoder._hip_runner().train_forward(captions, p, self.seed, self.offset)
        else:
            words_emb, sent_emb = self.text_encoder(captions)
        w_loss0, w_loss1, attn_maps = words_loss(words_features, words_emb, self.labels, cap_lens, class_ids, B)
        s_loss0, s_loss1 = sent_loss(sent_code, sent_emb, self.labels, class_ids, B)
        return w_loss0, w_loss1, s_loss0, s_loss1

    def step(self, img, captions, cap_lens, class_ids):
        """Returns the four loss terms as device scalars."""
        ops.det_reset()
        self.flat.zero_grad()
        w0, w1, s0, s1 = self.losses(img, captions, cap_lens, class_ids)
        loss = w0 + w1 + s0 + s1
        loss.backward()
        # torch.nn.utils.clip_grad_norm(rnn_model.parameters(), cfg.TRAIN.RNN_GRAD_CLIP)   (pretrain_DAMSM.py:99-100)
        total = torch.sqrt(sum((p.grad.float() ** 2).sum() for p in self._rnn_params if p.grad is not None))
        coef = torch.clamp(self.grad_clip / (total + 1e-6), max=1.0)
        for p in self._rnn_params:
            if p.grad is not None:
                p.grad.mul_(coef)
        self.opt.step()
        if self.bert:
            self.offset += 1
        return {'w_loss0': w0.detach(), 'w_loss1': w1.detach(), 's_loss0': s0.detach(), 's_loss1': s1.detach(),
                'rnn_grad_norm': total.detach()}

    @torch.no_grad()
    def evaluate(self, img, captions, cap_lens, class_ids):
        """pretrain_DAMSM.py:133-163 (one batch)."""
        was = self.text_encoder.training
        self.text_encoder.eval()
        w0, w1, s0, s1 = self.losses(img, captions, cap_lens, class_ids)
        self.text_encoder.train(was)
        return (s0 + s1).detach(), (w0 + w1).detach()


SQNORM_PARTS = 64       # workgroups (= f64 partial sums) of the gradient norm: part of the result's rounding, keep fixed


class DAMSMSlotStep(object):
    """DAMSMStep's update over a static batch slot, as ONE recording (pretrain_DAMSM.py --replay).

    Holds a DAMSMStep (`base`: the flat buffers, the trunk, the image side, evaluate) and a StaticBatch(B, WORDS_NUM,
    levels=1, crop): per batch the caller loads the slot (slot.load, or a DeviceBatchLoader bound to it) and calls
    train().  Everything the update reads lives at one address for the whole run:

        keep     uint8 [B][WORDS_NUM][ninput]   the dropout mask, DRAWN EAGERLY per batch from torch's generator
                                                (bernoulli_(1 - p); all ones and scale 1 in eval mode or with p = 0)
        lr_dev   f32 [1]                        the learning rate, read by the recorded sba_clip_adam_prepare
        opt      ONE FusedAdam for the run      set_lr() zeroes m, v and the step counter in place
        out      f32 [2] = (norm, coef)         the text encoder's gradient norm and clip coefficient
        last     f32 [5] = (w0, w1, s0, s1, 1)  the latest batch's loss terms
        acc      f32 [5]                        their sums and the batch count since read_losses()

    The recorded launches: ops.batch_masks (class mask from the slot's ids), det_reset + zero_grad, the image side,
    ops.EmbedDropoutFn -> ops.LstmBidirTrainFn at L = WORDS_NUM, the four losses, backward, sba_sqnorm_partials over the
    text encoder's range of the flat gradient, sba_clip_adam_prepare, sba_adam_step_dscale (the coefficient over the
    text range, no scale over the rest), acc += last.

    The clip is FOLDED INTO ADAM: the update uses g * coef for the text encoder, but .grad keeps the UNCLIPPED gradient
    (DAMSMStep.step scales .grad in place).  The parameters, m and v come out the same.

    Batch 0 trains eagerly on the capture stream; then the update is recorded (stream capture, nothing executes) and
    handed to sba_replay_create; every later batch is one sba_replay_launch.  torch's generator state is restored around
    the recording.  eager=True, or a Python exception while the recording is constructed (one line is printed): the
    same launches issued eagerly over the same slot.  Only the construction is guarded, once; there is no retry around a
    failing device step.  read_losses() is the only host synchronisation."""

    def __init__(self, text_encoder, image_encoder, batch_size, crop, lr=None, grad_clip=None, eager=False,
                 max_streams=4, levels=1, verbose=False):
        from .static_batch import StaticBatch
        self.base = base = DAMSMStep(text_encoder, image_encoder, batch_size, lr=lr, grad_clip=grad_clip)
        if base.bert:
            raise RuntimeError('DAMSMSlotStep: the BERT text side takes its dropout offset as a host argument and '
                               'cannot be recorded')
        if not (text_encoder._hip_shape_ok(base.flat.data) and base.flat.data.is_cuda):
            raise RuntimeError('DAMSMSlotStep needs the HIP bi-LSTM training path (one-layer bidirectional LSTM, '
                               'nhidden 128 / 256, ninput % 4 == 0)')
        self.text_encoder, self.image_encoder = text_encoder, image_encoder
        self.batch_size, self.device = int(batch_size), base.device
        dev, flat = base.device, base.flat
        W = int(cfg.TEXT.WORDS_NUM)
        # (levels: the scales the loader yields, TREE.BRANCH_NUM = 1 in the DAMSM configurations; the largest is used)
        self.slot = StaticBatch(batch_size, W, int(levels), int(crop), dev)
        self.flat, self.opt = flat, base.opt
        self.keep = torch.ones((self.batch_size, W, text_encoder.ninput), dtype=torch.uint8, device=dev)
        self.lr_dev = torch.full((1,), float(base.opt.lr), dtype=torch.float32, device=dev)
        self.out = torch.zeros(2, dtype=torch.float32, device=dev)
        self.last = torch.zeros(5, dtype=torch.float32, device=dev)
        self.last[4] = 1.0
        self.acc = torch.zeros(5, dtype=torch.float32, device=dev)
        self.partials = torch.zeros(SQNORM_PARTS, dtype=torch.float64, device=dev)
        hidden = text_encoder.init_hidden(self.batch_size)
        self.h0, self.c0 = hidden[0].detach().float().contiguous(), hidden[1].detach().float().contiguous()
        # _Trainable registers the text encoder first: its parameters are ONE range [0, text_hi) of the flat buffers
        n_text = len(base._rnn_params)
        assert n_text > 0 and all(a is b for a, b in zip(flat.params[:n_text], base._rnn_params)), \
            'the text encoder\'s parameters must lead the flat buffers'
        self.text_hi = flat.offsets[n_text] if n_text < len(flat.params) else flat.n
        self.eager = bool(eager)
        self.max_streams, self.verbose = int(max_streams), bool(verbose)
        self.recording = self.graph = self.info = None
        self.recorded_scale = None
        self.batches = self.launched = 0

    # ---- DAMSMStep's surface, for the loop's evaluate() and the tests
    trainable = property(lambda self: self.base.trainable)

    def evaluate(self, img, captions, cap_lens, class_ids):
        return self.base.evaluate(img, captions, cap_lens, class_ids)

    def set_lr(self, lr):
        """a new epoch's Adam (pretrain_DAMSM.py:264: moments and step counter restart, decayed rate) IN PLACE: no new
        tensor, the recording survives"""
        self.lr_dev.fill_(float(lr))
        self.opt.lr = float(lr)
        self.flat.m.zero_()
        self.flat.v.zero_()
        self.opt.state.zero_()

    def load(self, batch):
        return self.slot.load(batch)

    def _scale(self):
        p = float(self.text_encoder.drop_prob)
        if not self.text_encoder.training or p == 0.0:
            return 0.0, 1.0
        return p, float(1.0 / (1.0 - p))       # (in double, rounded once to f32 at the launch)

    def _update(self, scale):
        """the recorded launches (issued eagerly for batch 0, with eager=True and after a failed construction)"""
        base, slot, flat, opt, enc = self.base, self.slot, self.flat, self.opt, self.text_encoder
        st = torch.cuda.current_stream().cuda_stream
        ops.batch_masks(slot.captions, slot.class_ids, slot.mask, slot.class_mask)
        ops.det_reset()
        flat.zero_grad()
        words_features, sent_code = base.image_forward(slot.imgs[-1])
        r = enc.rnn
        emb = ops.EmbedDropoutFn.apply(slot.captions, enc.encoder.weight, self.keep, scale)
        w_ih = torch.stack((r.weight_ih_l0, r.weight_ih_l0_reverse))
        w_hh = torch.stack((r.weight_hh_l0, r.weight_hh_l0_reverse))
        b_ih = torch.stack((r.bias_ih_l0, r.bias_ih_l0_reverse))
        b_hh = torch.stack((r.bias_hh_l0, r.bias_hh_l0_reverse))
        words_emb, sent_emb = ops.LstmBidirTrainFn.apply(emb, slot.cap_lens, w_ih, w_hh, b_ih, b_hh, self.h0, self.c0,
                                                         slot.words_num)
        B = self.batch_size
        w0, w1, _ = words_loss(words_features, words_emb, base.labels, slot.cap_lens, slot.class_mask, B)
        s0, s1 = sent_loss(sent_code, sent_emb, base.labels, slot.class_mask, B)
        (w0 + w1 + s0 + s1).backward()
        # clip_grad_norm_(rnn_model.parameters(), RNN_GRAD_CLIP) and Adam, the coefficient never leaving the device
        g, b = flat.grad.data_ptr(), opt.betas
        call('sba_sqnorm_partials', g, self.text_hi, self.partials.data_ptr(), SQNORM_PARTS, st)
        call('sba_clip_adam_prepare', opt.state.data_ptr(), self.partials.data_ptr(), SQNORM_PARTS,
             self.lr_dev.data_ptr(), float(base.grad_clip), b[0], b[1], self.out.data_ptr(), st)
        for lo, hi, coef in ((0, self.text_hi, self.out.data_ptr() + 4), (self.text_hi, flat.n, None)):
            if hi > lo:
                o = 4 * lo
                call('sba_adam_step_dscale', flat.data.data_ptr() + o, g + o, flat.m.data_ptr() + o,
                     flat.v.data_ptr() + o, None, None, opt.state.data_ptr(), hi - lo, b[0], b[1], opt.eps, coef, st)
        # (written by the stack kernel itself: a copy_ here would be a device-to-device copy NODE, which the replayer
        # cannot decode)
        torch.stack((w0.detach(), w1.detach(), s0.detach(), s1.detach()), out=self.last[:4])
        self.acc.add_(self.last)

    def _record(self, cap, scale):
        import ctypes
        from ._lib import lib
        from .trainer import _CAPTURE_MODE
        dev = self.device
        rng = torch.cuda.get_rng_state(dev)      # (host-side state: the draws of a run do not depend on the launch mode)
        try:
            graph = torch.cuda.CUDAGraph(keep_graph=True)
            with torch.cuda.graph(graph, stream=cap, capture_error_mode=_CAPTURE_MODE):
                self._update(scale)
            torch.cuda.synchronize()
            handle = ctypes.c_void_p()
            rc = lib.sba_replay_create(ctypes.c_void_p(int(graph.raw_cuda_graph())), self.max_streams,
                                       1 if self.verbose else 0, ctypes.byref(handle))
            if rc != 0:
                raise RuntimeError('sba_replay_create failed (%d): the captured update holds a node the replayer '
                                   'cannot re-issue' % rc)
            info = (ctypes.c_int * 8)()
            call('sba_replay_info', handle, info)
            self.info = dict(zip(('nodes', 'kernels', 'copies', 'memsets', 'streams', 'waits', 'events', 'host_calls'),
                                 list(info)))
            self.graph, self.recording, self.recorded_scale = graph, handle, scale
        except Exception as e:
            print('--replay: the DAMSM update could not be recorded (%s: %s); training on with eager updates'
                  % (type(e).__name__, e))
            self.recording, self.eager = None, True
            torch.cuda.synchronize()
        torch.cuda.set_rng_state(rng, dev)

    def train(self):
        """one update on the batch in the slot; nothing is returned and nothing waits: read_losses()"""
        n, self.batches = self.batches, self.batches + 1
        p, scale = self._scale()
        if p > 0.0:
            self.keep.bernoulli_(1.0 - p)
        else:
            self.keep.fill_(1)
        if n == 0:
            cap = torch.cuda.Stream(device=self.device)
            cap.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(cap):
                self._update(scale)
            torch.cuda.current_stream().wait_stream(cap)
            torch.cuda.synchronize()
            if not self.eager:
                self._record(cap, scale)
        elif self.recording is None:
            self._update(scale)
        else:
            if scale != self.recorded_scale:
                raise RuntimeError('DAMSMSlotStep: the update was recorded with dropout scale %r; the text encoder now '
                                   'asks for %r (its mode or drop_prob changed)' % (self.recorded_scale, scale))
            call('sba_replay_launch', self.recording, torch.cuda.current_stream().cuda_stream)
            self.launched += 1
        self.opt.done()

    def read_losses(self):
        """{'w_loss0', 'w_loss1', 's_loss0', 's_loss1'}: means over the batches since the last call (host floats) and
        'batches'; copies the accumulator to the host -- the loop's only synchronisation -- and zeroes it"""
        host = self.acc.cpu().tolist()
        self.acc.zero_()
        n = max(host[4], 1.0)
        return {'w_loss0': host[0] / n, 'w_loss1': host[1] / n, 's_loss0': host[2] / n, 's_loss1': host[3] / n,
                'batches': int(host[4])}

    def __del__(self):
        h = getattr(self, 'recording', None)
        if h:
            try:
                call('sba_replay_destroy', h)
            except Exception:
                pass
            self.recording = None
