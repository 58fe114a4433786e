"""Fused inference generator: every conv + BatchNorm(eval) + GLU of a generator as ONE launch.

In eval mode a BatchNorm is a per-channel affine that is known once the checkpoint is loaded.  FusedGenerator folds it
into the weights of the layer in front of it (sba_fold_bn_pack: w' = w * gamma / sqrt(var + eps) in f32, rounded once
to the compute dtype; b' = beta - mean * gamma / sqrt(var + eps)) and runs

  * upBlock and the first half of a ResBlock as sba_conv_igemm_glu: the GLU is applied to the accumulators (the value
    and gate channels are interleaved at pack time so that both sit in the same lane) and only the C output channels
    are written -- the training layer sequence writes the 2C-channel pre-BatchNorm tensor, reads it back and writes C;
  * the second half of a ResBlock as sba_conv_igemm_bias with the folded bias and the block's input as the addend;
  * INIT_STAGE_G.fc (Linear + BatchNorm1d + GLU + view) as sba_linear_glu_fwd.

Everything else (CA_NET, MAPPING_NET, attention, AdaIN, the image heads, the stream forks) is the wrapped module's own
forward: the wrapper only takes over the three layer types above while its call runs.  It holds no parameters and
never writes to the wrapped module.
"""
import ctypes

import torch

from . import _lib, nets, ops
from ._lib import call

_p, _stream = ops._p, ops._stream


class _Folded(object):
    """folded operands of one layer: w (compute dtype, row-major packed), wf (fragment-major copy or None), bias (f32)"""
    __slots__ = ('w', 'wf', 'bias', 'rows', 'C', 'kind')


def _fold(weight, bn, taps, cin, glu, dtype, frag):
    O = weight.shape[0]
    f = _Folded()
    f.C = O // 2 if glu else O
    f.rows = 64 * ((f.C + 31) // 32) if glu else O
    f.w = torch.empty(f.rows * taps * cin, dtype=dtype, device=weight.device)
    f.bias = torch.empty(f.rows, dtype=torch.float32, device=weight.device)
    call('sba_fold_bn_pack', _lib.SBA_BF16 if dtype == torch.bfloat16 else _lib.SBA_F32, _p(weight), _p(bn.weight),
         _p(bn.bias), _p(bn.running_mean), _p(bn.running_var), ops.BN_EPS, _p(f.w), _p(f.bias), O, taps, cin,
         1 if glu else 0, _stream())
    f.wf = None
    # the register-weight halo kernel's operand: the layers PackedWeight.fwd_frag gives one to (bf16, Cin 64 / 128, rows % 64)
    if frag and dtype == torch.bfloat16 and taps == 9 and cin in (64, 128) and f.rows % 64 == 0:
        f.wf = torch.empty_like(f.w)
        ops._pack_frag([(f.w, f.wf, f.rows, 9, cin)], weight.device)
    return f


class FusedGenerator(object):
    """FusedGenerator(netG)(noise, sent_emb, words_embs, mask) == netG.eval()(...) with the BatchNorms folded.

    netG: model.G_NET, model_bert.G_NET or model_bert.G_NET_MIX (any BRANCH_NUM / R_NUM / GF_DIM).  Call refold() after
    the module's parameters or running statistics changed (load_state_dict, load_params) or after
    ops.set_compute_dtype()."""

    def __init__(self, netG):
        if not isinstance(netG, nets._GBase):
            raise TypeError('FusedGenerator wraps a generator (G_NET / G_NET_BERT / G_NET_MIX), got %s' % type(netG).__name__)
        self.netG = netG
        self.refold()

    def refold(self):
        dtype = ops.compute_dtype()
        L = {}
        with torch.no_grad():
            for m in self.netG.modules():
                if isinstance(m, nets._UpBlock):
                    l = m._layer()
                    w = l.pw._master()
                    # (behind the upsample the LDS-weight halo kernel is the measured choice: ops.conv_forward)
                    L[id(m)] = _fold(w, l.bn, 9, w.shape[1], True, dtype, frag=False)
                elif isinstance(m, nets.ResBlock):
                    l1, l2 = m._layers()
                    w1, w2 = l1.pw._master(), l2.pw._master()
                    L[id(m)] = (_fold(w1, l1.bn, 9, w1.shape[1], True, dtype, frag=True),
                                _fold(w2, l2.bn, 9, w2.shape[1], False, dtype, frag=True))
                elif isinstance(m, nets._FcBnGlu):
                    w = m[0].weight.detach()
                    if not w.is_contiguous():
                        raise RuntimeError('INIT_STAGE_G.fc weight must be contiguous')
                    L[id(m)] = _fold(w, m[1], 1, w.shape[1], True, torch.float32, frag=False)
        self._layers, self._dtype = L, dtype
        return self

    # ---- the call ------------------------------------------------------------------------------------------------
    def __call__(self, noise, sent_emb, words_embs, mask):
        if torch.is_grad_enabled():
            raise RuntimeError('FusedGenerator is an inference path (folded BatchNorm, no backward): call it under '
                               'torch.no_grad()')
        if self.netG.training:
            raise RuntimeError('FusedGenerator folds the RUNNING statistics: put the generator in eval mode first '
                               '(netG.eval())')
        if ops.compute_dtype() != self._dtype:
            raise RuntimeError('the compute dtype changed since the weights were folded: call refold()')
        if nets._FUSED[0] is not None:
            raise RuntimeError('another FusedGenerator call is running')
        nets._FUSED[0] = self
        try:
            return self.netG(noise, sent_emb, words_embs, mask)
        finally:
            nets._FUSED[0] = None

    def _of(self, m):
        f = self._layers.get(id(m))
        if f is None:
            raise RuntimeError('%s is not a layer of the wrapped generator' % type(m).__name__)
        return f

    @staticmethod
    def _glu_geom(kind, x, f):
        N, Cin, H, W = x.shape
        # (geometry objects are cached per shape; the kernel family depends on the dtype as well: one object per dtype)
        g = ops._geom((kind, N, H, W, Cin, f.rows, ('glu', f.C, ops._dt(x))))
        if getattr(g, '_glu_halo', None) is None:
            plan = (ctypes.c_int * 3)()
            g.w_layout = 0
            call('sba_conv_igemm_glu_plan', ops._dt(x), ctypes.byref(g), f.C, plan)
            g._glu_halo = plan[0] == 0
        return g

    def _conv_glu(self, x, f, kind):
        x = ops.as_act(x)
        ops._need_gpu(x)
        N, Cin, H, W = x.shape
        OH, OW = ops._conv_out_hw(kind, H, W)
        y = ops.empty_act(N, f.C, OH, OW, x)
        g = self._glu_geom(kind, x, f)
        w = f.w
        if f.wf is not None and g._glu_halo:
            w, g.w_layout = f.wf, 1
        try:
            call('sba_conv_igemm_glu', ops._dt(x), _p(x), _p(w), _p(f.bias), _p(y), f.C, ctypes.byref(g), _stream())
        finally:
            g.w_layout = 0
        return y

    def _conv_bias_add(self, x, f, res):
        N, Cin, H, W = x.shape
        y = ops.empty_act(N, f.C, H, W, x)
        g = ops._geom(('3x3', N, H, W, Cin, f.C, None))
        dt = ops._dt(x)
        ops.tune_geom(g, dt)
        ws = ops.workspace(x.device)
        w = f.w
        g.w_layout = 0
        if f.wf is not None and ops._halo_family(g):
            w, g.w_layout = f.wf, 1
        try:
            call('sba_conv_igemm_bias', dt, _p(x), _p(w), _p(y), _p(res), None, _p(f.bias), None, ctypes.byref(g),
                 ws.data_ptr(), ops.WORKSPACE_BYTES, _stream())
        finally:
            g.w_layout = 0
        return y

    # ---- called by the layer modules while a call runs (nets._FUSED) ----------------------------------------------
    def conv_glu(self, m, x):
        return self._conv_glu(x, self._of(m), m.kind)

    def res_block(self, m, x):
        f1, f2 = self._of(m)
        x = ops.as_act(x)
        a = self._conv_glu(x, f1, '3x3')
        return self._conv_bias_add(a, f2, x)

    def fc_glu(self, m, x):
        f = self._of(m)
        ops._need_gpu(x)
        x = x.float().contiguous()
        B, K = x.shape
        out = torch.empty((B, f.C // 16, 4, 4), dtype=self._dtype, device=x.device, memory_format=ops.CL)
        call('sba_linear_glu_fwd', _lib.SBA_BF16 if self._dtype == torch.bfloat16 else _lib.SBA_F32, _p(x), _p(f.w),
             _p(f.bias), _p(out), B, K, f.C, _stream())
        return out
