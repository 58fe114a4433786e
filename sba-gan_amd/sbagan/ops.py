"""Host-side operators over the C-ABI HIP library: tensor plumbing (torch owns the
device memory and the stream), convolution geometry, packed-weight caching, and the
torch.autograd.Function wrappers the module classes in model.py are built from.

Activations are logical NCHW tensors with channels_last strides, i.e. NHWC in
memory, of dtype COMPUTE_DTYPE (bfloat16 by default, float32 for the exact-f32
MFMA path).  Parameters, their gradients, statistics and losses are float32.

Parameter gradients are ACCUMULATED IN PLACE into `param.grad` by the kernels
(the reference only ever uses `loss.backward(); optimizer.step()`,
trainer.py:269-297); the autograd Functions therefore return None for
parameters.
"""
import collections
import ctypes
import os
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._lib import ACT_GLU, ACT_LRELU, ACT_NONE, ConvGeom, call

CL = torch.channels_last
COMPUTE_DTYPE = torch.bfloat16
BN_EPS, BN_MOMENTUM, IN_EPS = 1e-5, 0.1, 1e-5

_WEIGHT_EPOCH = [0]          # bumped whenever parameters are changed behind torch's back


def set_compute_dtype(dt):
    global COMPUTE_DTYPE
    assert dt in (torch.bfloat16, torch.float32)
    COMPUTE_DTYPE = dt
    _WEIGHT_EPOCH[0] += 1


def compute_dtype():
    return COMPUTE_DTYPE


def weights_changed():
    """Call after parameters were modified through raw pointers (fused Adam)."""
    _WEIGHT_EPOCH[0] += 1


_EPOCH_CELL = {}             # id(param) -> [counter] shared by all parameters of one network


def register_epoch(params, cell):
    """Give a group of parameters (one network) its own change counter, so that an optimizer step
    on one network does not invalidate the packed weights of the others."""
    for p in params:
        _EPOCH_CELL[id(p)] = cell


def _dt(t):
    if t.dtype == torch.float32:
        return _lib.SBA_F32
    if t.dtype == torch.bfloat16:
        return _lib.SBA_BF16
    if t.dtype == torch.float16:        # a raw conv output y in the bf16 path (Y_F16 below)
        return _lib.SBA_BF16_YH
    raise TypeError('unsupported activation dtype %s' % t.dtype)


# bf16 path, optional (SBA_Y_F16=1): the RAW conv outputs (the pre-BatchNorm tensors y, read only by the BatchNorm
# kernels, never an MFMA operand) stored as IEEE binary16 instead of bf16 -- the same bytes, three more mantissa bits:
# one of the two roundings per conv + BatchNorm + activation layer shrinks by 8x (include/sbagan_hip.h: SBA_BF16_YH;
# the epilogue saturates at +-65504).  Measured on the reference's B = 20 golden step in deterministic mode
# (profiles/r03_bf16_rounding_points.txt): it moves the bf16 step's deviation from the reference by +-3e-4 in BOTH
# directions (errD0 7.7e-4 -> 7.1e-4, errD2 9.3e-4 -> 1.2e-3): that deviation is a sum of ~30 roundings of ~1e-4 with
# random signs (tools/bf16_bisect.py), no single tensor dominates it -- so the default stays plain bf16.
Y_F16 = os.environ.get('SBA_Y_F16', '0') == '1'


def _act_dtype(y):
    """storage dtype of the activations around a raw conv output y"""
    return torch.bfloat16 if y.dtype == torch.float16 else y.dtype


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _need_gpu(t):
    if not t.is_cuda:
        raise RuntimeError('sbagan HIP operators need CUDA/HIP tensors (got a %s tensor); there is no CPU '
                           'fallback' % t.device)


def as_act(x, dtype=None):
    """logical NCHW, NHWC in memory, compute dtype."""
    dtype = dtype or COMPUTE_DTYPE
    if x.dtype != dtype:
        x = x.to(dtype)
    if x.dim() == 4 and not x.is_contiguous(memory_format=CL):
        x = x.contiguous(memory_format=CL)
    return x


def empty_act(n, c, h, w, like):
    return torch.empty((n, c, h, w), dtype=like.dtype, device=like.device, memory_format=CL)


def param_grad(p):
    """f32 gradient buffer of a parameter with the parameter's own memory layout."""
    if p.grad is None:
        p.grad = torch.zeros_like(p, memory_format=torch.preserve_format)
    return p.grad


# ----------------------------------------------------------------------------
# convolution geometry
# ----------------------------------------------------------------------------
_GEOM_CACHE = {}


def _geom(key):
    g = _GEOM_CACHE.get(key)
    if g is not None:
        return g
    kind, N, IH, IW, Cin, Cout, extra = key
    g = ConvGeom()
    g.N, g.IH, g.IW, g.Cin, g.Cout = N, IH, IW, Cin, Cout
    g.sy = g.sx = 1
    g.osy = g.osx = 1
    g.ooy = g.oox = 0
    g.ups = 0
    if kind in ('3x3', '3x3up'):
        up = 2 if kind == '3x3up' else 1
        g.OH, g.OW = IH * up, IW * up
        g.OHs, g.OWs = g.OH, g.OW
        g.ups = 1 if kind == '3x3up' else 0
        g.ntaps = 9
        for t in range(9):
            g.ty[t], g.tx[t] = t // 3 - 1, t % 3 - 1
    elif kind == '4x4s2':
        g.OH, g.OW = IH // 2, IW // 2
        g.OHs, g.OWs = g.OH, g.OW
        g.sy = g.sx = 2
        g.ntaps = 16
        for t in range(16):
            g.ty[t], g.tx[t] = t // 4 - 1, t % 4 - 1
    elif kind == '4x4s2_dgrad':
        # input = dY (IH x IW), output = dX (2IH x 2IW), parity class extra = (py, px)
        py, px = extra
        g.OH, g.OW = IH * 2, IW * 2
        g.OHs, g.OWs = IH, IW
        g.osy = g.osx = 2
        g.ooy, g.oox = py, px
        g.ntaps = 4
        for t in range(4):
            g.ty[t], g.tx[t] = py - t // 2, px - t % 2
    else:
        raise ValueError(kind)
    _GEOM_CACHE[key] = g
    return g


def _conv_out_hw(kind, H, W):
    if kind == '3x3':
        return H, W
    if kind == '3x3up':
        return 2 * H, 2 * W
    if kind == '4x4s2':
        return H // 2, W // 2
    raise ValueError(kind)


# data-gradient operand layouts (sba_pack_weight modes): flipped 3x3, four parity classes of the 4x4/s2
# conv, and the 4x4/s2 collapse of (nearest x2 -> conv3x3)
_DGRAD_MODE = {'3x3': 1, '4x4s2': 2, '3x3up': 3}


class PackedWeight(object):
    """Packed copies of one OIHW conv parameter (stored channels_last, i.e.
    [O][KH][KW][I] f32 in memory): the forward operand in the compute dtype and
    the data-gradient operand, rebuilt lazily when the parameter changes.  Inside a PackGroup
    (one per trained network) a stale copy triggers ONE launch that refreshes the whole network."""

    def __init__(self, param, kind=None):
        self.param = param
        self.kind = kind
        self.group = None
        self._fwd = self._dgrad = None
        self._kf = self._kd = None
        self._ffwd = self._fdgrad = None        # fragment-major copies (halo-tile 3x3 kernel: weights in registers)
        self._kff = self._kfd = None

    def _key(self, dtype):
        cell = _EPOCH_CELL.get(id(self.param))
        return (self.param._version, _WEIGHT_EPOCH[0], cell[0] if cell else 0, dtype, self.param.data_ptr())

    def _master(self):
        p = self.param.detach()
        if not p.is_contiguous(memory_format=CL):
            raise RuntimeError('conv parameters must be stored channels_last (use sbagan layers)')
        return p

    def fwd(self, dtype):
        if dtype == torch.float32:
            return self._master()
        k = self._key(dtype)
        if self._kf != k:
            if self.group is not None:
                self.group.refresh(dtype)
                return self._fwd
            p = self._master()
            O, I, KH, KW = p.shape
            if self._fwd is None or self._fwd.dtype != dtype:
                self._fwd = torch.empty(O * KH * KW * I, dtype=dtype, device=p.device)
            call('sba_pack_weight', _lib.SBA_BF16, _p(p), _p(self._fwd), O, KH, KW, I, 0, _stream())
            self._kf = k
        return self._fwd

    def fwd_frag(self, dtype):
        """the forward operand FRAGMENT-MAJOR (include/sbagan_hip.h: sba_pack_frag_multi), or None when the layer does not
        qualify (bf16, Cin 64 / 128, Cout % 64 == 0, 3 x 3)"""
        O, I, KH, KW = self.param.shape
        if dtype != torch.bfloat16 or KH != 3 or KW != 3 or I not in (64, 128) or O % 64:
            return None
        src = self.fwd(dtype)                   # (refreshes the group, frag copies included, when stale)
        k = self._key(dtype)
        if self._kff != k:
            if self._ffwd is None:
                self._ffwd = torch.empty(O * 9 * I, dtype=dtype, device=src.device)
            _pack_frag([(src, self._ffwd, O, 9, I)], src.device)
            self._kff = k
        return self._ffwd

    def dgrad_frag(self, dtype, kind):
        """the data-gradient operand of a stride-1 3 x 3 conv ([Cin][flipped tap][Cout]) fragment-major, or None"""
        O, I, KH, KW = self.param.shape
        if dtype != torch.bfloat16 or kind != '3x3' or O not in (64, 128) or I % 64:
            return None
        src = self.dgrad(dtype, kind)
        k = self._key(dtype) + (kind,)
        if self._kfd != k:
            if self._fdgrad is None:
                self._fdgrad = torch.empty(O * 9 * I, dtype=dtype, device=src.device)
            _pack_frag([(src, self._fdgrad, I, 9, O)], src.device)
            self._kfd = k
        return self._fdgrad

    def dgrad(self, dtype, kind):
        k = self._key(dtype) + (kind,)
        if self._kd != k:
            if self.group is not None and kind == self.kind:
                self.group.refresh(dtype)
                return self._dgrad
            p = self._master()
            O, I, KH, KW = p.shape
            mode = _DGRAD_MODE[kind]
            n = O * I * (16 if mode == 3 else KH * KW)
            if self._dgrad is None or self._dgrad.dtype != dtype or self._dgrad.numel() != n:
                self._dgrad = torch.empty(n, dtype=dtype, device=p.device)
            dcode = _lib.SBA_BF16 if dtype == torch.bfloat16 else _lib.SBA_F32
            call('sba_pack_weight', dcode, _p(p), _p(self._dgrad), O, KH, KW, I, mode, _stream())
            self._kd = k
        return self._dgrad


def _frag_descs(items, device):
    """device array of sba_frag_desc for items = [(src tensor, dst tensor, R, taps, K)] and the total unit count"""
    import numpy as np
    desc = np.zeros(len(items), dtype=np.dtype(_lib.STRUCTS['sba_frag_desc']))
    units = 0
    for d, (src, dst, R, taps, K) in zip(desc, items):
        d['src'], d['dst'], d['R'], d['taps'], d['K'], d['unit_begin'] = src.data_ptr(), dst.data_ptr(), R, taps, K, units
        units += R * taps * K // 8
    return torch.from_numpy(desc.view(np.uint8).copy()).to(device), units


def _pack_frag(items, device):
    descs, units = _frag_descs(items, device)
    call('sba_pack_frag_multi', descs.data_ptr(), len(items), units, _stream())
    _KEEP_DESC.append(descs)
    del _KEEP_DESC[:-64]


_KEEP_DESC = []         # descriptor arrays of the un-grouped path stay alive until their launch has surely run


class PackGroup(object):
    """The packed weights of all conv layers of one network, kept in two flat buffers (forward
    operands, data-gradient operands) and refreshed by ONE sba_pack_weights_multi launch when any
    of them is stale (normally: once after the network's optimizer step) instead of two launches
    per layer.  `layers` = [(PackedWeight, kind)] with kind in '3x3' | '3x3up' | '4x4s2'."""

    def __init__(self, layers):
        self.layers = [(pw, kind) for pw, kind in layers if pw.param.shape[1] % 4 == 0]
        self.state = {}             # dtype -> dict(fwd, tr, descs, ptrs, tiles)
        for pw, kind in self.layers:
            pw.group, pw.kind = self, kind

    def _build(self, dtype):
        import numpy as np
        dev = self.layers[0][0].param.device
        sizes = [pw.param.numel() for pw, _ in self.layers]
        tsizes = [pw.param.shape[0] * pw.param.shape[1] * (16 if kind == '3x3up' else pw.param.shape[2] * pw.param.shape[3])
                  for pw, kind in self.layers]
        offs, n = [], 0
        for k in sizes:
            offs.append(n)
            n += (k + 7) // 8 * 8
        toffs, tn = [], 0
        for k in tsizes:
            toffs.append(tn)
            tn += (k + 7) // 8 * 8
        st = {'fwd': torch.empty(n, dtype=dtype, device=dev) if dtype != torch.float32 else None,
              'tr': torch.empty(tn, dtype=dtype, device=dev)}
        esz = st['tr'].element_size()
        desc = np.zeros(len(self.layers), dtype=np.dtype(_lib.STRUCTS['sba_pack_desc']))
        tiles = 0
        for i, ((pw, kind), o) in enumerate(zip(self.layers, offs)):
            O, I, KH, KW = pw.param.shape
            d = desc[i]
            d['w'] = pw.param.data_ptr()
            d['fwd'] = st['fwd'].data_ptr() + o * esz if st['fwd'] is not None else 0
            d['tr'] = st['tr'].data_ptr() + toffs[i] * esz
            d['Cout'], d['KH'], d['KW'], d['Cin'] = O, KH, KW, I
            d['mode'] = _DGRAD_MODE[kind]
            d['tile_begin'] = tiles
            d['co_tiles'], d['ci_tiles'] = (O + 63) // 64, (I + 63) // 64
            tiles += (16 if d['mode'] == 3 else KH * KW) * d['co_tiles'] * d['ci_tiles']
            if st['fwd'] is not None:
                pw._fwd = st['fwd'][o:o + sizes[i]]
            pw._dgrad = st['tr'][toffs[i]:toffs[i] + tsizes[i]]
        st['descs'] = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
        st['ptrs'] = [pw.param.data_ptr() for pw, _ in self.layers]
        st['tiles'] = tiles
        # fragment-major copies of the 3 x 3 layers the halo-tile kernel serves (ONE more launch per refresh)
        st['frag'] = None
        if dtype == torch.bfloat16:
            items = []
            for pw, kind in self.layers:
                O, I, KH, KW = pw.param.shape
                if kind != '3x3' or KH != 3:
                    continue
                if I in (64, 128) and O % 64 == 0:
                    pw._ffwd = torch.empty(O * 9 * I, dtype=dtype, device=dev)
                    items.append((pw._fwd, pw._ffwd, O, 9, I))
                if kind == '3x3' and O in (64, 128) and I % 64 == 0:
                    pw._fdgrad = torch.empty(O * 9 * I, dtype=dtype, device=dev)
                    items.append((pw._dgrad, pw._fdgrad, I, 9, O))
            if items:
                st['frag'] = _frag_descs(items, dev) + (len(items),)
        self.state = {dtype: st}        # one compute dtype at a time (the views above belong to it)
        return st

    def refresh(self, dtype):
        st = self.state.get(dtype)
        if st is None or st['ptrs'] != [pw.param.data_ptr() for pw, _ in self.layers]:
            st = self._build(dtype)
        for pw, _ in self.layers:
            if not pw.param.is_contiguous(memory_format=CL):
                raise RuntimeError('conv parameters must be stored channels_last (use sbagan layers)')
        dcode = _lib.SBA_BF16 if dtype == torch.bfloat16 else _lib.SBA_F32
        call('sba_pack_weights_multi', dcode, st['descs'].data_ptr(), len(self.layers), st['tiles'], _stream())
        if st.get('frag') is not None:
            fd, units, nfrag = st['frag']
            call('sba_pack_frag_multi', fd.data_ptr(), nfrag, units, _stream())
        for pw, kind in self.layers:
            k = pw._key(dtype)
            pw._kf, pw._kd = k, k + (kind,)
            pw._kff, pw._kfd = k, k + (kind,)


class ZeroArena(object):
    """Bump allocator over one pre-zeroed f32 buffer for the many small accumulators of a step
    (BN statistics, backward reductions): ONE memset per step instead of one fill kernel per layer.
    Only active between begin() and end() (GANStep.step); otherwise zeros_f32 falls back to
    torch.zeros, so stand-alone module calls stay safe."""

    def __init__(self):
        self.buf, self.off, self.active = None, 0, False

    def begin(self, device, nfloats=4 << 20):
        if self.buf is None or self.buf.device != device or self.buf.numel() < nfloats:
            self.buf = torch.empty(nfloats, dtype=torch.float32, device=device)
        self.buf.zero_()
        self.off, self.active = 0, True

    def end(self):
        self.active = False

    def take(self, n, device):
        n4 = (n + 3) // 4 * 4
        if not self.active or self.buf.device != device or self.off + n4 > self.buf.numel():
            return None
        t = self.buf[self.off:self.off + n]
        self.off += n4
        return t


ARENA = ZeroArena()


def zeros_f32(shape, device):
    n = 1
    for d in (shape if isinstance(shape, (tuple, list)) else (shape,)):
        n *= d
    t = ARENA.take(n, device)
    if t is None:
        return torch.zeros(shape, dtype=torch.float32, device=device)
    return t.view(shape)


_WORKSPACE = {}
WORKSPACE_BYTES = 64 << 20


def workspace(device):
    """Per-(device, stream) scratch for split-K partial sums: launches on one stream reuse it in
    stream order; concurrent streams must not share it."""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = _WORKSPACE.get(key)
    if ws is None:
        with torch.cuda.stream(torch.cuda.default_stream(device)):
            ws = torch.zeros(WORKSPACE_BYTES, dtype=torch.uint8, device=device)   # contract: zero-filled
        torch.cuda.current_stream(device).wait_stream(torch.cuda.default_stream(device))
        _WORKSPACE[key] = ws
    return ws


_REDUCE_SCRATCH = {}
REDUCE_SCRATCH_BYTES = int(os.environ.get('SBA_REDUCE_SCRATCH_MB', '64')) << 20


def reduce_scratch(device):
    """The ring for the default mode's two-stage reductions (include/sbagan_hip.h: sba_set_reduce_scratch), handed to
    the library the first time an operator that uses it runs on `device` (SBA_REDUCE_SCRATCH_MB=0: none, atomics)."""
    if device not in _REDUCE_SCRATCH:
        if _REDUCE_SCRATCH and REDUCE_SCRATCH_BYTES:
            # the library keeps ONE ring (include/sbagan_hip.h): a second device would silently re-point it
            raise RuntimeError('sbagan runs one process per GPU: the reduction scratch ring already belongs to %s'
                               % next(iter(_REDUCE_SCRATCH)))
        buf = None
        if REDUCE_SCRATCH_BYTES:
            with torch.cuda.stream(torch.cuda.default_stream(device)):
                buf = torch.empty(REDUCE_SCRATCH_BYTES, dtype=torch.uint8, device=device)
            torch.cuda.current_stream(device).wait_stream(torch.cuda.default_stream(device))
            call('sba_set_reduce_scratch', buf.data_ptr(), REDUCE_SCRATCH_BYTES)
        _REDUCE_SCRATCH[device] = buf
    return _REDUCE_SCRATCH[device]


# ---- measured tile table (tools/tune_igemm.py -> sbagan/igemm_table.json) --------------------------------
# key -> [tile, ksplit]: the tile configuration / K split of sba_conv_igemm that was fastest for that layer shape
# on an MI355X (bf16).  Shapes that are not in the table use the library's rule table (tile = 0).
IGEMM_LOG = None            # set to a list to record the geometry of every implicit-GEMM launch (tuning aid)
_IGEMM_TABLE = None


def geom_key(g):
    return '%d_%dx%d_%d_%dx%d_%d_t%d_s%d_u%d' % (g.N, g.IH, g.IW, g.Cin, g.OHs, g.OWs, g.Cout, g.ntaps, g.sy, g.ups)


_TABLE_FILE = None


def _table_section(name):
    global _TABLE_FILE
    if _TABLE_FILE is None:
        _TABLE_FILE = {}
        path = os.environ.get('SBA_IGEMM_TABLE_FILE') or os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                      'igemm_table.json')      # (the override: an A/B aid)
        if os.environ.get('SBA_IGEMM_TABLE', '1') != '0' and os.path.exists(path):
            import json
            with open(path) as f:
                _TABLE_FILE = json.load(f)
    return _TABLE_FILE.get(name, {})


def _igemm_table():
    global _IGEMM_TABLE
    if _IGEMM_TABLE is None:
        _IGEMM_TABLE = _table_section('bf16')
    return _IGEMM_TABLE


def tune_geom(g, dt):
    """Fill g.tile / g.ksplit from the measured table, once per geometry object."""
    if getattr(g, '_tuned', None) != dt:
        g._tuned = dt
        ent = _igemm_table().get(geom_key(g)) if dt == _lib.SBA_BF16 else None
        g.tile, g.ksplit = (int(ent[0]), int(ent[1])) if ent else (0, 0)
    if IGEMM_LOG is not None:
        IGEMM_LOG.append(g)


def _igemm(dt, x, w, y, addend, stats, g, device, w_frag=None):
    """w_frag: the fragment-major copy of `w` (or None): used when the geometry goes to the halo-tile 3 x 3 kernel"""
    ws = workspace(device)
    tune_geom(g, _lib.SBA_BF16 if dt == _lib.SBA_BF16_YH else dt)
    g.w_layout = 0
    if w_frag is not None and _halo_family(g):
        w, g.w_layout = w_frag.data_ptr(), 1
    try:
        call('sba_conv_igemm', dt, x, w, y, addend, stats, ctypes.byref(g), ws.data_ptr(), WORKSPACE_BYTES, _stream())
    finally:
        g.w_layout = 0


def _halo_family(g):
    """does sba_conv_igemm send this (bf16) geometry to the halo-tile 3 x 3 kernel?  (asked once per geometry object)"""
    h = getattr(g, '_halo', None)
    if h is None:
        plan = (ctypes.c_int * 3)()
        old = g.w_layout
        g.w_layout = 0
        call('sba_conv_igemm_plan', _lib.SBA_BF16, ctypes.byref(g), WORKSPACE_BYTES, plan)
        g.w_layout = old
        h = g._halo = plan[0] == 0
    return h


# (Tried at the end of round 4 and removed: the BatchNorm-backward sums of a ResBlock's first BatchNorm taken in the epilogue of
# the second conv's data gradient -- sba_conv_igemm_bnred, commit 6ee6d14.  Correct, but 0.08 ms SLOWER per step when used, and
# the extra state in the epilogue every implicit-GEMM kernel shares cost 0.13 ms even when unused: DESIGN.md §8,
# profiles/r04_ab_fuse_bn_red.txt.)


# ----------------------------------------------------------------------------
# raw (non-autograd) building blocks
# ----------------------------------------------------------------------------
def conv_forward(x, pw, kind, want_stats=True, addend=None, pre_bn=False):
    """y = conv(x) in NHWC; returns (y, stats) with stats = BN_STAT_SLOTS replicas of the per-channel
    (sum, sumsq) pair (add them up; see SBA_BN_STAT_SLOTS in sbagan_hip.h).
    pre_bn: y goes to a BatchNorm and nowhere else -- in the bf16 path it is then a float16 tensor (Y_F16)."""
    _need_gpu(x)
    N, Cin, H, W = x.shape
    O = pw.param.shape[0]
    OH, OW = _conv_out_hw(kind, H, W)
    yh = pre_bn and Y_F16 and x.dtype == torch.bfloat16 and addend is None and O % 8 == 0
    if yh:
        y = torch.empty((N, O, OH, OW), dtype=torch.float16, device=x.device, memory_format=CL)
    else:
        y = empty_act(N, O, OH, OW, x)
    stats = zeros_f32((BN_STAT_SLOTS, 2 * O), x.device) if want_stats else None
    g = _geom((kind, N, H, W, Cin, O, None))
    # (behind the nearest x2 upsample the register-weight kernel measured no faster than the LDS-weight one at four
    #  workgroups per CU -- G3.up 124.5 vs 124.9 us, it is bound by its 335 MB of output -- so '3x3up' keeps row-major weights)
    wf = pw.fwd_frag(x.dtype) if kind == '3x3' else None
    _igemm(_lib.SBA_BF16_YH if yh else _dt(x), _p(x), _p(pw.fwd(x.dtype)), _p(y), _p(addend), _p(stats), g, x.device,
           w_frag=wf)
    return y, stats


def conv_dgrad(dy, pw, kind, in_hw, addend=None):
    """dx = conv_transpose(dy); `addend` (same shape as dx) is added in the epilogue."""
    N, O, OH, OW = dy.shape
    I = pw.param.shape[1]
    H, W = in_hw
    wd = pw.dgrad(dy.dtype, kind)
    if kind == '3x3':
        g = _geom(('3x3', N, OH, OW, O, I, None))
        dx = empty_act(N, I, H, W, dy)
        _igemm(_dt(dy), _p(dy), _p(wd), _p(dx), _p(addend), None, g, dy.device, w_frag=pw.dgrad_frag(dy.dtype, kind))
        return dx
    if kind == '3x3up':
        # every source pixel collects a 4x4 window of dy with the tap sums packed by mode 3: one stride-2
        # conv at the SOURCE resolution instead of a conv at the upsampled resolution + 2x2 sum pooling
        g = _geom(('4x4s2', N, OH, OW, O, I, None))
        dx = empty_act(N, I, H, W, dy)
        _igemm(_dt(dy), _p(dy), _p(wd), _p(dx), _p(addend), None, g, dy.device)
        return dx
    if kind == '4x4s2':
        dx = empty_act(N, I, H, W, dy)
        esz = dy.element_size()
        gs = [_geom(('4x4s2_dgrad', N, OH, OW, O, I, (cls // 2, cls % 2))) for cls in range(4)]
        if DGRAD4_GROUP and dy.dtype == torch.bfloat16 and O % 64 == 0:
            # the four parity classes read the same dy and write disjoint pixels of dx: ONE grid (4x the workgroups of a
            # class, one launch floor, one tail) instead of four launches of 80..640 workgroups
            arr = (_lib.ConvGroupItem * 4)()
            for cls, (a, g) in enumerate(zip(arr, gs)):
                a.x, a.w, a.y, a.addend = _p(dy), wd.data_ptr() + cls * I * 4 * O * esz, _p(dx), _p(addend)
                a.bias = a.relu_mask = None
                a.g = ctypes.pointer(g)
            tile, split = dgrad4_plan(gs[0])
            ws = workspace(dy.device)
            call('sba_conv_igemm_group_splitk', _lib.SBA_BF16, 4, arr, tile, split, ws.data_ptr(), WORKSPACE_BYTES, _stream())
            if IGEMM_LOG is not None:
                IGEMM_LOG.append(('group', tile, gs))
            return dx
        for cls in range(4):
            wptr = wd.data_ptr() + cls * I * 4 * O * esz
            _igemm(_dt(dy), _p(dy), wptr, _p(dx), _p(addend), None, gs[cls], dy.device)
        return dx
    raise ValueError(kind)


DGRAD4_GROUP = True         # False: four single launches (the reference of tests/test_kernels_gpu.py, tools/tune_dgrad4.py)
_DGRAD4_FORCE = None        # "tile,split": forces the grouped launch's plan (tests and tools/tune_dgrad4.py)


def dgrad4_plan(g):
    """(tile id, K splits) of the grouped launch of the four parity classes of a 4x4/s2 data gradient: from the measured
    table (igemm_table.json, section 'dgrad4'; tools/tune_dgrad4.py) or by rule -- the biggest tile that still gives
    two workgroups per CU, then K splits up to that occupancy while a split keeps >= 8 slabs of 64 channels."""
    if _DGRAD4_FORCE:
        t, s = _DGRAD4_FORCE.split(',')
        return int(t), int(s)
    ent = _table_section('dgrad4').get(geom_key(g))
    if ent:
        return int(ent[0]), int(ent[1])
    M = g.N * g.OHs * g.OWs
    ny = (g.Cout + 63) // 64
    for tile, bm in ((5, 128), (3, 96), (1, 64)):
        tiles = 4 * ((M + bm - 1) // bm) * ny
        if tiles >= 512 or tile == 1:
            break
    ns64 = g.ntaps * (g.Cin // 64)
    split = max(1, min(512 // max(tiles, 1), ns64 // 8))
    return tile, split


_KSPLIT_TARGET = 640
_KSPLIT_MIN_CHUNKS = 24


def _ksplit(tiles, M):
    chunks = (M + 63) // 64
    want = max(1, (_KSPLIT_TARGET + tiles - 1) // tiles)       # ~2.5 workgroups per CU ...
    # ... but every split adds a full copy of the tile's outputs to the f32 atomics: keep >= 24 pixel
    # chunks (1536 pixels) of MFMA work per workgroup behind each copy
    return max(1, min(want, chunks // _KSPLIT_MIN_CHUNKS if chunks >= 2 * _KSPLIT_MIN_CHUNKS else 1))


def conv_wgrad(x, dy, param, kind):
    """param.grad[O][KH][KW][I] += dy^T (*) x."""
    N, Cin, H, W = x.shape
    O = dy.shape[1]
    g = _geom((kind, N, H, W, Cin, O, None))
    gbuf = param_grad(param)
    M = N * g.OHs * g.OWs
    tiles = ((O + 63) // 64) * ((Cin + 63) // 64) * g.ntaps
    # first weight gradient of this parameter since its flat gradient buffer was cleared (trainer.FlatParams.zero_grad
    # bumps the cell): the kernel may store instead of read-modify-write.  Parameters outside a FlatParams never
    # qualify (somebody else owns their .grad).
    cell = getattr(param, '_sba_gepoch', None)
    first = 0
    if cell is not None and getattr(param, '_sba_wepoch', None) != cell[0]:
        param._sba_wepoch = cell[0]
        first = 1
    g.first_write = first
    call('sba_conv_wgrad', _dt(x), _p(x), _p(dy), _p(gbuf), ctypes.byref(g), _ksplit(tiles, M), _stream())


# ---- weight gradients on a companion stream ---------------------------------------------
# dW = dy^T (*) x and dx = conv^T(dy) of one layer are independent; with SIDE_WGRAD enabled the
# weight-gradient launch goes to a companion of the current stream so that it overlaps the
# data-gradient chain (the critical path of a backward pass).  The trainer joins the companions
# before the optimizer reads the gradients; tensors handed to the companion are kept alive until
# that join (no record_stream: safe under hipGraph capture).
SIDE_WGRAD = False
HOME_STREAM = None       # raw handle of the stream whose companion join_wgrads() will join (set by the trainer at the start of
#                          a backward pass): the dense layers use the companion only from there -- their backward may be
#                          replayed on a side stream (the mapping network's), whose companion nobody would join
_COMPANION, _KEEPALIVE, _COMP_NEXT = {}, {}, {}
N_COMPANIONS = int(os.environ.get('SBA_WGRAD_COMPANIONS', '1'))      # companion streams per stream, used in turn


def _companion(device, *keep):
    """the companion of the current stream, ordered behind everything issued to the current stream so far; `keep` =
    tensors the companion's launches read (held until the join)"""
    cur = torch.cuda.current_stream()
    key = cur.cuda_stream
    comps = _COMPANION.get(key)
    if comps is None:
        comps = _COMPANION[key] = [torch.cuda.Stream(device=device) for _ in range(N_COMPANIONS)]
        _KEEPALIVE[key] = []
        _COMP_NEXT[key] = 0
    comp = comps[_COMP_NEXT[key] % len(comps)]
    _COMP_NEXT[key] += 1
    comp.wait_stream(cur)
    _KEEPALIVE[key].extend(keep)
    return comp


def conv_wgrad_overlapped(x, dy, param, kind):
    if not SIDE_WGRAD:
        return conv_wgrad(x, dy, param, kind)
    param_grad(param)                     # allocate (if needed) on the caller's stream
    with torch.cuda.stream(_companion(x.device, x, dy)):
        conv_wgrad(x, dy, param, kind)


def join_wgrads():
    """Make the current stream wait for the weight gradients issued from it."""
    cur = torch.cuda.current_stream()
    comps = _COMPANION.get(cur.cuda_stream)
    if comps is not None:
        for comp in comps:
            cur.wait_stream(comp)
        _KEEPALIVE[cur.cuda_stream].clear()
        _COMP_NEXT[cur.cuda_stream] = 0


def wgrad_tail_stream():
    """One-way variant of join_wgrads for a stream that is itself a fork: returns the stream on
    which the rest of the update (all-reduce, Adam) must be issued -- the companion, ordered
    after everything the current stream has done -- instead of joining the companion back.
    hipStreamEndCapture (ROCm 7.2) crashes on a fork -> sub-fork -> join-into-the-fork round
    trip, while one-way edges that only re-join the capture's origin stream are fine
    (tools/debug_nested.py)."""
    cur = torch.cuda.current_stream()
    comps = _COMPANION.get(cur.cuda_stream)
    if comps is None:
        return cur
    comp = comps[0]
    comp.wait_stream(cur)
    for other in comps[1:]:
        comp.wait_stream(other)
    _KEEPALIVE[cur.cuda_stream].clear()
    _COMP_NEXT[cur.cuda_stream] = 0
    return comp


BN_STAT_SLOTS = _lib.lib.sba_bn_stat_slots()      # the replica count the library was COMPILED with (its kernels index
#                                                   the statistics buffers with it; include/sbagan_hip.h)


# ---- deterministic-reduction mode (include/sbagan_hip.h: sba_set_deterministic) ------------------------------
_DET_SCRATCH = [None]
DET_SCRATCH_BYTES = int(os.environ.get('SBA_DET_SCRATCH_MB', '2048')) << 20


def set_deterministic(flag, device=None):
    """Turn the library's deterministic-reduction mode on / off: with it on, two runs of the same launches on the
    same inputs are bit-identical in every launch mode (eager, hipGraph, native replayer).  Allocates the scratch
    ring the ordered reductions use (SBA_DET_SCRATCH_MB, default 2 GiB).  Call while the device is idle."""
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    if flag:
        dev = torch.device('cuda', torch.cuda.current_device()) if device is None else device
        if _DET_SCRATCH[0] is None or _DET_SCRATCH[0].device != dev:
            _DET_SCRATCH[0] = torch.empty(DET_SCRATCH_BYTES, dtype=torch.uint8, device=dev)
        call('sba_set_deterministic', 1, _DET_SCRATCH[0].data_ptr(), DET_SCRATCH_BYTES)
    else:
        call('sba_set_deterministic', 0, None, 0)


def deterministic():
    return bool(_lib.lib.sba_get_deterministic())


def det_reset():
    """Rewind the scratch ring of the deterministic mode (start of a step / before a capture)."""
    if _lib.lib.sba_get_deterministic():
        call('sba_det_reset')


if os.environ.get('SBA_DETERMINISTIC', '0') == '1' and torch.cuda.is_available():
    set_deterministic(True)


class BNState(object):
    """per-forward BatchNorm quantities: aux[g] = (scale, shift, mean, rstd) of group g."""
    __slots__ = ('aux', 'C', 'rows', 'groups')


def bn_act_forward(y, stats, bn, act, residual=None, groups=1):
    """BatchNorm (train: batch statistics `stats` = per-group (sum, sumsq); eval: running stats) +
    activation (+ residual) in ONE launch for all `groups` BatchNorm batches of y; returns (out, state)."""
    N, C, H, W = y.shape
    Co = C // 2 if act == ACT_GLU else C
    st = BNState()
    st.C, st.rows, st.groups = C, (N // groups) * H * W, groups
    st.aux = torch.empty((groups, 4, C), dtype=torch.float32, device=y.device)
    out = torch.empty((N, Co, H, W), dtype=_act_dtype(y), device=y.device, memory_format=CL)
    call('sba_bn_act_fwd', _dt(y), _p(y), _p(stats), _p(bn.weight), _p(bn.bias), _p(bn.running_mean),
         _p(bn.running_var), _p(bn.num_batches_tracked), _p(st.aux), _p(residual), _p(out), st.rows, groups, C,
         act, Co, 0, BN_EPS, BN_MOMENTUM, 1 if bn.training else 0, _stream())
    return out, st


BN_FUSED_BWD_ROWS = 2560        # rows per group up to which the one-launch forward (grouped maps) and backward are used


def bn_act_backward(y, dout, st, bn, act, need_param_grad=True, out=None, red=None):
    """red: the two backward sums when the caller has them already"""
    N, C, H, W = y.shape
    Co = C // 2 if act == ACT_GLU else C
    dy = out if out is not None else torch.empty(y.shape, dtype=_act_dtype(y), device=y.device, memory_format=CL)
    dg = db = None
    if need_param_grad:
        dg, db = param_grad(bn.weight), param_grad(bn.bias)
    if st.rows <= BN_FUSED_BWD_ROWS:
        call('sba_bn_act_bwd_fused', _dt(y), _p(y), _p(dout), _p(st.aux), _p(dy), _p(dg), _p(db), st.rows, st.groups,
             C, act, Co, 0, _stream())
        return dy
    if red is None:
        red = zeros_f32((st.groups, BN_STAT_SLOTS, 2 * C), y.device)
        call('sba_bn_act_bwd_reduce', _dt(y), _p(y), _p(dout), _p(st.aux), _p(red), st.rows, st.groups, C, act, Co, 0,
             _stream())
    call('sba_bn_act_bwd_apply', _dt(y), _p(y), _p(dout), _p(st.aux), _p(red), _p(dy), _p(dg), _p(db), st.rows,
         st.groups, C, act, Co, 0, _stream())
    return dy


def bn_act_forward_fused(y, bn, act, groups):
    """training-mode BatchNorm + activation of a small grouped map: statistics, finalize and normalise in one launch"""
    N, C, H, W = y.shape
    Co = C // 2 if act == ACT_GLU else C
    st = BNState()
    st.C, st.rows, st.groups = C, (N // groups) * H * W, groups
    st.aux = torch.empty((groups, 4, C), dtype=torch.float32, device=y.device)
    out = torch.empty((N, Co, H, W), dtype=_act_dtype(y), device=y.device, memory_format=CL)
    call('sba_bn_act_fwd_fused', _dt(y), _p(y), _p(bn.weight), _p(bn.bias), _p(bn.running_mean), _p(bn.running_var),
         _p(bn.num_batches_tracked), _p(st.aux), _p(out), st.rows, groups, C, act, Co, 0, BN_EPS, BN_MOMENTUM, _stream())
    return out, st


def bn_stats(y, groups=1):
    """per-group, per-channel (sum, sumsq) of an NHWC tensor by a separate pass (grouped batches)."""
    N, C, H, W = y.shape
    stats = zeros_f32((groups, BN_STAT_SLOTS, 2 * C), y.device)
    call('sba_bn_stats', _dt(y), _p(y), _p(stats), (N // groups) * H * W, groups, C, _stream())
    return stats


def bn_act_forward_grouped(y, bn, act, groups):
    """BatchNorm + activation of a conv output that came without statistics (`groups` BatchNorm batches back to back):
    a small map in training mode takes the one-launch kernel, everything else a statistics pass + bn_act_forward."""
    N, C, H, W = y.shape
    if bn.training and (N // groups) * H * W <= BN_FUSED_BWD_ROWS:
        return bn_act_forward_fused(y, bn, act, groups)
    stats = bn_stats(y, groups) if bn.training else None
    return bn_act_forward(y, stats, bn, act, None, groups)


# ----------------------------------------------------------------------------
# autograd Functions
# ----------------------------------------------------------------------------
def _c(t):
    """gradient tensors arrive with arbitrary strides: force the NHWC layout."""
    if t.dim() == 4:
        return t.contiguous(memory_format=CL)
    return t.contiguous()


class ConvBNActFn(torch.autograd.Function):
    """conv (3x3 / nearest-x2 + 3x3 / 4x4 s2) -> BatchNorm(train) -> GLU | LeakyReLU | none (+ residual).
    upBlock model.py:39-45, Block3x3_leakRelu :540-546, downBlock :550-556, ResBlock halves :60-65.

    groups > 1: the batch holds `groups` independent BatchNorm batches back to back (the
    discriminator's real | fake passes, losses.py:139-140): ONE conv / dgrad / wgrad launch over
    the whole batch, BatchNorm statistics, running-stat updates and normalisation per group in
    order -- bit-for-bit the same module state as calling the block once per group."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, layer, kind, act, residual, groups=1):
        x = as_act(x)
        if groups == 1:
            y, stats = conv_forward(x, layer.pw, kind, want_stats=layer.bn.training, pre_bn=True)
            out, sts = bn_act_forward(y, stats, layer.bn, act, residual)
        else:
            assert residual is None and x.shape[0] % groups == 0
            y, _ = conv_forward(x, layer.pw, kind, want_stats=False, pre_bn=True)
            out, sts = bn_act_forward_grouped(y, layer.bn, act, groups)
        ctx.layer, ctx.kind, ctx.act, ctx.sts, ctx.groups = layer, kind, act, sts, groups
        ctx.has_res = residual is not None
        ctx.save_for_backward(x, y)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, y = ctx.saved_tensors
        layer, kind, act, groups = ctx.layer, ctx.kind, ctx.act, ctx.groups
        dout = _c(dout)
        dy = bn_act_backward(y, dout, ctx.sts, layer.bn, act, ctx.needs_input_grad[2])
        if ctx.needs_input_grad[1]:
            conv_wgrad_overlapped(x, dy, layer.conv.weight, kind)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = conv_dgrad(dy, layer.pw, kind, x.shape[2:])
        dres = dout if (ctx.has_res and ctx.needs_input_grad[7]) else None
        return dx, None, None, None, None, None, None, dres, None


class ResBlockFn(torch.autograd.Function):
    """ResBlock (model.py:57-71) as one node so that the skip gradient is added in the
    epilogue of the first conv's data-gradient instead of a separate pass."""

    @staticmethod
    def forward(ctx, x, w1, g1, b1, w2, g2, b2, blk):
        x = as_act(x)
        y1, s1 = conv_forward(x, blk.l1.pw, '3x3', want_stats=blk.l1.bn.training, pre_bn=True)
        a1, st1 = bn_act_forward(y1, s1, blk.l1.bn, ACT_GLU)
        y2, s2 = conv_forward(a1, blk.l2.pw, '3x3', want_stats=blk.l2.bn.training, pre_bn=True)
        out, st2 = bn_act_forward(y2, s2, blk.l2.bn, ACT_NONE, residual=x)
        ctx.blk, ctx.st1, ctx.st2 = blk, st1, st2
        ctx.save_for_backward(x, y1, a1, y2)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, y1, a1, y2 = ctx.saved_tensors
        blk = ctx.blk
        dout = _c(dout)
        need_p = ctx.needs_input_grad[1]
        dy2 = bn_act_backward(y2, dout, ctx.st2, blk.l2.bn, ACT_NONE, need_p)
        if need_p:
            conv_wgrad_overlapped(a1, dy2, blk.l2.conv.weight, '3x3')
        da1 = conv_dgrad(dy2, blk.l2.pw, '3x3', a1.shape[2:])
        dy1 = bn_act_backward(y1, da1, ctx.st1, blk.l1.bn, ACT_GLU, need_p)
        if need_p:
            conv_wgrad_overlapped(x, dy1, blk.l1.conv.weight, '3x3')
        dx = None
        if ctx.needs_input_grad[0]:
            dx = conv_dgrad(dy1, blk.l1.pw, '3x3', x.shape[2:], addend=dout)
        return dx, None, None, None, None, None, None, None


class LinearFn(torch.autograd.Function):
    """f32 dense layer y = x W^T + b (nn.Linear; model.py:278,306-313,330,354)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        _need_gpu(x)
        x = x.float().contiguous()
        B, K = x.shape
        N = weight.shape[0]
        y = torch.empty((B, N), dtype=torch.float32, device=x.device)
        call('sba_linear_fwd', _p(x), _p(weight), _p(bias), _p(y), B, K, N, _stream())
        ctx.save_for_backward(x, weight)
        ctx.bias = bias
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = dy.float().contiguous()
        B, K = x.shape
        N = weight.shape[0]
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw = param_grad(weight) if ctx.needs_input_grad[1] else None
        db = param_grad(ctx.bias) if (ctx.bias is not None and ctx.needs_input_grad[2]) else None
        if SIDE_WGRAD and HOME_STREAM == _stream() and dx is not None and dw is not None:
            # the chain of dense layers at the END of the generator's backward pass (MAPPING_NET, INIT_STAGE_G.fc,
            # CA_NET.fc): only dx continues the chain -- dW / db go to the weight-gradient companion stream
            with torch.cuda.stream(_companion(x.device, x, dy)):
                call('sba_linear_bwd', _p(x), _p(weight), _p(dy), None, _p(dw), _p(db), B, K, N, _stream())
            call('sba_linear_bwd', _p(x), _p(weight), _p(dy), _p(dx), None, None, B, K, N, _stream())
        else:
            call('sba_linear_bwd', _p(x), _p(weight), _p(dy), _p(dx), _p(dw), _p(db), B, K, N, _stream())
        return dx, None, None


class CAFn(torch.autograd.Function):
    """CA_NET tail: GLU, split, reparametrise with an explicit eps (model.py:281-294)."""

    @staticmethod
    def forward(ctx, h, eps):
        B, C4 = h.shape
        C = C4 // 4
        h = h.contiguous()
        eps = eps.float().contiguous()
        c, mu, lv = (torch.empty((B, C), dtype=torch.float32, device=h.device) for _ in range(3))
        call('sba_ca_fwd', _p(h), _p(eps), _p(c), _p(mu), _p(lv), B, C, _stream())
        ctx.save_for_backward(h, eps)
        return c, mu, lv

    @staticmethod
    def backward(ctx, dc, dmu, dlv):
        h, eps = ctx.saved_tensors
        B, C4 = h.shape
        dh = torch.empty_like(h)
        dc = None if dc is None else dc.contiguous()
        dmu = None if dmu is None else dmu.contiguous()
        dlv = None if dlv is None else dlv.contiguous()
        call('sba_ca_bwd', _p(h), _p(eps), _p(dc), _p(dmu), _p(dlv), _p(dh), B, C4 // 4, _stream())
        return dh, None


class FcBnGluFn(torch.autograd.Function):
    """INIT_STAGE_G.fc: Linear(no bias) -> BatchNorm1d(train) -> GLU -> view(B, ngf, 4, 4)
    (model.py:353-356,372-373); the output is written NHWC."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, mod):
        _need_gpu(x)
        x = x.float().contiguous()
        B, K = x.shape
        F = weight.shape[0]
        y = torch.empty((B, F), dtype=torch.float32, device=x.device)
        call('sba_linear_fwd', _p(x), _p(weight), None, _p(y), B, K, F, _stream())
        bn = mod.bn
        aux = torch.empty((2, F), dtype=torch.float32, device=x.device)
        out = torch.empty((B, F // 32, 4, 4), dtype=COMPUTE_DTYPE, device=x.device, memory_format=CL)
        if not bn.training:
            # inference (netG.eval(): trainer.py:368 sampling / :437 gen_example): running statistics, plain
            # tensor ops -- this layer runs once per generated batch and is off the training path (nets._FcBnGlu
            # refuses the call when a gradient could be asked of it)
            yn = (y - bn.running_mean) * torch.rsqrt(bn.running_var + BN_EPS) * bn.weight + bn.bias
            glu = yn[:, :F // 2] * torch.sigmoid(yn[:, F // 2:])
            return glu.view(B, F // 32, 4, 4).to(COMPUTE_DTYPE).contiguous(memory_format=CL)
        call('sba_bn1d_glu_fwd', _dt(out), _p(y), _p(bn.weight), _p(bn.bias), _p(bn.running_mean),
             _p(bn.running_var), _p(bn.num_batches_tracked), _p(aux[0]), _p(aux[1]), _p(out), B, F, BN_EPS,
             BN_MOMENTUM, _stream())
        ctx.mod, ctx.aux = mod, aux
        ctx.save_for_backward(x, y, weight)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, y, weight = ctx.saved_tensors
        bn = ctx.mod.bn
        dout = _c(dout)
        B, K = x.shape
        F = weight.shape[0]
        dy = torch.empty_like(y)
        call('sba_bn1d_glu_bwd', _dt(dout), _p(y), _p(dout), _p(bn.weight), _p(bn.bias), _p(ctx.aux[0]),
             _p(ctx.aux[1]), _p(dy), _p(param_grad(bn.weight)), _p(param_grad(bn.bias)), B, F, _stream())
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw = param_grad(weight)
        if SIDE_WGRAD and HOME_STREAM == _stream() and dx is not None:       # (as LinearFn: beside the rest of the chain)
            with torch.cuda.stream(_companion(x.device, x, dy)):
                call('sba_linear_bwd', _p(x), _p(weight), _p(dy), None, _p(dw), None, B, K, F, _stream())
            call('sba_linear_bwd', _p(x), _p(weight), _p(dy), _p(dx), None, None, B, K, F, _stream())
        else:
            call('sba_linear_bwd', _p(x), _p(weight), _p(dy), _p(dx), _p(dw), None, B, K, F, _stream())
        return dx, None, None, None, None


# BASELINE config 5 ("fp8 MFMA for the attention / context GEMM"): the attention key projection (GlobalAttention.py:97
# conv_context) AND the two attention contractions (GlobalAttention.py:103 scores, :117 context) with FP8 (OCP e4m3)
# operands on v_mfma_f32_32x32x16_fp8_fp8 (forward only; the backward keeps bf16 / f32 operands).  Off by default.
ATTN_FP8 = os.environ.get('SBA_ATTN_FP8', '0') == '1'


def set_attention_fp8(flag):
    global ATTN_FP8
    ATTN_FP8 = bool(flag)


def _ctx_proj_fwd(words, wc, src, N, C, cdf, L):
    if ATTN_FP8 and cdf % 16 == 0:
        call('sba_ctx_proj_fwd_fp8', _p(words), _p(wc), _p(src), N, C, cdf, L, _stream())
    else:
        call('sba_ctx_proj_fwd', _p(words), _p(wc), _p(src), N, C, cdf, L, _stream())


def _word_attn_fwd(h, src, m8, out, att, N, HW, C, L, mask_mode, ocs, oco):
    if ATTN_FP8 and h.dtype == torch.bfloat16 and C in (32, 64):
        call('sba_word_attn_fwd_fp8', _p(h), _p(src), _p(m8), _p(out), _p(att), N, HW, C, L, mask_mode, ocs, oco,
             _stream())
    else:
        call('sba_word_attn_fwd', _dt(h), _p(h), _p(src), _p(m8), _p(out), _p(att), N, HW, C, L, mask_mode, ocs, oco,
             _stream())


def _mask_u8(mask):
    if mask is None:
        return None
    if mask.dtype == torch.bool and mask.is_contiguous():
        return mask.view(torch.uint8)       # the same bytes (False / True are stored as 0 / 1): no conversion launch
    # (a sliced mask -- trainer.py:253-256 cuts it to the longest caption -- is not contiguous.)  Both later stages of the
    # generator pass the SAME mask object: convert it once per generator forward (the cache is cleared at the start of every
    # forward, nets._GBase._run -- a recording must hold its own conversion launch, the caller refills a static mask between
    # replays) and per content (tensor identity + version counter)
    global _MASK_U8_CACHE
    c = _MASK_U8_CACHE
    if c is not None and c[0]() is mask and c[1] == mask._version and c[2].device == mask.device:
        return c[2]
    import weakref
    u8 = mask.to(torch.uint8).contiguous()
    try:
        _MASK_U8_CACHE = (weakref.ref(mask), mask._version, u8)
    except TypeError:
        _MASK_U8_CACHE = None
    return u8


_MASK_U8_CACHE = None


def reset_mask_cache():
    global _MASK_U8_CACHE
    _MASK_U8_CACHE = None


class CtxProjFn(torch.autograd.Function):
    """conv_context of GlobalAttentionGeneral (GlobalAttention.py:75,97) as a node of its own: src[b] = W words[b] depends on
    the captions and the weight only, so the generator evaluates it beside its first stage (nets._GBase._styles) and hands
    it to AttnAdainCatFn; autograd replays this node's backward on the stream of its forward."""

    @staticmethod
    def forward(ctx, words, w_ctx):
        words = words.float().contiguous()
        N, cdf, L = words.shape
        C = w_ctx.shape[0]
        src = torch.empty((N, C, L), dtype=torch.float32, device=words.device)
        _ctx_proj_fwd(words, w_ctx.detach().reshape(C, cdf), src, N, C, cdf, L)
        ctx.save_for_backward(words)
        ctx.w_ctx = w_ctx
        return src

    @staticmethod
    def backward(ctx, dsrc):
        (words,) = ctx.saved_tensors
        dsrc = dsrc.float().contiguous()
        N, cdf, L = words.shape
        C = ctx.w_ctx.shape[0]
        dwords = torch.empty_like(words) if ctx.needs_input_grad[0] else None
        wc = ctx.w_ctx.detach().reshape(C, cdf)
        if ctx.needs_input_grad[1] or dwords is not None:
            dW = param_grad(ctx.w_ctx) if ctx.needs_input_grad[1] else torch.zeros_like(wc)
            call('sba_ctx_proj_bwd', _p(words), _p(wc), _p(dsrc), _p(dW), _p(dwords), N, C, cdf, L, _stream())
        return dwords, None


class AttnAdainCatFn(torch.autograd.Function):
    """Entry of NEXT_STAGE_G (model.py:415-418): word attention (GlobalAttention.py:82-121),
    AdaIN (model.py:332-339) and the channel concat, written straight into one NHWC
    tensor [adain(h) | ctx].  Returns (h_c_code, att or empty)."""

    @staticmethod
    def forward(ctx, h, style, words, w_ctx, mask, want_att, mask_mode, src_in=None):
        """src_in: the key projection when the caller has evaluated it already (CtxProjFn): its gradient is then returned
        instead of being folded into dW / dwords here"""
        h = as_act(h)
        N, C, H, W = h.shape
        HW = H * W
        words = words.float().contiguous()
        cdf, L = words.shape[1], words.shape[2]
        style = style.float().contiguous()
        m8 = _mask_u8(mask)
        dev = h.device
        ctx.src_given = src_in is not None
        if src_in is not None:
            src = src_in.float().contiguous()
        else:
            src = torch.empty((N, C, L), dtype=torch.float32, device=dev)
            wc = w_ctx.detach().reshape(C, cdf)
            _ctx_proj_fwd(words, wc, src, N, C, cdf, L)
        out = empty_act(N, 2 * C, H, W, h)
        att = torch.empty((N, L, H, W), dtype=torch.float32, device=dev) if want_att else None
        _word_attn_fwd(h, src, m8, out, att, N, HW, C, L, mask_mode, 2 * C, C)
        mr = torch.empty((2, N, C), dtype=torch.float32, device=dev)
        call('sba_instnorm_stats', _dt(h), _p(h), _p(mr[0]), _p(mr[1]), N, HW, C, IN_EPS, _stream())
        call('sba_adain_fwd', _dt(h), _p(h), _p(mr[0]), _p(mr[1]), _p(style), _p(out), N, HW, C, 2 * C, 0,
             _stream())
        ctx.save_for_backward(h, style, words, src, mr)
        ctx.m8, ctx.w_ctx, ctx.mask_mode = m8, w_ctx, mask_mode
        if att is None:
            att = torch.empty(0, device=dev)
        ctx.mark_non_differentiable(att)
        return out, att

    @staticmethod
    def backward(ctx, dout, _datt):
        h, style, words, src, mr = ctx.saved_tensors
        dout = _c(dout)
        N, C, H, W = h.shape
        HW = H * W
        cdf, L = words.shape[1], words.shape[2]
        dev = h.device
        dh = torch.empty_like(h)
        dsrc = zeros_f32((N, C, L), dev)
        call('sba_word_attn_bwd', _dt(h), _p(h), _p(src), _p(ctx.m8), _p(dout), _p(dh), _p(dsrc), N, HW, C, L,
             ctx.mask_mode, 2 * C, C, 0, _stream())
        red = zeros_f32((N, C, 2), dev)
        call('sba_adain_bwd_reduce', _dt(h), _p(h), _p(dout), _p(mr[0]), _p(mr[1]), _p(red), N, HW, C, 2 * C, 0,
             _stream())
        dstyle = torch.empty_like(style)
        call('sba_adain_bwd_apply', _dt(h), _p(h), _p(dout), _p(mr[0]), _p(mr[1]), _p(style), _p(red), _p(dh),
             _p(dstyle), N, HW, C, 2 * C, 0, 1, _stream())
        if ctx.src_given:
            return dh, dstyle, None, None, None, None, None, dsrc
        dwords = torch.empty_like(words) if ctx.needs_input_grad[2] else None
        wc = ctx.w_ctx.detach().reshape(C, cdf)
        if ctx.needs_input_grad[3] or dwords is not None:
            dW = param_grad(ctx.w_ctx) if ctx.needs_input_grad[3] else torch.zeros_like(wc)
            call('sba_ctx_proj_bwd', _p(words), _p(wc), _p(dsrc), _p(dW), _p(dwords), N, C, cdf, L, _stream())
        return dh, dstyle, dwords, None, None, None, None, None


class WordAttnFn(torch.autograd.Function):
    """Stand-alone GlobalAttentionGeneral.forward (GlobalAttention.py:82-121)."""

    @staticmethod
    def forward(ctx, h, words, w_ctx, mask, mask_mode):
        h = as_act(h)
        N, C, H, W = h.shape
        words = words.float().contiguous()
        cdf, L = words.shape[1], words.shape[2]
        m8 = _mask_u8(mask)
        src = torch.empty((N, C, L), dtype=torch.float32, device=h.device)
        wc = w_ctx.detach().reshape(C, cdf)
        _ctx_proj_fwd(words, wc, src, N, C, cdf, L)
        out = empty_act(N, C, H, W, h)
        att = torch.empty((N, L, H, W), dtype=torch.float32, device=h.device)
        _word_attn_fwd(h, src, m8, out, att, N, H * W, C, L, mask_mode, C, 0)
        ctx.save_for_backward(h, words, src)
        ctx.m8, ctx.w_ctx, ctx.mask_mode = m8, w_ctx, mask_mode
        ctx.mark_non_differentiable(att)
        return out, att

    @staticmethod
    def backward(ctx, dout, _datt):
        h, words, src = ctx.saved_tensors
        dout = _c(dout)
        N, C, H, W = h.shape
        cdf, L = words.shape[1], words.shape[2]
        dh = torch.empty_like(h)
        dsrc = torch.zeros((N, C, L), dtype=torch.float32, device=h.device)
        call('sba_word_attn_bwd', _dt(h), _p(h), _p(src), _p(ctx.m8), _p(dout), _p(dh), _p(dsrc), N, H * W, C, L,
             ctx.mask_mode, C, 0, 0, _stream())
        dwords = torch.empty_like(words) if ctx.needs_input_grad[1] else None
        wc = ctx.w_ctx.detach().reshape(C, cdf)
        dW = param_grad(ctx.w_ctx) if ctx.needs_input_grad[2] else torch.zeros_like(wc)
        call('sba_ctx_proj_bwd', _p(words), _p(wc), _p(dsrc), _p(dW), _p(dwords), N, C, cdf, L, _stream())
        return dh, dwords, None, None, None


class AdainFn(torch.autograd.Function):
    """Stand-alone ADAIN_NORM core (model.py:336-337) given style = Linear(w)."""

    @staticmethod
    def forward(ctx, h, style):
        h = as_act(h)
        N, C, H, W = h.shape
        style = style.float().contiguous()
        mr = torch.empty((2, N, C), dtype=torch.float32, device=h.device)
        call('sba_instnorm_stats', _dt(h), _p(h), _p(mr[0]), _p(mr[1]), N, H * W, C, IN_EPS, _stream())
        out = torch.empty_like(h)
        call('sba_adain_fwd', _dt(h), _p(h), _p(mr[0]), _p(mr[1]), _p(style), _p(out), N, H * W, C, C, 0, _stream())
        ctx.save_for_backward(h, style, mr)
        return out

    @staticmethod
    def backward(ctx, dout):
        h, style, mr = ctx.saved_tensors
        dout = _c(dout)
        N, C, H, W = h.shape
        red = torch.zeros((N, C, 2), dtype=torch.float32, device=h.device)
        call('sba_adain_bwd_reduce', _dt(h), _p(h), _p(dout), _p(mr[0]), _p(mr[1]), _p(red), N, H * W, C, C, 0,
             _stream())
        dh = torch.empty_like(h)
        dstyle = torch.empty_like(style)
        call('sba_adain_bwd_apply', _dt(h), _p(h), _p(dout), _p(mr[0]), _p(mr[1]), _p(style), _p(red), _p(dh),
             _p(dstyle), N, H * W, C, C, 0, 0, _stream())
        return dh, dstyle


class ImgHeadFn(torch.autograd.Function):
    """GET_IMAGE_G: conv3x3(ngf->3) + tanh, NHWC features -> NCHW f32 image (model.py:426-437)."""

    @staticmethod
    def forward(ctx, h, weight):
        h = as_act(h)
        reduce_scratch(h.device)         # (allocated here, outside any later graph capture of the backward)
        N, C, H, W = h.shape
        if not weight.is_contiguous(memory_format=CL):
            raise RuntimeError('img head weight must be channels_last')
        img = torch.empty((N, 3, H, W), dtype=torch.float32, device=h.device)
        call('sba_img_head_fwd', _dt(h), _p(h), _p(weight), _p(img), N, H, W, C, _stream())
        ctx.save_for_backward(h, weight, img)
        return img

    @staticmethod
    def backward(ctx, dimg):
        h, weight, img = ctx.saved_tensors
        dimg = dimg.float().contiguous()
        N, C, H, W = h.shape
        dh = torch.empty_like(h)
        dw = param_grad(weight) if ctx.needs_input_grad[1] else torch.zeros_like(weight)
        call('sba_img_head_bwd', _dt(h), _p(h), _p(weight), _p(img), _p(dimg), _p(dh), _p(dw), N, H, W, C, 0,
             _stream())
        return dh, None


class DStemFn(torch.autograd.Function):
    """conv4x4 s2 (3->ndf) + LeakyReLU(0.2): NCHW f32 image -> NHWC features (model.py:563-564)."""

    @staticmethod
    def forward(ctx, img, weight):
        _need_gpu(img)
        reduce_scratch(img.device)       # (allocated here, outside any later graph capture of the backward)
        img = img.float().contiguous()
        N, _, S, S2 = img.shape
        assert S == S2
        C = weight.shape[0]
        out = torch.empty((N, C, S // 2, S // 2), dtype=COMPUTE_DTYPE, device=img.device, memory_format=CL)
        call('sba_d_stem_fwd', _dt(out), _p(img), _p(weight), _p(out), N, S, C, _stream())
        ctx.save_for_backward(img, weight, out)
        return out

    @staticmethod
    def backward(ctx, dout):
        img, weight, out = ctx.saved_tensors
        dout = _c(dout)
        N, _, S, _ = img.shape
        C = weight.shape[0]
        dimg = torch.empty_like(img) if ctx.needs_input_grad[0] else None
        dw = param_grad(weight) if ctx.needs_input_grad[1] else None
        if dimg is not None or dw is not None:
            call('sba_d_stem_bwd', _dt(out), _p(img), _p(weight), _p(out), _p(dout), _p(dimg), _p(dw), N, S, C,
                 _stream())
        return dimg, None


class LogitsFn(torch.autograd.Function):
    """outlogits: conv4x4 s4 (8ndf->1, bias) + sigmoid on the 4x4 map (model.py:590-592,606-607)."""

    @staticmethod
    def forward(ctx, h, weight, bias):
        h = as_act(h)
        B, C, H, W = h.shape
        assert H == 4 and W == 4
        prob = torch.empty(B, dtype=torch.float32, device=h.device)
        call('sba_logits_fwd', _dt(h), _p(h), _p(weight), _p(bias), _p(prob), B, 16 * C, _stream())
        ctx.save_for_backward(h, weight, prob)
        ctx.bias = bias
        return prob

    @staticmethod
    def backward(ctx, dprob):
        h, weight, prob = ctx.saved_tensors
        dprob = dprob.float().contiguous()
        B, C = h.shape[0], h.shape[1]
        dh = torch.empty_like(h)
        dw = param_grad(weight) if ctx.needs_input_grad[1] else None
        db = param_grad(ctx.bias) if ctx.needs_input_grad[2] else None
        call('sba_logits_bwd', _dt(h), _p(h), _p(weight), _p(prob), _p(dprob), _p(dh), _p(dw), _p(db), B, 16 * C, 0,
             _stream())
        return dh, None, None


class CondCatFn(torch.autograd.Function):
    """cat(h_code, c_code tiled 4x4) along channels (model.py:597-600)."""

    @staticmethod
    def forward(ctx, h, sent):
        h = as_act(h)
        B, C = h.shape[0], h.shape[1]
        sent = sent.float().contiguous()
        E = sent.shape[1]
        out = empty_act(B, C + E, 4, 4, h)
        call('sba_cond_cat_fwd', _dt(h), _p(h), _p(sent), _p(out), B, C, E, _stream())
        ctx.dims = (B, C, E)
        ctx.like = h
        return out

    @staticmethod
    def backward(ctx, dout):
        B, C, E = ctx.dims
        dout = _c(dout)
        dh = empty_act(B, C, 4, 4, dout)
        ds = torch.zeros((B, E), dtype=torch.float32, device=dout.device) if ctx.needs_input_grad[1] else None
        call('sba_cond_cat_bwd', _dt(dout), _p(dout), _p(dh), _p(ds), B, C, E, 0, _stream())
        return dh, ds


class BCEMultiFn(torch.autograd.Function):
    """sum_s weight_s * BCELoss(prob_s, target_s) in one launch (losses.py:144-158,175-182)."""

    @staticmethod
    def forward(ctx, targets, weights, *probs):
        dev = probs[0].device
        sizes = [int(p.numel()) for p in probs]
        cat = torch.cat([p.float().reshape(-1) for p in probs])
        offs = [0]
        for s in sizes:
            offs.append(offs[-1] + s)
        meta = _bce_meta(offs, targets, weights, dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        dprob = torch.empty_like(cat)
        call('sba_bce_multi', _p(cat), _p(meta[0]), _p(meta[1]), _p(meta[2]), len(sizes), _p(loss), _p(dprob),
             _stream())
        ctx.sizes = sizes
        ctx.save_for_backward(dprob)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (dprob,) = ctx.saved_tensors
        d = dprob * g
        return (None, None) + tuple(d.split(ctx.sizes))


_BCE_META = {}


def _bce_meta(offs, targets, weights, dev):
    key = (tuple(offs), tuple(targets), tuple(weights), dev)
    meta = _BCE_META.get(key)
    if meta is None:
        meta = (torch.tensor(offs, dtype=torch.int32, device=dev),
                torch.tensor(targets, dtype=torch.float32, device=dev),
                torch.tensor(weights, dtype=torch.float32, device=dev))
        _BCE_META[key] = meta
    return meta


Head = namedtuple('Head', 'row0 rows cond_row0 target weight segment')


class _CondGroup(object):
    """Conditional heads that share one jointConv launch: their inputs back to back in `xin`, the conv output `y`;
    off[head index] = the head's first row in both (and in the gradient of y)."""
    __slots__ = ('heads', 'off', 'xin', 'y', 'stats', 'want_stats', 'bn_forward')


def _cond_groups(heads, bn):
    """The conditional heads of one term (real / fake / wrong pairs, losses.py:143-149) share jointConv's weights: in
    training mode their inputs go into ONE tensor and one conv / data-gradient / weight-gradient launch serves all of them
    (M = 944 rows at B = 20 instead of three GEMM-like launches of 320 / 320 / 304 rows, each with its own K split +
    finishing launch); otherwise every head is a group of its own.  BatchNorm stays per head, in the reference's call
    order (batch statistics and running-statistic updates of three separate module calls)."""
    cond_idx = [i for i, hd in enumerate(heads) if hd.cond_row0 is not None]
    together = len(cond_idx) >= 2 and bn.training
    groups = []
    for idx in ([cond_idx] if together else [[i] for i in cond_idx]):
        g = _CondGroup()
        g.heads, g.off = idx, {}
        if len(idx) == 1:       # the statistics come out of the conv epilogue
            g.want_stats = bn.training
            g.bn_forward = lambda y, stats: bn_act_forward(y, stats, bn, ACT_LRELU)
        else:
            g.want_stats = False
            g.bn_forward = lambda y, stats: bn_act_forward_grouped(y, bn, ACT_LRELU, 1)
        groups.append(g)
    return groups


def _issue_order(heads):
    """the heads' backward passes go widest first (stable)"""
    return sorted(range(len(heads)), key=lambda i: -heads[i][1])


def _row_modes(heads, n_rows, groups=()):
    """The issue order of the heads' backward passes and, per head, how it writes its rows of
    d feats: 0 = store (nobody has written them yet), 1 = accumulate (all of them are written).  A head writes at its
    place in the issue order, except the heads of a `groups` entry (lists of head indices that share one data-gradient
    launch), which all write behind the last of them.  Widest first, so that the row ranges of the reference's five heads
    never overlap partially."""
    heads = [Head(*h) for h in heads]
    order = _issue_order(heads)
    pos = {i: k for k, i in enumerate(order)}
    at = dict(pos)
    for g in groups:
        for i in g:
            at[i] = max(pos[j] for j in g)
    written, modes = [], {}
    for i in sorted(order, key=lambda i: (at[i], pos[i])):
        r0, r1 = heads[i].row0, heads[i].row0 + heads[i].rows
        inside = any(a <= r0 and r1 <= b for a, b in written)
        if not inside:
            assert all(r1 <= a or b <= r0 for a, b in written), 'partially overlapping head rows'
            written.append((r0, r1))
        modes[i] = 1 if inside else 0
    covered = sorted(written)
    assert covered and covered[0][0] == 0 and covered[-1][1] == n_rows and \
        all(covered[k][1] == covered[k + 1][0] for k in range(len(covered) - 1)), 'rows without a head'
    return order, modes


def _logits_bwd(dt, h, o, prob, dprob, dh, need_p, rows, K, accumulate):
    call('sba_logits_bwd', dt, _p(h), _p(o.weight), _p(prob), _p(dprob), _p(dh),
         _p(param_grad(o.weight)) if need_p else None, _p(param_grad(o.bias)) if need_p else None,
         rows, K, accumulate, _stream())


class DHeadsFn(torch.autograd.Function):
    """Every head of one discriminator's loss term as ONE autograd node: the conditional heads
    (cat with the sentence code, jointConv + BatchNorm + LeakyReLU, logits; model.py:594-607), the unconditional
    heads (model.py:590-592) and the weighted BCE sum (losses.py:141-158 for the discriminator update,
    :169-178 for the generator term).

    `heads` = tuple of Head(row0, rows, cond_row0 | None, target, weight, segment): the head reads feats[row0:row0+rows]
    (and cond[cond_row0:cond_row0+rows] when conditional); they are evaluated in the order given (the reference's
    call order, which fixes the order of the jointConv BatchNorm running-statistic updates) and summed in `segment`
    order (the reference's order of the terms of errD / g_loss).  The same kernels as the per-head Functions
    run; what goes away is the autograd glue between them (row slices copied into zero-filled gradients, gradient sums
    of the shared feature map, cat of the probabilities): each head's backward writes or accumulates straight into
    its rows of d feats."""

    @staticmethod
    def forward(ctx, feats, cond, netD, heads, sink, *params):
        feats = as_act(feats)
        dev = feats.device
        dt = _dt(feats)
        C = feats.shape[1]
        assert feats.shape[2] == 4 and feats.shape[3] == 4
        K = 16 * C
        cnet, unet = netD.COND_DNET, netD.UNCOND_DNET
        if cond is not None:
            cond = cond.reshape(-1, cnet.ef_dim).float().contiguous()
        sizes, targets, weights = [0] * len(heads), [0.] * len(heads), [0.] * len(heads)
        for hd in heads:
            sizes[hd.segment], targets[hd.segment], weights[hd.segment] = hd.rows, hd.target, hd.weight
        offs = [0]
        for s in sizes:
            offs.append(offs[-1] + s)
        prob = torch.empty(offs[-1], dtype=torch.float32, device=dev)
        layer = cnet.jointConv._layer() if any(hd.cond_row0 is not None for hd in heads) else None
        groups = _cond_groups(heads, layer.bn) if layer is not None else []
        group_of = {i: g for g in groups for i in g.heads}
        tape = [None] * len(heads)
        for hi, hd in enumerate(heads):
            if hd.cond_row0 is None:
                x, o = feats[hd.row0:hd.row0 + hd.rows], unet.outlogits[0]
            else:
                g = group_of[hi]
                if hi == g.heads[0]:        # the inputs of the group's heads, then its one conv launch
                    E = cond.shape[1]
                    g.xin = empty_act(sum(heads[i].rows for i in g.heads), C + E, 4, 4, feats)
                    off = 0
                    for i in g.heads:
                        r0, rows, c0 = heads[i][:3]
                        call('sba_cond_cat_fwd', dt, _p(feats[r0:r0 + rows]), _p(cond[c0:c0 + rows]),
                             _p(g.xin[off:off + rows]), rows, C, E, _stream())
                        g.off[i] = off
                        off += rows
                    g.y, g.stats = conv_forward(g.xin, layer.pw, '3x3', want_stats=g.want_stats, pre_bn=True)
                y = g.y[g.off[hi]:g.off[hi] + hd.rows]
                x, st = g.bn_forward(y, g.stats)
                tape[hi] = (y, st, x)
                o = cnet.outlogits[0]
            pslice = prob[offs[hd.segment]:offs[hd.segment] + hd.rows]
            call('sba_logits_fwd', dt, _p(x), _p(o.weight), _p(o.bias), _p(pslice), hd.rows, K, _stream())
        meta = _bce_meta(offs, targets, weights, dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        dprob = torch.empty_like(prob)
        call('sba_bce_multi', _p(prob), _p(meta[0]), _p(meta[1]), _p(meta[2]), len(heads), _p(loss), _p(dprob),
             _stream())
        if sink is not None:
            # the overfitting read-out: the probabilities of the heads whose target is 1, counted right
            # behind the loss on this stream; segments next to each other are one slice of prob, one launch
            runs = []
            for seg in range(len(sizes)):
                if targets[seg] == 1. and sizes[seg] > 0:
                    if runs and runs[-1][1] == offs[seg]:
                        runs[-1][1] = offs[seg + 1]
                    else:
                        runs.append([offs[seg], offs[seg + 1]])
            sink([prob[a:b] for a, b in runs])
        ctx.netD, ctx.heads, ctx.offs, ctx.tape, ctx.groups = netD, heads, offs, tape, groups
        ctx.has_cond = cond is not None
        ctx.cond_shape = None if cond is None else tuple(cond.shape)
        ctx.save_for_backward(feats, prob, dprob)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        feats, prob, dprob = ctx.saved_tensors
        netD, heads, offs, groups = ctx.netD, ctx.heads, ctx.offs, ctx.groups
        cnet, unet = netD.COND_DNET, netD.UNCOND_DNET
        dt = _dt(feats)
        C = feats.shape[1]
        K = 16 * C
        d = dprob * g
        need_feats = ctx.needs_input_grad[0]
        need_cond = ctx.has_cond and ctx.needs_input_grad[1]
        need_p = any(ctx.needs_input_grad[5:])
        dfeats = torch.empty_like(feats) if need_feats else None
        dcond = torch.zeros(ctx.cond_shape, dtype=torch.float32, device=feats.device) if need_cond else None
        # (a term without a gradient to feats may hold any subset of the heads: nothing to cover)
        order, modes = _row_modes(heads, feats.shape[0], [grp.heads for grp in groups]) if need_feats \
            else (_issue_order(heads), None)
        group_of = {i: grp for grp in groups for i in grp.heads}
        issued = {grp: [j for j in order if j in grp.off] for grp in groups}      # a group's heads in issue order
        dy = {grp: torch.empty(grp.y.shape, dtype=_act_dtype(grp.y), device=grp.y.device, memory_format=CL)
              for grp in groups}

        def dh_rows(i):
            """(head i's rows of d feats | a scratch tensor when nobody wants them, store / accumulate)"""
            rows = slice(heads[i].row0, heads[i].row0 + heads[i].rows)
            return (dfeats[rows], modes[i]) if need_feats else (torch.empty_like(feats[rows]), 0)

        for i in order:
            hd = heads[i]
            ps, ds = prob[offs[hd.segment]:offs[hd.segment] + hd.rows], d[offs[hd.segment]:offs[hd.segment] + hd.rows]
            if hd.cond_row0 is None:
                if need_feats or need_p:
                    dh, acc = dh_rows(i)
                    _logits_bwd(dt, feats[hd.row0:hd.row0 + hd.rows], unet.outlogits[0], ps, ds, dh, need_p, hd.rows, K,
                                acc)
                continue
            # a conditional head: back to its rows of the group's dy; behind the group's last head the conv gradients, once
            grp, layer = group_of[i], cnet.jointConv._layer()
            y, st, hc = ctx.tape[i]
            dhc = torch.empty_like(hc)
            _logits_bwd(dt, hc, cnet.outlogits[0], ps, ds, dhc, need_p, hd.rows, K, 0)
            bn_act_backward(y, dhc, st, layer.bn, ACT_LRELU, need_p, out=dy[grp][grp.off[i]:grp.off[i] + hd.rows])
            if i != issued[grp][-1]:
                continue
            if need_p:
                conv_wgrad_overlapped(grp.xin, dy[grp], layer.conv.weight, '3x3')
            if need_feats or need_cond:
                dxin = conv_dgrad(dy[grp], layer.pw, '3x3', (4, 4))
                E = grp.xin.shape[1] - C
                for j in issued[grp]:
                    r0, rows, c0 = heads[j][:3]
                    dh, acc = dh_rows(j)
                    call('sba_cond_cat_bwd', dt, _p(dxin[grp.off[j]:grp.off[j] + rows]), _p(dh),
                         _p(dcond[c0:c0 + rows]) if need_cond else None, rows, C, E, acc, _stream())
        return (dfeats, dcond, None, None, None) + (None,) * (len(ctx.needs_input_grad) - 5)


def d_heads(netD, feats, cond, heads, sink=None):
    """DHeadsFn with the parameters of netD's heads passed as autograd inputs (their gradients go to the flat
    gradient buffers like every other layer's).  sink (optional, sbagan.diffaug.DiffAugment.count_sink): called in the
    forward with the slices of the probability vector that belong to heads of target 1 -- it counts their signs on the
    device (ops.ada_count); None: nothing more is launched."""
    params = []
    if netD.COND_DNET is not None:
        c = netD.COND_DNET
        if c.bcondition:
            l = c.jointConv._layer()
            params += [l.conv.weight, l.bn.weight, l.bn.bias]
        params += [c.outlogits[0].weight, c.outlogits[0].bias]
    if netD.UNCOND_DNET is not None:
        u = netD.UNCOND_DNET
        params += [u.outlogits[0].weight, u.outlogits[0].bias]
    return DHeadsFn.apply(feats, cond, netD, tuple(Head(*h) for h in heads), sink, *params)


class KLFn(torch.autograd.Function):
    """KL_loss (losses.py:210-214)."""

    @staticmethod
    def forward(ctx, mu, logvar):
        mu, logvar = mu.contiguous(), logvar.contiguous()
        loss = torch.empty(1, dtype=torch.float32, device=mu.device)
        dmu, dlv = torch.empty_like(mu), torch.empty_like(logvar)
        call('sba_kl_loss', _p(mu), _p(logvar), _p(loss), _p(dmu), _p(dlv), mu.numel(), _stream())
        ctx.save_for_backward(dmu, dlv)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        dmu, dlv = ctx.saved_tensors
        return dmu * g, dlv * g


DAMSM_MFMA = True       # the words loss on the matrix cores where the shape allows (False: the f32 kernels)


def _damsm_prep(feat, words, cap_lens, B, nef, R, L):
    """bf16 hi + lo operand copies for the matrix-core words loss (include/sbagan_hip.h: sba_damsm_prep), or None when the
    shape is outside that path (the f32 kernels then run)"""
    if not DAMSM_MFMA:
        return None
    nbytes = int(_lib.lib.sba_damsm_prep_bytes(B, nef, R, L))
    if nbytes <= 0:
        return None
    prep = torch.empty(nbytes, dtype=torch.uint8, device=feat.device)
    call('sba_damsm_prep', _p(feat), _p(words), _p(cap_lens), _p(prep), nbytes, B, nef, R, L, _stream())
    return prep


def _damsm_words_fwd(prep, feat, words, cap_lens, sim, attn, attn1, wctx, B, nef, R, L, g1, g2, st):
    if prep is not None:
        call('sba_damsm_words_fwd_mfma', _p(prep), _p(words), _p(cap_lens), _p(sim), _p(attn), _p(attn1), _p(wctx), B, nef,
             R, L, g1, g2, st)
    else:
        call('sba_damsm_words_fwd', _p(feat), _p(words), _p(cap_lens), _p(sim), _p(attn), _p(attn1), _p(wctx), B, nef, R,
             L, g1, g2, st)


def _damsm_words_bwd(prep, feat, words, cap_lens, sim, attn, attn1, wctx, dsim, dwords, B, nef, R, L, g1, g2, st):
    """returns dfeat (f32, feat's shape); dwords (zero-filled or None) is accumulated into"""
    if prep is not None:
        nbytes = int(_lib.lib.sba_damsm_bwd_bytes(B, nef, R, L))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=feat.device)
        dfeat = torch.empty_like(feat)              # (the matrix-core path STORES every element)
        call('sba_damsm_words_bwd_mfma', _p(prep), _p(words), _p(cap_lens), _p(sim), _p(attn), _p(attn1), _p(wctx),
             _p(dsim), _p(scratch), nbytes, _p(dfeat), 0, _p(dwords), B, nef, R, L, g1, g2, st)
    else:
        dfeat = torch.zeros_like(feat)
        call('sba_damsm_words_bwd', _p(feat), _p(words), _p(cap_lens), _p(sim), _p(attn), _p(attn1), _p(wctx), _p(dsim),
             _p(dfeat), _p(dwords), B, nef, R, L, g1, g2, st)
    return dfeat


class WordsLossFn(torch.autograd.Function):
    """words_loss (losses.py:62-132): returns (loss0, loss1)."""

    @staticmethod
    def forward(ctx, feat, words, cap_lens, mask, gammas):
        _need_gpu(feat)
        g1, g2, g3 = gammas
        B, nef = feat.shape[0], feat.shape[1]
        R = feat.shape[2] * feat.shape[3]
        feat = feat.float().contiguous()
        words = words.float().contiguous()
        L = words.shape[2]
        dev = feat.device
        cap_lens = cap_lens.to(device=dev, dtype=torch.int64).contiguous()
        sim = torch.empty((B, B), dtype=torch.float32, device=dev)
        attn = torch.empty((B * B, L, R), dtype=torch.float32, device=dev)
        attn1 = torch.empty((B * B, L, R), dtype=torch.float32, device=dev)
        wctx = torch.empty((B * B, L, nef), dtype=torch.float32, device=dev)
        prep = _damsm_prep(feat, words, cap_lens, B, nef, R, L)
        _damsm_words_fwd(prep, feat, words, cap_lens, sim, attn, attn1, wctx, B, nef, R, L, g1, g2, _stream())
        loss = torch.empty(2, dtype=torch.float32, device=dev)
        d0, d1 = torch.empty_like(sim), torch.empty_like(sim)
        call('sba_ce_pair', _p(sim), _p(mask), g3, _p(loss), _p(d0), _p(d1), B, _stream())
        ctx.save_for_backward(feat, words, cap_lens, sim, attn, attn1, wctx, d0, d1)
        ctx.g = (g1, g2)
        ctx.prep = prep
        ctx.fshape = None
        return loss[0], loss[1]

    @staticmethod
    def backward(ctx, gl0, gl1):
        feat, words, cap_lens, sim, attn, attn1, wctx, d0, d1 = ctx.saved_tensors
        B, nef = feat.shape[0], feat.shape[1]
        R = feat.shape[2] * feat.shape[3]
        L = words.shape[2]
        dev = feat.device
        z = torch.zeros(1, dtype=torch.float32, device=dev)
        gl0 = z if gl0 is None else gl0.reshape(1).float()
        gl1 = z if gl1 is None else gl1.reshape(1).float()
        dsim = torch.empty_like(sim)
        call('sba_combine2', _p(dsim), _p(d0), _p(gl0), _p(d1), _p(gl1), B * B, _stream())
        dwords = torch.zeros_like(words) if ctx.needs_input_grad[1] else None
        dfeat = _damsm_words_bwd(ctx.prep, feat, words, cap_lens, sim, attn, attn1, wctx, dsim, dwords, B, nef, R, L,
                                 ctx.g[0], ctx.g[1], _stream())
        return dfeat, dwords, None, None, None


class SentLossFn(torch.autograd.Function):
    """sent_loss (losses.py:20-59): returns (loss0, loss1)."""

    @staticmethod
    def forward(ctx, cnn, rnn, mask, gamma3, eps):
        _need_gpu(cnn)
        cnn, rnn = cnn.float().contiguous(), rnn.float().contiguous()
        B, nef = cnn.shape
        dev = cnn.device
        s = torch.empty((B, B), dtype=torch.float32, device=dev)
        call('sba_damsm_sent_fwd', _p(cnn), _p(rnn), _p(s), B, nef, gamma3, eps, _stream())
        loss = torch.empty(2, dtype=torch.float32, device=dev)
        d0, d1 = torch.empty_like(s), torch.empty_like(s)
        call('sba_ce_pair', _p(s), _p(mask), 1.0, _p(loss), _p(d0), _p(d1), B, _stream())
        ctx.save_for_backward(cnn, rnn, d0, d1)
        ctx.k = (gamma3, eps)
        return loss[0], loss[1]

    @staticmethod
    def backward(ctx, gl0, gl1):
        cnn, rnn, d0, d1 = ctx.saved_tensors
        B, nef = cnn.shape
        dev = cnn.device
        z = torch.zeros(1, dtype=torch.float32, device=dev)
        gl0 = z if gl0 is None else gl0.reshape(1).float()
        gl1 = z if gl1 is None else gl1.reshape(1).float()
        ds = torch.empty_like(d0)
        call('sba_combine2', _p(ds), _p(d0), _p(gl0), _p(d1), _p(gl1), B * B, _stream())
        dcnn = torch.zeros_like(cnn) if ctx.needs_input_grad[0] else None
        drnn = torch.zeros_like(rnn) if ctx.needs_input_grad[1] else None
        call('sba_damsm_sent_bwd', _p(cnn), _p(rnn), _p(ds), _p(dcnn), _p(drnn), B, nef, ctx.k[0], ctx.k[1],
             _stream())
        return dcnn, drnn, None, None, None


_LAMBDA_CELL = {}
_DAMSM_SIDE = {}


def _damsm_side_stream(dev):
    s = _DAMSM_SIDE.get(dev)
    if s is None:
        s = _DAMSM_SIDE[dev] = torch.cuda.Stream(device=dev)
    return s


def damsm_terms_direct(region_features, cnn_code, words_embs, sent_emb, cap_lens, mask, gammas, lam, eps=1e-8):
    """w_loss = LAMBDA (loss0 + loss1) of words_loss, s_loss likewise of sent_loss (losses.py:187-204), TOGETHER WITH
    their gradients w.r.t. the image-side inputs (region features, global code), no autograd in between.  For a frozen
    text side the upstream gradient of the four cross-entropy terms is the constant LAMBDA, so the words head is
    prep (2 launches) -> forward -> cross entropies + their gradient (sba_ce_pair_direct) -> backward (2 launches), the
    sentence loss ONE launch (sba_damsm_sent_direct): 7 launches on the image encoder's chain -- the critical one of the
    step -- where the autograd path issues ~35 (scalar adds, LAMBDA multiplications, fills).  B <= 96.
    Returns (w_loss, s_loss, d region_features, d cnn_code)."""
    g1, g2, g3 = gammas
    feat = region_features.detach().float().contiguous()
    cnn = cnn_code.detach().float().contiguous()
    words = words_embs.detach().float().contiguous()
    rnn = sent_emb.detach().float().contiguous()
    B, nef = feat.shape[0], feat.shape[1]
    R = feat.shape[2] * feat.shape[3]
    L = words.shape[2]
    dev = feat.device
    cap_lens = cap_lens.to(device=dev, dtype=torch.int64).contiguous()
    st = _stream()
    losses = torch.empty(2, dtype=torch.float32, device=dev)        # [w_loss, s_loss], written by the two head kernels
    dcnn = torch.empty_like(cnn)
    # the sentence loss depends on nothing of the words path: a one-workgroup launch (96 us inside the step) -- on a side
    # stream, beside the words kernels; joined below (its outputs were allocated above, on this stream, and outlive the join)
    cur = torch.cuda.current_stream()
    side = _damsm_side_stream(dev)
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        call('sba_damsm_sent_direct', _p(cnn), _p(rnn), _p(mask), g3, eps, float(lam), _p(losses[1:2]), _p(dcnn), B, nef,
             _stream())
    sim = torch.empty((B, B), dtype=torch.float32, device=dev)
    attn = torch.empty((B * B, L, R), dtype=torch.float32, device=dev)
    attn1 = torch.empty((B * B, L, R), dtype=torch.float32, device=dev)
    wctx = torch.empty((B * B, L, nef), dtype=torch.float32, device=dev)
    prep = _damsm_prep(feat, words, cap_lens, B, nef, R, L)
    _damsm_words_fwd(prep, feat, words, cap_lens, sim, attn, attn1, wctx, B, nef, R, L, g1, g2, st)
    dsim = torch.empty_like(sim)
    call('sba_ce_pair_direct', _p(sim), _p(mask), g3, float(lam), _p(losses[0:1]), _p(dsim), B, st)
    dfeat = _damsm_words_bwd(prep, feat, words, cap_lens, sim, attn, attn1, wctx, dsim, None, B, nef, R, L, g1, g2, st)
    cur.wait_stream(side)
    w_loss, s_loss = losses[0], losses[1]
    return w_loss, s_loss, dfeat, dcnn


# ----------------------------------------------------------------------------
# text encoder
def lstm_bidir_forward(captions, cap_lens, emb_weight, w_ih, w_hh, b_ih, b_hh, hidden=None, max_len=None, out=None):
    """RNN_ENCODER.forward (model.py:127-159) of the frozen text encoder, sync-free: cap_lens stays on the
    device.  w_ih [2][4H][ninput], w_hh [2][4H][H], b_* [2][4H]; returns (words_emb B x 2H x L,
    sent_emb B x 2H) with L = max_len (the reference's max(cap_lens), if the host knows it) or T."""
    _need_gpu(captions)
    B, T = captions.shape
    H = w_hh.shape[2]
    L = T if max_len is None else int(max_len)
    dev = captions.device
    captions = captions.to(torch.int64).contiguous()
    cap_lens = cap_lens.to(device=dev, dtype=torch.int64).contiguous()
    gx = torch.empty((2, B * T, 4 * H), dtype=torch.float32, device=dev)
    if out is not None:         # caller-owned (static) output tensors: no copy in a recorded / captured step
        words, sent = out
        assert words.shape == (B, 2 * H, L) and sent.shape == (B, 2 * H) and words.is_contiguous() and \
            sent.is_contiguous() and words.dtype == torch.float32 and sent.dtype == torch.float32
    else:
        words = torch.empty((B, 2 * H, L), dtype=torch.float32, device=dev)
        sent = torch.empty((B, 2 * H), dtype=torch.float32, device=dev)
    h0 = c0 = None
    if hidden is not None:
        h0, c0 = hidden[0].float().contiguous(), hidden[1].float().contiguous()
    call('sba_lstm_bidir_fwd', _p(captions), _p(cap_lens), _p(emb_weight), _p(w_ih), _p(w_hh), _p(b_ih), _p(b_hh),
         _p(h0), _p(c0), _p(gx), _p(words), _p(sent), B, T, L, emb_weight.shape[0], emb_weight.shape[1], H, _stream())
    return words, sent


class LstmBidirTrainFn(torch.autograd.Function):
    """One-layer bidirectional LSTM over packed sequences with gradients (RNN_ENCODER in training mode: DAMSM
    pre-training, pretrain_DAMSM.py:79-100).  x [B][T][ninput] is the (dropped-out) embedded caption batch; the
    recurrence and back-propagation through time are csrc/text.hip kernels, the dense projections around them are
    plain GEMMs through the BLAS library (torch.matmul).  Returns (words_emb B x 2H x L, sent_emb B x 2H)."""

    @staticmethod
    def forward(ctx, x, cap_lens, w_ih, w_hh, b_ih, b_hh, h0, c0, L):
        _need_gpu(x)
        B, T, _ = x.shape
        H = w_hh.shape[2]
        dev = x.device
        x2 = x.reshape(B * T, -1).float().contiguous()
        gx = torch.matmul(x2.unsqueeze(0), w_ih.transpose(1, 2)) + (b_ih + b_hh).unsqueeze(1)     # [2][B*T][4H]
        gx = gx.contiguous()
        cap_lens = cap_lens.to(device=dev, dtype=torch.int64).contiguous()
        words = torch.empty((B, 2 * H, L), dtype=torch.float32, device=dev)
        sent = torch.empty((B, 2 * H), dtype=torch.float32, device=dev)
        gates = torch.zeros((2, B * T, 4 * H), dtype=torch.float32, device=dev)
        cs = torch.zeros((2, B * T, H), dtype=torch.float32, device=dev)
        hs = torch.zeros((2, B * T, H), dtype=torch.float32, device=dev)
        w_hh = w_hh.contiguous()
        call('sba_lstm_recur_train', _p(gx), _p(cap_lens), _p(w_hh), _p(h0), _p(c0), _p(words), _p(sent), _p(gates),
             _p(cs), _p(hs), B, T, L, H, _stream())
        ctx.save_for_backward(x2, cap_lens, w_ih, w_hh, gates, cs, hs)
        ctx.h0c0, ctx.dims = (h0, c0), (B, T, L, H)
        return words, sent

    @staticmethod
    def backward(ctx, dwords, dsent):
        x2, cap_lens, w_ih, w_hh, gates, cs, hs = ctx.saved_tensors
        B, T, L, H = ctx.dims
        h0, c0 = ctx.h0c0
        dev = x2.device
        dwords = torch.zeros((B, 2 * H, L), device=dev) if dwords is None else dwords.float().contiguous()
        dsent = torch.zeros((B, 2 * H), device=dev) if dsent is None else dsent.float().contiguous()
        dG = torch.zeros((2, B * T, 4 * H), dtype=torch.float32, device=dev)
        hprev = torch.zeros((2, B * T, H), dtype=torch.float32, device=dev)
        call('sba_lstm_recur_bwd', _p(cap_lens), _p(w_hh), _p(h0), _p(c0), _p(gates), _p(cs), _p(hs), _p(dwords),
             _p(dsent), _p(dG), _p(hprev), B, T, L, H, _stream())
        dGt = dG.transpose(1, 2)                                   # [2][4H][B*T]
        dw_ih = torch.matmul(dGt, x2.unsqueeze(0))                 # [2][4H][ninput]
        dw_hh = torch.matmul(dGt, hprev)                           # [2][4H][H]
        db = dG.sum(1)                                             # [2][4H]
        dx = torch.matmul(dG, w_ih).sum(0).view(B, T, -1) if ctx.needs_input_grad[0] else None
        return dx, None, dw_ih, dw_hh, db, db, None, None, None


class EmbedDropoutFn(torch.autograd.Function):
    """Embedding -> Dropout of RNN_ENCODER's training path with the keep mask as a tensor (sba_embed_dropout_fwd / _bwd):
    out[b][t][c] = keep[b][t][c] ? weight[captions[b][t]][c] * scale : 0.  `keep` (uint8 [B][T][ninput]) is drawn by the
    caller per batch, so the launch holds no random state and can be recorded (sbagan.damsm.DAMSMSlotStep).  The
    backward ADDS the weight's gradient straight into weight.grad (the parameter's view of its flat gradient buffer,
    cleared by zero_grad) and hands autograd nothing for it."""

    @staticmethod
    def forward(ctx, captions, weight, keep, scale):
        _need_gpu(captions)
        B, T = captions.shape
        ntoken, ninput = weight.shape
        if captions.dtype != torch.int64 or not captions.is_contiguous():
            raise ValueError('EmbedDropoutFn: captions must be contiguous int64 [B][T]')
        if weight.dtype != torch.float32 or not weight.is_contiguous() or ninput % 4:
            raise ValueError('EmbedDropoutFn: weight must be contiguous f32 [ntoken][ninput], ninput % 4 == 0')
        if keep.dtype != torch.uint8 or tuple(keep.shape) != (B, T, ninput) or not keep.is_contiguous():
            raise ValueError('EmbedDropoutFn: keep must be contiguous uint8 [%d][%d][%d]' % (B, T, ninput))
        out = torch.empty((B, T, ninput), dtype=torch.float32, device=captions.device)
        call('sba_embed_dropout_fwd', _p(captions), _p(weight), _p(keep), float(scale), _p(out), B * T, ntoken, ninput,
             _stream())
        ctx.captions, ctx.weight, ctx.keep, ctx.scale = captions, weight, keep, float(scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        captions, weight, keep = ctx.captions, ctx.weight, ctx.keep
        B, T = captions.shape
        ntoken, ninput = weight.shape
        dW = param_grad(weight)
        if dW.dtype != torch.float32 or not dW.is_contiguous():
            raise ValueError('EmbedDropoutFn: weight.grad must be contiguous f32')
        dout = dout.float().contiguous()
        call('sba_embed_dropout_bwd', _p(captions), _p(keep), ctx.scale, _p(dout), _p(dW), B * T, ntoken, ninput,
             _stream())
        return None, None, None, None


# ----------------------------------------------------------------------------
# evaluation: R-precision ranking (sbagan/rprecision.py)
def rprec_rank(cnn, true_emb, pool, idx, eps=1e-8, want_scores=False):
    """rank[b] = #{ m : NOT (cos(cnn[b], pool[idx[b, m]]) < cos(cnn[b], true_emb[b])) }, cos = dot / max(|a| |c|, eps) in
    f32 (sba_rprec_rank): ties and NaNs count against the image.  cnn, true_emb [B][nef] and pool [P][nef]: contiguous
    f32 device tensors, nef % 4 == 0, 4 <= nef <= 1024.  idx [B][M]: int32 rows of pool, either on the HOST (a numpy
    array or CPU tensor: range-checked there and uploaded, no device sync) or on the device (range-checked with one
    sync).  Everything is checked before the launch: TypeError for a dtype, ValueError for a shape, a stride or an index
    out of range.  Returns rank (int32 [B], device), or (rank, scores [B][M + 1], column 0 = the true caption)."""
    for t in (cnn, true_emb, pool):
        _need_gpu(t)
    for name, t in (('cnn', cnn), ('true_emb', true_emb), ('pool', pool)):
        if t.dtype != torch.float32:
            raise TypeError('rprec_rank: %s must be float32 (got %s)' % (name, t.dtype))
        if t.dim() != 2:
            raise ValueError('rprec_rank: %s must be 2-D (got %s)' % (name, tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError('rprec_rank: %s must be contiguous' % name)
        if t.device != cnn.device:
            raise ValueError('rprec_rank: %s is on %s, cnn on %s' % (name, t.device, cnn.device))
    if not torch.is_tensor(idx):
        idx = torch.as_tensor(idx)
    if idx.dtype != torch.int32:
        raise TypeError('rprec_rank: idx must be int32 (got %s)' % idx.dtype)
    B, nef = cnn.shape
    P = pool.shape[0]
    if B < 1 or P < 1:
        raise ValueError('rprec_rank: needs at least one image and one pool row (B = %d, P = %d)' % (B, P))
    if nef % 4 or not 4 <= nef <= 1024:
        raise ValueError('rprec_rank: nef must be a multiple of 4 in [4, 1024] (got %d)' % nef)
    if tuple(true_emb.shape) != (B, nef) or pool.shape[1] != nef:
        raise ValueError('rprec_rank: true_emb %s / pool %s do not match cnn %s'
                         % (tuple(true_emb.shape), tuple(pool.shape), tuple(cnn.shape)))
    if idx.dim() != 2 or idx.shape[0] != B:
        raise ValueError('rprec_rank: idx must be [B][M] with B = %d (got %s)' % (B, tuple(idx.shape)))
    if not idx.is_contiguous():
        raise ValueError('rprec_rank: idx must be contiguous')
    M = idx.shape[1]
    if M > 0:
        lo, hi = int(idx.min()), int(idx.max())          # (a device idx: the one sync of this call)
        if lo < 0 or hi >= P:
            raise ValueError('rprec_rank: idx out of range [0, %d): min %d, max %d' % (P, lo, hi))
    dev = cnn.device
    if not idx.is_cuda:
        idx = idx.pin_memory().to(dev, non_blocking=True) if M > 0 else idx.to(dev)
    elif idx.device != dev:
        raise ValueError('rprec_rank: idx is on %s, cnn on %s' % (idx.device, dev))
    rank = torch.empty(B, dtype=torch.int32, device=dev)
    scores = torch.empty((B, M + 1), dtype=torch.float32, device=dev) if want_scores else None
    call('sba_rprec_rank', _p(cnn), _p(true_emb), _p(pool), _p(idx) if M > 0 else None, float(eps), _p(rank), _p(scores),
         B, M, nef, P, _stream())
    return (rank, scores) if want_scores else rank


# ----------------------------------------------------------------------------
# attention-map overlays (sbagan/visualize.py)
def _vis_need(name, t, what, dtype, dim):
    if not torch.is_tensor(t):
        raise TypeError('%s: %s must be a tensor' % (name, what))
    _need_gpu(t)
    if t.dtype != dtype:
        raise TypeError('%s: %s must be %s (got %s)' % (name, what, dtype, t.dtype))
    if t.dim() != dim:
        raise ValueError('%s: %s must be %d-D (got %s)' % (name, what, dim, tuple(t.shape)))
    if not t.is_contiguous():
        raise ValueError('%s: %s must be contiguous' % (name, what))


def vis_expand(maps, M=None, thresh=None):
    """out[i] = M maps'[i] M^T in f32, all maps in one launch (sba_vis_expand).  maps [n][a][a] and M [V][a]: contiguous
    f32 device tensors, 1 <= a <= 128, a <= V <= 1024; M None: the maps themselves (V = a).  thresh (optional, [n] f32):
    maps' = maps * (maps > thresh[i]).  Everything is checked before the launch: TypeError for a dtype, ValueError for
    a shape, a stride or a size.  Returns (out [n][V][V], stats [3][n] = per-map min and max of out, and conf = the sum of
    the map's values above 2 thresh[i] (of all of them without thresh))."""
    _vis_need('vis_expand', maps, 'maps', torch.float32, 3)
    n, a, a2 = maps.shape
    if a != a2 or n < 1 or n > 65535 or not 1 <= a <= 128:
        raise ValueError('vis_expand: maps must be [n][a][a] with 1 <= n <= 65535, 1 <= a <= 128 (got %s)'
                         % (tuple(maps.shape),))
    V = a
    if M is not None:
        _vis_need('vis_expand', M, 'M', torch.float32, 2)
        V = M.shape[0]
        if M.shape[1] != a or not a <= V <= 1024:
            raise ValueError('vis_expand: M must be [V][a] with a = %d <= V <= 1024 (got %s)' % (a, tuple(M.shape)))
        if M.device != maps.device:
            raise ValueError('vis_expand: M is on %s, maps on %s' % (M.device, maps.device))
        if M.data_ptr() % 16:
            raise ValueError('vis_expand: M must be 16-byte aligned')
    if thresh is not None:
        _vis_need('vis_expand', thresh, 'thresh', torch.float32, 1)
        if thresh.shape[0] != n or thresh.device != maps.device:
            raise ValueError('vis_expand: thresh must be [n] = [%d] on %s (got %s on %s)'
                             % (n, maps.device, tuple(thresh.shape), thresh.device))
    out = torch.empty((n, V, V), dtype=torch.float32, device=maps.device)
    stats = torch.empty((3, n), dtype=torch.float32, device=maps.device)
    call('sba_vis_expand', _p(maps), _p(thresh), _p(M), _p(out), _p(stats[0]), _p(stats[1]), _p(stats[2]), n, a, V,
         _stream())
    return out, stats


VIS_BLACK, VIS_IMAGE, VIS_MAP, VIS_BLEND = 0, 1, 2, 3


def vis_compose(V, band, desc, par, band_rgb, expanded=None, imgs0=None, imgs1=None):
    """The uint8 HWC canvas of an overlay image, all but its text, in one launch (sba_vis_compose; the layout is
    described in include/sbagan_hip.h).  desc [nS][nr][nc][4] int32, par [nS][nr][nc][2] f32 and band_rgb [nS][nc] uint32:
    HOST arrays (numpy), checked here -- kinds, mask values, image and map indices -- and uploaded; expanded [nE][V][V],
    imgs0 / imgs1 [n][3][S][S]: contiguous f32 device tensors or None.  TypeError for a dtype, ValueError for a shape, a
    stride or an index, before any launch.  Returns the canvas, a [nS (band + nr V)][nc (V + 2)][3] uint8 device tensor."""
    import numpy as np
    desc, par, band_rgb = np.asarray(desc), np.asarray(par), np.asarray(band_rgb)
    if desc.dtype != np.int32 or par.dtype != np.float32 or band_rgb.dtype != np.uint32:
        raise TypeError('vis_compose: desc / par / band_rgb must be int32 / float32 / uint32 (got %s / %s / %s)'
                        % (desc.dtype, par.dtype, band_rgb.dtype))
    if desc.ndim != 4 or desc.shape[3] != 4:
        raise ValueError('vis_compose: desc must be [nS][nr][nc][4] (got %s)' % (desc.shape,))
    nS, nr, nc = desc.shape[:3]
    if par.shape != (nS, nr, nc, 2) or band_rgb.shape != (nS, nc):
        raise ValueError('vis_compose: par %s / band_rgb %s do not match desc %s' % (par.shape, band_rgb.shape, desc.shape))
    V, band = int(V), int(band)
    if not (1 <= V <= 1024 and 0 <= band <= 4096 and 1 <= nS <= 64 and 1 <= nr <= 8 and 1 <= nc <= 64):
        raise ValueError('vis_compose: V %d, band %d or the cell grid %s is out of range' % (V, band, desc.shape[:3]))
    W, H = nc * (V + 2), nS * (band + nr * V)
    if H > 65535:
        raise ValueError('vis_compose: the canvas is %d rows high (at most 65535)' % H)
    dev = None
    counts = []
    for what, t in (('expanded', expanded), ('imgs0', imgs0), ('imgs1', imgs1)):
        if t is None:
            counts.append(0)
            continue
        _vis_need('vis_compose', t, what, torch.float32, 3 if what == 'expanded' else 4)
        if dev is not None and t.device != dev:
            raise ValueError('vis_compose: %s is on %s, not on %s' % (what, t.device, dev))
        dev = t.device
        if what == 'expanded':
            if tuple(t.shape[1:]) != (V, V):
                raise ValueError('vis_compose: expanded must be [nE][%d][%d] (got %s)' % (V, V, tuple(t.shape)))
        elif t.shape[1] != 3 or t.shape[2] != t.shape[3] or not 1 <= t.shape[2] <= 4096:
            raise ValueError('vis_compose: %s must be [n][3][S][S] (got %s)' % (what, tuple(t.shape)))
        if not 1 <= t.shape[0] <= 65535:
            raise ValueError('vis_compose: %s holds %d entries' % (what, t.shape[0]))
        counts.append(t.shape[0])
    if dev is None:
        raise ValueError('vis_compose: needs the expanded maps or an image batch')
    kind, img, mp, m = (desc[..., k] for k in range(4))
    if kind.min() < 0 or kind.max() > 3:
        raise ValueError('vis_compose: cell kinds must be 0..3')
    uses_map, uses_img = kind >= VIS_MAP, (kind == VIS_IMAGE) | (kind == VIS_BLEND)
    if uses_map.any() and (mp[uses_map].min() < 0 or mp[uses_map].max() >= counts[0]):
        raise ValueError('vis_compose: a map index is outside [0, %d)' % counts[0])
    if (kind == VIS_BLEND).any() and (m[kind == VIS_BLEND].min() < 0 or m[kind == VIS_BLEND].max() > 255):
        raise ValueError('vis_compose: a blend mask is outside [0, 255]')
    if uses_img.any():
        which, idx = img[uses_img] >> 16, img[uses_img] & 65535
        if which.min() < 0 or which.max() > 1:
            raise ValueError('vis_compose: an image batch is not 0 or 1')
        for w in (0, 1):
            if (which == w).any() and idx[which == w].max() >= counts[1 + w]:
                raise ValueError('vis_compose: an image index of batch %d is outside [0, %d)' % (w, counts[1 + w]))
    words = np.concatenate([np.ascontiguousarray(desc).view(np.uint32).ravel(),
                            np.ascontiguousarray(par).view(np.uint32).ravel(),
                            np.ascontiguousarray(band_rgb).ravel()]).view(np.int32)
    table = torch.from_numpy(words).to(dev)          # one upload: desc | par | band_rgb
    nd, npar = desc.size, par.size
    canvas = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    base = table.data_ptr()
    call('sba_vis_compose', _p(canvas), W, H, V, band, nS, nr, nc, base, base + 4 * nd, base + 4 * (nd + npar),
         _p(expanded), counts[0], _p(imgs0), counts[1], imgs0.shape[2] if imgs0 is not None else 0,
         _p(imgs1), counts[2], imgs1.shape[2] if imgs1 is not None else 0, _stream())
    return canvas


# ----------------------------------------------------------------------------
# evaluation (sbagan/fid.py, sbagan/prdc.py, sbagan/retrieval.py, sbagan/kid.py): what the kernel families check alike
EVAL_MAX_SPLITS = 32
PRDC_MAX_SPLITS = KID_MAX_SPLITS = EVAL_MAX_SPLITS


def _feature_tensor(name, x, what):
    """an f32 2-D tensor on the device"""
    if not torch.is_tensor(x):
        raise TypeError('%s: %s must be a tensor' % (name, what))
    _need_gpu(x)
    if x.dtype != torch.float32:
        raise TypeError('%s: %s must be float32 (got %s)' % (name, what, x.dtype))
    if x.dim() != 2:
        raise ValueError('%s: %s must be 2-D (got %s)' % (name, what, tuple(x.shape)))


def _feature_rows(name, x, what, device=None, D=None):
    """(n, D, row stride) of an f32 [n][D] feature-row tensor the evaluation kernels can read"""
    _feature_tensor(name, x, what)
    if device is not None and x.device != device:
        raise ValueError('%s: %s is on %s, not on %s' % (name, what, x.device, device))
    n, d = x.shape
    if n < 1 or d < 64 or d % 64 or (D is not None and d != D):
        raise ValueError('%s: %s must be [n >= 1][%s] (got %s)'
                         % (name, what, D if D is not None else 'a positive multiple of 64', tuple(x.shape)))
    ld = x.stride(0) if n > 1 else d        # (a single row has no meaningful row stride)
    if x.stride(1) != 1 or ld < d or ld % 4:
        raise ValueError('%s: %s needs unit column stride and a row stride >= D that is a multiple of 4 (got strides '
                         '%s)' % (name, what, tuple(x.stride())))
    if x.data_ptr() % 16:
        raise ValueError('%s: %s must be 16-byte aligned' % (name, what))
    return n, d, ld


def _eval_splits(name, splits):
    if isinstance(splits, bool) or not isinstance(splits, int) or not 0 <= splits <= EVAL_MAX_SPLITS:
        raise ValueError('%s: splits must be an integer in [0, %d], 0 = the library\'s choice (got %r)'
                         % (name, EVAL_MAX_SPLITS, splits))


# ----------------------------------------------------------------------------
# evaluation: FID statistics (sbagan/fid.py)
def _fid_need_moments(name, x_device, sum, gram):
    for what, t, dim in (('sum', sum, 1), ('gram', gram, 2)):
        _vis_need(name, t, what, torch.float64, dim)
        if x_device is not None and t.device != x_device:
            raise ValueError('%s: %s is on %s, x on %s' % (name, what, t.device, x_device))
    D = sum.shape[0]
    if D < 64 or D % 64:
        raise ValueError('%s: D must be a positive multiple of 64 (got %d)' % (name, D))
    if tuple(gram.shape) != (D, D) or gram.device != sum.device:
        raise ValueError('%s: gram must be [%d][%d] on %s (got %s on %s)'
                         % (name, D, D, sum.device, tuple(gram.shape), gram.device))
    return D


def fid_accumulate(x, sum, gram):
    """sum += x.sum(0) and gram += x^T x in float64, in place (sba_fid_accumulate): x [n][D] f32 rows on the device (unit
    column stride, row stride >= D and a multiple of 4, 16-byte aligned), sum [D] and gram [D][D] contiguous f64 on the
    same device, D % 64 == 0, n >= 1.  Only the upper-triangular 64 x 64 tiles of gram are updated.  No atomics, a fixed
    summation order.  Everything is checked before the launch: TypeError for a dtype, ValueError for a shape, a stride
    or an alignment."""
    _feature_tensor('fid_accumulate', x, 'x')           # (what x is comes before the moments, its shape after them)
    D = _fid_need_moments('fid_accumulate', x.device, sum, gram)
    n, _, ldx = _feature_rows('fid_accumulate', x, 'x', D=D)
    call('sba_fid_accumulate', _p(x), n, D, ldx, _p(sum), _p(gram), _stream())


def fid_finalize(sum, gram, n):
    """(mu [D], sigma [D][D], trace [1]), f64 on the device, from fid_accumulate's moments of n >= 2 rows
    (sba_fid_finalize): mu = sum / n, sigma = (gram - sum sum^T / n) / (n - 1) as the full matrix, its lower triangle a
    bitwise copy of the upper, trace = sum_i sigma_ii in a fixed order.  Reads the upper triangle of gram only."""
    D = _fid_need_moments('fid_finalize', None, sum, gram)
    n = int(n)
    if n < 2:
        raise ValueError('fid_finalize: a covariance needs n >= 2 rows (got %d)' % n)
    mu = torch.empty(D, dtype=torch.float64, device=sum.device)
    sigma = torch.empty((D, D), dtype=torch.float64, device=sum.device)
    trace = torch.empty(1, dtype=torch.float64, device=sum.device)
    call('sba_fid_finalize', _p(sum), _p(gram), n, D, _p(mu), _p(sigma), _p(trace), _stream())
    return mu, sigma, trace


# ----------------------------------------------------------------------------
# evaluation: k-NN manifold metrics (sbagan/prdc.py)
PRDC_MAX_K = 8


def _prdc_workspace(name, na, nb, splits, device):
    """(workspace tensor or None, its size in bytes) for a launch over na x nb rows"""
    _eval_splits(name, splits)
    nbytes = int(_lib.lib.sba_prdc_workspace_bytes(na, nb, splits))
    if nbytes < 0:
        raise ValueError('%s: no workspace size for %d x %d rows in %d splits' % (name, na, nb, splits))
    if nbytes == 0:
        return None, 0
    return torch.empty(nbytes // 8, dtype=torch.float64, device=device), nbytes


def prdc_knn_radius(x, k, splits=0):
    """radius2 [n] f64: the k-th smallest squared distance from every row of x [n][D] to the OTHER rows of x, in float64
    (sba_prdc_knn_radius).  x: f32 rows on the device, unit column stride, row stride >= D and a multiple of 4, 16-byte
    aligned, D % 64 == 0; 1 <= k <= 8, n >= k + 1.  Self is excluded by index: a duplicate row counts at distance 0.
    splits: column parts of the launch (0 = the library's choice); the result has the same bits for every value.  The
    workspace is a torch allocation on the current stream; no host sync.  Everything is checked before the launch:
    TypeError for a dtype, ValueError for a shape, a stride, an alignment, k or splits."""
    n, D, ld = _feature_rows('prdc_knn_radius', x, 'x')
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= PRDC_MAX_K:
        raise ValueError('prdc_knn_radius: k must be an integer in [1, %d] (got %r)' % (PRDC_MAX_K, k))
    if n < k + 1:
        raise ValueError('prdc_knn_radius: the %d-th neighbour needs at least %d rows (got %d)' % (k, k + 1, n))
    ws, nbytes = _prdc_workspace('prdc_knn_radius', n, n, splits, x.device)
    radius2 = torch.empty(n, dtype=torch.float64, device=x.device)
    call('sba_prdc_knn_radius', _p(x), n, D, ld, k, splits, _p(radius2), _p(ws), nbytes, _stream())
    return radius2


def prdc_ball_counts(a, b, radius_a=None, radius_b=None, splits=0):
    """(in_b, in_own), int32 [na] each or None (sba_prdc_ball_counts): for every row i of a [na][D],
    in_b[i] = #{j : d2(i, j) <= radius_b[j]} and in_own[i] = #{j : d2(i, j) <= radius_a[i]} over the rows j of b [nb][D],
    d2 the float64 squared distance of prdc_knn_radius.  radius_a [na] / radius_b [nb]: contiguous f64 on the rows'
    device; a count whose radius vector is None is not computed and comes back as None (one of the two is needed).
    Rows, splits, workspace and refusals as in prdc_knn_radius."""
    name = 'prdc_ball_counts'
    na, D, lda = _feature_rows(name, a, 'a')
    nb, _, ldb = _feature_rows(name, b, 'b', a.device, D)
    if radius_a is None and radius_b is None:
        raise ValueError('%s: one of radius_a and radius_b is needed' % name)
    for what, r, n in (('radius_a', radius_a, na), ('radius_b', radius_b, nb)):
        if r is None:
            continue
        _vis_need(name, r, what, torch.float64, 1)
        if r.shape[0] != n or r.device != a.device:
            raise ValueError('%s: %s must be [%d] on %s (got %s on %s)' % (name, what, n, a.device, tuple(r.shape), r.device))
    ws, nbytes = _prdc_workspace(name, na, nb, splits, a.device)
    in_b = torch.empty(na, dtype=torch.int32, device=a.device) if radius_b is not None else None
    in_own = torch.empty(na, dtype=torch.int32, device=a.device) if radius_a is not None else None
    call('sba_prdc_ball_counts', _p(a), na, lda, _p(b), nb, ldb, D, _p(radius_a), _p(radius_b), splits, _p(in_b),
         _p(in_own), _p(ws), nbytes, _stream())
    return in_b, in_own


# ----------------------------------------------------------------------------
# evaluation: nearest rows of another set (sbagan/nearest.py)
KNN_MAX_K = 8


def knn_topk(a, b, k, splits=0):
    """(d2 f64 [na][k], idx int32 [na][k]) on the device (sba_knn_topk): for every row i of a [na][D] the k rows j of
    b [nb][D] with the smallest (d2(i, j), j), ascending; d2 the float64 squared distance of prdc_knn_radius, bit for
    bit.  A tie goes to the smaller j; a NaN (or +inf) d2 is never listed; where b has fewer than k listable rows the
    tail is d2 = +inf, idx = -1.  a, b: f32 rows on one device, unit column stride, row stride >= D and a multiple of 4,
    16-byte aligned, D % 64 == 0; 1 <= k <= 8.  splits: column parts of the launch (0 = the library's choice); the result
    has the same bits and indices for every value.  The workspace is a torch allocation on the current stream; no host
    sync.  Everything is checked before the launch: TypeError for a dtype, ValueError for a shape, a stride, an
    alignment, k or splits."""
    na, D, lda = _feature_rows('knn_topk', a, 'a')
    nb, _, ldb = _feature_rows('knn_topk', b, 'b', a.device, D)
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= KNN_MAX_K:
        raise ValueError('knn_topk: k must be an integer in [1, %d] (got %r)' % (KNN_MAX_K, k))
    _eval_splits('knn_topk', splits)
    nbytes = int(_lib.lib.sba_knn_workspace_bytes(na, nb, k, splits))
    if nbytes < 0:
        raise ValueError('knn_topk: no workspace size for %d x %d rows, k = %d, in %d splits' % (na, nb, k, splits))
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=a.device) if nbytes else None
    d2 = torch.empty((na, k), dtype=torch.float64, device=a.device)
    idx = torch.empty((na, k), dtype=torch.int32, device=a.device)
    call('sba_knn_topk', _p(a), na, lda, _p(b), nb, ldb, D, k, splits, _p(d2), _p(idx), _p(ws), nbytes, _stream())
    return d2, idx


# ----------------------------------------------------------------------------
# evaluation: cross-modal retrieval ranks of the DAMSM encoders (sbagan/retrieval.py)
def _retrieval_workspace(name, na, nb, splits, device):
    """(workspace tensor or None, its size in bytes) for a launch over na x nb rows"""
    _eval_splits(name, splits)
    nbytes = int(_lib.lib.sba_retrieval_workspace_bytes(na, nb, splits))
    if nbytes < 0:
        raise ValueError('%s: no workspace size for %d x %d rows in %d splits' % (name, na, nb, splits))
    if nbytes == 0:
        return None, 0
    return torch.empty(nbytes // 8, dtype=torch.float64, device=device), nbytes


def _retrieval_rows(name, a, b, key_a, key_b, eps):
    na, D, lda = _feature_rows(name, a, 'a')
    nb, _, ldb = _feature_rows(name, b, 'b', a.device, D)
    for what, v, n in (('key_a', key_a, na), ('key_b', key_b, nb)):
        _retrieval_vector(name, v, what, torch.int32, n, a.device)
    eps = float(eps)
    if not eps > 0.0:
        raise ValueError('%s: eps must be positive (got %r)' % (name, eps))
    return na, nb, D, lda, ldb, eps


def _retrieval_vector(name, v, what, dtype, n, device):
    _vis_need(name, v, what, dtype, 1)
    if v.shape[0] != n or v.device != device:
        raise ValueError('%s: %s must be [%d] on %s (got %s on %s)' % (name, what, n, device, tuple(v.shape), v.device))


def retrieval_own_best(a, b, key_a, key_b, eps=1e-8, splits=0):
    """best [na] f64 (sba_retrieval_own_best): for every row i of a [na][D] the largest float64 cosine score
    s(i, j) = a_i . b_j / max(sqrt(|a_i|^2 |b_j|^2), eps) over the rows j of b [nb][D] with key_b[j] == key_a[i]; -inf
    when there is none, NaN when any such score is NaN.  a, b: f32 rows on the device, unit column stride, row stride >= D
    and a multiple of 4, 16-byte aligned, D % 64 == 0; key_a [na], key_b [nb]: contiguous int32 on the same device (only
    compared).  s(i, j) has the same bits for every split count and whichever set is `a`.  The workspace is a torch
    allocation on the current stream; no host sync.  Everything is checked before the launch: TypeError for a dtype,
    ValueError for a shape, a stride, an alignment, eps or splits."""
    name = 'retrieval_own_best'
    na, nb, D, lda, ldb, eps = _retrieval_rows(name, a, b, key_a, key_b, eps)
    ws, nbytes = _retrieval_workspace(name, na, nb, splits, a.device)
    best = torch.empty(na, dtype=torch.float64, device=a.device)
    call('sba_retrieval_own_best', _p(a), na, lda, _p(b), nb, ldb, D, _p(key_a), _p(key_b), eps, splits, _p(best), _p(ws),
         nbytes, _stream())
    return best


def retrieval_counts(a, b, key_a, key_b, best, cls_a=None, cls_b=None, eps=1e-8, splits=0):
    """(above, above_masked), int32 [na] each (sba_retrieval_counts): above[i] = #{j : key_b[j] != key_a[i] and
    NOT (s(i, j) < best[i])} over the rows j of b -- a tie counts and so does a NaN on either side -- and above_masked[i]
    the same count over the rows whose class differs as well (cls_b[j] != cls_a[i]); None when cls_a and cls_b are None
    (they go together).  best [na]: contiguous f64, retrieval_own_best's.  Rows, keys, splits, workspace and refusals as
    in retrieval_own_best."""
    name = 'retrieval_counts'
    na, nb, D, lda, ldb, eps = _retrieval_rows(name, a, b, key_a, key_b, eps)
    _retrieval_vector(name, best, 'best', torch.float64, na, a.device)
    if (cls_a is None) != (cls_b is None):
        raise ValueError('%s: cls_a and cls_b go together' % name)
    if cls_a is not None:
        _retrieval_vector(name, cls_a, 'cls_a', torch.int32, na, a.device)
        _retrieval_vector(name, cls_b, 'cls_b', torch.int32, nb, a.device)
    ws, nbytes = _retrieval_workspace(name, na, nb, splits, a.device)
    above = torch.empty(na, dtype=torch.int32, device=a.device)
    above_masked = torch.empty(na, dtype=torch.int32, device=a.device) if cls_a is not None else None
    call('sba_retrieval_counts', _p(a), na, lda, _p(b), nb, ldb, D, _p(key_a), _p(key_b), _p(cls_a), _p(cls_b), _p(best),
         eps, splits, _p(above), _p(above_masked), _p(ws), nbytes, _stream())
    return above, above_masked


# ----------------------------------------------------------------------------
# evaluation: Kernel Inception Distance (sbagan/kid.py)
KID_MAX_SUBSETS = 1024


def _kid_indices(name, idx, what, n):
    """the host int32 [subsets][m] array of an index argument, every entry checked against [0, n)"""
    if torch.is_tensor(idx):
        if idx.device.type != 'cpu':
            raise ValueError('%s: %s must be on the CPU: it is range-checked there before the upload' % (name, what))
        idx = idx.numpy()
    idx = np.asarray(idx)
    if idx.dtype not in (np.dtype(np.int32), np.dtype(np.int64)):
        raise TypeError('%s: %s must be int32 or int64 (got %s)' % (name, what, idx.dtype))
    if idx.ndim != 2 or idx.shape[0] < 1 or idx.shape[1] < 1:
        raise ValueError('%s: %s must be [subsets >= 1][m >= 1] (got %s)' % (name, what, idx.shape))
    if idx.min() < 0 or idx.max() >= n:
        raise ValueError('%s: %s holds a row number outside [0, %d)' % (name, what, n))
    return np.array(idx, dtype=np.int32, order='C')         # (a copy: the caller's array may be read-only)


def kid_kernel_sums(a, b, idx_a=None, idx_b=None, exclude_diag=False, splits=0):
    """sums [subsets] f64 on the device (sba_kid_kernel_sums): for every subset s the sum over the positions i < ma,
    j < mb of k(a[idx_a[s][i]], b[idx_b[s][j]]), k(x, y) = (x . y / D + 1)^3 in float64 on the f64 matrix instruction;
    with exclude_diag (ma == mb) the pairs of equal POSITION are left out.  a [na][D], b [nb][D]: f32 rows on the device
    as for prdc_knn_radius.  idx_a [subsets][ma], idx_b [subsets][mb]: int32 / int64 row numbers on the HOST (numpy or
    CPU tensors), range-checked here against na / nb and then uploaded; None = the rows 0 .. n - 1 for every subset
    (both None: one subset).  splits: column parts of the launch (0 = the library's choice); the sums of different
    values differ by rounding only, the same value gives the same bits.  The workspace is a torch allocation on the
    current stream; no host sync.  Everything is checked before the launch: TypeError for a dtype, ValueError for a
    shape, a stride, an alignment, an index, exclude_diag or splits."""
    name = 'kid_kernel_sums'
    na, D, lda = _feature_rows(name, a, 'a')
    nb, _, ldb = _feature_rows(name, b, 'b', a.device, D)
    _eval_splits(name, splits)
    ia = _kid_indices(name, idx_a, 'idx_a', na) if idx_a is not None else None
    ib = _kid_indices(name, idx_b, 'idx_b', nb) if idx_b is not None else None
    if ia is not None and ib is not None and ia.shape[0] != ib.shape[0]:
        raise ValueError('%s: idx_a holds %d subsets, idx_b %d' % (name, ia.shape[0], ib.shape[0]))
    subsets = ia.shape[0] if ia is not None else ib.shape[0] if ib is not None else 1
    ma = ia.shape[1] if ia is not None else na
    mb = ib.shape[1] if ib is not None else nb
    if subsets > KID_MAX_SUBSETS:
        raise ValueError('%s: at most %d subsets a launch (got %d)' % (name, KID_MAX_SUBSETS, subsets))
    if exclude_diag and ma != mb:
        raise ValueError('%s: exclude_diag pairs equal positions: ma (%d) must equal mb (%d)' % (name, ma, mb))
    nbytes = int(_lib.lib.sba_kid_workspace_bytes(ma, mb, subsets, splits))
    if nbytes < 0:
        raise ValueError('%s: no workspace size for %d x %d rows, %d subsets, %d splits' % (name, ma, mb, subsets, splits))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=a.device) if nbytes else None
    ia_dev = torch.from_numpy(ia).to(a.device) if ia is not None else None
    ib_dev = torch.from_numpy(ib).to(a.device) if ib is not None else None
    sums = torch.empty(subsets, dtype=torch.float64, device=a.device)
    call('sba_kid_kernel_sums', _p(a), na, lda, _p(ia_dev), ma, _p(b), nb, ldb, _p(ib_dev), mb, D, subsets,
         1 if exclude_diag else 0, splits, _p(sums), _p(ws), nbytes, _stream())
    return sums


# ----------------------------------------------------------------------------
# evaluation: multi-scale structural similarity of image pairs (sbagan/msssim.py)
MSSSIM_MAX_SCALES, MSSSIM_MAX_SIDE, MSSSIM_MAX_PAIRS, MSSSIM_WINDOW = 5, 1024, 1 << 20, 11


def msssim_pairs(imgs, pairs, scales=5):
    """out [P][3][scales][2] f64 on the device (sba_msssim_pairs): per pair, channel and scale the mean SSIM and the mean
    contrast-structure term over the valid positions of the 11-tap Gaussian window, all arithmetic in float64.
    imgs [n][3][H][W]: uint8, contiguous, on the device.  pairs [P][2]: image numbers, int32 or int64, a numpy array /
    CPU tensor (uploaded here) or an int32 tensor on the device of imgs; a pair that names an image outside [0, n)
    reads nothing and gives NaN.  scales: 1 .. 5, and min(H, W) >> (scales - 1) >= 11; H, W <= 1024.  The workspace
    (the workgroups' partial sums; its size does not depend on n) is a torch allocation on the current stream; no host
    sync.  Everything is checked before the launch: TypeError for a dtype, ValueError for a shape or a stride."""
    name = 'msssim_pairs'
    if not torch.is_tensor(imgs):
        raise TypeError('%s: imgs must be a tensor (got %s)' % (name, type(imgs)))
    _need_gpu(imgs)
    if imgs.dtype != torch.uint8:
        raise TypeError('%s: imgs must be uint8 (got %s)' % (name, imgs.dtype))
    if imgs.dim() != 4 or imgs.shape[1] != 3 or imgs.shape[0] < 1:
        raise ValueError('%s: imgs must be [n >= 1][3][H][W] (got %s)' % (name, tuple(imgs.shape)))
    if not imgs.is_contiguous():
        raise ValueError('%s: imgs must be contiguous (strides %s)' % (name, imgs.stride()))
    n, _, H, W = imgs.shape
    if isinstance(scales, bool) or not isinstance(scales, int) or not 1 <= scales <= MSSSIM_MAX_SCALES:
        raise ValueError('%s: scales must be an integer in [1, %d] (got %r)' % (name, MSSSIM_MAX_SCALES, scales))
    if max(H, W) > MSSSIM_MAX_SIDE or min(H, W) >> (scales - 1) < MSSSIM_WINDOW:
        raise ValueError('%s: %d x %d images do not hold the %d-tap window at %d scales (at most %d a side)'
                         % (name, H, W, MSSSIM_WINDOW, scales, MSSSIM_MAX_SIDE))
    if torch.is_tensor(pairs) and pairs.device.type != 'cpu':
        if pairs.device != imgs.device:
            raise ValueError('%s: pairs are on %s, imgs on %s' % (name, pairs.device, imgs.device))
        if pairs.dtype != torch.int32:
            raise TypeError('%s: pairs on the device must be int32 (got %s)' % (name, pairs.dtype))
        if pairs.dim() != 2 or pairs.shape[1] != 2 or not pairs.is_contiguous():
            raise ValueError('%s: pairs must be contiguous [P][2] (got %s)' % (name, tuple(pairs.shape)))
        pairs_dev = pairs
    else:
        host = np.asarray(pairs.numpy() if torch.is_tensor(pairs) else pairs)
        if host.dtype not in (np.dtype(np.int32), np.dtype(np.int64)):
            raise TypeError('%s: pairs must be int32 or int64 (got %s)' % (name, host.dtype))
        if host.ndim != 2 or host.shape[1] != 2:
            raise ValueError('%s: pairs must be [P][2] (got %s)' % (name, host.shape))
        lim = np.iinfo(np.int32)
        host = np.clip(host, lim.min, lim.max) if host.dtype != np.int32 else host   # (outside [0, n) either way)
        pairs_dev = torch.from_numpy(np.array(host, dtype=np.int32, order='C')).to(imgs.device)
    P = pairs_dev.shape[0]
    if not 1 <= P <= MSSSIM_MAX_PAIRS:
        raise ValueError('%s: 1 to %d pairs a launch (got %d)' % (name, MSSSIM_MAX_PAIRS, P))
    nbytes = int(_lib.lib.sba_msssim_workspace_bytes(H, W, P, scales))
    if nbytes < 0:
        raise ValueError('%s: no workspace size for %d pairs of %d x %d images at %d scales' % (name, P, H, W, scales))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=imgs.device)
    out = torch.empty((P, 3, scales, 2), dtype=torch.float64, device=imgs.device)
    call('sba_msssim_pairs', _p(imgs), n, H, W, _p(pairs_dev), P, scales, _p(out), _p(ws), nbytes, _stream())
    return out


# ----------------------------------------------------------------------------
# evaluation: sliced Wasserstein distance of Laplacian-pyramid patch descriptors (sbagan/swd.py)
SWD_SIZES, SWD_PATCH, SWD_DESC, SWD_MAX_PATCHES, SWD_MAX_DIRS = (32, 64, 128, 256), 7, 147, 4096, 65535
SWD_SORT_TILE = 2048            # values one workgroup sorts in LDS; longer columns are merged from sorted tiles
SWD_MEAN_CHUNK = 4096


def swd_levels(size):
    """pyramid levels of a size x size image: log2(size / 16) + 1; ValueError for a size outside SWD_SIZES"""
    if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or int(size) not in SWD_SIZES:
        raise ValueError('swd: images must be square with a side in %s (got %r)' % (SWD_SIZES, size))
    return SWD_SIZES.index(int(size)) + 2


def _swd_f64(name, what, t, shape, like=None):
    if not torch.is_tensor(t):
        raise TypeError('%s: %s must be a tensor (got %s)' % (name, what, type(t)))
    _need_gpu(t)
    if t.dtype != torch.float64:
        raise TypeError('%s: %s must be float64 (got %s)' % (name, what, t.dtype))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError('%s: %s must be %s (got %s)' % (name, what, tuple(shape), tuple(t.shape)))
    if not t.is_contiguous():
        raise ValueError('%s: %s must be contiguous (strides %s)' % (name, what, t.stride()))
    if like is not None and t.device != like.device:
        raise ValueError('%s: %s is on %s, not on %s' % (name, what, t.device, like.device))
    return t


def _swd_columns(name, D, m):
    if not 1 <= D <= SWD_MAX_DIRS or m < 1 or D * m > 1 << 40:
        raise ValueError('%s: 1 to %d columns of at least 1 value, at most 2^40 values in all (got %d x %d)'
                         % (name, SWD_MAX_DIRS, D, m))


def swd_descriptors(imgs, level, centres, desc=None):
    """(desc [n * P][147] f64, stats [6] f64) on the device (sba_swd_descriptors): the un-normalised 7 x 7 x 3 patch
    descriptors of Laplacian-pyramid level `level` (0 = finest) and, per channel, the sum and the sum of the squared
    deviations from the channel mean.  imgs
    [n][3][S][S]: uint8, contiguous, on the device, S in SWD_SIZES.  centres [n * P][2]: {x, y} per descriptor, an
    integer numpy array on the HOST (descriptor j belongs to image j // P), every value in [3, (S >> level) - 4]; the
    library checks them and uploads them on the current stream.  desc: an optional buffer to fill, [n * P][147] f64.
    Everything is checked before the launch."""
    name = 'swd_descriptors'
    if not torch.is_tensor(imgs):
        raise TypeError('%s: imgs must be a tensor (got %s)' % (name, type(imgs)))
    _need_gpu(imgs)
    if imgs.dtype != torch.uint8:
        raise TypeError('%s: imgs must be uint8 (got %s)' % (name, imgs.dtype))
    if imgs.dim() != 4 or imgs.shape[1] != 3 or imgs.shape[0] < 1 or imgs.shape[2] != imgs.shape[3]:
        raise ValueError('%s: imgs must be [n >= 1][3][S][S] (got %s)' % (name, tuple(imgs.shape)))
    if not imgs.is_contiguous():
        raise ValueError('%s: imgs must be contiguous (strides %s)' % (name, imgs.stride()))
    n, S = imgs.shape[0], imgs.shape[2]
    levels = swd_levels(S)
    if isinstance(level, bool) or not isinstance(level, (int, np.integer)) or not 0 <= level < levels:
        raise ValueError('%s: a %d px image has levels 0 .. %d (got %r)' % (name, S, levels - 1, level))
    host = np.asarray(centres)
    if host.dtype.kind not in 'iu':
        raise TypeError('%s: centres must be integers (got %s)' % (name, host.dtype))
    if host.ndim != 2 or host.shape[1] != 2 or host.shape[0] < n or host.shape[0] % n:
        raise ValueError('%s: centres must be [n * P][2] for the %d images (got %s)' % (name, n, host.shape))
    P = host.shape[0] // n
    if P > SWD_MAX_PATCHES:
        raise ValueError('%s: at most %d patches an image (got %d)' % (name, SWD_MAX_PATCHES, P))
    Sl = S >> int(level)
    if host.min() < 3 or host.max() > Sl - 4:
        raise ValueError('%s: patch centres of a %d px level must lie in [3, %d] (got %d .. %d)'
                         % (name, Sl, Sl - 4, host.min(), host.max()))
    host = np.ascontiguousarray(host, dtype=np.int32)
    if desc is None:
        desc = torch.empty((n * P, SWD_DESC), dtype=torch.float64, device=imgs.device)
    else:
        _swd_f64(name, 'desc', desc, (n * P, SWD_DESC), imgs)
    stats = torch.empty(6, dtype=torch.float64, device=imgs.device)
    nbytes = 48 * n + 8 * n * P
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=imgs.device)
    call('sba_swd_descriptors', _p(imgs), n, S, int(level), host.ctypes.data, P, _p(desc), _p(stats), _p(ws), nbytes,
         _stream())
    return desc, stats


def swd_project(desc, stats, dirs, out=None):
    """out [D][m] f64 (sba_swd_project): the descriptors desc [m][147], normalised per channel from stats [6] (the
    population mean and deviation over all m * 49 values of a channel), projected on the directions dirs [147][D]; the
    result is direction-major.  All f64 on one device; the normalisation is folded into the directions on the device."""
    name = 'swd_project'
    _swd_f64(name, 'desc', desc, None)
    if desc.dim() != 2 or desc.shape[1] != SWD_DESC or desc.shape[0] < 1:
        raise ValueError('%s: desc must be [m >= 1][%d] (got %s)' % (name, SWD_DESC, tuple(desc.shape)))
    _swd_f64(name, 'dirs', dirs, None, desc)
    if dirs.dim() != 2 or dirs.shape[0] != SWD_DESC:
        raise ValueError('%s: dirs must be [%d][D] (got %s)' % (name, SWD_DESC, tuple(dirs.shape)))
    _swd_f64(name, 'stats', stats, (6,), desc)
    m, D = desc.shape[0], dirs.shape[1]
    _swd_columns(name, D, m)
    if out is None:
        out = torch.empty((D, m), dtype=torch.float64, device=desc.device)
    else:
        _swd_f64(name, 'out', out, (D, m), desc)
    nbytes = 8 * (SWD_DESC + 1) * D
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=desc.device)
    call('sba_swd_project', _p(desc), m, _p(stats), _p(dirs), D, _p(out), _p(ws), nbytes, _stream())
    return out


def swd_sort_columns(data, tmp=None):
    """sorts every row of data [D][m] f64 (a column of m projections each) ascending, in place (sba_swd_sort_columns),
    and returns it.  tmp: a second buffer of the same shape, used when m > SWD_SORT_TILE (allocated here when missing).
    -0 and +0 compare equal; the order of NaNs is undefined."""
    name = 'swd_sort_columns'
    _swd_f64(name, 'data', data, None)
    if data.dim() != 2:
        raise ValueError('%s: data must be [D][m] (got %s)' % (name, tuple(data.shape)))
    D, m = data.shape
    _swd_columns(name, D, m)
    if m > SWD_SORT_TILE:
        if tmp is None:
            tmp = torch.empty_like(data)
        _swd_f64(name, 'tmp', tmp, (D, m), data)
        if tmp.data_ptr() == data.data_ptr():
            raise ValueError('%s: tmp must be a second buffer' % name)
    call('sba_swd_sort_columns', _p(data), _p(tmp) if m > SWD_SORT_TILE else None, D, m, _stream())
    return data


def swd_abs_mean(a, b, out=None):
    """out [D] f64 (sba_swd_abs_mean): the mean of |a - b| along every row of a, b [D][m] f64, added in a fixed order"""
    name = 'swd_abs_mean'
    _swd_f64(name, 'a', a, None)
    if a.dim() != 2:
        raise ValueError('%s: a must be [D][m] (got %s)' % (name, tuple(a.shape)))
    D, m = a.shape
    _swd_columns(name, D, m)
    _swd_f64(name, 'b', b, (D, m), a)
    if out is None:
        out = torch.empty(D, dtype=torch.float64, device=a.device)
    else:
        _swd_f64(name, 'out', out, (D,), a)
    chunks = (m + SWD_MEAN_CHUNK - 1) // SWD_MEAN_CHUNK
    ws = torch.empty(D * chunks, dtype=torch.float64, device=a.device)
    call('sba_swd_abs_mean', _p(a), _p(b), D, m, _p(out), _p(ws), 8 * D * chunks, _stream())
    return out


# ----------------------------------------------------------------------------
# training batches from the device-resident image cache (sbagan/device_data.py)
def check_pyramid_shape(T, levels):
    """ValueError unless sba_batch_pyramid takes a T px crop at `levels` scales"""
    if not 1 <= levels <= 3:
        raise ValueError('batch_pyramid: levels must be 1, 2 or 3 (got %r)' % (levels,))
    if not 4 <= T <= 1024 or T % (1 << (levels - 1)):
        raise ValueError('batch_pyramid: T must be in [4, 1024] and a multiple of %d for %d levels (got %r)'
                         % (1 << (levels - 1), levels, T))


def batch_pyramid(cache, params_host, T, levels, params_dev=None, out=None):
    """The image pyramids of one batch from a sbagan.device_data.DeviceImageCache in one launch (sba_batch_pyramid).
    params_host: int32 [B][4] = {index, x1, y1, flip} on the HOST (numpy): image `index`, window [y1, y1 + T) x
    [x1, x1 + T), mirrored when flip != 0.  Every row is checked against the cache's host size table before anything
    is uploaded: ValueError for an index or a window out of range, or a T / levels the kernel does not take.
    params_dev: the same rows already on the cache's device (the loader uploads them with its captions); otherwise
    they are uploaded here.  Returns [out_0 .. out_{levels-1}], out_l [B][3][T >> l][T >> l] float32: level 0 the
    normalised crop, the others resized from it as PIL's BILINEAR does.  out (optional): that list preallocated by the
    caller (shapes, dtype and device are checked); the launch writes into it and it is what is returned."""
    T, levels = int(T), int(levels)
    check_pyramid_shape(T, levels)
    params_host = np.ascontiguousarray(params_host)
    if params_host.dtype != np.int32 or params_host.ndim != 2 or params_host.shape[1] != 4 or params_host.shape[0] < 1:
        raise ValueError('batch_pyramid: params must be int32 [B][4], B >= 1 (got %s %s)'
                         % (params_host.dtype, params_host.shape))
    B, N = params_host.shape[0], len(cache)
    index = params_host[:, 0].astype(np.int64)
    x1, y1 = params_host[:, 1].astype(np.int64), params_host[:, 2].astype(np.int64)
    if (index < 0).any() or (index >= N).any():
        raise ValueError('batch_pyramid: image index out of range [0, %d): %s' % (N, index.tolist()))
    H, W = cache.hw_host[index, 0].astype(np.int64), cache.hw_host[index, 1].astype(np.int64)
    bad = (x1 < 0) | (y1 < 0) | (x1 + T > W) | (y1 + T > H)
    if bad.any():
        b = int(np.nonzero(bad)[0][0])
        raise ValueError('batch_pyramid: row %d: the %d px window at (x1 = %d, y1 = %d) is not inside image %d (%d x %d)'
                         % (b, T, x1[b], y1[b], index[b], H[b], W[b]))
    dev = cache.device
    _need_gpu(cache.data)
    if params_dev is None:
        params_dev = torch.from_numpy(params_host).pin_memory().to(dev, non_blocking=True)
    elif (params_dev.dtype != torch.int32 or tuple(params_dev.shape) != (B, 4) or params_dev.device != dev
          or not params_dev.is_contiguous()):
        raise ValueError('batch_pyramid: params_dev must be contiguous int32 [%d][4] on %s' % (B, dev))
    from .device_data import pyramid_tables
    tab1, tab2, lut = pyramid_tables(T, levels, dev)
    if out is None:
        outs = [torch.empty((B, 3, T >> l, T >> l), dtype=torch.float32, device=dev) for l in range(levels)]
    else:
        outs = list(out)
        if len(outs) != levels:
            raise ValueError('batch_pyramid: out must hold %d tensors (got %d)' % (levels, len(outs)))
        for l, o in enumerate(outs):
            if (not torch.is_tensor(o) or o.dtype != torch.float32 or tuple(o.shape) != (B, 3, T >> l, T >> l)
                    or o.device != dev or not o.is_contiguous()):
                raise ValueError('batch_pyramid: out[%d] must be contiguous float32 [%d][3][%d][%d] on %s'
                                 % (l, B, T >> l, T >> l, dev))
    call('sba_batch_pyramid', _p(cache.data), _p(cache.offset), _p(cache.hw), N, _p(params_dev), B, T, levels, _p(tab1),
         _p(tab2), _p(lut), _p(outs[0]), _p(outs[1]) if levels > 1 else None, _p(outs[2]) if levels > 2 else None,
         _stream())
    return outs


class ClassMask(object):
    """A same-class mask already on the device (uint8 [B][B], what miscc.losses.class_mask builds from host ids),
    handed to the losses in the `class_ids` position: the wrapper keeps a [B][B] tensor from being taken for ids."""
    __slots__ = ('tensor',)

    def __init__(self, tensor):
        if (not torch.is_tensor(tensor) or tensor.dtype != torch.uint8 or tensor.dim() != 2
                or tensor.size(0) != tensor.size(1) or not tensor.is_contiguous()):
            raise ValueError('ClassMask: needs a contiguous uint8 [B][B] tensor')
        self.tensor = tensor


def batch_masks(captions, class_ids, word_mask, class_mask):
    """Both masks of one batch in one launch (sba_batch_masks), from integers already on the device: word_mask [B][L]
    (bool or uint8) = (captions == 0), class_mask [B][B] (uint8, or a ClassMask) = same class and not the same row.
    captions int64 [B][L] and class_ids int64 [B], contiguous; the outputs are written in place and returned."""
    cm = class_mask.tensor if isinstance(class_mask, ClassMask) else class_mask
    _need_gpu(captions)
    if captions.dtype != torch.int64 or captions.dim() != 2 or not captions.is_contiguous() or captions.numel() == 0:
        raise ValueError('batch_masks: captions must be contiguous int64 [B][L], B, L >= 1')
    B, L = captions.shape
    dev = captions.device
    if class_ids.dtype != torch.int64 or tuple(class_ids.shape) != (B,) or not class_ids.is_contiguous() \
            or class_ids.device != dev:
        raise ValueError('batch_masks: class_ids must be contiguous int64 [%d] on %s' % (B, dev))
    if word_mask.dtype not in (torch.bool, torch.uint8) or tuple(word_mask.shape) != (B, L) \
            or not word_mask.is_contiguous() or word_mask.device != dev:
        raise ValueError('batch_masks: word_mask must be contiguous bool / uint8 [%d][%d] on %s' % (B, L, dev))
    if cm.dtype != torch.uint8 or tuple(cm.shape) != (B, B) or not cm.is_contiguous() or cm.device != dev:
        raise ValueError('batch_masks: class_mask must be contiguous uint8 [%d][%d] on %s' % (B, B, dev))
    call('sba_batch_masks', _p(captions), _p(class_ids), _p(word_mask), _p(cm), B, L, _stream())
    return word_mask, class_mask


# ----------------------------------------------------------------------------
# Differentiable Augmentation (csrc/diffaug.hip; sbagan/diffaug.py)
# ----------------------------------------------------------------------------
DIFFAUG_COLOR, DIFFAUG_TRANSLATION, DIFFAUG_CUTOUT = 1, 2, 4


def _diffaug_workspace(n, S, flags, device):
    """the f64 partial sums of sba_diffaug_fwd / _bwd over n images (None with color off: no reduction runs)"""
    if not flags & DIFFAUG_COLOR:
        return None
    nbytes = _lib.lib.sba_diffaug_workspace_bytes(n, S)
    if nbytes <= 0:
        raise ValueError('diffaug: %d images of side %d are not supported (S even, 8..4096; 1..65535 images)' % (n, S))
    return torch.empty(nbytes // 8, dtype=torch.float64, device=device)


class DiffAugFn(torch.autograd.Function):
    """[real | fake] -> T([real | fake]): the step's concatenation and the augmentation in one pass (sba_diffaug_fwd).
    The gradient goes to `fake` only (real images are data); when `fake` needs none -- the discriminator update's
    detached images -- the backward pass launches nothing."""

    @staticmethod
    def forward(ctx, fake, real, params, flags):
        _need_gpu(fake)
        nf, C, S, S2 = fake.shape
        nr = 0 if real is None else real.size(0)
        if C != 3 or S != S2 or fake.dtype != torch.float32 or not fake.is_contiguous():
            raise ValueError('diffaug: fake must be contiguous float32 [n][3][S][S], got %s %s'
                             % (fake.dtype, tuple(fake.shape)))
        if real is not None and (real.dtype != torch.float32 or not real.is_contiguous() or real.device != fake.device
                                 or tuple(real.shape[1:]) != (3, S, S)):
            raise ValueError('diffaug: real must be contiguous float32 [n][3][%d][%d] on %s' % (S, S, fake.device))
        if (params.dtype != torch.float32 or tuple(params.shape) != (nr + nf, 8) or not params.is_contiguous()
                or params.device != fake.device):
            raise ValueError('diffaug: params must be contiguous float32 [%d][8] on %s' % (nr + nf, fake.device))
        flags = int(flags)
        # both workspaces here, outside any later graph capture of the backward
        ws = _diffaug_workspace(nr + nf, S, flags, fake.device)
        ctx.ws_bwd = _diffaug_workspace(nf, S, flags, fake.device) if ctx.needs_input_grad[0] else None
        out = torch.empty((nr + nf, 3, S, S), dtype=torch.float32, device=fake.device)
        call('sba_diffaug_fwd', _p(real), nr, _p(fake), nf, _p(params), _p(out), S, flags, _p(ws), _stream())
        ctx.save_for_backward(params)
        ctx.geom = (nr, nf, S, flags)
        return out

    @staticmethod
    def backward(ctx, dout):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        (params,) = ctx.saved_tensors
        nr, nf, S, flags = ctx.geom
        dout = dout.float().contiguous()[nr:]            # (a contiguous batch: its tail is contiguous and 16-byte aligned)
        dx = torch.empty((nf, 3, S, S), dtype=torch.float32, device=dout.device)
        call('sba_diffaug_bwd', _p(dout), nf, _p(params[nr:]), _p(dx), S, flags, _p(ctx.ws_bwd), _stream())
        return dx, None, None, None


def diffaug(real, fake, params, flags):
    """The augmented [real | fake] batch of one discriminator pass (real = None: the fake images alone).  params: f32
    [(nr + nf)][8] uniforms in [0, 1), one row per image (sbagan.diffaug.DiffAugment); flags: DIFFAUG_* bits."""
    return DiffAugFn.apply(fake.float().contiguous(), None if real is None else real.float().contiguous(), params, flags)


class DiffAugGatedFn(torch.autograd.Function):
    """DiffAugFn with per-image flags (sba_diffaug_gated_fwd): image n gets the parts of `flags` whose gate
    gates[n][b] is below the probability p_dev holds WHEN THE KERNEL RUNS.  The forward records what it applied
    (ctx.applied, int32 [n]); the backward reads that, not p, so it is the backward of its own forward whatever the
    controller has done in between.  As with DiffAugFn, a `fake` that needs no gradient launches nothing backward."""

    @staticmethod
    def forward(ctx, fake, real, params, gates, p_dev, flags):
        _need_gpu(fake)
        nf, C, S, S2 = fake.shape
        nr = 0 if real is None else real.size(0)
        dev = fake.device
        if C != 3 or S != S2 or fake.dtype != torch.float32 or not fake.is_contiguous():
            raise ValueError('diffaug_gated: fake must be contiguous float32 [n][3][S][S], got %s %s'
                             % (fake.dtype, tuple(fake.shape)))
        if real is not None and (real.dtype != torch.float32 or not real.is_contiguous() or real.device != dev
                                 or tuple(real.shape[1:]) != (3, S, S)):
            raise ValueError('diffaug_gated: real must be contiguous float32 [n][3][%d][%d] on %s' % (S, S, dev))
        for name, t, shape in (('params', params, (nr + nf, 8)), ('gates', gates, (nr + nf, 4)), ('p_dev', p_dev, (1,))):
            if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
                raise ValueError('diffaug_gated: %s must be contiguous float32 %s on %s' % (name, list(shape), dev))
        flags = int(flags)
        # both workspaces here, outside any later graph capture of the backward
        ws = _diffaug_workspace(nr + nf, S, flags, dev)
        ctx.ws_bwd = _diffaug_workspace(nf, S, flags, dev) if ctx.needs_input_grad[0] else None
        out = torch.empty((nr + nf, 3, S, S), dtype=torch.float32, device=dev)
        applied = torch.empty(nr + nf, dtype=torch.int32, device=dev)
        call('sba_diffaug_gated_fwd', _p(real), nr, _p(fake), nf, _p(params), _p(gates), _p(p_dev), _p(out), _p(applied),
             S, flags, _p(ws), _stream())
        ctx.save_for_backward(params, applied)
        ctx.applied = applied
        ctx.geom = (nr, nf, S, flags)
        DiffAugGatedFn.last_applied = applied
        DiffAugGatedFn.applied_log.append(applied)
        return out

    last_applied = None                             # `applied` of the most recent forward, and of the last 16 (tests,
    applied_log = collections.deque(maxlen=16)      # diagnostics; under --replay: of the recording, refilled by every replay)

    @staticmethod
    def backward(ctx, dout):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        params, applied = ctx.saved_tensors
        nr, nf, S, flags = ctx.geom
        dout = dout.float().contiguous()[nr:]            # (a contiguous batch: its tail is contiguous and 16-byte aligned)
        dx = torch.empty((nf, 3, S, S), dtype=torch.float32, device=dout.device)
        call('sba_diffaug_gated_bwd', _p(dout), nf, _p(params[nr:]), _p(applied[nr:]), _p(dx), S, flags, _p(ctx.ws_bwd),
             _stream())
        return dx, None, None, None, None, None


def diffaug_gated(real, fake, params, gates, p_dev, flags):
    """ops.diffaug with each of the three parts applied to image n only where gates[n][part] < p_dev[0] (f32 [1] in
    device memory, read by the kernel): gates f32 [(nr + nf)][4] uniforms in [0, 1) (sbagan.diffaug.DiffAugment)."""
    return DiffAugGatedFn.apply(fake.float().contiguous(), None if real is None else real.float().contiguous(), params,
                                gates, p_dev, flags)


def ada_count(prob, counters_row):
    """counters_row (int32 [4]: pos, neg, cnt, calls) += the signs of prob - 0.5 over the contiguous f32 vector `prob`
    (sba_ada_count: one tiny launch on the current stream, no host sync)"""
    if prob.dtype != torch.float32 or prob.dim() != 1 or not prob.is_contiguous() or prob.numel() < 1:
        raise ValueError('ada_count: prob must be a contiguous float32 vector')
    if counters_row.dtype != torch.int32 or tuple(counters_row.shape) != (4,) or not counters_row.is_contiguous() \
            or counters_row.device != prob.device:
        raise ValueError('ada_count: counters_row must be contiguous int32 [4] on %s' % prob.device)
    call('sba_ada_count', _p(prob), prob.numel(), _p(counters_row), _stream())


def ada_adjust(p, rt, counters, interval, target, adjust, p_max):
    """one controller update of every row whose `calls` has reached `interval` (sba_ada_adjust): p [nD], rt [nD] f32,
    counters int32 [nD][4], all in device memory; one launch on the current stream, no host sync"""
    nD = p.numel()
    for name, t, dtype, shape in (('p', p, torch.float32, (nD,)), ('rt', rt, torch.float32, (nD,)),
                                  ('counters', counters, torch.int32, (nD, 4))):
        if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != p.device:
            raise ValueError('ada_adjust: %s must be contiguous %s %s on %s' % (name, dtype, list(shape), p.device))
    call('sba_ada_adjust', _p(p), _p(rt), _p(counters), nD, int(interval), float(target), float(adjust), float(p_max),
         _stream())


# ----------------------------------------------------------------------------
# Geometric augmentation (csrc/geoaug.hip; sbagan/geoaug.py)
# ----------------------------------------------------------------------------
GEOAUG_FLIP, GEOAUG_ROT90, GEOAUG_SCALE, GEOAUG_ROTATE = 1, 2, 4, 8


def geoaug_prepare(uniforms, gates, p_dev, rows_per_p, flags, mats, applied):
    """mats [N][4] and applied [N] (int32) from uniforms [N][8]: the one launch of sba_geoaug_prepare on the current
    stream.  gates [N][4] and p_dev [nP] (row r reads p_dev[r // rows_per_p]) gate each part per row; both None: every
    part of `flags` (GEOAUG_* bits) on every row."""
    _need_gpu(uniforms)
    N, dev = uniforms.size(0), uniforms.device
    need = [('uniforms', uniforms, torch.float32, (N, 8)), ('mats', mats, torch.float32, (N, 4)),
            ('applied', applied, torch.int32, (N,))]
    if (gates is None) != (p_dev is None):
        raise ValueError('geoaug_prepare: gates and p_dev go together')
    if gates is not None:
        rows_per_p = int(rows_per_p)
        if rows_per_p < 1 or p_dev.dim() != 1 or p_dev.numel() * rows_per_p < N:
            raise ValueError('geoaug_prepare: %d rows at %d rows per p need more than %d values of p'
                             % (N, rows_per_p, p_dev.numel()))
        need += [('gates', gates, torch.float32, (N, 4)), ('p_dev', p_dev, torch.float32, tuple(p_dev.shape))]
    for name, t, dtype, shape in need:
        if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
            raise ValueError('geoaug_prepare: %s must be contiguous %s %s on %s' % (name, dtype, list(shape), dev))
    call('sba_geoaug_prepare', _p(uniforms), _p(gates), _p(p_dev), int(rows_per_p) if gates is not None else 1, N,
         int(flags), _p(mats), _p(applied), _stream())


class GeoAugFn(torch.autograd.Function):
    """[real | fake] -> W([real | fake]): the step's concatenation and the per-image affine warp in one pass
    (sba_geoaug_fwd).  The map is linear: no input is saved, the backward is its exact adjoint (sba_geoaug_bwd) on the
    fake rows' matrices.  The gradient goes to `fake` only; when `fake` needs none the backward launches nothing."""

    @staticmethod
    def forward(ctx, fake, real, mats):
        _need_gpu(fake)
        nf, C, S, S2 = fake.shape
        nr = 0 if real is None else real.size(0)
        if C != 3 or S != S2 or fake.dtype != torch.float32 or not fake.is_contiguous():
            raise ValueError('geoaug: fake must be contiguous float32 [n][3][S][S], got %s %s'
                             % (fake.dtype, tuple(fake.shape)))
        if real is not None and (real.dtype != torch.float32 or not real.is_contiguous() or real.device != fake.device
                                 or tuple(real.shape[1:]) != (3, S, S)):
            raise ValueError('geoaug: real must be contiguous float32 [n][3][%d][%d] on %s' % (S, S, fake.device))
        if (mats.dtype != torch.float32 or tuple(mats.shape) != (nr + nf, 4) or not mats.is_contiguous()
                or mats.device != fake.device):
            raise ValueError('geoaug: mats must be contiguous float32 [%d][4] on %s' % (nr + nf, fake.device))
        out = torch.empty((nr + nf, 3, S, S), dtype=torch.float32, device=fake.device)
        call('sba_geoaug_fwd', _p(real), nr, _p(fake), nf, _p(mats), _p(out), S, _stream())
        ctx.save_for_backward(mats)
        ctx.geom = (nr, nf, S)
        return out

    @staticmethod
    def backward(ctx, dout):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        (mats,) = ctx.saved_tensors
        nr, nf, S = ctx.geom
        dout = dout.float().contiguous()[nr:]            # (a contiguous batch: its tail is contiguous and 16-byte aligned)
        dx = torch.empty((nf, 3, S, S), dtype=torch.float32, device=dout.device)
        call('sba_geoaug_bwd', _p(dout), nf, _p(mats[nr:]), _p(dx), S, _stream())
        return dx, None, None


def geoaug(real, fake, mats):
    """The geometrically augmented [real | fake] batch of one discriminator pass (real = None: the fake images alone).
    mats: f32 [(nr + nf)][4], one matrix per image, as sba_geoaug_prepare writes them (sbagan.geoaug.GeoAugment)."""
    return GeoAugFn.apply(fake.float().contiguous(), None if real is None else real.float().contiguous(), mats)


# ----------------------------------------------------------------------------
# The truncation trick in W (csrc/truncation.hip; sbagan/truncation.py)
# ----------------------------------------------------------------------------
STYLE_MEAN_CHUNK = 256      # rows per float64 partial sum of sba_style_mean: part of its contract


def style_mean(w):
    """(mean64 [D] float64, mean32 [D] float32): the column means of the contiguous f32 matrix w [n][D] in the fixed order
    of sba_style_mean -- float64 partial sums over chunks of 256 rows in row order, added in chunk order, one division,
    mean32 its rounding.  One launch for n <= 256, two otherwise, on the current stream; no host sync."""
    _need_gpu(w)
    if w.dtype != torch.float32 or w.dim() != 2 or not w.is_contiguous() or w.numel() < 1:
        raise ValueError('style_mean: w must be a non-empty contiguous float32 matrix [n][D], got %s %s'
                         % (w.dtype, tuple(w.shape)))
    n, D = w.shape
    chunks = (n + STYLE_MEAN_CHUNK - 1) // STYLE_MEAN_CHUNK
    mean64 = torch.empty((D,), dtype=torch.float64, device=w.device)
    mean32 = torch.empty((D,), dtype=torch.float32, device=w.device)
    workspace = torch.empty((chunks, D), dtype=torch.float64, device=w.device) if chunks > 1 else None
    call('sba_style_mean', _p(w), n, D, _p(mean64), _p(mean32), _p(workspace), _stream())
    return mean64, mean32


def style_truncate(w, w_avg, psi, out=None):
    """w_avg + psi (w - w_avg) over the rows of the contiguous f32 matrix w [n][D] (sba_style_truncate): three separately
    rounded f32 operations, psi == 1 a bit-exact copy.  out: where to write (w itself: in place); default a new tensor.
    One launch on the current stream, no host sync; no backward."""
    _need_gpu(w)
    if w.dtype != torch.float32 or w.dim() != 2 or not w.is_contiguous() or w.numel() < 1:
        raise ValueError('style_truncate: w must be a non-empty contiguous float32 matrix [n][D], got %s %s'
                         % (w.dtype, tuple(w.shape)))
    n, D = w.shape
    if w_avg.dtype != torch.float32 or tuple(w_avg.shape) != (D,) or not w_avg.is_contiguous() or w_avg.device != w.device:
        raise ValueError('style_truncate: w_avg must be contiguous float32 [%d] on %s' % (D, w.device))
    if out is None:
        out = torch.empty_like(w)
    elif out.dtype != torch.float32 or tuple(out.shape) != (n, D) or not out.is_contiguous() or out.device != w.device:
        raise ValueError('style_truncate: out must be contiguous float32 [%d][%d] on %s' % (n, D, w.device))
    call('sba_style_truncate', _p(w), _p(w_avg), float(psi), _p(out), n, D, _stream())
    return out
