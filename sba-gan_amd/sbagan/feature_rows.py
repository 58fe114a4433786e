"""The feature rows of the real and the generated images on the device, as the evaluators that need every row keep them
(sbagan/prdc.py, sbagan/kid.py): per side one f32 [capacity][D] buffer that grows by doubling, appended to without a
host-device sync per batch.  Also the few lines those evaluators share with sbagan/fid.py."""
import torch

from . import ops

SIDES = ('real', 'fake')


def dtype_name(dtype=None):
    """the name the evaluators report a compute dtype by ('bfloat16'); None: the current compute dtype"""
    return str(dtype if dtype is not None else ops.compute_dtype()).replace('torch.', '')


def check_side(owner, side, sides=SIDES):
    if side not in sides:
        raise ValueError("%s: side must be %s (got %r)" % (owner, ' or '.join(repr(s) for s in sides), side))
    return side


def check_features(owner, feats, D):
    """feats is a batch of feature rows [B][D], f32, on the device"""
    if not torch.is_tensor(feats) or feats.dim() != 2 or feats.shape[1] != D:
        raise ValueError('%s: features must be a [B][%d] tensor (got %s)'
                         % (owner, D, tuple(feats.shape) if torch.is_tensor(feats) else type(feats)))
    ops._need_gpu(feats)
    if feats.dtype != torch.float32:
        raise TypeError('%s: features must be float32 (got %s)' % (owner, feats.dtype))


class Evaluator(object):
    """what FID, PRDC and KID do alike with their `features` callable"""

    def update(self, side, images):
        """one batch of images of either side"""
        with torch.no_grad():
            feats = self.features(images)
        self.update_features(side, feats)


class FeatureRows(object):
    """owner: the evaluator's name, for the messages; sides: the sides it keeps (sbagan/nearest.py adds 'train')"""

    def __init__(self, owner, D, capacity=256, sides=SIDES):
        if D < 64 or D % 64:
            raise ValueError('%s: D must be a positive multiple of 64 (got %d)' % (owner, D))
        if capacity < 1:
            raise ValueError('%s: capacity must be >= 1 (got %d)' % (owner, capacity))
        self.owner, self.D, self.capacity, self.sides = owner, int(D), int(capacity), tuple(sides)
        self._rows = {}                             # side -> [buffer [capacity][D], rows held]

    def _side(self, side):
        return check_side(self.owner, side, self.sides)

    def append(self, side, feats):
        """one batch of feature rows [B][D] (f32, on the device); no host-device sync"""
        side = self._side(side)
        check_features(self.owner, feats, self.D)
        held = self._rows.get(side)
        if held is None:
            held = self._rows[side] = [torch.empty((self.capacity, self.D), dtype=torch.float32, device=feats.device), 0]
        buf, n, B = held[0], held[1], feats.shape[0]
        if n + B > buf.shape[0]:
            cap = buf.shape[0]
            while cap < n + B:
                cap *= 2
            grown = torch.empty((cap, self.D), dtype=torch.float32, device=buf.device)
            grown[:n].copy_(buf[:n])
            buf = held[0] = grown
        buf[n:n + B].copy_(feats)
        held[1] = n + B

    def count(self, side):
        """rows held for a side"""
        held = self._rows.get(self._side(side))
        return held[1] if held else 0

    def rows(self, side):
        """the rows held for a side: f32 [n][D] on the device (a view of the buffer)"""
        held = self._rows.get(self._side(side))
        if held is None:
            raise RuntimeError('%s: the %s side holds no rows' % (self.owner, side))
        return held[0][:held[1]]
