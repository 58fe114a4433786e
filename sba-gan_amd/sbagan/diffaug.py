"""--diffaug: Differentiable Augmentation of everything the discriminators see (Zhao et al., NeurIPS 2020, "Differentiable
Augmentation for Data-Efficient GAN Training").

The transform itself is one HIP unit (csrc/diffaug.hip, ops.diffaug).  This module owns its random input: ONE static f32
tensor of uniforms, drawn by whoever draws the step's noise -- never by the step -- so that a recorded step holds the
augmentation launches over a fixed address and every replay sees fresh draws.

Layout, per discriminator i (B = batch size), rows of 8 floats (seven uniforms, one unused):
    [i * 3B, i * 3B + 2B)      the D update: B rows for the real images, then B rows for the fake images
    [i * 3B + 2B, (i + 1) * 3B) the G term: B rows for the fake images
All rows are independent, as in the paper (it augments each call with its own draws).

--diffaug_p / --ada: each of the three parts is applied to an image with probability p.  A second static
tensor, `gates` (rows of 4 floats -- three uniforms, one unused -- laid out like `uniforms`), is drawn right behind the
uniforms, and the gated kernels (ops.diffaug_gated) compare it with p[i], ONE f32 per discriminator in device memory.
With a target (--ada; Karras et al., NeurIPS 2020, "Training GANs with Limited Data") p is moved by a controller that
lives on the device as well: count_sink(i) counts the signs of discriminator i's real-row probabilities behind its loss
(ops.ada_count), adjust() -- one launch at the tail of the step -- turns the counts of every `interval` iterations into
r_t = (pos - neg) / cnt and moves p by B * interval / (kimg * 1000) towards r_t = target.  Nothing is read back: a
recorded step holds these launches like any other, and every replay moves p by itself."""
import torch

from . import ops

POLICIES = {'color': ops.DIFFAUG_COLOR, 'translation': ops.DIFFAUG_TRANSLATION, 'cutout': ops.DIFFAUG_CUTOUT}


def parse_policy(policy):
    """'color,translation,cutout' (any non-empty subset, any order) -> the flags bitmask of sba_diffaug_fwd"""
    names = [p.strip() for p in str(policy).split(',')]
    flags = 0
    for name in names:
        if name not in POLICIES:
            raise ValueError('--diffaug: unknown policy %r; valid names are %s (comma separated)'
                             % (name, ', '.join(sorted(POLICIES))))
        flags |= POLICIES[name]
    return flags


class DiffAugment(object):
    def __init__(self, policy, batch_size, n_discriminators, device, p0=None, target=None, kimg=500.0, interval=4,
                 p_max=1.0):
        """p0 None and target None: every part on every image (the ungated kernels).  p0 alone: the gated kernels at a
        fixed p = p0, no controller.  target: the controller, p starting at p0 (None: 0)."""
        self.policy = str(policy)
        self.flags = parse_policy(policy)
        if batch_size < 1 or n_discriminators < 1:
            raise ValueError('DiffAugment: batch_size and n_discriminators must be positive')
        self.batch_size, self.n = int(batch_size), int(n_discriminators)
        self.uniforms = torch.zeros((self.n * 3 * self.batch_size, 8), dtype=torch.float32, device=device)
        self.adaptive, self.gated = target is not None, target is not None or p0 is not None
        self.gates = self.p = self.rt = self.counters = None
        self.last_prob = [None] * self.n
        if not self.gated:
            return
        self.p0 = 0.0 if p0 is None else float(p0)
        self.p_max, self.interval, self.kimg = float(p_max), int(interval), float(kimg)
        self.target = None if target is None else float(target)
        if not 0.0 <= self.p_max <= 1.0 or not 0.0 <= self.p0 <= 1.0:
            raise ValueError('DiffAugment: p0 and p_max must be in [0, 1]')
        if self.adaptive:
            if not -1.0 < self.target < 1.0:
                raise ValueError('DiffAugment: target must be in (-1, 1)')
            if not 1 <= self.interval <= 1024 or not self.kimg > 0 or self.n > 8:
                raise ValueError('DiffAugment: interval must be 1..1024, kimg positive, at most 8 discriminators')
            if self.p0 > self.p_max:
                raise ValueError('DiffAugment: the initial p %g is above p_max %g' % (self.p0, self.p_max))
        # the step of p per controller update: p crosses [0, 1] in kimg thousand real images
        self.adjust_step = self.batch_size * self.interval / (self.kimg * 1000.0)
        self.gates = torch.zeros((self.n * 3 * self.batch_size, 4), dtype=torch.float32, device=device)
        self._state = torch.zeros((2, self.n), dtype=torch.float32, device=device)       # p | rt: one read-back
        self.p, self.rt = self._state[0], self._state[1]
        self.p.fill_(self.p0)
        self.counters = torch.zeros((self.n, 4), dtype=torch.int32, device=device)       # pos, neg, cnt, calls

    def draw(self):
        """fresh uniforms for one step: a single launch from torch's generator of the tensor's device, no host sync (a
        second one for the gates where there are any)"""
        self.uniforms.uniform_()
        if self.gated:
            self.gates.uniform_()

    def d_rows(self, i):
        """[2B][8]: the rows of discriminator i's update, real rows first"""
        lo = i * 3 * self.batch_size
        return self.uniforms[lo:lo + 2 * self.batch_size]

    def g_rows(self, i):
        """[B][8]: the rows of discriminator i's term of the generator loss"""
        lo = i * 3 * self.batch_size + 2 * self.batch_size
        return self.uniforms[lo:lo + self.batch_size]

    def d_arg(self, i):
        """the `augment` argument of miscc.losses.discriminator_loss for discriminator i"""
        if not self.gated:
            return self.d_rows(i), self.flags
        lo = i * 3 * self.batch_size
        return self.d_rows(i), self.flags, self.gates[lo:lo + 2 * self.batch_size], self.p[i:i + 1]

    def g_arg(self, i):
        """the `augment` argument of miscc.losses.generator_d_term for discriminator i"""
        if not self.gated:
            return self.g_rows(i), self.flags
        lo = i * 3 * self.batch_size + 2 * self.batch_size
        return self.g_rows(i), self.flags, self.gates[lo:lo + self.batch_size], self.p[i:i + 1]

    # ---- the controller (adaptive mode; no-ops otherwise) -------------------------------------------------------------
    def count_sink(self, i):
        """the `sink` of ops.d_heads for discriminator i's update: counts the real rows' probabilities into row i of
        the counters, on the stream of that update, and keeps the slices as last_prob[i]; None outside adaptive mode"""
        if not self.adaptive:
            return None

        def sink(slices):
            for s in slices:
                ops.ada_count(s, self.counters[i])
            self.last_prob[i] = slices
        return sink

    def adjust(self):
        """ONE launch for all discriminators, at the tail of the step: rows whose interval is full get a new r_t and p"""
        if self.adaptive:
            ops.ada_adjust(self.p, self.rt, self.counters, self.interval, self.target, self.adjust_step, self.p_max)

    def report(self):
        """(p, r_t) as two lists of floats: one device-to-host copy"""
        host = self._state.cpu()
        return host[0].tolist(), host[1].tolist()

    def state_dict(self):
        return {'p': self.p.cpu().clone(), 'rt': self.rt.cpu().clone(), 'counters': self.counters.cpu().clone()}

    def load_state_dict(self, state):
        """into the SAME device tensors: a recording over them stays valid"""
        for name in ('p', 'rt', 'counters'):
            dst = getattr(self, name)
            if tuple(state[name].shape) != tuple(dst.shape) or state[name].dtype != dst.dtype:
                raise ValueError('DiffAugment.load_state_dict: %s is %s %s, expected %s %s'
                                 % (name, state[name].dtype, tuple(state[name].shape), dst.dtype, tuple(dst.shape)))
        for name in ('p', 'rt', 'counters'):
            getattr(self, name).copy_(state[name])
