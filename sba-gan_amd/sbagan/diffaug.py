"""--diffaug: Differentiable Augmentation of everything the discriminators see (Zhao et al., NeurIPS 2020, "Differentiable
Augmentation for Data-Efficient GAN Training").

The transform itself is one HIP unit (csrc/diffaug.hip, ops.diffaug).  This module owns its random input: ONE static f32
tensor of uniforms, drawn by whoever draws the step's noise -- never by the step -- so that a recorded step holds the
augmentation launches over a fixed address and every replay sees fresh draws.

Layout, per discriminator i (B = batch size), rows of 8 floats (seven uniforms, one unused):
    [i * 3B, i * 3B + 2B)      the D update: B rows for the real images, then B rows for the fake images
    [i * 3B + 2B, (i + 1) * 3B) the G term: B rows for the fake images
All rows are independent, as in the paper (it augments each call with its own draws)."""
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
    def __init__(self, policy, batch_size, n_discriminators, device):
        self.policy = str(policy)
        self.flags = parse_policy(policy)
        if batch_size < 1 or n_discriminators < 1:
            raise ValueError('DiffAugment: batch_size and n_discriminators must be positive')
        self.batch_size, self.n = int(batch_size), int(n_discriminators)
        self.uniforms = torch.zeros((self.n * 3 * self.batch_size, 8), dtype=torch.float32, device=device)

    def draw(self):
        """fresh uniforms for one step: a single launch from torch's generator of the tensor's device, no host sync"""
        self.uniforms.uniform_()

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
        return self.d_rows(i), self.flags

    def g_arg(self, i):
        """the `augment` argument of miscc.losses.generator_d_term for discriminator i"""
        return self.g_rows(i), self.flags
