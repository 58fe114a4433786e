"""--geoaug: the geometric family of Karras et al. (NeurIPS 2020, "Training GANs with Limited Data") in front of the
discriminators -- x-flip, 90-degree rotation, isotropic scaling, arbitrary rotation -- as ONE per-image affine warp with
bilinear taps and zero padding (csrc/geoaug.hip, ops.geoaug).

This module owns the random input and the matrices.  Rows are laid out like sbagan.diffaug.DiffAugment's, per
discriminator i (B = batch size):
    [i * 3B, i * 3B + 2B)        the D update: B rows for the real images, then B rows for the fake images
    [i * 3B + 2B, (i + 1) * 3B)  the G term: B rows for the fake images
`uniforms` ([nD * 3B][8] f32, five used) is drawn by whoever draws the step's noise (draw()), never by the step.
prepare() -- ONE launch, issued by the step itself ahead of its first discriminator launch -- turns every row into its
2 x 2 matrix (`mats`, [nD * 3B][4]) and records the parts it applied (`applied`, int32): a recorded step holds that
launch over fixed addresses, and every replay sees fresh draws.  The matrix does not depend on the image size, so the
same layout serves discriminators of every scale.

p (optional): the device tensor [nD] of a DiffAugment in its gated modes (--diffaug_p, --ada).  Each part is then
applied to a row of discriminator i only where its own gate (`gates`, [nD * 3B][4], drawn behind the uniforms) is
below p[i] when the prepare launch runs: geometry follows the probability the controller moves.  Without p every part
of the policy is on for every image."""
import torch

from . import ops

POLICIES = {'flip': ops.GEOAUG_FLIP, 'rot90': ops.GEOAUG_ROT90, 'scale': ops.GEOAUG_SCALE, 'rotate': ops.GEOAUG_ROTATE}


def parse_policy(policy):
    """'flip,rot90,scale,rotate' (any non-empty subset, any order) -> the flags bitmask of sba_geoaug_prepare"""
    names = [p.strip() for p in str(policy).split(',')]
    flags = 0
    for name in names:
        if name not in POLICIES:
            raise ValueError('--geoaug: unknown policy %r; valid names are %s (comma separated)'
                             % (name, ', '.join(sorted(POLICIES))))
        flags |= POLICIES[name]
    return flags


class GeoAugment(object):
    def __init__(self, policy, batch_size, n_discriminators, device, p=None):
        self.policy = str(policy)
        self.flags = parse_policy(policy)
        if batch_size < 1 or n_discriminators < 1:
            raise ValueError('GeoAugment: batch_size and n_discriminators must be positive')
        self.batch_size, self.n = int(batch_size), int(n_discriminators)
        rows = self.n * 3 * self.batch_size
        self.uniforms = torch.zeros((rows, 8), dtype=torch.float32, device=device)
        self.mats = torch.zeros((rows, 4), dtype=torch.float32, device=device)
        self.applied = torch.zeros(rows, dtype=torch.int32, device=device)
        self.gated = p is not None
        self.p, self.gates = p, None
        if self.gated:
            if p.dtype != torch.float32 or tuple(p.shape) != (self.n,) or not p.is_contiguous() \
                    or p.device != self.uniforms.device:
                raise ValueError('GeoAugment: p must be contiguous float32 [%d] on %s' % (self.n, self.uniforms.device))
            self.gates = torch.zeros((rows, 4), dtype=torch.float32, device=device)

    def draw(self):
        """fresh uniforms (and gates) for one step: one launch each from torch's generator of the tensors' device"""
        self.uniforms.uniform_()
        if self.gated:
            self.gates.uniform_()

    def prepare(self):
        """the step's one launch: every row's matrix from its uniforms, its gates and the p of its discriminator"""
        ops.geoaug_prepare(self.uniforms, self.gates, self.p, 3 * self.batch_size, self.flags, self.mats, self.applied)

    def d_mats(self, i):
        """[2B][4]: the `geo` argument of miscc.losses.discriminator_loss for discriminator i, real rows first"""
        lo = i * 3 * self.batch_size
        return self.mats[lo:lo + 2 * self.batch_size]

    def g_mats(self, i):
        """[B][4]: the `geo` argument of miscc.losses.generator_d_term for discriminator i"""
        lo = i * 3 * self.batch_size + 2 * self.batch_size
        return self.mats[lo:lo + self.batch_size]
