"""--diffaug without a GPU: the float64 reference (tests/diffaug_ref.py) against a torch restatement of the paper's own
functions and its autograd, the adjoint identity, the integer maps at their edges, the error bound against an f32
emulation of the kernel's chain and five mutations of it, and the interface: header, bindings, policy, flags."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import diffaug_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_FLAGS = [1, 2, 3, 4, 5, 6, 7]


def paper_forward(x, params, flags):
    """DiffAugment_pytorch.py of Zhao et al. (rand_brightness, rand_saturation, rand_contrast, rand_translation with
    ratio 0.125, rand_cutout with ratio 0.5) in float64, with the random draws replaced by the values the uniforms of
    `params` map to: u0, u1, u2 as they are, the integer draws through diffaug_ref.int_maps."""
    n, _, S, _ = x.shape
    u = torch.from_numpy(np.asarray(params, dtype=np.float32)).double()
    maps = [R.int_maps(params[a], S, flags) for a in range(n)]
    if flags & 1:
        x = x + (u[:, 0].view(n, 1, 1, 1) - 0.5)
        x_mean = x.mean(dim=1, keepdim=True)
        x = (x - x_mean) * (u[:, 1].view(n, 1, 1, 1) * 2) + x_mean
        x_mean = x.mean(dim=[1, 2, 3], keepdim=True)
        x = (x - x_mean) * (u[:, 2].view(n, 1, 1, 1) + 0.5) + x_mean
    if flags & 2:
        translation_x = torch.tensor([m[0] for m in maps]).view(n, 1, 1)
        translation_y = torch.tensor([m[1] for m in maps]).view(n, 1, 1)
        grid_batch, grid_x, grid_y = torch.meshgrid(torch.arange(n), torch.arange(S), torch.arange(S), indexing='ij')
        grid_x = torch.clamp(grid_x + translation_x + 1, 0, S + 1)
        grid_y = torch.clamp(grid_y + translation_y + 1, 0, S + 1)
        x_pad = F.pad(x, [1, 1, 1, 1, 0, 0, 0, 0])
        x = x_pad.permute(0, 2, 3, 1).contiguous()[grid_batch, grid_x, grid_y].permute(0, 3, 1, 2)
    if flags & 4:
        cut = int(S * 0.5 + 0.5)
        offset_x = torch.tensor([m[2] for m in maps]).view(n, 1, 1)
        offset_y = torch.tensor([m[3] for m in maps]).view(n, 1, 1)
        grid_batch, grid_x, grid_y = torch.meshgrid(torch.arange(n), torch.arange(cut), torch.arange(cut), indexing='ij')
        grid_x = torch.clamp(grid_x + offset_x - cut // 2, min=0, max=S - 1)
        grid_y = torch.clamp(grid_y + offset_y - cut // 2, min=0, max=S - 1)
        mask = torch.ones(n, S, S, dtype=x.dtype)
        mask[grid_batch, grid_x, grid_y] = 0
        x = x * mask.unsqueeze(1)
    return x


def _rows(S, seed, n=200):
    rng = np.random.RandomState(seed)
    return rng, R.corner_params(S, rng, n)


@pytest.mark.parametrize('S', [8, 10, 20])
def test_reference_equals_the_papers_functions_and_their_autograd(S):
    rng, params = _rows(S, 100 + S)
    n = len(params)
    x = rng.standard_normal((n, 3, S, S))
    g = rng.standard_normal((n, 3, S, S))
    for flags in ALL_FLAGS:
        xt = torch.from_numpy(x).requires_grad_(True)
        want = paper_forward(xt, params, flags)
        (dwant,) = torch.autograd.grad(want, xt, torch.from_numpy(g))
        out, A, live = R.forward(x, params, flags)
        dx, _ = R.backward(g, params, flags)
        scale = 1.0 + np.abs(want.detach().numpy()).max()
        assert np.abs(out - want.detach().numpy()).max() <= 1e-12 * scale, flags
        assert np.abs(dx - dwant.numpy()).max() <= 1e-12 * (1.0 + np.abs(dwant.numpy()).max()), flags
        if not flags & 1:       # nothing is computed: the same numbers, not merely close ones
            assert np.array_equal(out, want.detach().numpy()) and np.array_equal(dx, dwant.numpy())
        # what is not live is exactly zero, in the reference as in the paper
        dead = ~np.broadcast_to(live[:, None], out.shape)
        assert not out[dead].any() and not want.detach().numpy()[dead].any()
    # the rows reach both ends of both integer ranges, and rectangles that leave the image
    maps = np.array([R.int_maps(p, S, 7) for p in params])
    sh, cut = R.shift_of(S), R.cut_of(S)
    assert maps[:, 0].min() == -sh and maps[:, 0].max() == sh and maps[:, 1].min() == -sh and maps[:, 1].max() == sh
    assert maps[:, 2].min() == 0 and maps[:, 2].max() == S - cut % 2 and maps[:, 3].max() == S - cut % 2


@pytest.mark.parametrize('S', [8, 10, 20])
@pytest.mark.parametrize('flags', ALL_FLAGS)
def test_adjoint_identity(S, flags):
    """the map is affine: <bwd(G), X> == <G, fwd(X) - fwd(0)>"""
    rng, params = _rows(S, 7 * S + flags, n=24)
    n = len(params)
    X, G = rng.standard_normal((n, 3, S, S)), rng.standard_normal((n, 3, S, S))
    lhs = (R.backward(G, params, flags)[0] * X).sum()
    rhs = (G * (R.forward(X, params, flags)[0] - R.forward(np.zeros_like(X), params, flags)[0])).sum()
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1.0), (lhs, rhs)


@pytest.mark.parametrize('S', [8, 10, 20, 64, 256])
def test_integer_maps_stay_in_range(S):
    sh, cut = R.shift_of(S), R.cut_of(S)
    assert sh == int(S / 8 + 0.5) and cut == S // 2
    if S == 10:
        assert cut == 5         # odd: oy, ox range over [0, S - 1]
    top = S - cut % 2
    us = [np.float32(0), np.float32(0.5), R.BELOW_ONE] + list(np.linspace(0, 1, 4099, endpoint=False).astype(np.float32))
    us += [np.nextafter(np.float32(k / (2 * sh + 1)), np.float32(d)) for k in range(1, 2 * sh + 1) for d in (0, 1)]
    seen_t, seen_o = set(), set()
    for u in us:
        ty, tx, oy, ox = R.int_maps(np.array([0, 0, 0, u, u, u, u, 0], dtype=np.float32), S, 7)
        assert ty == tx and oy == ox
        assert -sh <= ty <= sh and 0 <= oy <= top, (u, ty, oy)
        seen_t.add(ty)
        seen_o.add(oy)
    assert seen_t == set(range(-sh, sh + 1)) and seen_o == set(range(0, top + 1))
    assert R.int_maps(np.array([0] * 8, dtype=np.float32), S, 7) == (-sh, -sh, 0, 0)
    assert R.int_maps(np.array([R.BELOW_ONE] * 8, dtype=np.float32), S, 7) == (sh, sh, top, top)
    # the min() of the contract guards a u that is not below 1 (a uniform_ that returned 1.0): still in range
    assert R.int_maps(np.array([1] * 8, dtype=np.float32), S, 7) == (sh, sh, top, top)
    # the cut rectangle always meets the image (what makes the paper's clamped index grid equal to the intersection)
    for o in range(0, top + 1):
        m = R.cut_mask(S, o, o)
        assert m.any() and m.sum() == m[m.any(1)][:, m.any(0)].size


def _bound_case(S, flags, seed):
    rng, params = _rows(S, seed, n=16)
    n = len(params)
    return params, rng.standard_normal((n, 3, S, S)).astype(np.float32), \
        rng.standard_normal((n, 3, S, S)).astype(np.float32)


def _violations(S, flags, mutation, seed=11):
    params, x, g = _bound_case(S, flags, seed)
    out, A, _ = R.forward(x, params, flags)
    dx, Ab = R.backward(g, params, flags)
    f = np.abs(R.chain_forward(x, params, flags, mutation).astype(np.float64) - out) > R.bound_forward(A)
    b = np.abs(R.chain_backward(g, params, flags, mutation).astype(np.float64) - dx) > R.bound_backward(Ab)
    return int(f.sum()), int(b.sum())


@pytest.mark.parametrize('S', [8, 10, 20])
@pytest.mark.parametrize('flags', ALL_FLAGS)
def test_bound_passes_the_f32_chain(S, flags):
    assert _violations(S, flags, None) == (0, 0)
    if not flags & 1:       # exact: the bound is zero there and the chain meets it
        params, x, g = _bound_case(S, flags, 11)
        assert not R.forward(x, params, flags)[1].any() and not R.backward(g, params, flags)[1].any()


@pytest.mark.parametrize('mutation,flags,forward_fails,backward_fails', [
    ('swap_s_k', 7, True, True), ('swap_s_k', 1, True, True),
    ('contrast_per_channel', 7, True, False), ('contrast_per_channel', 1, True, False),
    ('shift_off_by_one', 7, True, True), ('shift_off_by_one', 2, True, True),
    ('drop_sum_term', 7, False, True), ('drop_sum_term', 1, False, True),
    ('cutout_before_translation', 7, True, True), ('cutout_before_translation', 6, True, True)])
@pytest.mark.parametrize('S', [8, 10, 20])
def test_bound_fails_every_mutation(S, mutation, flags, forward_fails, backward_fails):
    assert mutation in R.MUTATIONS
    f, b = _violations(S, flags, mutation)
    assert (f > 0) == forward_fails and (b > 0) == backward_fails, (f, b)


def _declared(name):
    from sbagan import _lib
    assert name in _lib.DECLS and _lib.DECLS[name].ret == 'int', '%s is not declared' % name
    return ['%s %s' % (ctext, arg) for ctext, arg, _ in _lib.DECLS[name].params]


def test_header_and_bindings_agree():
    from ctypes import c_int, c_void_p
    from sbagan import _lib
    for name in ('sba_diffaug_fwd', 'sba_diffaug_bwd'):
        args = _declared(name)
        sig = _lib.SIGNATURES[name]
        assert len(args) == len(sig), (name, args)
        for a, t in zip(args, sig):
            assert t is (c_void_p if '*' in a else c_int), (name, a, t)
            assert '*' in a or a.startswith('int '), a
        assert hasattr(_lib.lib, name)
    assert _declared('sba_diffaug_fwd')[:6] == ['const float* real', 'int nr', 'const float* fake', 'int nf',
                                                'const float* params', 'float* out']
    assert _declared('sba_diffaug_bwd')[:4] == ['const float* dout', 'int n', 'const float* params', 'float* dx']
    with open(os.path.join(ROOT, 'sba-gan_amd', 'csrc', 'Makefile')) as fh:
        assert 'diffaug.hip' in fh.read()
    # the argument checks need no device: each refusal comes back before any launch
    assert _lib.lib.sba_diffaug_workspace_bytes(40, 256) == 40 * 48 * 8
    assert _lib.lib.sba_diffaug_workspace_bytes(3, 8) == 3 * 8 and _lib.lib.sba_diffaug_workspace_bytes(3, 9) == 0


def test_policy_parsing_and_refusals():
    from sbagan import diffaug
    assert diffaug.parse_policy('color,translation,cutout') == 7
    assert diffaug.parse_policy('cutout, color') == 5 and diffaug.parse_policy('translation') == 2
    for bad in ('', 'colour', 'color,', 'color,flip', 'color translation'):
        with pytest.raises(ValueError, match='color, cutout, translation'):
            diffaug.parse_policy(bad)
    a = diffaug.DiffAugment('color,cutout', 4, 3, torch.device('cpu'))
    assert a.flags == 5 and tuple(a.uniforms.shape) == (3 * 3 * 4, 8) and a.uniforms.dtype == torch.float32
    ptr = a.uniforms.data_ptr()
    torch.manual_seed(1)
    a.draw()
    first = a.uniforms.clone()
    a.draw()
    assert a.uniforms.data_ptr() == ptr and not torch.equal(first, a.uniforms)
    assert bool((a.uniforms >= 0).all()) and bool((a.uniforms < 1).all())
    # views of the one tensor, disjoint, real rows | fake rows | G rows per discriminator
    seen = []
    for i in range(3):
        d, g = a.d_rows(i), a.g_rows(i)
        assert tuple(d.shape) == (8, 8) and tuple(g.shape) == (4, 8) and d.is_contiguous() and g.is_contiguous()
        assert d.data_ptr() == ptr + (i * 12) * 32 and g.data_ptr() == ptr + (i * 12 + 8) * 32
        assert a.d_arg(i)[1] == 5 and a.g_arg(i)[0].data_ptr() == g.data_ptr()
        seen += [d, g]
    assert sum(t.numel() for t in seen) == a.uniforms.numel()
    with pytest.raises(ValueError):
        diffaug.DiffAugment('color', 0, 3, torch.device('cpu'))


def test_step_refuses_the_two_pass_layouts():
    """at construction, before anything is built: distributed=True and force_overlap_layout with an augmentation"""
    from sbagan import diffaug
    from sbagan.trainer import GANStep
    aug = diffaug.DiffAugment('color', 2, 1, torch.device('cpu'))

    class Augmented(GANStep):
        augment = aug

    class Overlapped(Augmented):
        force_overlap_layout = True

    with pytest.raises(ValueError, match='distributed'):
        Augmented(None, None, None, 2, distributed=True)
    with pytest.raises(ValueError, match='force_overlap_layout'):
        Overlapped(None, None, None, 2)
    assert GANStep.augment is None


@pytest.mark.parametrize('module', ['main', 'main_bert', 'pretrain_DAMSM', 'pretrain_DAMSM_bert'])
def test_flag_parses_on_every_entry_point_and_defaults_to_off(module):
    import importlib
    m = importlib.import_module(module)
    assert m.parse_args([]).diffaug == ''
    assert m.parse_args(['--diffaug', 'color,translation,cutout']).diffaug == 'color,translation,cutout'
    assert m.parse_args(['--diffaug', '']).diffaug == ''
    assert m.parse_args(['--device_data', '--replay', '--diffaug', 'cutout']).diffaug == 'cutout'
    with pytest.raises(SystemExit):
        m.parse_args(['--diffaug', 'color,flip'])


def test_trainer_default_is_off():
    import trainer
    import trainer_bert
    for cls in (trainer.condGANTrainer, trainer_bert.condGANTrainer):
        assert cls.diffaug == ''
