"""CPU checks of the fused inference path: the oracle's eval mode against the reference's eval-mode fixtures
(tests/golden/infer_*.npz, tools/make_golden.py gen_infer), the BatchNorm fold as exact algebra, the command-line flag."""
import numpy as np
import pytest
import torch

from helpers import FULL, SMOOTH, TINY, check, g_shapes, load_golden, make_inputs
from oracle import fill
from oracle import sbagan_oracle as O

# rtol is the 5e-4 tests/test_oracle_golden.py uses for the oracle against reference fixtures, with check()'s own
# absolute floor (1e-5; 1e-4 for images, as test_oracle_golden._check_steps): held elementwise at the first stage, mu
# and logvar.  Behind the attention softmax (stages 1 / 2) a handful of isolated tanh outputs of two float32
# evaluations differ by more than any useful elementwise bound while the images agree to a relative L2 of 5e-5 ..
# 5e-4; there the check is the relative L2 alone, at 1e-3.  A wrong eval mode (batch statistics, a stale buffer)
# moves the images by O(0.1) in either measure.
IMG_L2 = 1e-3

CASES = [('infer_tiny_model.npz', TINY, 'model'), ('infer_tiny_bert.npz', TINY, 'bert'),
         ('infer_tiny_mix.npz', TINY, 'mix'), ('infer_full_model_b4.npz', FULL, 'model'),
         ('infer_full_bert_b4.npz', FULL, 'bert'), ('infer_full_mix_b4.npz', FULL, 'mix')]


@pytest.mark.parametrize('name,d,variant', CASES)
def test_oracle_eval_mode_vs_reference_fixture(golden_dir, name, d, variant):
    G = load_golden(golden_dir, name)
    B, tag = int(G['B']), int(G['tag'])
    x = make_inputs(d, B, 18, lmax=18, tag=tag)
    P = fill.fill_state_dict(g_shapes(d, 3, 'model' if variant == 'model' else 'bert'))
    z = x['z2'] if variant == 'mix' else x['z']
    with torch.no_grad():
        imgs, _, mu, lv = O.g_net(P, z, x['sent'], x['words'], x['mask'], torch.from_numpy(G['eps']), 3, variant,
                                  train=False)
    for i, im in enumerate(imgs):
        if i == 0:
            check(G, 'img0', im, rtol=5e-4, atol=1e-4)
        check(G, 'img%d' % i, im, l2tol=IMG_L2)
    check(G, 'mu', mu, rtol=5e-4)
    check(G, 'logvar', lv, rtol=5e-4)
    # eval mode leaves the running statistics alone
    Q = fill.fill_state_dict(g_shapes(d, 3, 'model' if variant == 'model' else 'bert'))
    assert all(torch.equal(P[k], Q[k]) for k in P)


# The REFERENCE's own float32 error on the full-size fixtures: relative L2 per stage between the float32 fixture and the same
# forward evaluated in float64 (measured 5.8e-7 / 2.9e-5 / 6.3e-4 bert, 5.9e-7 / 5.8e-5 / 2.5e-4 mix, 6.0e-7 / 1.6e-5 /
# 4.6e-5 model; rounded up).  tests/test_infer_gpu.py derives its f32 bounds for the bert / mix fixtures from these.
REF_F32_L2 = {'infer_full_model_b4.npz': (1e-6, 1.7e-5, 4.7e-5), 'infer_full_bert_b4.npz': (1e-6, 3e-5, 6.5e-4),
              'infer_full_mix_b4.npz': (1e-6, 6e-5, 2.6e-4)}


@pytest.mark.parametrize('name,d,variant', CASES[3:])
def test_reference_float32_error_vs_float64_oracle(golden_dir, name, d, variant):
    G = load_golden(golden_dir, name)
    x = make_inputs(d, int(G['B']), 18, lmax=18, tag=int(G['tag']))
    P = fill.fill_state_dict(g_shapes(d, 3, 'model' if variant == 'model' else 'bert'))
    P = {k: (v.double() if v.is_floating_point() else v) for k, v in P.items()}
    z = x['z2'] if variant == 'mix' else x['z']
    with torch.no_grad():
        imgs, _, _, _ = O.g_net(P, z.double(), x['sent'].double(), x['words'].double(), x['mask'],
                                torch.from_numpy(G['eps']).double(), 3, variant, train=False)
    for i, im in enumerate(imgs):
        check(G, 'img%d' % i, im, l2tol=REF_F32_L2[name][i])


def test_fold_is_exact_algebra():
    """conv(x, w') + b' == BN_eval(conv(x, w)) in float64, w' = w * gamma / sqrt(var + eps), b' = beta - mean * (...)"""
    rng = np.random.RandomState(3)
    N, Cin, O, H = 2, 5, 6, 7
    x, w = rng.randn(N, Cin, H, H), rng.randn(O, Cin, 3, 3)
    gamma, beta, mean = rng.randn(O), rng.randn(O), rng.randn(O)
    var, eps = rng.rand(O) + 0.1, 1e-5
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))

    def conv(wt):
        y = np.zeros((N, O, H, H))
        for ky in range(3):
            for kx in range(3):
                y += np.einsum('nchw,oc->nohw', xp[:, :, ky:ky + H, kx:kx + H], wt[:, :, ky, kx])
        return y
    s = gamma / np.sqrt(var + eps)
    want = (conv(w) - mean[None, :, None, None]) * s[None, :, None, None] + beta[None, :, None, None]
    got = conv(w * s[:, None, None, None]) + (beta - mean * s)[None, :, None, None]
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)


def test_cli_fused_inference_flag():
    from miscc import cli
    assert cli.options('x', 'cfg/bird_style.yml', []).fused_inference is False
    assert cli.options('x', 'cfg/bird_style.yml', ['--fused_inference']).fused_inference is True
    assert cli.options('x', 'cfg/bird_style.yml', ['--fused_inference'], bert=True).fused_inference is True
