"""The recorded DAMSM update without a GPU: the float64 references of its kernels (tests/damsm_step_ref.py) against
torch on the CPU, the declared entry points, and the flag on the four entry points."""
import os

import numpy as np
import pytest
import torch

import damsm_step_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = {'sba_embed_dropout_fwd': 9, 'sba_embed_dropout_bwd': 9, 'sba_sqnorm_partials': 5, 'sba_clip_adam_prepare': 9,
       'sba_adam_step_dscale': 13}


@pytest.mark.parametrize('N,ntoken,ninput,p', [(1, 3, 4, 0.5), (37, 11, 300, 0.3), (37, 5, 4, 0.0)])
def test_embed_dropout_reference_is_embedding_times_mask(N, ntoken, ninput, p):
    """Embedding, then x * keep * scale, with autograd, all in float64"""
    rng = np.random.RandomState(N + ninput)
    ids = rng.randint(0, ntoken, N).astype(np.int64)
    W = rng.randn(ntoken, ninput)
    keep = (rng.rand(N, ninput) >= p).astype(np.uint8)
    dout = rng.randn(N, ninput)
    scale = 1.0 / (1.0 - p)
    emb = torch.nn.Embedding(ntoken, ninput).double()
    with torch.no_grad():
        emb.weight.copy_(torch.from_numpy(W))
    out = emb(torch.from_numpy(ids)) * torch.from_numpy(keep).double() * scale
    out.backward(torch.from_numpy(dout))
    np.testing.assert_allclose(R.embed_dropout_fwd(ids, W, keep, scale), out.detach().numpy(), rtol=1e-15, atol=0)
    dW, mag, count = R.embed_dropout_bwd(ids, keep, scale, dout, ntoken)
    np.testing.assert_allclose(dW, emb.weight.grad.numpy(), rtol=1e-12, atol=1e-14)
    assert count.tolist() == np.bincount(ids, minlength=ntoken).tolist()
    assert (mag >= np.abs(dW) - 1e-12).all()


def test_embed_dropout_reference_skips_ids_out_of_range():
    ids = np.array([2, 5, -1, 0], dtype=np.int64)          # ntoken = 5: 5 and -1 are outside
    W = np.arange(20, dtype=np.float64).reshape(5, 4) + 1
    keep = np.ones((4, 4), dtype=np.uint8)
    out = R.embed_dropout_fwd(ids, W, keep, 2.0)
    assert not out[1].any() and not out[2].any() and (out[0] == W[2] * 2).all() and (out[3] == W[0] * 2).all()
    dW0 = np.full((5, 4), 0.5)
    dW, _, count = R.embed_dropout_bwd(ids, keep, 2.0, np.ones((4, 4)), 5, dW0)
    assert count.tolist() == [1, 0, 1, 0, 0]
    assert (dW[[1, 3, 4]] == 0.5).all() and (dW[[0, 2]] == 2.5).all()


@pytest.mark.parametrize('n,scale', [(1, 1.0), (257, 1e-3), (257, 10.0), (5, 0.0)])
def test_norm_reference_is_clip_grad_norm(n, scale):
    rng = np.random.RandomState(n)
    g = rng.randn(n) * scale
    p = torch.nn.Parameter(torch.zeros(n, dtype=torch.float64))
    p.grad = torch.from_numpy(g.copy())
    total = torch.nn.utils.clip_grad_norm_([p], 0.25)
    norm, coef = R.norm_and_coef(g, 0.25)
    assert abs(norm - float(total)) <= 1e-14 * max(norm, 1.0)
    np.testing.assert_allclose(p.grad.numpy(), g * coef, rtol=1e-13, atol=0)
    if scale == 0.0:
        assert norm == 0.0 and coef == 1.0


def test_new_entry_points_are_declared():
    from sbagan import _lib
    for name, nargs in NEW.items():
        assert name in _lib.DECLS and _lib.DECLS[name].ret == 'int', '%s is not declared' % name
        args = ['%s %s' % (ctext, arg) for ctext, arg, _ in _lib.DECLS[name].params]
        assert len(args) == nargs and args[-1].startswith('void*'), (name, args)
        assert len(_lib.SIGNATURES[name]) == nargs
        assert hasattr(_lib.lib, name)
    assert ('const float*', 'grad_scale_dev') in [p[:2] for p in _lib.DECLS['sba_adam_step_dscale'].params]
    with open(os.path.join(ROOT, 'sba-gan_amd', 'csrc', 'Makefile')) as f:
        assert 'damsm_step.hip' in f.read()


@pytest.mark.parametrize('module', ['main', 'main_bert', 'pretrain_DAMSM', 'pretrain_DAMSM_bert'])
def test_replay_flag_still_parses(module):
    import importlib
    m = importlib.import_module(module)
    assert m.parse_args([]).replay is False
    assert m.parse_args(['--replay']).replay is True
    a = m.parse_args(['--device_data', '--replay'])
    assert a.device_data is True and a.replay is True


def test_help_says_what_the_flag_does_in_pretraining(capsys):
    import pretrain_DAMSM
    with pytest.raises(SystemExit):
        pretrain_DAMSM.parse_args(['--help'])
    text = ' '.join(capsys.readouterr().out.split())
    assert 'DAMSMSlotStep' in text and 'Ignored by DAMSM pre-training' not in text
