"""What the sampling() tests of the evaluators share (a plain helper module, like attn_ref.py): the toy configuration, the
toy data set with its loader, generator checkpoints and trainer factory, and one seeded sampling run -- through the
trainer (sample) or through an entry point's main() (run_main) -- that returns the files it wrote, the generator states
it left and the number of trunk forwards it made."""
import glob
import os
import pickle
import random

import numpy as np
import torch

DEV = 'cuda:0'


def toy_cfg():
    from miscc.config import cfg, reset_cfg
    reset_cfg()
    cfg.GAN.GF_DIM, cfg.GAN.DF_DIM, cfg.TREE.BRANCH_NUM = 32, 64, 2
    cfg.TEXT.CAPTIONS_PER_IMAGE, cfg.TEXT.WORDS_NUM, cfg.TEXT.EMBEDDING_DIM = 2, 8, 256
    cfg.TRAIN.BATCH_SIZE = 2
    cfg.TRAIN.NET_E, cfg.TRAIN.NET_G, cfg.TRAIN.FLAG, cfg.CUDA, cfg.GPU_ID = '', '', False, True, 0
    return cfg


def seed_all(seed):
    for seeder in (random.seed, np.random.seed, torch.manual_seed, torch.cuda.manual_seed_all):
        seeder(seed)


class CountForwards(object):
    """counts InceptionHIP.forward calls while active"""

    def __enter__(self):
        from sbagan.inception_hip import InceptionHIP
        self.cls, self.orig, self.n = InceptionHIP, InceptionHIP.forward, 0
        counter = self

        def forward(runner, img, *args, **kwargs):
            counter.n += 1
            return counter.orig(runner, img, *args, **kwargs)
        InceptionHIP.forward = forward
        return self

    def __exit__(self, *exc):
        self.cls.forward = self.orig


def rng_states():
    return np.random.get_state(), torch.cuda.get_rng_state(), torch.get_rng_state()


def same_states(a, b):
    return (a[0][0] == b[0][0] and np.array_equal(a[0][1], b[0][1]) and a[0][2:] == b[0][2:]
            and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]))


def files_under(out_dir):
    """{path relative to out_dir: bytes} of every file below it"""
    return {os.path.relpath(f, out_dir): open(f, 'rb').read()
            for f in glob.glob(os.path.join(out_dir, '**', '*'), recursive=True) if os.path.isfile(f)}


def images(files):
    return {k: v for k, v in files.items() if k.endswith('.png')}


def setup(tmp_path, names, size=128, bert=False, classes=None):
    """the toy data set (6 test images; classes: their class ids in place of the data set's own) with images of `size`
    px (128: two stages, 256: three), its loader (shuffled for the RNN path), one copy of a seeded generator's
    checkpoint in <tmp_path>/<name>/ per name, and make(*a): the RNN or the BERT trainer on random encoders.
    Returns (make, loader, ds, checkpoint paths)."""
    from test_host_cpu import _make_dataset
    cfg = toy_cfg()
    cfg.TREE.BRANCH_NUM = {128: 2, 256: 3}[size]
    from miscc import transforms
    from miscc.utils import weights_init
    from sbagan import ops
    ops.set_compute_dtype(torch.bfloat16)
    root = str(tmp_path / ('toy' if size == 128 else 'toy%d' % size))
    _make_dataset(root, n_test=6)
    if classes is not None:
        with open(os.path.join(root, 'test', 'class_info.pickle'), 'wb') as f:
            pickle.dump(classes, f)
    tfm = transforms.Compose([transforms.Resize(int(size * 76 / 64)), transforms.RandomCrop(size),
                              transforms.RandomHorizontalFlip()])
    if bert:
        import datasets_bert
        import model_bert
        from test_bert_entry_gpu import _bert_dir
        from trainer_bert import condGANTrainer
        bert_dir = _bert_dir(tmp_path)
        ds = datasets_bert.TextDataset(root, 'test', base_size=64, transform=tfm, bert_dir=bert_dir)
        G_NET = model_bert.G_NET

        def make(*a):
            return condGANTrainer(*a, allow_random_encoders=True, bert_dir=bert_dir)
    else:
        import datasets
        import model
        from trainer import condGANTrainer
        ds = datasets.TextDataset(root, 'test', base_size=64, transform=tfm)
        G_NET = model.G_NET

        def make(*a):
            return condGANTrainer(*a, allow_random_encoders=True)
    assert ds.imsize[-1] == size
    loader = torch.utils.data.DataLoader(ds, batch_size=2, drop_last=True, shuffle=not bert)
    torch.manual_seed(1)
    netG = G_NET()
    netG.apply(weights_init)
    ckpts = []
    for d in names:
        os.makedirs(str(tmp_path / d))
        ckpts.append(str(tmp_path / d / 'netG_epoch_0.pth'))
        torch.save(netG.state_dict(), ckpts[-1])
    return make, loader, ds, ckpts


def sample(make, loader, ds, ckpt, **trainer_attrs):
    """sampling('test') from `ckpt` with the given trainer attributes, after identical seeding, in the
    deterministic-reduction mode: the generator's attention / AdaIN kernels add partial sums with f32 atomics in the
    default mode, so two runs of the SAME command differ in a few image bytes there; the byte comparisons of the tests
    need the mode in which a run is reproducible.  Returns (trainer, files, generator states after, trunk forwards)."""
    from miscc.config import cfg
    from sbagan import ops
    ops.set_deterministic(True, DEV)
    try:
        cfg.TRAIN.NET_G = ckpt
        algo = make(os.path.dirname(ckpt), loader, ds.n_words, ds.ixtoword)
        for name, value in trainer_attrs.items():
            setattr(algo, name, value)
        seed_all(100)
        with CountForwards() as count:
            out_dir = algo.sampling('test')
        return algo, files_under(out_dir), rng_states(), count.n
    finally:
        ops.set_deterministic(False)


def run_main(mod, tmp_path, name, extra, root, bert_dir=None, dtype=torch.bfloat16):
    """<mod>.main() sampling the toy data set's test split from a fresh copy of one generator checkpoint
    (<tmp_path>/netG.pth), in the deterministic-reduction mode (see sample); returns (files, generator states, trunk
    forwards)"""
    from sbagan import ops
    toy_cfg()
    ops.set_compute_dtype(dtype)
    os.makedirs(str(tmp_path / name))
    ckpt = str(tmp_path / name / 'netG_epoch_0.pth')
    torch.save(torch.load(str(tmp_path / 'netG.pth')), ckpt)
    yml = str(tmp_path / (name + '.yml'))
    with open(yml, 'w') as f:
        f.write('CONFIG_NAME: toy\nDATASET_NAME: toy\nB_VALIDATION: True\nWORKERS: 0\n'
                'TREE: {BRANCH_NUM: 2}\nTRAIN: {FLAG: False, BATCH_SIZE: 2, NET_G: "%s"}\n'
                'GAN: {GF_DIM: 32, DF_DIM: 64}\nTEXT: {CAPTIONS_PER_IMAGE: 2, WORDS_NUM: 8, EMBEDDING_DIM: 256}\n' % ckpt)
    argv = ['--cfg', yml, '--data_dir', root] + (['--bert_dir', bert_dir] if bert_dir else []) + extra
    ops.set_deterministic(True, DEV)
    try:
        with CountForwards() as count:
            mod.main(argv)
    finally:
        ops.set_deterministic(False)
    out_dir = os.path.join(os.path.dirname(ckpt), 'netG_epoch_0', 'valid')
    return files_under(out_dir), rng_states(), count.n
