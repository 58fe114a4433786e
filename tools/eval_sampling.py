#!/usr/bin/env python3
"""Two toy sampling runs with all seven evaluators on, through main.main() and through main_bert.main(), in the
deterministic mode and from fixed seeds, each in a fresh child process:

    --r_precision 4 --fid --prdc 3 --kid --kid_subsets 4 --kid_subset_size 5 --ms_ssim 2 --swd 4 --nearest 2 --nearest_show 2

at 256 px / three stages (MS-SSIM needs at least 176 px) on the toy data set of the tests: 6 test images in the classes
of tests/test_msssim_gpu.py, 4 training images.  Per run it prints the seven report lines, the bytes of the seven JSON
files, a SHA-256 of every PNG (nearest.png included), the digests of the three generator states the run leaves behind and
the number of trunk forwards.  It depends on the entry-point contract alone -- main(argv), the flags, the files -- and on
two helpers of tests/ that build the toy inputs, so the same script runs against any checkout.  A change of the
evaluation path that claims to change nothing must leave every line equal:

    python tools/eval_sampling.py > branch.txt
    python tools/eval_sampling.py --root tools/_ab/parent_tree > parent.txt      # (a checkout with its own built library)
"""
import argparse
import contextlib
import hashlib
import io
import os
import pathlib
import pickle
import subprocess
import sys
import tempfile

FLAGS = ['--r_precision', '4', '--fid', '--prdc', '3', '--kid', '--kid_subsets', '4', '--kid_subset_size', '5',
         '--ms_ssim', '2', '--swd', '4', '--nearest', '2', '--nearest_show', '2']       # (--ms_ssim: PER_CLASS of the tests)
CLASSES = [1, 1, 1, 2, 2, 3]        # of the 6 test images, as tests/test_msssim_gpu.py
STEMS = ('r_precision', 'fid', 'prdc', 'kid', 'ms_ssim', 'swd', 'nearest')
LINES = ('R-precision', 'FID', 'PRDC', 'KID', 'MS-SSIM', 'SWD', 'Nearest')
ENTRIES = ('main', 'main_bert')
CHILD_SECONDS = 240


def _digest(data):
    return hashlib.sha256(data).hexdigest()


def child(root, entry):
    for p in (os.path.join(root, 'sba-gan_amd'), os.path.join(root, 'tests')):
        sys.path.insert(0, p)
    import importlib

    import numpy as np
    import torch
    from test_host_cpu import _make_dataset
    mod = importlib.import_module(entry)
    import trainer
    from miscc.utils import weights_init
    from sbagan import ops
    from sbagan.inception_hip import InceptionHIP

    init = trainer.condGANTrainer.__init__      # (the entry points have no switch for randomly initialised encoders)

    def init_random(self, *a, **kw):
        kw['allow_random_encoders'] = True
        init(self, *a, **kw)
    trainer.condGANTrainer.__init__ = init_random
    forward, calls = InceptionHIP.forward, [0]

    def counted(runner, img, *a, **kw):
        calls[0] += 1
        return forward(runner, img, *a, **kw)
    InceptionHIP.forward = counted

    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        out = io.StringIO()
        with contextlib.redirect_stdout(out):               # (the run's other lines name the temporary directory)
            data = str(tmp / 'toy')
            _make_dataset(data, n_train=4, n_test=6)
            with open(os.path.join(data, 'test', 'class_info.pickle'), 'wb') as f:
                pickle.dump(CLASSES, f)
            extra = []
            if entry == 'main_bert':
                import model_bert as model
                from test_bert_entry_gpu import _bert_dir
                extra = ['--bert_dir', _bert_dir(tmp)]
            else:
                import model
            from miscc.config import cfg, reset_cfg
            reset_cfg()
            cfg.GAN.GF_DIM, cfg.GAN.DF_DIM, cfg.TREE.BRANCH_NUM = 32, 64, 3
            torch.manual_seed(1)
            netG = model.G_NET()
            netG.apply(weights_init)
            os.makedirs(str(tmp / 'run'))
            ckpt = str(tmp / 'run' / 'netG_epoch_0.pth')
            torch.save(netG.state_dict(), ckpt)
            yml = str(tmp / 'toy.yml')
            with open(yml, 'w') as f:
                f.write('CONFIG_NAME: toy\nDATASET_NAME: toy\nB_VALIDATION: True\nWORKERS: 0\n'
                        'TREE: {BRANCH_NUM: 3}\nTRAIN: {FLAG: False, BATCH_SIZE: 2, NET_G: "%s"}\n'
                        'GAN: {GF_DIM: 32, DF_DIM: 64}\n'
                        'TEXT: {CAPTIONS_PER_IMAGE: 2, WORDS_NUM: 8, EMBEDDING_DIM: 256}\n' % ckpt)
            reset_cfg()
            ops.set_compute_dtype(torch.bfloat16)
            ops.set_deterministic(True, 'cuda:0')
            try:
                mod.main(['--cfg', yml, '--data_dir', data] + extra + FLAGS)
            finally:
                ops.set_deterministic(False)
            states = (np.random.get_state()[1].tobytes(), torch.cuda.get_rng_state().numpy().tobytes(),
                      torch.get_rng_state().numpy().tobytes())
        lines = out.getvalue().splitlines()
        for head in LINES:
            for line in lines:
                if line.split(' ')[0] == head:
                    print('%s: %s' % (entry, line))
        out_dir = tmp / 'run' / 'netG_epoch_0' / 'valid'
        for stem in STEMS:
            print('%s: %s.json %r' % (entry, stem, (out_dir / (stem + '.json')).read_bytes()))
        for png in sorted(out_dir.rglob('*.png')):
            print('%s: %s sha256 %s' % (entry, png.relative_to(out_dir).as_posix(), _digest(png.read_bytes())))
        for name, state in zip(('numpy', 'torch.cuda', 'torch'), states):
            print('%s: %s generator state sha256 %s' % (entry, name, _digest(state)))
        print('%s: trunk forwards %d' % (entry, calls[0]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help='the checkout whose sba-gan_amd/ and tests/ are used (default: this one)')
    ap.add_argument('--child', choices=ENTRIES, help=argparse.SUPPRESS)
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    if args.child:
        return child(root, args.child)
    for entry in ENTRIES:           # one fresh process per run; a run that fails ends the listing
        cmd = [sys.executable, os.path.abspath(__file__), '--root', root, '--child', entry]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=CHILD_SECONDS)
        sys.stdout.write(done.stdout.decode())
        sys.stdout.flush()
        if done.returncode != 0:
            sys.exit('%s: the run ended with status %d' % (entry, done.returncode))


if __name__ == '__main__':
    main()
