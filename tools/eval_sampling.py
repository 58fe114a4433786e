#!/usr/bin/env python3
"""One toy sampling run with all four evaluators on (--fid, --prdc 5, --kid, R-precision), in the deterministic mode and
from fixed seeds: the toy setup of tests/test_kid_gpu.py.  Prints the evaluators' lines and the bytes of fid.json,
prdc.json, kid.json and r_precision.json.  Run it once per build (and, with --root, per checkout), each in a fresh process,
and diff the listings -- a refactor of the evaluation path must leave every line equal:

    python tools/eval_sampling.py > branch.txt
    SBA_LIB_PATH=tools/_ab/parent/libsbagan_hip.so python tools/eval_sampling.py --root tools/_ab/parent_tree > parent.txt
"""
import argparse
import contextlib
import io
import os
import pathlib
import sys
import tempfile

ap = argparse.ArgumentParser()
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help='the checkout whose sba-gan_amd/ and tests/ are used')
ROOT = os.path.abspath(ap.parse_args().root)
for p in (ROOT, os.path.join(ROOT, 'sba-gan_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

import test_fid_gpu as tf  # noqa: E402
import test_kid_gpu as tk  # noqa: E402


def main():
    with tempfile.TemporaryDirectory() as tmp:
        out = io.StringIO()
        with contextlib.redirect_stdout(out):               # (the data set's own lines name the temporary directory)
            make, loader, ds, ckpts = tf._rnn_setup(pathlib.Path(tmp), ('all',))
            algo, files, _, _ = tk._sample(make, loader, ds, ckpts[0], kid=True, prdc=5, fid=True, R=4)
    for line in out.getvalue().splitlines():
        if line.split(' ')[0] in ('R-precision', 'FID', 'PRDC', 'KID'):
            print(line)
    for name in ('fid.json', 'prdc.json', 'kid.json', 'r_precision.json'):
        print('%s %r' % (name, files[name]))


if __name__ == '__main__':
    main()
