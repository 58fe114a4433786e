#!/usr/bin/env python3
"""One SHA-256 per output buffer of every entry point of csrc/norm_act.hip, at the cases of tests/test_norm_kernels_gpu.py
(its runners and case lists are imported: no second shape list here).  Run it once per build of the library, each in a
fresh process, and diff the two listings -- a refactor of the kernels must leave every line equal:

    python tools/norm_bytes.py > branch.txt
    SBA_LIB_PATH=tools/_ab/parent/libsbagan_hip.so python tools/norm_bytes.py > parent.txt

Part 'det': deterministic mode, every output.  Part 'default': only what no atomic order can reach -- the fused kernels
with one group, BatchNorm1d, the one-launch InstanceNorm statistics, adain_fwd, and bn_act_fwd / bn_bwd_apply /
adain_bwd_apply fed the statistics / backward sums of the deterministic part."""
import hashlib
import os
import sys
from unittest import mock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'sba-gan_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import torch  # noqa: E402

import test_norm_kernels_gpu as N  # noqa: E402

# the float64 references of results are not needed here (those of inputs -- instnorm_stats for AdaIN -- are)
N.R.bn_act_fwd = N.R.bn_act_bwd = N.R.adain_fwd = N.R.adain_bwd = mock.MagicMock()


def params_of(test, name):
    """the values of one pytest.mark.parametrize axis of a test function"""
    return next(m.args[1] for m in test.pytestmark if m.args[0] == name)


class Feed(object):
    """Deterministic part: records the statistics / backward sums in run order.  Default part: hands them back in the same
    order -- run_stats returns the recorded statistics, and the recorded sums overwrite `red` just before an apply pass.
    The `red` buffer of an apply call is found by the pointer the call passes, among the buffers zeros_guarded handed out."""
    RED_ARG = {'sba_bn_act_bwd_apply': 4, 'sba_adain_bwd_apply': 6}     # position of `red` after the entry point's name

    def __init__(self):
        self.stats, self.red, self.replay, self.guarded = [], [], False, {}
        self.run_stats, self.zeros_guarded, self.call = N.run_stats, N.zeros_guarded, N.lib().call
        N.run_stats, N.zeros_guarded, N.lib().call = self.stats_, self.zeros_, self.call_

    def stats_(self, *a):
        if self.replay:
            return self.stats.pop(0).clone()
        self.stats.append(self.run_stats(*a))
        return self.stats[-1].clone()

    def zeros_(self, n, dev):
        t = self.zeros_guarded(n, dev)
        self.guarded[t.data_ptr()] = t
        return t

    def call_(self, name, *a):
        if name in self.RED_ARG:
            red = self.guarded[a[self.RED_ARG[name]]]
            if self.replay:
                red.copy_(self.red.pop(0))
            else:
                self.red.append(red.clone())
        return self.call(name, *a)


def run_bn1d(mode, dev, B, Fd):
    code, _, T, _ = N.MODES[mode]
    Cg = Fd // 32
    y, _ = N.draw((B, Fd), 41, torch.float32, dev)
    gamma, beta, _, _ = N.params(Fd, 42, dev)
    rm, rv = (0.1 * N.fill.unit((Fd,), 44)).to(dev), (1 + 0.3 * N.fill.unit((Fd,), 45)).to(dev)
    nbt = torch.tensor([3], dtype=torch.int64, device=dev)
    mean, rstd = N.nans(Fd + N.PAD, torch.float32, dev), N.nans(Fd + N.PAD, torch.float32, dev)
    out = N.nans(B * 16 * Cg + N.PAD, T, dev)
    N.lib().call('sba_bn1d_glu_fwd', code, N.p(y), N.p(gamma), N.p(beta), N.p(rm), N.p(rv), N.p(nbt), N.p(mean), N.p(rstd),
                 N.p(out), B, Fd, N.R.EPS, N.R.MOMENTUM, N.stream())
    dout, _ = N.draw((B, 16, Cg), 46, T, dev)
    dy = N.nans(B * Fd + N.PAD, torch.float32, dev)
    dg, _ = N.prefilled(Fd, 47, dev)
    db, _ = N.prefilled(Fd, 48, dev)
    N.lib().call('sba_bn1d_glu_bwd', code, N.p(y), N.p(dout), N.p(gamma), N.p(beta), N.p(mean), N.p(rstd), N.p(dy), N.p(dg),
                 N.p(db), B, Fd, N.stream())
    return dict(out=out, mean=mean, rstd=rstd, running_mean=rm, running_var=rv, nbt=nbt, dy=dy, dgamma=dg, dbeta=db)


def listing(part, dev, ops, feed):
    det = part == 'det'

    def emit(case, bufs):
        torch.cuda.synchronize()
        for name, t in bufs.items():
            h = hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()
            print('%-8s %-44s %-14s %s' % (part, case, name, h))
        feed.guarded.clear()
        if det:
            ops.det_reset()

    def fwd_bufs(r):
        return dict(out=r.out, aux=r.aux, running_mean=r.rm, running_var=r.rv, nbt=r.nbt)

    for rows, G, C, mode in N.STATS:
        C = C or N.MODES[mode][3]
        y, _ = N.draw((G, rows, C), 3, N.MODES[mode][1], dev)
        stats = N.run_stats(mode, dev, y, rows, G, C)
        emit('bn_stats r%d-g%d-c%d-%s' % (rows, G, C, mode), dict(stats=stats) if det else {})
    for mode in N.BN_MODES:
        for case in N.FWD_CASES:
            rows, G, C, a, residual, training, cs, coff = case
            r = N.run_fwd(mode, dev, rows, G, C, a, residual=residual, training=training, cs=cs, coff=coff)
            bufs = fwd_bufs(r)
            if det and r.stats is not None:
                bufs['stats'] = r.stats
            emit('bn_act_fwd %s %s' % ('-'.join(str(v) for v in case), mode), bufs)
    for rows, C, a, mode in N.TWO_PASS:
        b = N.run_bwd(N.run_fwd(mode, dev, rows, 1, C, a), dev, 'two_pass')
        bufs = dict(dy=b.dy, dgamma=b.dg, dbeta=b.db)
        if det:
            bufs['red'] = b.red
        emit('bn_bwd two-pass r%d-c%d-a%d-%s' % (rows, C, a, mode), bufs)
    for mode in N.BN_MODES:
        for a in N.ACTS3:                                   # two groups, a channel slice of dout, dgamma = NULL
            Co = 16 if a == N.GLU else 32
            fw = N.run_fwd(mode, dev, 331, 2, 32, a)
            b = N.run_bwd(fw, dev, 'two_pass', dcs=2 * Co, dco=Co)
            # (default mode: two groups add into dgamma / dbeta by atomics -- not compared)
            emit('bn_bwd two-pass slice g2 a%d-%s' % (a, mode), dict(dy=b.dy, dgamma=b.dg, dbeta=b.db, red=b.red) if det else dict(dy=b.dy))
            b = N.run_bwd(fw, dev, 'two_pass', null_param=True)
            emit('bn_bwd two-pass null a%d-%s' % (a, mode), dict(dy=b.dy, dgamma=b.dg, dbeta=b.db))
    for mode in N.BN_MODES:
        for rows, C, a, G in N.FUSED_CASES:
            C = C or 2 * N.MODES[mode][3]
            if not det and G > 1:                           # groups add into dgamma / dbeta by atomics
                continue
            fw = N.run_fwd(mode, dev, rows, G, C, a, fused=True)
            b = N.run_bwd(fw, dev, 'fused')
            bufs = fwd_bufs(fw)
            bufs.update(dy=b.dy, dgamma=b.dg, dbeta=b.db)
            emit('bn_fused r%d-c%d-a%d-g%d-%s' % (rows, C, a, G, mode), bufs)
    for mode in N.IN_MODES:
        for B in params_of(N.test_bn1d_glu, 'B'):
            for Fd in params_of(N.test_bn1d_glu, 'Fd'):
                emit('bn1d_glu b%d-f%d-%s' % (B, Fd, mode), run_bn1d(mode, dev, B, Fd))
    for mode in N.IN_MODES:
        for n, cv, HW in N.IN_CASES:
            one_launch = n * cv >= 64 and HW >= 1024        # sba_instnorm_stats: instnorm_stats_fused_kernel
            r = N.run_instnorm(mode, dev, n, cv, HW)
            emit('instnorm n%d-cv%d-hw%d-%s' % (n, cv, HW, mode), dict(mean=r.mean, rstd=r.rstd) if det or one_launch else {})
    for mode in N.IN_MODES:
        for case in N.ADAIN_CASES:
            for acc, want in params_of(N.test_adain, 'variant'):
                r = N.run_adain(mode, dev, *case, accumulate=acc, want_dstyle=want)
                bufs = dict(('out@%d' % oco, out) for oco, out in r.outs)
                bufs.update(dh=r.dh, dstyle=r.dstyle)
                if det:
                    bufs['red'] = r.red
                emit('adain n%d-cv%d-hw%d acc%d-dstyle%d-%s' % (case + (acc, int(want), mode)), bufs)


def main():
    dev = torch.device('cuda:0')
    feed = Feed()
    print('# library: %s' % N.lib().LIB_PATH)
    with N.deterministic(dev) as ops:
        ops.det_reset()
        listing('det', dev, ops, feed)
    feed.replay = True
    from sbagan import ops
    listing('default', dev, ops, feed)
    assert not feed.stats and not feed.red, 'the two parts did not walk the same cases'


if __name__ == '__main__':
    main()
