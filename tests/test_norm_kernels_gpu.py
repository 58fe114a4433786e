"""Every entry point of csrc/norm_act.hip called directly through the C ABI (sbagan._lib), at the smallest shape
that reaches each kernel and each branch, against the float64 references of tests/norm_ref.py evaluated on the
kernel's own (storage-rounded) inputs.

V = 4 (f32) or 8 (16-bit) elements per 16-byte vector, cv = channel vectors per row, rpi = 256 / cv rows per iteration.

kernel                         host condition that selects it                          covered by
-----------------------------  ------------------------------------------------------  ------------------------------------
bn_stats_kernel                sba_bn_stats (always)                                   test_bn_stats: cv = 1, cv = 20 / 10
                                                                                       (idle threads), one row, cv > 256
                                                                                       (channel-vector loop), two groups,
                                                                                       both workgroup caps (512, 64)
  det_part branch              deterministic mode                                      test_deterministic_bn (C = 80, 4096)
bn_act_fwd_kernel              sba_bn_act_fwd: training 1 / 0, act NONE / GLU /        test_bn_act_fwd, test_offset_inputs
                               LRELU / RELU, residual, out_cstride / out_coff
bn_bwd_reduce_kernel           sba_bn_act_bwd_reduce (ops: rows > BN_FUSED_BWD_ROWS)   test_bn_bwd_two_pass,
                                                                                       test_blocks_above_the_fused_threshold
  det_part branch              deterministic mode                                      test_deterministic_bn (3072 rows)
bn_bwd_apply_kernel            sba_bn_act_bwd_apply (same condition)                   test_bn_bwd_two_pass (C = 4096: 96 KB
                                                                                       of dynamic LDS)
  per-group relaunch           deterministic mode, groups > 1, dgamma != NULL          test_deterministic_bn (groups = 2)
bn_fwd_fused_kernel            sba_bn_act_fwd_fused (ops: small grouped maps)          test_bn_fused, test_offset_inputs
bn_bwd_fused_kernel            sba_bn_act_bwd_fused (ops: rows <= BN_FUSED_BWD_ROWS)   test_bn_fused
  per-group relaunch           deterministic mode, groups > 1, dgamma != NULL          test_deterministic_bn (fused, groups 2)
bn1d_glu_fwd_kernel            sba_bn1d_glu_fwd; B <= 32 cached, B > 32 uncached       test_bn1d_glu (B = 2 .. 32 | 33, 40)
bn1d_glu_bwd_kernel            sba_bn1d_glu_bwd; same two branches                     test_bn1d_glu
instnorm_stats_fused_kernel    sba_instnorm_stats: N * cv >= 64 and HW >= 1024         test_instnorm_stats: HW 1024 (no tail),
                                                                                       1296, 2047 (tails); test_offset_inputs
instnorm_accum_kernel +        sba_instnorm_stats otherwise                            test_instnorm_stats: HW 1023, N * cv =
instnorm_finalize_kernel                                                               56, cv = 256, cv = 1
  det branch (splits = 1)      deterministic mode                                      test_deterministic_instnorm_adain
adain_fwd_kernel               sba_adain_fwd                                           test_adain (oco = 0 and C of 2C)
adain_bwd_reduce_kernel        sba_adain_bwd_reduce                                    test_adain (dcs = 2C, dco = C)
  det branch (splits = 1)      deterministic mode                                      test_deterministic_instnorm_adain
adain_bwd_apply_kernel         sba_adain_bwd_apply: accumulate 0 / 1, dstyle or NULL   test_adain
every SBA_E_ARG condition      --                                                      test_refusals

No environment switch selects a kernel (ops.BN_FUSED_BWD_ROWS, the workgroup caps and the InstanceNorm threshold are
constants): the entry point called -- for InstanceNorm the shape -- does.

Bounds.  f32 outputs: elementwise rtol 2e-4 / atol 2e-5 (test_kernels_gpu.tol).  Per-channel sums (statistics, red,
dgamma, dbeta, dstyle): |error| <= 1e-5 x the float64 sum of the ABSOLUTE summands of that channel (f32 partial sums
are a few 1e-6 there; one dropped row of 3072 is 3e-4).  bf16 outputs: the kernels compute in f32 and round once, so
the floor is the relative L2 distance between the float64 result and that result rounded to bf16 (about 2e-3, computed
per case); allowed: twice the floor.  LeakyReLU backward: the branch per element is taken from the sign of the
kernel's own forward value, so no element is excluded.

Every output buffer is longer (and, with a channel stride, wider) than the kernel should write and is prefilled with
NaN -- dgamma / dbeta, which the kernels add to, with non-zero values in front of a NaN tail; everything outside the
window must still be NaN afterwards and everything inside finite.
"""
import contextlib
from types import SimpleNamespace as NS

import pytest
import torch

pytestmark = pytest.mark.gpu

import norm_ref as R  # noqa: E402
from helpers import rel_l2  # noqa: E402
from oracle import fill  # noqa: E402
from test_kernels_gpu import (_check_module, _load, _oracle_P, _reset_cfg, act, close, dev, rounded, tol)  # noqa: E402,F401

NAN = float('nan')
PAD = 64                                                    # guard elements behind every flat output
OFFSET = 4.0                                                # |mean| / std of the offset-input cases (see test_norm_ref_cpu)
NONE, GLU, LRELU, RELU = R.ACT_NONE, R.ACT_GLU, R.ACT_LRELU, R.ACT_RELU
ACTS3 = [NONE, GLU, LRELU]
# mode -> (dtype code, storage of the raw conv output y, storage of the activations T, V)
MODES = {'f32': (0, torch.float32, torch.float32, 4), 'bf16': (1, torch.bfloat16, torch.bfloat16, 8),
         'yh': (2, torch.float16, torch.bfloat16, 8)}
BN_MODES = ['f32', 'bf16', 'yh']
IN_MODES = ['f32', 'bf16']


def lib():
    from sbagan import _lib
    return _lib


def slots():
    return lib().lib.sba_bn_stat_slots()


def p(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------ inputs, guards, bounds
def draw(shape, tag, dt, dev, offset=0.0, scale=1.0):
    """(device tensor in storage type dt, the same values as float64 on the CPU)"""
    x = (offset + scale * fill.unit(shape, tag)).to(dt)
    return x.to(dev).contiguous(), x.double()


def params(C, tag, dev):
    g, b = 1 + 0.3 * fill.unit((C,), tag), 0.2 * fill.unit((C,), tag + 1)
    return g.to(dev), b.to(dev), g.double(), b.double()


def nans(n, dt, dev):
    return torch.full((n,), NAN, dtype=dt, device=dev)


def zeros_guarded(n, dev):
    """n zeros (a buffer the caller clears) in front of PAD NaNs"""
    t = nans(n + PAD, torch.float32, dev)
    t[:n] = 0
    return t


def prefilled(n, tag, dev):
    """non-zero values the kernel adds to, in front of PAD NaNs; (buffer, the prefill as float64)"""
    v = 0.5 + 0.25 * fill.unit((n,), tag)
    t = nans(n + PAD, torch.float32, dev)
    t[:n] = v.to(dev)
    return t, v.double()


def front(buf, n, name):
    """the first n elements (all finite) of a guarded flat buffer whose tail must still be NaN"""
    b = buf.detach().float().cpu()
    assert bool(torch.isnan(b[n:]).all()), '%s: wrote past its end' % name
    assert bool(torch.isfinite(b[:n]).all()), '%s: non-finite or unwritten values' % name
    return b[:n].double()


def window(buf, rows, cs, coff, Co, name):
    """rows x [coff, coff + Co) of a [rows + extra][cs] buffer: finite inside, NaN everywhere else"""
    v = buf.detach().float().cpu().view(-1, cs)
    inside = v[:rows, coff:coff + Co]
    assert bool(torch.isfinite(inside).all()), '%s: non-finite or unwritten values' % name
    outside = torch.ones(v.shape, dtype=torch.bool)
    outside[:rows, coff:coff + Co] = False
    assert bool(torch.isnan(v[outside]).all()), '%s: wrote outside its channel window / past the last row' % name
    return inside.double()


def elem_close(got, ref, name):
    got, ref = got.double().cpu().flatten(), ref.double().flatten()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    t = tol(torch.float32)
    err = (got - ref).abs()
    worst = float((err / (t['atol'] + t['rtol'] * ref.abs())).max())
    print('%-28s f32 elementwise: worst error / bound = %.3f' % (name, worst))
    assert worst <= 1.0, '%s: max err %.3e' % (name, float(err.max()))


def sums_close(got, ref, ref_abs, name):
    got, ref, ref_abs = got.double().cpu().flatten(), ref.double().flatten(), ref_abs.double().flatten()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    worst = float(((got - ref).abs() / ref_abs.clamp(min=1e-30)).max())
    print('%-28s per-channel sums: worst |err| / sum|summands| = %.2e' % (name, worst))
    assert worst <= 1e-5, '%s: %.3e > 1e-5' % (name, worst)


def bf16_floor(ref):
    return rel_l2(ref.to(torch.bfloat16).double(), ref)


def low_close(got, ref, name, factor=2.0):
    floor, r = bf16_floor(ref), rel_l2(got, ref)
    print('%-28s bf16 rel L2 %.3e, one-rounding floor %.3e' % (name, r, floor))
    assert r <= factor * floor, '%s: rel L2 %.3e > %g x floor %.3e' % (name, r, factor, floor)


def out_close(got, ref, T, name):
    if T == torch.float32:
        elem_close(got, ref, name)
    else:
        low_close(got.flatten(), ref.flatten(), name)


# ------------------------------------------------------------------ BatchNorm: runners
def run_stats(mode, dev, y, rows, G, C):
    stats = zeros_guarded(G * slots() * 2 * C, dev)
    lib().call('sba_bn_stats', MODES[mode][0], p(y), p(stats), rows, G, C, stream())
    return stats


def check_stats(stats, yd, G, C, name='stats'):
    got = front(stats, G * slots() * 2 * C, name).view(G, slots(), 2, C).sum(1)          # add the replicas up
    ref = R.bn_stats(yd)
    sums_close(got, ref.sums, ref.sums_abs, name)


def run_fwd(mode, dev, rows, G, C, a, residual=False, training=1, cs=None, coff=0, offset=0.0, fused=False, tag=11):
    """sba_bn_stats + sba_bn_act_fwd (or sba_bn_act_fwd_fused) on fresh inputs, and the float64 reference"""
    code, YT, T, V = MODES[mode]
    Co = C // 2 if a == GLU else C
    cs = cs or Co
    r = NS(mode=mode, rows=rows, G=G, C=C, Co=Co, act=a, cs=cs, coff=coff, T=T, training=training)
    r.y, r.yd = draw((G, rows, C), tag, YT, dev, offset)
    r.gamma, r.beta, r.gd, r.bd = params(C, tag + 1, dev)
    rm0, rv0 = 0.1 * fill.unit((C,), tag + 3), 1 + 0.3 * fill.unit((C,), tag + 4)
    r.rm, r.rv, r.nbt = rm0.to(dev), rv0.to(dev), torch.tensor([7], dtype=torch.int64, device=dev)
    res = resd = None
    if residual:
        res, resd = draw((G, rows, Co), tag + 5, T, dev)
    r.out = nans((G * rows + 3) * cs, T, dev)
    r.aux = nans(G * 4 * C + PAD, torch.float32, dev)
    r.stats = None
    if fused:
        lib().call('sba_bn_act_fwd_fused', code, p(r.y), p(r.gamma), p(r.beta), p(r.rm), p(r.rv), p(r.nbt), p(r.aux),
                   p(r.out), rows, G, C, a, cs, coff, R.EPS, R.MOMENTUM, stream())
    else:
        if training:
            r.stats = run_stats(mode, dev, r.y, rows, G, C)
        lib().call('sba_bn_act_fwd', code, p(r.y), p(r.stats), p(r.gamma), p(r.beta), p(r.rm), p(r.rv), p(r.nbt),
                   p(r.aux), p(res), p(r.out), rows, G, C, a, cs, coff, R.EPS, R.MOMENTUM, training, stream())
    torch.cuda.synchronize()
    r.ref = R.bn_act_fwd(r.yd, r.gd, r.bd, rm0, rv0, 7, a, residual=resd, training=bool(training))
    return r


def check_fwd(r, name):
    got = window(r.out, r.G * r.rows, r.cs, r.coff, r.Co, name + ' out')
    out_close(got, r.ref.out.reshape(r.G * r.rows, r.Co), r.T, name + ' out')
    aux = front(r.aux, r.G * 4 * r.C, name + ' aux').view(r.G, 4, r.C)
    for g in range(r.G):                                    # per group: scale, shift, mean, rstd
        elem_close(aux[g], r.ref.aux[g], '%s aux[%d]' % (name, g))
    elem_close(r.rm, r.ref.running_mean, name + ' running_mean')
    elem_close(r.rv, r.ref.running_var, name + ' running_var')
    assert int(r.nbt) == r.ref.nbt, (name, int(r.nbt), r.ref.nbt)
    if r.stats is not None:
        check_stats(r.stats, r.yd, r.G, r.C, name + ' stats')


def positive_of(r):
    """LeakyReLU: the branch the kernels take, from the sign of the kernel's own forward value"""
    if r.act != LRELU:
        return None
    v = r.out.detach().float().cpu().view(-1, r.cs)[:r.G * r.rows, r.coff:r.coff + r.Co]
    return (v > 0).reshape(r.G, r.rows, r.C)


def run_bwd(fw, dev, kind, dcs=None, dco=0, null_param=False, tag=31):
    """kind 'two_pass': sba_bn_act_bwd_reduce + _apply; 'fused': sba_bn_act_bwd_fused -- on the data and aux of `fw`"""
    code, YT, T, V = MODES[fw.mode]
    G, rows, C, Co, a = fw.G, fw.rows, fw.C, fw.Co, fw.act
    dcs = dcs or Co
    b = NS(fw=fw, T=T, null_param=null_param)
    b.dout, doutd = draw((G * rows, dcs), tag, T, dev)      # the channels outside [dco, dco + Co) hold other values
    b.dy = nans(G * rows * C + PAD, T, dev)
    b.dg, b.dg0 = prefilled(C, tag + 1, dev)
    b.db, b.db0 = prefilled(C, tag + 2, dev)
    dg, db = (None, None) if null_param else (b.dg, b.db)
    b.red = None
    if kind == 'two_pass':
        b.red = zeros_guarded(G * slots() * 2 * C, dev)
        lib().call('sba_bn_act_bwd_reduce', code, p(fw.y), p(b.dout), p(fw.aux), p(b.red), rows, G, C, a, dcs, dco, stream())
        lib().call('sba_bn_act_bwd_apply', code, p(fw.y), p(b.dout), p(fw.aux), p(b.red), p(b.dy), p(dg), p(db), rows, G,
                   C, a, dcs, dco, stream())
    else:
        lib().call('sba_bn_act_bwd_fused', code, p(fw.y), p(b.dout), p(fw.aux), p(b.dy), p(dg), p(db), rows, G, C, a, dcs,
                   dco, stream())
    torch.cuda.synchronize()
    b.ref = R.bn_act_bwd(fw.yd, doutd[:, dco:dco + Co].reshape(G, rows, Co), fw.ref.aux, fw.gd, fw.bd, a,
                         positive=positive_of(fw))
    return b


def check_bwd(b, name):
    fw = b.fw
    n = fw.G * fw.rows * fw.C
    out_close(front(b.dy, n, name + ' dy'), b.ref.dy, b.T, name + ' dy')
    dg, db = front(b.dg, fw.C, name + ' dgamma'), front(b.db, fw.C, name + ' dbeta')
    if b.null_param:                                        # nothing else is written
        assert torch.equal(dg, b.dg0) and torch.equal(db, b.db0), name
    else:                                                   # the kernels ADD to dgamma / dbeta
        sums_close(dg - b.dg0, b.ref.dgamma, b.ref.dgamma_abs, name + ' dgamma')
        sums_close(db - b.db0, b.ref.dbeta, b.ref.dbeta_abs, name + ' dbeta')
    if b.red is not None:
        red = front(b.red, fw.G * slots() * 2 * fw.C, name + ' red').view(fw.G, slots(), 2, fw.C)
        sums_close(red.sum(1), b.ref.red, b.ref.red_abs, name + ' red')
        return red
    return None


# ------------------------------------------------------------------ sba_bn_stats
#              rows  groups  C (None: V)  modes
STATS_CASES = [(331, 1, None, BN_MODES), (331, 1, 80, BN_MODES), (1, 1, 64, BN_MODES), (331, 1, 4096, BN_MODES),
               (77, 2, 64, BN_MODES),
               (4100, 1, 1024, ['f32']), (520, 8, 1024, ['f32'])]       # cv = 256: 513 > 512 and 65 > 64 workgroups asked for
STATS = [(rows, G, C, m) for rows, G, C, modes in STATS_CASES for m in modes]


@pytest.mark.parametrize('case', STATS, ids=lambda c: 'r%d-g%d-c%s-%s' % c)
def test_bn_stats(dev, case):
    rows, G, C, mode = case
    C = C or MODES[mode][3]
    y, yd = draw((G, rows, C), 3, MODES[mode][1], dev)
    stats = run_stats(mode, dev, y, rows, G, C)
    torch.cuda.synchronize()
    check_stats(stats, yd, G, C)


# ------------------------------------------------------------------ sba_bn_act_fwd
#            rows      G  C     act    residual training cstride coff
FWD_CASES = [(331, 1, 64, NONE, False, 1, None, 0), (331, 1, 64, NONE, True, 1, None, 0), (331, 1, 64, GLU, False, 1, None, 0),
             (331, 1, 64, LRELU, False, 1, None, 0), (331, 1, 64, RELU, False, 1, None, 0),
             (331, 2, 64, GLU, False, 1, None, 0), (331, 2, 64, LRELU, False, 1, None, 0),
             (331, 1, 64, LRELU, False, 0, None, 0), (331, 2, 64, GLU, False, 0, None, 0),       # eval mode
             (331, 1, 80, RELU, False, 1, 192, 96),         # the Inception concat pattern
             # the widest BatchNorm2d of the networks: nets.D_NET256.img_code_s64 = downBlock(ndf * 16, ndf * 32) = 2048
             # channels + LeakyReLU on a 4x4 map at DF_DIM = 64 (the widest GLU one is INIT_STAGE_G.upsample1 = upBlock(16 ngf,
             # 8 ngf): 16 ngf = 1024 channels at GF_DIM = 64); both activations at that width
             (20 * 16, 1, 2048, LRELU, False, 1, None, 0), (20 * 16, 1, 2048, GLU, False, 1, None, 0)]


@pytest.mark.parametrize('mode', BN_MODES)
@pytest.mark.parametrize('case', FWD_CASES, ids=lambda c: 'r%d-g%d-c%d-a%d-res%d-t%d-cs%s-co%d' % c)
def test_bn_act_fwd(dev, mode, case):
    rows, G, C, a, residual, training, cs, coff = case
    r = run_fwd(mode, dev, rows, G, C, a, residual=residual, training=training, cs=cs, coff=coff)
    check_fwd(r, 'fwd')
    if not training:                                        # eval: reads the running statistics, changes nothing
        assert torch.equal(r.rm.cpu(), (0.1 * fill.unit((C,), 14))) and int(r.nbt) == 7
        assert torch.equal(r.rv.cpu(), (1 + 0.3 * fill.unit((C,), 15)))


# ------------------------------------------------------------------ sba_bn_act_bwd_reduce + sba_bn_act_bwd_apply
#               rows  C     acts   modes
TWO_PASS_CASES = [(331, 32, ACTS3, BN_MODES), (3072, 64, ACTS3, BN_MODES), (4100, 1024, [NONE], ['f32']), (5, 64, ACTS3, BN_MODES),
                  # 6 * C * 4 bytes of dynamic LDS in the apply pass = 96 KB: a gfx950 workgroup may take all 160 KB of
                  # a CU's LDS, and HIP on AMD needs no opt-in above 48 KB, so the entry points accept it and it runs
                  (331, 4096, [NONE, GLU], BN_MODES)]
TWO_PASS = [(rows, C, a, m) for rows, C, acts, modes in TWO_PASS_CASES for a in acts for m in modes]


@pytest.mark.parametrize('case', TWO_PASS, ids=lambda c: 'r%d-c%d-a%d-%s' % c)
def test_bn_bwd_two_pass(dev, case):
    rows, C, a, mode = case
    fw = run_fwd(mode, dev, rows, 1, C, a)
    red = check_bwd(run_bwd(fw, dev, 'two_pass'), 'two-pass')
    if rows == 3072 and not (a == GLU and mode != 'f32'):
        # more workgroups than replicas (GLU on the 16-bit types packs 64 rows per iteration and asks for 6 workgroups
        # only): every replica is used
        assert int((red[0].abs().sum((1, 2)) > 0).sum()) == slots()


@pytest.mark.parametrize('mode', BN_MODES)
@pytest.mark.parametrize('a', ACTS3)
def test_bn_bwd_two_pass_slice_groups_and_null(dev, mode, a):
    C = 32
    Co = C // 2 if a == GLU else C
    fw = run_fwd(mode, dev, 331, 2, C, a)
    # dout is the upper half of a 2 Co wide tensor; two groups add into a prefilled dgamma / dbeta
    check_bwd(run_bwd(fw, dev, 'two_pass', dcs=2 * Co, dco=Co), 'slice, 2 groups')
    # dgamma = dbeta = NULL: dy is still right and nothing else is written
    check_bwd(run_bwd(fw, dev, 'two_pass', null_param=True), 'null dgamma')


# ------------------------------------------------------------------ sba_bn_act_fwd_fused / sba_bn_act_bwd_fused
# rows {16, 255, 257, 2560} x C {2V, 64, 1024} x act x groups {1, 2}: a covering selection, not the cross product -- every
# value of every axis, every act at every row count and at every width, both group counts at every row count and width
#              rows  C (None: 2V)  act  groups
FUSED_CASES = [(16, None, NONE, 1), (16, None, GLU, 2), (16, None, LRELU, 1),
               (255, 64, NONE, 2), (255, 64, GLU, 1), (255, 64, LRELU, 2),
               (257, 64, NONE, 1), (257, 64, GLU, 2), (257, 64, LRELU, 1),
               (2560, 1024, NONE, 1), (2560, 1024, GLU, 2), (2560, 1024, LRELU, 1),
               (16, 1024, LRELU, 2), (257, 1024, NONE, 2), (2560, None, GLU, 1), (2560, 64, LRELU, 2), (255, None, NONE, 2)]


@pytest.mark.parametrize('mode', BN_MODES)
@pytest.mark.parametrize('case', FUSED_CASES, ids=lambda c: 'r%d-c%s-a%d-g%d' % c)
def test_bn_fused(dev, mode, case):
    rows, C, a, G = case
    C = C or 2 * MODES[mode][3]
    T = MODES[mode][2]
    fw = run_fwd(mode, dev, rows, G, C, a, fused=True)
    check_fwd(fw, 'fused fwd')
    b = run_bwd(fw, dev, 'fused')
    check_bwd(b, 'fused bwd')
    # the same buffers through the two-pass entry points
    f2 = run_fwd(mode, dev, rows, G, C, a, fused=False)
    b2 = run_bwd(fw, dev, 'two_pass')                       # (the fused forward's aux: the same LeakyReLU branches)
    n_out, n_dy = G * rows * fw.Co, G * rows * C
    pairs = [('out', fw.out[:n_out], f2.out[:n_out], fw.ref.out), ('dy', b.dy[:n_dy], b2.dy[:n_dy], b.ref.dy)]
    for name, x, x2, ref in pairs:
        if T == torch.float32:
            elem_close(x, x2.double().cpu(), 'fused vs two-pass ' + name)
        else:                                               # two independent roundings: twice the bf16 bound
            r, floor = rel_l2(x, x2), bf16_floor(ref)
            print('fused vs two-pass %-10s bf16 rel L2 %.3e, floor %.3e' % (name, r, floor))
            assert r <= 4 * floor, (name, r, floor)
    elem_close(fw.aux[:G * 4 * C], f2.aux[:G * 4 * C].double().cpu(), 'fused vs two-pass aux')
    sums_close(b.dg[:C].double().cpu() - b.dg0, b2.dg[:C].double().cpu() - b2.dg0, b.ref.dgamma_abs, 'fused vs two-pass dgamma')
    sums_close(b.db[:C].double().cpu() - b.db0, b2.db[:C].double().cpu() - b2.db0, b.ref.dbeta_abs, 'fused vs two-pass dbeta')


# ------------------------------------------------------------------ sba_bn1d_glu_fwd / _bwd
@pytest.mark.parametrize('mode', IN_MODES)
@pytest.mark.parametrize('B', [2, 20, 32, 33, 40])          # 33 and 40: the uncached branch
@pytest.mark.parametrize('Fd', [32, 16384])
def test_bn1d_glu(dev, mode, B, Fd):
    code, _, T, _ = MODES[mode]
    Cg = Fd // 32
    y, yd = draw((B, Fd), 41, torch.float32, dev)
    gamma, beta, gd, bd = params(Fd, 42, dev)
    rm0, rv0 = 0.1 * fill.unit((Fd,), 44), 1 + 0.3 * fill.unit((Fd,), 45)
    rm, rv, nbt = rm0.to(dev), rv0.to(dev), torch.tensor([3], dtype=torch.int64, device=dev)
    mean, rstd = nans(Fd + PAD, torch.float32, dev), nans(Fd + PAD, torch.float32, dev)
    out = nans(B * 16 * Cg + PAD, T, dev)
    lib().call('sba_bn1d_glu_fwd', code, p(y), p(gamma), p(beta), p(rm), p(rv), p(nbt), p(mean), p(rstd), p(out), B, Fd,
               R.EPS, R.MOMENTUM, stream())
    dout, doutd = draw((B, 16, Cg), 46, T, dev)
    dy = nans(B * Fd + PAD, torch.float32, dev)
    dg, dg0 = prefilled(Fd, 47, dev)
    db, db0 = prefilled(Fd, 48, dev)
    lib().call('sba_bn1d_glu_bwd', code, p(y), p(dout), p(gamma), p(beta), p(mean), p(rstd), p(dy), p(dg), p(db), B, Fd,
               stream())
    torch.cuda.synchronize()
    f = R.bn1d_glu_fwd(yd, gd, bd, rm0, rv0, 3)
    out_close(front(out, B * 16 * Cg, 'out'), f.out, T, 'bn1d out (NHWC)')
    elem_close(front(mean, Fd, 'mean'), f.mean, 'bn1d mean'); elem_close(front(rstd, Fd, 'rstd'), f.rstd, 'bn1d rstd')
    elem_close(rm, f.running_mean, 'bn1d running_mean'); elem_close(rv, f.running_var, 'bn1d running_var')
    assert int(nbt) == f.nbt
    # mean and rstd are INPUTS of the backward entry point (f32, checked against float64 just above): the reference is
    # evaluated on them, as on every other rounded input.
    gmean, grstd = front(mean, Fd, 'mean'), front(rstd, Fd, 'rstd')
    b = R.bn1d_glu_bwd(yd, doutd, gd, bd, gmean, grstd)
    elem_close(front(dy, B * Fd, 'dy'), b.dy, 'bn1d dy')
    ideal = R.bn1d_glu_bwd(yd, doutd, gd, bd, f.mean, f.rstd)
    # ... and against the float64 statistics, independent of the forward kernel: the plain f32 bound for B > 2.  At
    # B = 2 no f32 mean can hold it: xhat = +-x, dy_b = scale * (dz_1 - dz_2) / 2 * (1 - x^2) is what is left of a
    # cancellation, and a batch mean that is off by delta (f32: delta <= 2^-24 |mean|, half an ulp of the sum a + b)
    # shifts both xhat by epsilon = delta * rstd the same way, which leaves, to first order,
    #     dy_b error = +-scale * epsilon * x * dz_b,   |.| <= |gamma| * rstd^2 * 2^-24 |mean| * |dz_b|.
    # Allowed on top of the f32 bound: twice that term (second-order terms, the same effect inside the gate's dz).
    # Measured at F = 16384: 3.6 x the plain f32 bound (max error 2.9e-3 on |dy| about 4), 0.36 of this one.
    got_dy = front(dy, B * Fd, 'dy')
    if B > 2:
        elem_close(got_dy, ideal.dy, 'bn1d dy (float64 statistics)')
    else:
        err = (got_dy - ideal.dy.flatten()).abs()
        plain = 2e-5 + 2e-4 * ideal.dy.flatten().abs()
        cond = (2 * gd.abs() * f.rstd ** 2 * 2.0 ** -24 * f.mean.abs())[None, :] * ideal.dz.abs()
        print('B = 2, dy against float64 statistics: max err %.3e, worst error / f32 bound %.2f, worst error / '
              '(f32 bound + conditioning term) %.2f' % (float(err.max()), float((err / plain).max()),
                                                        float((err / (plain + cond.flatten())).max())))
        assert bool((err <= plain + cond.flatten()).all()), 'bn1d dy (float64 statistics, B = 2)'
    sums_close(front(dg, Fd, 'dgamma') - dg0, b.dgamma, b.dgamma_abs, 'bn1d dgamma')
    sums_close(front(db, Fd, 'dbeta') - db0, b.dbeta, b.dbeta_abs, 'bn1d dbeta')


# ------------------------------------------------------------------ sba_instnorm_stats
def in_eps():
    from sbagan import ops
    return ops.IN_EPS


def run_instnorm(mode, dev, N, cv, HW, offset=0.0, tag=51):
    code, _, T, V = MODES[mode]
    C = cv * V                                              # bf16: twice the f32 width, N * cv on the same side of 64
    h, hd = draw((N, HW, C), tag, T, dev, offset)
    mean, rstd = nans(N * C + PAD, torch.float32, dev), nans(N * C + PAD, torch.float32, dev)
    lib().call('sba_instnorm_stats', code, p(h), p(mean), p(rstd), N, HW, C, in_eps(), stream())
    torch.cuda.synchronize()
    return NS(h=h, hd=hd, mean=mean, rstd=rstd, N=N, C=C, HW=HW, ref=R.instnorm_stats(hd, in_eps()))


def check_instnorm(r, name='instnorm'):
    elem_close(front(r.mean, r.N * r.C, name + ' mean'), r.ref.mean, name + ' mean')
    elem_close(front(r.rstd, r.N * r.C, name + ' rstd'), r.ref.rstd, name + ' rstd')


#               N  cv   HW      (f32: C = 4 cv; bf16: C = 8 cv)
IN_CASES = [(8, 8, 1024), (8, 8, 1296), (8, 8, 2047),       # one launch: no tail, ragged tail, three-step ragged tail
            (8, 8, 1023), (7, 8, 1024),                     # accumulate + finalize: HW below the switch, N * cv = 56
            (2, 256, 50), (3, 1, 17)]                       # cv = 256 (rpi = 1), cv = 1


@pytest.mark.parametrize('mode', IN_MODES)
@pytest.mark.parametrize('case', IN_CASES, ids=lambda c: 'n%d-cv%d-hw%d' % c)
def test_instnorm_stats(dev, mode, case):
    check_instnorm(run_instnorm(mode, dev, *case))


# ------------------------------------------------------------------ sba_adain_fwd / _bwd_reduce / _bwd_apply
def run_adain(mode, dev, N, cv, HW, accumulate, want_dstyle, tag=61):
    code, _, T, V = MODES[mode]
    C = cv * V
    r = NS(N=N, C=C, HW=HW, T=T, accumulate=accumulate, want_dstyle=want_dstyle)
    h, hd = draw((N, HW, C), tag, T, dev, 0.3)
    style, styled = draw((N, 2 * C), tag + 1, torch.float32, dev, scale=0.5)
    st = R.instnorm_stats(hd, in_eps())
    mean, rstd = st.mean.float().to(dev), st.rstd.float().to(dev)       # (the statistics kernel has its own tests)
    md, rd = mean.double().cpu(), rstd.double().cpu()
    r.outs = []
    for oco in (0, C):                                      # either half of a 2C wide buffer; the other keeps its NaN
        out = nans((N * HW + 3) * 2 * C, T, dev)
        lib().call('sba_adain_fwd', code, p(h), p(mean), p(rstd), p(style), p(out), N, HW, C, 2 * C, oco, stream())
        r.outs.append((oco, out))
    dout, doutd = draw((N * HW, 2 * C), tag + 2, T, dev)    # read at dcs = 2C, dco = C
    r.red = zeros_guarded(N * C * 2, dev)                   # zeroed by the caller, as ops does
    lib().call('sba_adain_bwd_reduce', code, p(h), p(dout), p(mean), p(rstd), p(r.red), N, HW, C, 2 * C, C, stream())
    dh0, dh0d = draw((N * HW * C,), tag + 3, T, dev)
    r.dh = nans(N * HW * C + PAD, T, dev)
    if accumulate:
        r.dh[:N * HW * C] = dh0
    r.dstyle = nans(N * 2 * C + PAD, torch.float32, dev)
    lib().call('sba_adain_bwd_apply', code, p(h), p(dout), p(mean), p(rstd), p(style), p(r.red), p(r.dh),
               p(r.dstyle) if want_dstyle else None, N, HW, C, 2 * C, C, accumulate, stream())
    torch.cuda.synchronize()
    r.ref_out = R.adain_fwd(hd, md, rd, styled)
    r.ref = R.adain_bwd(hd, doutd[:, C:].reshape(N, HW, C), md, rd, styled)
    r.ref_dh = r.ref.dh.flatten() + (dh0d if accumulate else 0)
    return r


def check_adain(r, name='adain'):
    N, C, HW = r.N, r.C, r.HW
    for oco, out in r.outs:
        got = window(out, N * HW, 2 * C, oco, C, '%s out@%d' % (name, oco))
        out_close(got, r.ref_out.reshape(N * HW, C), r.T, '%s out@%d' % (name, oco))
    sums_close(front(r.red, N * C * 2, name + ' red'), r.ref.red, r.ref.red_abs, name + ' red')
    out_close(front(r.dh, N * HW * C, name + ' dh'), r.ref_dh, r.T, name + ' dh (accumulate %d)' % r.accumulate)
    if r.want_dstyle:
        sums_close(front(r.dstyle, N * 2 * C, name + ' dstyle'), r.ref.dstyle, r.ref.dstyle_abs, name + ' dstyle')
    else:
        assert bool(torch.isnan(r.dstyle).all()), 'dstyle = NULL, yet something was written'


ADAIN_CASES = [(8, 8, 1296), (2, 256, 50), (3, 1, 17)]


@pytest.mark.parametrize('mode', IN_MODES)
@pytest.mark.parametrize('variant', [(0, True), (1, False), (1, True), (0, False)], ids=lambda v: 'acc%d-dstyle%d' % v)
@pytest.mark.parametrize('case', ADAIN_CASES, ids=lambda c: 'n%d-cv%d-hw%d' % c)
def test_adain(dev, mode, case, variant):
    check_adain(run_adain(mode, dev, *case, accumulate=variant[0], want_dstyle=variant[1]))


# ------------------------------------------------------------------ offset inputs: E[x^2] - mean^2 in f32
@pytest.mark.parametrize('mode', BN_MODES)
def test_offset_inputs_batchnorm(dev, mode):
    """x = 4 + unit, |mean| / std about 4 (a float32 evaluation of the single-pass variance at this ratio stays inside
    the f32 bound: test_norm_ref_cpu).  Pins the formula at a realistic offset; not a stress test.  The rstd error at
    ratio 30 is printed, not asserted: it shows where the formula stops."""
    check_fwd(run_fwd(mode, dev, 331, 1, 64, LRELU, offset=OFFSET), 'offset 4, two-pass fwd')
    check_fwd(run_fwd(mode, dev, 257, 2, 64, GLU, offset=OFFSET, fused=True), 'offset 4, fused fwd')
    for fused in (False, True):
        r = run_fwd(mode, dev, 331, 1, 64, NONE, offset=30.0, fused=fused)
        got, ref = r.aux[:4 * 64].double().cpu().view(4, 64)[3], r.ref.aux[0, 3]
        print('[recorded, not asserted] ratio 30, %s, fused=%d: worst relative rstd error %.2e'
              % (mode, fused, float(((got - ref).abs() / ref).max())))


@pytest.mark.parametrize('mode', IN_MODES)
def test_offset_inputs_instnorm(dev, mode):
    check_instnorm(run_instnorm(mode, dev, 8, 8, 1296, offset=OFFSET), 'offset 4, one launch')
    check_instnorm(run_instnorm(mode, dev, 8, 8, 1023, offset=OFFSET), 'offset 4, accumulate')
    for HW in (1296, 1023):
        r = run_instnorm(mode, dev, 8, 8, HW, offset=30.0)
        got = r.rstd[:r.N * r.C].double().cpu().view(r.N, r.C)
        print('[recorded, not asserted] ratio 30, %s, HW=%d: worst relative rstd error %.2e'
              % (mode, HW, float(((got - r.ref.rstd).abs() / r.ref.rstd).max())))


# ------------------------------------------------------------------ deterministic mode
@contextlib.contextmanager
def deterministic(dev):
    from sbagan import ops
    ops.set_deterministic(True, dev)
    try:
        yield ops
    finally:
        ops.set_deterministic(False)


def twice(ops, fn):
    ops.det_reset()
    a = fn()
    ops.det_reset()
    return a, fn()


def same_bits(x, y, name):
    assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), '%s: two deterministic runs differ' % name


@pytest.mark.parametrize('mode', BN_MODES)
def test_deterministic_bn(dev, mode):
    """the ordered branches (det_part + sba_det_fold, the per-group relaunch of the apply pass and of the fused
    backward) against the same reference at the same bounds, and bit-equal run to run"""
    with deterministic(dev) as ops:
        for C in (80, 4096):                                # statistics
            y, yd = draw((1, 331, C), 3, MODES[mode][1], dev)
            s1, s2 = twice(ops, lambda: run_stats(mode, dev, y, 331, 1, C))
            torch.cuda.synchronize()
            check_stats(s1, yd, 1, C, 'det stats C=%d' % C)
            same_bits(s1, s2, 'stats')
        for a, G in [(NONE, 1), (GLU, 1), (LRELU, 1), (GLU, 2)]:     # 3072-row two-pass backward
            def go():
                return run_bwd(run_fwd(mode, dev, 3072, G, 64, a), dev, 'two_pass')
            b1, b2 = twice(ops, go)
            check_fwd(b1.fw, 'det fwd')
            check_bwd(b1, 'det two-pass act %d groups %d' % (a, G))
            for k in ('dy', 'dg', 'db', 'red'):
                same_bits(getattr(b1, k), getattr(b2, k), k)
        b1, b2 = twice(ops, lambda: run_bwd(run_fwd(mode, dev, 257, 2, 64, GLU, fused=True), dev, 'fused'))
        check_bwd(b1, 'det fused groups 2')
        for k in ('dy', 'dg', 'db'):
            same_bits(getattr(b1, k), getattr(b2, k), k)


@pytest.mark.parametrize('mode', IN_MODES)
def test_deterministic_instnorm_adain(dev, mode):
    with deterministic(dev) as ops:
        for case in [(8, 8, 1023), (7, 8, 1024), (2, 256, 50), (3, 1, 17)]:      # the accumulate path
            r1, r2 = twice(ops, lambda: run_instnorm(mode, dev, *case))
            check_instnorm(r1, 'det instnorm %s' % (case,))
            same_bits(r1.mean, r2.mean, 'mean'); same_bits(r1.rstd, r2.rstd, 'rstd')
        for case in ADAIN_CASES:
            r1, r2 = twice(ops, lambda: run_adain(mode, dev, *case, accumulate=1, want_dstyle=True))
            check_adain(r1, 'det adain %s' % (case,))
            for k in ('red', 'dh', 'dstyle'):
                same_bits(getattr(r1, k), getattr(r2, k), k)


# ------------------------------------------------------------------ refusals
E_ARG = -1
BIG = 1 << 19                                               # elements per buffer: room for every refused shape below but
#                                                             groups = 65536, which no launch accepts (grid.y limit)


def _refuse(name, order, base, changes, outputs):
    """every change of one (or more) arguments of an accepted call must come back as SBA_E_ARG and write nothing"""
    L = lib().lib
    for what, delta in changes:
        args = dict(base)
        args.update(delta)
        rc = getattr(L, name)(*[p(args[k]) if torch.is_tensor(args[k]) else args[k] for k in order])
        torch.cuda.synchronize()
        assert rc == E_ARG, '%s accepted "%s" (status %d)' % (name, what, rc)
        for k in outputs:
            assert bool(torch.isnan(base[k]).all()), '%s wrote to %s although it refused "%s"' % (name, k, what)
    rc = getattr(L, name)(*[p(base[k]) if torch.is_tensor(base[k]) else base[k] for k in order])
    torch.cuda.synchronize()
    assert rc == 0, '%s refuses the accepted call the refusals were derived from (status %d)' % (name, rc)


def _stride_changes(V, Co, cs='cs', co='co'):
    return [('stride below Co + offset', {cs: Co, co: V}), ('stride not a multiple of V', {cs: Co + V + 1}),
            ('offset not a multiple of V', {cs: 2 * Co, co: 1}), ('unaligned offset, bytes', {cs: 2 * Co, co: V // 2})]


@pytest.mark.parametrize('mode', IN_MODES)
def test_refusals(dev, mode):
    code, _, T, V = MODES[mode]
    f32 = torch.float32
    st = stream()

    def ins(dt=T):
        return torch.ones(BIG, dtype=dt, device=dev)

    def outs(dt=T):
        return nans(BIG, dt, dev)
    shape = [('rows = 0', dict(rows=0)), ('groups = 0', dict(G=0)), ('groups > 65535', dict(G=65536)), ('C = 0', dict(C=0)),
             ('C % V != 0', dict(C=64 + V // 2)), ('C > 4096', dict(C=8192)), ('unknown dtype', dict(dt=7))]
    pow2 = [('C not a power of two', dict(C=80 if V == 4 else 96)), ('GLU: C / 2 no multiple of V', dict(C=V, act=GLU))]

    # sba_bn_stats
    b = dict(dt=code, y=ins(), stats=outs(f32), rows=8, G=1, C=64, st=st)
    _refuse('sba_bn_stats', ['dt', 'y', 'stats', 'rows', 'G', 'C', 'st'], b,
            shape + [('y = NULL', dict(y=None)), ('stats = NULL', dict(stats=None))], ['stats'])

    # sba_bn_act_fwd
    order = ['dt', 'y', 'stats', 'gamma', 'beta', 'rm', 'rv', 'nbt', 'aux', 'res', 'out', 'rows', 'G', 'C', 'act', 'cs', 'co',
             'eps', 'mom', 'train', 'st']
    b = dict(dt=code, y=ins(), stats=torch.zeros(BIG, device=dev), gamma=ins(f32), beta=ins(f32), rm=outs(f32), rv=outs(f32),
             nbt=None, aux=outs(f32), res=None, out=outs(), rows=8, G=1, C=64, act=NONE, cs=64, co=0, eps=R.EPS,
             mom=R.MOMENTUM, train=1, st=st)
    nulls = [('%s = NULL' % k, {k: None}) for k in ('y', 'gamma', 'beta', 'aux', 'out')]
    _refuse('sba_bn_act_fwd', order, b, shape + nulls + _stride_changes(V, 64) + [
        ('training without statistics', dict(stats=None)), ('running_mean without running_var', dict(rv=None)),
        ('running_var without running_mean', dict(rm=None)), ('eval without running statistics', dict(train=0, rm=None, rv=None)),
        ('GLU with a residual', dict(act=GLU, res=b['y'], cs=32)), ('GLU: C / 2 no multiple of V', dict(C=V, act=GLU, cs=V)),
        ('unknown activation', dict(act=9))], ['rm', 'rv', 'aux', 'out'])

    # sba_bn_act_fwd_fused
    order = ['dt', 'y', 'gamma', 'beta', 'rm', 'rv', 'nbt', 'aux', 'out', 'rows', 'G', 'C', 'act', 'cs', 'co', 'eps', 'mom', 'st']
    b = dict(dt=code, y=ins(), gamma=ins(f32), beta=ins(f32), rm=outs(f32), rv=outs(f32), nbt=None, aux=outs(f32), out=outs(),
             rows=8, G=1, C=64, act=NONE, cs=64, co=0, eps=R.EPS, mom=R.MOMENTUM, st=st)
    _refuse('sba_bn_act_fwd_fused', order, b, shape + pow2 + nulls + _stride_changes(V, 64) + [
        ('running_mean without running_var', dict(rv=None)), ('running_var without running_mean', dict(rm=None)),
        ('ReLU (forward-only activation of sba_bn_act_fwd)', dict(act=RELU))], ['rm', 'rv', 'aux', 'out'])

    # the three backward entry points
    bw = dict(dt=code, y=ins(), dout=ins(), aux=ins(f32), red=outs(f32), dy=outs(), dg=outs(f32), db=outs(f32), rows=8, G=1,
              C=64, act=NONE, cs=64, co=0, st=st)
    param = [('dgamma without dbeta', dict(db=None)), ('dbeta without dgamma', dict(dg=None))]
    common = shape + pow2 + _stride_changes(V, 64) + [('ReLU', dict(act=RELU)), ('unknown activation', dict(act=9))]
    _refuse('sba_bn_act_bwd_reduce', ['dt', 'y', 'dout', 'aux', 'red', 'rows', 'G', 'C', 'act', 'cs', 'co', 'st'], bw,
            common + [('%s = NULL' % k, {k: None}) for k in ('y', 'dout', 'aux', 'red')], ['red'])
    bw['red'] = torch.zeros(BIG, device=dev)                # (an input of the apply pass)
    _refuse('sba_bn_act_bwd_apply', ['dt', 'y', 'dout', 'aux', 'red', 'dy', 'dg', 'db', 'rows', 'G', 'C', 'act', 'cs', 'co', 'st'],
            bw, common + param + [('%s = NULL' % k, {k: None}) for k in ('y', 'dout', 'aux', 'red', 'dy')], ['dy', 'dg', 'db'])
    bw.update(dy=outs(), dg=outs(f32), db=outs(f32))
    _refuse('sba_bn_act_bwd_fused', ['dt', 'y', 'dout', 'aux', 'dy', 'dg', 'db', 'rows', 'G', 'C', 'act', 'cs', 'co', 'st'],
            bw, common + param + [('%s = NULL' % k, {k: None}) for k in ('y', 'dout', 'aux', 'dy')], ['dy', 'dg', 'db'])

    # sba_bn1d_glu_fwd / _bwd
    order = ['dt', 'y', 'gamma', 'beta', 'rm', 'rv', 'nbt', 'mean', 'rstd', 'out', 'B', 'F', 'eps', 'mom', 'st']
    b = dict(dt=code, y=ins(f32), gamma=ins(f32), beta=ins(f32), rm=None, rv=None, nbt=None, mean=outs(f32), rstd=outs(f32),
             out=outs(), B=4, F=64, eps=R.EPS, mom=R.MOMENTUM, st=st)
    dims = [('B = 0', dict(B=0)), ('F = 0', dict(F=0)), ('F % 32 != 0', dict(F=48)), ('unknown dtype', dict(dt=7)),
            ('binary16 y has no meaning here', dict(dt=2))]
    half = outs(f32)
    _refuse('sba_bn1d_glu_fwd', order, b, dims + [('%s = NULL' % k, {k: None}) for k in ('y', 'gamma', 'beta', 'mean', 'rstd', 'out')]
            + [('running_mean without running_var', dict(rm=half)), ('running_var without running_mean', dict(rv=half))],
            ['mean', 'rstd', 'out'])
    assert bool(torch.isnan(half).all()), 'sba_bn1d_glu_fwd wrote running statistics although it refused the call'
    order = ['dt', 'y', 'dout', 'gamma', 'beta', 'mean', 'rstd', 'dy', 'dg', 'db', 'B', 'F', 'st']
    b = dict(dt=code, y=ins(f32), dout=ins(), gamma=ins(f32), beta=ins(f32), mean=ins(f32), rstd=ins(f32), dy=outs(f32),
             dg=outs(f32), db=outs(f32), B=4, F=64, st=st)
    _refuse('sba_bn1d_glu_bwd', order, b, dims + [('%s = NULL' % k, {k: None}) for k in order[1:10]], ['dy', 'dg', 'db'])

    # InstanceNorm / AdaIN
    C = 8 * V
    inshape = [('N = 0', dict(N=0)), ('HW = 0', dict(HW=0)), ('C = 0', dict(C=0)), ('C % V != 0', dict(C=C + V // 2)),
               ('C / V not a power of two', dict(C=3 * V)), ('C / V > 256', dict(C=512 * V)), ('unknown dtype', dict(dt=7)),
               ('binary16 y has no meaning here', dict(dt=2))]
    b = dict(dt=code, h=ins(), mean=outs(f32), rstd=outs(f32), N=2, HW=16, C=C, eps=R.EPS, st=st)
    _refuse('sba_instnorm_stats', ['dt', 'h', 'mean', 'rstd', 'N', 'HW', 'C', 'eps', 'st'], b,
            inshape + [('%s = NULL' % k, {k: None}) for k in ('h', 'mean', 'rstd')], ['mean', 'rstd'])
    b = dict(dt=code, h=ins(), mean=ins(f32), rstd=ins(f32), style=ins(f32), out=outs(), N=2, HW=16, C=C, cs=C, co=0, st=st)
    _refuse('sba_adain_fwd', ['dt', 'h', 'mean', 'rstd', 'style', 'out', 'N', 'HW', 'C', 'cs', 'co', 'st'], b,
            inshape + _stride_changes(V, C) + [('%s = NULL' % k, {k: None}) for k in ('h', 'mean', 'rstd', 'style', 'out')], ['out'])
    b = dict(dt=code, h=ins(), dout=ins(), mean=ins(f32), rstd=ins(f32), red=outs(f32), N=2, HW=16, C=C, cs=C, co=0, st=st)
    _refuse('sba_adain_bwd_reduce', ['dt', 'h', 'dout', 'mean', 'rstd', 'red', 'N', 'HW', 'C', 'cs', 'co', 'st'], b,
            inshape + _stride_changes(V, C) + [('%s = NULL' % k, {k: None}) for k in ('h', 'dout', 'mean', 'rstd', 'red')], ['red'])
    b = dict(dt=code, h=ins(), dout=ins(), mean=ins(f32), rstd=ins(f32), style=ins(f32), red=torch.zeros(BIG, device=dev),
             dh=outs(), dstyle=outs(f32), N=2, HW=16, C=C, cs=C, co=0, acc=0, st=st)
    _refuse('sba_adain_bwd_apply', ['dt', 'h', 'dout', 'mean', 'rstd', 'style', 'red', 'dh', 'dstyle', 'N', 'HW', 'C', 'cs', 'co',
                                    'acc', 'st'], b,
            inshape + _stride_changes(V, C) + [('%s = NULL' % k, {k: None}) for k in ('h', 'dout', 'mean', 'rstd', 'style', 'red', 'dh')],
            ['dh', 'dstyle'])


# ------------------------------------------------------------------ the dispatch threshold through ops
@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('which', ['up', 'leak', 'down', 'res'])
def test_blocks_above_the_fused_threshold(dev, dt, which):
    """The four blocks of test_kernels_gpu.test_conv_bn_act_blocks with a 32x32 BatchNorm map: 3 * 32 * 32 = 3072 rows, just
    above ops.BN_FUSED_BWD_ROWS, so ops.bn_act_backward takes the two-pass kernels; same reference, same bounds."""
    from oracle import sbagan_oracle as O
    from sbagan import nets, ops
    ops.set_compute_dtype(dt)
    N, C = 3, 64
    H = {'up': 16, 'leak': 32, 'down': 64, 'res': 32}[which]
    rows = N * 32 * 32
    assert rows > ops.BN_FUSED_BWD_ROWS, 'a retuned threshold moved this case back onto the fused path: raise the map size'
    if which == 'up':
        mod, fn = nets.upBlock(C, C // 2), lambda x, Q: O.up_block(x, Q, 'm')
    elif which == 'leak':
        mod, fn = nets.Block3x3_leakRelu(C, 128), lambda x, Q: O._block3x3_leak(x, Q, 'm', True)
    elif which == 'down':
        mod, fn = nets.downBlock(C, 128), lambda x, Q: O._down(x, Q, 'm', 0, 1, True)
    else:
        mod, fn = nets.ResBlock(C), lambda x, Q: O.res_block(x, Q, 'm')
    P = fill.fill_state_dict({k: tuple(v.shape) for k, v in mod.state_dict().items()})
    _load(mod, P, dev)
    x = fill.unit((N, C, H, H), 5)
    xr = rounded(x, dt).requires_grad_(True)
    Q = _oracle_P(P, 'm.')
    yref = fn(xr, Q)
    assert yref.shape[0] * yref.shape[2] * yref.shape[3] == rows
    dy = fill.unit(tuple(yref.shape), 6)
    yref.backward(rounded(dy, dt))
    xa = act(x, dt, dev).requires_grad_(True)
    y = mod(xa)
    y.backward(act(dy, dt, dev))
    torch.cuda.synchronize()
    assert y.dtype == dt and y.is_contiguous(memory_format=torch.channels_last)
    close(y, yref, dt, 'out', scale=3)
    close(xa.grad, xr.grad, dt, 'dx', scale=3)
    _check_module(mod, Q, dt, 'm.', gscale=3)
