"""The kernel choice of sba_conv_wgrad is pure host code: sba_conv_wgrad_plan answers without a device.
tests/golden/wgrad_plan.npz holds its answers on the grid below, recorded (tools/make_golden.py wgrad_plan) from the
commit BEFORE the dispatch of wgrad.hip became a plan + a launcher -- that commit had no query, so its own
sba_conv_wgrad was compiled a second time with its launches redirected to a recorder (profiles/wgrad_plan_refactor.txt).
The current library must give the same (rc, family, variant, grid, block, LDS bytes, chunks per split, epilogue mode,
deterministic partials, wclog) row by row.  The claims beside CONV_CASES of tests/test_kernels_gpu.py (which
weight-gradient kernel a case is there for) are checked here too, so that they cannot go stale."""
import ctypes
import itertools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'wgrad_plan.npz')

KINDS = ('3x3', '3x3up', '4x4s2', '1x1', '4x4s2_dgrad')
BATCHES = (1, 2, 3, 20, 40)
MAPS = ((2, 2), (4, 4), (5, 3), (8, 8), (16, 24), (64, 64), (128, 128), (256, 128))      # input H x W
CHANNELS = (32, 64, 96, 128, 224, 512, 544, 1024, 1056)
KSPLITS = (0, 1, 3)
# beyond the grid: what only a batch above 40 reaches -- pixel splits of the 4 x 4-map kernel-row variant (M >= 768)
EXTRA = (('3x3', 48, 4, 4, 64, 64), ('3x3', 64, 4, 4, 128, 512))


def geom(_lib, kind, N, H, W, Cin, Cout):
    """the geometry ops.conv_wgrad builds for `kind` (sbagan.ops._geom), plus a 1 x 1 conv and one parity class of the
    4x4 / stride-2 data gradient (osy = osx = 2)"""
    g = _lib.ConvGeom()
    g.N, g.IH, g.IW, g.Cin, g.Cout = N, H, W, Cin, Cout
    g.sy = g.sx = g.osy = g.osx = 1
    k, s, off, up = {'3x3': (3, 1, 1, 1), '3x3up': (3, 1, 1, 2), '4x4s2': (4, 2, 1, 1), '1x1': (1, 1, 0, 1),
                     '4x4s2_dgrad': (2, 1, 0, 2)}[kind]
    g.OH, g.OW = (H * up, W * up) if s == 1 else (H // 2, W // 2)
    g.OHs, g.OWs = g.OH, g.OW
    g.sy = g.sx = s
    g.ups = 1 if kind == '3x3up' else 0
    g.ntaps = k * k
    for t in range(k * k):
        g.ty[t], g.tx[t] = t // k - off, t % k - off
    if kind == '4x4s2_dgrad':           # parity class (py, px) = (1, 0)
        g.OHs, g.OWs, g.osy, g.osx, g.ooy, g.oox = H, W, 2, 2, 1, 0
        for t in range(4):
            g.ty[t], g.tx[t] = 1 - t // 2, 0 - t % 2
    return g


def replay(_lib):
    """the answers of the library behind `_lib`: name -> int32 array of (rc, plan[0..13]); 'grid' = dtype x KINDS x
    BATCHES x MAPS x Cin x Cout x first_write x det x ksplit in that order, 'extra' = dtype x EXTRA x the same inner three"""
    n = _lib.WGRAD_PLAN_INTS
    plan = (ctypes.c_int * n)()
    query = _lib.lib.sba_conv_wgrad_plan
    inner = list(itertools.product((0, 1), (0, 1), KSPLITS))

    def rows_of(dtype, shapes):
        rows = []
        for kind, N, H, W, Cin, Cout in shapes:
            g = geom(_lib, kind, N, H, W, Cin, Cout)
            ref = ctypes.byref(g)
            for fw, det, ks in inner:
                g.first_write = fw
                plan[:] = [-1] * n
                rc = query(dtype, ref, ks, det, plan)
                rows.append((rc,) + tuple(plan))
        return rows

    grid = [(k, N, H, W, ci, co) for k, N, (H, W), ci, co in itertools.product(KINDS, BATCHES, MAPS, CHANNELS, CHANNELS)]
    out = {}
    for name, shapes in (('grid', grid), ('extra', EXTRA)):
        out[name] = np.array(rows_of(_lib.SBA_F32, shapes) + rows_of(_lib.SBA_BF16, shapes), dtype=np.int32)
    return out


# every (family, variant, epilogue mode) the dispatch can produce: mode 0 = +=, 1 = f32 atomics, 2 = store
ROW_DMA, SMALL_DMA, SMALL, ROWS, GENERIC = range(5)
F32, BF16 = 0, 1
TRIPLES = ([(ROW_DMA, v, m) for v in ((4, 2, 10, 4), (3, 1, 6, 4), (3, 1, 5, 4)) for m in (0, 1, 2)]
           + [(SMALL_DMA, (1, 4, 0, 0), m) for m in (0, 1, 2)] + [(SMALL_DMA, (2, 3, 0, 0), 2)]
           # (bf16 takes the register-staged small kernel only beyond 512 workgroups, where nothing is split: no atomics)
           + [(SMALL, (F32, 0, 0, 0), m) for m in (0, 1, 2)] + [(SMALL, (BF16, 0, 0, 0), m) for m in (0, 2)]
           + [(ROWS, (dt, 0, 0, 0), m) for dt in (F32, BF16) for m in (1, 2)]
           + [(GENERIC, (dt, 0, 0, 0), m) for dt in (F32, BF16) for m in (0, 1, 2)])


def test_wgrad_plans_equal_the_recorded_ones():
    from sbagan import _lib
    want = np.load(GOLDEN)
    got = replay(_lib)
    assert set(want.files) == set(got)
    # the recording itself covers what it claims to
    rec = np.concatenate([want['grid'], want['extra']])
    assert len(want['grid']) == 2 * 12 * len(KINDS) * len(BATCHES) * len(MAPS) * len(CHANNELS) ** 2 == 388800
    assert set(np.unique(rec[:, 0]).tolist()) == {0, -1}
    ok = rec[rec[:, 0] == 0]
    seen = set((r[0], tuple(r[1:5]), r[5]) for r in np.unique(ok[:, [1, 2, 3, 4, 5, 12]], axis=0).tolist())
    assert seen == set(TRIPLES), (sorted(seen - set(TRIPLES)), sorted(set(TRIPLES) - seen))
    assert (ok[ok[:, 13] > 0][:, 12] == 2).all()        # deterministic partials are stored, never added
    for name in want.files:
        w, g = want[name], got[name]
        assert w.shape == g.shape, name
        bad = np.nonzero((w != g).any(axis=1))[0]
        assert bad.size == 0, '%s: %d of %d rows differ, first at %d: recorded %s, now %s' % (
            name, bad.size, len(w), bad[0], w[bad[0]].tolist(), g[bad[0]].tolist())


def test_conv_cases_take_the_kernels_they_name():
    """WGRAD_KERNELS of tests/test_kernels_gpu.py: the kernel (and pixel splits) each case is there for, asked of the
    plan query with the geometry and the ksplit ops.conv_wgrad passes"""
    from sbagan import _lib, ops
    import test_kernels_gpu as K
    assert set(K.WGRAD_KERNELS) <= set(K.CONV_CASES)
    for case, claims in K.WGRAD_KERNELS.items():
        kind, N, Cin, Cout, H, W = case
        g = geom(_lib, kind, N, H, W, Cin, Cout)
        tiles = ((Cout + 63) // 64) * ((Cin + 63) // 64) * g.ntaps
        for (dt, fw), name in claims.items():
            g.first_write = fw
            p = _lib.wgrad_plan({'f32': _lib.SBA_F32, 'bf16': _lib.SBA_BF16}[dt], g, ops._ksplit(tiles, N * g.OH * g.OW))
            assert _lib.wgrad_plan_name(p) == name, (case, dt, fw, _lib.wgrad_plan_name(p), name)
    # between them the cases reach every kernel of wgrad.hip
    reached = set(n.split(' ')[0] for c in K.WGRAD_KERNELS.values() for n in c.values())
    assert reached == {'row_dma<4,2,10,4>', 'row_dma<3,1,6,4>', 'row_dma<3,1,5,4>', 'small_dma<1,4>', 'small_dma<2,3>',
                       'small<f32>', 'small<bf16>', 'rows<f32>', 'rows<bf16>', 'generic<f32>'}, reached
