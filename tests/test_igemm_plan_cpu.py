"""The kernel choice of sba_conv_igemm / sba_conv_igemm_glu is pure host code: sba_conv_igemm_plan and
sba_conv_igemm_glu_plan answer without a device.  tests/golden/igemm_plan.npz holds their answers on the grids below,
recorded (tools/make_golden.py igemm_plan) with a library built from the commit BEFORE the tile table of igemm.hip
became one constexpr table; the current library must give the same (rc, family, id, splits) row by row.  bench.py
(DOMINANT), ops._halo_family, inception_hip._frag_for and infer.py read these numbers."""
import ctypes
import itertools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'igemm_plan.npz')

TAPS = {1: [(0, 0)], 9: [(y, x) for y in (-1, 0, 1) for x in (-1, 0, 1)],
        16: [(y, x) for y in (-1, 0, 1, 2) for x in (-1, 0, 1, 2)]}
WS = (0, 64 << 20)


def _geom(_lib, N, S, Cin, Cout, ntaps, stride, ups=0):
    g = _lib.ConvGeom()
    O = S * 2 if ups else (S if stride == 1 else S // 2)
    g.N, g.IH, g.IW, g.Cin, g.OH, g.OW, g.Cout, g.OHs, g.OWs = N, S, S, Cin, O, O, Cout, O, O
    g.sy = g.sx = stride
    g.osy = g.osx = 1
    g.ups, g.ntaps = ups, ntaps
    for t, (y, x) in enumerate(TAPS[ntaps]):
        g.ty[t], g.tx[t] = y, x
    return g


def conv_grid(full):
    """(N, S, Cin, Cout, ntaps, stride, tile, ksplit, workspace bytes, w_layout) of the sba_conv_igemm_plan queries"""
    if full:        # bf16
        dims = ((1, 7, 20, 40), (4, 5, 8, 17, 32, 64), (32, 64, 96, 128, 160, 512), (32, 64, 72, 128, 192, 1024),
                (1, 9, 16), (1, 2), range(20), (0, 1, 3), WS, (0,))
    else:           # f32: Cin % 16, tiles and forced splits are ignored by its dispatch
        dims = ((1, 20), (4, 8, 32, 64), (16, 48, 64, 512), (32, 64, 128, 1024), (1, 9, 16), (1, 2), (0, 5, 11),
                (0, 3), WS, (0,))
    return itertools.product(*dims)


def frag_grid():
    """bf16 with fragment-major weights (w_layout = 1): families 0 / 4, or SBA_E_ARG where no halo kernel takes it"""
    return itertools.product((1, 20, 40), (8, 17, 32, 64), (32, 64, 96, 128), (32, 64, 96, 128), (1, 9), (1,), (0, 7),
                             (0,), WS, (1,))


def glu_grid():
    """(dtype, N, S, Cin, C, ntaps, ups, w_layout) of the sba_conv_igemm_glu_plan queries"""
    return itertools.product((0, 1), (1, 7, 20, 40), (8, 17, 32, 64), (32, 64, 128), (8, 32, 48, 64, 256), (1, 9),
                             (0, 1), (0, 1))


def replay(_lib):
    """the answers of the library behind `_lib` on every grid: name -> int16 array of (rc, plan[0], plan[1], plan[2])"""
    plan = (ctypes.c_int * 3)()

    def conv(dtype, grid):
        rows = []
        for N, S, Cin, Cout, ntaps, stride, tile, ksplit, ws, wl in grid:
            g = _geom(_lib, N, S, Cin, Cout, ntaps, stride)
            g.tile, g.ksplit, g.w_layout = tile, ksplit, wl
            plan[0] = plan[1] = plan[2] = -1
            rc = _lib.lib.sba_conv_igemm_plan(dtype, ctypes.byref(g), ws, plan)
            rows.append((rc, plan[0], plan[1], plan[2]))
        return np.array(rows, dtype=np.int16)

    out = {'bf16': conv(_lib.SBA_BF16, conv_grid(True)), 'f32': conv(_lib.SBA_F32, conv_grid(False)),
           'frag': conv(_lib.SBA_BF16, frag_grid())}
    rows = []
    for dtype, N, S, Cin, C, ntaps, ups, wl in glu_grid():
        g = _geom(_lib, N, S, Cin, 64 * ((C + 31) // 32), ntaps, 1, ups)
        g.w_layout = wl
        plan[0] = plan[1] = plan[2] = -1
        rc = _lib.lib.sba_conv_igemm_glu_plan(dtype, ctypes.byref(g), C, plan)
        rows.append((rc, plan[0], plan[1], plan[2]))
    out['glu'] = np.array(rows, dtype=np.int16)
    return out


def test_igemm_plans_equal_the_recorded_ones():
    from sbagan import _lib
    want = np.load(GOLDEN)
    got = replay(_lib)
    assert set(want.files) == set(got)
    # the recording itself covers what it claims to: every family, and every tile id in both LDS-DMA generations
    bf = want['bf16']
    assert len(bf) == 622080 and (bf[:, 0] == 0).all()
    assert [int((bf[:, 1] == f).sum()) for f in range(4)] == [2880, 292344, 293760, 33096]
    for fam in (1, 2):
        ids = bf[bf[:, 1] == fam, 2]
        assert all((ids == t).sum() >= 15408 for t in range(1, _lib.IGEMM_TILES + 1) if t != 11 and (fam == 1 or t <= 12))
    for name in want.files:
        w, g = want[name], got[name]
        assert w.shape == g.shape, name
        bad = np.nonzero((w != g).any(axis=1))[0]
        assert bad.size == 0, '%s: %d of %d rows differ, first at %d: recorded %s, now %s' % (
            name, bad.size, len(w), bad[0], w[bad[0]].tolist(), g[bad[0]].tolist())
