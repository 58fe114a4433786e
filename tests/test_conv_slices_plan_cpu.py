"""sba_conv_igemm_plan needs no device: every single-launch case of tests/test_conv_slices_gpu.py must take the kernel
family, the tile and the K splits it is listed for (the case tables are imported, so the two cannot drift), and between
them the cases must reach every family."""
import ctypes

import test_conv_slices_gpu as S


def plan_of(_lib, c, sliced):
    g = S.geom_of(c, S.slices(c, sliced))
    cg = _lib.ConvGeom()
    for name, _ in cg._fields_:
        if name not in ('ty', 'tx'):
            setattr(cg, name, getattr(g, name))
    for t in range(g.ntaps):
        cg.ty[t], cg.tx[t] = g.ty[t], g.tx[t]
    M = c.N * c.OHs * c.OWs
    ws_bytes = {'none': 0, 'full': 4 * M * c.Cout, 'small': 4 * M * c.Cout - 16}[c.ws]
    plan = (ctypes.c_int * 3)(-1, -1, -1)
    code = _lib.SBA_BF16 if c.mode == 'yh' else S.MODES[c.mode][0]       # (the binary16 output takes the bf16 kernels)
    rc = _lib.lib.sba_conv_igemm_plan(code, ctypes.byref(cg), ws_bytes, plan)
    return rc, tuple(plan)


def test_slice_cases_take_the_kernels_they_name():
    from sbagan import _lib
    assert len(set(c.id for c in S.PLAN_CASES)) == len(S.PLAN_CASES)
    for c in S.PLAN_CASES:
        for sliced in (True, False):        # the slice fields do not enter the choice
            assert plan_of(_lib, c, sliced) == (0, c.plan), (c.id, sliced, plan_of(_lib, c, sliced), c.plan)
    fam = dict((c.id, c.plan[0]) for c in S.PLAN_CASES)
    assert set(fam.values()) == {0, 1, 2, 3, 4}
    # what the issue's table names per case number
    want = {'1': 1, '2': 1, '3': 2, '4': 3, '5': 1, '6': 1, '7': 2, '8a': 3, '8b': 3, '9': 0, '10a': 4, '10b': 4,
            '10c': 4, '10d': 4, '10e': 4, '10f': 4, '11': 1}
    for c in S.PLAN_CASES:
        assert fam[c.id] == want[c.id.split('-')[0]], c.id
    by_id = dict((c.id, c) for c in S.PLAN_CASES)
    assert by_id['4'].mode == 'bf16' and by_id['4'].tile == 11                      # family 3 in bf16
    assert by_id['5-rule-full-add_mask'].plan[2] > 1 and by_id['5-t1k3-full-add_mask'].plan[2] == 3
    assert by_id['5-rule-small-add_mask'].plan[2] == 1 and by_id['8b'].plan[2] > 1
    assert set(c.tile for c in S.SINGLE if c.id.startswith('2-')) == {0, 3, 7, 12, 14}
    assert set(c.tile for c in S.SINGLE if c.id.startswith('3-')) == {0, 1, 5, 9}
    # the scalar tail of the bf16 epilogue needs Cout % 8 != 0
    assert all(c.Cout % 8 == 4 for c in S.SINGLE if c.id.startswith('2-'))
    # the register-weight halo kernel's four instantiations: (channels per chunk, Cout % 64 == 0)
    assert set((c.plan[1], c.Cout % 64 == 0) for c in S.SINGLE if c.id.startswith('10')) == {
        (32, False), (64, True), (32, True), (64, False)}
    # both halo-tile kernels, behind the upsample and not
    assert set((c.layout, c.ups) for c in S.SINGLE if c.id.startswith('9-')) == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_group_items_are_what_the_group_kernels_need():
    """shapes of the grouped cases: G1 every Cin % 64 == 0, G2 exactly one member at 96, G3 the (M, Cout) of the issue"""
    assert all(c.Cin % 64 == 0 for c in S.G1) and len(S.G1) == 8
    assert [c.Cin % 64 for c in S.G2].count(32) == 1 and len(S.G2) == 5
    assert [(c.N * c.OHs * c.OWs, c.Cout, c.Cin) for c in S.G3] == [(32, 72, 256), (128, 136, 128), (72, 40, 64)]
    assert S.G1[3].N * S.G1[3].OHs * S.G1[3].OWs == 128 and S.G1[3].s == 2
    assert (S.G1[4].N, S.G1[4].IH) == (3, 9) and len(S.G1[4].taps) == 25
    # members of one launch write disjoint channel windows of the tensors they share
    for items in (S.G1, S.G2, S.G3, S.G3_96):
        seen = {}
        for c in items:
            for ch in range(c.yco, c.yco + c.Cout):
                assert (c.yb, ch) not in seen, (c.id, seen.get((c.yb, ch)))
                seen[(c.yb, ch)] = c.id
