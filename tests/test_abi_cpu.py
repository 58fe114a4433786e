"""sbagan/abi.py, the one reader of include/sbagan_hip.h, on its own: small header texts written here for every form it
has to read and every refusal it has to make, then the real header's counts, sizes and offsets as explicit numbers.
Needs neither torch nor the library."""
import ast
import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int8, c_int32, c_int64, c_uint64, c_void_p

import numpy as np
import pytest

from sbagan import abi

TEXT = '''
#ifndef T_H
#define T_H
#include <stdint.h>
#define SBA_OK 0
#define SBA_E_ARG (-1)      /* a comment; with ( and a fake prototype: int sba_fake(int x); */
#define SBA_MAX_TAPS 3
typedef struct sba_conv_geom {
    int32_t N, IH;
    int8_t ty[SBA_MAX_TAPS];    /* bounded by a #define */
    int8_t tx[2], pad;
    int32_t tile;
} sba_conv_geom;
typedef struct sba_conv_group_item {
    const void* x; const float* bias; const sba_conv_geom* g;
} sba_conv_group_item;
typedef struct sba_dev_desc { const sba_conv_geom* g; int32_t n; } sba_dev_desc;
const char* sba_version(void);
/* int sba_commented_out(int a); */
int sba_three_lines(int dtype, const void* x, float* y, const sba_conv_geom* g,
                    int64_t n, uint64_t seed, float eps,
                    double tol, int* plan, void** out, const sba_dev_desc* descs, void* stream);
int64_t sba_bytes(int n, int S);   // int sba_line_comment(void);
int sba_none();
#endif
'''


def test_small_header_parses():
    constants, structs, decls = abi.parse(TEXT)
    assert constants == {'SBA_OK': 0, 'SBA_E_ARG': -1, 'SBA_MAX_TAPS': 3}
    assert list(structs) == ['sba_conv_geom', 'sba_conv_group_item', 'sba_dev_desc']
    geom, item, dev = structs.values()
    assert geom._fields_ == [('N', c_int32), ('IH', c_int32), ('ty', c_int8 * 3), ('tx', c_int8 * 2), ('pad', c_int8),
                             ('tile', c_int32)]
    assert [getattr(geom, n).offset for n in ('ty', 'tx', 'pad', 'tile')] + [ctypes.sizeof(geom)] == [8, 11, 13, 16, 20]
    # two statements on one line; a pointer to an earlier host struct is typed, any other pointer is an address
    assert item._fields_ == [('x', c_void_p), ('bias', c_void_p), ('g', POINTER(geom))]
    assert dev._fields_ == [('g', POINTER(geom)), ('n', c_int32)] and ctypes.sizeof(dev) == 16
    assert list(decls) == ['sba_version', 'sba_three_lines', 'sba_bytes', 'sba_none']      # not the commented ones
    assert decls['sba_version'] == ('const char*', c_char_p, []) and decls['sba_none'] == ('int', c_int, [])
    assert decls['sba_bytes'] == ('int64_t', c_int64, [('int', 'n', c_int), ('int', 'S', c_int)])
    d = decls['sba_three_lines']
    assert (d.ret, d.restype) == ('int', c_int)
    assert d.params == [
        ('int', 'dtype', c_int), ('const void*', 'x', c_void_p), ('float*', 'y', c_void_p),
        ('const sba_conv_geom*', 'g', POINTER(geom)), ('int64_t', 'n', c_int64), ('uint64_t', 'seed', c_uint64),
        ('float', 'eps', c_float), ('double', 'tol', c_double), ('int*', 'plan', POINTER(c_int)),
        ('void**', 'out', POINTER(c_void_p)), ('const sba_dev_desc*', 'descs', c_void_p), ('void*', 'stream', c_void_p)]


@pytest.mark.parametrize('text,names', [
    ('int sba_f(int a, short b);', ('sba_f', 'short b')),                             # a scalar outside the map
    ('int sba_f(int32_t n);', ('sba_f', 'int32_t n')),                                # (struct fields only)
    ('typedef struct sba_s { int32_t a; long b; } sba_s;', ('sba_s', 'long b')),
    ('int sba_f(int);', ('sba_f', 'int')),                                            # no parameter name
    ('int sba_f(int a);\nint64_t sba_f(void);', ('sba_f', 'twice')),
    ('#define SBA_A 1\n#define SBA_A 2', ('SBA_A', 'twice')),
    ('typedef struct sba_s { int32_t a; } sba_s;\nint sba_s(void);', ('sba_s', 'twice')),
    ('float sba_f(int a);', ('sba_f', 'float')),                                      # a return type outside the three
    ('#define SBA_A 1.5', ('SBA_A', '1.5')),
    ('typedef struct sba_s { int8_t t[SBA_N]; } sba_s;', ('sba_s', 'SBA_N')),         # an array bound never defined
    ('typedef struct sba_s { int32_t a; } sba_t;', ('sba_s', 'sba_t')),
    ('int sba_f(const sba_conv_geom* g);', ('sba_f', 'sba_conv_geom')),               # a host struct not declared yet
    ('int other_f(int a);', ('other_f',)),
    ('static int x = 3;', ('static int x = 3',))])
def test_refusals_name_the_declaration(text, names):
    with pytest.raises(ValueError) as e:
        abi.parse(text)
    for name in names:
        assert name in str(e.value), (name, str(e.value))


def test_real_header_counts_sizes_and_offsets():
    assert len(abi.DECLS) == 134
    assert sum(d.restype is c_int for d in abi.DECLS.values()) == 124
    assert sum(d.restype is c_int64 for d in abi.DECLS.values()) == 9
    assert [n for n, d in abi.DECLS.items() if d.restype is c_char_p] == ['sba_version']
    assert len(abi.CONSTANTS) == 16
    assert [abi.CONSTANTS['SBA_' + k] for k in ('E_ARG', 'E_LAUNCH', 'E_UNSUPPORTED', 'GROUP_MAX')] == [-1, -2, -3, 8]
    assert [abi.CONSTANTS['SBA_' + k] for k in ('MAX_TAPS', 'IGEMM_TILES', 'WGRAD_PLAN_INTS')] == [32, 18, 14]
    assert {n: ctypes.sizeof(s) for n, s in abi.STRUCTS.items()} == {
        'sba_conv_geom': 168, 'sba_conv_group_item': 56, 'sba_pack_desc': 56, 'sba_frag_desc': 32}
    geom, item = abi.STRUCTS['sba_conv_geom'], abi.STRUCTS['sba_conv_group_item']
    assert [n for n, _ in geom._fields_] == ('N IH IW Cin OH OW Cout OHs OWs sy sx osy osx ooy oox ups ntaps ty tx x_cstride '
                                             'x_coff y_cstride y_coff relu tile ksplit first_write w_layout').split()
    assert all(t is c_int32 for n, t in geom._fields_ if n not in ('ty', 'tx'))
    assert geom.ty.size == geom.tx.size == 32 and dict(geom._fields_)['ty'] is c_int8 * 32
    assert (geom.N.offset, geom.ntaps.offset, geom.ty.offset, geom.tx.offset, geom.x_cstride.offset,
            geom.w_layout.offset) == (0, 64, 68, 100, 132, 164)
    assert item._fields_ == [(n, c_void_p) for n in ('x', 'w', 'y', 'addend', 'bias', 'relu_mask')] + [('g', POINTER(geom))]
    assert [getattr(item, n).offset for n, _ in item._fields_] == [0, 8, 16, 24, 32, 40, 48]


def test_descriptor_layouts_the_kernels_read():
    """sba_frag_desc and sba_pack_desc are read from DEVICE memory by the packing kernels: field by field"""
    def layout(name):
        dt = np.dtype(abi.STRUCTS[name])
        return ' '.join('%s:%s@%d' % (n, dt.fields[n][0].str, dt.fields[n][1]) for n in dt.names) + ' size %d' % dt.itemsize
    assert layout('sba_frag_desc') == 'src:<u8@0 dst:<u8@8 R:<i4@16 taps:<i4@20 K:<i4@24 unit_begin:<i4@28 size 32'
    assert layout('sba_pack_desc') == ('w:<u8@0 fwd:<u8@8 tr:<u8@16 Cout:<i4@24 KH:<i4@28 KW:<i4@32 Cin:<i4@36 mode:<i4@40 '
                                       'tile_begin:<i4@44 co_tiles:<i4@48 ci_tiles:<i4@52 size 56')


def test_parser_stands_alone():
    """it imports the standard library only: neither torch nor the library (its package's __init__ is empty)"""
    nodes = list(ast.walk(ast.parse(open(abi.__file__).read())))
    mods = {a.name for n in nodes if isinstance(n, ast.Import) for a in n.names} | \
           {'.' * n.level + (n.module or '') for n in nodes if isinstance(n, ast.ImportFrom)}
    assert mods <= {'os', 're', 'collections', 'ctypes'}, mods
    assert not open(os.path.join(os.path.dirname(abi.__file__), '__init__.py')).read().strip()
