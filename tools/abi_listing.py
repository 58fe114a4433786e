#!/usr/bin/env python3
"""What sbagan._lib binds, as text: every entry point of include/sbagan_hip.h with the argtypes and restype set on the
loaded library, the layout of the structs that cross the ABI, and the constants.  Types are spelled by structure (a
struct pointer lists the fields it points to), so the listing does not depend on what a Python class is called.  Two
checkouts bind the same ABI when their listings are equal:  python tools/abi_listing.py > listing.txt"""
import ctypes
import hashlib
import os
import re
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'sba-gan_amd'))

CONSTANTS = ('SBA_F32', 'SBA_BF16', 'SBA_BF16_YH', 'ACT_NONE', 'ACT_GLU', 'ACT_LRELU', 'ACT_RELU', 'MAX_TAPS',
             'IGEMM_TILES', 'WGRAD_PLAN_INTS', 'GROUP_MAX', 'WGRAD_FAMILIES', '_ERR')


def spell(t, full=False):
    """full: a struct with its fields and offsets; else by size and a digest of that full spelling"""
    if t is None:
        return 'None'
    if issubclass(t, ctypes.Structure):
        s = 'struct{%s}' % ', '.join('%s %s @%d' % (spell(ft), f, getattr(t, f).offset) for f, ft in t._fields_)
        return s if full else 'struct<%d bytes, %s>' % (ctypes.sizeof(t), hashlib.sha1(s.encode()).hexdigest()[:10])
    if issubclass(t, ctypes.Array):
        return '%s[%d]' % (spell(t._type_), t._length_)
    if issubclass(t, ctypes._Pointer):
        return 'POINTER(%s)' % spell(t._type_)
    return t.__name__


def main():
    import numpy as np
    from sbagan import _lib, ops
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'sbagan_hip.h')).read(), flags=re.S)
    names = sorted(set(re.findall(r'\b(sba_\w+)\s*\(', text)))
    print('== %d entry points ==' % len(names))
    for name in names:
        fn = getattr(_lib.lib, name)
        print('%s %s(%s)' % (spell(fn.restype), name, ', '.join(spell(t) for t in fn.argtypes)))
    print('== SIGNATURES: %d keys, each the argtypes above: %s ==' % (
        len(_lib.SIGNATURES), all(list(getattr(_lib.lib, n).argtypes) == list(s) for n, s in _lib.SIGNATURES.items())))
    print(textwrap.fill(' '.join(sorted(_lib.SIGNATURES)), 118))
    print('== structs ==')
    for name, t in (('sba_conv_geom', _lib.ConvGeom), ('sba_conv_group_item', _lib.ConvGroupItem)):
        print('%s = %s: %s' % (name, spell(t), spell(t, full=True)))
    print('G is POINTER(ConvGeom):', _lib.G is ctypes.POINTER(_lib.ConvGeom))
    structs = getattr(_lib, 'STRUCTS', {})      # ops.py's descriptor arrays: generated structs, or dtype field lists
    for name, fields in (('sba_frag_desc', getattr(ops, '_FRAG_DESC', None)),
                         ('sba_pack_desc', getattr(ops.PackGroup, '_DESC', None))):
        dt = np.dtype(fields, align=True) if fields else np.dtype(structs[name])
        print('%s: %d bytes, %s' % (name, dt.itemsize, ', '.join(
            '%s %s @%d' % (dt.fields[f][0].str, f, dt.fields[f][1]) for f in dt.names)))
    print('== constants ==')
    for name in CONSTANTS:
        print('%s = %r' % (name, getattr(_lib, name)))


if __name__ == '__main__':
    main()
