"""The C ABI of libsbagan_hip.so as include/sbagan_hip.h declares it, read from the header itself: its integer #defines,
its structs as ctypes.Structure classes and its prototypes with their ctypes.  Pure Python (no torch, no library), and
the only reader of the header: sbagan._lib binds from DECLS, sbagan.ops takes its descriptor layouts from STRUCTS.

Regular expressions over the comment-stripped text, not a C grammar: the header is written in the few forms below, and
whatever is not one of them raises at import, naming the declaration.  Nothing is skipped or defaulted."""
import os
import re
from collections import namedtuple
from ctypes import (POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int8, c_int32, c_int64, c_uint64,
                    c_void_p)

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))),
                      'include', 'sbagan_hip.h')
EXT_HEADER = os.path.join(os.path.dirname(HEADER), 'sbagan_hip_ext.h')

# The type map.  Scalars by name; `int*` and `void**` are host out-parameters; a pointer to one of HOST_STRUCTS is a
# struct the host fills in; every other pointer is an address (device memory, a stream, a handle): c_void_p.
TYPES = {'int': c_int, 'int64_t': c_int64, 'uint64_t': c_uint64, 'float': c_float, 'double': c_double,
         'int*': POINTER(c_int), 'void**': POINTER(c_void_p)}
FIELD_TYPES = dict(TYPES, int32_t=c_int32, int8_t=c_int8)
RETURNS = {'int': c_int, 'int64_t': c_int64, 'const char*': c_char_p}
HOST_STRUCTS = ('sba_conv_geom', 'sba_conv_group_item')

Decl = namedtuple('Decl', 'ret restype params')       # C return type, its ctype, [(C type, parameter name, ctype)]


def _squeeze(ctext):
    return re.sub(r'\s*\*', '*', ' '.join(ctext.split()))


def _ctype(ctext, types, structs, host_structs, where):
    base = re.sub(r'\bconst\b|\s', '', ctext)
    if base in types:
        return types[base]
    if base.endswith('*') and base[:-1] in host_structs:
        if base[:-1] not in structs:
            raise ValueError('%s: %s is used before it is declared' % (where, base[:-1]))
        return POINTER(structs[base[:-1]])
    if re.fullmatch(r'\w+\*+', base):
        return c_void_p
    raise ValueError('%s: unknown type %r' % (where, ctext))


def parse(text, host_structs=HOST_STRUCTS):
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    constants, structs, decls = {}, {}, {}

    def new(name):
        if name in constants or name in structs or name in decls:
            raise ValueError('%s is declared twice' % name)
        return name

    for m in re.finditer(r'^[ \t]*#[ \t]*define[ \t]+(SBA_\w+)(.*)$', text, flags=re.M):
        value = re.fullmatch(r'\s+\(?(-?\d+)\)?\s*', m.group(2))
        if not value:
            raise ValueError('#define %s: not an integer: %r' % (m.group(1), m.group(2).strip()))
        constants[new(m.group(1))] = int(value.group(1))
    text = re.sub(r'^[ \t]*#.*$', '', text, flags=re.M)

    def struct(m):
        name, fields = m.group(1), []
        if m.group(3) != name:
            raise ValueError('typedef struct %s: named %s' % (name, m.group(3)))
        for stmt in filter(None, (s.strip() for s in m.group(2).split(';'))):
            f = re.fullmatch(r'(.*?)(\w+(?:\[\w+\])?(?:\s*,\s*\w+(?:\[\w+\])?)*)', stmt, flags=re.S)
            if not f:
                raise ValueError('struct %s: cannot read %r' % (name, stmt))
            ctype = _ctype(f.group(1), FIELD_TYPES, structs, host_structs, 'struct %s: %r' % (name, stmt))
            for field, bound in re.findall(r'(\w+)(?:\[(\w+)\])?', f.group(2)):
                if bound and not bound.isdigit() and bound not in constants:
                    raise ValueError('struct %s: %s[%s]: unknown bound' % (name, field, bound))
                fields.append((field, ctype * int(constants.get(bound, bound)) if bound else ctype))
        structs[new(name)] = type(name, (Structure,), {'_fields_': fields})
        return ''
    text = re.sub(r'typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;', struct, text, flags=re.S)

    text = re.sub(r'extern\s+"C"\s*\{|\}', '', text)
    for stmt in filter(None, (' '.join(s.split()) for s in text.split(';'))):
        m = re.fullmatch(r'(.+?)\s*\b(sba_\w+)\s*\(([^()]*)\)', stmt)
        if not m:
            raise ValueError('cannot read the declaration %r' % stmt)
        ret, name = _squeeze(m.group(1)), m.group(2)
        if ret not in RETURNS:
            raise ValueError('%s: unknown return type %r' % (name, ret))
        params = []
        for p in ([] if m.group(3).strip() in ('', 'void') else m.group(3).split(',')):
            f = re.fullmatch(r'\s*(.*?)\s*(\w+)\s*', p)
            ctext = _squeeze(f.group(1)) if f else p
            params.append((ctext, f.group(2) if f else '', _ctype(ctext, TYPES, structs, host_structs,
                                                                 '%s: parameter %r' % (name, p.strip()))))
        decls[new(name)] = Decl(ret, RETURNS[ret], params)
    return constants, structs, decls


def disjoint(core, ext):
    """refuse a name that both headers declare (constants, structs and entry points share one namespace in C)"""
    names = [set().union(*tables) for tables in (core, ext)]
    both = sorted(names[0] & names[1])
    if both:
        raise ValueError('%s: declared in both headers' % ', '.join(both))


with open(HEADER) as _f:
    CONSTANTS, STRUCTS, DECLS = parse(_f.read())

# The second header: entry points added since the first one's declaration count was pinned by its tests.  Parsed the
# same way into tables of its own; the three above stay those of sbagan_hip.h alone.
with open(EXT_HEADER) as _f:
    EXT_CONSTANTS, EXT_STRUCTS, EXT_DECLS = parse(_f.read())
disjoint((CONSTANTS, STRUCTS, DECLS), (EXT_CONSTANTS, EXT_STRUCTS, EXT_DECLS))
