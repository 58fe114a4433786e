"""ctypes binding of libsbagan_hip.so.  include/sbagan_hip.h is the only statement of the C ABI: sbagan.abi parses its
prototypes, structs and constants, and every signature, struct and constant below is taken from that parse.

The library is loaded eagerly and every symbol the header declares is bound with explicit argtypes and restype; a
missing library or symbol, or a declaration the parser cannot read, raises at import time -- there is no CPU or
PyTorch fallback behind these calls.
"""
import ctypes
import os

import torch  # noqa: F401  -- FIRST: PyTorch-ROCm brings its own libamdhip64; if this library is loaded before
#                     it, it binds /opt/rocm's copy and its kernels are registered with a HIP runtime that does
#                     not own torch's streams (every launch then fails)
from ctypes import POINTER, byref, c_float, c_int, c_int64, c_uint64, c_void_p

from .abi import CONSTANTS, DECLS, EXT_DECLS, STRUCTS

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('SBA_LIB_PATH') or os.path.join(os.path.dirname(_HERE), 'csrc', 'libsbagan_hip.so')

SBA_F32, SBA_BF16, SBA_BF16_YH = (CONSTANTS['SBA_' + k] for k in ('F32', 'BF16', 'BF16_YH'))
ACT_NONE, ACT_GLU, ACT_LRELU, ACT_RELU = (CONSTANTS['SBA_ACT_' + k] for k in ('NONE', 'GLU', 'LRELU', 'RELU'))
MAX_TAPS, IGEMM_TILES, WGRAD_PLAN_INTS, GROUP_MAX = (
    CONSTANTS['SBA_' + k] for k in ('MAX_TAPS', 'IGEMM_TILES', 'WGRAD_PLAN_INTS', 'GROUP_MAX'))
WGRAD_FAMILIES = ('row_dma', 'small_dma', 'small', 'rows', 'generic')       # sba_conv_wgrad_plan: plan[0]
ConvGeom, ConvGroupItem = STRUCTS['sba_conv_geom'], STRUCTS['sba_conv_group_item']

if not os.path.exists(LIB_PATH):
    raise ImportError('libsbagan_hip.so not built: run `python __graft_entry__.py` or '
                      '`make -C sba-gan_amd/csrc` (expected %s)' % LIB_PATH)
lib = ctypes.CDLL(LIB_PATH)

P, I, F, L, U = c_void_p, c_int, c_float, c_int64, c_uint64
G = POINTER(ConvGeom)

SIGNATURES = {}         # name -> argtypes of the entry points that return int (DECLS has every entry point)
for _name, _decl in DECLS.items():
    _fn = getattr(lib, _name)          # AttributeError if the .so lacks a declared symbol
    _fn.argtypes = _args = [_ctype for _, _, _ctype in _decl.params]
    _fn.restype = _decl.restype
    if _decl.restype is c_int:
        SIGNATURES[_name] = _args

EXT_SIGNATURES = {}     # the same for the second header (include/sbagan_hip_ext.h): its tables stay apart from the core's
for _name, _decl in EXT_DECLS.items():
    _fn = getattr(lib, _name)          # AttributeError if the .so lacks a declared symbol
    _fn.argtypes = _args = [_ctype for _, _, _ctype in _decl.params]
    _fn.restype = _decl.restype
    if _decl.restype is c_int:
        EXT_SIGNATURES[_name] = _args


def signature(name):
    """argtypes of an int-returning entry point of either header, or None"""
    return SIGNATURES.get(name) or EXT_SIGNATURES.get(name)


_ERR = {CONSTANTS['SBA_E_ARG']: 'SBA_E_ARG (unsupported shape/alignment/enum)',
        CONSTANTS['SBA_E_LAUNCH']: 'SBA_E_LAUNCH (HIP launch failed)',
        CONSTANTS['SBA_E_UNSUPPORTED']: 'SBA_E_UNSUPPORTED (graph node kind the replayer cannot re-issue)'}


AUDIT_HOOK = None        # sbagan.stream_audit: called with (name, args) before every launch while an audit records


def call(name, *args):
    """Invoke a C-ABI entry point; non-zero status becomes RuntimeError (the
    reference surfaces errors as Python exceptions)."""
    if AUDIT_HOOK is not None:
        AUDIT_HOOK(name, args)
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise RuntimeError('%s failed: %s' % (name, _ERR.get(rc, rc)))


def wgrad_plan(dtype, g, ksplit, det=None):
    """sba_conv_wgrad_plan: the 14 integers of the launch sba_conv_wgrad would make for geometry `g` (needs no device);
    det = None: the current deterministic-mode flag"""
    plan = (c_int * WGRAD_PLAN_INTS)()
    det = lib.sba_get_deterministic() if det is None else int(det)
    call('sba_conv_wgrad_plan', dtype, byref(g), ksplit, det, plan)
    return list(plan)


def wgrad_plan_name(plan):
    """'row_dma<3,1,5,4> x2': kernel family, template arguments and pixel splits of a wgrad_plan"""
    fam, nargs = WGRAD_FAMILIES[plan[0]], (4, 2, 0, 0, 0)[plan[0]]
    args = ','.join(str(v) for v in plan[1:1 + nargs]) if nargs else ('f32', 'bf16')[plan[1]]
    return '%s<%s> x%d' % (fam, args, plan[7])


def version():
    return lib.sba_version().decode()
