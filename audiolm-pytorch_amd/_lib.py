"""ctypes binding of libaudiolm_hip.so, DERIVED from its C ABI header include/audiolm_hip.h when this module is imported.

The header is the one description of the boundary: parse_header() turns its `int alm_*(...)` prototypes into SIGNATURES (name -> argtypes), its
typedef'd structs into ctypes.Structure classes (AlmTnJob, AlmPackJob, AlmOptTensor, AlmOptPackJob, AlmListEntry) and its integer `#define ALM_*`
lines into CONSTANTS.  A new entry point is declared in the header and defined in csrc/ (every source compiles against the header through
common.hpp): nothing is added here.  A declaration the parser cannot read is an error at import, never a silently missing binding.

This is the reference-side binding a maintainer would add.  There is NO fallback: if the shared
library is missing / cannot be built the import fails loudly, and every op refuses non-CUDA tensors.
"""
from __future__ import annotations

import ctypes
import os
import re
from ctypes import c_char_p, c_float, c_int, c_longlong, c_ulonglong, c_void_p

from .build import HEADER

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('ALM_LIB_PATH') or os.path.join(_HERE, 'libaudiolm_hip.so')      # ALM_LIB_PATH: A/B runs of an alternative build

_P, _F = c_void_p, c_float          # launchlist.py tells pointer and float arguments apart by identity with these
_SCALARS = {'int': c_int, 'long long': c_longlong, 'unsigned long long': c_ulonglong, 'float': _F}
_SCALAR_DECL = re.compile(r'(?:const )?(unsigned long long|long long|int|float)(?: \w+)?')
_DEFINE = re.compile(r'^[ \t]*#[ \t]*define[ \t]+(ALM_\w+)[ \t]+(\S.*?)[ \t]*$', re.M)
_STRUCT = re.compile(r'\btypedef\s+struct\s*(\w*)\s*\{([^{}]*)\}\s*(\w+)\s*;')
_PROTO = re.compile(r'([\w*][\w\s*]*?)\s*\b(alm_\w+)\s*\(([^()]*)\)\s*;')


def _ctype(decl: str, where: str):
    """ctypes type of one parameter / field declaration (`const float* x`, `long long lda`, `int`)"""
    decl = ' '.join(decl.split())
    if '*' in decl:
        return c_char_p if re.fullmatch(r'const char ?\* ?\w*', decl) else _P
    m = _SCALAR_DECL.fullmatch(decl)
    if m is None:
        raise ValueError(f'{where}: unrecognised type in "{decl}"')
    return _SCALARS[m.group(1)]


def parse_header(text: str):
    """C ABI header text -> (prototypes {name: [ctype, ...]}, structs {name: [(field, ctype), ...]}, constants {ALM_*: int}).
    Strict: whatever it cannot read raises ValueError naming the declaration."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    consts = {}
    for name, value in _DEFINE.findall(text):
        try:
            consts[name] = int(value, 0)
        except ValueError:
            raise ValueError(f'#define {name} {value}: not an integer constant') from None
    text = re.sub(r'^[ \t]*#.*$', '', text, flags=re.M)
    structs, protos = {}, {}

    def struct(m):
        tag, body, name = m.groups()
        if tag and tag != name:
            raise ValueError(f'typedef struct {tag} {{...}} {name}: tag and typedef name differ')
        fields = structs[name] = []
        for decl in filter(None, (d.strip() for d in body.split(';'))):
            first, *more = decl.split(',')                       # `int M, N, K`: the first declarator carries the type
            base = re.sub(r'\w+\s*$', '', first).replace('*', ' ')
            for d in [first] + [base + d for d in more]:
                fields.append((re.search(r'(\w*)\s*$', d).group(1), _ctype(d, f'struct {name}')))
        return ' '

    def proto(m):
        ret, name, args = m.groups()
        if ret.split() != ['int']:
            raise ValueError(f'{name}: return type "{" ".join(ret.split())}" is not int')
        args = args.strip()
        protos[name] = [] if args in ('', 'void') else [_ctype(a, name) for a in args.split(',')]
        return ' '

    text = _PROTO.sub(proto, _STRUCT.sub(struct, text))
    m = re.search(r'\balm_\w+\s*\(|\b(typedef|struct)\b', text)    # what no prototype / struct match consumed
    if m:
        line = text[text.rfind('\n', 0, m.start()) + 1:].split('\n', 1)[0].strip()
        raise ValueError(f'cannot parse the declaration at "{line}"')
    return protos, structs, consts


try:
    with open(HEADER) as _fh:
        SIGNATURES, _structs, CONSTANTS = parse_header(_fh.read())         # once per process
except OSError as e:
    raise ImportError(f'{HEADER} (the C ABI header the binding is derived from) cannot be read: {e}') from e
# AlmTnJob, AlmPackJob, AlmOptTensor, AlmOptPackJob, AlmListEntry: the header's typedefs, field for field
globals().update({n: type(n, (ctypes.Structure,), {'_fields_': f, '__doc__': f'{n} of include/audiolm_hip.h'}) for n, f in _structs.items()})
_ERRORS = {v: k for k, v in CONSTANTS.items() if k.startswith('ALM_ERR_')}

_lib = None


class AlmError(RuntimeError):
    pass


def load(build_if_missing: bool = True):
    """Loads (building in-tree with hipcc if necessary) the shared library.  Raises if that is impossible."""
    global _lib
    if _lib is not None:
        return _lib
    if build_if_missing and not os.environ.get('ALM_LIB_PATH'):
        from . import build as _build
        try:
            _build.build(verbose=False)
        except Exception as e:  # no hipcc on the box: fine as long as the prebuilt .so that travelled with the tree matches the sources
            if not os.path.exists(LIB_PATH):
                raise ImportError(f'libaudiolm_hip.so is missing and could not be built: {e}') from e
            if not _build._fresh(_build._digest()):
                raise ImportError(f'libaudiolm_hip.so is stale (csrc/ or include/ changed since it was built) and could not be rebuilt: {e}') from e
    if not os.path.exists(LIB_PATH):
        raise ImportError(f'{LIB_PATH} not found: run `python -c "import __graft_entry__ as g; g.build()"`')
    # torch FIRST: its wheel bundles its own libamdhip64 / libhsa-runtime64, and whichever copy enters the process first serves both torch
    # and this library (same SONAME).  Loaded the other way round, torch ends up on the system runtime it was not built against and every
    # launch fails with hipErrorNoDevice (seen on MI355X when the package was imported before torch).
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise ImportError(f'{LIB_PATH} does not export {name} (declared in include/audiolm_hip.h): stale or foreign library')
        fn.argtypes = argtypes
        fn.restype = c_int
    _lib = lib
    return lib

_BOUND = {}          # name -> bound ctypes function (one dict lookup per call instead of load() + getattr on the CDLL: ~150 calls per training step)
RECORDER = None      # launchlist.Recorder while a stack pass is being recorded (the launches still run: recording is an ordinary step that is also written down)


def call(name: str, *args):
    fn = _BOUND.get(name)
    if fn is None:
        fn = _BOUND[name] = getattr(load(), name)
    if RECORDER is not None:
        RECORDER.note(name, args)
    rc = fn(*args)
    if rc != 0:
        raise AlmError(f'{name} failed with code {rc} ({_ERRORS.get(rc, "hipError_t")})')
    return rc


def query(name: str, *args) -> int:
    """For the int-returning size queries (alm_*_blocks / alm_*_width)."""
    fn = _BOUND.get(name)
    if fn is None:
        fn = _BOUND[name] = getattr(load(), name)
    return fn(*args)
