"""ctypes binding of libwmz_hip.so, read from the headers that declare its C ABI (include/wmz.h, csrc/wmz_debug.h).

There is no CPU fallback: if the library is missing or a call fails, this raises.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('WMZ_LIB_PATH') or os.path.join(_HERE, 'libwmz_hip.so')    # override: kernel A/B builds (tools/)

HEADERS = (os.path.join(os.path.dirname(_HERE), 'include', 'wmz.h'),          # the interface
           os.path.join(_HERE, 'csrc', 'wmz_debug.h'))                        # the development probes (tools/)

_lib = None

c_void_p, c_int, c_long, c_float, c_double = (ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float,
                                              ctypes.c_double)


class WmzError(RuntimeError):
    pass


# The headers are the only place the ABI is written.  parse_header reads what they hold -- declarations `ret wmz_name(args);`, WMZ_*
# enumerators and #defines, the fields of wmz_bn_stats -- and raises on anything else: a type outside these tables, a wmz_name( that
# no declaration accounts for.
_BY_VALUE = {'int': c_int, 'long': c_long, 'int64_t': ctypes.c_int64, 'float': c_float, 'double': c_double,
             'unsigned long long': ctypes.c_ulonglong}          # (an argument with a `*` is a c_void_p, whatever it points to)
_DECLARATION = re.compile(r'\b(int|long|const char\s*\*)\s*(wmz_\w+)\s*\(([^()]*)\)\s*;')


def _argtype(name, arg):
    if '*' in arg:
        return c_void_p
    base = ' '.join(arg.split()[:-1])          # (the last word is the parameter's name)
    if base not in _BY_VALUE:
        raise WmzError(f'{name}: no ctypes type for the argument `{arg.strip()}`')
    return _BY_VALUE[base]


def parse_header(text):
    """C header text -> ({function: (restype, [argtypes])}, {WMZ_* constant: int}, [field names of wmz_bn_stats, in order])."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    constants = {n: int(v) for n, v in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(WMZ_\w+)[ \t]+(\d+)[ \t]*$', text, flags=re.M)}
    text = re.sub(r'^[ \t]*#.*$', '', text, flags=re.M)
    for body in re.findall(r'\benum\s*\{(.*?)\}', text, flags=re.S):
        for item in body.split(','):
            m = re.fullmatch(r'\s*(WMZ_\w+)\s*=\s*(\d+)\s*', item)
            if m is None:
                raise WmzError(f'unreadable enumerator `{item.strip()}`')
            constants[m.group(1)] = int(m.group(2))
    m = re.search(r'\bstruct\s+wmz_bn_stats\s*\{(.*?)\}', text, flags=re.S)
    fields = re.findall(r'(\w+)\s*[,;]', m.group(1)) if m else []
    functions = {}
    for ret, name, args in _DECLARATION.findall(text):
        args = [] if args.strip() in ('', 'void') else args.split(',')
        functions[name] = (ctypes.c_char_p if '*' in ret else _BY_VALUE[ret], [_argtype(name, a) for a in args])
    stray = re.findall(r'\bwmz_\w+\s*\(', _DECLARATION.sub(' ', text))
    if stray:
        raise WmzError(f'declarations the header reader cannot parse: {stray}')
    return functions, constants, fields


def _read_headers():
    functions, constants, fields = {}, {}, []
    for path in HEADERS:
        if not os.path.exists(path):
            raise WmzError(f'{path} not found: the ctypes binding is read from it')
        with open(path) as f:
            fn, cn, fl = parse_header(f.read())
        functions.update(fn)
        constants.update(cn)
        fields += fl
    return functions, constants, fields


DECLARATIONS, CONSTANTS, BN_STATS_FIELDS = _read_headers()                  # once, at import: ~2 ms
SIGNATURES = {name: argtypes for name, (_, argtypes) in DECLARATIONS.items()}
EXPECTED_VERSION = CONSTANTS['WMZ_VERSION']      # bumped with every ABI change; lib() refuses another build
WMZ_F32, WMZ_BF16, WMZ_F16 = (CONSTANTS[n] for n in ('WMZ_F32', 'WMZ_BF16', 'WMZ_F16'))
WMZ_LIN_GELU, WMZ_LIN_GELU_IN, WMZ_LIN_DGELU = (CONSTANTS[n] for n in ('WMZ_LIN_GELU', 'WMZ_LIN_GELU_IN', 'WMZ_LIN_DGELU'))


class BnStats(ctypes.Structure):
    """include/wmz.h wmz_bn_stats: a host struct of device pointers, read by the call."""
    _fields_ = [('sum', c_void_p), ('sq', c_void_p), ('gamma', c_void_p), ('beta', c_void_p), ('running_mean', c_void_p),
                ('running_var', c_void_p), ('num_batches_tracked', c_void_p), ('scale', c_void_p), ('shift', c_void_p),
                ('mean', c_void_p), ('rstd', c_void_p), ('count', c_double), ('momentum', c_double), ('eps', c_double)]


def lib():
    """Load (once) and return the shared library; raises WmzError if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise WmzError(f'{LIB_PATH} not found: build it with `python -m world_modelz_amd.build` '
                           '(there is no CPU fallback for the HIP path)')
        L = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in DECLARATIONS.items():
            fn = getattr(L, name, None)
            if fn is None:
                continue  # declared but not built (a probe behind a -D switch): calling it raises below
            fn.argtypes, fn.restype = argtypes, restype
        if L.wmz_version() != EXPECTED_VERSION:
            raise WmzError(f'{LIB_PATH} is version {L.wmz_version()}, this Python package expects {EXPECTED_VERSION} (include/wmz.h '
                           'WMZ_VERSION): a stale build -- run `python -m world_modelz_amd.build`')
        _lib = L
    return _lib


after_call = None      # ops: launches deferred until the compute stream's NEXT launch has been issued (ops._flush_deferred)


def call(name, *args):
    L = lib()
    fn = getattr(L, name, None)
    if fn is None:
        raise WmzError(f'{name} is not exported by {LIB_PATH}')
    rc = fn(*args)
    if rc != 0:
        raise WmzError(f'{name} failed (code {rc}): {L.wmz_last_error().decode()}')
    if after_call is not None:
        after_call()


def half_form(name, dt):
    """The entry point (or cache tag) `name` for tensors of dtype dt: its _f16 form for IEEE half, else `name` itself."""
    return name + '_f16' if dt == torch.float16 else name


def dtype_code(dt):
    if dt == torch.float32:
        return WMZ_F32
    if dt == torch.bfloat16:
        return WMZ_BF16
    if dt == torch.float16:
        return WMZ_F16          # (the precise fused inference mode: the few entry points that take it say so in include/wmz.h)
    raise WmzError(f'unsupported activation dtype {dt}: the HIP path computes in float32 or bfloat16')


def ptr(t):
    """Device pointer of a tensor (None -> NULL).  CPU tensors are refused: the product path is GPU-only."""
    if t is None:
        return None
    if not t.is_cuda:
        raise WmzError('libwmz_hip.so needs device (ROCm) tensors; got a CPU tensor '
                       '(the CPU oracle lives under oracle/ and is test infrastructure only)')
    return t.data_ptr()


_COLUMN = {'p': c_void_p, 'i': c_int, 'l': c_long}


def columns(rows, kinds):
    """The per-problem argument arrays of a batched entry point: rows = one tuple per problem, kinds = one letter per column
    ('p' pointer: an address or None for NULL, 'i' int, 'l' long) -> one ctypes array of len(rows) per column."""
    assert all(len(r) == len(kinds) for r in rows)
    return [(_COLUMN[k] * len(rows))(*[r[j] for r in rows]) for j, k in enumerate(kinds)]


def stream():
    return torch.cuda.current_stream().cuda_stream
