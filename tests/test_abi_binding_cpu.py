"""The ctypes binding is read from include/wmz.h and csrc/wmz_debug.h (world_modelz_amd/_lib.py::parse_header): the reader against
declarations written out by hand, against a count it does not make itself, and against headers it has to refuse."""
import ctypes
import re

import pytest

import abi_header

vp, i, l, f, d, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_double, ctypes.c_ulonglong

# (restype, argtypes) transcribed from include/wmz.h by hand, one declaration per kind of argument
PINNED = {
    'wmz_local3d_attn_bwd': (i, [vp] * 10 + [i] * 9 + [l] * 8 + [i, vp]),                               # long strides
    'wmz_linear_wgrad_batch_ln': (i, [i] + [vp] * 15 + [l, i, vp]),                                     # host tables of pointers
    'wmz_corrupt_tokens_dev': (i, [vp, l, vp, vp, l, vp, i, i, i, u64, u64, vp, vp]),                   # unsigned long long, and a pointer to one
    'wmz_conv_point_fwd_bn': (i, [vp] * 11 + [f] + [i] * 10 + [f, vp]),                                 # const wmz_bn_stats* between floats
    'wmz_bn_finalize': (i, [vp, vp, d] + [vp] * 4 + [d, d, i] + [vp] * 4 + [i, vp, vp]),                # doubles
    'wmz_linear_wgrad_workspace_floats': (l, [i] * 4),                                                  # a long return
}


def test_reader_against_written_out_declarations_and_argument_counts():
    from world_modelz_amd import _lib
    for name, want in PINNED.items():
        assert _lib.DECLARATIONS[name] == want, name
        assert _lib.SIGNATURES[name] == want[1], name
    both = abi_header.code() + abi_header.code(abi_header.DEBUG_HEADER)
    assert set(_lib.DECLARATIONS) == set(re.findall(r'\b(wmz_[a-z0-9_]+)\s*\(', both))
    assert len(_lib.DECLARATIONS) >= 115
    for name, (restype, argtypes) in _lib.DECLARATIONS.items():
        path = abi_header.DEBUG_HEADER if name.startswith('wmz_debug_') else abi_header.HEADER
        args = abi_header.arguments(name, path)
        assert len(argtypes) == (0 if args.strip() in ('', 'void') else args.count(',') + 1), name
        assert restype in (i, l, ctypes.c_char_p), name
        if name.endswith('_f16'):                      # the half forms take their base forms' arguments
            assert _lib.DECLARATIONS[name] == _lib.DECLARATIONS[name[:-4]], name
    assert sum(name.endswith('_f16') for name in _lib.DECLARATIONS) == 12
    assert _lib.DECLARATIONS['wmz_version'] == (i, []) and _lib.DECLARATIONS['wmz_last_error'] == (ctypes.c_char_p, [])


def test_constants_come_from_the_header():
    from world_modelz_amd import _lib, fused, half_guard, ops
    assert _lib.EXPECTED_VERSION == 115 == abi_header.constants('WMZ_VERSION')['WMZ_VERSION']
    assert (_lib.WMZ_F32, _lib.WMZ_BF16, _lib.WMZ_F16) == (0, 1, 2)
    assert (_lib.WMZ_LIN_GELU, _lib.WMZ_LIN_GELU_IN, _lib.WMZ_LIN_DGELU) == tuple(abi_header.constants('WMZ_LIN_').values()) == (1, 2, 4)
    assert ops.STAT_REPLICAS == abi_header.constants('WMZ_STAT_REPLICAS')['WMZ_STAT_REPLICAS'] == 8
    assert ((fused.X_IN_TILED, fused.X_OUT_TILED, fused.X1_NORMALISED, fused.XRM_NORMALISED)
            == tuple(abi_header.constants('WMZ_FUSED_X').values()) == (1, 2, 4, 8))
    assert tuple(bit for bit, _ in half_guard.KINDS) == tuple(abi_header.constants('WMZ_HG_').values()) == (1, 2, 4)
    assert abi_header.constants('WMZ_OPERAND_') == {'WMZ_OPERAND_TRANSPOSE': 1, 'WMZ_OPERAND_F32': 2}
    assert len(_lib.CONSTANTS) == 21
    for name, value in _lib.CONSTANTS.items():
        assert abi_header.constants(name + r'\b')[name] == value, name


def test_bn_stats_structure_follows_the_header():
    from world_modelz_amd import _lib
    m = re.search(r'typedef struct wmz_bn_stats \{(.*?)\} wmz_bn_stats;', abi_header.code(), flags=re.S)
    names = [w.split()[-1].lstrip('*') for decl in m.group(1).split(';') for w in decl.split(',') if w.strip()]
    assert names == _lib.BN_STATS_FIELDS == [name for name, _ in _lib.BnStats._fields_] and len(names) == 14
    doubles = ('count', 'momentum', 'eps')
    assert [name for name, t in _lib.BnStats._fields_ if t is d] == list(doubles)
    assert all(t is vp for name, t in _lib.BnStats._fields_ if name not in doubles)
    assert ctypes.sizeof(_lib.BnStats) == 11 * 8 + 3 * 8


def test_reader_refuses_what_it_does_not_know():
    from world_modelz_amd import _lib
    ok = 'enum { WMZ_A = 3 };\n#define WMZ_B 4\nint wmz_f(const void* x, long ld, void* stream); /* wmz_g( in a comment */\nlong wmz_n(void);\n'
    fns, consts, fields = _lib.parse_header(ok)
    assert fns == {'wmz_f': (i, [vp, l, vp]), 'wmz_n': (l, [])} and consts == {'WMZ_A': 3, 'WMZ_B': 4} and fields == []
    with pytest.raises(_lib.WmzError, match='size_t n'):
        _lib.parse_header(ok + 'int wmz_h(const void* x, size_t n);\n')               # a type outside the table
    with pytest.raises(_lib.WmzError, match='wmz_h'):
        _lib.parse_header(ok + 'void wmz_h(int n);\n')                                # a return type outside int / long / const char*
    with pytest.raises(_lib.WmzError, match='wmz_h'):
        _lib.parse_header(ok + 'int wmz_h(int (*callback)(int), void* stream);\n')    # no `ret wmz_name(args);` shape
    with pytest.raises(_lib.WmzError):
        _lib.parse_header(ok + 'int wmz_h(int);\n')                                   # an unnamed parameter: no base type left
    with pytest.raises(_lib.WmzError):
        _lib.parse_header('enum { WMZ_A = 1 << 2 };\n')
