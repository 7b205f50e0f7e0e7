"""The context cache at the chain kernels' widths, host side: the new entry points in include/wmz.h, in the built
library and in the binding derived from the header; what wmz_layer_chain_fwd_slots refuses, asked without a device; and that the
GPU kernel test covers every width triple the library holds.

The refusal is asked of the library itself: with widths no unit is built for, an accepted slot triple ends in
WMZ_ERR_UNSUPPORTED behind the slot check and in front of any launch, a refused one in WMZ_ERR_ARG with the slot message -- no
pointer is read on either way."""
import ctypes

import pytest

import chain_cache_cases as cases

# (the half form is the slots form of the _f16 entry point, `_f16_slots`: tests/test_abi_binding_cpu.py pins the number of
#  declarations that END in _f16)
NEW = ('wmz_layer_chain_fwd_slots', 'wmz_layer_chain_fwd_f16_slots', 'wmz_embed_pos3d_fwd_planes')


def test_header_declares_the_entry_points_and_the_binding_exposes_them():
    import abi_header
    from world_modelz_amd import _lib
    assert set(NEW) <= abi_header.declared()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
    # the trailing-planes form's arguments, then int dst_planes, int dst_plane0 in front of the stream
    planes = 'wmz_layer_chain_fwd_planes'
    want = _lib.SIGNATURES[planes][:-1] + [_lib.c_int, _lib.c_int, _lib.c_void_p]
    assert _lib.SIGNATURES['wmz_layer_chain_fwd_slots'] == want == _lib.SIGNATURES['wmz_layer_chain_fwd_f16_slots']
    assert _lib.SIGNATURES[planes] == _lib.SIGNATURES[planes + '_f16']
    args = [a.split()[-1].lstrip('*') for a in abi_header.arguments('wmz_layer_chain_fwd_slots').split(',')]
    assert args[-3:] == ['dst_planes', 'dst_plane0', 'stream']
    assert args[:-3] == [a.split()[-1].lstrip('*') for a in abi_header.arguments(planes).split(',')][:-1]
    # wmz_embed_pos3d_fwd with planes_out behind the grid
    full = [a.split()[-1].lstrip('*') for a in abi_header.arguments('wmz_embed_pos3d_fwd').split(',')]
    part = [a.split()[-1].lstrip('*') for a in abi_header.arguments('wmz_embed_pos3d_fwd_planes').split(',')]
    assert part == full[:full.index('W') + 1] + ['planes_out'] + full[full.index('W') + 1:]
    abi_header.assert_bound(_lib.lib(), *NEW)                       # exported by the built library


@pytest.mark.parametrize('name', NEW[:2])
def test_the_slot_check_is_fused_slots_ok(name):
    from world_modelz_amd import _lib
    L = _lib.lib()
    ARG, UNSUPPORTED = _lib.CONSTANTS['WMZ_ERR_ARG'], _lib.CONSTANTS['WMZ_ERR_UNSUPPORTED']
    assert len({0, ARG, UNSUPPORTED}) == 3
    room = ctypes.create_string_buffer(64)                          # an address to hand over: never read (nothing is launched)
    p = ctypes.addressof(room)
    fn = getattr(L, name)
    D = I = M = 8                                                   # no unit holds these widths
    assert L.wmz_layer_chain_supported(D, I, M, None) == 0
    assert any(not cases.slots_ok(*t) for t in cases.SLOT_TABLE) and any(cases.slots_ok(*t) for t in cases.SLOT_TABLE)
    for n_q, dp, d0 in cases.SLOT_TABLE:
        for head in (0, 1):
            rc = fn(p, p, p, p, p, p, p, 2, n_q, n_q + 1, 24, D, I, M, head, 1, 1e-5,
                    dp, d0, None)
            msg = L.wmz_last_error().decode()
            if cases.slots_ok(n_q, dp, d0):
                assert rc == UNSUPPORTED and 'not built' in msg, (n_q, dp, d0, rc, msg)
            else:
                assert rc == ARG and 'must lie inside the dst_planes slots' in msg and name in msg, (n_q, dp, d0, rc, msg)
    # a launch without a tail places nothing, but the slots it names are checked all the same
    rc = fn(p, p, p, None, None, p, p, 2, 1, 1, 24, D, I, M, 1, 0, 1e-5, 3, 3, None)
    assert rc == ARG and 'must lie inside the dst_planes slots' in L.wmz_last_error().decode()


def test_the_gpu_kernel_test_covers_every_width_the_library_holds():
    from world_modelz_amd import _lib
    L = _lib.lib()
    table = cases.width_table()
    assert cases.KERNEL_WIDTHS == table and len(table) >= 12
    held = set()
    for D in range(32, 513, 32):                                    # (the templates take multiples of 32 up to 512: chain_widths.h)
        for I in (64, 128, 192, 256, 384, 512):
            for M in (128, 256, 512, 1024, 2048):
                mc = ctypes.c_int(0)
                if L.wmz_layer_chain_supported(D, I, M, ctypes.byref(mc)):
                    held.add((D, I, M, mc.value))
    assert held == set(table)
    import test_context_cache_chain_gpu as gpu                      # (importable without a device: its tests are marked gpu)
    marks = [m for m in gpu.test_slot_launches_are_the_planes_launches_in_place.pytestmark if m.name == 'parametrize']
    widths = [m for m in marks if m.args[0] == 'widths']
    assert len(widths) == 1 and list(widths[0].args[1]) == table
