"""Cases shared by tests/test_context_cache_chain_cpu.py and tests/test_context_cache_chain_gpu.py: the width triples of
csrc/chain_widths.h, read from the header (a triple added there is a case here), and the slot tables of the kernel tests."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def width_table():
    """(D, I, M, MC) of every triple the chain kernels are instantiated for."""
    text = open(os.path.join(ROOT, 'world_modelz_amd', 'csrc', 'chain_widths.h')).read()
    text = '\n'.join(ln for ln in text.splitlines() if not ln.lstrip().startswith('//'))
    rows = [tuple(int(v) for v in m.groups()) for m in re.finditer(r'X\((\d+), (\d+), (\d+), (\d+)\)', text)]
    assert len(rows) >= 12 and len(set(rows)) == len(rows)
    return rows


KERNEL_WIDTHS = width_table()                # what test_slot_launches_are_the_planes_launches_in_place is parametrised over

# planes_out, dst_planes, dst_plane0 (tests/test_context_cache_gpu.py SLOTS; slot 0: no hard-wired last slot)
SLOTS = [(1, 1, 0), (1, 3, 2), (1, 3, 0), (2, 3, 0)]

# (n_q, dst_planes, dst_plane0) the entry points are asked about, and whether fused_slots_ok (csrc/fused_row_maps.h) accepts them:
# the n_q slots from dst_plane0 on lie inside the dst_planes slots
SLOT_TABLE = [(1, 1, 0), (1, 3, 2), (1, 3, 0), (2, 3, 0), (2, 3, 1), (3, 3, 0), (1, 5, 4),
              (1, 3, -1), (1, 3, 3), (2, 3, 2), (1, 0, 0), (3, 2, 0), (1, 5, 5), (2, 2, -1)]


def slots_ok(n_q, dst_planes, dst_plane0):
    return n_q > 0 and dst_plane0 >= 0 and dst_plane0 + n_q <= dst_planes
