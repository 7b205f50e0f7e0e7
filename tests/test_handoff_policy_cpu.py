"""Cache-policy bits (sc0 / sc1 / nt) of the global stores, loads and LDS-DMA requests of the forward step's kernels, read from the
ISA (compiled for gfx950, no GPU needed): the inference units carry exactly the bits of SHIPPED below, on exactly that many
instructions, every run-time kernel of the same sources carries none, and the register budgets of the units hold.

The policy is a compile-time parameter of the store / load helpers (csrc/mem_policy.h, fused_common.h) that only
the per-token inference unit sets; what was measured for each class of stores and loads: profiles/handoff_policy/README.md."""
import importlib.util
import os
import re
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


fused_isa, attn_isa = _tool('fused_infer_isa'), _tool('attn_infer_isa')
pytestmark = pytest.mark.skipif(fused_isa.hipcc() is None, reason='hipcc not available')

UNITS = ('layer_fused.hip', 'layer_fused_f16.hip', 'attn_fwd_row16_infer.hip', 'attn_fwd_row16.hip', 'attn_fwd_row32.hip')
# What the inference units ship, per kernel (a substring of its mangled name): {(instruction, policy bits): count}.  A kernel that is
# not named here -- every run-time kernel -- may carry no policy bit at all.  Global memory instructions per kernel, for reference:
#   layer_fused_infer_kernel<true, true>     40 stores (16 x | 8 q | 8 k | 8 v), 16 residual loads, 8 o-tile LDS-DMA requests of 61
#   layer_fused_infer_kernel<true, false>    16 stores (the row-major stream),   16 residual loads, 8 o-tile LDS-DMA requests of 37
#   layer_fused_infer_kernel<false, true>    40 stores (16 x | 8 q | 8 k | 8 v)
#   attn_fwd_row16_infer_kernel<3, 3>, <1, 1>  4 stores (o), 4 Q loads, 22 K / V LDS-DMA requests
# Shipped: the tiled stream, q and k | v are written through (sc1) -- every store of the two kernels with a tail; the last layer's
# row-major stream, the attention output, every load and every LDS-DMA request stay plain.
SC1_STORE = ('global_store_dwordx4', 'sc1')
SHIPPED = {'layer_fused_infer_kernelILb1ELb1E': {SC1_STORE: 40}, 'layer_fused_infer_kernelILb0ELb1E': {SC1_STORE: 40}}
# budgets of tests/test_fused_infer_unit_cpu.py and tests/test_attn_infer_unit_cpu.py
VGPRS = {'layer_fused_infer_kernel': 254, 'attn_fwd_row16_infer_kernel': 128}
MEMOP = re.compile(r'^\s+((?:global|flat|buffer|scratch)_\S+)\s+([^;\n]*)', re.M)


@pytest.fixture(scope='module')
def listings():
    with ThreadPoolExecutor(max_workers=len(UNITS)) as ex:
        asms = list(ex.map(lambda u: fused_isa.compile_asm(os.path.join(fused_isa.CSRC, u)), UNITS))
    out = {}
    for unit, asm in zip(UNITS, asms):
        meta = {m.group(1): m.group(2) for m in re.finditer(r'^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)\.end_amdhsa_kernel', asm, flags=re.S | re.M)}
        for m in re.finditer(r'^(_Z\w+):[^\n]*\n(.*?)s_endpgm', asm, flags=re.S | re.M):
            if m.group(1) not in meta:
                continue
            tally = {}
            for op, args in MEMOP.findall(m.group(2)):
                bits = ' '.join(w for w in args.split() if w in ('sc0', 'sc1', 'nt'))
                tally[(op, bits)] = tally.get((op, bits), 0) + 1
            g = lambda k, name=m.group(1): int(re.search(r'\.' + k + r'\s+(\d+)', meta[name]).group(1))          # noqa: E731
            out[(unit, m.group(1))] = dict(tally=tally, vgprs=g('amdhsa_next_free_vgpr'), scratch=g('amdhsa_private_segment_fixed_size'))
    return out


def shipped_for(name):
    hits = [v for k, v in SHIPPED.items() if k in name]
    assert len(hits) <= 1, name
    return hits[0] if hits else {}


def test_the_listings_hold_the_kernels_of_the_step(listings):
    names = [n for _, n in listings]
    assert sum('layer_fused_infer_kernel' in n for n in names) == 3
    assert sum('attn_fwd_row16_infer_kernel' in n for n in names) == 2
    assert sum('layer_fused_kernel' in n for n in names) >= 6           # the run-time kernels, bfloat16 and half units
    assert sum('attn_fwd_row16_kernel' in n for n in names) >= 2
    for key in SHIPPED:
        assert any(key in n for n in names), key
    # no flat access in a unit: its stores and loads are global ones, counted by vmcnt alone
    for (unit, name), k in listings.items():
        if 'infer_kernel' in name:
            assert not any(op.startswith('flat_') for op, _ in k['tally']), (unit, name)


def test_only_the_inference_units_carry_policy_bits_and_exactly_the_shipped_ones(listings):
    for (unit, name), k in listings.items():
        carried = {key: n for key, n in k['tally'].items() if key[1]}
        print(unit, name[:90], carried)
        assert carried == shipped_for(name), (unit, name)
        if 'infer_kernel' not in name:
            assert not carried, (unit, name)


def test_the_units_keep_their_register_budgets(listings):
    seen = 0
    for (unit, name), k in listings.items():
        for key, budget in VGPRS.items():
            if key in name:
                seen += 1
                assert k['scratch'] == 0 and k['vgprs'] <= budget, (name, k['vgprs'], k['scratch'])
    assert seen == 5
