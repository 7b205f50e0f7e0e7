"""The inference unit of the row16 attention forward (csrc/attn_fwd_row16_infer.hip), read from its ISA beside the run-time kernel's
headline instantiation (csrc/attn_fwd_row16.hip), both compiled for gfx950 -- no GPU needed.  Counting: tools/attn_infer_isa.py."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('attn_infer_isa', os.path.join(ROOT, 'tools', 'attn_infer_isa.py'))
isa = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa)

pytestmark = pytest.mark.skipif(isa.hipcc() is None, reason='hipcc not available')

EXTENTS = [(3, 3), (1, 1)]          # (eH, eW): the headline window and the 7x3x3 one


@pytest.fixture(scope='module')
def listing():
    rt_asm = isa.compile_asm(os.path.join(isa.CSRC, 'attn_fwd_row16.hip'))
    inf_asm = isa.compile_asm(os.path.join(isa.CSRC, 'attn_fwd_row16_infer.hip'))
    return inf_asm, isa.kernels(rt_asm, isa.RUNTIME), isa.kernels(inf_asm, isa.INFER)


def test_the_unit_has_exactly_its_two_kernels(listing):
    inf_asm, rt, inf = listing
    assert len(rt) == 1                                  # the tool's pattern names one run-time instantiation: the headline's
    assert sorted(inf) == sorted(EXTENTS)
    assert len(re.findall(r'^\s*\.amdhsa_kernel\s', inf_asm, flags=re.M)) == 2


@pytest.mark.parametrize('ext', EXTENTS)
def test_inference_kernel_budgets(listing, ext):
    """No scratch, at most 128 VGPRs (16 waves a CU), fewer than HALF the scalar instructions of the run-time kernel -- in the whole
    kernel, which holds two slabs written out against the run-time kernel's one, and per slab iteration -- and no more conditional
    branches than it."""
    _, rt, inf = listing
    old, new = next(iter(rt.values())), inf[ext]
    assert old['loop'] is not None and new['loop'] is not None
    slab_new, slab_old = isa.per_slab(new['loop'], 2), old['loop']
    print(f'infer {ext}: whole {new["whole"]} slab {slab_new} vgprs {new["vgprs"]} scratch {new["scratch"]}')
    print(f'runtime: whole {old["whole"]} slab {slab_old} vgprs {old["vgprs"]} scratch {old["scratch"]}')
    print(f'conditional branches: infer {ext} {new["whole"]["cbranch"]}, runtime {old["whole"]["cbranch"]}')
    assert new['scratch'] == 0
    assert new['vgprs'] <= 128
    assert new['whole']['mfma'] > 0 and new['loop']['mfma'] == 2 * slab_new['mfma']
    assert 2 * new['whole']['scalar'] < old['whole']['scalar'], (new['whole']['scalar'], old['whole']['scalar'])
    assert 2 * slab_new['scalar'] < slab_old['scalar'], (slab_new['scalar'], slab_old['scalar'])
    assert new['whole']['cbranch'] <= old['whole']['cbranch'], (new['whole']['cbranch'], old['whole']['cbranch'])
