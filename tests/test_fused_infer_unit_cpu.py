"""The inference unit of the fused per-token kernel, read from its ISA (csrc/layer_fused.hip compiled for gfx950, no GPU needed):
what the compile-time option policy is there to remove is gone.  Counting: tools/fused_infer_isa.py."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('fused_infer_isa', os.path.join(ROOT, 'tools', 'fused_infer_isa.py'))
isa = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa)

pytestmark = pytest.mark.skipif(isa.hipcc() is None, reason='hipcc not available')

# Conditional branches a kernel of the unit may hold, from its source:
#   the feed-forward chunk loop's back edge (head kernels)                                                  1
#   head only writes the stream row-major: store_tile256 stages one lane half per pass, two passes          2
#   embedding: embed_coop's two plane-row passes each end in a lane-divergent pick-up, and the token
#   class is clamped to the table (a divergent range test)                                                  3
BRANCHES = {(True, True): 1, (True, False): 1 + 2, (False, True): 3}


@pytest.fixture(scope='module')
def listing():
    asm = isa.compile_asm(os.path.join(isa.CSRC, 'layer_fused.hip'))
    return asm, isa.kernels(asm)


def test_the_unit_has_its_three_kernels_beside_the_runtime_ones(listing):
    _, ks = listing
    assert sorted(ks) == sorted([(u, h, t) for u in ('infer', 'runtime') for (h, t) in BRANCHES])


@pytest.mark.parametrize('head,tail', sorted(BRANCHES))
def test_inference_kernel_budgets(listing, head, tail):
    """scratch 0, at most 254 VGPRs, no conditional branch beyond the chunk loop and the embedding path, and fewer than HALF the
    scalar instructions of the run-time kernel of the same build (head + tail, parent commit: 2 678 scalar, 582 branches)."""
    _, ks = listing
    new, old = ks[('infer', head, tail)], ks[('runtime', head, tail)]
    print(isa.KINDS[(head, tail)], 'infer', new['whole'], 'vgprs', new['vgprs'], '| runtime', old['whole'], 'vgprs', old['vgprs'])
    assert new['scratch'] == 0
    assert new['vgprs'] <= 254
    assert new['whole']['cbranch'] <= BRANCHES[(head, tail)], new['whole']
    assert 2 * new['whole']['scalar'] < old['whole']['scalar'], (new['whole']['scalar'], old['whole']['scalar'])
    assert new['whole']['mfma'] > 0
    if head:
        assert new['loop'] is not None and new['loop']['cbranch'] == 1, new['loop']


def test_every_counted_wait_of_the_unit_is_a_literal(listing):
    """The inference kernels hold no jump table and no compare-and-branch ladder in front of an s_waitcnt: between a kernel's
    first and last barrier every s_waitcnt vmcnt sits in straight-line code (its only branch is the chunk loop's back edge),
    and the weight ring's waits are followed by the slab barrier."""
    asm, ks = listing
    for (unit, head, tail), k in ks.items():
        if unit != 'infer':
            continue
        body = re.search(re.escape(k['name']) + r':[^\n]*\n(.*?)s_endpgm', asm, flags=re.S).group(1).split('\n')
        ops = [l.split() for l in body if re.match(r'\s+[a-z]', l)]
        bars = [i for i, o in enumerate(ops) if o[0] == 's_barrier']
        assert len(bars) >= 6, (head, tail, len(bars))
        inner = ops[bars[0]:bars[-1] + 1]
        assert sum(o[0].startswith('s_cbranch') for o in inner) == (1 if head else 0), (head, tail)
        assert not any(o[0] in ('s_setpc_b64', 's_swappc_b64', 's_getpc_b64') for o in ops), (head, tail)
        # every slab barrier is directly behind its counted wait
        for i in bars[1:]:
            prev = [o for o in ops[max(0, i - 3):i] if o[0] == 's_waitcnt' and o[1].startswith('vmcnt(')]
            assert prev, (head, tail, ops[max(0, i - 3):i + 1])
