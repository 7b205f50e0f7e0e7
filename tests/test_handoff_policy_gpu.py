"""The hand-offs between the launches of the inference step: every activation tensor is written by one launch and read by the next,
almost always on another XCD, and the per-token inference unit writes the stream, q and k | v through (sc1 stores, csrc/mem_policy.h)
instead of leaving the lines dirty in L2.  Whatever the policy, the bytes must be the ones the run-time kernels (plain stores) hand over.

The inference-unit route against the run-time kernels -- wmz_debug_fused_knobs(8) and wmz_debug_attn_knobs(0, 1) keep them where the
units would run -- bit for bit on the final stream and the logits, eagerly and through GraphedForward, whose replays reuse every
buffer: input A, then B, then A again, each against its own reference, so a consumer that read a stale line would show.

What this file guards is the DATA: the two routes agreed bit for bit before any store carried a policy, so a pass here does not show
that the written-through stores are what ran -- tests/test_handoff_policy_cpu.py shows that, from the ISA of the unit's kernels.

One clip of 9 x 16 x 16 (nine workgroups per launch: all eight XCDs, and the ninth wraps onto the first) and two clips of 4 x 16 x 16
with the last-frame cone on (trailing-planes launches); depth 2, dim 256, dim_head 128, mlp 256, bf16, extents (3, 3, 3) and (1, 1, 1)."""
import contextlib

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

D, I, M, C = 256, 128, 256, 64
SHAPES = {'one_clip_nine_planes': dict(data_shape=(9, 16, 16), B=1, cone=False),
          'two_clips_cone': dict(data_shape=(4, 16, 16), B=2, cone=True)}
EXTENTS = [(3, 3, 3), (1, 1, 1)]


@contextlib.contextmanager
def runtime_kernels(keep):
    from world_modelz_amd import _lib as L
    L.call('wmz_debug_fused_knobs', 8 if keep else 0)
    L.call('wmz_debug_attn_knobs', 0, 1 if keep else 0)
    try:
        yield
    finally:
        L.call('wmz_debug_fused_knobs', 0)
        L.call('wmz_debug_attn_knobs', 0, 0)


class StreamAndLogits(nn.Module):
    """The denoiser's inference forward with the final stream kept: [the stream the logits are taken from (every plane of the full
    grid; the last plane under the cone), the logits], flattened into one fp32 vector (exact: bf16 -> fp32)."""

    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, z):
        from world_modelz_amd import config, fused
        m = self.model
        if config.get_last_frame_cone():
            stream = last = fused.transformer_forward_last(m.transformer, z)
        else:
            stream = m.transformer.forward_compute(z)
            last = stream[:, -1]
        return torch.cat([stream.reshape(-1).float(), m._logits(last).reshape(-1)])


@pytest.fixture(scope='module', params=[(s, e) for s in SHAPES for e in EXTENTS], ids=lambda p: f'{p[0]}-{p[1][0]}{p[1][1]}{p[1][2]}')
def case(request):
    """The model, inputs A and B and their references from the run-time kernels: computed once, shared, left unchanged."""
    assert torch.cuda.is_available()
    from world_modelz_amd import config, fused
    from world_modelz_amd.main import VqVideoDiffusionModel
    shape, ext = request.param
    sh = SHAPES[shape]
    torch.manual_seed(17)
    m = VqVideoDiffusionModel(data_shape=sh['data_shape'], dim=D, num_classes=C, extents=ext, depth=2, dim_head=I, mlp_dim=M,
                              heads=1).cuda().eval()
    both = StreamAndLogits(m)
    g = torch.Generator(device='cuda').manual_seed(3)
    za, zb = (torch.randint(0, C + 1, (sh['B'],) + sh['data_shape'], device='cuda', generator=g) for _ in range(2))
    with config.compute_dtype(torch.bfloat16), config.last_frame_cone(sh['cone']), torch.no_grad():
        assert fused.inference_route(m.transformer, config.get_fused_dtype(), 16, 16, za.numel()) == 'fused'
        with runtime_kernels(True):
            ref_a, ref_b = both(za).clone(), both(zb).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(ref_a).all() and torch.isfinite(ref_b).all() and not torch.equal(ref_a, ref_b)
    return dict(both=both, cone=sh['cone'], za=za, zb=zb, ref_a=ref_a, ref_b=ref_b)


def test_eager_forward_matches_the_runtime_kernels_bit_for_bit(case):
    from world_modelz_amd import config
    with config.compute_dtype(torch.bfloat16), config.last_frame_cone(case['cone']), torch.no_grad(), runtime_kernels(False):
        for z, ref in ((case['za'], case['ref_a']), (case['zb'], case['ref_b']), (case['za'], case['ref_a'])):
            assert torch.equal(case['both'](z), ref)


def test_graph_replays_match_the_runtime_kernels_bit_for_bit(case):
    """A, B, A through one captured graph: every activation buffer of the step is reused by every replay."""
    from world_modelz_amd import config
    from world_modelz_amd.graph import GraphedForward
    with config.compute_dtype(torch.bfloat16), config.last_frame_cone(case['cone']), torch.no_grad(), runtime_kernels(False):
        run = GraphedForward(case['both'], case['za'])
        for z, ref in ((case['za'], case['ref_a']), (case['zb'], case['ref_b']), (case['za'], case['ref_a'])):
            assert torch.equal(run(z), ref)
        assert run.recaptures == 0
