"""The inference unit of the fused per-token kernel (csrc/layer_fused.hip: layer_fused_infer_kernel -- the kernel body with the
options of the plain full-grid inference launch compiled in) against the run-time kernel it replaces, bit for bit.

wmz_debug_fused_knobs(8) keeps the run-time kernel where the inference unit would run; every case runs once per route on the
same inputs.  The launches fused_launch must NOT hand to the inference unit (a ragged token count, 8-wide planes, the
last-frame cone, the precise mode) run the same way: both routes are then the run-time kernel, and the results are checked
against the oracle's as well."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import denoiser as oden          # noqa: E402

D, I, M = 256, 128, 256
KEEP_RUNTIME_KERNEL = 8
ORACLE_REL = 1e-2            # the bound the existing fused-path tests hold against the oracle (bf16 operands: measured 3-5e-3)


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@contextlib.contextmanager
def knobs(value):
    from world_modelz_amd import _lib as L
    L.call('wmz_debug_fused_knobs', value)
    try:
        yield
    finally:
        L.call('wmz_debug_fused_knobs', 0)


def both_routes(fn):
    """fn() -> tensors, once with the dispatch left alone and once with the run-time kernel forced."""
    with knobs(0):
        new = [t.clone() for t in fn()]
    with knobs(KEEP_RUNTIME_KERNEL):
        old = [t.clone() for t in fn()]
    torch.cuda.synchronize()
    return new, old


@pytest.fixture(scope='module')
def stack():
    """A depth-2 denoiser at the fused widths: layer streams for embedding + tail, head + tail and head only."""
    assert torch.cuda.is_available()
    from world_modelz_amd import fused
    from world_modelz_amd.main import VqVideoDiffusionModel
    torch.manual_seed(11)
    m = VqVideoDiffusionModel(data_shape=(3, 16, 16), dim=D, num_classes=64, extents=(1, 1, 1), depth=2, dim_head=I,
                              mlp_dim=M, heads=1).cuda().eval()
    layers = list(m.transformer.layers)
    packs = {'embed_tail': fused._layer_pack(None, layers[0]), 'head_tail': fused._layer_pack(layers[0], layers[1]),
             'head_only': fused._layer_pack(layers[1], None)}
    return dict(model=m, packs=packs)


def run_head(stack, kind, ntok, xflags, seed):
    """One wmz_layer_fused_fwd_planes launch on random rows; returns (x_out, q, kv) -- q / kv only with a tail -- each carved
    out of a larger canary-filled buffer, and checks that nothing was written behind them."""
    from world_modelz_amd import _lib as L
    bf, canary = torch.bfloat16, 12345.0
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randn(ntok * D, device='cuda', generator=g).to(bf)
    o = torch.randn(ntok * I, device='cuda', generator=g).to(bf)
    tail = kind == 'head_tail'
    wpack, vec = stack['packs'][kind]

    def run():
        bufs = {k: torch.full((n + 4096,), canary, dtype=bf, device='cuda')
                for k, n in (('xo', ntok * D), ('q', ntok * I), ('kv', 2 * ntok * I))}
        L.call('wmz_layer_fused_fwd_planes', L.ptr(o), L.ptr(x), L.ptr(bufs['xo']), L.ptr(bufs['q']) if tail else None,
               L.ptr(bufs['kv']) if tail else None, L.ptr(wpack), L.ptr(vec), 1, 1, 1, ntok, D, I, M, 1, 1 if tail else 0,
               xflags, 1e-5, L.stream())
        torch.cuda.synchronize()
        sizes = {'xo': ntok * D, 'q': ntok * I if tail else 0, 'kv': 2 * ntok * I if tail else 0}
        for k, n in sizes.items():
            assert (bufs[k][n:] == canary).all(), f'{kind}: {k} written past its end (ntok={ntok}, xflags={xflags})'
            assert torch.isfinite(bufs[k][:n].float()).all(), k
        return [bufs[k][:n] for k, n in sizes.items() if n]
    return both_routes(run)


@pytest.mark.parametrize('ntok', [256, 768])
@pytest.mark.parametrize('kind,xflags', [('head_tail', 3), ('head_only', 1)])
def test_head_launches_match_the_runtime_kernel_bit_for_bit(stack, kind, xflags, ntok):
    """head + tail (stream tiled in and out) and head only (tiled in, row-major out: the last layer) at one workgroup and at
    three."""
    new, old = run_head(stack, kind, ntok, xflags, seed=ntok + xflags)
    assert len(new) == (3 if kind == 'head_tail' else 1)
    for a, b in zip(new, old):
        assert torch.equal(a, b)


def run_embed(stack, B, S, H, W, xflags):
    from world_modelz_amd import _lib as L
    tr = stack['model'].transformer
    bf = torch.bfloat16
    ntok = B * S * H * W
    g = torch.Generator(device='cuda').manual_seed(ntok)
    z = torch.randint(0, tr.embedding.num_embeddings, (B, S, H, W), device='cuda', generator=g)
    wpack, vec = stack['packs']['embed_tail']

    def run():
        x = torch.zeros(ntok * D, dtype=bf, device='cuda')
        q = torch.zeros(ntok * I, dtype=bf, device='cuda')
        kv = torch.zeros(2 * ntok * I, dtype=bf, device='cuda')
        L.call('wmz_embed_qkv_fused_fwd_planes', L.ptr(z), L.ptr(tr.embedding.weight.detach()),
               L.ptr(tr.pos_emb_s.weight.detach()), L.ptr(tr.pos_emb_h.weight.detach()), L.ptr(tr.pos_emb_w.weight.detach()),
               L.ptr(x), L.ptr(q), L.ptr(kv), L.ptr(wpack), L.ptr(vec), B, S, H, W, S, D, I, M,
               tr.embedding.num_embeddings, xflags, 1e-5, L.stream())
        return [x, q, kv]
    return both_routes(run)


@pytest.mark.parametrize('S', [1, 3])
def test_embedding_launch_matches_the_runtime_kernel_bit_for_bit(stack, S):
    """embedding + tail on 16 x 16 planes, x_out tiled: 256 tokens (one workgroup) and 768."""
    new, old = run_embed(stack, 1, S, 16, 16, 2)
    for a, b in zip(new, old):
        assert torch.equal(a, b)
    assert float(new[0].float().abs().max()) > 0


def test_launches_outside_the_unit_fall_back(stack):
    """288 tokens (a ragged last workgroup), tiled and row-major, and a row-major stream at a whole count: the run-time kernel on
    both routes -- equal results, nothing written past the end (run_head's canaries)."""
    for kind, ntok, xflags in (('head_tail', 288, 3), ('head_tail', 288, 0), ('head_only', 288, 1), ('head_tail', 256, 0),
                               ('head_only', 256, 0)):
        new, old = run_head(stack, kind, ntok, xflags, seed=7)
        for a, b in zip(new, old):
            assert torch.equal(a, b), (kind, ntok, xflags)


def model_logits(data_shape, B, seed, dtype=torch.bfloat16, cone=False):
    from world_modelz_amd import config
    from world_modelz_amd.main import VqVideoDiffusionModel
    torch.manual_seed(seed)
    C = 64
    m = VqVideoDiffusionModel(data_shape=data_shape, dim=D, num_classes=C, extents=(1, 1, 1), depth=2, dim_head=I, mlp_dim=M,
                              heads=1)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    z = torch.randint(0, C + 1, (B,) + tuple(data_shape))
    ref = oden.denoiser_forward(sd, z, (1, 1, 1), 1)
    m = m.cuda().eval()
    zc = z.cuda()

    def run():
        with config.compute_dtype(dtype), config.last_frame_cone(cone), torch.no_grad():
            return [m(zc)]
    (new,), (old,) = both_routes(run)
    return new, old, ref


def test_whole_forward_matches_between_the_routes_and_the_oracle():
    """VqVideoDiffusionModel.forward, B = 1, 3 x 16 x 16, depth 2, full grid: embedding + tail, head + tail and head only all
    take the inference unit; logits equal to the run-time kernels' and within the oracle bound."""
    new, old, ref = model_logits((3, 16, 16), 1, seed=5)
    assert torch.equal(new, old)
    assert rel(new, ref) < ORACLE_REL


def test_eight_wide_planes_keep_the_runtime_embedding():
    """4 x 8 x 8 = 256 tokens: the embedding launch is not the unit's (8-wide planes), the head launches are."""
    new, old, ref = model_logits((4, 8, 8), 1, seed=6)
    assert torch.equal(new, old)
    assert rel(new, ref) < ORACLE_REL


def test_cone_and_precise_mode_keep_the_runtime_kernels():
    """The last-frame cone (trailing planes: re-mapped rows) and the precise mode (the half unit has no inference unit)."""
    full, _, ref = model_logits((3, 16, 16), 1, seed=5)
    new, old, _ = model_logits((3, 16, 16), 1, seed=5, cone=True)
    assert torch.equal(new, old) and torch.equal(new, full)
    new, old, ref = model_logits((3, 16, 16), 1, seed=5, dtype=torch.float16)
    assert torch.equal(new, old)
    assert rel(new, ref) < 1e-3          # (the precise mode's own bound: bench.py's gate for it)
