"""The context cache on the GPU: the _slots per-token launches against the trailing-planes launches they extend, the
cached forward of the causal denoiser against the uncached one bit for bit and against tests/causal_ref.py at the mode's bar, and
the sampler with the cache against the sampler without it, token for token.

                          kernel (_slots vs _planes)       model (forward_last vs forward)        sampler
  bf16                    bit-identical, sentinel intact    torch.equal; 1e-2 of the reference     same tokens
  precise (half)          bit-identical, sentinel intact    torch.equal; 1e-3 of the reference     same tokens, half guard 'raise'
"""
import contextlib

import pytest
import torch

import causal_ref
import route_table as rt
from conftest import recorded_calls

pytestmark = pytest.mark.gpu

BF, HALF = torch.bfloat16, torch.float16
D_, I_, M_ = 256, 128, 256
C = 48
FUSED, OPS = (256, 1, 128, 256), (160, 1, 128, 256)          # dim, heads, dim_head, mlp_dim
TOL = {'bf16': 1e-2, 'precise': 1e-3}                         # test_route_matrix_gpu.py
SENTINEL = 0x5A3C                                             # an int16 pattern no launch below is asked to write everywhere
GUARD = 4096                                                  # elements behind each slot buffer


@pytest.fixture(scope='module')
def wmz():
    assert torch.cuda.is_available()
    from world_modelz_amd import _lib, config, fused, main, sample
    return dict(lib=_lib, config=config, fused=fused, main=main, sample=sample)


def denoiser(wmz, widths, clip, seed, causal=True, depth=3, ext=(1, 1, 1)):
    dim, heads, dh, mlp = widths
    torch.manual_seed(seed)
    return wmz['main'].VqVideoDiffusionModel(data_shape=clip, dim=dim, num_classes=C, extents=ext, depth=depth, dim_head=dh,
                                             mlp_dim=mlp, heads=heads, causal=causal)


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def slots_entry(base, dtype):
    """base_slots, or for half the slots form of the _f16 entry point."""
    return base + ('_f16_slots' if dtype == HALF else '_slots')


def bits(t):
    return t.contiguous().view(torch.int16)


# ----------------------------------------------------------------------------------------------------------------------- kernel

SLOTS = [(1, 1, 0), (1, 3, 2), (1, 3, 0), (2, 3, 0)]           # planes_out, dst_planes, dst_plane0 (slot 0: no hard-wired last slot)
PLANES = [(16, 16), (5, 16), (4, 32)]                          # tiled + cooperative embedding | 80 rows: ragged, row-major | 32 wide


@pytest.fixture(scope='module')
def stack(wmz):
    """Two layers' parameters to pack weight streams from (any values do: both launches of a comparison read the same stream)."""
    return denoiser(wmz, FUSED, (4, 16, 32), seed=5, depth=2).cuda().transformer


def sentinel(n, dtype):
    return torch.full((n + GUARD,), SENTINEL, dtype=torch.int16, device='cuda').view(dtype)


def check_slots(buf, ref, B, dp, d0, po, HW, halves):
    """buf: `halves` x [B, dp, HW, I] + guard, all sentinel before the launch; ref [halves, B, po, HW, I]: the named slots hold
    ref's bits, every other element still the sentinel."""
    n = halves * B * dp * HW * I_
    got = bits(buf)[:n].view(halves, B, dp, HW, I_)
    assert torch.equal(got[:, :, d0:d0 + po], bits(ref).view(halves, B, po, HW, I_)), 'the named slots do not hold the rows'
    rest = got.clone()
    rest[:, :, d0:d0 + po] = SENTINEL
    assert bool((rest == SENTINEL).all()), 'a byte outside the named slots was written'
    assert bool((bits(buf)[n:] == SENTINEL).all()), 'the guard band behind the buffer was written'


@pytest.mark.parametrize('dtype', [BF, HALF], ids=['bf16', 'f16'])
@pytest.mark.parametrize('plane', PLANES, ids=lambda p: 'x'.join(map(str, p)))
def test_slots_launches_are_the_planes_launches_in_place(wmz, stack, plane, dtype):
    L, fused = wmz['lib'], wmz['fused']
    H, W = plane
    HW, B = H * W, 2
    tiled = HW % 32 == 0
    layers = list(stack.layers)
    emb = [t.weight.detach() for t in (stack.embedding, stack.pos_emb_s, stack.pos_emb_h, stack.pos_emb_w)]
    torch.manual_seed(HW)
    for po, dp, d0 in SLOTS:
        pi = po + 1                                                   # one more input plane: the source map is live too
        # ---- head + tail
        wpack, vec = fused._layer_pack(layers[0], layers[1], dtype)
        o = torch.randn(B, po, HW, I_, device='cuda').to(dtype)
        x = torch.randn(B, pi, HW, D_, device='cuda').to(dtype)
        xflags = (fused.X_IN_TILED | fused.X_OUT_TILED) if tiled else 0
        x_ref, q_ref = torch.empty(B, po, HW, D_, dtype=dtype, device='cuda'), torch.empty(B, po, HW, I_, dtype=dtype, device='cuda')
        kv_ref = torch.empty(2, B, po, HW, I_, dtype=dtype, device='cuda')
        L.call(L.half_form('wmz_layer_fused_fwd_planes', dtype), L.ptr(o), L.ptr(x), L.ptr(x_ref), L.ptr(q_ref), L.ptr(kv_ref), L.ptr(wpack),
               L.ptr(vec), B, po, pi, HW, D_, I_, M_, 1, 1, xflags, 1e-5, L.stream())
        x_out = sentinel(B * po * HW * D_, dtype)
        q, kv = sentinel(B * dp * HW * I_, dtype), sentinel(2 * B * dp * HW * I_, dtype)
        L.call(slots_entry('wmz_layer_fused_fwd', dtype), L.ptr(o), L.ptr(x), L.ptr(x_out), L.ptr(q), L.ptr(kv), L.ptr(wpack),
               L.ptr(vec), B, po, pi, HW, D_, I_, M_, 1, 1, xflags, 1e-5, dp, d0, L.stream())
        n = B * po * HW * D_
        assert torch.equal(bits(x_out)[:n], bits(x_ref).view(-1)) and bool((bits(x_out)[n:] == SENTINEL).all()), (po, dp, d0)
        check_slots(q, q_ref[None], B, dp, d0, po, HW, 1)
        check_slots(kv, kv_ref, B, dp, d0, po, HW, 2)
        # ---- embedding + tail
        wpack, vec = fused._layer_pack(None, layers[0], dtype)
        S = pi
        z = torch.randint(0, C + 1, (B, S, H, W), device='cuda')
        eflags = fused.X_OUT_TILED if tiled else 0
        L.call(L.half_form('wmz_embed_qkv_fused_fwd_planes', dtype), L.ptr(z), *map(L.ptr, emb), L.ptr(x_ref), L.ptr(q_ref), L.ptr(kv_ref),
               L.ptr(wpack), L.ptr(vec), B, S, H, W, po, D_, I_, M_, C + 1, eflags, 1e-5, L.stream())
        x_out = sentinel(n, dtype)
        q, kv = sentinel(B * dp * HW * I_, dtype), sentinel(2 * B * dp * HW * I_, dtype)
        L.call(slots_entry('wmz_embed_qkv_fused_fwd', dtype), L.ptr(z), *map(L.ptr, emb), L.ptr(x_out), L.ptr(q), L.ptr(kv),
               L.ptr(wpack), L.ptr(vec), B, S, H, W, po, D_, I_, M_, C + 1, eflags, 1e-5, dp, d0, L.stream())
        assert torch.equal(bits(x_out)[:n], bits(x_ref).view(-1)) and bool((bits(x_out)[n:] == SENTINEL).all()), (po, dp, d0)
        check_slots(q, q_ref[None], B, dp, d0, po, HW, 1)
        check_slots(kv, kv_ref, B, dp, d0, po, HW, 2)


@pytest.mark.parametrize('dtype', [BF, HALF], ids=['bf16', 'f16'])
def test_slots_refusals(wmz, stack, dtype):
    """dst_plane0 < 0 and dst_plane0 + planes_out > dst_planes are refused before anything is launched."""
    L, fused = wmz['lib'], wmz['fused']
    layers = list(stack.layers)
    B, H, W = 1, 2, 16
    HW = H * W
    emb = [t.weight.detach() for t in (stack.embedding, stack.pos_emb_s, stack.pos_emb_h, stack.pos_emb_w)]
    o, x = torch.zeros(B, 2, HW, I_, device='cuda', dtype=dtype), torch.zeros(B, 2, HW, D_, device='cuda', dtype=dtype)   # (room for two planes)
    z = torch.zeros(B, 2, H, W, dtype=torch.int64, device='cuda')
    x_out = sentinel(B * 2 * HW * D_, dtype)
    q, kv = sentinel(B * 3 * HW * I_, dtype), sentinel(2 * B * 3 * HW * I_, dtype)
    for po, dp, d0 in ((1, 3, -1), (1, 3, 3), (2, 3, 2), (1, 0, 0)):
        wpack, vec = fused._layer_pack(layers[0], layers[1], dtype)
        with pytest.raises(L.WmzError, match='must lie inside the dst_planes slots'):
            L.call(slots_entry('wmz_layer_fused_fwd', dtype), L.ptr(o), L.ptr(x), L.ptr(x_out), L.ptr(q), L.ptr(kv), L.ptr(wpack),
                   L.ptr(vec), B, po, po, HW, D_, I_, M_, 1, 1, 0, 1e-5, dp, d0, L.stream())
        wpack, vec = fused._layer_pack(None, layers[0], dtype)
        with pytest.raises(L.WmzError, match='must lie inside the dst_planes slots'):
            L.call(slots_entry('wmz_embed_qkv_fused_fwd', dtype), L.ptr(z), *map(L.ptr, emb), L.ptr(x_out), L.ptr(q), L.ptr(kv),
                   L.ptr(wpack), L.ptr(vec), B, 2, H, W, po, D_, I_, M_, C + 1, 0, 1e-5, dp, d0, L.stream())
    torch.cuda.synchronize()
    for buf in (x_out, q, kv):
        assert bool((bits(buf) == SENTINEL).all())


@contextlib.contextmanager
def slots_waves(L, waves):
    """The context cache's per-token launches on the `waves`-per-workgroup build for the block (wmz_debug_fused_slots_waves)."""
    L.call('wmz_debug_fused_slots_waves', waves)
    try:
        yield
    finally:
        L.call('wmz_debug_fused_slots_waves', 0)


@pytest.mark.parametrize('dtype', [BF, HALF], ids=['bf16', 'f16'])
@pytest.mark.parametrize('plane', PLANES, ids=lambda p: 'x'.join(map(str, p)))
def test_small_workgroup_form_is_bit_identical(wmz, stack, plane, dtype):
    """The 4-wave build of the _slots kernels (128 tokens per workgroup) against the 8-wave one: per-token arithmetic does not
    depend on the workgroup size, so every byte of x_out and of the slot buffers -- sentinel and guard band included -- is equal."""
    L, fused = wmz['lib'], wmz['fused']
    H, W = plane
    HW, B = H * W, 2
    tiled = HW % 32 == 0
    layers = list(stack.layers)
    emb = [t.weight.detach() for t in (stack.embedding, stack.pos_emb_s, stack.pos_emb_h, stack.pos_emb_w)]
    torch.manual_seed(HW + 1)
    with pytest.raises(L.WmzError):
        L.call('wmz_debug_fused_slots_waves', 2)
    for po, dp, d0 in SLOTS:
        pi = po + 1
        o = torch.randn(B, po, HW, I_, device='cuda').to(dtype)
        x = torch.randn(B, pi, HW, D_, device='cuda').to(dtype)
        z = torch.randint(0, C + 1, (B, pi, H, W), device='cuda')
        got = {}
        for waves in (8, 4):
            bufs = []
            with slots_waves(L, waves):
                wpack, vec = fused._layer_pack(layers[0], layers[1], dtype)
                x_out = sentinel(B * po * HW * D_, dtype)
                q, kv = sentinel(B * dp * HW * I_, dtype), sentinel(2 * B * dp * HW * I_, dtype)
                L.call(slots_entry('wmz_layer_fused_fwd', dtype), L.ptr(o), L.ptr(x), L.ptr(x_out), L.ptr(q), L.ptr(kv), L.ptr(wpack),
                       L.ptr(vec), B, po, pi, HW, D_, I_, M_, 1, 1, (fused.X_IN_TILED | fused.X_OUT_TILED) if tiled else 0, 1e-5, dp, d0,
                       L.stream())
                bufs += [x_out, q, kv]
                wpack, vec = fused._layer_pack(None, layers[0], dtype)
                x_out = sentinel(B * po * HW * D_, dtype)
                q, kv = sentinel(B * dp * HW * I_, dtype), sentinel(2 * B * dp * HW * I_, dtype)
                L.call(slots_entry('wmz_embed_qkv_fused_fwd', dtype), L.ptr(z), *map(L.ptr, emb), L.ptr(x_out), L.ptr(q), L.ptr(kv),
                       L.ptr(wpack), L.ptr(vec), B, pi, H, W, po, D_, I_, M_, C + 1, fused.X_OUT_TILED if tiled else 0, 1e-5, dp, d0,
                       L.stream())
                bufs += [x_out, q, kv]
            got[waves] = bufs
        for a, b in zip(got[8], got[4]):
            assert torch.equal(bits(a), bits(b)), (po, dp, d0)
        assert not bool((bits(got[4][1]) == SENTINEL).all())                    # (the small form did write)


# ------------------------------------------------------------------------------------------------------------------------ model

# clip (S, H, W), time extent, depth
MODEL_CASES = [
    pytest.param((4, 16, 16), 1, 3, id='4x16x16-eS1'),
    pytest.param((4, 16, 16), 2, 3, id='4x16x16-eS2'),               # S = eS + 2
    pytest.param((2, 16, 16), 3, 3, id='2x16x16-eS3'),               # the window reaches over the clip
    pytest.param((1, 16, 16), 1, 3, id='1x16x16-no-context'),
    pytest.param((3, 4, 32), 1, 3, id='3x4x32'),
    pytest.param((3, 5, 16), 1, 3, id='3x5x16'),
    pytest.param((3, 16, 16), 1, 1, id='3x16x16-depth1'),
]
_references = {}


def reference(wmz, clip, eS, depth):
    """(state dict, tokens, the causal reference's logits) of a case: computed once on the CPU, shared by both modes, left alone."""
    key = (clip, eS, depth)
    if key not in _references:
        m = denoiser(wmz, FUSED, clip, seed=17 + clip[0] + eS, depth=depth, ext=(eS, 1, 1))
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        z = torch.randint(0, C + 1, (2,) + clip)
        _references[key] = (sd, z, causal_ref.denoiser_forward(sd, z, (eS, 1, 1), FUSED[1]))
    return _references[key]


@pytest.mark.parametrize('mode', ['bf16', 'precise'])
@pytest.mark.parametrize('clip,eS,depth', MODEL_CASES)
def test_cached_forward_is_the_forward(wmz, clip, eS, depth, mode):
    cfg, fused = wmz['config'], wmz['fused']
    sd, z, ref = reference(wmz, clip, eS, depth)
    m = denoiser(wmz, FUSED, clip, seed=0, depth=depth, ext=(eS, 1, 1))
    m.load_state_dict(sd)
    m = m.cuda()
    z = z.cuda()
    S = clip[0]
    sfx = '_f16_slots' if mode == 'precise' else '_slots'
    with cfg.compute_dtype(rt.MODES[mode]), torch.no_grad():
        assert m.context_cache_eligible(z)
        y = m(z)
        cache = m.context_prefill(z)
        assert cache.a == fused.context_planes(S, eS, depth) and [t.shape[1] for t in cache.q] == [n + 1 for n in cache.a]
        addresses = [t.data_ptr() for t in cache.q + cache.kv]
        with recorded_calls() as seen:
            yc = m.forward_last(z, cache)
        assert yc.dtype == torch.float32 and yc.shape == (2,) + clip[1:] + (C,)
        assert torch.equal(yc, y), 'the cached forward is not the forward'
        # a decode step: depth attention launches, depth + 1 per-token launches, one plane each, on the cache's entry points
        assert seen.count('wmz_local3d_attn_fwd_window') == depth, seen
        per_token = [n for n in seen if rt.is_fused_or_chain(n)]
        assert per_token == ['wmz_embed_qkv_fused_fwd' + sfx] + ['wmz_layer_fused_fwd' + sfx] * depth, seen
        assert not [n for n in seen if 'attn' in n and n != 'wmz_local3d_attn_fwd_window'], seen
        # the point of the feature: another last frame on the SAME cache
        z2 = z.clone()
        z2[:, -1] = (z2[:, -1] + 7) % (C + 1)
        y2 = m(z2)
        assert not torch.equal(y2, y)
        assert torch.equal(m.forward_last(z2, cache), y2), 'a new last frame on the kept context is not the forward'
        assert [t.data_ptr() for t in cache.q + cache.kv] == addresses
        if S > 1:
            # ... and the cache is what is read: a changed context token without a refill gives the OLD context's answer
            z3 = z2.clone()
            z3[:, -2] = (z3[:, -2] + 5) % (C + 1)
            y3 = m(z3)
            stale = m.forward_last(z3, cache)
            assert not torch.equal(stale, y3) and torch.equal(stale, y2)
            assert m.context_prefill(z3, cache) is cache                          # refilled in place
            assert [t.data_ptr() for t in cache.q + cache.kv] == addresses
            assert torch.equal(m.forward_last(z3, cache), y3)
    e = rel(yc, ref)
    print(f'[context cache {clip} eS {eS} depth {depth} {mode}] logits rel {e:.2e} (bar {TOL[mode]:.0e})')
    assert e < TOL[mode], (mode, e)


@pytest.mark.parametrize('mode', ['bf16', 'precise'])
@pytest.mark.parametrize('clip', [(4, 16, 16), (3, 5, 16)], ids=lambda c: 'x'.join(map(str, c)))
def test_cached_forward_on_either_workgroup_form(wmz, clip, mode):
    """The whole cached forward with its per-token launches forced to the 4-wave build, to the 8-wave build, and under the entry
    points' own rule (4 waves at these sizes): the forward, bit for bit, every time."""
    cfg, L = wmz['config'], wmz['lib']
    m = denoiser(wmz, FUSED, clip, seed=23, depth=3).cuda()
    z = torch.randint(0, C + 1, (2,) + clip).cuda()
    with cfg.compute_dtype(rt.MODES[mode]), torch.no_grad():
        y = m(z)
        for waves in (4, 8):
            with slots_waves(L, waves):
                assert torch.equal(m.forward_last(z, m.context_prefill(z)), y), waves
        assert torch.equal(m.forward_last(z, m.context_prefill(z)), y)


def test_who_may_keep_a_cache(wmz):
    cfg = wmz['config']
    clip = (3, 16, 16)
    z = torch.randint(0, C + 1, (1,) + clip).cuda()
    m = denoiser(wmz, FUSED, clip, seed=3, depth=2).cuda()
    sym = denoiser(wmz, FUSED, clip, seed=3, depth=2, causal=False).cuda()
    other = denoiser(wmz, OPS, clip, seed=3, depth=2).cuda()
    with cfg.compute_dtype(BF), torch.no_grad():
        cache = m.context_prefill(z)
        for bad in (sym, other):
            assert not bad.context_cache_eligible(z)
            with pytest.raises(ValueError):
                bad.context_prefill(z)
            with pytest.raises(ValueError):
                bad.forward_last(z, cache)
        with pytest.raises(ValueError):                                           # another geometry than the cache's
            m.forward_last(z[:, 1:].contiguous(), cache)
    with cfg.compute_dtype(BF):                                                   # with grad
        assert not m.context_cache_eligible(z)
        with pytest.raises(ValueError):
            m.context_prefill(z)
    with cfg.compute_dtype(torch.float32), torch.no_grad():                       # fp32: op by op
        assert not m.context_cache_eligible(z)
        with pytest.raises(ValueError):
            m.forward_last(z, cache)
    with cfg.compute_dtype(BF), torch.no_grad():
        assert not m.context_cache_eligible(z.cpu())


# ---------------------------------------------------------------------------------------------------------------------- sampler

CLIP = (3, 16, 16)
KW = dict(num_frames=2, num_eval_iterations=3, sample_topk=5)


def draw(wmz, m, z, cache, seed=1, **kw):
    frames, zf = wmz['sample'].sample_frames(m, z, C, generator=torch.Generator().manual_seed(seed), context_cache=cache, **KW, **kw)
    return frames + [zf]


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope='module')
def causal_model(wmz):
    return denoiser(wmz, FUSED, CLIP, seed=71, depth=2).cuda()


@pytest.mark.parametrize('kw', [dict(), dict(consistent_masking=True), dict(remask='confidence')],
                         ids=['plain', 'consistent-masking', 'confidence'])
def test_captured_sampler_same_tokens(wmz, causal_model, kw):
    m = causal_model
    z = torch.randint(0, C, (1,) + CLIP).cuda()
    with wmz['config'].compute_dtype(BF), torch.no_grad():
        plain = draw(wmz, m, z, False, **kw)
        with recorded_calls() as seen:
            cached = draw(wmz, m, z, True, **kw)
        assert same(cached, plain)
        if not kw:
            # a second call replays the session's graphs (no capture: nothing is launched outside them but the frame's first draw)
            sessions = m._wmz_sampler_sessions
            ses = [s for s in sessions.values() if s.prefill is not None]
            assert len(ses) == 1 and ses[0].fwd.static_in is ses[0].prefill.static_in
            captures = (ses[0].fwd.recaptures, ses[0].prefill.recaptures)
            with recorded_calls() as again_seen:
                again = draw(wmz, m, z, True)
            assert same(again, plain) and (ses[0].fwd.recaptures, ses[0].prefill.recaptures) == captures
            assert not [n for n in again_seen if rt.is_fused_or_chain(n) or 'attn' in n], again_seen
            assert same(draw(wmz, m, z, True, seed=2), draw(wmz, m, z, False, seed=2))
            assert not same(draw(wmz, m, z, True, seed=2), plain)
            assert 'wmz_layer_fused_fwd_slots' in seen and 'wmz_embed_qkv_fused_fwd_slots' in seen       # (the capture's launches)


def test_sampler_recaptures_after_a_weight_update(wmz):
    m = denoiser(wmz, FUSED, CLIP, seed=72, depth=2).cuda()
    z = torch.randint(0, C, (1,) + CLIP).cuda()
    with wmz['config'].compute_dtype(BF), torch.no_grad():
        before = draw(wmz, m, z, True)
        assert same(before, draw(wmz, m, z, False))
        ses = [s for s in m._wmz_sampler_sessions.values() if s.prefill is not None][0]
        for p in (m.transformer.layers[0][0].fn.to_k.weight, m.transformer.embedding.weight):
            p.add_(0.05 * torch.randn_like(p))
        after = draw(wmz, m, z, True)
        assert ses.fwd.recaptures == 1 and ses.prefill.recaptures == 1
        assert same(after, draw(wmz, m, z, False)) and not same(after, before)


def test_injected_uniforms_loop_same_tokens(wmz, causal_model):
    m = causal_model
    z = torch.randint(0, C, (1,) + CLIP).cuda()
    HW = CLIP[1] * CLIP[2]
    g = torch.Generator().manual_seed(9)
    uniforms = (torch.rand(2, 3, HW, generator=g), torch.rand(2, 3, 1, HW, generator=g))
    with wmz['config'].compute_dtype(BF), torch.no_grad():
        plain = draw(wmz, m, z, False, uniforms=uniforms)
        with recorded_calls() as seen:
            cached = draw(wmz, m, z, True, uniforms=uniforms)
        eager = draw(wmz, m, z, True, uniforms=uniforms, use_graph=False)
    assert same(cached, plain) and same(eager, plain)
    # two frames: two prefills (an embedding launch of the context + one of the generated plane per decode step), 2 x 2 decode steps
    assert seen.count('wmz_embed_qkv_fused_fwd_slots') == 2 + 4 and 'wmz_layer_fused_fwd_planes' not in seen, seen


def test_ineligible_models(wmz):
    """context_cache=True on a model that cannot keep a cache is a ValueError; the config default keeps today's path there."""
    cfg = wmz['config']
    z = torch.randint(0, C, (1,) + CLIP).cuda()
    sym = denoiser(wmz, FUSED, CLIP, seed=73, depth=2, causal=False).cuda()
    other = denoiser(wmz, OPS, CLIP, seed=74, depth=2).cuda()
    with cfg.compute_dtype(BF), torch.no_grad():
        for m in (sym, other):
            with pytest.raises(ValueError):
                draw(wmz, m, z, True)
            today = draw(wmz, m, z, False)
            with cfg.context_cache(True), recorded_calls() as seen:
                assert same(draw(wmz, m, z, None), today)
            assert not [n for n in seen if 'slots' in n], seen


def test_config_default_turns_the_cache_on(wmz, causal_model):
    cfg, m = wmz['config'], causal_model
    z = torch.randint(0, C, (1,) + CLIP).cuda()
    HW = CLIP[1] * CLIP[2]
    g = torch.Generator().manual_seed(11)
    uniforms = (torch.rand(2, 3, HW, generator=g), torch.rand(2, 3, 1, HW, generator=g))
    with cfg.compute_dtype(BF), torch.no_grad():
        with recorded_calls() as off:
            today = draw(wmz, m, z, None, uniforms=uniforms, use_graph=False)
        with cfg.context_cache(True), recorded_calls() as on:
            cached = draw(wmz, m, z, None, uniforms=uniforms, use_graph=False)
    assert same(cached, today)
    assert not [n for n in off if 'slots' in n] and [n for n in on if 'slots' in n]


def test_precise_mode_under_the_half_guard(wmz):
    cfg = wmz['config']
    m = denoiser(wmz, FUSED, CLIP, seed=75, depth=2).cuda()
    z = torch.randint(0, C, (1,) + CLIP).cuda()
    with cfg.compute_dtype(HALF), cfg.half_guard('raise'), torch.no_grad():
        with recorded_calls() as seen:
            cached = draw(wmz, m, z, True)
        assert same(cached, draw(wmz, m, z, False))
    assert 'wmz_layer_fused_fwd_f16_slots' in seen and 'wmz_embed_qkv_fused_fwd_f16_slots' in seen, set(seen)
