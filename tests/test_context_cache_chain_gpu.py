"""The context cache at the chain kernels' widths on the GPU: the _slots form of the chain inference launch against
the trailing-planes launch it extends, the embedding of trailing planes against the whole grid's, the cached forward of a causal
chain-width denoiser against the uncached one bit for bit and against tests/causal_ref.py at the mode's bar, and the sampler with
the cache against the sampler without it, token for token.

                          kernel (_slots vs _planes)       model (forward_last vs forward)        sampler
  bf16                    bit-identical, sentinel intact    torch.equal; 1e-2 of the reference     same tokens
  precise (half)          bit-identical, sentinel intact    torch.equal; 1e-3 of the reference     same tokens, half guard 'raise'

A decode step of a depth-L model is L attention launches and L + 1 chain launches (the embedding's tail-only launch, then one per
layer), as the fused widths' decode step is L + 1 per-token launches.  bf16 grids this small take the chain kernels under
config.chain_policy 'always' only; the policy is restored behind every test."""
import contextlib

import pytest
import torch

import causal_ref
import chain_cache_cases as cases
import route_table as rt
from conftest import chain_policy, recorded_calls

pytestmark = pytest.mark.gpu

BF, HALF = torch.bfloat16, torch.float16
C = 48
FUSED, OPS = (256, 1, 128, 256), (160, 1, 128, 256)          # dim, heads, dim_head, mlp_dim
PUBLISHED_SMALL, REF_TEST, PUBLISHED_LARGE = (96, 1, 128, 256), (128, 3, 64, 256), (384, 1, 128, 512)
TOL = {'bf16': 1e-2, 'precise': 1e-3}                         # test_route_matrix_gpu.py
SENTINEL = 0x5A3C                                             # an int16 pattern no launch below is asked to write everywhere
GUARD = 4096                                                  # elements behind each buffer
SLOTS = cases.SLOTS


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


def sentinel(n, dtype):
    return torch.full((n + GUARD,), SENTINEL, dtype=torch.int16, device='cuda').view(dtype)


def intact(*bufs):
    return all(bool((bits(b) == SENTINEL).all()) for b in bufs)


def check_compact(buf, ref):
    n = ref.numel()
    assert torch.equal(bits(buf)[:n], bits(ref).view(-1)), 'x_out is not the trailing-planes launch\'s'
    assert bool((bits(buf)[n:] == SENTINEL).all()), 'the guard band behind x_out was written'


def check_slots(buf, ref, B, dp, d0, po, HW, I, halves):
    """buf: `halves` x [B, dp, HW, I] + guard, all sentinel before the launch; ref [halves, B, po, HW, I]: the named slots hold
    ref's bits, every other element still the sentinel."""
    n = halves * B * dp * HW * I
    got = bits(buf)[:n].view(halves, B, dp, HW, I)
    assert torch.equal(got[:, :, d0:d0 + po], bits(ref).view(halves, B, po, HW, I)), 'the named slots do not hold the rows'
    rest = got.clone()
    rest[:, :, d0:d0 + po] = SENTINEL
    assert bool((rest == SENTINEL).all()), 'a byte outside the named slots was written'
    assert bool((bits(buf)[n:] == SENTINEL).all()), 'the guard band behind the buffer was written'


def heads_of(D, I):
    """heads x dim_head of a stack with these widths (tests/test_chain_widths_gpu.py): never ONE head as wide as the model."""
    if I == 192:
        return 3, 64
    return (I // 128, 128) if I != D or I // 128 > 1 else (I // 64, 64)


# ----------------------------------------------------------------------------------------------------------------------- kernel

# (H, W) of a plane, clips: 80 rows per plane -- a ragged last workgroup -- | 24 rows per plane: with one plane out a wave's 16
# lanes span two clips
PLANES = [((5, 16), 2), ((3, 8), 3)]


def chain_call(L, entry, o, x, xo, q, kv, wpack, vec, B, n_q, n_in, HW, D, I, M, head, tail, *slots):
    L.call(entry, L.ptr(o), L.ptr(x), L.ptr(xo), L.ptr(q), L.ptr(kv), L.ptr(wpack), L.ptr(vec), B, n_q, n_in, HW, D, I, M, head,
           tail, 1e-5, *slots, L.stream())


@pytest.mark.parametrize('dtype', [BF, HALF], ids=['bf16', 'f16'])
@pytest.mark.parametrize('widths', cases.KERNEL_WIDTHS, ids=lambda w: 'x'.join(map(str, w[:3])))
def test_slot_launches_are_the_planes_launches_in_place(wmz, widths, dtype):
    L, fused = wmz['lib'], wmz['fused']
    D, I, M, MC = widths
    heads, dh = heads_of(D, I)
    layers = list(denoiser(wmz, (D, heads, dh, M), (2, 4, 16), seed=5, depth=2).cuda().transformer.layers)
    packs = {'head+tail': fused._chain_pack(layers[0], layers[1], D, I, M, MC, dtype),       # (any stream does: both launches of a
             'tail': fused._chain_pack(None, layers[0], D, I, M, MC, dtype)}                 #  comparison read the same one)
    planes = L.half_form('wmz_layer_chain_fwd_planes', dtype)
    slots = slots_entry('wmz_layer_chain_fwd', dtype)
    torch.manual_seed(D + I + M)
    for (H, W), B in PLANES:
        HW = H * W
        for po, dp, d0 in SLOTS:
            pi = po + 1                                                   # one more input plane: the source map is live too
            o = torch.randn(B, po, HW, I, device='cuda').to(dtype)
            x = torch.randn(B, pi, HW, D, device='cuda').to(dtype)
            for form, head in (('head+tail', 1), ('tail', 0)):
                wpack, vec = packs[form]
                x_ref = torch.empty(B, po, HW, D, dtype=dtype, device='cuda') if head else None
                q_ref = torch.empty(B, po, HW, I, dtype=dtype, device='cuda')
                kv_ref = torch.empty(2, B, po, HW, I, dtype=dtype, device='cuda')
                chain_call(L, planes, o if head else None, x, x_ref, q_ref, kv_ref, wpack, vec, B, po, pi, HW, D, I, M, head, 1)
                x_out = sentinel(B * po * HW * D, dtype)
                q, kv = sentinel(B * dp * HW * I, dtype), sentinel(2 * B * dp * HW * I, dtype)
                chain_call(L, slots, o if head else None, x, x_out if head else None, q, kv, wpack, vec, B, po, pi, HW, D, I, M,
                           head, 1, dp, d0)
                case = (form, (H, W), po, dp, d0)
                if head:
                    check_compact(x_out, x_ref)
                else:
                    assert intact(x_out), case
                check_slots(q, q_ref[None], B, dp, d0, po, HW, I, 1)
                check_slots(kv, kv_ref, B, dp, d0, po, HW, I, 2)
                assert bool(torch.isfinite(q_ref.float()).all()) and float(q_ref.float().abs().max()) > 0, case   # (real rows)


@pytest.mark.parametrize('dtype', [BF, HALF], ids=['bf16', 'f16'])
def test_a_launch_without_a_tail_is_the_planes_launch(wmz, dtype):
    """tail == 0 places nothing: x_out of the trailing-planes launch, the slot buffers untouched."""
    L, fused = wmz['lib'], wmz['fused']
    D, I, M, MC = cases.KERNEL_WIDTHS[0]
    heads, dh = heads_of(D, I)
    layers = list(denoiser(wmz, (D, heads, dh, M), (2, 4, 16), seed=6, depth=2).cuda().transformer.layers)
    wpack, vec = fused._chain_pack(layers[1], None, D, I, M, MC, dtype)
    B, HW = 3, 24
    torch.manual_seed(3)
    o, x = torch.randn(B, 1, HW, I, device='cuda').to(dtype), torch.randn(B, 2, HW, D, device='cuda').to(dtype)
    x_ref = torch.empty(B, 1, HW, D, dtype=dtype, device='cuda')
    chain_call(L, L.half_form('wmz_layer_chain_fwd_planes', dtype), o, x, x_ref, None, None, wpack, vec, B, 1, 2, HW, D, I, M, 1, 0)
    x_out = sentinel(B * HW * D, dtype)
    q, kv = sentinel(B * 3 * HW * I, dtype), sentinel(2 * B * 3 * HW * I, dtype)
    chain_call(L, slots_entry('wmz_layer_chain_fwd', dtype), o, x, x_out, q, kv, wpack, vec, B, 1, 2, HW, D, I, M, 1, 0, 3, 1)
    check_compact(x_out, x_ref)
    assert intact(q, kv)


@pytest.mark.parametrize('dtype', [BF, HALF], ids=['bf16', 'f16'])
def test_slots_refusals(wmz, dtype):
    """dst_plane0 < 0 and dst_plane0 + n_q > dst_planes are refused before anything is launched."""
    L, fused = wmz['lib'], wmz['fused']
    D, I, M, MC = cases.KERNEL_WIDTHS[0]
    heads, dh = heads_of(D, I)
    layers = list(denoiser(wmz, (D, heads, dh, M), (2, 4, 16), seed=7, depth=2).cuda().transformer.layers)
    B, HW = 1, 32
    o, x = torch.zeros(B, 2, HW, I, device='cuda', dtype=dtype), torch.zeros(B, 2, HW, D, device='cuda', dtype=dtype)   # (room for two planes)
    x_out = sentinel(B * 2 * HW * D, dtype)
    q, kv = sentinel(B * 3 * HW * I, dtype), sentinel(2 * B * 3 * HW * I, dtype)
    for po, dp, d0 in ((1, 3, -1), (1, 3, 3), (2, 3, 2), (1, 0, 0)):
        assert not cases.slots_ok(po, dp, d0)
        for head, pack in ((1, fused._chain_pack(layers[0], layers[1], D, I, M, MC, dtype)),
                           (0, fused._chain_pack(None, layers[0], D, I, M, MC, dtype))):
            with pytest.raises(L.WmzError, match='must lie inside the dst_planes slots'):
                chain_call(L, slots_entry('wmz_layer_chain_fwd', dtype), o if head else None, x, x_out if head else None, q, kv,
                           *pack, B, po, po, HW, D, I, M, head, 1, dp, d0)
    torch.cuda.synchronize()
    assert intact(x_out, q, kv)


# -------------------------------------------------------------------------------------------------------------------- embedding

@pytest.mark.parametrize('dtype', [torch.float32, BF], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('grid', [(2, 3, 5, 16), (3, 4, 3, 8)], ids=lambda g: 'x'.join(map(str, g)))
def test_embedding_of_trailing_planes(wmz, grid, dtype):
    L = wmz['lib']
    B, S, H, W = grid
    D = 96
    torch.manual_seed(S * H * W)
    emb, ps, ph, pw = (torch.randn(n, D, device='cuda') for n in (C + 1, S + 2, H, W))
    z = torch.randint(0, C + 1, grid, device='cuda')
    z[:, -1, 0, :4] = C                                                   # the mask id, in the plane every case produces
    z[0, 0, -1, -1] = C
    assert int((z == C).sum()) >= 4 * B + 1
    whole = torch.empty(B, S, H, W, D, dtype=dtype, device='cuda')
    L.call('wmz_embed_pos3d_fwd', L.ptr(z), L.ptr(emb), L.ptr(ps), L.ptr(ph), L.ptr(pw), L.ptr(whole), B, S, H, W, D, C + 1,
           L.dtype_code(dtype), L.stream())
    assert sorted({1, 2, S}) == [1, 2, S]
    for po in (1, 2, S):
        n = B * po * H * W * D
        guard = GUARD * 2 // whole.element_size()
        buf = torch.full((n + guard,), -7.0, dtype=dtype, device='cuda')
        L.call('wmz_embed_pos3d_fwd_planes', L.ptr(z), L.ptr(emb), L.ptr(ps), L.ptr(ph), L.ptr(pw), L.ptr(buf), B, S, H, W, po, D,
               C + 1, L.dtype_code(dtype), L.stream())
        assert torch.equal(buf[:n].view(B, po, H, W, D), whole[:, S - po:]), po
        assert bool((buf[n:] == -7.0).all()), po
    for po in (0, S + 1):
        with pytest.raises(L.WmzError, match='bad plane count'):
            L.call('wmz_embed_pos3d_fwd_planes', L.ptr(z), L.ptr(emb), L.ptr(ps), L.ptr(ph), L.ptr(pw), L.ptr(whole), B, S, H, W, po,
                   D, C + 1, L.dtype_code(dtype), L.stream())


# ------------------------------------------------------------------------------------------------------------------------ model

@contextlib.contextmanager
def recorded_chain_args():
    """(entry point, n_q, n_in) of every chain launch a block makes through the binding."""
    from world_modelz_amd import _lib
    seen = []
    orig = _lib.call

    def call(name, *a):
        if 'layer_chain_fwd' in name:
            seen.append((name, a[8], a[9]))
        return orig(name, *a)
    _lib.call = call
    try:
        yield seen
    finally:
        _lib.call = orig


MODEL_WIDTHS = [PUBLISHED_SMALL, REF_TEST, PUBLISHED_LARGE]
MODEL_CLIPS = [(4, 4, 16), (3, 4, 8), (3, 3, 8)]              # (3, 3, 8): an odd 8-wide plane has no half attention unit
_references = {}


def reference(wmz, widths, clip, eS, depth):
    """(state dict, two token grids, the causal reference's logits of each) of a case: computed once on the CPU, shared by both
    modes, left alone."""
    key = (widths, clip, eS, depth)
    if key not in _references:
        m = denoiser(wmz, widths, clip, seed=17 + clip[0] + eS + widths[0], depth=depth, ext=(eS, 1, 1))
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        z = torch.randint(0, C + 1, (2,) + clip)
        z2 = torch.randint(0, C + 1, (2,) + clip)
        _references[key] = (sd, z, z2, causal_ref.denoiser_forward(sd, z, (eS, 1, 1), widths[1]),
                            causal_ref.denoiser_forward(sd, z2, (eS, 1, 1), widths[1]))
    return _references[key]


@pytest.mark.parametrize('mode', ['bf16', 'precise'])
@pytest.mark.parametrize('depth', [3, 1], ids=['depth3', 'depth1'])
@pytest.mark.parametrize('eS', [1, 2], ids=['eS1', 'eS2'])
@pytest.mark.parametrize('clip', MODEL_CLIPS, ids=lambda c: 'x'.join(map(str, c)))
@pytest.mark.parametrize('widths', MODEL_WIDTHS, ids=lambda w: 'x'.join(map(str, w)))
def test_cached_forward_is_the_forward(wmz, widths, clip, eS, depth, mode):
    cfg, fused = wmz['config'], wmz['fused']
    S = clip[0]
    if mode == 'precise' and clip == (3, 3, 8):
        m = denoiser(wmz, widths, clip, seed=0, depth=depth, ext=(eS, 1, 1)).cuda()
        z = torch.randint(0, C + 1, (2,) + clip).cuda()
        with cfg.compute_dtype(HALF), torch.no_grad(), recorded_calls() as seen:
            assert not m.context_cache_eligible(z)                        # no half attention unit for this plane: the fp32 route
            with pytest.raises(ValueError):
                m.context_prefill(z)
        assert not [n for n in seen if 'slots' in n], seen
        return
    sd, z, z2, ref, ref2 = reference(wmz, widths, clip, eS, depth)
    m = denoiser(wmz, widths, clip, seed=0, depth=depth, ext=(eS, 1, 1))
    m.load_state_dict(sd)
    m = m.cuda()
    z, z2 = z.cuda(), z2.cuda()
    sfx = '_f16_slots' if mode == 'precise' else '_slots'
    with chain_policy('always'), cfg.compute_dtype(rt.MODES[mode]), torch.no_grad():
        assert m.context_cache_eligible(z)
        with recorded_calls() as plain_seen:
            y = m(z)
        assert any('layer_chain_fwd_planes' in n for n in plain_seen), plain_seen      # (the uncached forward is the chain kernels')
        cache = m.context_prefill(z)
        assert cache.family == 'chain' and cache.widths == (widths[0], widths[1] * widths[2], widths[3])
        assert cache.a == fused.context_planes(S, eS, depth) and [t.shape[1] for t in cache.q] == [n + 1 for n in cache.a]
        addresses = [t.data_ptr() for t in cache.q + cache.kv]
        with recorded_calls() as seen, recorded_chain_args() as chain:
            yc = m.forward_last(z, cache)
        assert yc.dtype == torch.float32 and yc.shape == (2,) + clip[1:] + (C,)
        assert torch.equal(yc, y), 'the cached forward is not the forward'
        # a decode step: depth attention launches and depth + 1 chain launches -- the embedding's tail, then one per layer --, one
        # plane each, on the cache's entry points; no chain launch over the whole clip
        assert seen.count('wmz_local3d_attn_fwd_window') == depth, seen
        assert not [n for n in seen if 'attn' in n and n != 'wmz_local3d_attn_fwd_window'], seen
        assert [n for n in seen if rt.is_fused_or_chain(n)] == ['wmz_layer_chain_fwd' + sfx] * (depth + 1), seen
        assert seen.count('wmz_embed_pos3d_fwd_planes') == 1 and 'wmz_embed_pos3d_fwd' not in seen, seen
        assert chain == [('wmz_layer_chain_fwd' + sfx, 1, 1)] * (depth + 1), chain
        assert S > 1 and not [c for c in chain if c[1] == S]
        # the same cache refilled for a second grid
        y2 = m(z2)
        assert not torch.equal(y2, y)
        assert m.context_prefill(z2, cache) is cache
        assert [t.data_ptr() for t in cache.q + cache.kv] == addresses
        yc2 = m.forward_last(z2, cache)
        assert torch.equal(yc2, y2), 'the cached forward on a refilled cache is not the forward'
        # ... and another last frame on the kept context
        z3 = z2.clone()
        z3[:, -1] = (z3[:, -1] + 7) % (C + 1)
        assert torch.equal(m.forward_last(z3, cache), m(z3)), 'a new last frame on the kept context is not the forward'
    e, e2 = rel(yc, ref), rel(yc2, ref2)
    print(f'[chain context cache {widths} {clip} eS {eS} depth {depth} {mode}] logits rel {e:.2e} {e2:.2e} (bar {TOL[mode]:.0e})')
    assert e < TOL[mode] and e2 < TOL[mode], (mode, e, e2)


def test_who_may_keep_a_cache(wmz):
    cfg = wmz['config']
    clip = (3, 4, 16)
    z = torch.randint(0, C + 1, (1,) + clip).cuda()
    m = denoiser(wmz, PUBLISHED_SMALL, clip, seed=3, depth=2).cuda()
    sym = denoiser(wmz, PUBLISHED_SMALL, clip, seed=3, depth=2, causal=False).cuda()
    other = denoiser(wmz, OPS, clip, seed=3, depth=2).cuda()
    wide = denoiser(wmz, REF_TEST, clip, seed=3, depth=2).cuda()
    fusedm = denoiser(wmz, FUSED, clip, seed=3, depth=2).cuda()

    def refused(model, zz, cache):
        assert not model.context_cache_eligible(zz)
        with pytest.raises(ValueError):
            model.context_prefill(zz)
        with pytest.raises(ValueError):
            model.forward_last(zz, cache)

    with recorded_calls() as seen:
        with chain_policy('always'), cfg.compute_dtype(BF), torch.no_grad():
            with recorded_calls() as good:
                cache = m.context_prefill(z)
                fcache = fusedm.context_prefill(z)
            assert cache.family == 'chain' and fcache.family == 'fused' and [n for n in good if 'slots' in n]
            del seen[:]
            refused(sym, z, cache)                                                # not causal
            refused(other, z, cache)                                              # the op-by-op widths
            refused(m, z.cpu(), cache)                                            # a CPU tensor
            with pytest.raises(ValueError):                                       # another geometry than the cache's
                m.forward_last(z[:, 1:].contiguous(), cache)
            # a cache of the other family, or of other widths of the same family
            for model, wrong in ((m, fcache), (fusedm, cache), (wide, cache)):
                assert model.context_cache_eligible(z)
                with pytest.raises(ValueError, match='this ContextCache was built for the'):
                    model.forward_last(z, wrong)
                with pytest.raises(ValueError, match='this ContextCache was built for the'):
                    model.context_prefill(z, wrong)
        with chain_policy('never'), cfg.compute_dtype(BF), torch.no_grad():      # bf16 off the chain kernels: today's path
            refused(m, z, cache)
        with chain_policy('auto'), cfg.compute_dtype(BF), torch.no_grad():       # ... and a grid too small for them to pay
            assert wmz['fused'].inference_route(m.transformer, BF, 4, 16, z.numel()) == 'ops'
            refused(m, z, cache)
        with chain_policy('always'), cfg.compute_dtype(BF):                       # with grad
            refused(m, z, cache)
        with chain_policy('always'), cfg.compute_dtype(torch.float32), torch.no_grad():     # fp32: op by op
            refused(m, z, cache)
        with chain_policy('never'), cfg.compute_dtype(HALF), torch.no_grad():     # the precise mode always takes the chain kernels
            assert m.context_cache_eligible(z)
    assert not [n for n in seen if 'slots' in n], seen


# ---------------------------------------------------------------------------------------------------------------------- sampler

CLIP = (3, 4, 16)
KW = dict(num_frames=2, num_eval_iterations=4, sample_topk=5)


def draw(wmz, m, z, cache, seed=1, **kw):
    frames, zf = wmz['sample'].sample_frames(m, z, C, generator=torch.Generator().manual_seed(seed), context_cache=cache, **KW, **kw)
    return frames + [zf]


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def injected(seed):
    HW = CLIP[1] * CLIP[2]
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(2, 4, HW, generator=g), torch.rand(2, 4, 1, HW, generator=g))


@pytest.fixture(scope='module')
def causal_model(wmz):
    return denoiser(wmz, PUBLISHED_SMALL, CLIP, seed=71, depth=2).cuda()


@pytest.mark.parametrize('mode', ['bf16', 'precise'])
def test_captured_sampler_same_tokens(wmz, causal_model, mode):
    m = causal_model
    z = torch.randint(0, C, (1,) + CLIP).cuda()
    sfx = '_f16_slots' if mode == 'precise' else '_slots'
    guard = wmz['config'].half_guard('raise') if mode == 'precise' else contextlib.nullcontext()
    with chain_policy('always'), wmz['config'].compute_dtype(rt.MODES[mode]), guard, torch.no_grad():
        plain = draw(wmz, m, z, False)
        with recorded_calls() as seen:
            cached = draw(wmz, m, z, True)
        assert same(cached, plain)
        assert 'wmz_layer_chain_fwd' + sfx in seen and 'wmz_embed_pos3d_fwd_planes' in seen, set(seen)      # (the capture's launches)
        # a second call replays the session's graphs: the prefill graph and the decode graph hold the chain passes
        ses = [s for s in m._wmz_sampler_sessions.values() if s.prefill is not None and s.cache.dtype == rt.MODES[mode]]
        assert len(ses) == 1 and ses[0].cache.family == 'chain' and ses[0].fwd.static_in is ses[0].prefill.static_in
        captures = (ses[0].fwd.recaptures, ses[0].prefill.recaptures)
        with recorded_calls() as again_seen:
            again = draw(wmz, m, z, True)
        assert same(again, plain) and (ses[0].fwd.recaptures, ses[0].prefill.recaptures) == captures
        assert not [n for n in again_seen if rt.is_fused_or_chain(n) or 'attn' in n or 'embed' in n], again_seen
        assert same(draw(wmz, m, z, True, seed=2), draw(wmz, m, z, False, seed=2))
        assert not same(draw(wmz, m, z, True, seed=2), plain)


@pytest.mark.parametrize('mode', ['bf16', 'precise'])
def test_injected_uniforms_loop_same_tokens(wmz, causal_model, mode):
    m = causal_model
    z = torch.randint(0, C, (1,) + CLIP).cuda()
    uniforms = injected(9)
    sfx = '_f16_slots' if mode == 'precise' else '_slots'
    guard = wmz['config'].half_guard('raise') if mode == 'precise' else contextlib.nullcontext()
    with chain_policy('always'), wmz['config'].compute_dtype(rt.MODES[mode]), guard, torch.no_grad():
        plain = draw(wmz, m, z, False, uniforms=uniforms)
        with recorded_calls() as seen:
            cached = draw(wmz, m, z, True, uniforms=uniforms)
    assert same(cached, plain)
    # two frames of the eager loop: two prefills and 2 x 3 decode steps (none behind a frame's last draw), each with one embedding
    # launch of trailing planes; depth 2: a prefill makes 2 chain launches, a decode step 3; no chain launch over the whole clip
    assert seen.count('wmz_embed_pos3d_fwd_planes') == 2 + 6, seen
    assert seen.count('wmz_layer_chain_fwd' + sfx) == 2 * 2 + 6 * 3, seen
    assert not [n for n in seen if 'layer_chain_fwd_planes' in n], seen


def test_config_default_turns_the_cache_on_and_ineligible_models_keep_their_launches(wmz, causal_model):
    cfg, m = wmz['config'], causal_model
    z = torch.randint(0, C, (1,) + CLIP).cuda()
    uniforms = injected(11)
    sym = denoiser(wmz, PUBLISHED_SMALL, CLIP, seed=73, depth=2, causal=False).cuda()
    with chain_policy('always'), cfg.compute_dtype(BF), torch.no_grad():
        with recorded_calls() as off:
            today = draw(wmz, m, z, None, uniforms=uniforms, use_graph=False)
        with cfg.context_cache(True), recorded_calls() as on:
            cached = draw(wmz, m, z, None, uniforms=uniforms, use_graph=False)
        assert same(cached, today)
        assert not [n for n in off if 'slots' in n] and [n for n in on if n == 'wmz_layer_chain_fwd_slots']
        # not causal: True is a ValueError, the config default keeps today's launches
        with pytest.raises(ValueError):
            draw(wmz, sym, z, True)
        with recorded_calls() as before:
            today = draw(wmz, sym, z, False, uniforms=uniforms, use_graph=False)
        with cfg.context_cache(True), recorded_calls() as seen:
            assert same(draw(wmz, sym, z, None, uniforms=uniforms, use_graph=False), today)
        assert seen == before and not [n for n in seen if 'slots' in n], seen
    # bf16 under chain_policy 'never': the model runs op by op and keeps that path under the config default
    with chain_policy('never'), cfg.compute_dtype(BF), torch.no_grad():
        with recorded_calls() as before:
            today = draw(wmz, m, z, False, uniforms=uniforms, use_graph=False)
        with cfg.context_cache(True), recorded_calls() as seen:
            assert same(draw(wmz, m, z, None, uniforms=uniforms, use_graph=False), today)
        assert seen == before and not [n for n in seen if 'slots' in n or 'layer_chain' in n], seen
