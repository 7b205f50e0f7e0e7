"""config.half_guard on the GPU: the half per-token kernels (csrc/layer_fused_f16.hip, layer_chain*_f16.hip) report a value whose
rounding to IEEE half left +-65504; 'raise' raises, 'fallback' gives the fp32 mode's result bit for bit, 'off' is the precise mode
as it was (and shows the hazard).  Models as in tests/test_route_matrix_gpu.py (B 2, S 3, 48 classes, depth 2): the default widths
on 16 x 16 and 8 x 8 planes (fused kernels) and the dim-96 chain triple.  Overflow to an infinity is ordinary arithmetic: nothing
here faults.  The conv encoder / decoder's half route: tests/test_half_guard_conv_gpu.py."""
import warnings

import pytest
import torch

import route_table as rt
from conftest import recorded_calls

pytestmark = pytest.mark.gpu

from oracle import denoiser as oden          # noqa: E402

B, S, C = 2, 3, 48
DEFAULT, CHAIN96 = (256, 1, 128, 256), (96, 1, 128, 256)
CELLS = [(DEFAULT, 16, 16), (DEFAULT, 8, 8), (CHAIN96, 16, 16)]
IDS = ['256-16x16', '256-8x8', '96-16x16']
EXT = {(16, 16): (1, 1, 2), (8, 8): (3, 3, 3)}
TOL_FP32 = 1e-5                              # tests/test_route_matrix_gpu.py TOL['fp32']


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(scope='module')
def wmz():
    assert torch.cuda.is_available()
    from world_modelz_amd import config, main
    from world_modelz_amd._lib import WmzError
    return dict(config=config, main=main, WmzError=WmzError)


def _model(wmz, widths, H, W, seed):
    dim, heads, dh, mlp = widths
    torch.manual_seed(seed)
    return wmz['main'].VqVideoDiffusionModel(data_shape=(S, H, W), dim=dim, num_classes=C, extents=EXT[(H, W)], depth=2,
                                             dim_head=dh, mlp_dim=mlp, heads=heads)


# ---- how each case makes a value leave the half range (in place, on the CPU model, before .cuda())
def first_store(m):                          # the stream at the embedding's store
    m.transformer.embedding.weight.data.mul_(1e5)


def first_store_negative(m):                 # ... towards -inf only
    w = m.transformer.embedding.weight.data
    w.copy_(-w.abs() * 1e5 - 1e5)


def last_ff_out(m):                          # the stream at the LAST per-token kernel's store only
    m.transformer.layers[-1][1].fn.net[3].weight.data.mul_(1e7)


def last_gelu_hidden(m):                     # an MFMA operand only: GELU hidden ~1e6, W2 scaled back -- every STORED tensor is O(1) in fp32
    ff = m.transformer.layers[-1][1].fn
    ff.net[0].weight.data.mul_(1e6)
    ff.net[0].bias.data.mul_(1e6)
    ff.net[3].weight.data.mul_(1e-6)


def keys_only(m):
    m.transformer.layers[1][0].fn.to_k.weight.data.mul_(1e5)


def values_only(m):
    a = m.transformer.layers[1][0].fn
    a.to_v.weight.data.mul_(1e6)
    a.to_v.bias.data.mul_(1e6)


OVERFLOWS = [first_store, first_store_negative, last_ff_out, last_gelu_hidden, keys_only, values_only]
KIND = {first_store: 'residual stream', first_store_negative: 'residual stream', last_ff_out: 'residual stream',
        last_gelu_hidden: 'residual stream', keys_only: 'q / k', values_only: 'q / k'}       # (regular expressions: no '|')


def _oracle_bound(sd, z, ext, heads, ref, e):
    """The fp32 bound of the route matrix (1e-5 relative); only where the fallback's distance e misses it -- magnitudes nobody
    measured the fp32 route at -- 4 x the oracle's own float32-against-float64 distance on the same input (the kernels' summation
    order differs from ATen's).  Returns (bound, that distance)."""
    ref64 = oden.denoiser_forward({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, z, ext, heads)
    own = rel(ref, ref64)
    return (TOL_FP32 if e < TOL_FP32 else 4 * own), own


@pytest.mark.parametrize('overflow', OVERFLOWS, ids=[f.__name__ for f in OVERFLOWS])
@pytest.mark.parametrize('widths,H,W', CELLS, ids=IDS)
def test_overflow_is_raised_or_falls_back_to_the_fp32_mode(wmz, widths, H, W, overflow):
    cfg = wmz['config']
    ext, heads = EXT[(H, W)], widths[1]
    m = _model(wmz, widths, H, W, seed=H * W + widths[0])
    overflow(m)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    z = torch.randint(0, C + 1, (B, S, H, W))
    ref = oden.denoiser_forward(sd, z, ext, heads)
    m, zc = m.cuda().eval(), z.cuda()
    route = rt.expected_route(widths, 'precise', H, W, 'always')
    assert route in ('fused', 'chain')
    with torch.no_grad():
        with cfg.compute_dtype(torch.float32):
            y32 = m(zc)
        with cfg.compute_dtype(torch.float16):
            assert cfg.get_half_guard() == 'off'
            with recorded_calls() as seen_off:
                y_off = m(zc)
            assert not any('half_guard' in n for n in seen_off), seen_off
            e_off = rel(y_off, ref) if bool(torch.isfinite(y_off).all()) else float('inf')
            print(f'[half guard] {overflow.__name__} {widths[0]} {H}x{W}: guard off, half route rel {e_off:.2e}')
            assert e_off > 0.1, 'the case does not overflow: it shows nothing'          # the hazard: not finite, or grossly wrong
            with cfg.half_guard('raise'), pytest.raises(wmz['WmzError'], match=KIND[overflow]) as ei:
                m(zc)
            assert 'VqVideoDiffusionModel.forward' in str(ei.value)
            with cfg.half_guard('fallback'), warnings.catch_warnings(record=True) as w:
                warnings.simplefilter('always')
                with recorded_calls() as seen:
                    y = m(zc)
                y_again = m(zc)                                                        # the second call warns no more
            assert cfg.get_half_guard() == 'off'
    assert len([x for x in w if 'IEEE half' in str(x.message)]) == 1, [str(x.message) for x in w]
    assert torch.equal(y, y32) and torch.equal(y_again, y32), 'the fallback must be the fp32 mode bit for bit'
    assert bool(torch.isfinite(y).all())
    # the half entry points, then the fp32 route
    half = [i for i, n in enumerate(seen) if n.endswith('_f16')]
    ops = [i for i, n in enumerate(seen) if n.startswith('wmz_linear_fwd') and not n.endswith('_f16')]
    assert half and ops and max(half) < min(ops), seen
    assert seen[0] == 'wmz_half_guard_clear' or seen[:2] == ['wmz_half_guard_bind', 'wmz_half_guard_clear'], seen[:3]
    assert not any(rt.is_fused_or_chain(n) and not n.endswith('_f16') for n in seen), seen
    e = rel(y, ref)
    tol, own = _oracle_bound(sd, z, ext, heads, ref, e)
    print(f'[half guard] {overflow.__name__} {widths[0]} {H}x{W}: fallback rel {e:.2e} to the fp32 oracle (oracle f32 vs f64 {own:.2e}, '
          f'bound {tol:.2e})')
    assert e < tol, f'fallback {e:.3e} against the fp32 oracle; bound {tol:.3e}; the oracle\'s own f32-vs-f64 distance {own:.3e}'


@pytest.mark.parametrize('widths,H,W', CELLS, ids=IDS)
def test_no_false_positive_below_the_range(wmz, widths, H, W):
    """A stream that peaks between 3e4 and 6e4 (asserted on the fp32 route's stream), and the default random model: 'raise' raises
    nothing and the logits are the 'off' run's bit for bit."""
    cfg = wmz['config']
    for scaled in (True, False):
        m = _model(wmz, widths, H, W, seed=5 + H).cuda().eval()
        zc = torch.randint(0, C + 1, (B, S, H, W), device='cuda')
        tr = m.transformer
        with torch.no_grad():
            if scaled:
                x0 = tr.embedding.weight[zc] + tr.get_pos_embedding(zc.shape)
                for t in (tr.embedding, tr.pos_emb_s, tr.pos_emb_h, tr.pos_emb_w):      # x0 is linear in the four tables
                    t.weight.mul_(4.5e4 / float(x0.abs().max()))
                with cfg.compute_dtype(torch.float32):
                    peak = max(float((tr.embedding.weight[zc] + tr.get_pos_embedding(zc.shape)).abs().max()),
                               float(tr(zc).abs().max()))
                print(f'[half guard] {widths[0]} {H}x{W}: fp32 stream peak {peak:.4g}')
                assert 3e4 < peak < 6e4, peak
            with cfg.compute_dtype(torch.float16):
                y_off = m(zc)
                with cfg.half_guard('raise'), recorded_calls() as seen:
                    y = m(zc)
                    t = tr(zc)
        assert 'wmz_half_guard_clear' in seen and any(n.endswith('_f16') for n in seen), seen
        assert bool(torch.isfinite(y_off).all()) and torch.equal(y, y_off)
        assert bool(torch.isfinite(t).all())


def test_guard_is_inert_outside_the_half_route(wmz):
    """bf16 and fp32 modes, and a precise-mode plane on the fp32 route: no guard entry point is reached whatever the policy."""
    cfg = wmz['config']
    m = _model(wmz, DEFAULT, 16, 16, seed=3).cuda().eval()
    zc = torch.randint(0, C + 1, (B, S, 16, 16), device='cuda')
    m12 = wmz['main'].VqVideoDiffusionModel(data_shape=(S, 12, 12), dim=256, num_classes=C, extents=(1, 0, 1), depth=2, dim_head=128,
                                            mlp_dim=256, heads=1).cuda().eval()
    z12 = torch.randint(0, C + 1, (B, S, 12, 12), device='cuda')
    with torch.no_grad(), cfg.half_guard('raise'):
        for mode, model, z in ((torch.bfloat16, m, zc), (torch.float32, m, zc), (torch.float16, m12, z12)):
            with cfg.compute_dtype(mode), recorded_calls() as seen:
                model(z)
                model.transformer(z)
            assert not any('half_guard' in n for n in seen), (mode, seen)


def _uniforms(n_iter, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(1, n_iter, B * H * W, generator=g), torch.rand(1, n_iter, B, H * W, generator=g)


def test_graphed_forward_clean_overflowing_clean(wmz):
    """GraphedForward under 'fallback': a clean replay, one after the weights were scaled in place (the way a trainer step changes
    them: the runner re-captures), a clean one again -- the word does not stay set."""
    from world_modelz_amd.graph import GraphedForward
    cfg = wmz['config']
    H = W = 16
    m = _model(wmz, DEFAULT, H, W, seed=11).cuda().eval()
    zc = torch.randint(0, C + 1, (B, S, H, W), device='cuda')
    emb = m.transformer.embedding.weight
    with torch.no_grad():
        with cfg.compute_dtype(torch.float16):
            y_clean = m(zc).clone()
        with cfg.compute_dtype(torch.float16), cfg.half_guard('fallback'), warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            run = GraphedForward(m, zc)
            with recorded_calls() as seen:
                y1 = run(zc).clone()
            assert torch.equal(y1, y_clean) and len(w) == 0
            assert 'wmz_half_guard_clear' in seen and not any(n.endswith('_f16') for n in seen), seen     # a replay launches nothing by name
            emb.mul_(1e5)
            with cfg.compute_dtype(torch.float32):
                y32 = m(zc).clone()
            y2 = run(zc).clone()
            assert torch.equal(y2, y32) and bool(torch.isfinite(y2).all())
            assert len([x for x in w if 'GraphedForward' in str(x.message)]) == 1, [str(x.message) for x in w]
            emb.mul_(1e-5)
            y3 = run(zc).clone()
            assert bool(torch.isfinite(y3).all()) and rel(y3, y_clean) < 1e-3          # (emb * 1e5 * 1e-5 rounds: not bit-equal weights)
            assert len([x for x in w if 'GraphedForward' in str(x.message)]) == 1
        with cfg.compute_dtype(torch.float16), cfg.half_guard('raise'):
            emb.mul_(1e5)
            with pytest.raises(wmz['WmzError'], match='GraphedForward'):
                run(zc)
            emb.mul_(1e-5)
            run(zc)                                                                    # clean again: nothing raised


def test_graphed_sampler_falls_back_to_the_fp32_tokens(wmz):
    """sample_frames(use_graph=True) on injected uniforms, an overflowing model: one check per call, the tokens are the fp32 mode's;
    a clean model under 'raise' gives the 'off' run's tokens."""
    from world_modelz_amd import sample
    cfg = wmz['config']
    H, W, n_iter = 8, 16, 4
    u = _uniforms(n_iter, H, W, seed=9)
    for overflowing in (True, False):
        torch.manual_seed(77)
        m = wmz['main'].VqVideoDiffusionModel(data_shape=(S, H, W), dim=256, num_classes=C, extents=(1, 1, 1), depth=2, dim_head=128,
                                              mlp_dim=256, heads=1)
        if overflowing:
            first_store(m)
        m = m.cuda().eval()
        z = torch.randint(0, C, (B, S, H, W), device='cuda')
        kw = dict(num_frames=1, num_eval_iterations=n_iter, uniforms=u, use_graph=True)
        with cfg.compute_dtype(torch.float32):
            f32, _ = sample.sample_frames(m, z, C, **kw)
        with cfg.compute_dtype(torch.float16):
            off, _ = sample.sample_frames(m, z, C, **kw)
            policy = 'fallback' if overflowing else 'raise'
            with cfg.half_guard(policy), warnings.catch_warnings(record=True) as w, recorded_calls() as seen:
                warnings.simplefilter('always')
                got, _ = sample.sample_frames(m, z, C, **kw)
        assert seen.count('wmz_half_guard_clear') == 1, seen
        if overflowing:
            assert len([x for x in w if 'sample.sample_frames' in str(x.message)]) == 1
            assert torch.equal(got[0], f32[0])
        else:
            assert len(w) == 0 and torch.equal(got[0], off[0])
