"""The precise mode's half conv route (config.precise_conv): csrc/conv_direct_f16.hip, conv_point_f16.hip and the half forms of the
element-wise kernels, against torch / the fp32 CPU oracle -- kernels on half-rounded operands, the frame encoder of main.py:229-237
(BatchNorm in training mode, quirk Q3) and the decoder, the captured encoder, and the routes that must NOT change."""
import copy

import pytest
import torch
import torch.nn.functional as F

import conv_bounds as cb
import gemm_bounds as gb
from conftest import recorded_calls
from test_conv_bf16_oracle_gpu import account_for_token_disagreements

pytestmark = pytest.mark.gpu

from oracle import autoencoder as oae        # noqa: E402

HALF_CONV = ('wmz_conv3x3_direct_fwd_strided_f16', 'wmz_conv_point_fwd_bn_f16')
BF16_CONV = ('wmz_conv3x3_direct_fwd_strided', 'wmz_conv_point_fwd_bn')


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _vqae(seed, C, hidden=128):
    from world_modelz_amd.train_vqae import VqAutoEncoder
    torch.manual_seed(seed)
    return VqAutoEncoder(embedding_dim=64, num_embeddings=C, downscale_steps=2, hidden_planes=hidden).cuda()


def _cpu_state(m):
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


def _half_mode():
    from world_modelz_amd import config
    import contextlib
    st = contextlib.ExitStack()
    st.enter_context(config.compute_dtype(torch.float16))
    st.enter_context(config.precise_conv(True))
    return st


def _check_out(y, ref, what):
    """y: the kernel's half output; ref: fp64 of the same arithmetic on the same half operands -- within the half rounding of the
    stored result."""
    y, ref = y.double().cpu(), ref.double().cpu()
    big = ref.abs() > 1e-2
    e_el = float(((y - ref).abs() / ref.abs().clamp_min(1e-30))[big].max())
    e_norm = float((y - ref).norm() / ref.norm())
    assert e_el <= 1e-3 and e_norm <= 6e-4, (what, e_el, e_norm)


def _check_stats(out, s, q):
    """the statistics are those of the STORED (rounded) half output, fp32 sums of its values"""
    y = out.double().reshape(-1, out.shape[-1])
    rs, rq = y.sum(0), (y * y).sum(0)
    ks, kq = s.double().sum(0).cpu(), q.double().sum(0).cpu()
    assert torch.allclose(ks, rs.cpu(), rtol=1e-5, atol=1e-5 * float(y.abs().sum(0).max())), float((ks - rs.cpu()).abs().max())
    assert torch.allclose(kq, rq.cpu(), rtol=1e-5), float(((kq - rq.cpu()) / rq.cpu()).abs().max())


DIRECT_GEOMS = [(2, 16, 16, ci, co, 1) for ci in (64, 128) for co in (8, 32, 64, 128)] + \
               [(2, 16, 32, ci, co, 1) for ci in (64, 128) for co in (8, 32, 64, 128)] + \
               [(1, 8, 64, ci, co, 1) for ci in (64, 128) for co in (32, 128)] + \
               [(2, 32, 32, ci, 128, 2) for ci in (64, 128)]


@pytest.mark.parametrize('geom', DIRECT_GEOMS)
def test_half_direct_3x3_vs_fp64(geom):
    """wmz_conv3x3_direct_fwd_strided_f16 (stride 1 on 16- and 32 / 64-wide planes, stride 2 at Cout 128) with and without bias,
    folded affine, LeakyReLU, residual and statistics against fp64 of the same half operands."""
    from world_modelz_amd import ops
    B, H, W, Ci, Co, st = geom
    assert ops.L.lib().wmz_conv3x3_direct_supported_strided(H, W, Ci, Co, st)
    torch.manual_seed(11)
    x = torch.randn(B, H, W, Ci, device='cuda').half()
    w = (torch.randn(Co, 9 * Ci, device='cuda') * (9 * Ci) ** -0.5).half()
    bias, sc, sh = torch.randn(Co, device='cuda'), torch.rand(Co, device='cuda') + 0.5, torch.randn(Co, device='cuda')
    Ho, Wo = H // st, W // st
    res = torch.randn(B, Ho, Wo, Co, device='cuda').half()
    w4 = w.double().view(Co, 3, 3, Ci).permute(0, 3, 1, 2)
    base = F.conv2d(x.double().permute(0, 3, 1, 2), w4, None, stride=st, padding=1).permute(0, 2, 3, 1)
    cases = [(dict(), base),
             (dict(bias=bias, leaky=True, stats=True), F.leaky_relu(base + bias.double(), 0.01)),
             (dict(scale=sc, shift=sh, stats=True), base * sc.double() + sh.double()),
             (dict(bias=bias, scale=sc, shift=sh, residual=res, leaky=True, stats=True),
              F.leaky_relu((base + bias.double()) * sc.double() + sh.double() + res.double(), 0.01)),
             (dict(residual=res), base + res.double())]
    for kw, ref in cases:
        with recorded_calls() as seen:
            out = ops.conv2d_nhwc(x, w, 3, 3, st, 1, **kw)
        assert [n for n in seen if n != 'wmz_conv3x3_direct_pack'] == ['wmz_conv3x3_direct_fwd_strided_f16'], seen
        y = out[0] if kw.get('stats') else out
        assert y.dtype == torch.float16 and y.shape == ref.shape
        _check_out(y, ref, (geom, sorted(kw)))
        if kw.get('stats'):
            _check_stats(y, out[1], out[2])


POINT_GEOMS = [(4, 16, 16, 128, 64, 1, 1, 0, False), (4, 16, 16, 128, 64, 1, 1, 0, True), (2, 16, 16, 64, 128, 1, 1, 0, False),
               (2, 16, 16, 128, 128, 1, 1, 0, True), (2, 32, 32, 64, 64, 2, 2, 0, False), (2, 32, 32, 8, 64, 3, 1, 1, False)]


@pytest.mark.parametrize('geom', POINT_GEOMS)
def test_half_small_k_conv_vs_fp64(geom):
    """wmz_conv_point_fwd_bn_f16: 1x1 with and without the training-mode BatchNorm prologue from raw statistics (finalised by the
    launch), 2x2 / stride 2, the 3-channel conv_1 (3x3 / pad 1 over 8 padded channels)."""
    from world_modelz_amd import ops
    B, H, W, Ci, Co, k, st, pad, pre = geom
    assert ops.L.lib().wmz_conv_point_supported(B, H, W, Ci, Co, k, k, st, pad)
    torch.manual_seed(12)
    x = (torch.randn(B, H, W, Ci, device='cuda') * 0.7 + 0.2).half()
    if Ci == 8:
        x[..., 3:] = 0
    w = (torch.randn(Co, k * k * Ci, device='cuda') * (k * k * Ci) ** -0.5).half()
    bias, sc, sh = torch.randn(Co, device='cuda'), torch.rand(Co, device='cuda') + 0.5, torch.randn(Co, device='cuda')
    xin = x.double()
    for kw in (dict(bias=bias, leaky=True, stats=True), dict(scale=sc, shift=sh)):
        prol = None
        if pre:
            bn = torch.nn.BatchNorm2d(Ci).cuda().train()
            with torch.no_grad():
                bn.weight.copy_(torch.rand(Ci) + 0.5)
                bn.bias.copy_(torch.randn(Ci) * 0.3)
            s, q = ops.channel_stats_nhwc(x)
            lz = ops.bn_lazy(bn, s, q, B * H * W)
            prol = (lz, None, 0.01)
            xf = x.double().reshape(-1, Ci)
            mean, var = xf.mean(0), xf.var(0, unbiased=False)
            scale = bn.weight.detach().double() / torch.sqrt(var + bn.eps)
            shift = bn.bias.detach().double() - mean * scale
            # (the kernel rounds the prologue's result to the half MFMA operand)
            xin = F.leaky_relu(x.double() * scale + shift, 0.01).half().double()
        w4 = w.double().view(Co, k, k, Ci).permute(0, 3, 1, 2)
        base = F.conv2d(xin.permute(0, 3, 1, 2), w4, None, stride=st, padding=pad).permute(0, 2, 3, 1)
        ref = F.leaky_relu(base + bias.double(), 0.01) if 'bias' in kw else base * sc.double() + sh.double()
        with recorded_calls() as seen:
            out = ops.conv2d_nhwc(x, w, k, k, st, pad, pre=prol, **kw)
        assert seen[-1] == 'wmz_conv_point_fwd_bn_f16' and not any(n in BF16_CONV for n in seen), seen
        y = out[0] if kw.get('stats') else out
        assert y.dtype == torch.float16
        if pre:
            # the prologue's half rounding may land one ulp apart from the fp64 reference's: element by element under the bound that
            # carries that rounding and the error of the launch's own BatchNorm finalisation through |w| (tests/conv_bounds.py)
            assert rel(y, ref) < 1e-3, (geom, rel(y, ref))
            fold = cb.bn_fold_ref(s.cpu(), q.cpu(), B * H * W, bn.weight.detach(), bn.bias.detach(), bn.eps)
            a = cb.prologue(x.cpu(), fold['scale'], fold['shift'], 0.01, torch.float16, fold['e_scale'], fold['e_shift'])
            r = cb.conv_fwd_ref(x.cpu(), w.cpu(), k, k, st, pad, pre=a, **{n: (v.cpu() if torch.is_tensor(v) else v)
                                                                          for n, v in kw.items() if n != 'stats'})
            print(f'[bound] half small-K {geom} {sorted(kw)}: {gb.check("prologue", y.cpu(), r["ref"], r["e_in"], norm_tol=1e-3):.3f}')
        else:
            _check_out(y, ref, geom)
        if kw.get('stats'):
            _check_stats(y, out[1], out[2])


def test_half_elementwise_kernels_vs_torch():
    """nchw_to_nhwc8 (fp32 frames -> half NHWC), channel_stats, affine_act (plain and the _bn form that finalises a training-mode
    BatchNorm and moves its running statistics), bilinear2x -- the half forms against torch on the same half values."""
    from world_modelz_amd import ops
    torch.manual_seed(13)
    fr = torch.rand(3, 3, 32, 32, device='cuda') * 2 - 1
    with recorded_calls() as seen:
        y = ops.nchw_to_nhwc8(fr, torch.float16)
    assert seen == ['wmz_nchw_to_nhwc8'] and y.dtype == torch.float16 and y.shape == (3, 32, 32, 8)
    assert torch.equal(y.cpu(), F.pad(fr.permute(0, 2, 3, 1), (0, 5)).half().cpu())

    x = (torch.randn(4, 16, 16, 64, device='cuda') * 2 + 0.5).half()
    for t in (x, x[..., :24].contiguous()):                   # (the 16-byte kernel, and the scalar one: 256 % (24 / 8) != 0)
        s, q = ops.channel_stats_nhwc(t)
        tf = t.double().reshape(-1, t.shape[-1]).cpu()
        assert torch.allclose(s.double().sum(0).cpu(), tf.sum(0), rtol=1e-5, atol=1e-3)
        assert torch.allclose(q.double().sum(0).cpu(), (tf * tf).sum(0), rtol=1e-5)

    b = torch.randn(4, 16, 16, 64, device='cuda').half()
    sa, ta = torch.rand(64, device='cuda') + 0.5, torch.randn(64, device='cuda')
    sb, tb = torch.rand(64, device='cuda') + 0.5, torch.randn(64, device='cuda')
    y = ops.affine_act_nhwc(x, sa, ta, b, sb, tb, leaky=True, slope=0.01)
    ref = F.leaky_relu(x.double() * sa.double() + ta.double() + (b.double() * sb.double() + tb.double()), 0.01)
    assert y.dtype == torch.float16 and rel(y, ref) < 6e-4
    x24 = x[..., :24].contiguous()
    y = ops.affine_act_nhwc(x24, sa[:24].contiguous(), ta[:24].contiguous(), leaky=True, slope=0.01)
    assert rel(y, F.leaky_relu(x24.double() * sa[:24].double() + ta[:24].double(), 0.01)) < 6e-4

    bn = torch.nn.BatchNorm2d(64).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(64) + 0.5)
        bn.bias.copy_(torch.randn(64))
    bn_ref = copy.deepcopy(bn)
    s, q = ops.channel_stats_nhwc(x)
    with recorded_calls() as seen:
        y = ops.affine_act_nhwc(x, ops.bn_lazy(bn, s, q, x.numel() // 64), None, b, sb, tb, leaky=True, slope=0.01)
    assert seen == ['wmz_affine_act_nhwc_bn'], seen
    xr = bn_ref(x.float().permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    ref = F.leaky_relu(xr.double() + b.double() * sb.double() + tb.double(), 0.01)
    assert rel(y, ref) < 1e-3, rel(y, ref)
    assert torch.allclose(bn.running_mean, bn_ref.running_mean, rtol=1e-4, atol=1e-5)
    assert torch.allclose(bn.running_var, bn_ref.running_var, rtol=1e-4, atol=1e-5)
    assert int(bn.num_batches_tracked) == int(bn_ref.num_batches_tracked) == 1

    for t in (x, x24):
        y = ops.bilinear2x_nhwc(t)
        ref = F.interpolate(t.double().permute(0, 3, 1, 2), scale_factor=2, mode='bilinear', align_corners=False).permute(0, 2, 3, 1)
        assert y.dtype == torch.float16 and y.shape == ref.shape
        assert float(((y.double() - ref).abs() / ref.abs().clamp_min(1e-2)).max()) < 1e-3


@pytest.mark.parametrize('C', [512, 1024])
def test_half_route_frame_encoder_vs_oracle(C):
    """main.py:229-237 on the half route: 32 frames of 64 x 64, BatchNorm in training mode.  Latents, tokens (every disagreement a
    near-tie within the latent error), running statistics against the fp32 oracle; strictly fewer disagreements than the bf16 route
    on the same frames and weights."""
    from world_modelz_amd import config
    m = _vqae(51, C)
    m.train()
    m16 = copy.deepcopy(m)
    sd = _cpu_state(m)
    torch.manual_seed(52)
    frames = torch.rand(32, 3, 64, 64)
    p = {k: v.clone() for k, v in sd.items()}
    lat_ref = oae.encoder_forward(p, frames, training=True).permute(0, 2, 3, 1).contiguous()
    with _half_mode(), torch.no_grad(), recorded_calls() as seen:
        h = m.encoder.forward_nhwc(frames.cuda())
        lat = h.float()
        tok = m.vq.encode(lat).reshape(-1).cpu()
    assert h.dtype == torch.float16
    assert all(n in seen for n in HALF_CONV), set(seen)
    assert not any(n.startswith('wmz_conv2d_nhwc_fwd') or n in BF16_CONV for n in seen), set(seen)
    lat = lat.cpu()
    e_lat = rel(lat, lat_ref)
    cb = sd['vq.embedding'][0]
    agree, n_bad = account_for_token_disagreements(tok, lat.reshape(-1, 64), lat_ref.reshape(-1, 64), cb)
    with config.compute_dtype(torch.bfloat16), torch.no_grad():
        lat16 = m16._latents(frames.cuda())
        tok16 = m16.vq.encode(lat16).reshape(-1).cpu()
    agree16, n_bad16 = account_for_token_disagreements(tok16, lat16.float().cpu().reshape(-1, 64), lat_ref.reshape(-1, 64), cb)
    print(f'[precise conv, C={C}] latents rel {e_lat:.3e} (target 3e-3; bf16 route {rel(lat16, lat_ref):.3e}); token agreement '
          f'{agree:.4f} (target 0.995; bf16 route {agree16:.4f}), disagreements {n_bad} vs {n_bad16}')
    assert lat.shape == lat_ref.shape and torch.isfinite(lat).all() and e_lat < 5e-3, e_lat
    assert agree >= 0.99, agree
    assert n_bad < n_bad16, (n_bad, n_bad16)
    for k, v in m.state_dict().items():
        if not k.startswith('encoder.'):
            continue
        if k.endswith('running_mean'):
            assert torch.allclose(v.cpu(), p[k], rtol=5e-3, atol=5e-4), (k, float((v.cpu() - p[k]).abs().max()))
        elif k.endswith('running_var'):
            assert torch.allclose(v.cpu(), p[k], rtol=5e-3, atol=5e-5), (k, float((v.cpu() - p[k]).abs().max()))
        elif k.endswith('num_batches_tracked'):
            assert int(v) == int(p[k]) == 1, k


@pytest.mark.parametrize('training', [False, True])
def test_half_route_decoder_vs_oracle(training):
    """VqAutoEncoder.decode(tokens) on the half route against oracle.vqae_decode on the same weights, BatchNorm in eval mode (with
    moved running statistics) and in training mode."""
    m = _vqae(53, 512)
    with torch.no_grad():
        for mod in m.decoder.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.copy_(torch.randn_like(mod.running_mean) * 0.1)
                mod.running_var.copy_(torch.rand_like(mod.running_var) + 0.5)
                mod.weight.copy_(torch.rand_like(mod.weight) + 0.5)
                mod.bias.copy_(torch.randn_like(mod.bias) * 0.1)
    m.train(training)
    sd = _cpu_state(m)
    torch.manual_seed(54)
    z = torch.randint(0, 512, (8, 16, 16))
    ref = oae.vqae_decode({k: v.clone() for k, v in sd.items()}, z, training)
    with _half_mode(), torch.no_grad(), recorded_calls() as seen:
        y = m.decode(z.cuda())
    assert all(n in seen for n in HALF_CONV), set(seen)
    assert not any(n.startswith('wmz_conv2d_nhwc_fwd') or n in BF16_CONV for n in seen), set(seen)
    e = rel(y, ref)
    print(f'[precise conv decoder, training={training}] rel {e:.3e}')
    assert y.shape == ref.shape and e < 5e-3, e


def test_half_route_graphed_encoder_matches_eager():
    """graph.GraphedEncoder (what bench.py's frame encoder replays) on the half route: the captured pass is the eager one (same
    entry points, in order) and gives eager encode's tokens and running statistics on an identical model copy.  Training-mode
    BatchNorm sums its statistics with float atomics, so the last bits of a pass vary from run to run -- in fp32 invisible in the
    tokens, in half they can move an element across a rounding boundary and, rarely, flip a near-tie token: the comparison
    allows that (and prints how often a second eager copy differs from the first, for scale)."""
    from world_modelz_amd.graph import GraphedEncoder
    a1 = _vqae(55, 512)
    a1.train()
    a0, a2 = copy.deepcopy(a1), copy.deepcopy(a1)
    frames = [torch.rand(16, 3, 64, 64, device='cuda') for _ in range(3)]
    with _half_mode(), torch.no_grad():
        with recorded_calls() as eager_calls:
            a0.encode(frames[0])
        with recorded_calls() as seen:
            enc = GraphedEncoder(a2, frames[0], warmup=1)
        assert all(n in seen for n in HALF_CONV), set(seen)
        # (warm-up + capture: the eager sequence twice; weight packs run at an operand's first use only)
        unpacked = [n for n in eager_calls if not n.endswith('_pack')]
        assert [n for n in seen if not n.endswith('_pack')] == unpacked * 2, seen
        a1.load_state_dict(a2.state_dict())                 # (the warm-up call moved a2's statistics: a1 starts from there)
        a3 = copy.deepcopy(a1)
        n_graph = n_eager = 0
        for f in frames:
            t1 = a1.encode(f)
            t2 = enc(f).clone()
            t3 = a3.encode(f)
            n_graph += int((t1 != t2).sum())
            n_eager += int((t1 != t3).sum())
        n = 3 * t1.numel()
        print(f'[captured half encoder] tokens differing from eager: {n_graph} of {n}; a second eager copy: {n_eager} of {n}')
        # (measured: 17 and 15 of 12 288 -- the graph differs from eager as much as eager differs from itself)
        assert n_graph <= max(3, 2 * n_eager) and n_graph <= n // 200, (n_graph, n_eager)
    sd1, sd2 = a1.state_dict(), a2.state_dict()
    for k in sd1:
        if 'running' in k or 'num_batches' in k:
            assert torch.allclose(sd1[k].float(), sd2[k].float(), rtol=1e-4, atol=1e-6), k


def _encode_calls_and_latents(m, frames, **mode):
    from world_modelz_amd import config
    with config.compute_dtype(mode['dtype']), config.precise_conv(mode['switch']), torch.no_grad(), recorded_calls() as seen:
        lat = m._latents(frames)
        img = m.decode(m.vq.encode(lat).view(lat.shape[:-1]))
    return list(seen), lat, img


def _same_passes(m, frames, a, b):
    """Eval-mode BatchNorm gives bit-comparable passes (training mode sums its statistics with float atomics); the training-mode
    pass is compared by the entry points it reaches, in order."""
    for training in (False, True):
        m.train(training)
        c_a, l_a, i_a = _encode_calls_and_latents(m, frames, **a)
        c_b, l_b, i_b = _encode_calls_and_latents(m, frames, **b)
        unpacked = lambda c: [n for n in c if not n.endswith('_pack')]      # (a weight pack runs at an operand's first use only)
        assert unpacked(c_a) == unpacked(c_b), (training, c_a, c_b)
        assert not any(n in HALF_CONV for n in c_a), c_a
        if not training:
            assert torch.equal(l_a, l_b) and torch.equal(i_a, i_b)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_switch_has_no_effect_in_the_bf16_and_fp32_modes(dtype):
    m = _vqae(57, 256)
    frames = torch.rand(8, 3, 64, 64, device='cuda')
    _same_passes(m, frames, dict(dtype=dtype, switch=False), dict(dtype=dtype, switch=True))


def test_precise_mode_with_the_switch_off_is_the_fp32_route():
    from world_modelz_amd import config
    m = _vqae(58, 256)
    frames = torch.rand(8, 3, 64, 64, device='cuda')
    assert not config.get_precise_conv()                    # (the default)
    _same_passes(m, frames, dict(dtype=torch.float16, switch=False), dict(dtype=torch.float32, switch=False))
    m.train()
    with config.compute_dtype(torch.float16), torch.no_grad(), recorded_calls() as seen:
        h = m.encoder.forward_nhwc(frames)
    assert h.dtype == torch.float32 and 'wmz_conv2d_nhwc_fwd_pre' in seen
    assert not any(n in HALF_CONV or n in BF16_CONV for n in seen), set(seen)


def test_switch_on_with_gradients_takes_the_fp32_route():
    m = _vqae(59, 256)
    m.train()
    frames = torch.rand(8, 3, 64, 64, device='cuda')
    with _half_mode(), recorded_calls() as seen:
        h = m.encoder.forward_nhwc(frames.requires_grad_(True))
        h.float().sum().backward()
    assert h.dtype == torch.float32 and frames.grad is not None
    assert not any(n in HALF_CONV for n in seen), set(seen)


def test_geometry_off_the_half_kernels_runs_the_whole_pass_fp32():
    """hidden_planes = 96: the stride-2 3x3 (Cout 96) has no direct kernel and K = 576 is beyond the streaming one -- the whole
    encoder pass runs fp32 (not a mix of half and fp32 layers), and so does the decoder (Cin 96 3x3)."""
    from world_modelz_amd import autoencoder
    m = _vqae(60, 256, hidden=96)
    m.train()
    sd = _cpu_state(m)
    frames = torch.rand(8, 3, 32, 32)
    lat_ref = oae.encoder_forward({k: v.clone() for k, v in sd.items()}, frames, training=True).permute(0, 2, 3, 1)
    with _half_mode(), torch.no_grad(), recorded_calls() as seen:
        assert autoencoder.conv_route(m.encoder, frames.shape) == torch.float32
        h = m.encoder.forward_nhwc(frames.cuda())
        m.decode(m.vq.encode(h.float()).view(h.shape[:-1]))
    assert h.dtype == torch.float32
    assert not any(n in HALF_CONV or n in BF16_CONV for n in seen), set(seen)
    assert rel(h, lat_ref) < 2e-3


@pytest.mark.parametrize('lo', [0.0, -1.0])
def test_half_route_latents_finite_over_the_frame_range(lo):
    m = _vqae(61, 256)
    m.train()
    frames = torch.rand(16, 3, 64, 64, device='cuda') * (1.0 - lo) + lo
    with _half_mode(), torch.no_grad(), recorded_calls() as seen:
        h = m.encoder.forward_nhwc(frames)
    assert h.dtype == torch.float16 and 'wmz_conv3x3_direct_fwd_strided_f16' in seen
    assert torch.isfinite(h).all()
