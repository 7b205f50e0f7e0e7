"""Planes 32 wide on the attention row kernel (csrc/attn_fwd_row32.hip, attn_fwd_row32_f16.hip: the W32 mode of attn_fwd_row16.hip,
a plane [H, 32] read as 2H tile rows of 16) against the fp32 CPU oracle and the general kernel, at the bars of the 16- and 8-wide
tests (tests/test_kernels_gpu.py, tests/test_precise_mode_gpu.py): probed logits <= 1e-3 with the literal -1e9 in exactly the
oracle's masked slots, lse 1e-4, out <= 3e-3; half operands <= 1e-3 on un-rounded fp32 inputs; the default denoiser in the
precise mode <= 1e-3 on the fused half kernels.  The cases reach every instantiation the dispatch can launch: workgroup shape
(`small`: up to 8 tile rows, `big` above) x chunks whole (`aligned`) or not (`ragged`) x dim_head, named in the test ids."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import attention as oat          # noqa: E402
from oracle import denoiser as oden          # noqa: E402

CASES = [
    pytest.param((1, 2, 1, 32), 1, 128, (1, 0, 1), id='small-ragged-128-one-plane-row'),          # one plane row = two tile rows
    pytest.param((1, 3, 2, 32), 2, 64, (1, 1, 3), id='small-aligned-64'),
    pytest.param((2, 3, 4, 32), 1, 128, (1, 3, 3), id='small-aligned-128-two-workgroups'),        # 8 tile rows
    pytest.param((1, 2, 5, 32), 4, 32, (0, 2, 2), id='big-ragged-32-ten-tile-rows'),
    pytest.param((1, 2, 8, 32), 1, 128, (1, 1, 1), id='big-aligned-128-one-chunk'),               # exactly one 16-row chunk
    pytest.param((1, 2, 20, 32), 1, 64, (1, 2, 2), id='big-ragged-64-three-workgroups'),
    pytest.param((1, 2, 3, 32), 1, 128, (0, 1, 16), id='small-ragged-128-seam-open'),             # eW = 16: the seam mask opens for most lanes
    pytest.param((1, 2, 4, 32), 1, 128, (1, 9, 31), id='small-aligned-128-window-over-plane'),
    pytest.param((1, 2, 2, 32), 4, 32, (1, 1, 15), id='small-aligned-32-seam-15'),                # eW = 15: every lane but one pair sees over the seam
    pytest.param((1, 2, 3, 32), 4, 32, (1, 1, 2), id='small-ragged-32'),
    pytest.param((1, 2, 1, 32), 2, 64, (0, 0, 40), id='small-ragged-64-whole-row'),
    pytest.param((1, 1, 8, 32), 4, 32, (0, 1, 17), id='big-aligned-32-seam-17'),
    pytest.param((1, 2, 16, 32), 2, 64, (0, 3, 0), id='big-aligned-64-column-only'),              # eW = 0: nothing over the seam at all
    pytest.param((1, 2, 9, 32), 1, 128, (1, 2, 5), id='big-ragged-128'),
]


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(scope='module')
def wmz():
    assert torch.cuda.is_available()
    from world_modelz_amd import _lib, config, fused, main, ops
    return dict(lib=_lib, config=config, fused=fused, main=main, ops=ops)


def fwd_planes(L, q, k, v, ext, heads, n_q):
    """wmz_local3d_attn_fwd_planes (the cone's entry point): the last n_q query planes only, compact output."""
    B, S, H, W, I = q.shape
    out = torch.empty((B, n_q, H, W, I), dtype=q.dtype, device=q.device)
    L.call('wmz_local3d_attn_fwd_planes', L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(out), None, B, S, H, W, heads, I // heads,
           int(ext[0]), int(ext[1]), int(ext[2]), I, I, I, I, S - n_q, n_q, L.dtype_code(q.dtype), L.stream())
    return out


@pytest.mark.parametrize('shape,heads,dh,ext', CASES)
def test_attention_32_wide_planes_fast_path(wmz, shape, heads, dh, ext):
    """bf16: the kernel's own logits dump against the fp32 oracle on the same bf16 inputs (<= 1e-3, masked slots the literal -1e9
    in exactly the oracle's places), the un-probed instantiation bit-equal to the probed one, lse, out, and the general kernel."""
    ops = wmz['ops']
    torch.manual_seed(29)
    B, S, H, W = shape
    I = heads * dh
    q, k, v = (torch.randn(B, S, H, W, I).bfloat16() for _ in range(3))
    ref, ref_logits = oat.local_attention(k.float(), v.float(), q.float(), ext, heads, return_logits=True)
    fast, lse_f, dbg = ops.local3d_attention_fwd(q.cuda(), k.cuda(), v.cuda(), ext, heads, need_lse=True, logits_dbg=True)
    plain, _, _ = ops.local3d_attention_fwd(q.cuda(), k.cuda(), v.cuda(), ext, heads)
    gen, lse_g, _ = ops.local3d_attention_fwd(q.cuda(), k.cuda(), v.cuda(), ext, heads, need_lse=True, general=True)
    assert torch.equal(fast, plain)
    logits = dbg.cpu().reshape(ref_logits.shape)
    live = ref_logits != -1e9
    assert torch.equal(logits == -1e9, ~live)
    err = float((logits[live] - ref_logits[live]).abs().max() / ref_logits[live].abs().max())
    assert err < 1e-3 and rel(logits[live], ref_logits[live]) < 1e-3, err
    e_out, e_gen = rel(fast, ref), rel(fast, gen)
    print(f'[32-wide {shape} {ext}] logits max err {err:.1e}, out vs oracle {e_out:.2e}, vs general kernel {e_gen:.2e}')
    assert e_out < 3e-3 and e_gen < 3e-3
    lse_ref = torch.logsumexp(ref_logits, -1).reshape(-1, heads)
    assert torch.allclose(lse_f.cpu(), lse_ref, rtol=1e-4, atol=1e-4)
    assert torch.allclose(lse_f.cpu(), lse_g.cpu(), rtol=1e-5, atol=2e-5)
    if S > 1:                                                              # the cone's entry point: the full grid's last plane, bit for bit
        assert torch.equal(fwd_planes(wmz['lib'], q.cuda(), k.cuda(), v.cuda(), ext, heads, 1), fast[:, S - 1:])


@pytest.mark.parametrize('shape,heads,dh,ext', CASES)
def test_half_attention_32_wide_logits_and_output_vs_oracle(wmz, shape, heads, dh, ext):
    """dtype WMZ_F16 on 32-wide planes: the scaled logits of every in-window slot and the attention output within 1e-3 of the fp32
    oracle fed the SAME un-rounded fp32 q, k, v; the un-probed form and the trailing-planes entry point bit-equal to the probed
    full grid."""
    ops = wmz['ops']
    torch.manual_seed(7)
    B, S, H, W = shape
    I = heads * dh
    q, k, v = (torch.randn(B, S, H, W, I) for _ in range(3))
    ref_out, ref_logits = oat.local_attention(k, v, q, ext, heads, return_logits=True)
    qh, kh, vh = (t.cuda().half() for t in (q, k, v))
    out, _, logits = ops.local3d_attention_fwd(qh, kh, vh, ext, heads, logits_dbg=True)
    plain, _, _ = ops.local3d_attention_fwd(qh, kh, vh, ext, heads)
    assert out.dtype == torch.float16 and torch.equal(out, plain)
    logits = logits.cpu().reshape(ref_logits.shape)
    inside = ref_logits > -1e8
    assert torch.equal(logits == -1e9, ~inside)                         # the same slots are masked, with the literal
    e_log = float((logits[inside] - ref_logits[inside]).norm() / ref_logits[inside].norm())
    e_out = rel(out.reshape(ref_out.shape), ref_out)
    print(f'half attention {shape} heads {heads} dh {dh}: logits rel {e_log:.2e}, out rel {e_out:.2e}')
    assert e_log < 1e-3 and e_out < 1e-3, (e_log, e_out)
    n_q = max(S - 1, 1)
    assert torch.equal(fwd_planes(wmz['lib'], qh, kh, vh, ext, heads, n_q), out[:, S - n_q:])


def test_default_denoiser_on_32_wide_planes_precise_and_bf16(wmz):
    """The default denoiser (dim 256, dh 128, depth 4) on (3, 4, 32) clips.  Precise mode: logits within 1e-3 of the fp32 oracle,
    on the fused half kernels (it ran the fp32 route on such planes before), the last-frame cone bit-equal to the full grid.
    bf16: inside the default model's bar (tests/test_modules_gpu.py: 1e-2)."""
    from conftest import recorded_calls
    cfg = wmz['config']
    torch.manual_seed(42)
    m = wmz['main'].VqVideoDiffusionModel(data_shape=(3, 4, 32), dim=256, num_classes=1024, extents=(1, 1, 1), depth=4,
                                          dim_head=128, mlp_dim=256, heads=1)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    z = torch.randint(0, 1025, (2, 3, 4, 32))
    ref = oden.denoiser_forward(sd, z, (1, 1, 1), 1)
    m = m.cuda()
    with torch.no_grad():
        with cfg.compute_dtype(torch.float16), recorded_calls() as seen:
            y_p = m(z.cuda())
            cfg.set_last_frame_cone(False)
            try:
                y_full = m(z.cuda())
            finally:
                cfg.set_last_frame_cone(True)
        with cfg.compute_dtype(torch.bfloat16):
            y_b = m(z.cuda())
    e_p, e_b = rel(y_p, ref), rel(y_b, ref)
    print(f'32-wide planes, default denoiser: precise mode {e_p:.3e}, bf16 {e_b:.3e} from the fp32 oracle')
    assert e_p < 1e-3, e_p
    assert 'wmz_layer_fused_fwd_planes_f16' in seen and 'wmz_embed_qkv_fused_fwd_planes_f16' in seen, set(seen)
    assert y_p.dtype == torch.float32 and torch.equal(y_p, y_full)
    assert e_b < 1e-2, e_b


# ---------------------------------------------------------------------------------------------------------------- backward

def grads(ops, q, k, v, do, ext, heads, general=False):
    """dq, dk, dv of the bf16 kernels (forward for out / lse on the same route)."""
    I = q.shape[-1]
    qd, kd, vd, dod = (t.cuda() for t in (q, k, v, do))
    out, lse, _ = ops.local3d_attention_fwd(qd, kd, vd, ext, heads, need_lse=True, general=general)
    dq, dkv = ops.local3d_attention_bwd(qd, kd, vd, out, lse, dod, ext, heads, general=general)
    return dq.float().cpu(), dkv[..., :I].float().cpu(), dkv[..., I:].float().cpu()


def oracle_grads(q, k, v, do, ext, heads):
    qr, kr, vr = (t.float().clone().requires_grad_(True) for t in (q, k, v))
    oat.local_attention(kr, vr, qr, ext, heads).backward(do.float())
    return qr.grad, kr.grad, vr.grad


def worst_row(a, ref):
    """Largest relative error of one token's gradient row (all heads)."""
    a, ref = a.reshape(-1, a.shape[-1]), ref.reshape(-1, ref.shape[-1])
    return float(((a - ref).norm(dim=1) / (ref.norm(dim=1) + 1e-30)).max())


@pytest.mark.parametrize('shape,heads,dh,ext', CASES)
def test_attention_backward_32_wide_planes(wmz, shape, heads, dh, ext):
    """bf16, W == 32: the row kernels of attn_bwd_row16.hip in their 32-wide mode against torch.autograd over the oracle -- dq, dk,
    dv at 2e-2 (P and dS are bf16 MFMA operands) -- and against the general kernels.  One norm can hide a seam bug (seam pairs are
    few), so per token row as well: the worst row's relative error may be at most twice what the general bf16 kernels show on the
    same inputs against the same oracle (both round P and dS to bf16; they differ in summation order only)."""
    torch.manual_seed(33)
    ops = wmz['ops']
    B, S, H, W = shape
    I = heads * dh
    q, k, v, do = (torch.randn(B, S, H, W, I).bfloat16() for _ in range(4))
    ref = oracle_grads(q, k, v, do, ext, heads)
    row = grads(ops, q, k, v, do, ext, heads)
    gen = grads(ops, q, k, v, do, ext, heads, general=True)
    e = [rel(a, r) for a, r in zip(row, ref)]
    eg = [rel(a, g) for a, g in zip(row, gen)]
    wr = [worst_row(a, r) for a, r in zip(row, ref)]
    wg = [worst_row(a, r) for a, r in zip(gen, ref)]
    print(f'[32-wide bwd {shape} {ext}] dq dk dv vs oracle {e[0]:.2e} {e[1]:.2e} {e[2]:.2e}, vs general {eg[0]:.2e} {eg[1]:.2e} {eg[2]:.2e}; '
          f'worst row: row kernels {wr[0]:.2e} {wr[1]:.2e} {wr[2]:.2e}, general kernels {wg[0]:.2e} {wg[1]:.2e} {wg[2]:.2e}')
    assert max(e) < 2e-2 and max(eg) < 2e-2, (e, eg)
    for name, a, b in zip(('dq', 'dk', 'dv'), wr, wg):
        assert a <= 2.0 * b, (name, a, b)


@pytest.mark.parametrize('shape,heads,dh,ext', [
    pytest.param((1, 2, 3, 32), 1, 64, (1, 1, 3), id='small-ragged-64-seam-3'),
    pytest.param((1, 1, 9, 32), 1, 128, (0, 2, 17), id='big-ragged-128-seam-17'),
    pytest.param((1, 2, 8, 32), 2, 32, (1, 1, 1), id='big-aligned-32-seam-1'),
])
def test_attention_backward_32_wide_support_probes(wmz, shape, heads, dh, ext):
    """Where a gradient may be non-zero.  dO non-zero at ONE query: the dk and dv rows are exactly zero outside that query's
    window and non-zero inside it.  K non-zero at ONE key: the dq rows are exactly zero for queries that do not see the key and
    non-zero for those that do.  Probes next to the seam on both sides, at the plane's corners and in its middle; each compared
    element-wise with the oracle's autograd as well (2e-2 of the largest element: the gradient bar, per element)."""
    torch.manual_seed(35)
    ops = wmz['ops']
    B, S, H, W = shape
    I = heads * dh
    eS, eH, eW = ext
    q, k, v, do = (torch.randn(B, S, H, W, I).bfloat16() for _ in range(4))
    ss, hh, ww = torch.meshgrid(torch.arange(S), torch.arange(H), torch.arange(W), indexing='ij')
    for s, h, w in [(S - 1, H // 2, 15), (0, H // 2, 16), (0, 0, 0), (S - 1, H - 1, 31), (0, H // 2, 8), (S - 1, 0, 17), (0, H - 1, 14)]:
        window = ((ss - s).abs() <= eS) & ((hh - h).abs() <= eH) & ((ww - w).abs() <= eW)          # symmetric: sees / is seen by
        one_do = torch.zeros_like(do)
        one_do[0, s, h, w] = do[0, s, h, w]
        _, dk, dv = grads(ops, q, k, v, one_do, ext, heads)
        _, dk_ref, dv_ref = oracle_grads(q, k, v, one_do, ext, heads)
        for name, g, ref in (('dk', dk, dk_ref), ('dv', dv, dv_ref)):
            live = (g[0] != 0).any(-1)
            assert torch.equal(live, window), (name, (s, h, w), (live != window).nonzero()[:4])
            assert float((g - ref).abs().max()) <= 2e-2 * float(ref.abs().max()), (name, (s, h, w))
        one_k = torch.zeros_like(k)
        one_k[0, s, h, w] = k[0, s, h, w]
        dq, _, _ = grads(ops, q, one_k, v, do, ext, heads)
        dq_ref, _, _ = oracle_grads(q, one_k, v, do, ext, heads)
        live = (dq[0] != 0).any(-1)
        assert torch.equal(live, window), ('dq', (s, h, w), (live != window).nonzero()[:4])
        assert float((dq - dq_ref).abs().max()) <= 2e-2 * float(dq_ref.abs().max()), ('dq', (s, h, w))


def test_default_denoiser_training_step_on_32_wide_planes(wmz):
    """One bf16 DenoiserTrainer step of the default denoiser (depth 2) on (3, 4, 32) clips -- attention forward and backward on the
    row kernels' 32-wide mode -- against the oracle's autograd at the bf16 bars of the default model (loss 2e-2, gradients 6e-2)."""
    from oracle import train_step as ots
    from world_modelz_amd import train
    torch.manual_seed(42)
    C = 64
    m = wmz['main'].VqVideoDiffusionModel(data_shape=(3, 4, 32), dim=256, num_classes=C, extents=(1, 1, 1), depth=2, dim_head=128,
                                          mlp_dim=256, heads=1)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    z = torch.randint(0, C + 1, (2, 3, 4, 32))
    target = torch.randint(0, C, (2, 4, 32))
    _, _, loss_ref, grads_ref = ots.step_grads(sd, z, target, (1, 1, 1), 1)
    m = m.cuda()
    with wmz['config'].compute_dtype(torch.bfloat16):
        tr = train.DenoiserTrainer(m, C, lr=1e-3, warmup=0, max_steps=100, distributed=False)
        tr.arena.zero_grad()
        _, mean = tr.forward_backward(z.cuda(), target.cuda())
    worst = max((rel(p.grad, grads_ref[n]), n) for n, p in m.named_parameters())
    print(f'32-wide planes, bf16 training step: loss diff {abs(float(mean) - float(loss_ref)):.1e}, worst gradient {worst[0]:.2e} ({worst[1]})')
    assert abs(float(mean) - float(loss_ref)) < 2e-2
    assert worst[0] < 6e-2, worst
