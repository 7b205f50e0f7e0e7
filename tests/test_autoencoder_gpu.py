"""GPU parity of the conv encoder / decoder / VqAutoEncoder drop-ins against the reference captures
(tests/golden/ae_roundtrip.npz, ae_cfg1_meta.npz) and the oracle."""
import pytest
import torch

from conftest import load_golden, near_tie_mismatches, recorded_calls, sub

pytestmark = pytest.mark.gpu

from oracle import autoencoder as oae        # noqa: E402


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(scope='module')
def wmz():
    assert torch.cuda.is_available()
    from world_modelz_amd import config, ops, train_vqae
    return dict(config=config, ops=ops, tv=train_vqae)


def _model(wmz, sd):
    m = wmz['tv'].VqAutoEncoder(embedding_dim=16, num_embeddings=32, downscale_steps=2, hidden_planes=24, in_channels=3)
    m.load_state_dict(sd, strict=True)                        # reference state_dict loads key-for-key
    return m.cuda()


def test_conv_kernel_vs_torch(wmz):
    ops = wmz['ops']
    torch.manual_seed(0)
    for (B, H, W, Ci, Co, k, s, p) in [(2, 9, 11, 8, 40, 3, 1, 1), (1, 16, 16, 24, 16, 3, 2, 1), (3, 8, 8, 16, 130, 1, 1, 0),
                                       (2, 10, 6, 8, 8, 2, 2, 0)]:
        x = torch.randn(B, Ci, H, W)
        w = torch.randn(Co, Ci, k, k) / (Ci * k * k) ** 0.5
        b = torch.randn(Co)
        ref = torch.nn.functional.conv2d(x, w, b, stride=s, padding=p)
        xn = x.permute(0, 2, 3, 1).contiguous().cuda()
        wop = w.permute(0, 2, 3, 1).reshape(Co, -1).contiguous().cuda()
        out, s1, s2 = ops.conv2d_nhwc(xn, wop, k, k, s, p, bias=b.cuda(), stats=True)
        assert rel(out.permute(0, 3, 1, 2), ref) < 2e-6
        assert torch.allclose(s1.sum(0).cpu(), ref.sum(dim=(0, 2, 3)), rtol=1e-4, atol=1e-4)      # [replicas, C] partial sums
        assert torch.allclose(s2.sum(0).cpu(), (ref ** 2).sum(dim=(0, 2, 3)), rtol=1e-4, atol=1e-4)
        outb = ops.conv2d_nhwc(xn.bfloat16(), wop.bfloat16(), k, k, s, p, bias=b.cuda(), leaky=True)
        refb = torch.nn.functional.leaky_relu(torch.nn.functional.conv2d(x.bfloat16().float(), w.bfloat16().float(), b,
                                                                         stride=s, padding=p), 0.01)
        assert rel(outb.permute(0, 3, 1, 2), refb) < 6e-3


def test_bilinear_and_affine(wmz):
    ops = wmz['ops']
    torch.manual_seed(1)
    x = torch.randn(2, 8, 5, 7)
    ref = torch.nn.functional.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False)
    y = ops.bilinear2x_nhwc(x.permute(0, 2, 3, 1).contiguous().cuda())
    assert rel(y.permute(0, 3, 1, 2), ref) < 1e-6
    a, b = torch.randn(3, 4, 4, 8), torch.randn(3, 4, 4, 8)
    sa, ta, sb, tb = (torch.randn(8) for _ in range(4))
    ref = torch.nn.functional.leaky_relu(a * sa + ta + b * sb + tb, 0.01)
    y = ops.affine_act_nhwc(a.cuda(), sa.cuda(), ta.cuda(), b.cuda(), sb.cuda(), tb.cuda(), leaky=True)
    assert rel(y, ref) < 1e-6


def test_autoencoder_eval_vs_golden(wmz):
    g = load_golden('ae_roundtrip')
    m = _model(wmz, sub(g, 'sd0/'))
    m.eval()
    x = g['x'].cuda()
    with wmz['config'].compute_dtype(torch.float32), torch.no_grad():
        h = m.encoder(x)
        idx = m.encode(x)
        rec = m.decode(g['eval/idx'].cuda())
        out, ll, ppl = m(x)
    assert h.shape == g['eval/enc_out'].shape and rel(h, g['eval/enc_out']) < 1e-5
    assert idx.dtype == torch.int64 and idx.shape == g['eval/idx'].shape
    # indices bit-identical to the reference except at genuine near-ties of the ORACLE's distances (the argmin kernel is
    # bit-exact on equal inputs; the conv encoder in front of it differs from ATen's in the last bits)
    near_tie_mismatches(idx, g['eval/idx'], g['eval/enc_out'].permute(0, 2, 3, 1), g['sd0/vq.embedding'][0])
    assert rel(rec, g['eval/decoded']) < 1e-5
    if torch.equal(idx.cpu(), g['eval/idx']):
        assert rel(out, g['eval/recon']) < 1e-5
        assert torch.allclose(ll.cpu(), g['eval/latent_loss'], rtol=1e-4)
        assert torch.allclose(ppl.cpu(), g['eval/perplexity'], rtol=1e-4)


def test_autoencoder_train_mode_bn_vs_golden(wmz):
    """Quirk Q3: the frozen AE is never .eval()-ed in main.py, so BatchNorm uses batch statistics and updates its
    running statistics even under no_grad.  Indices and the mutated state_dict against the reference capture."""
    g = load_golden('ae_roundtrip')
    m = _model(wmz, sub(g, 'sd0/'))
    m.train()
    with wmz['config'].compute_dtype(torch.float32), torch.no_grad():
        idx = m.encode(g['x'].cuda())
    lat_ref = oae.encoder_forward({k: v.clone() for k, v in sub(g, 'sd0/').items()}, g['x'], training=True)
    near_tie_mismatches(idx, g['train/idx'], lat_ref.permute(0, 2, 3, 1), g['sd0/vq.embedding'][0])
    assert not torch.equal(idx.cpu(), g['eval/idx'])
    sd1 = sub(g, 'sd1/')
    for k, v in m.state_dict().items():
        if k.startswith('encoder.') and v.dtype.is_floating_point:
            assert torch.allclose(v.cpu(), sd1[k], rtol=1e-4, atol=1e-5), k
        elif k.startswith('encoder.'):
            assert torch.equal(v.cpu(), sd1[k]), k
    # full forward in train mode: recon against the oracle fed with the SAME state (decoder BN batch statistics)
    m2 = _model(wmz, sub(g, 'sd1/'))
    m2.train()
    p = oae.with_vq_stats({k: v.clone() for k, v in sub(g, 'sd1/').items()})
    rec_ref, ll_ref, _ = oae.vqae_forward(p, g['x'], training=True)
    with wmz['config'].compute_dtype(torch.float32), torch.no_grad():
        rec, ll, _ = m2(g['x'].cuda())
    assert rel(rec, rec_ref) < 2e-3          # a flipped index moves one 4x4 patch; most runs are ~1e-6
    assert abs(float(ll) - float(ll_ref)) < 1e-3


def test_config1_frame_roundtrip(wmz):
    """BASELINE.json configs[0]: encode -> quantize -> decode one 64x64 RGB frame, codebook 512, default sizes.
    The model is re-created from the reference's seed: same construction order => same initial weights."""
    g = load_golden('ae_cfg1_meta')
    torch.manual_seed(int(g['seed']))
    m = wmz['tv'].VqAutoEncoder(embedding_dim=64, num_embeddings=512, downscale_steps=3, hidden_planes=128, in_channels=3)
    m = m.cuda().eval()
    with wmz['config'].compute_dtype(torch.float32), torch.no_grad():
        idx = m.encode(g['x'].cuda())
        rec = m.decode(g['idx'].cuda())
    assert idx.shape == (1, 8, 8)
    sd_cpu = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    lat_ref = oae.encoder_forward(sd_cpu, g['x'], training=False)
    near_tie_mismatches(idx, g['idx'], lat_ref.permute(0, 2, 3, 1), sd_cpu['vq.embedding'][0])
    assert rec.shape == (1, 3, 64, 64)
    assert torch.allclose(rec[0, :, :4, :4].cpu(), g['recon_corner'], rtol=1e-4, atol=1e-5)
    assert abs(float(rec.mean()) - float(g['recon_mean'])) < 1e-5
    with wmz['config'].compute_dtype(torch.bfloat16), torch.no_grad():
        rec16 = m.decode(g['idx'].cuda())
    assert rel(rec16, rec) < 3e-2


def test_conv_backward_kernels_vs_torch(wmz):
    """dgrad (flipped-weight conv on the dilated gradient) and implicit-im2col wgrad against torch.autograd."""
    from world_modelz_amd import autoencoder as ae
    torch.manual_seed(2)
    for (B, H, W, Ci, Co, k, s, p, bias) in [(2, 9, 11, 8, 40, 3, 1, 1, True), (1, 16, 16, 24, 16, 3, 2, 1, False),
                                             (2, 8, 8, 16, 136, 1, 1, 0, True), (2, 10, 6, 8, 8, 2, 2, 0, False),
                                             (1, 8, 8, 3, 16, 3, 1, 1, False), (1, 8, 8, 16, 3, 3, 1, 1, False)]:
        conv = torch.nn.Conv2d(Ci, Co, k, stride=s, padding=p, bias=bias)
        x = torch.randn(B, Ci, H, W, requires_grad=True)
        y = conv(x)
        w_out = torch.randn_like(y)
        (y * w_out).sum().backward()
        conv_g = torch.nn.Conv2d(Ci, Co, k, stride=s, padding=p, bias=bias).cuda()
        conv_g.load_state_dict(conv.state_dict())
        xg = x.detach().cuda().requires_grad_(True)
        with wmz['config'].compute_dtype(torch.float32):
            xn = ae._to_nhwc(xg, torch.float32)
            yg = ae._conv_g(xn, conv_g)
            assert rel(yg.permute(0, 3, 1, 2), y) < 2e-6
            (yg * w_out.permute(0, 2, 3, 1).cuda()).sum().backward()
        assert rel(xg.grad, x.grad) < 5e-6, (k, s)
        assert rel(conv_g.weight.grad, conv.weight.grad) < 5e-6, (k, s)
        if bias:
            assert rel(conv_g.bias.grad, conv.bias.grad) < 5e-6


def test_bn_and_bilinear_backward_vs_torch(wmz):
    from world_modelz_amd import autoencoder as ae
    torch.manual_seed(3)
    x = torch.randn(3, 16, 6, 5, requires_grad=True)
    r = torch.randn(3, 16, 6, 5, requires_grad=True)
    bn = torch.nn.BatchNorm2d(16)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.3, 0.3)
    y = torch.nn.functional.leaky_relu(bn(x) + r, 0.01)
    up = torch.nn.functional.interpolate(y, scale_factor=2, mode='bilinear', align_corners=False)
    w = torch.randn_like(up)
    (up * w).sum().backward()
    bn_g = torch.nn.BatchNorm2d(16).cuda()
    with torch.no_grad():
        bn_g.weight.copy_(bn.weight)
        bn_g.bias.copy_(bn.bias)
    xg = x.detach().permute(0, 2, 3, 1).contiguous().cuda().requires_grad_(True)
    rg = r.detach().permute(0, 2, 3, 1).contiguous().cuda().requires_grad_(True)
    yg = ae._bnact_g(xg, bn_g, r=rg)
    upg = ae._Bilinear2xFn.apply(yg)
    assert rel(upg.permute(0, 3, 1, 2), up) < 2e-6
    (upg * w.permute(0, 2, 3, 1).cuda()).sum().backward()
    assert rel(xg.grad.permute(0, 3, 1, 2), x.grad) < 1e-5
    assert rel(rg.grad.permute(0, 3, 1, 2), r.grad) < 1e-5
    assert rel(bn_g.weight.grad, bn.weight.grad) < 1e-5
    assert rel(bn_g.bias.grad, bn.bias.grad) < 1e-5
    assert torch.allclose(bn_g.running_var.cpu(), bn.running_var, rtol=1e-5)


def test_vqae_training_step_grads_vs_golden(wmz):
    """VqAutoEncoder.forward in .train() with gradients (train_vqae.py:145-151): recon, latent loss and every
    parameter gradient against the reference capture.  A code index flipped by last-bit differences of the latents
    would move a handful of gradients, so the index agreement is asserted first."""
    g = load_golden('ae_roundtrip')
    m = _model(wmz, sub(g, 'sd1/'))
    m.train()
    x = g['x'].cuda().requires_grad_(True)
    with wmz['config'].compute_dtype(torch.float32):
        with torch.no_grad():
            m_probe = _model(wmz, sub(g, 'sd1/'))
            m_probe.train()
            idx = m_probe.encode(g['x'].cuda())
        out, ll, ppl = m(x)
        loss = torch.nn.functional.smooth_l1_loss(out, g['x'].cuda()) + 0.25 * ll
        loss.backward()
    ref = {'recon': g['train/recon'], 'loss': g['train/loss'], 'dx': g['train/dx'],
           'grad': {n: g['train/grad/' + n] for n, _ in m.named_parameters()}}
    if not torch.equal(idx.cpu(), g['train/idx']):
        # a code index flipped on last-bit latent differences: it has to be a genuine near-tie of the oracle's distances (this
        # FAILS otherwise), and the comparison then runs against the oracle's autograd on the SAME assignment (oracle.vq.forward's
        # test knob) instead of the capture -- never a skip
        sd1 = sub(g, 'sd1/')
        lat_ref = oae.encoder_forward({k: v.clone() for k, v in sd1.items()}, g['x'], training=True)
        near_tie_mismatches(idx, g['train/idx'], lat_ref.permute(0, 2, 3, 1), sd1['vq.embedding'][0])
        leaves = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and 'running' not in k and not k.startswith('vq.')
                      else v.clone()) for k, v in sd1.items()}
        xo = g['x'].clone().requires_grad_(True)
        rec_o, ll_o, _ = oae.vqae_forward(oae.with_vq_stats(leaves), xo, training=True, assign=idx.cpu().reshape(-1, 1))
        lo = torch.nn.functional.smooth_l1_loss(rec_o, g['x']) + 0.25 * ll_o
        lo.backward()
        ref = {'recon': rec_o.detach(), 'loss': lo.detach(), 'dx': xo.grad, 'grad': {n: leaves[n].grad for n, _ in m.named_parameters()}}
    assert rel(out, ref['recon']) < 1e-4
    assert abs(float(loss) - float(ref['loss'])) < 1e-5
    assert rel(x.grad, ref['dx']) < 2e-4
    # a bias in front of a training-mode BatchNorm has an exactly-zero true gradient (the reference holds 1e-9 noise
    # there): measure errors against the typical gradient magnitude, not against that noise
    floor = 1e-3 * max(float(ref['grad'][n].norm()) for n, _ in m.named_parameters())

    def err(a, b):
        a, b = a.detach().float().cpu(), b.float()
        return float((a - b).norm() / max(float(b.norm()), floor))
    worst = max((err(p.grad, ref['grad'][n]), n) for n, p in m.named_parameters())
    assert worst[0] < 5e-4, worst


def test_eval_mode_backward_vs_oracle_autograd(wmz):
    """Gradients THROUGH an evaluated encoder / decoder (eval-mode BatchNorm = the affine map of its running statistics; round 4:
    used to raise): input gradient and every parameter gradient, BatchNorm gamma / beta included, against torch.autograd over the
    oracle with training=False.  sd1 = the state after a training step, so the running statistics are not the initial 0 / 1."""
    from oracle import autoencoder as oae
    g = load_golden('ae_roundtrip')
    sd = sub(g, 'sd1/')
    m = _model(wmz, sd)
    m.eval()
    torch.manual_seed(9)
    xin = g['x'].clone()
    zin = torch.randn(xin.shape[0], 16, xin.shape[2] // 4, xin.shape[3] // 4)
    leaves = {k: (v.clone().float().requires_grad_(True) if v.is_floating_point() and 'running' not in k and not k.startswith('vq.')
                  else v.clone()) for k, v in sd.items()}
    with wmz['config'].compute_dtype(torch.float32):
        for name, mod, fwd, inp in (('encoder', m.encoder, oae.encoder_forward, xin), ('decoder', m.decoder, oae.decoder_forward, zin)):
            xd = inp.cuda().requires_grad_(True)
            y = mod(xd)
            xo = inp.clone().requires_grad_(True)
            yo = fwd(leaves, xo, False)
            assert y.shape == yo.shape and rel(y, yo) < 1e-5, name
            w = torch.randn_like(yo)
            (y * w.cuda()).sum().backward()
            (yo * w).sum().backward()
            assert rel(xd.grad, xo.grad) < 1e-4, name
            for n, p in mod.named_parameters():
                ref = leaves[f'{name}.{n}'].grad
                assert p.grad is not None and rel(p.grad, ref) < 2e-4, (name, n)
    # the running statistics did not move
    for n, b in m.named_buffers():
        if 'running' in n:
            assert torch.equal(b.cpu(), sd[n]), n


@pytest.mark.parametrize('dtype,tol', [(torch.float32, 1e-5), (torch.bfloat16, 2e-2)])
def test_conv1x1_input_prologue(dtype, tol):
    """wmz_conv2d_nhwc_fwd_pre: LeakyReLU(x * scale[c] + shift[c]) applied while the 1x1 conv stages its operand, against
    the two-pass formulation (affine_act then conv) and torch; ragged pixel count, channel counts off the tile sizes."""
    from world_modelz_amd import ops
    torch.manual_seed(23)
    B, H, W, Cin, Cout = 3, 7, 5, 136, 72
    x = torch.randn(B, H, W, Cin, device='cuda')
    w = torch.randn(Cout, Cin, device='cuda') * 0.1
    sc = torch.rand(Cin, device='cuda') + 0.5
    sh = torch.randn(Cin, device='cuda') * 0.3
    ref = torch.nn.functional.leaky_relu(x * sc + sh, 0.01) @ w.t()
    xd, wd = x.to(dtype).contiguous(), w.to(dtype).contiguous()
    fused, s1, q1 = ops.conv2d_nhwc(xd, wd, 1, 1, 1, 0, stats=True, pre=(sc, sh, 0.01))
    two = ops.conv2d_nhwc(ops.affine_act_nhwc(xd, sc, sh, leaky=True, slope=0.01), wd, 1, 1, 1, 0)
    err = float((fused.float() - ref).norm() / ref.norm())
    assert err < tol, err
    assert float((fused.float() - two.float()).norm() / ref.norm()) < tol
    assert torch.allclose(s1.sum(0), fused.float().sum(dim=(0, 1, 2)), rtol=2e-3, atol=2e-2)


def test_vqae_trainer_step_matches_torch_adamw_and_revives_dead_codes(wmz):
    """VqaeTrainer (train_vqae.py:125-164): one fp32 step from the reference capture's state == the captured gradients fed to
    torch.optim.AdamW (lr 2e-4, weight decay 0); the StepLR epoch schedule; reuse_inactive + reset_stats on the interval."""
    from world_modelz_amd import train
    g = load_golden('ae_roundtrip')
    m = _model(wmz, sub(g, 'sd1/'))
    with wmz['config'].compute_dtype(torch.float32):
        tr = train.VqaeTrainer(m, lr=2e-4, loss_fn='SmoothL1', latent_loss_weight=0.25, vq_reuse_interval=2, steps_per_epoch=1,
                               distributed=False)
        before = {n: p.detach().clone() for n, p in m.named_parameters()}
        loss, r_loss, l_loss, ppl = tr.train_step(g['x'].cuda())
    if abs(loss - float(g['train/loss'])) < 1e-5:              # no VQ index flipped at a near-tie
        ref = {n: before[n].cpu().clone().requires_grad_(True) for n in before}
        for n in ref:
            ref[n].grad = g['train/grad/' + n].clone()
        torch.optim.AdamW(list(ref.values()), lr=2e-4, betas=(0.9, 0.999), weight_decay=0.0).step()
        # a bias in front of a training-mode BatchNorm has an exactly-zero true gradient; the reference holds 1e-9 noise
        # there, whose SIGN Adam's first step turns into a full lr-sized move: those parameters are not comparable
        floor = 1e-4 * max(float(g['train/grad/' + n].abs().max()) for n in before)
        for n, p in m.named_parameters():
            if float(g['train/grad/' + n].abs().max()) < floor:
                continue
            assert torch.allclose(p.detach().cpu(), ref[n].detach(), rtol=1e-4, atol=3e-6), n
    assert tr.lr_now() == 2e-4
    with wmz['config'].compute_dtype(torch.float32):
        m.vq.activation_count[0, :5] = 0                         # pretend five codes were never used since the last reset
        tr.train_step(g['x'].cuda())                              # step 2: interval hit
    assert tr.step_count == 2 and float(m.vq.activation_count.sum()) == 0 and float(m.vq.accumulated_error.sum()) == 0
    tr.step_count = 7
    assert abs(tr.lr_now() - 2e-4 * 0.25) < 1e-12               # epoch 7 // 3 = 2 halvings
    with pytest.raises(RuntimeError):
        train.VqaeTrainer(m, loss_fn='Huber')


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_vqae_graphed_training_step_matches_eager(wmz, dtype):
    """VqaeTrainer.enable_graph: the whole VQ-AE training step (encoder, VectorQuantizerEMA with its in-place EMA update, decoder,
    losses, backward, AdamW) as ONE hipGraph.  The step has no randomness, so a graphed and an eager trainer started from the
    same weights and fed the same batches walk the same trajectory: losses, codebook, every weight; the dead-code revival on
    its interval still runs (between replays)."""
    from world_modelz_amd import train
    from world_modelz_amd.train_vqae import VqAutoEncoder
    def make():
        torch.manual_seed(31)
        return VqAutoEncoder(embedding_dim=64, num_embeddings=128, downscale_steps=2, hidden_planes=32).cuda()
    torch.manual_seed(32)
    batches = [torch.rand(8, 3, 32, 32, device='cuda') for _ in range(5)]
    with wmz['config'].compute_dtype(dtype):
        me, mg = make(), make()
        mg.load_state_dict(me.state_dict())
        te = train.VqaeTrainer(me, lr=2e-4, vq_reuse_interval=4, distributed=False)
        tg = train.VqaeTrainer(mg, lr=2e-4, vq_reuse_interval=4, distributed=False)
        tg.enable_graph(batches[0], warmup=2)
        assert tg.step_count == 2                               # the graph's warm-up steps are real steps
        # ONE step from identical state: the eager trainer takes over the graphed one's weights, moments, BatchNorm and VQ buffers
        def sync_state():
            me.load_state_dict(mg.state_dict())
            me.vq.activation_count.copy_(mg.vq.activation_count); me.vq.accumulated_error.copy_(mg.vq.accumulated_error)
            te.m.copy_(tg.m); te.v.copy_(tg.v); te.step_count = tg.step_count
            from world_modelz_amd import _cast
            _cast.invalidate()
        tol = 1e-4 if dtype == torch.float32 else 1e-2
        for b in batches[:3]:
            sync_state()
            le = te.train_step(b)
            lg = tg.train_step(b)
            for k_, (a_, b_) in enumerate(zip(le, lg)):
                # (bf16: the perplexity is a statistic of the code assignments, which near-ties move: 5 %)
                tk = 5e-2 if (k_ == 3 and dtype != torch.float32) else tol
                assert abs(a_ - b_) <= tk * max(1.0, abs(a_)), (le, lg)
            ptol = dict(rtol=0, atol=2.5 * 2e-4 + (0 if dtype == torch.float32 else 1e-2))      # (Adam: a sign flip of a ~0 gradient = 2 lr)
            for (n, a_), b_ in zip(me.named_parameters(), mg.parameters()):
                assert torch.allclose(a_, b_, **ptol), n
            if dtype == torch.float32:
                assert torch.allclose(me.vq.embedding, mg.vq.embedding, rtol=1e-4, atol=1e-5)
                assert torch.equal(me.vq.activation_count, mg.vq.activation_count)
            else:                               # bf16 activations: a latent at a near-tie may pick the other code in one of the runs
                # (a rarely used code's EMA mean moves a lot when one latent changes sides: bound the NUMBER of codes that moved)
                moved = ((me.vq.embedding - mg.vq.embedding).abs().amax(dim=-1) > 0.1).sum()
                # (0-13 of 128 over ~80 runs: the count depends on which near-ties the run's atomically summed BatchNorm statistics
                #  tip -- 15 % leaves that noise room; the fp32 branch above is exact.  NOT on a step that ended with the dead-code
                #  revival (step_count % 4 == 0): it re-seeds every dead code -- ~50 of these 128 -- from the latents ranked by their
                #  accumulated error, and one near-tie in that ranking re-seeds them all differently: 51 moved, 1 run in 36,
                #  with and without this round's changes)
                if tg.step_count % 4 != 0:
                    assert int(moved) <= 0.15 * me.vq.embedding.shape[-2], int(moved)
                assert float((me.vq.activation_count - mg.vq.activation_count).abs().sum()) <= 0.05 * 8 * 64 * 2
        # ... and on: the interval-4 dead-code revival runs between replays; the loss stays finite and falls on a repeated batch
        hist = [tg.train_step(batches[0])[0] for _ in range(8)]
        assert tg.step_count == 13 and all(v == v for v in hist) and hist[-1] < hist[0]
        assert float(mg.vq.activation_count.sum()) <= 8 * 64    # reset at step 12, one batch counted since
        # another batch shape falls back to eager launches
        out = tg.train_step(torch.rand(4, 3, 32, 32, device='cuda'))
        assert len(out) == 4 and all(v == v for v in out)


@pytest.mark.parametrize('geom', [(3, 16, 64, 64, 128), (2, 32, 32, 64, 64), (2, 16, 16, 64, 128), (1, 8, 32, 128, 128),
                                  (2, 16, 16, 128, 64), (1, 16, 32, 128, 8), (2, 48, 16, 64, 24)])
def test_direct_3x3_conv_equals_the_implicit_gemm_kernel(wmz, geom):
    """csrc/conv_direct.hip (3x3, stride 1, pad 1, bf16; patch + weight stream by LDS-DMA) against conv2d_kernel on the same
    data: same K order and epilogue arithmetic -> the same bits for Cin = 64 (Cin = 128 accumulates in two channel passes: fp32
    summation order), statistics to fp32 summation order; every epilogue combination (bias, folded BatchNorm, LeakyReLU,
    residual, statistics); and against torch."""
    from world_modelz_amd import ops
    B, H, W, Ci, Co = geom
    assert ops.L.lib().wmz_conv3x3_direct_supported(H, W, Ci, Co)
    torch.manual_seed(12)
    x = torch.randn(B, H, W, Ci, device='cuda').bfloat16()
    w = (torch.randn(Co, 9 * Ci, device='cuda') * 0.05).bfloat16()
    bias = torch.randn(Co, device='cuda')
    sc, sh = torch.rand(Co, device='cuda') + 0.5, torch.randn(Co, device='cuda')
    res = torch.randn(B, H, W, Co, device='cuda').bfloat16()
    for kw in (dict(bias=bias, residual=res, leaky=True, stats=True), dict(bias=bias, leaky=True, stats=True), dict(stats=True),
               dict(scale=sc, shift=sh, leaky=True), dict(bias=bias, scale=sc, shift=sh, residual=res), dict()):
        ops.DIRECT_CONV = True
        try:
            out_d = ops.conv2d_nhwc(x, w, 3, 3, 1, 1, **kw)
            ops.DIRECT_CONV = False
            out_g = ops.conv2d_nhwc(x, w, 3, 3, 1, 1, **kw)
        finally:
            ops.DIRECT_CONV = True
        y_d, y_g = (out_d[0], out_g[0]) if kw.get('stats') else (out_d, out_g)
        if Ci == 64:
            assert torch.equal(y_d, y_g), kw.keys()
        else:
            assert float((y_d.float() - y_g.float()).norm() / y_g.float().norm()) < 2e-3
        if kw.get('stats'):
            assert torch.allclose(out_d[1].sum(0), y_d.float().sum((0, 1, 2)), rtol=1e-4, atol=2e-2)
            assert torch.allclose(out_d[2].sum(0), (y_d.float() ** 2).sum((0, 1, 2)), rtol=1e-4, atol=2e-2)
    ref = torch.nn.functional.conv2d(x.float().permute(0, 3, 1, 2), w.float().view(Co, 3, 3, Ci).permute(0, 3, 1, 2),
                                     bias=bias, padding=1).permute(0, 2, 3, 1) + res.float()
    ref = torch.nn.functional.leaky_relu(ref, 0.01)
    y = ops.conv2d_nhwc(x, w, 3, 3, 1, 1, bias=bias, residual=res, leaky=True)
    assert float((y.float() - ref).norm() / ref.norm()) < 4e-3


@pytest.mark.parametrize('geom', [(4, 16, 16, 128, 64, 1, 1, 0, True), (2, 32, 32, 64, 64, 2, 2, 0, False), (4, 16, 16, 8, 64, 3, 1, 1, False),
                                  (1, 8, 8, 64, 128, 1, 1, 0, False), (2, 16, 16, 128, 128, 1, 1, 0, False), (4, 16, 16, 8, 128, 3, 1, 1, False),
                                  (2, 8, 16, 64, 24, 1, 1, 0, True), (3, 16, 16, 64, 64, 2, 2, 0, False), (4, 24, 24, 16, 40, 3, 2, 1, False)])
def test_small_k_conv_equals_the_implicit_gemm_kernel(wmz, geom):
    """csrc/conv_point.hip (K = KH KW Cin <= 256: 1x1 with and without the BatchNorm + LeakyReLU prologue, 2x2 / stride 2, the
    3-channel 3x3 layers; bf16, persistent waves) against conv2d_kernel on the same data: same k order and epilogue arithmetic ->
    the same bits, statistics to fp32 summation order; every epilogue combination without a residual."""
    from world_modelz_amd import ops
    B, H, W, Ci, Co, k, st, pad, pre = geom
    assert ops.L.lib().wmz_conv_point_supported(B, H, W, Ci, Co, k, k, st, pad)
    torch.manual_seed(5)
    x = torch.randn(B, H, W, Ci, device='cuda').bfloat16()
    w = (torch.randn(Co, k * k * Ci, device='cuda') * 0.1).bfloat16()
    bias = torch.randn(Co, device='cuda')
    sc, sh = torch.rand(Co, device='cuda') + 0.5, torch.randn(Co, device='cuda')
    prol = (torch.rand(Ci, device='cuda') + 0.5, torch.randn(Ci, device='cuda'), 0.01) if pre else None
    for kw in (dict(bias=bias, leaky=True, stats=True), dict(stats=True), dict(scale=sc, shift=sh, leaky=True),
               dict(bias=bias, scale=sc, shift=sh, stats=True), dict()):
        ops.DIRECT_CONV = True
        try:
            out_p = ops.conv2d_nhwc(x, w, k, k, st, pad, pre=prol, **kw)
            ops.DIRECT_CONV = False
            out_g = ops.conv2d_nhwc(x, w, k, k, st, pad, pre=prol, **kw)
        finally:
            ops.DIRECT_CONV = True
        y_p, y_g = (out_p[0], out_g[0]) if kw.get('stats') else (out_p, out_g)
        assert torch.equal(y_p, y_g), (geom, list(kw))
        if kw.get('stats'):
            assert torch.allclose(out_p[1].sum(0), y_p.float().sum((0, 1, 2)), rtol=1e-4, atol=2e-2)
            assert torch.allclose(out_p[2].sum(0), (y_p.float() ** 2).sum((0, 1, 2)), rtol=1e-4, atol=2e-2)


@pytest.mark.parametrize('C,dtype', [(128, torch.bfloat16), (128, torch.float32), (16, torch.bfloat16), (24, torch.bfloat16),
                                     (512, torch.float32), (2048, torch.bfloat16), (24, torch.float32)])
def test_training_elementwise_kernels_vector_and_scalar_forms(wmz, C, dtype):
    """BatchNorm(+LeakyReLU) backward (reduce + apply), channel statistics, the two-operand affine + LeakyReLU and bilinear x2 forward /
    adjoint against fp32 torch formulas on the same (rounded) inputs.  C = 24 is not a vector-form shape (its 3 / 6 channel groups do
    not divide the workgroup): the scalar kernels; the others run the 16-byte kernels, C = 2048 with several channels per reducing
    thread."""
    from world_modelz_amd import ops
    torch.manual_seed(13)
    B, H, W = 2, 5, 7
    x = torch.randn(B, H, W, C, device='cuda').to(dtype)
    dy = torch.randn(B, H, W, C, device='cuda').to(dtype)
    y = torch.randn(B, H, W, C, device='cuda').to(dtype)
    gamma = torch.rand(C, device='cuda') + 0.5
    xf, dyf, yf = x.float(), dy.float(), y.float()
    M = B * H * W
    mean = xf.reshape(M, C).mean(0).contiguous()
    rstd = (xf.reshape(M, C).var(0, unbiased=False) + 1e-5).rsqrt().contiguous()
    tol = 2e-2 if dtype == torch.bfloat16 else 1e-5
    # statistics ([replicas, C] partial sums)
    s, q = ops.channel_stats_nhwc(x)
    assert torch.allclose(s.sum(0), xf.reshape(M, C).sum(0), rtol=1e-4, atol=1e-3)
    assert torch.allclose(q.sum(0), (xf.reshape(M, C) ** 2).sum(0), rtol=1e-4, atol=1e-3)
    # BatchNorm + LeakyReLU backward
    dx, sgx, sg, g = ops.bn_act_bwd(x, y, dy, mean, rstd, gamma, True, 0.01)
    g_ref = torch.where(yf <= 0, dyf * 0.01, dyf)
    assert rel(g, g_ref) < tol
    gr = g.float().reshape(M, C)                                   # the sums see the stored (rounded) g
    xh = (xf.reshape(M, C) - mean) * rstd
    assert torch.allclose(sg, gr.sum(0), rtol=1e-4, atol=1e-3)
    assert torch.allclose(sgx, (gr * xh).sum(0), rtol=1e-4, atol=1e-3)
    dx_ref = gamma * rstd * (gr - sg / M - xh * sgx / M)
    assert rel(dx.reshape(M, C), dx_ref) < tol
    # the same layer without a skip input: the mask recomputed from x and the forward's (scale, shift) -- wmz_bn_leaky_bwd, against
    # torch autograd through F.batch_norm + leaky_relu on the same x; and a larger tensor (several sweeps of the unrolled loops)
    if ops.bn_leaky_bwd_supported(x):
        for (b2, h2) in ((B, H), (9, 40)):
            x2 = torch.randn(b2, h2, W, C, device='cuda').to(dtype)
            dy2 = torch.randn(b2, h2, W, C, device='cuda').to(dtype)
            beta = torch.randn(C, device='cuda')
            M2 = b2 * h2 * W
            x2f = x2.float().reshape(M2, C)
            mean2 = x2f.mean(0).contiguous()
            rstd2 = (x2f.var(0, unbiased=False) + 1e-5).rsqrt().contiguous()
            scale2 = (gamma * rstd2).contiguous()
            shift2 = (beta - mean2 * scale2).contiguous()
            dx2, dgamma2, dbeta2, g2 = ops.bn_act_bwd(x2, None, dy2, mean2, rstd2, gamma, True, 0.01, remask=(scale2, shift2))
            assert g2 is None
            xin = x2f.clone().requires_grad_(True)
            gin, bin_ = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
            out = torch.nn.functional.leaky_relu(torch.nn.functional.batch_norm(xin, None, None, gin, bin_, True, 0.1, 1e-5), 0.01)
            (out * dy2.float().reshape(M2, C)).sum().backward()
            assert rel(dx2.reshape(M2, C), xin.grad) < tol
            assert rel(dgamma2, gin.grad) < (1e-4 if dtype == torch.float32 else 2e-3)
            assert rel(dbeta2, bin_.grad) < (1e-4 if dtype == torch.float32 else 2e-3)
    # y = LeakyReLU(x sa + ta + (dy sb + tb)): one rounding of the fp32 result
    sa, ta, sb, tb = (torch.randn(C, device='cuda') for _ in range(4))
    aff = ops.affine_act_nhwc(x, sa, ta, dy, sb, tb, leaky=True, slope=0.01)
    assert aff.dtype == dtype and rel(aff, torch.nn.functional.leaky_relu(xf * sa + ta + (dyf * sb + tb), 0.01)) < tol
    # bilinear x2 and its adjoint
    up = ops.bilinear2x_nhwc(x)
    up_ref = torch.nn.functional.interpolate(xf.permute(0, 3, 1, 2), scale_factor=2, mode='bilinear', align_corners=False)
    assert rel(up.permute(0, 3, 1, 2), up_ref) < tol
    dup = torch.randn(B, 2 * H, 2 * W, C, device='cuda').to(dtype)
    xin = xf.permute(0, 3, 1, 2).clone().requires_grad_(True)
    (torch.nn.functional.interpolate(xin, scale_factor=2, mode='bilinear', align_corners=False)
     * dup.float().permute(0, 3, 1, 2)).sum().backward()
    assert rel(ops.bilinear2x_nhwc_bwd(dup).permute(0, 3, 1, 2), xin.grad) < tol


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_conv_operands_bulk_refresh_equals_the_tensor_op_builds(wmz, dtype):
    """_cast.ConvOperands (wmz_conv_operands_refresh_packed: every conv layer's forward and data-gradient GEMM operands by one
    launch) == autoencoder._w_op / _wT_op's permute / pad / flip / cast builds, bit for bit, incl. channel counts that are not
    multiples of 8 (the RGB input, an odd width) and 1x1 / 3x3 / 4x4 taps; afterwards the cache serves them without a rebuild."""
    from world_modelz_amd import _cast, autoencoder
    torch.manual_seed(3)
    convs = [torch.nn.Conv2d(3, 32, 4, 2, 1), torch.nn.Conv2d(32, 20, 3, 1, 1), torch.nn.Conv2d(20, 64, 1), torch.nn.Conv2d(64, 3, 3, 1, 1)]
    convs = [c.cuda() for c in convs]
    _cast.clear()
    ref = [(autoencoder._w_op(c, dtype).clone(), autoencoder._wT_op(c.weight, dtype).clone()) for c in convs]
    _cast.clear()
    bulk = _cast.ConvOperands(convs, dtype)
    bulk.refresh()
    for c, (rw, rt) in zip(convs, ref):
        w, t = autoencoder._w_op(c, dtype), autoencoder._wT_op(c.weight, dtype)
        assert any(w.data_ptr() == e[4].data_ptr() for e in bulk.entries)          # served from the bulk buffers (a cache hit)
        assert w.shape == rw.shape and t.shape == rt.shape and torch.equal(w, rw) and torch.equal(t, rt)
    with torch.no_grad():
        convs[1].weight.mul_(2.0)                                                # a new version: the stale entry must not be served
    assert torch.equal(autoencoder._w_op(convs[1], dtype), (ref[1][0].float() * 2).to(dtype))
    if dtype == torch.bfloat16:
        # ... and the fragment-order weight streams of the direct kernels (conv_direct.hip / conv_point.hip), written by the same
        # launch: identical to what the stand-alone pack kernels make of the refreshed operands, and served from the cache
        from world_modelz_amd import ops
        convs = [torch.nn.Conv2d(64, 128, 3, 1, 1), torch.nn.Conv2d(128, 64, 1), torch.nn.Conv2d(64, 64, 2, 2), torch.nn.Conv2d(3, 64, 3, 1, 1),
                 torch.nn.Conv2d(128, 128, 3, 1, 1), torch.nn.Conv2d(128, 3, 3, 1, 1)]
        convs = [c.cuda() for c in convs]
        _cast.clear()
        bulk = _cast.ConvOperands(convs, dtype)
        bulk.refresh()
        packs = [e for e in bulk.entries if e[3] != 0]
        assert len(packs) >= 9
        for w, tag, mode, kind, dst, op in packs:
            rows, K = op.shape
            if kind == 1:
                got = ops._direct_pack(op, K // 9, rows)
                assert got.data_ptr() == dst.data_ptr()
                _cast.clear()
                assert torch.equal(ops._direct_pack(op, K // 9, rows), dst)
            else:
                got = ops._point_pack(op, K, rows)
                assert got.data_ptr() == dst.data_ptr()
                _cast.clear()
                assert torch.equal(ops._point_pack(op, K, rows), dst)
            bulk.refresh()


def test_graphed_frame_encoder_matches_eager_calls():
    """GraphedEncoder (round 4): VqAutoEncoder.encode as one hipGraph launch.  The encoder runs with BatchNorm in TRAINING mode
    (main.py:236, quirk Q3), so every call moves the running statistics: three graphed calls on fresh batches must return the
    tokens of three eager calls from the same starting state and leave the same running statistics behind."""
    from world_modelz_amd.graph import GraphedEncoder
    from world_modelz_amd.train_vqae import VqAutoEncoder
    from world_modelz_amd import config
    torch.manual_seed(9)
    with config.compute_dtype(torch.float32):
        a1 = VqAutoEncoder(embedding_dim=16, num_embeddings=64, downscale_steps=2, hidden_planes=24).cuda()
        a2 = VqAutoEncoder(embedding_dim=16, num_embeddings=64, downscale_steps=2, hidden_planes=24).cuda()
        a2.load_state_dict(a1.state_dict())
        frames = [torch.rand(6, 3, 32, 32, device='cuda') for _ in range(3)]
        with torch.no_grad():
            enc = GraphedEncoder(a2, frames[0], warmup=1)
            a1.load_state_dict(a2.state_dict())             # the warm-up call moved a2's statistics: a1 starts from there
            # (writing a2's buffers instead would change their versions and make the runner capture -- and warm up -- again)
            for f in frames:
                t1 = a1.encode(f)
                t2 = enc(f).clone()
                assert torch.equal(t1, t2)
        sd1, sd2 = a1.state_dict(), a2.state_dict()
        for k in sd1:
            if 'running' in k or 'num_batches' in k:
                assert torch.allclose(sd1[k].float(), sd2[k].float(), rtol=1e-6, atol=1e-7), k


def test_frozen_encoder_graph_survives_the_denoiser_optimizer_steps():
    """main.py:229-287 runs the FROZEN auto-encoder's encode and a denoiser training step in every iteration.  The trainer's
    optimizer launch rewrites its arena behind torch's version counters and says so (_cast.invalidate): that must name the
    trainer's own parameters -- the encoder's captured graph (GraphedEncoder) re-captured on every step before (5 ms per step on
    the reference's configuration 3), while a graph over the TRAINED model still has to re-capture."""
    from world_modelz_amd import config
    from world_modelz_amd.graph import GraphedEncoder, GraphedForward
    from world_modelz_amd.main import VqVideoDiffusionModel
    from world_modelz_amd.train import DenoiserTrainer
    from world_modelz_amd.train_vqae import VqAutoEncoder
    torch.manual_seed(3)
    with config.compute_dtype(torch.bfloat16):
        ae = VqAutoEncoder(embedding_dim=16, num_embeddings=32, downscale_steps=2, hidden_planes=24).cuda()
        frames = torch.rand(8, 3, 32, 32, device='cuda')
        model = VqVideoDiffusionModel(data_shape=(2, 8, 8), dim=64, num_classes=32, extents=(1, 1, 1), depth=1, dim_head=32,
                                      mlp_dim=64, heads=2).cuda()
        with torch.no_grad():
            enc = GraphedEncoder(ae, frames, warmup=1)
            fwd = GraphedForward(model, torch.randint(0, 33, (4, 2, 8, 8), device='cuda'))
        tr = DenoiserTrainer(model, 32, lr=1e-3, warmup=1, max_steps=100, distributed=False)
        for _ in range(3):
            with torch.no_grad():
                tok = enc(frames)
            tr.train_step(tok.view(4, 2, 8, 8).clone(), r=torch.full((4,), 0.5))
        assert enc.recaptures == 0
        with torch.no_grad():
            fwd(fwd.static_in)
        assert fwd.recaptures == 1                      # the trained model's weights did move


@pytest.mark.parametrize('geom', [(2, 16, 32, 64, True, 128), (1, 8, 16, 128, True, 128), (3, 24, 48, 128, False, 128),
                                  (5, 16, 16, 64, False, 128), (70, 16, 32, 128, True, 128), (3, 16, 32, 128, False, 8),
                                  (2, 8, 16, 64, True, 24), (40, 16, 16, 128, True, 8)])
def test_direct_3x3_weight_gradient_vs_torch(wmz, geom):
    """csrc/conv_wgrad.hip (3x3 / stride 1 / pad 1, Cout = 128 or <= 32, Cin 64 or 128, bf16: the pixel axis tiled, all nine taps from one
    staged patch, persistent workgroups + the deterministic two-stage reduction) against torch.autograd on the same bf16 operands:
    weight and bias gradients, plain [N, K] result and nn.Conv2d's layout accumulated in place; more tiles than workgroups, fewer
    tiles than workgroups, image borders."""
    from world_modelz_amd import ops
    B, H, W, Ci, bias, Co = geom
    torch.manual_seed(21)
    x = torch.randn(B, H, W, Ci, device='cuda').bfloat16()
    dy = (torch.randn(B, H, W, Co, device='cuda') * 0.5).bfloat16()
    xr = x.float().permute(0, 3, 1, 2).requires_grad_(False)
    w = torch.zeros(Co, Ci, 3, 3, device='cuda', requires_grad=True)
    b = torch.zeros(Co, device='cuda', requires_grad=True)
    y = torch.nn.functional.conv2d(xr, w, b, padding=1)
    (y * dy.float().permute(0, 3, 1, 2)).sum().backward()
    dw, db = ops.conv2d_nhwc_wgrad(x, dy, 3, 3, 1, 1, bias)                   # [Co, 9 * Ci] (tap-major), [Co]
    ref = w.grad.permute(0, 2, 3, 1).reshape(Co, 9 * Ci)
    assert rel(dw, ref) < 2e-5, geom
    if bias:
        assert rel(db, b.grad) < 2e-5
    # nn.Conv2d's own gradient tensors, accumulated (twice: the second call adds)
    gw = torch.zeros(Co, Ci, 3, 3, device='cuda')
    gb = torch.zeros(Co, device='cuda') if bias else None
    for _ in range(2):
        ops.conv2d_nhwc_wgrad(x, dy, 3, 3, 1, 1, bias, into=(gw, gb))
    ops.wgrad_join()
    assert rel(gw, 2 * w.grad) < 2e-5
    if bias:
        assert rel(gb, 2 * b.grad) < 2e-5


@pytest.mark.parametrize('geom', [(3, 32, 64, 64), (2, 16, 32, 128), (5, 64, 64, 64)])
def test_direct_3x3_stride2_conv_vs_the_implicit_gemm_kernel_and_torch(wmz, geom):
    """convr_kernel<.., STRIDE = 2> (3x3 / stride 2 / pad 1, Cout = 128: autoencoder.py:27-33; the four parity planes of the input
    staged 32 channels at a time) against conv2d_kernel (other k order: fp32 summation order) and torch, statistics included."""
    from world_modelz_amd import ops
    B, H, W, Ci = geom
    Co = 128
    assert ops.L.lib().wmz_conv3x3_direct_supported_strided(H, W, Ci, Co, 2)
    torch.manual_seed(31)
    x = torch.randn(B, H, W, Ci, device='cuda').bfloat16()
    w = (torch.randn(Co, 9 * Ci, device='cuda') * 0.05).bfloat16()
    bias = torch.randn(Co, device='cuda')
    for kw in (dict(stats=True), dict(bias=bias, leaky=True, stats=True), dict()):
        ops.DIRECT_CONV = True
        try:
            out_d = ops.conv2d_nhwc(x, w, 3, 3, 2, 1, **kw)
            ops.DIRECT_CONV = False
            out_g = ops.conv2d_nhwc(x, w, 3, 3, 2, 1, **kw)
        finally:
            ops.DIRECT_CONV = True
        y_d, y_g = (out_d[0], out_g[0]) if kw.get('stats') else (out_d, out_g)
        assert y_d.shape == (B, H // 2, W // 2, Co)
        assert float((y_d.float() - y_g.float()).norm() / y_g.float().norm()) < 2e-3
        if kw.get('stats'):
            assert torch.allclose(out_d[1].sum(0), y_d.float().sum((0, 1, 2)), rtol=1e-4, atol=2e-2)
            assert torch.allclose(out_d[2].sum(0), (y_d.float() ** 2).sum((0, 1, 2)), rtol=1e-4, atol=2e-2)
    ref = torch.nn.functional.conv2d(x.float().permute(0, 3, 1, 2), w.float().view(Co, 3, 3, Ci).permute(0, 3, 1, 2), bias=bias,
                                     stride=2, padding=1).permute(0, 2, 3, 1)
    y = ops.conv2d_nhwc(x, w, 3, 3, 2, 1, bias=bias)
    assert float((y.float() - ref).norm() / ref.norm()) < 4e-3



@pytest.mark.gpu
def test_batchnorm_finalised_by_the_kernel_that_applies_it(wmz):
    """include/wmz.h wmz_bn_stats (ops.BnLazy): a training-mode BatchNorm handed to its consumer -- the streaming 1x1 conv's input
    prologue, wmz_affine_act_nhwc_bn -- as raw statistics is the same arithmetic as a wmz_bn_finalize launch in between (one device
    function computes both).  The statistics themselves are summed by atomics in either mode, so two runs agree to fp32 summation
    order, not bit for bit: tokens (a few near-ties may flip), running statistics, step counters, loss and gradients are compared
    at that level; the kernel-level check below is exact."""
    import copy
    from world_modelz_amd import ops
    from world_modelz_amd.train_vqae import VqAutoEncoder
    torch.manual_seed(3)
    with wmz['config'].compute_dtype(torch.bfloat16):
        ae_l = VqAutoEncoder(embedding_dim=64, num_embeddings=256, downscale_steps=2, hidden_planes=128).cuda()
        ae_f = copy.deepcopy(ae_l)
        frames = torch.rand(16, 3, 64, 64, device='cuda')
        outs = {}
        for lazy, ae in ((True, ae_l), (False, ae_f)):
            ops.BN_LAZY = lazy
            try:
                with torch.no_grad():
                    tok = ae.encode(frames)
                recon, latent_loss, _ = ae(frames)
                loss = torch.nn.functional.mse_loss(recon, frames) + 0.25 * latent_loss
                loss.backward()
            finally:
                ops.BN_LAZY = True
            outs[lazy] = (tok, float(loss))
        assert float((outs[True][0] != outs[False][0]).float().mean()) < 0.02
        assert abs(outs[True][1] - outs[False][1]) < 2e-3 * abs(outs[False][1])
        n_bn = 0
        for (n, ml), mf in zip(ae_l.named_modules(), ae_f.modules()):
            if isinstance(ml, torch.nn.BatchNorm2d):
                n_bn += 1
                at = 3e-3 if n.startswith('decoder') else 1e-4          # (behind the codebook a flipped near-tie changes the input)
                assert torch.allclose(ml.running_mean, mf.running_mean, rtol=1e-3, atol=at), n
                assert torch.allclose(ml.running_var, mf.running_var, rtol=1e-2 if n.startswith('decoder') else 1e-3, atol=at / 10), n
                assert int(ml.num_batches_tracked) == int(mf.num_batches_tracked) >= 1, n
        assert n_bn >= 10
    # gradients: through one residual block (no codebook in between, whose flipped near-ties move the whole encoder's gradient)
    from world_modelz_amd.autoencoder import Residual
    with wmz['config'].compute_dtype(torch.bfloat16):
        torch.manual_seed(4)
        blk_l = Residual(64, 128, 2).cuda()
        blk_f = copy.deepcopy(blk_l)
        xin = torch.randn(8, 64, 32, 32, device='cuda')
        dy = torch.randn(8, 64, 16, 16, device='cuda')
        gin = {}
        for lazy, blk in ((True, blk_l), (False, blk_f)):
            ops.BN_LAZY = lazy
            try:
                xi = xin.clone().requires_grad_(True)
                (blk(xi) * dy).sum().backward()
            finally:
                ops.BN_LAZY = True
            gin[lazy] = xi.grad
        assert rel(gin[True], gin[False]) < 2e-2
        for (n, pl), pf in zip(blk_l.named_parameters(), blk_f.parameters()):
            assert pl.grad is not None and pf.grad is not None and rel(pl.grad, pf.grad) < 2e-2, n
    # kernel level, exact: the same statistics through both routes
    C, M = 128, 4096
    x = torch.randn(4, 32, 32, C, device='cuda').bfloat16()
    r = torch.randn(4, 32, 32, C, device='cuda').bfloat16()
    bn_a = torch.nn.BatchNorm2d(C).cuda()
    with torch.no_grad():
        bn_a.weight.uniform_(0.5, 1.5)
        bn_a.bias.normal_()
    bn_b = copy.deepcopy(bn_a)
    s, q = ops.channel_stats_nhwc(x)
    lz = ops.BnLazy(bn_a, s, q, M, want_stats=True)
    y_l = ops.affine_act_nhwc(x, lz, None, r, leaky=True)
    sc, sh, mean, rstd = ops.bn_finalize(bn_b, s, q, M, want_stats=True)
    y_f = ops.affine_act_nhwc(x, sc, sh, r, leaky=True)
    assert torch.equal(y_l, y_f)
    for a_, b_ in ((lz.scale, sc), (lz.shift, sh), (lz.mean, mean), (lz.rstd, rstd), (bn_a.running_mean, bn_b.running_mean),
                   (bn_a.running_var, bn_b.running_var), (bn_a.num_batches_tracked, bn_b.num_batches_tracked)):
        assert torch.equal(a_, b_)
    # ... and as the streaming 1x1 conv's input prologue
    w = (torch.randn(64, C, device='cuda') * 0.1).bfloat16()
    bn_c, bn_d = copy.deepcopy(bn_a), copy.deepcopy(bn_a)
    y_l = ops.conv2d_nhwc(x, w, 1, 1, 1, 0, pre=(ops.BnLazy(bn_c, s, q, M), None, 0.01))
    sc, sh = ops.bn_finalize(bn_d, s, q, M)
    y_f = ops.conv2d_nhwc(x, w, 1, 1, 1, 0, pre=(sc, sh, 0.01))
    assert torch.equal(y_l, y_f) and torch.equal(bn_c.running_var, bn_d.running_var) and torch.equal(bn_c.running_mean, bn_d.running_mean)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_zero_inserted_plane_of_a_strided_data_gradient(wmz, dtype):
    """wmz_dilate_nhwc: dz[:, ::s, ::s] = dy, zeros elsewhere, in one pass (the plane a strided conv's data gradient runs on),
    against the fill + strided copy it replaces; then the whole data gradient of a stride-2 conv against torch autograd."""
    from world_modelz_amd import ops
    torch.manual_seed(2)
    for (B, Ho, Wo, C, Hz, Wz, st) in ((3, 5, 7, 16, 10, 14, 2), (2, 4, 4, 128, 7, 7, 2), (1, 3, 2, 8, 9, 5, 3)):
        dy = torch.randn(B, Ho, Wo, C, device='cuda').to(dtype)
        ref = torch.zeros(B, Hz, Wz, C, device='cuda', dtype=dtype)
        ref[:, 0:(Ho - 1) * st + 1:st, 0:(Wo - 1) * st + 1:st] = dy
        assert torch.equal(ops.dilate_nhwc(dy, Hz, Wz, st), ref)
    # the whole data gradient of a stride-2 block (autoencoder.py:18-42: conv3x3 / s2 and the 2x2 / s2 skip conv, both strided data
    # gradients landing in one input) and every parameter gradient against torch autograd over the oracle's block on the same
    # weights, training-mode BatchNorm
    from world_modelz_amd.autoencoder import Residual
    torch.manual_seed(4)
    with wmz['config'].compute_dtype(dtype):
        blk = Residual(64, 128, 2).cuda()
        with torch.no_grad():
            for mod in blk.modules():
                if isinstance(mod, torch.nn.BatchNorm2d):
                    mod.weight.uniform_(0.5, 1.5)
                    mod.bias.normal_(0, 0.3)
        x0 = torch.randn(4, 64, 32, 32)
        dyo = torch.randn(4, 64, 16, 16)
        x = x0.cuda().requires_grad_(True)
        with recorded_calls() as seen:
            y = blk(x)
            (y * dyo.cuda()).sum().backward()
        assert 'wmz_dilate_nhwc' in seen
    leaves = {'b.' + k: (v.detach().cpu().clone().requires_grad_(True) if v.is_floating_point() and 'running' not in k
                          else v.detach().cpu().clone()) for k, v in blk.state_dict().items()}
    for k in leaves:                                   # (the HIP pass already moved the running statistics; the oracle gets its own)
        if k.endswith('running_mean'):
            leaves[k] = torch.zeros_like(leaves[k])
        elif k.endswith('running_var'):
            leaves[k] = torch.ones_like(leaves[k])
    xo = x0.clone().requires_grad_(True)
    yo = oae.residual_block(leaves, 'b.', xo, 2, True)
    (yo * dyo).sum().backward()
    # bf16: the gradient of a LeakyReLU network against a RANDOM output direction is not smooth in the activations -- an element whose
    # pre-activation lies within the bf16 error of zero (~0.4 % of them here) changes its mask, i.e. its whole contribution: expected
    # error ~ sqrt(0.004) = 6 % in every gradient, from the last BatchNorm's bias on (tools/diag_resblock_grad.py; any bf16 framework
    # shows it).  The fp32 branch is the exact check of the kernels; the bf16 one bounds the route and pins the explanation below.
    t_out, t_g = (1e-5, 2e-4) if dtype == torch.float32 else (1e-2, 1e-1)
    assert y.shape == yo.shape and rel(y, yo) < t_out, rel(y, yo)
    if dtype == torch.bfloat16:
        # ... the last BatchNorm's bias gradient is sum(dy * mask): with the mask of the HIP path's OWN output it is reproduced to
        # bf16 rounding of dy -- the 6 % is the mask, not the arithmetic
        emul = (dyo.bfloat16().float() * torch.where(y.detach().float().cpu() > 0, 1.0, 0.01)).sum((0, 2, 3))
        assert rel(blk._block[4].bias.grad, emul) < 5e-3, rel(blk._block[4].bias.grad, emul)
    assert rel(x.grad, xo.grad) < t_g, rel(x.grad, xo.grad)
    for n, prm in blk.named_parameters():
        assert prm.grad is not None and rel(prm.grad, leaves['b.' + n].grad) < t_g, (n, rel(prm.grad, leaves['b.' + n].grad))


@pytest.mark.gpu
def test_frame_encoder_at_full_size_on_the_direct_kernels_vs_the_implicit_gemm_path(wmz):
    """BASELINE config 3's frame batch (256 frames of 64 x 64, the VQ auto-encoder of main.py:229-237, BatchNorm in training mode):
    the round-5 kernels (direct 3x3 / streaming small-K / consumer-finalised BatchNorm) against the implicit-GEMM kernels with a
    wmz_bn_finalize launch each, on the same weights -- the same latents to bf16 rounding (the stride-2 form sums in another
    order), tokens up to near-ties, running statistics to the same level (two forward passes each); and the encoder's output is invariant under a
    permutation of the frames (BatchNorm statistics are sums over the batch: a size-independent property at full size)."""
    import copy
    from world_modelz_amd import ops
    from world_modelz_amd.train_vqae import VqAutoEncoder
    torch.manual_seed(11)
    with wmz['config'].compute_dtype(torch.bfloat16):
        ae_a = VqAutoEncoder(embedding_dim=64, num_embeddings=1024, downscale_steps=2, hidden_planes=128).cuda()
        ae_b, ae_c = copy.deepcopy(ae_a), copy.deepcopy(ae_a)
        frames = torch.rand(256, 3, 64, 64, device='cuda')
        with torch.no_grad():
            lat_a = ae_a._latents(frames).float()
            tok_a = ae_a.vq.encode(ae_a._latents(frames)).view(256, 16, 16)
            ops.DIRECT_CONV, ops.BN_LAZY = False, False
            try:
                lat_b = ae_b._latents(frames).float()
                tok_b = ae_b.vq.encode(ae_b._latents(frames)).view(256, 16, 16)
            finally:
                ops.DIRECT_CONV, ops.BN_LAZY = True, True
            perm = torch.randperm(256, device='cuda')
            lat_c = ae_c._latents(frames[perm]).float()
        # (bf16 activations: the two routes round differently in the stride-2 layers; a random-init codebook has many near-ties)
        assert rel(lat_a, lat_b) < 2e-2, rel(lat_a, lat_b)
        assert float((tok_a != tok_b).float().mean()) < 0.04
        assert rel(lat_a[perm], lat_c) < 1.5e-2, rel(lat_a[perm], lat_c)     # (statistics summed in another order: bf16 rounding, six normalisations deep)
        for (n, ma), mb in zip(ae_a.named_modules(), ae_b.modules()):
            if isinstance(ma, torch.nn.BatchNorm2d) and n.startswith('encoder'):
                assert torch.allclose(ma.running_mean, mb.running_mean, rtol=2e-3, atol=2e-4), n
                assert torch.allclose(ma.running_var, mb.running_var, rtol=5e-3, atol=1e-5), n


@pytest.mark.parametrize('in_dt,out_dt,E', [(torch.float32, torch.float32, 64), (torch.bfloat16, torch.bfloat16, 64),
                                            (torch.float32, torch.bfloat16, 20), (torch.bfloat16, torch.float32, 12)])
def test_vq_tail_kernels_vs_torch(wmz, in_dt, out_dt, E):
    """ops.vq_tail (wmz_vq_tail_fwd / _bwd: vq.py:67 commitment loss, :70 straight-through estimator, :72-73 perplexity) against the
    torch expressions of the reference, forward and backward, with channel padding and every dtype pairing the model uses."""
    from world_modelz_amd import ops
    torch.manual_seed(E)
    N, C = 3 * 5 * 7, 96
    Ep = -(-E // 8) * 8
    inp = torch.randn(3, 5, 7, E, device='cuda').to(in_dt).requires_grad_(True)
    flat = inp.detach().reshape(-1, E).float()
    q = (flat + 0.3 * torch.randn_like(flat)).contiguous()
    counts = torch.bincount(torch.randint(0, C, (N,), device='cuda'), minlength=C).float()
    st, loss, ppl = ops.vq_tail(inp, flat, q, counts, out_dt, Ep)
    assert st.shape == (3, 5, 7, Ep) and st.dtype == out_dt and loss.dtype == torch.float32
    x32 = inp.detach().float().requires_grad_(True)
    q32 = q.view(3, 5, 7, E)
    loss_ref = torch.nn.functional.mse_loss(q32, x32)
    st_ref = x32 + (q32 - x32).detach()
    p = counts / N
    ppl_ref = torch.exp(-torch.sum(p * torch.log(p + 1e-10)))
    assert torch.equal(st[..., :E].float(), st_ref.detach().to(out_dt).float())             # the reference's own two roundings
    assert Ep == E or float(st[..., E:].abs().max()) == 0.0
    assert torch.allclose(loss, loss_ref, rtol=2e-6) and torch.allclose(ppl, ppl_ref, rtol=2e-6)
    w = torch.randn(3, 5, 7, Ep, device='cuda').to(out_dt)
    ((st.float() * w.float()).sum() + 0.37 * loss).backward()
    ((st_ref * w[..., :E].float()).sum() + 0.37 * loss_ref).backward()
    tol = 1e-6 if in_dt == torch.float32 else 8e-3
    assert rel(inp.grad, x32.grad) < tol, rel(inp.grad, x32.grad)
    # the loss alone (no gradient through the straight-through tensor) and the tensor alone
    inp.grad = None
    _, loss2, _ = ops.vq_tail(inp, flat, q, counts, out_dt, Ep)
    loss2.backward()
    g_ref = 2.0 / (N * E) * (flat - q).view(3, 5, 7, E)
    assert rel(inp.grad, g_ref) < tol


@pytest.mark.parametrize('kind', ['SmoothL1', 'MSE', 'MAE'])
@pytest.mark.parametrize('dt,Cp', [(torch.bfloat16, 8), (torch.float32, 8), (torch.bfloat16, 3)])
def test_recon_loss_kernels_vs_torch(wmz, kind, dt, Cp):
    """ops.recon_loss (wmz_recon_loss_fwd / _bwd: train_vqae.py:139-150, :264-271) on the decoder's NHWC channel-padded output in
    place against torch's loss on the NCHW fp32 reconstruction, value and gradient (zero in the padding channels)."""
    from world_modelz_amd import ops
    from world_modelz_amd.train import VqaeTrainer
    torch.manual_seed(5)
    B, C, H, W = 5, 3, 24, 20
    y = (2.0 * torch.randn(B, H, W, Cp, device='cuda')).to(dt).requires_grad_(True)      # (|y - t| on both sides of SmoothL1's beta)
    t = torch.rand(B, C, H, W, device='cuda')
    loss = ops.recon_loss(y, t, kind)
    y32 = y.detach().float().requires_grad_(True)
    ref = VqaeTrainer.LOSSES[kind](y32[..., :C].permute(0, 3, 1, 2), t)
    assert torch.allclose(loss, ref, rtol=3e-6), (float(loss), float(ref))
    (1.7 * loss).backward()
    (1.7 * ref).backward()
    assert y.grad.dtype == dt and (Cp == C or float(y.grad[..., C:].abs().max()) == 0.0)
    assert rel(y.grad, y32.grad) < (1e-6 if dt == torch.float32 else 4e-3)


def test_vqae_step_fused_losses_vs_torch_losses(wmz):
    """VqaeTrainer with the fused scalar side (quantiser tail + reconstruction loss kernels: the default) against the same step
    with the reconstruction as an NCHW fp32 tensor and torch's loss on it: the four step scalars and every gradient, fp32 and bf16."""
    from world_modelz_amd import train
    from world_modelz_amd.train_vqae import VqAutoEncoder
    for dt, tol in ((torch.float32, 1e-4), (torch.bfloat16, 2e-2)):
        out = {}
        for fused in (True, False):
            torch.manual_seed(21)
            m = VqAutoEncoder(embedding_dim=64, num_embeddings=256, downscale_steps=2, hidden_planes=64).cuda()
            x = torch.rand(8, 3, 32, 32, device='cuda')
            with wmz['config'].compute_dtype(dt):
                tr = train.VqaeTrainer(m, loss_fn='SmoothL1', latent_loss_weight=0.25, distributed=False)
                tr.fused_losses = fused
                tr.arena.zero_grad()
                tr._refresh_conv_operands()
                scal = tr._forward_backward(x)
            out[fused] = (scal.clone(), tr.arena.flat_grad.clone())
        s_f, g_f = out[True]
        s_t, g_t = out[False]
        assert torch.allclose(s_f, s_t, rtol=tol, atol=tol * 1e-2), (s_f, s_t)
        e = rel(g_f, g_t)
        print(f'[vqae fused losses {dt}] scalars {s_f.tolist()} gradient rel {e:.2e}')
        # (bf16: the two routes round the straight-through tensor and the loss gradient differently -- one bf16 ulp -- and every
        #  LeakyReLU / SmoothL1 branch that flips on it moves a gradient by its full size: 4-5 %, the level of
        #  test_bf16_vqae_forward_backward_vs_oracle_autograd's bound on the same model)
        # (fp32: two runs of the SAME route already differ by up to ~2e-4 -- BatchNorm's statistics are atomic sums, and a
        #  pre-activation within an ulp of zero takes the other LeakyReLU slope: measured 1.8e-4 once in four runs)
        assert e < (2e-3 if dt == torch.float32 else 8e-2), e
