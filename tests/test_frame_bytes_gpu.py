"""GPU: byte frames in and out of the VQ auto-encoder (csrc/frame_bytes.hip).  Everything here is exact: the ingest against
wmz_nchw_to_nhwc8 of the fp32 frames the reference prepares on the CPU (byte / 255), the egress against save_image's law computed
by torch on the CPU (frame_bytes_cases.py), every output inside a sentinel frame; then the methods built on the two launches
against the float paths they stand in for, with BatchNorm in eval mode (a training-mode pass sums its statistics with float atomics:
there only the entry points are compared)."""
import contextlib

import pytest
import torch

import frame_bytes_cases as fb
from conftest import recorded_calls

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SHAPES = [(3, 3, 8, 8), (2, 3, 5, 7), (3, 1, 8, 8), (2, 1, 3, 5), (2, 11, 4, 6)]          # (N, C, H, W)
SENTINEL = 0xA5


@pytest.fixture(scope='module')
def L():
    assert torch.cuda.is_available()
    from world_modelz_amd import _lib
    _lib.lib()
    return _lib


def framed(shape, dtype, offset=64, pad=64):
    """A contiguous device tensor of `shape` `offset` bytes into a buffer of sentinel bytes, `pad` more behind it -> (view, intact),
    intact() true while no byte outside the view has changed."""
    n = torch.empty(shape, dtype=dtype).numel() * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((offset + n + pad,), SENTINEL, dtype=torch.uint8, device='cuda')
    view = buf[offset:offset + n].view(dtype).view(shape)

    def intact():
        return bool((buf[:offset] == SENTINEL).all()) and bool((buf[offset + n:] == SENTINEL).all())
    return view, intact


def byte_frames(N, C, H, W, channels_last, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (N, H, W, C) if channels_last else (N, C, H, W), dtype=torch.uint8, generator=g)


def as_nchw(x, channels_last):
    return x.permute(0, 3, 1, 2) if channels_last else x


def reference_nhwc8(x_cpu, channels_last, dtype):
    """What the parent's path makes of these bytes: transform_batch on the CPU, upload, wmz_nchw_to_nhwc8."""
    from world_modelz_amd import ops
    ref = fb.unit_of_bytes(as_nchw(x_cpu, channels_last)).contiguous()
    return ops.nchw_to_nhwc8(ref.cuda(), dtype)


def ingest(L, xd, N, C, H, W, frame_stride, channels_last, dtype):
    """The entry point itself on device bytes xd (frame n at xd.data_ptr() + n * frame_stride) into a framed output."""
    C8 = (C + 7) // 8 * 8
    y, intact = framed((N, H, W, C8), dtype)
    L.call('wmz_frames_u8_to_nhwc8', xd.data_ptr(), y.data_ptr(), N, C, H, W, frame_stride, int(channels_last), L.dtype_code(dtype),
           L.stream())
    torch.cuda.synchronize()
    assert intact(), 'the ingest wrote outside its output'
    if C8 != C:
        assert bool((y[..., C:].view(torch.uint8) == 0).all()), 'padding channels are not exactly zero'
    return y


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('channels_last', [True, False])
@pytest.mark.parametrize('shape', SHAPES)
def test_ingest_is_nchw_to_nhwc8_of_the_cpu_frames(L, shape, channels_last, dtype):
    N, C, H, W = shape
    x = byte_frames(N, C, H, W, channels_last, seed=sum(shape))
    want = reference_nhwc8(x, channels_last, dtype)
    got = ingest(L, x.cuda(), N, C, H, W, C * H * W, channels_last, dtype)
    assert got.dtype == dtype and torch.equal(got, want)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('channels_last', [True, False])
def test_ingest_of_every_byte_value_in_every_channel(L, channels_last, dtype):
    g = torch.Generator().manual_seed(3)
    planes = torch.stack([torch.randperm(256, generator=g).to(torch.uint8).view(16, 16) for _ in range(3)])      # [C, H, W]
    x = (planes.permute(1, 2, 0) if channels_last else planes).contiguous()[None]
    got = ingest(L, x.cuda(), 1, 3, 16, 16, 768, channels_last, dtype)
    assert torch.equal(got, reference_nhwc8(x, channels_last, dtype))
    assert torch.equal(got[0, ..., 0].flatten().float().sort().values.cpu(), fb.unit_of_bytes(torch.arange(256, dtype=torch.uint8)).to(dtype).float())


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('channels_last', [True, False])
def test_ingest_from_a_misaligned_base_and_with_a_frame_stride(L, channels_last, dtype):
    """The base pointer one byte off (storage_offset 1) and frames 2 F + 3 bytes apart, the bytes between them never read into the
    result: they differ between two runs that must agree."""
    N, C, H, W = 3, 3, 5, 7
    F = C * H * W
    stride = 2 * F + 3
    x = byte_frames(N, C, H, W, channels_last, seed=11)
    want = reference_nhwc8(x, channels_last, dtype)
    for filler in (0, 255):
        buf = torch.full((1 + N * stride,), filler, dtype=torch.uint8, device='cuda')
        view = buf[1:].view(N, stride)[:, :F]
        view.copy_(x.view(N, F))
        assert view.data_ptr() % 2 == 1 and view.storage_offset() == 1
        got = ingest(L, view, N, C, H, W, stride, channels_last, dtype)
        assert torch.equal(got, want), filler


@contextlib.contextmanager
def recorded_arguments():
    """(name, args) of every C-ABI call of the block."""
    from world_modelz_amd import _lib
    seen, orig = [], _lib.call

    def call(name, *a):
        seen.append((name, a))
        return orig(name, *a)
    _lib.call = call
    try:
        yield seen
    finally:
        _lib.call = orig


@pytest.mark.parametrize('channels_last', [True, False])
def test_wrapper_reads_strided_batches_where_they_are(L, channels_last):
    """ops.frames_u8_to_nhwc8 on views of a [B, T] batch: one launch, handed the view's own address and its frame stride (no copy),
    leading dimensions flattened; a view without a single stride is copied and still right."""
    from world_modelz_amd import ops
    B, T, C, H, W = 4, 2, 3, 6, 5
    F = C * H * W
    fshape = (H, W, C) if channels_last else (C, H, W)
    g = torch.Generator().manual_seed(5)
    batch = torch.randint(0, 256, (B, T) + fshape, dtype=torch.uint8, generator=g)
    bd = batch.cuda()
    cases = [(bd[:, 1:], batch[:, 1:], T * F, True),            # sliced in T: frame stride != frame size
             (bd[:, 0], batch[:, 0], T * F, True),
             (bd, batch, F, True)]
    wide = torch.randint(0, 256, (B, 3) + fshape, dtype=torch.uint8, generator=g)
    cases.append((wide.cuda()[:, 1:], wide[:, 1:], F, False))   # two frames per clip, clips three apart: no single stride
    for view, cpu, stride, in_place in cases:
        with recorded_arguments() as seen:
            got = ops.frames_u8_to_nhwc8(view, torch.bfloat16, channels_last)
        assert [n for n, _ in seen] == ['wmz_frames_u8_to_nhwc8']
        a = seen[0][1]
        N = cpu.numel() // F
        assert a[2:9] == (N, C, H, W, stride, int(channels_last), L.dtype_code(torch.bfloat16))
        assert (a[0] == view.data_ptr()) == in_place
        assert got.shape == (N, H, W, 8)
        assert torch.equal(got, reference_nhwc8(cpu.reshape((N,) + fshape), channels_last, torch.bfloat16))


def law_frames(raw_cpu, C, channels_last):
    """save_image's law on the real channels of a raw NHWC tensor -> uint8 [N, H, W, C] or [N, C, H, W]."""
    out = fb.bytes_of_units(raw_cpu[..., :C])
    return out if channels_last else out.permute(0, 3, 1, 2).contiguous()


def egress(L, raw, C, channels_last):
    """The entry point on a raw [N, H, W, C8] device tensor whose padding channels hold NaN, into a framed, misaligned output."""
    N, H, W, C8 = raw.shape
    raw = raw.clone()
    raw[..., C:] = float('nan')
    out, intact = framed((N, H, W, C) if channels_last else (N, C, H, W), torch.uint8, offset=61)
    L.call('wmz_nhwc8_to_frames_u8', raw.data_ptr(), out.data_ptr(), N, C, H, W, int(channels_last), L.dtype_code(raw.dtype), L.stream())
    torch.cuda.synchronize()
    assert intact(), 'the egress wrote outside its output'
    return out.cpu()


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('channels_last', [True, False])
@pytest.mark.parametrize('C', [1, 3])
def test_egress_of_every_16_bit_pattern(L, C, channels_last, dtype):
    pat = fb.all_patterns(dtype)
    N, H, W = 2, 128, 256                                              # 65 536 pixels: every pattern in every real channel
    raw = torch.zeros(N, H, W, 8, dtype=dtype)
    for c in range(C):
        raw[..., c] = pat.roll(977 * c).view(N, H, W)
    got = egress(L, raw.cuda(), C, channels_last)
    want = law_frames(raw, C, channels_last)
    assert torch.equal(got, want), (got != want).nonzero()[:4]
    assert int(got.min()) == 0 and int(got.max()) == 255


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('channels_last', [True, False])
@pytest.mark.parametrize('C', [3, 11])
def test_egress_of_the_fp32_boundaries_and_odd_shapes(L, C, channels_last, dtype):
    """The fp32 boundary set (rounded into the operand dtype for the 16-bit formats: whatever they hold is taken to fp32 exactly)
    over an odd plane, one and two channel groups."""
    v = fb.fp32_boundaries().to(dtype)
    N, H, W = 2, 17, 23
    n = N * H * W * C
    assert n >= v.numel()
    raw = torch.full((N, H, W, (C + 7) // 8 * 8), 0.25, dtype=dtype)
    raw[..., :C] = v.repeat(-(-n // v.numel()))[:n].view(N, H, W, C)
    got = egress(L, raw.cuda(), C, channels_last)
    want = law_frames(raw, C, channels_last)
    assert torch.equal(got, want), (got != want).nonzero()[:4]


def test_wrappers_reach_one_entry_point_each_and_refuse_what_they_cannot_take(L):
    from world_modelz_amd import ops
    from world_modelz_amd._lib import WmzError
    x = byte_frames(2, 3, 8, 8, True)
    with recorded_calls() as seen:
        y = ops.frames_u8_to_nhwc8(x.cuda(), torch.float16)
        out = ops.nhwc8_to_frames_u8(y, 3)
        out_cf = ops.nhwc8_to_frames_u8(y.view(1, 2, 8, 8, 8), 3, channels_last=False)
    assert seen == ['wmz_frames_u8_to_nhwc8', 'wmz_nhwc8_to_frames_u8', 'wmz_nhwc8_to_frames_u8']
    assert torch.equal(out.cpu(), x) and torch.equal(out_cf.cpu(), x.permute(0, 3, 1, 2))          # the round trip is the identity
    with pytest.raises(WmzError):
        ops.frames_u8_to_nhwc8(x, torch.float16)                        # CPU bytes
    with pytest.raises(WmzError):
        ops.nhwc8_to_frames_u8(y.cpu(), 3)
    with pytest.raises(WmzError):
        ops.frames_u8_to_nhwc8(x.cuda().float(), torch.float16)         # not bytes
    with pytest.raises(WmzError):
        ops.nhwc8_to_frames_u8(y, 9)                                    # C8 of 9 channels is 16
    with pytest.raises(WmzError, match='frame_stride'):
        L.call('wmz_frames_u8_to_nhwc8', x.cuda().data_ptr(), y.data_ptr(), 2, 3, 8, 8, 191, 1, L.dtype_code(torch.float16), L.stream())


# ---------------------------------------------------------------------------------------------------- the methods on top

MODES = {'bf16': (torch.bfloat16, False), 'fp32': (torch.float32, False), 'precise': (torch.float16, True)}


@contextlib.contextmanager
def mode(name):
    from world_modelz_amd import config
    dt, switch = MODES[name]
    with config.compute_dtype(dt), config.precise_conv(switch), torch.no_grad():
        yield


def transform_batch(frames_u8_cpu):
    """minecraft/main2.py:51-56 on the host: [..., H, W, C] bytes -> [N, C, H, W] fp32 in [0, 1]."""
    x = frames_u8_cpu.reshape((-1,) + tuple(frames_u8_cpu.shape[-3:])).permute(0, 3, 1, 2)
    return fb.unit_of_bytes(x).contiguous()


def block_frames(N, C, size, seed):
    """uint8 [N, size, size, C]: 4 x 4 blocks of random colours under a little noise -- frames whose latents differ from token to
    token (uniform noise encodes to one and the same token everywhere: a comparison of such tokens would show nothing)."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randint(0, 256, (N, size // 4, size // 4, C), generator=g).repeat_interleave(4, 1).repeat_interleave(4, 2)
    return (base + torch.randint(-8, 9, (N, size, size, C), generator=g)).clamp(0, 255).to(torch.uint8)


def calibrated(ae, C, size, seed):
    """The auto-encoder on the GPU in eval mode, BatchNorm statistics off the identity, its codebook set to latents of block frames (of
    another seed than any test's): the tokens of such frames then spread over the codebook."""
    from world_modelz_amd import config
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in ae.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
        ae = ae.cuda().eval()
        with config.compute_dtype(torch.float32):
            lat = ae._latents(transform_batch(block_frames(8, C, size, seed)).cuda())
        lat = lat.reshape(-1, lat.shape[-1])
        pick = torch.randperm(lat.shape[0], generator=g)[:ae.vq.num_embeddings]
        ae.vq.embedding[0].copy_(lat[pick.cuda()])
        # ... and the decoder's last convolution (no bias) scaled so that its images reach from below 0 to beyond 1: bytes over the
        # whole range, both clamps at work (a freshly initialised decoder stays within a few bytes of 0)
        with config.compute_dtype(torch.float32):
            img = ae.decode(ae.vq.encode(lat).view(8, size // 4, size // 4))
        ae.decoder.decoder_stack[-1].weight.mul_(1.5 / float(img.abs().max()))
    return ae


def make_ae(hidden_planes, seed=21):
    from world_modelz_amd.train_vqae import VqAutoEncoder
    torch.manual_seed(seed)
    return calibrated(VqAutoEncoder(embedding_dim=64, num_embeddings=64, downscale_steps=2, hidden_planes=hidden_planes), 3, 32, seed)


@pytest.mark.parametrize('mode_name', list(MODES))
@pytest.mark.parametrize('hidden_planes', [128, 32])
def test_eval_mode_auto_encoder_bytes_equal_the_float_paths(hidden_planes, mode_name):
    ae = make_ae(hidden_planes).eval()
    frames = block_frames(3, 3, 32, seed=31)
    floats = transform_batch(frames).cuda()
    with mode(mode_name):
        z = ae.encode(floats)
        assert torch.equal(z, ae.encode(floats)), 'an eval-mode pass is not deterministic: nothing below would mean anything'
        assert len(torch.unique(z)) >= 16, 'degenerate tokens: nothing below would mean anything'
        with recorded_calls() as seen:
            zb = ae.encode_frames(frames.cuda())
        assert 'wmz_frames_u8_to_nhwc8' in seen and 'wmz_nchw_to_nhwc8' not in seen
        assert zb.dtype == torch.int64 and zb.shape == (3, 8, 8) and torch.equal(zb, z)
        zc = ae.encode_frames(frames.permute(0, 3, 1, 2).contiguous().cuda().view(1, 3, 3, 32, 32), channels_last=False)
        assert zc.shape == (1, 3, 8, 8) and torch.equal(zc[0], z)
        img = ae.decode(z)                                                      # fp32 logical NCHW
        with recorded_calls() as seen:
            out = ae.decode_frames(z)
        assert seen[-1] == 'wmz_nhwc8_to_frames_u8'
        assert out.dtype == torch.uint8 and out.shape == (3, 32, 32, 3)
        assert torch.equal(out.cpu(), fb.bytes_of_units(img).permute(0, 2, 3, 1))
        assert len(torch.unique(out)) >= 16
        out_cf = ae.decode_frames(z.view(1, 3, 8, 8), channels_last=False)
        assert out_cf.shape == (1, 3, 3, 32, 32) and torch.equal(out_cf[0].cpu(), fb.bytes_of_units(img))


@pytest.mark.parametrize('mode_name', list(MODES))
def test_training_mode_auto_encoder_takes_the_same_pass_behind_the_ingest(mode_name):
    """BatchNorm in training mode (quirk Q3, how the frozen auto-encoder runs in main.py): no values compared, the entry points are
    those of encode with the byte ingest in the layout flip's place."""
    ae = make_ae(128).train()
    frames = block_frames(3, 3, 32, seed=32)
    floats = transform_batch(frames).cuda()
    with mode(mode_name):
        ae.encode(floats)                                      # (weight packs and operand casts run at first use only)
        with recorded_calls() as plain:
            z = ae.encode(floats)
        with recorded_calls() as seen:
            zb = ae.encode_frames(frames.cuda())
        assert plain.count('wmz_nchw_to_nhwc8') == 1
        assert seen == ['wmz_frames_u8_to_nhwc8' if n == 'wmz_nchw_to_nhwc8' else n for n in plain]
        assert zb.shape == z.shape == (3, 8, 8) and zb.dtype == z.dtype == torch.int64
        out = ae.decode_frames(zb)
        assert out.shape == (3, 32, 32, 3) and out.dtype == torch.uint8


def test_captured_encoder_replays_from_pinned_bytes():
    from world_modelz_amd.graph import GraphedEncoder
    ae = make_ae(128).eval()
    batches = [block_frames(3, 3, 32, seed=s).pin_memory() for s in (41, 42)]
    with mode('bf16'):
        with recorded_calls() as seen:
            enc = GraphedEncoder(ae, torch.zeros(3, 32, 32, 3, dtype=torch.uint8, device='cuda'), warmup=1)
        assert enc.static_in.dtype == torch.uint8 and 'wmz_frames_u8_to_nhwc8' in seen and 'wmz_nchw_to_nhwc8' not in seen
        got = [enc(b).clone() for b in batches]
        want = [ae.encode_frames(b.cuda()) for b in batches]
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(got[0], got[1])


def test_predict_frames_is_the_hand_composed_pipeline():
    """sample.predict_frames on the tiny denoiser of tests/golden/sampler_tiny.npz's geometry with injected uniforms: tokens and
    bytes of CPU transform_batch -> encode -> sample_frames -> decode (one generated frame at a time) -> save_image's law."""
    from world_modelz_amd import config, sample
    from world_modelz_amd.main import VqVideoDiffusionModel
    from world_modelz_amd.train_vqae import VqAutoEncoder
    torch.manual_seed(51)
    C, B, n_frames, n_iter = 16, 2, 2, 3
    model = VqVideoDiffusionModel(data_shape=(3, 4, 4), dim=16, num_classes=C, extents=(1, 1, 1), depth=2, dim_head=8, mlp_dim=24,
                                  heads=2).cuda()
    ae = calibrated(VqAutoEncoder(embedding_dim=8, num_embeddings=C, downscale_steps=2, hidden_planes=8, in_channels=1), 1, 16, 52)
    context = block_frames(B * 2, 1, 16, seed=53).view(B, 2, 16, 16, 1)
    uniforms = (torch.rand(n_frames, n_iter, B * 16), torch.rand(n_frames, n_iter, B, 16))
    kw = dict(num_eval_iterations=n_iter, sample_topk=4, uniforms=uniforms, use_graph=False)
    with config.compute_dtype(torch.float32), torch.no_grad():
        z = ae.encode(transform_batch(context).cuda()).view(B, 2, 4, 4)
        batch_z = torch.cat([z, torch.full_like(z[:, :1], C)], dim=1)
        latents, zf = sample.sample_frames(model, batch_z, C, n_frames, **kw)
        want = torch.stack([fb.bytes_of_units(ae.decode(f)).permute(0, 2, 3, 1) for f in latents], dim=1)
        frames, zf_b = sample.predict_frames(model, ae, context.cuda(), C, n_frames, **kw)
        frames_cf, _ = sample.predict_frames(model, ae, context.permute(0, 1, 4, 2, 3).contiguous().cuda(), C, n_frames,
                                             channels_last=False, **kw)
    assert frames.dtype == torch.uint8 and frames.shape == (B, n_frames, 16, 16, 1)
    assert torch.equal(zf_b, zf) and torch.equal(frames.cpu(), want)
    assert torch.equal(frames_cf.cpu(), want.permute(0, 1, 4, 2, 3))
    assert len(torch.unique(z)) > 2 and len(torch.unique(torch.stack(latents))) > 2 and len(torch.unique(frames)) > 2


def test_methods_refuse_wrong_frames():
    from world_modelz_amd._lib import WmzError
    ae = make_ae(32).eval()
    with torch.no_grad():
        with pytest.raises(WmzError):
            ae.encode_frames(torch.zeros(2, 32, 32, 3, dtype=torch.uint8))                    # CPU bytes
        with pytest.raises(WmzError):
            ae.encode_frames(torch.zeros(2, 3, 32, 32, device='cuda'))                        # float frames
        with pytest.raises(WmzError):
            ae.encode_frames(torch.zeros(2, 32, 32, 1, dtype=torch.uint8, device='cuda'))     # one channel for a 3-channel encoder
        with pytest.raises(WmzError):
            ae.encode_frames(torch.zeros(2, 32, 32, 3, dtype=torch.uint8, device='cuda'), channels_last=False)
