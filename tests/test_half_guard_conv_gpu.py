"""config.half_guard on the conv encoder / decoder's half route (config.precise_conv): frames and latents scaled out of the half range
are raised or fall back to the fp32 route; unscaled inputs raise nothing and match the 'off' run.  The fallback IS the fp32 route
(the recorded calls show it), and where that route is deterministic -- BatchNorm in eval mode -- its result is asserted bit for
bit.  With BatchNorm in training mode the fp32 route sums its batch statistics with float atomics: two fp32 passes on
identical copies already differ in the last digits (measured here: printed as 'fp32 vs fp32'), so no implementation can be
torch.equal to "the" fp32 result there; those cases assert the route matrix's fp32 bound, 1e-5 relative, against a second fp32
pass.  Overflow to an infinity is ordinary arithmetic: nothing here faults."""
import contextlib
import copy
import warnings

import pytest
import torch

from conftest import recorded_calls

pytestmark = pytest.mark.gpu

from oracle import autoencoder as oae        # noqa: E402

HALF_CONV = ('wmz_conv3x3_direct_fwd_strided_f16', 'wmz_conv_point_fwd_bn_f16')
TOL_FP32 = 1e-5                              # tests/test_route_matrix_gpu.py TOL['fp32']


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _vqae(seed, training):
    from world_modelz_amd.train_vqae import VqAutoEncoder
    torch.manual_seed(seed)
    m = VqAutoEncoder(embedding_dim=64, num_embeddings=512, downscale_steps=2, hidden_planes=128).cuda()
    m.train(training)
    return m


@contextlib.contextmanager
def _half(policy):
    from world_modelz_amd import config
    with config.compute_dtype(torch.float16), config.precise_conv(True), config.half_guard(policy), torch.no_grad():
        yield


@contextlib.contextmanager
def _fp32():
    from world_modelz_amd import config
    with config.compute_dtype(torch.float32), torch.no_grad():
        yield


def _same_state(a, b, exact):
    """Integer buffers (num_batches_tracked: ONE pass was counted) equal; float tensors equal, or -- training-mode BatchNorm, whose
    sums are float atomics -- within the fp32 bound relative to the tensor's norm (the statistics of frames x 1e6 are ~1e11)."""
    sa, sb = a.state_dict(), b.state_dict()
    return all(torch.equal(sa[k], sb[k]) if exact or not sa[k].is_floating_point() else rel(sa[k], sb[k]) < TOL_FP32 for k in sa)


@pytest.mark.parametrize('scale', [1e6, 1.0], ids=['frames-x1e6', 'frames'])
def test_encoder_train_mode(scale):
    from world_modelz_amd._lib import WmzError
    m = _vqae(61, True)
    torch.manual_seed(62)
    frames = torch.rand(32, 3, 64, 64) * scale
    fc = frames.cuda()
    m32, m32b, moff, mraise, mfb = (copy.deepcopy(m) for _ in range(5))
    with _fp32():
        lat32 = m32.encoder.forward_nhwc(fc)
        print(f'[half guard conv] encoder, fp32 vs fp32 on identical copies: rel {rel(m32b.encoder.forward_nhwc(fc), lat32):.2e}')
    with _half('off'), recorded_calls() as seen_off:
        lat_off = moff.encoder.forward_nhwc(fc)
    assert all(n in seen_off for n in HALF_CONV) and not any('half_guard' in n for n in seen_off), set(seen_off)
    if scale == 1.0:
        with _half('raise'), recorded_calls() as seen:
            lat = mraise.encoder.forward_nhwc(fc)
        assert 'wmz_half_guard_clear' in seen and lat.dtype == torch.float16
        e = rel(lat, lat_off)                # (training-mode BatchNorm sums are float atomics: two half passes agree to rounding)
        print(f'[half guard conv] clean encoder: guarded vs off rel {e:.2e}')
        assert bool(torch.isfinite(lat).all()) and e < 1e-3
        return
    assert not bool(torch.isfinite(lat_off).all()), 'the case does not overflow: it shows nothing'
    with _half('raise'), pytest.raises(WmzError, match='SimpleResidualEncoder.*conv activation'):
        mraise.encoder.forward_nhwc(fc)
    with _half('fallback'), warnings.catch_warnings(record=True) as w, recorded_calls() as seen:
        warnings.simplefilter('always')
        lat = mfb.encoder.forward_nhwc(fc)
        tok = mfb.vq.encode(lat.float())
    assert len([x for x in w if 'IEEE half' in str(x.message)]) == 1
    assert any(n in HALF_CONV for n in seen) and any(n.startswith('wmz_conv2d_nhwc_fwd') for n in seen), set(seen)
    assert lat.dtype == torch.float32 and bool(torch.isfinite(lat).all())
    e32 = rel(lat, lat32)
    print(f'[half guard conv] encoder fallback vs a separate fp32 pass: rel {e32:.2e}')
    assert e32 < TOL_FP32, e32
    assert float((tok != m32.vq.encode(lat32)).float().mean()) < 1e-3
    assert _same_state(mfb, m32, exact=False), 'running statistics: those of ONE fp32 pass'
    # against the oracle: the fp32 bound, or 4 x the oracle's own float32-against-float64 distance where 1e-5 is missed
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    ref = oae.encoder_forward({k: v.clone() for k, v in sd.items()}, frames, training=True).permute(0, 2, 3, 1)
    e = rel(lat, ref)
    tol = TOL_FP32
    if e >= tol:
        ref64 = oae.encoder_forward({k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}, frames.double(),
                                    training=True).permute(0, 2, 3, 1)
        own = rel(ref, ref64)
        tol = 4 * own
        print(f'[half guard conv] encoder fallback rel {e:.2e} misses 1e-5; oracle f32 vs f64 {own:.2e}, bound {tol:.2e}')
    print(f'[half guard conv] encoder fallback rel {e:.2e} to the fp32 oracle (bound {tol:.2e})')
    assert e < tol, (e, tol)


@pytest.mark.parametrize('training', [False, True], ids=['eval', 'train'])
@pytest.mark.parametrize('scale', [1e6, 1.0], ids=['latents-x1e6', 'latents'])
def test_decoder(scale, training):
    from world_modelz_amd._lib import WmzError
    m = _vqae(63, training)
    torch.manual_seed(64)
    lat = (torch.randn(8, 16, 16, 64) * scale).cuda()
    m32, m32b, moff, mraise, mfb = (copy.deepcopy(m) for _ in range(5))
    with _fp32():
        y32 = m32.decoder.forward_nhwc(lat)
        print(f'[half guard conv] decoder (training={training}), fp32 vs fp32 on identical copies: rel {rel(m32b.decoder.forward_nhwc(lat), y32):.2e}')
    with _half('off'), recorded_calls() as seen_off:
        y_off = moff.decoder.forward_nhwc(lat)
    assert all(n in seen_off for n in HALF_CONV) and not any('half_guard' in n for n in seen_off), set(seen_off)
    if scale == 1.0:
        with _half('raise'):
            y = mraise.decoder.forward_nhwc(lat)
        e = rel(y, y_off)
        print(f'[half guard conv] clean decoder (training={training}): guarded vs off rel {e:.2e}')
        assert bool(torch.isfinite(y).all()) and (torch.equal(y, y_off) if not training else e < 1e-3)
        return
    assert not bool(torch.isfinite(y_off).all()), 'the case does not overflow: it shows nothing'
    with _half('raise'), pytest.raises(WmzError, match='SimpleResidualDecoder.*conv activation'):
        mraise.decoder.forward_nhwc(lat)
    with _half('fallback'), warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        y = mfb.decoder.forward_nhwc(lat)
    assert len([x for x in w if 'IEEE half' in str(x.message)]) == 1
    e32 = rel(y, y32)
    print(f'[half guard conv] decoder (training={training}) fallback vs a separate fp32 pass: rel {e32:.2e}')
    assert bool(torch.isfinite(y).all())
    assert torch.equal(y, y32) if not training else e32 < TOL_FP32, e32          # eval: deterministic route, bit for bit
    assert _same_state(mfb, m32, exact=not training)
