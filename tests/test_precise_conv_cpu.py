"""Build-time checks of the half conv units (csrc/conv_direct_f16.hip, conv_point_f16.hip) and host checks of the precise conv
route's rule (autoencoder.conv_route; the library loads on a CPU-only host)."""
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'world_modelz_amd', 'csrc')
HIPCC = '/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else shutil.which('hipcc')


def _kernel_budgets(units):
    """{unit: {kernel: (VGPRs incl. AGPRs, scratch bytes)}} of the device ISA of each unit, compiled in parallel."""
    procs = {u: subprocess.Popen([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only',
                                  os.path.join(CSRC, u), '-o', '-'], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
             for u in units}
    out = {}
    for u, p in procs.items():
        asm, _ = p.communicate(timeout=900)
        assert p.returncode == 0, u
        ker = {}
        for m in re.finditer(r'^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)\.end_amdhsa_kernel', asm, flags=re.S | re.M):
            body = m.group(2)
            g = lambda k: int(re.search(r'\.' + k + r'\s+(\d+)', body).group(1))
            ker[m.group(1)] = (g('amdhsa_next_free_vgpr'), g('amdhsa_private_segment_fixed_size'))
        out[u] = ker
    return out


@pytest.mark.skipif(HIPCC is None, reason='hipcc not available')
def test_half_conv_units_keep_the_bf16_register_budgets():
    """Every half instantiation of convr_kernel / convp_kernel keeps its bfloat16 form's register budget (the launch bounds are the
    same source), the stride-2 convr_kernel <= 168 VGPRs (three workgroups per CU), and spills nothing: zero scratch wherever the
    bfloat16 form has none.  (The bfloat16 stride-1 Cout-128 convr_kernel forms carry a 16-byte spill of their own -- 256
    registers, outside this change; their half forms may not exceed it.)  The half units hold no format-agnostic kernel: the
    weight packs and wmz_nchw_to_nhwc8 exist once, in the bfloat16 units."""
    b = _kernel_budgets(['conv_direct.hip', 'conv_direct_f16.hip', 'conv_point.hip', 'conv_point_f16.hip'])
    for bf, hf, n in (('conv_direct.hip', 'conv_direct_f16.hip', 14), ('conv_point.hip', 'conv_point_f16.hip', 4)):
        half = b[hf]
        assert len(half) == n and all('convr_kernel' in k or 'convp_kernel' in k for k in half), sorted(half)
        for k, (v, scratch) in half.items():
            v0, scratch0 = b[bf][k]
            assert v <= v0, (k, v, v0)
            assert scratch <= scratch0 and (scratch0 > 0 or scratch == 0), (k, scratch, scratch0)
            if re.search(r'convr_kernelILi4ELi16ELi[12]ELi2E', k):              # <NCB 4, TW 16, NPASS, STRIDE 2>
                assert v <= 168 and scratch == 0, (k, v)
    assert sum(1 for k in b['conv_direct_f16.hip'] if re.search(r'ELi2EEEvNS_12DirectParams', k)) == 2


@pytest.mark.skipif(HIPCC is None, reason='hipcc not available')
def test_half_direct_conv_never_touches_loads_in_flight():
    """tools/check_untracked_conv.py on the half unit (conv_direct.hip compiled with WMZ_OP16_F16, what conv_direct_f16.hip is):
    no instruction touches an inline-asm load's destination registers before the wait that retires it, in all 14 instantiations."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'check_untracked_conv.py'), '-DWMZ_OP16_F16=1'],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count('touches before their waits: 0') == 14, r.stdout


def test_half_conv_entry_points_are_declared_and_bound():
    import abi_header
    from world_modelz_amd import _lib
    lib = _lib.lib()
    for n in ('wmz_conv3x3_direct_fwd_strided_f16', 'wmz_conv_point_fwd_bn_f16'):
        abi_header.assert_bound(lib, n)
        assert _lib.SIGNATURES[n] == _lib.SIGNATURES[n[:-4]], n
    assert lib.wmz_version() == _lib.EXPECTED_VERSION == 115
    # the half forms share the bfloat16 units' format-agnostic entry points: one of each
    for n in ('wmz_conv3x3_direct_fwd_strided_f16', 'wmz_conv_point_fwd_bn_f16', 'wmz_nchw_to_nhwc8', 'wmz_conv3x3_direct_pack'):
        assert hasattr(lib, n), n
    for n in ('wmz_conv3x3_direct_pack_f16', 'wmz_conv_point_pack_f16', 'wmz_nchw_to_nhwc8_f16', 'wmz_debug_conv_knobs_f16'):
        assert not hasattr(lib, n), n
    # element-wise entry points that now take WMZ_F16
    assert lib.wmz_affine_act_bn_supported(64, _lib.WMZ_F16) == 1 and lib.wmz_affine_act_bn_supported(64, 3) == 0


def _encoder_and_decoder(hidden=128, training=True):
    from world_modelz_amd.train_vqae import VqAutoEncoder
    m = VqAutoEncoder(embedding_dim=64, num_embeddings=32, downscale_steps=2, hidden_planes=hidden)
    m.train(training)
    return m


def test_conv_route_rule():
    """autoencoder.conv_route: half only in the precise mode with the switch on, without a gradient path, and only when every
    convolution of the pass has a half kernel; otherwise the compute dtype (fp32 in the precise mode) for the whole pass."""
    from world_modelz_amd import config
    from world_modelz_amd.autoencoder import conv_route
    frames, lat = (32, 3, 64, 64), (32, 16, 16, 64)
    m = _encoder_and_decoder()
    assert not config.get_precise_conv()                            # default off (WMZ_PRECISE_CONV unset)
    for mode, switch, want in ((torch.bfloat16, False, torch.bfloat16), (torch.bfloat16, True, torch.bfloat16),
                               (torch.float32, True, torch.float32), (torch.float16, False, torch.float32),
                               (torch.float16, True, torch.float16)):
        with config.compute_dtype(mode), config.precise_conv(switch):
            assert conv_route(m.encoder, frames) == want, (mode, switch)
            assert conv_route(m.decoder, lat) == want, (mode, switch)
            assert conv_route(m.encoder, frames, grad=True) == config.get_compute_dtype()
    with config.compute_dtype(torch.float16), config.precise_conv(True):
        # off the half kernels: hidden 96 (stride-2 3x3 at Cout 96; K = 576 beyond the streaming kernel), a plane off the direct
        # kernel's tiles, an eval-mode encoder (its 1x1 carries the skip add: implicit-GEMM only)
        m96 = _encoder_and_decoder(hidden=96)
        assert conv_route(m96.encoder, frames) == torch.float32 and conv_route(m96.decoder, lat) == torch.float32
        assert conv_route(m.encoder, (32, 3, 40, 40)) == torch.float32
        assert conv_route(_encoder_and_decoder(training=False).encoder, frames) == torch.float32
        assert conv_route(_encoder_and_decoder(training=False).decoder, lat) == torch.float16
        with pytest.raises(TypeError):
            conv_route(m, frames)
