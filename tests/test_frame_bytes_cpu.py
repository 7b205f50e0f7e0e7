"""Byte frames in and out, the host side: the two laws of csrc/frame_bytes.h, run from the header itself by
tests/frame_bytes_host.cpp, against what the reference computes with torch on the CPU (frame_bytes_cases.py) -- byte / 255 by IEEE
division on the way in, save_image's mul(255).add_(0.5).clamp_(0, 255).to(uint8) on the way out -- and the declarations of the two
entry points that apply them on the GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import abi_header
import frame_bytes_cases as fb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'frame_bytes_host.cpp')
CXX = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/llvm/bin/clang++')
            if c and os.path.exists(c)), None)
needs_cxx = pytest.mark.skipif(CXX is None, reason='no host C++ compiler available')


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('frame_bytes') / 'frame_bytes_host')
    # (-ffp-contract=off: the header's pragma is clang's; the law's multiply and add are two roundings under any compiler)
    r = subprocess.run([CXX, '-std=c++17', '-O2', '-ffp-contract=off', '-Wall', '-Werror', SRC, '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]

    def run(mode, values=None):
        data = b'' if values is None else values.contiguous().numpy().astype('<f4', copy=False).tobytes()
        out = subprocess.run([exe, mode], input=data, capture_output=True)
        assert out.returncode == 0, (out.returncode, out.stderr)
        return out.stdout
    return run


def units(host):
    return torch.from_numpy(np.frombuffer(host('unit'), dtype='<f4').copy())


def to_bytes(host, values):
    """frame_unit_to_byte of every element of an fp32 CPU tensor."""
    got = np.frombuffer(host('byte', values.reshape(-1)), dtype=np.uint8)
    assert got.size == values.numel()
    return torch.from_numpy(got.copy()).view(values.shape)


@needs_cxx
def test_every_byte_goes_to_the_ieee_quotient(host):
    """frame_byte_to_unit(b) is np.float32(b) / np.float32(255), which is what torch computes, for all 256 bytes -- and is NOT the
    product with fl(1 / 255) (that the two differ is why the law is stated as a division)."""
    got = units(host)
    b = np.arange(256, dtype=np.float32)
    want = b / np.float32(255)
    assert got.dtype == torch.float32 and got.shape == (256,)
    assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))
    assert torch.equal(got, fb.unit_of_bytes(torch.arange(256, dtype=torch.uint8)))
    assert int((want != b * (np.float32(1) / np.float32(255))).sum()) == 126


@needs_cxx
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_every_16_bit_pattern_goes_to_the_byte_of_the_torch_law(host, dtype):
    """All 65 536 patterns of the operand format, taken to fp32 exactly: negatives, -0.0, values beyond 1, +-inf (0 / 255 through the
    clamp) and every NaN (0, by this project's definition)."""
    x = fb.all_patterns(dtype).float()
    got, want = to_bytes(host, x), fb.bytes_of_units(x)
    assert torch.equal(got, want), (dtype, x[got != want][:8], got[got != want][:8], want[got != want][:8])
    assert int(got[x.isnan()].max()) == 0 and int(got[x == float('inf')].min()) == 255 and int(got[x == -float('inf')].max()) == 0
    assert len(torch.unique(got)) == 256


@needs_cxx
def test_fp32_rounding_boundaries_go_to_the_byte_of_the_torch_law(host):
    x = fb.fp32_boundaries()
    got, want = to_bytes(host, x), fb.bytes_of_units(x)
    assert torch.equal(got, want), (x[got != want][:8], got[got != want][:8], want[got != want][:8])
    # the set does straddle boundaries: hundreds of its values land on another byte than their lower neighbour
    n = 3 * 256
    assert int((got[:n] != got[2 * n:3 * n]).sum()) > 256
    assert int(got[x.isnan()].max()) == 0


@needs_cxx
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
def test_byte_to_unit_to_operand_format_to_byte_is_the_identity(host, dtype):
    """A frame that goes in as bytes, is rounded to nearest even into the operand format (the cast behind frame_byte_to_unit) and
    comes straight back out is the frame: all 256 bytes, in all three formats."""
    back = to_bytes(host, units(host).to(dtype).float())
    assert torch.equal(back, torch.arange(256, dtype=torch.uint8))


def squeeze(s):
    return ' '.join(s.replace('\n', ' ').split())


def test_entry_points_are_declared_with_the_agreed_argument_lists():
    from world_modelz_amd import _lib
    vp, i, l = _lib.c_void_p, _lib.c_int, _lib.c_long
    assert squeeze(abi_header.arguments('wmz_frames_u8_to_nhwc8')) == (
        'const void* x, void* y, long N, int C, int H, int W, long frame_stride, int channels_last, int out_dtype, void* stream')
    assert squeeze(abi_header.arguments('wmz_nhwc8_to_frames_u8')) == (
        'const void* y, void* out, long N, int C, int H, int W, int channels_last, int in_dtype, void* stream')
    assert _lib.DECLARATIONS['wmz_frames_u8_to_nhwc8'] == (i, [vp, vp, l, i, i, i, l, i, i, vp])
    assert _lib.DECLARATIONS['wmz_nhwc8_to_frames_u8'] == (i, [vp, vp, l, i, i, i, i, i, vp])
    abi_header.assert_bound(_lib.lib(), 'wmz_frames_u8_to_nhwc8', 'wmz_nhwc8_to_frames_u8')
    text = abi_header.text()
    for line in ('main2.py:51-56', 'minecraft/sparse_diffusion.py:23-28', 'main.py:121-132'):       # the reference lines replaced
        assert line in text, line


def test_cpu_tensors_and_wrong_inputs_are_refused():
    from world_modelz_amd import ops
    from world_modelz_amd._lib import WmzError
    from world_modelz_amd.train_vqae import VqAutoEncoder
    with pytest.raises(WmzError):
        ops.frames_u8_to_nhwc8(torch.zeros(2, 4, 4, 3, dtype=torch.uint8), torch.float32)
    with pytest.raises(WmzError):
        ops.nhwc8_to_frames_u8(torch.zeros(2, 4, 4, 8), 3)
    ae = VqAutoEncoder(embedding_dim=8, num_embeddings=8, downscale_steps=1, hidden_planes=8)
    with pytest.raises(WmzError):
        ae.encode_frames(torch.zeros(2, 3, 4, 4))                                  # float frames: encode's business
    with pytest.raises(WmzError):
        ae.encode_frames(torch.zeros(2, 4, 4, 3, dtype=torch.uint8))               # CPU bytes


def test_uniform_frame_stride_is_found_or_refused():
    """ops._uniform_frame_stride: the one stride the C entry point can take, or None (then the wrapper copies)."""
    from world_modelz_amd.ops import _uniform_frame_stride as ufs
    F = 4 * 5 * 3
    x = torch.zeros(6, 7, 4, 5, 3, dtype=torch.uint8)
    assert ufs(x, 2) == F and ufs(x[0], 1) == F and ufs(x[0, 0], 0) == F
    assert ufs(x[:, 1], 1) == 7 * F and ufs(x[:, 6:], 2) == 7 * F and ufs(x[:, ::2], 2) is None and ufs(x[2:, :], 2) == F
    assert ufs(x[:1, 1:], 2) == F and ufs(x[:, 1:], 2) is None                     # two strides: no single one
    assert ufs(x[..., 1:, :], 2) is None and ufs(x.permute(0, 1, 4, 2, 3), 2) is None     # frames not contiguous each
    assert ufs(x[:, :1].expand(6, 3, 4, 5, 3), 2) is None                          # stride 0: frames overlap
    assert ufs(x.flatten()[1:1 + 5 * F].view(5, 4, 5, 3), 1) == F                  # (alignment is not its business)
