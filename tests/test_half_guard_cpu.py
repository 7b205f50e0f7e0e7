"""Host-side checks of the half guard (config.half_guard; DESIGN 4.7 "Range"): the policy plumbing, the C ABI, and the register
budgets of the half denoiser units against the parent commit's build."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'world_modelz_amd', 'csrc')
HIPCC = '/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else shutil.which('hipcc')


def test_policy_plumbing():
    from world_modelz_amd import config
    assert config.get_half_guard() == 'off'                          # default (WMZ_HALF_GUARD unset)
    with config.half_guard('raise'):
        assert config.get_half_guard() == 'raise'
        with config.half_guard('fallback'):
            assert config.get_half_guard() == 'fallback'
        assert config.get_half_guard() == 'raise'
    assert config.get_half_guard() == 'off'
    with pytest.raises(RuntimeError):
        with config.half_guard('fallback'):
            raise RuntimeError('x')
    assert config.get_half_guard() == 'off'                          # restored on the way out of an exception
    for bad in ('on', 'warn', '', None, 1):
        with pytest.raises(ValueError):
            config.set_half_guard(bad)
    assert config.get_half_guard() == 'off'
    config.set_half_guard('raise')
    config.set_half_guard('off')


def test_policy_from_the_environment():
    import sys
    code = 'from world_modelz_amd import config; print(config.get_half_guard())'
    for val, want in (('fallback', 'fallback'), ('RAISE', 'raise'), ('off', 'off')):
        r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, WMZ_HALF_GUARD=val))
        assert r.returncode == 0 and r.stdout.strip() == want, (val, r.stdout, r.stderr[-300:])
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, WMZ_HALF_GUARD='maybe'))
    assert r.returncode != 0 and 'ValueError' in r.stderr


def test_guard_off_or_not_precise_wants_nothing():
    """half_guard.wanted() without a GPU: off by default; on only in the precise mode."""
    import torch
    from world_modelz_amd import config, half_guard
    assert not half_guard.wanted()
    with config.half_guard('raise'):
        for mode in (torch.bfloat16, torch.float32):
            with config.compute_dtype(mode):
                assert not half_guard.wanted()
    assert half_guard.describe(1) == 'the residual stream' and half_guard.describe(3) == 'the residual stream and q / k | v'
    assert half_guard.describe(4) == 'a conv activation'


def test_guard_entry_points_are_declared_exported_and_bound():
    import abi_header
    from world_modelz_amd import _lib, half_guard
    lib = _lib.lib()
    for n in ('wmz_half_guard_bind', 'wmz_half_guard_clear'):
        abi_header.assert_bound(lib, n)
        assert not any(s in n for s in ('layer_fused', 'layer_chain', 'embed_qkv_fused'))
    assert lib.wmz_version() == _lib.EXPECTED_VERSION == 115           # the guard adds entry points, changes none
    kinds = abi_header.constants('WMZ_HG_')
    assert list(kinds) == ['WMZ_HG_STREAM', 'WMZ_HG_QKV', 'WMZ_HG_CONV']
    assert tuple(kinds.values()) == tuple(b for b, _ in half_guard.KINDS) == (1, 2, 4)


# (VGPRs incl. AGPRs, scratch bytes) of every kernel of the half denoiser units in the PARENT commit's build (dee100e), taken with
# the extraction below (hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only) before the guard went into the sources
# (the three pack kernels whose argument types csrc/fused_pack_rows.h renamed keep that build's figures under their new names)
PARENT = {
    ('layer_fused_f16.hip', '_ZN12_GLOBAL__N_117fused_pack_kernelENS_8PackRowsE'): (36, 0),
    ('layer_fused_f16.hip', '_ZN12_GLOBAL__N_121fused_pack_vec_kernelENS_7VecJobGEiii'): (14, 0),
    ('layer_fused_f16.hip', '_ZN12_GLOBAL__N_123fused_pack_table_kernelEPK12FusedPackRowil'): (37, 0),
    ('layer_fused_f16.hip', '_ZN12_GLOBAL__N_127fused_pack_vec_table_kernelEPKNS_7VecJobGEiii'): (14, 0),
    ('layer_fused_f16.hip', '_ZN12_GLOBAL__N_118layer_fused_kernelILi256ELi128ELi256ELb1ELb1EEEvNS_11FusedParamsE'): (254, 0),
    ('layer_fused_f16.hip', '_ZN12_GLOBAL__N_118layer_fused_kernelILi256ELi128ELi256ELb1ELb0EEEvNS_11FusedParamsE'): (254, 0),
    ('layer_fused_f16.hip', '_ZN12_GLOBAL__N_118layer_fused_kernelILi256ELi128ELi256ELb0ELb1EEEvNS_11FusedParamsE'): (220, 0),
    ('layer_chain_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi96ELi128ELi256ELi256ELb1ELb1ELb0EEEvNS_11ChainParamsE'): (169, 0),
    ('layer_chain_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi96ELi128ELi256ELi256ELb1ELb0ELb0EEEvNS_11ChainParamsE'): (169, 0),
    ('layer_chain_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi96ELi128ELi256ELi256ELb0ELb1ELb0EEEvNS_11ChainParamsE'): (169, 0),
    ('layer_chain_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi384ELi128ELi512ELi64ELb1ELb1ELb0EEEvNS_11ChainParamsE'): (246, 0),
    ('layer_chain_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi384ELi128ELi512ELi64ELb1ELb0ELb0EEEvNS_11ChainParamsE'): (242, 0),
    ('layer_chain_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi384ELi128ELi512ELi64ELb0ELb1ELb0EEEvNS_11ChainParamsE'): (202, 0),
    ('layer_chain_g1_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi128ELi192ELi256ELi64ELb1ELb1ELb0EEEvNS_11ChainParamsE'): (169, 0),
    ('layer_chain_g1_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi128ELi192ELi256ELi64ELb1ELb0ELb0EEEvNS_11ChainParamsE'): (169, 0),
    ('layer_chain_g1_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi128ELi192ELi256ELi64ELb0ELb1ELb0EEEvNS_11ChainParamsE'): (169, 0),
    ('layer_chain_g1_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi128ELi128ELi256ELi64ELb1ELb1ELb0EEEvNS_11ChainParamsE'): (169, 0),
    ('layer_chain_g1_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi128ELi128ELi256ELi64ELb1ELb0ELb0EEEvNS_11ChainParamsE'): (169, 0),
    ('layer_chain_g1_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi128ELi128ELi256ELi64ELb0ELb1ELb0EEEvNS_11ChainParamsE'): (169, 0),
    ('layer_chain_g1_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi128ELi128ELi512ELi64ELb1ELb1ELb0EEEvNS_11ChainParamsE'): (169, 0),
    ('layer_chain_g1_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi128ELi128ELi512ELi64ELb1ELb0ELb0EEEvNS_11ChainParamsE'): (169, 0),
    ('layer_chain_g1_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi128ELi128ELi512ELi64ELb0ELb1ELb0EEEvNS_11ChainParamsE'): (169, 0),
    ('layer_chain_g2_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi192ELi128ELi512ELi128ELb1ELb1ELb0EEEvNS_11ChainParamsE'): (198, 0),
    ('layer_chain_g2_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi192ELi128ELi512ELi128ELb1ELb0ELb0EEEvNS_11ChainParamsE'): (195, 0),
    ('layer_chain_g2_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi192ELi128ELi512ELi128ELb0ELb1ELb0EEEvNS_11ChainParamsE'): (169, 0),
    ('layer_chain_g2_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi256ELi128ELi512ELi32ELb1ELb1ELb0EEEvNS_11ChainParamsE'): (182, 0),
    ('layer_chain_g2_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi256ELi128ELi512ELi32ELb1ELb0ELb0EEEvNS_11ChainParamsE'): (169, 0),
    ('layer_chain_g2_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi256ELi128ELi512ELi32ELb0ELb1ELb0EEEvNS_11ChainParamsE'): (169, 0),
    ('layer_chain_g2_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi256ELi128ELi1024ELi32ELb1ELb1ELb0EEEvNS_11ChainParamsE'): (182, 0),
    ('layer_chain_g2_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi256ELi128ELi1024ELi32ELb1ELb0ELb0EEEvNS_11ChainParamsE'): (169, 0),
    ('layer_chain_g2_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi256ELi128ELi1024ELi32ELb0ELb1ELb0EEEvNS_11ChainParamsE'): (169, 0),
    ('layer_chain_g3_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi256ELi256ELi256ELi32ELb1ELb1ELb0EEEvNS_11ChainParamsE'): (214, 0),
    ('layer_chain_g3_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi256ELi256ELi256ELi32ELb1ELb0ELb0EEEvNS_11ChainParamsE'): (169, 0),
    ('layer_chain_g3_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi256ELi256ELi256ELi32ELb0ELb1ELb0EEEvNS_11ChainParamsE'): (186, 0),
    ('layer_chain_g3_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi256ELi256ELi512ELi32ELb1ELb1ELb0EEEvNS_11ChainParamsE'): (214, 0),
    ('layer_chain_g3_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi256ELi256ELi512ELi32ELb1ELb0ELb0EEEvNS_11ChainParamsE'): (169, 0),
    ('layer_chain_g3_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi256ELi256ELi512ELi32ELb0ELb1ELb0EEEvNS_11ChainParamsE'): (186, 0),
    ('layer_chain_g3_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi256ELi256ELi1024ELi32ELb1ELb1ELb0EEEvNS_11ChainParamsE'): (214, 0),
    ('layer_chain_g3_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi256ELi256ELi1024ELi32ELb1ELb0ELb0EEEvNS_11ChainParamsE'): (169, 0),
    ('layer_chain_g3_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi256ELi256ELi1024ELi32ELb0ELb1ELb0EEEvNS_11ChainParamsE'): (186, 0),
    ('layer_chain_g3_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi512ELi128ELi1024ELi32ELb1ELb1ELb0EEEvNS_11ChainParamsE'): (256, 20),
    ('layer_chain_g3_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi512ELi128ELi1024ELi32ELb1ELb0ELb0EEEvNS_11ChainParamsE'): (250, 0),
    ('layer_chain_g3_f16.hip', '_ZN12_GLOBAL__N_118layer_chain_kernelILi512ELi128ELi1024ELi32ELb0ELb1ELb0EEEvNS_11ChainParamsE'): (250, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi128ENS_5ShapeILi4ELi4ELi2EEELi9ELb1ELb1ELb0ELb1EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (128, 32),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi64ENS_5ShapeILi4ELi4ELi2EEELi9ELb1ELb1ELb0ELb1EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (93, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi32ENS_5ShapeILi4ELi4ELi2EEELi9ELb1ELb1ELb0ELb1EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (68, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi128ENS_5ShapeILi4ELi4ELi2EEELi9ELb0ELb1ELb0ELb1EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (128, 24),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi64ENS_5ShapeILi4ELi4ELi2EEELi9ELb0ELb1ELb0ELb1EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (91, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi32ENS_5ShapeILi4ELi4ELi2EEELi9ELb0ELb1ELb0ELb1EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (68, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi128ENS_5ShapeILi4ELi4ELi2EEELi9ELb1ELb0ELb0ELb1EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (122, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi64ENS_5ShapeILi4ELi4ELi2EEELi9ELb1ELb0ELb0ELb1EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (78, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi32ENS_5ShapeILi4ELi4ELi2EEELi9ELb1ELb0ELb0ELb1EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (54, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi128ENS_5ShapeILi4ELi4ELi2EEELi9ELb0ELb0ELb0ELb1EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (121, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi64ENS_5ShapeILi4ELi4ELi2EEELi9ELb0ELb0ELb0ELb1EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (78, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi32ENS_5ShapeILi4ELi4ELi2EEELi9ELb0ELb0ELb0ELb1EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (55, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi128ENS_5ShapeILi16ELi16ELi8EEELi9ELb1ELb1ELb0ELb1EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (128, 88),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi64ENS_5ShapeILi16ELi16ELi8EEELi9ELb1ELb1ELb0ELb1EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (106, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi32ENS_5ShapeILi16ELi16ELi8EEELi9ELb1ELb1ELb0ELb1EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (81, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi128ENS_5ShapeILi16ELi16ELi8EEELi9ELb0ELb1ELb0ELb1EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (128, 80),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi64ENS_5ShapeILi16ELi16ELi8EEELi9ELb0ELb1ELb0ELb1EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (105, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi32ENS_5ShapeILi16ELi16ELi8EEELi9ELb0ELb1ELb0ELb1EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (81, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi128ENS_5ShapeILi16ELi16ELi8EEELi9ELb1ELb0ELb0ELb1EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (125, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi64ENS_5ShapeILi16ELi16ELi8EEELi9ELb1ELb0ELb0ELb1EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (82, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi32ENS_5ShapeILi16ELi16ELi8EEELi9ELb1ELb0ELb0ELb1EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (57, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi128ENS_5ShapeILi16ELi16ELi8EEELi9ELb0ELb0ELb0ELb1EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (125, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi64ENS_5ShapeILi16ELi16ELi8EEELi9ELb0ELb0ELb0ELb1EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (82, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi32ENS_5ShapeILi16ELi16ELi8EEELi9ELb0ELb0ELb0ELb1EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (58, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi128ENS_5ShapeILi16ELi16ELi8EEELi9ELb1ELb1ELb0ELb0EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (128, 40),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi64ENS_5ShapeILi16ELi16ELi8EEELi9ELb1ELb1ELb0ELb0EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (95, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi32ENS_5ShapeILi16ELi16ELi8EEELi9ELb1ELb1ELb0ELb0EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (73, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi128ENS_5ShapeILi16ELi16ELi8EEELi9ELb0ELb1ELb0ELb0EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (128, 28),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi64ENS_5ShapeILi16ELi16ELi8EEELi9ELb0ELb1ELb0ELb0EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (93, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi32ENS_5ShapeILi16ELi16ELi8EEELi9ELb0ELb1ELb0ELb0EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (73, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi128ENS_5ShapeILi16ELi16ELi8EEELi9ELb1ELb0ELb1ELb0EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (124, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi64ENS_5ShapeILi16ELi16ELi8EEELi9ELb1ELb0ELb1ELb0EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (82, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi32ENS_5ShapeILi16ELi16ELi8EEELi9ELb1ELb0ELb1ELb0EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (58, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi128ENS_5ShapeILi16ELi16ELi8EEELi9ELb0ELb0ELb1ELb0EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (124, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi64ENS_5ShapeILi16ELi16ELi8EEELi9ELb0ELb0ELb1ELb0EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (82, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi32ENS_5ShapeILi16ELi16ELi8EEELi9ELb0ELb0ELb1ELb0EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (60, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi128ENS_5ShapeILi16ELi16ELi8EEELi9ELb1ELb0ELb0ELb0EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (124, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi64ENS_5ShapeILi16ELi16ELi8EEELi9ELb1ELb0ELb0ELb0EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (82, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi32ENS_5ShapeILi16ELi16ELi8EEELi9ELb1ELb0ELb0ELb0EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (58, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi128ENS_5ShapeILi16ELi16ELi8EEELi9ELb0ELb0ELb0ELb0EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (124, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi64ENS_5ShapeILi16ELi16ELi8EEELi9ELb0ELb0ELb0ELb0EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (82, 0),
    ('attn_fwd_row16_f16.hip', '_ZN12_GLOBAL__N_121attn_fwd_row16_kernelILi32ENS_5ShapeILi16ELi16ELi8EEELi9ELb0ELb0ELb0ELb0EEEvPK14__hip_bfloat16S5_S5_PS3_PfS7_8AttnGeomPx'): (60, 0),
    ('linear_fwd_f16.hip', '_ZN12_GLOBAL__N_113linear_kernelI14__hip_bfloat16Li1ELi64EEEvNS_9LinParamsE'): (166, 0),
    ('linear_fwd_f16.hip', '_ZN12_GLOBAL__N_113linear_kernelI14__hip_bfloat16Li2ELi64EEEvNS_9LinParamsE'): (124, 0),
    ('linear_fwd_f16.hip', '_ZN12_GLOBAL__N_113linear_kernelI14__hip_bfloat16Li0ELi64EEEvNS_9LinParamsE'): (169, 0),
    ('linear_fwd_f16.hip', '_ZN12_GLOBAL__N_113linear_kernelI14__hip_bfloat16Li1ELi128EEEvNS_9LinParamsE'): (248, 0),
    ('linear_fwd_f16.hip', '_ZN12_GLOBAL__N_113linear_kernelI14__hip_bfloat16Li2ELi128EEEvNS_9LinParamsE'): (200, 0),
    ('linear_fwd_f16.hip', '_ZN12_GLOBAL__N_113linear_kernelI14__hip_bfloat16Li0ELi128EEEvNS_9LinParamsE'): (173, 0),
    ('linear_fwd_f16.hip', '_ZN12_GLOBAL__N_113linear_kernelIfLi0ELi64EEEvNS_9LinParamsE'): (125, 0),
    ('linear_fwd_f16.hip', '_ZN12_GLOBAL__N_113linear_kernelIfLi1ELi128EEEvNS_9LinParamsE'): (202, 0),
    ('linear_fwd_f16.hip', '_ZN12_GLOBAL__N_113linear_kernelIfLi2ELi128EEEvNS_9LinParamsE'): (219, 0),
    ('linear_fwd_f16.hip', '_ZN12_GLOBAL__N_113linear_kernelIfLi0ELi128EEEvNS_9LinParamsE'): (170, 0),
}
UNITS = sorted({u for u, _ in PARENT})


def _kernel_budgets(units):
    procs = {u: subprocess.Popen([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only',
                                  os.path.join(CSRC, u), '-o', '-'], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
             for u in units}
    out = {}
    for u, p in procs.items():
        asm, _ = p.communicate(timeout=1800)
        assert p.returncode == 0, u
        for m in re.finditer(r'^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)\.end_amdhsa_kernel', asm, flags=re.S | re.M):
            body = m.group(2)
            g = lambda k: int(re.search(r'\.' + k + r'\s+(\d+)', body).group(1))
            out[(u, m.group(1))] = (g('amdhsa_next_free_vgpr'), g('amdhsa_private_segment_fixed_size'))
    return out


@pytest.mark.skipif(HIPCC is None, reason='hipcc not available')
def test_half_denoiser_units_keep_the_parents_register_budgets():
    """Every kernel of layer_fused_f16.hip, layer_chain*_f16.hip, attn_fwd_row16_f16.hip and linear_fwd_f16.hip: scratch no larger,
    and VGPRs no more, than the parent commit's build of the same kernel; no kernel crosses 128 or 256 registers; no kernel added.

    Figures of this commit: all 95 kernels meet the bound (layer_fused_f16 254 -> 252, three g3 chain kernels 214 -> 210, the
    rest equal; attn_fwd_row16_f16 and linear_fwd_f16 are untouched).  The chain check holds no VGPR of its own (a compare of the
    fp32 value into a scalar mask), and the commit computes its lane test at the kernel's end: a lane id carried from the
    prologue stayed live across the GEMMs and cost eight chain instantiations 1-2 registers."""
    now = _kernel_budgets(UNITS)
    assert set(now) == set(PARENT), sorted(set(now) ^ set(PARENT))
    over = []
    for k, (v0, s0) in sorted(PARENT.items()):
        v, s = now[k]
        assert s <= s0, (k, 'scratch', s, s0)
        for step in (128, 256):
            assert not (v0 <= step < v), (k, 'crosses', step, v, v0)
        if v > v0:
            over.append((k[0], k[1][:70], v, v0))
    assert not over, over
