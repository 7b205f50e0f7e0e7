"""The time window (back, fwd) of the attention kernels, everything that can be checked without a GPU: the asymmetric slab walk
of csrc/attn_slab_walk.h (compiled into tests/causal_window_host.cpp by the host compiler and compared with the law restated here),
the two C entry points as the binding reads them from include/wmz.h, the `causal` keyword of the three constructors, the
`time_window` keyword of ops, checkpoint.build_denoiser's reading of opt.causal, and the reference tests/causal_ref.py itself."""
import argparse
import inspect
import os
import shutil
import subprocess

import pytest
import torch

import causal_ref
from oracle import attention as oat
from oracle import denoiser as oden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'causal_window_host.cpp')
CXX = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/llvm/bin/clang++')
            if c and os.path.exists(c)), None)
needs_cxx = pytest.mark.skipif(CXX is None, reason='no host C++ compiler available')

SHAPES = {'big': (16, 16, 8), 'small': (4, 4, 2)}        # NW, CH, KC (as in test_attn_slab_walk_cpu.py)
GEOMS = [(16, 3, 'big'),        # whole 16-row planes: the clamped and the whole-plane form
         (5, 1, 'big'),         # ragged, idle waves
         (21, 2, 'big'),        # two workgroups
         (3, 1, 'small'), (8, 2, 'small')]


@pytest.fixture(scope='module')
def walks(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('causal_window') / 'causal_window_host')
    r = subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror', SRC, '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]

    def run(H, eHv, shape):
        out = subprocess.run([exe, str(H), str(eHv), shape], capture_output=True, text=True)
        assert out.returncode == 0, (out.returncode, out.stderr)
        wgs = []
        for line in out.stdout.split('\n'):
            f = line.split()
            if f and f[0] == 'wg':
                keys = ('H', 'S', 'b', 'f', 's', 'og', 'sk_lo', 'sk_hi', 'nch', 'nslab', 'p_first', 'same')
                wgs.append(dict(zip(keys, map(int, f[2:])), form=f[1], slabs=[]))
            elif f:
                assert f[0] == 'slab'
                wgs[-1]['slabs'].append((int(f[1]), int(f[2])))
        return wgs
    return run


@needs_cxx
@pytest.mark.parametrize('geom', GEOMS, ids=lambda g: '-'.join(map(str, g)))
def test_asymmetric_walk_stages_exactly_the_window(walks, geom):
    """Every S <= 6, b, f <= 4, query plane and workgroup: the planes staged are max(0, s - b) .. min(S - 1, s + f), each plane's
    slabs exactly once and plane after plane, starting at the window's plane with S - 1 - p = 0 (mod b + f + 1) -- the rotation
    that keeps the workgroups sharing a plane in step -- or at its first plane where the clip cuts that one off."""
    H, eHv, shape = geom
    NW, CH, KC = SHAPES[shape]
    wgs = walks(*geom)
    forms = 1 + (shape == 'big' and H % 16 == 0)
    assert len(wgs) == forms * sum(S for S in range(1, 7)) * 25 * -(-H // NW)
    for w in wgs:
        S, b, f, s = w['S'], w['b'], w['f'], w['s']
        lo, hi = max(0, s - b), min(S - 1, s + f)
        assert (w['sk_lo'], w['sk_hi']) == (lo, hi), w
        start = next(p for p in range(s - b, s + f + 1) if (S - 1 - p) % (b + f + 1) == 0)
        if not lo <= start <= hi:
            start = lo
        planes = list(range(start, hi + 1)) + list(range(lo, start))
        assert w['p_first'] == start
        owners = range(w['og'] * NW, min(w['og'] * NW + NW, H))
        rows = range(max(0, owners[0] - eHv), min(H - 1, owners[-1] + eHv) + 1)
        slabs = [(c * CH + ph) for c in range(rows[0] // CH, rows[-1] // CH + 1) for ph in range(CH // KC)]
        assert w['nch'] == len(slabs) and w['nslab'] == len(planes) * len(slabs)
        assert w['slabs'] == [(p, base) for p in planes for base in slabs], w          # each (plane, slab) once, in this order


@needs_cxx
@pytest.mark.parametrize('geom', GEOMS, ids=lambda g: '-'.join(map(str, g)))
def test_old_overloads_are_the_symmetric_case(walks, geom):
    """slab_geom / slab_first_plane with one eS equal the (eS, eS) case of the new overloads, field for field."""
    wgs = walks(*geom)
    sym = [w for w in wgs if w['b'] == w['f']]
    assert sym and all(w['same'] == 1 for w in sym)
    assert all(w['same'] == -1 for w in wgs if w['b'] != w['f'])


@needs_cxx
def test_trailing_planes_walk_like_the_whole_clip_causal(walks):
    """A causal clip cut down to its trailing planes (the last-frame cone): a query plane whose window survives the cut visits the
    same planes in the same order -- the phase counts from the clip's end."""
    wgs = [w for w in walks(16, 3, 'big') if w['f'] == 0]
    by = {(w['form'], w['S'], w['b'], w['s'], w['og']): w for w in wgs}
    compared = 0
    for w in wgs:
        for d in range(1, 6 - w['S'] + 1):
            full = by[(w['form'], w['S'] + d, w['b'], w['s'] + d, w['og'])]
            if w['s'] + d - w['b'] >= d:
                assert [(p + d, base) for p, base in w['slabs']] == full['slabs']
                compared += 1
    assert compared > 0


def test_entry_points_are_declared():
    from world_modelz_amd import _lib
    vp, i, l = _lib.c_void_p, _lib.c_int, _lib.c_long
    assert _lib.SIGNATURES['wmz_local3d_attn_fwd_window'] == [vp] * 6 + [i] * 10 + [l] * 4 + [i] * 4 + [vp]
    assert _lib.SIGNATURES['wmz_local3d_attn_bwd_window'] == [vp] * 10 + [i] * 10 + [l] * 8 + [i] * 2 + [vp]
    # the symmetric entry points are declared as before
    assert _lib.SIGNATURES['wmz_local3d_attn_fwd'] == [vp] * 6 + [i] * 9 + [l] * 4 + [i, vp]
    assert _lib.SIGNATURES['wmz_local3d_attn_fwd_planes'] == [vp] * 5 + [i] * 9 + [l] * 4 + [i] * 3 + [vp]
    assert _lib.SIGNATURES['wmz_local3d_attn_bwd'] == [vp] * 10 + [i] * 9 + [l] * 8 + [i, vp]


def test_constructors_accept_and_keep_causal():
    from world_modelz_amd.local_3d_attention import Local3dAttention, Local3dAttentionTransformer
    from world_modelz_amd.main import VqVideoDiffusionModel
    for cls in (Local3dAttention, Local3dAttentionTransformer, VqVideoDiffusionModel):
        params = list(inspect.signature(cls.__init__).parameters.values())
        assert params[-1].name == 'causal' and params[-1].default is False, cls          # trailing, off by default
    assert [p.name for p in inspect.signature(Local3dAttention.__init__).parameters.values()] == \
        ['self', 'extents', 'dim', 'heads', 'dim_head', 'dropout', 'use_checkpointing', 'causal']
    kw = dict(data_shape=(3, 4, 4), dim=32, num_classes=16, extents=(2, 1, 1), depth=2, dim_head=16, mlp_dim=32, heads=2)
    sym, cau = VqVideoDiffusionModel(**kw), VqVideoDiffusionModel(**kw, causal=True)
    assert sym.causal is False and sym.transformer.causal is False and cau.causal is True and cau.transformer.causal is True
    assert all(a.fn.causal is False and a.fn.time_window is None for a, _ in sym.transformer.layers)
    assert all(a.fn.causal is True and a.fn.time_window == (2, 0) for a, _ in cau.transformer.layers)
    assert list(sym.state_dict()) == list(cau.state_dict())                             # no new keys
    att = Local3dAttention((1, 2, 3), 32, 2, 16, .0, True, True)
    assert att.causal is True and att.time_window == (1, 0) and Local3dAttention((1, 2, 3), 32).time_window is None


def test_ops_keywords_default_to_the_symmetric_entry_points():
    from world_modelz_amd import ops
    for fn in (ops.local3d_attention_fwd, ops.local3d_attention_bwd):
        p = inspect.signature(fn).parameters['time_window']
        assert p.default is None
    assert ops.causal_window((3, 1, 1), True) == (3, 0) and ops.causal_window((3, 1, 1), False) is None


def test_build_denoiser_reads_opt_causal():
    from world_modelz_amd import checkpoint
    from world_modelz_amd.main import VqVideoDiffusionModel
    m = VqVideoDiffusionModel(data_shape=(3, 4, 4), dim=32, num_classes=16, extents=(1, 1, 1), depth=1, dim_head=16, mlp_dim=32,
                              heads=2)
    opt = argparse.Namespace(extents='1,1,1', dim=32, depth=1, mlp_dim=32, dim_head=16, heads=2, dropout=0.0)
    data = {'opt': opt, 'model_state_dict': m.state_dict(), 'ema_model_state_dict': None}
    assert checkpoint.build_denoiser(data, 16).causal is False             # a reference checkpoint: no such field
    opt.causal = True
    built = checkpoint.build_denoiser(data, 16)
    assert built.causal is True and all(a.fn.causal for a, _ in built.transformer.layers)


# ---------------------------------------------------------------------------------------------- the reference itself

def test_reference_symmetric_window_is_the_oracle():
    torch.manual_seed(0)
    ext, heads = (1, 1, 2), 2
    q, k, v = (torch.randn(2, 4, 3, 5, 16) for _ in range(3))
    out, logits = causal_ref.local_attention(k, v, q, ext, heads, window=(1, 1), return_logits=True)
    ref, ref_logits = oat.local_attention(k, v, q, ext, heads, return_logits=True)
    assert torch.allclose(out, ref, rtol=1e-6, atol=1e-6) and torch.equal(logits, ref_logits)


@pytest.mark.parametrize('window', [(2, 0), (1, 2), (0, 0), (5, 0)])
def test_reference_sees_its_window_and_nothing_else(window):
    """Edits of K, V behind the window change nothing (bit for bit), the probe's leading slots are the symmetric oracle's, and the
    gradient of plane s reaches exactly the planes s - back .. s + fwd."""
    torch.manual_seed(1)
    back, fwd = window
    ext, heads = (2, 1, 1), 1
    S = 5
    q, k, v = (torch.randn(1, S, 3, 4, 8) for _ in range(3))
    out, logits = causal_ref.local_attention(k, v, q, ext, heads, window=window, return_logits=True)
    assert logits.shape[-1] == (back + fwd + 1) * 9
    for s in range(S):
        k2, v2 = k.clone(), v.clone()
        k2[:, s + fwd + 1:] = 7.0
        v2[:, s + fwd + 1:] = float('nan')
        k2[:, :max(0, s - back)] = -3.0
        v2[:, :max(0, s - back)] = float('nan')
        assert torch.equal(causal_ref.local_attention(k2, v2, q, ext, heads, window=window)[:, s], out[:, s])
        kr = k.clone().requires_grad_(True)
        causal_ref.local_attention(kr, v, q, ext, heads, window=window)[:, s].sum().backward()
        live = [bool((kr.grad[:, p] != 0).any()) for p in range(S)]
        assert live == [max(0, s - back) <= p <= min(S - 1, s + fwd) for p in range(S)]
    if window == (2, 0):
        sym = oat.local_attention_logits(q, k, ext, heads)
        assert torch.equal(logits, sym[..., :3 * 9])


def test_reference_denoiser_has_no_look_ahead():
    from world_modelz_amd.main import VqVideoDiffusionModel
    torch.manual_seed(2)
    ext = (1, 1, 1)
    m = VqVideoDiffusionModel(data_shape=(4, 4, 4), dim=32, num_classes=16, extents=ext, depth=3, dim_head=16, mlp_dim=32, heads=2)
    sd = m.state_dict()
    z = torch.randint(0, 17, (1, 4, 4, 4))
    z2 = z.clone()
    z2[:, -1] = (z2[:, -1] + 5) % 17
    a, b = causal_ref.transformer_forward(sd, z, ext, 2), causal_ref.transformer_forward(sd, z2, ext, 2)
    assert torch.equal(a[:, :-1], b[:, :-1]) and not torch.equal(a[:, -1], b[:, -1])
    sa, sb = oden.transformer_forward(sd, z, ext, 2), oden.transformer_forward(sd, z2, ext, 2)
    assert not torch.equal(sa[:, 2], sb[:, 2])                            # (the symmetric stack does look ahead)
