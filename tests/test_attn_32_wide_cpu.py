"""Planes 32 wide on the attention row kernels, the host side: the window law in tile coordinates (csrc/attn_slab_walk.h, w32_*)
against the plain rule of the reference, run from the header itself by tests/attn_32_wide_host.cpp; what a workgroup stages in that
mode against the 16-wide walk of the same memory; and the inference routes the precise mode now takes on such planes."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'attn_32_wide_host.cpp')
CXX = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/llvm/bin/clang++')
            if c and os.path.exists(c)), None)
needs_cxx = pytest.mark.skipif(CXX is None, reason='no host C++ compiler available')

SHAPES = {'big': (16, 16, 8), 'small': (4, 4, 2)}        # NW, CH, KC


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('attn_32_wide') / 'attn_32_wide_host')
    r = subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror', SRC, '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
        assert out.returncode == 0, (out.returncode, out.stderr)
        return out.stdout
    return run


@needs_cxx
@pytest.mark.parametrize('H', [1, 2, 3, 5, 9])
def test_window_law_in_tile_coordinates_is_the_reference_rule(host, H):
    """Every query and every key token of a [H, 32] plane: "key tile row among the owner's visited rows and the column rule" is
    exactly |h' - h| <= eH and |w' - w| <= eW, and the (dh, dw) slot computed from tile coordinates is (h' - h, w' - w)."""
    tok = np.arange(H * 32)
    h, w = tok // 32, tok % 32
    for eH in (0, 1, 2, 3, H + 1):
        for eW in (0, 1, 3, 15, 16, 31, 40):
            got = np.array(host('law', H, eH, eW).split(), dtype=np.int64).reshape(-1, 4)
            q, k = got[:, 0], got[:, 1]
            assert len(np.unique(q * (H * 32) + k)) == len(got), 'a pair is admitted twice'
            admitted = np.zeros((H * 32, H * 32), dtype=bool)
            admitted[q, k] = True
            want = (np.abs(h[None, :] - h[:, None]) <= eH) & (np.abs(w[None, :] - w[:, None]) <= eW)      # [query, key]
            assert np.array_equal(admitted, want), (H, eH, eW, np.argwhere(admitted != want)[:5])
            assert np.array_equal(got[:, 2], h[k] - h[q]) and np.array_equal(got[:, 3], w[k] - w[q]), (H, eH, eW)


@needs_cxx
@pytest.mark.parametrize('H,eH,shape', [(1, 0, 'small'), (1, 2, 'small'), (3, 1, 'small'), (4, 3, 'small'), (2, 0, 'small'),
                                        (5, 2, 'big'), (8, 1, 'big'), (20, 2, 'big'), (32, 3, 'big'), (9, 10, 'big'), (16, 0, 'big')])
def test_staged_rows_cover_the_visited_ones_within_the_16_wide_walk(host, H, eH, shape):
    """The rows a workgroup stages in the 32-wide mode are among those the 16-wide walk stages for the [2H, 16] plane with the
    extent 2 eH + 1 -- no new bytes: piece_voff and the clamps are shared -- and hold every visited row of every owner."""
    NW, CH, KC = SHAPES[shape]
    wgs = []
    for line in host('walk', H, eH, shape).split('\n'):
        f = line.split()
        if not f:
            continue
        if f[0] == 'wg':
            wgs.append(dict(og=int(f[1]), owners=[]))
        elif f[0] in ('stage32', 'stage16'):
            wgs[-1][f[0]] = set(map(int, f[1:]))
        else:
            assert f[0] == 'owner'
            wgs[-1]['owners'].append(tuple(map(int, f[1:])))
    assert [g['og'] for g in wgs] == list(range(-(-2 * H // NW)))
    owners = []
    for g in wgs:
        assert g['stage32'] <= g['stage16'], (g['og'], sorted(g['stage32'] - g['stage16']))
        assert max(g['stage16']) <= 2 * H - 1
        for R, lo, hi in g['owners']:
            # the visited rows, restated from plane coordinates: both halves of the plane rows h - eH .. h + eH
            hq = R // 2
            assert (lo, hi) == (2 * max(hq - eH, 0), 2 * min(hq + eH, H - 1) + 1)
            assert set(range(lo, hi + 1)) <= g['stage32'], (g['og'], R)
            owners.append(R)
    assert owners == list(range(2 * H))


def test_precise_mode_routes_32_wide_planes_to_the_half_kernels():
    """fused.inference_route on (H, 32) planes, every width row of tests/route_table.py: the precise mode takes 'fused' / 'chain'
    exactly where it does on a 16-wide plane (it took the fp32 route, 'ops', before the row kernel had the 32-wide mode); bf16 and
    fp32 routes do not depend on the plane."""
    import route_table as rt
    from world_modelz_amd import config, fused
    from world_modelz_amd.local_3d_attention import Local3dAttentionTransformer
    some_half_route = False
    for widths in rt.WIDTHS:
        dim, heads, dh, mlp = widths
        tr = Local3dAttentionTransformer(data_shape=(3, 16, 32), dim=dim, num_classes=17, extents=(1, 1, 2), depth=2, heads=heads,
                                         dim_head=dh, mlp_dim=mlp)
        for H in (1, 3, 4, 32):
            for mode, dt in rt.MODES.items():
                for policy in ('always', 'never'):
                    prev = config.set_chain_policy(policy)
                    try:
                        got = fused.inference_route(tr, dt, H, 32, 2 * 3 * H * 32)
                        wide16 = fused.inference_route(tr, dt, H, 16, 2 * 3 * H * 32)
                    finally:
                        config.set_chain_policy(prev)
                    assert got == wide16 == rt.expected_route(widths, mode, H, 16, policy), (widths, H, mode, policy, got, wide16)
                    some_half_route |= mode == 'precise' and got in ('fused', 'chain')
        assert fused.half_attention_ok(tr, 5, 32) == (dh in rt.HALF_DIM_HEADS)
        assert not fused.half_attention_ok(tr, 4, 48) and not fused.half_attention_ok(tr, 4, 64)     # W = 32 only
    assert some_half_route
