"""The context cache's host side: the plane law (fused.context_planes) against a brute-force dependency walk, the row maps of
csrc/fused_row_maps.h -- compiled into tests/context_cache_host.cpp by the host compiler -- against a restatement kept here, and
the four entry points in include/wmz.h and in the binding derived from it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'context_cache_host.cpp')
CXX = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/llvm/bin/clang++')
            if c and os.path.exists(c)), None)

# (the half forms are the slots forms of the _f16 entry points, `_f16_slots`: tests/test_abi_binding_cpu.py pins the number of
#  declarations that END in _f16)
NEW = ('wmz_layer_fused_fwd_slots', 'wmz_layer_fused_fwd_f16_slots', 'wmz_embed_qkv_fused_fwd_slots',
       'wmz_embed_qkv_fused_fwd_f16_slots')


def walk(S, eS, depth):
    """Which context planes each layer's input stream must exist on, by walking the dependencies plane by plane.  Under the
    causal window layer l's output on plane p reads layer l's input stream on the planes max(0, p - eS) .. p (q from p itself,
    K / V from the window).  The decode step runs every layer on the generated plane g = S - 1 and so reads every layer's K / V --
    its input stream -- on the context planes of g's window."""
    g = S - 1
    need = [set() for _ in range(depth)]
    for l in range(depth):
        need[l] |= {p for p in range(max(0, g - eS), g)}
    for l in range(depth - 1, 0, -1):                  # layer l's input on p is layer l-1's output on p
        for p in sorted(need[l]):
            need[l - 1] |= set(range(max(0, p - eS), p + 1))
    return need


def test_context_planes_against_the_dependency_walk():
    from world_modelz_amd import fused
    for S in range(1, 9):
        for eS in range(0, 4):
            for depth in range(1, 6):
                a = fused.context_planes(S, eS, depth)
                need = walk(S, eS, depth)
                assert len(a) == depth
                for l in range(depth):
                    assert need[l] == set(range(S - 1 - a[l], S - 1)), (S, eS, depth, l, a, need)     # the TRAILING a[l] context planes
    assert fused.context_planes(32, 3, 4) == [12, 9, 6, 3]
    assert fused.context_planes(1, 3, 4) == [0, 0, 0, 0] and fused.context_planes(5, 0, 3) == [0, 0, 0]
    assert fused.context_planes(2, 3, 3) == [1, 1, 1]


@pytest.fixture(scope='module')
def host_lines(tmp_path_factory):
    assert CXX is not None, 'no host C++ compiler: the build machine has one (a missing compiler is a broken environment)'
    exe = str(tmp_path_factory.mktemp('context_cache') / 'context_cache_host')
    r = subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror', SRC, '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr)
    return [line.split() for line in out.stdout.split('\n') if line.strip()]


def test_destination_map_is_injective_inside_its_slots_and_the_restated_one(host_lines):
    seen = set()
    for f in host_lines:
        if f[0] != 'dst':
            continue
        B, HW, po, dp, d0, total = (int(v) for v in f[1:7])
        assert f[7] == ':'
        rows = [int(v) for v in f[8:]]
        seen.add((B, HW, po, dp, d0))
        rows_out, rows_dst, row0 = po * HW, dp * HW, d0 * HW
        assert len(rows) == B * rows_out and total == B * rows_dst
        assert rows == [(t // rows_out) * rows_dst + row0 + t % rows_out for t in range(B * rows_out)]     # row for row
        assert len(set(rows)) == len(rows)                                                                 # injective
        for t, r in enumerate(rows):                                     # inside its own clip's slots d0 .. d0 + po - 1
            c = t // rows_out
            assert c * rows_dst + row0 <= r < c * rows_dst + row0 + rows_out <= (c + 1) * rows_dst <= total
        if dp == po:                                                     # the compact layout: the identity
            assert d0 == 0 and rows == list(range(B * rows_out))
    want = {(B, HW, po, dp, d0) for B in (1, 2) for HW in (16, 80, 256) for po in (1, 3) for dp in (po, po + 1, 5)
            for d0 in range(0, dp - po + 1)}
    assert seen == want                                                  # every legal dst_plane0 of every case, nothing else


def test_source_map_and_identity_parameters(host_lines):
    n = 0
    for f in host_lines:
        if f[0] == 'src':
            B, HW, po, pi = (int(v) for v in f[1:5])
            rows = [int(v) for v in f[6:]]
            rows_out, rows_in = po * HW, pi * HW
            assert rows == [(t // rows_out) * rows_in + (rows_in - rows_out) + t % rows_out for t in range(B * rows_out)]
            if pi == po:
                assert rows == list(range(B * rows_out))
            n += 1
        elif f[0] == 'idn':
            vals = [int(v) for v in f[3:]]
            assert vals == [t for t in range(int(f[1])) for _ in range(2)]       # rows_out == 0: both maps are the identity
            n += 100
    assert n == 100 + 2 * 3 * 2 * 2


def test_what_the_entry_points_accept(host_lines):
    oks = {tuple(int(v) for v in f[1:4]): int(f[4]) for f in host_lines if f[0] == 'ok'}
    assert len(oks) > 20
    for (po, dp, d0), ok in oks.items():
        assert ok == int(d0 >= 0 and d0 + po <= dp), (po, dp, d0)
    assert oks[(1, 5, -1)] == 0 and oks[(1, 5, 5)] == 0 and oks[(3, 4, 2)] == 0 and oks[(1, 5, 4)] == 1 and oks[(3, 5, 2)] == 1


def test_header_declares_the_entry_points_and_the_binding_exposes_them():
    import abi_header
    from world_modelz_amd import _lib
    assert set(NEW) <= abi_header.declared()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
    for base, planes in (('wmz_layer_fused_fwd_slots', 'wmz_layer_fused_fwd_planes'),
                         ('wmz_embed_qkv_fused_fwd_slots', 'wmz_embed_qkv_fused_fwd_planes')):
        # the trailing-planes form's arguments, then int dst_planes, int dst_plane0 in front of the stream
        want = _lib.SIGNATURES[planes][:-1] + [_lib.c_int, _lib.c_int, _lib.c_void_p]
        assert _lib.SIGNATURES[base] == want == _lib.SIGNATURES[base[:-len('_slots')] + '_f16_slots'], base
        args = [a.split()[-1].lstrip('*') for a in abi_header.arguments(base).split(',')]
        assert args[-3:] == ['dst_planes', 'dst_plane0', 'stream']
        assert args[:-3] == [a.split()[-1].lstrip('*') for a in abi_header.arguments(planes).split(',')][:-1]
    abi_header.assert_bound(_lib.lib(), *NEW)


def test_config_switch_defaults_off_and_restores():
    from world_modelz_amd import config
    if 'WMZ_CONTEXT_CACHE' not in os.environ:
        assert config.get_context_cache() is False
    prev = config.get_context_cache()
    with config.context_cache(True):
        assert config.get_context_cache() is True
        with config.context_cache(False):
            assert config.get_context_cache() is False
        assert config.get_context_cache() is True
    assert config.get_context_cache() is prev
    config.set_context_cache(1)
    assert config.get_context_cache() is True
    config.set_context_cache(prev)
