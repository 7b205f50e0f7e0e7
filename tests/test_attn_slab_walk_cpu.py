"""What the slab walk of the attention row kernels (csrc/attn_slab_walk.h) promises, checked on the host: the header is compiled
into tests/attn_slab_walk_host.cpp by the host compiler and its output compared with a restatement of the rules written here (from
DESIGN 4.1 / 4.2, not from the header): which slabs, in which order, and which bytes their LDS-DMA fetches."""
import functools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'attn_slab_walk_host.cpp')
CXX = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/llvm/bin/clang++')
            if c and os.path.exists(c)), None)
pytestmark = pytest.mark.skipif(CXX is None, reason='no host C++ compiler available')

SHAPES = {'big': (16, 16, 8), 'big8': (8, 16, 8), 'small': (4, 4, 2)}        # NW, CH (rows per chunk), KC (rows per slab); RS = CH / KC row phases
# (S, H in tile rows, eS, eH in tile rows, shape): the smallest that reach each branch
GEOMS = [(2, 1, 0, 1, 'big'),        # one row, no odd phase
         (2, 17, 1, 2, 'big'),       # H = 1 mod 16
         (2, 5, 0, 1, 'big'),        # idle waves
         (3, 40, 2, 2, 'big'),       # several workgroups, ragged last chunk
         (5, 16, 3, 3, 'big'),       # window wider than the clip: the start falls back to sk_lo
         (9, 16, 3, 1, 'big'),       # rotation with wrap
         (3, 24, 1, 3, 'big8'), (2, 16, 1, 2, 'big8'),    # the backward's 8-wave workgroups on 16-row chunks: ragged, whole
         (8, 4, 3, 2, 'small'), (3, 8, 1, 2, 'small'), (2, 3, 1, 1, 'small'), (3, 1, 1, 1, 'small')]   # whole, two workgroups, ragged, one row
LAYOUTS = [(32, 1, 1), (32, 2, 3), (128, 1, 1), (128, 2, 3)]     # (dim_head, heads, ld / (heads dh)): own tensor, fused qkv buffer


@pytest.fixture(scope='module')
def walker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('slab_walk') / 'attn_slab_walk_host')
    r = subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror', SRC, '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]

    @functools.lru_cache(maxsize=None)
    def run(S, H, eS, eH, shape, dh=32, heads=1, ldf=1):
        out = subprocess.run([exe] + [str(a) for a in (S, H, eS, eH, shape, dh, ldf * heads * dh, heads)], capture_output=True, text=True)
        assert out.returncode == 0, (out.returncode, out.stderr)
        wgs = []
        for line in out.stdout.split('\n'):
            f = line.split()
            if f and f[0] == 'wg':
                keys = ('s', 'og', 't_lo', 't_hi', 'sk_lo', 'sk_hi', 'c_first', 'nch', 'nslab', 'p_first')
                wgs.append(dict(zip(keys, map(int, f[2:])), form=f[1], slabs=[]))
            elif f:
                assert f[0] == 'slab'
                wgs[-1]['slabs'].append(tuple(map(int, f[1:])))
        return wgs
    return run


def rules(S, H, eS, eH, shape, s, og):
    """The rules, restated: (rows the workgroup needs, planes in visiting order, slabs of a plane in order as (chunk, phase))."""
    NW, CH, KC = SHAPES[shape]
    owners = range(og * NW, min(og * NW + NW, H))
    rows = range(max(0, owners[0] - eH), min(H - 1, owners[-1] + eH) + 1)
    lo, hi = max(0, s - eS), min(S - 1, s + eS)
    start = next(p for p in range(s - eS, s + eS + 1) if (S - 1 - p) % (2 * eS + 1) == 0)
    if not lo <= start <= hi:
        start = lo
    planes = list(range(start, hi + 1)) + list(range(lo, start))
    slabs = [(c, ph) for c in range(rows[0] // CH, rows[-1] // CH + 1) for ph in range(CH // KC)]
    return rows, planes, slabs


@pytest.mark.parametrize('geom', GEOMS, ids=lambda g: '-'.join(map(str, g)))
def test_slabs_order_and_cover(walker, geom):
    S, H, eS, eH, shape = geom
    NW, CH, KC = SHAPES[shape]
    RS = CH // KC
    wgs = walker(*geom)
    forms = {'clamp'} | ({'whole'} if shape == 'big' and H % 16 == 0 else set())
    assert {(w['form'], w['s'], w['og']) for w in wgs} == {(f, s, og) for f in forms for s in range(S) for og in range(-(-H // NW))}
    assert len(wgs) == len(forms) * S * -(-H // NW)
    for w in wgs:
        rows, planes, slabs = rules(S, H, eS, eH, shape, w['s'], w['og'])
        assert (w['t_lo'], w['t_hi'], w['sk_lo'], w['sk_hi'], w['p_first']) == (rows[0], rows[-1], min(planes), max(planes), planes[0]), w
        # 1. nslab = planes x nch, every (plane, chunk, phase) exactly once
        assert w['nch'] == len(slabs) and w['nslab'] == len(planes) * len(slabs) == len(w['slabs'])
        seen = [(p, base // CH, base % CH) for p, base, *_ in w['slabs']]
        assert len(set(seen)) == len(seen) and set(seen) == {(p, c, ph) for p in planes for c, ph in slabs}
        # 2. the planes in the rotated order, whole planes one after the other, a plane's slabs chunk by chunk and phase by phase
        assert seen == [(p, c, ph) for p in planes for c, ph in slabs], (w['s'], w['og'])
        # 4. every needed row of every visited plane in exactly one slab (row = base + RS r, r < KC), inside the plane
        for p in planes:
            hits = {}
            for q, base, *_ in w['slabs']:
                if q == p:
                    for r in range(KC):
                        hits[base + RS * r] = hits.get(base + RS * r, 0) + 1
            assert all(hits.get(row) == 1 for row in rows), (p, hits)
            assert all(n == 1 for n in hits.values())


@pytest.mark.parametrize('geom', GEOMS, ids=lambda g: '-'.join(map(str, g)))
def test_trailing_planes_walk_like_the_whole_clip(walker, geom):
    """3. A clip cut down to its trailing planes (S - d of S, what the last-frame cone hands over): a query plane whose window the
    cut does not touch visits the same planes in the same order, slab by slab."""
    S, H, eS, eH, shape = geom
    whole = {(w['form'], w['s'], w['og']): w for w in walker(*geom)}
    compared = 0
    for d in range(1, S):
        for w in walker(S - d, H, eS, eH, shape):
            s = w['s'] + d
            if max(0, s - eS) >= d:
                full = whole[(w['form'], s, w['og'])]
                assert [(p + d, base) for p, base, *_ in w['slabs']] == [(p, base) for p, base, *_ in full['slabs']], (d, s)
                compared += 1
    assert (compared > 0) == (S >= eS + 2)               # (a shorter clip has no query plane whose window survives a cut)


@pytest.mark.parametrize('layout', LAYOUTS, ids=lambda t: 'dh%d-heads%d-ld%dx' % t)
@pytest.mark.parametrize('geom', GEOMS, ids=lambda g: '-'.join(map(str, g)))
def test_fetched_bytes_stay_inside_the_plane(walker, geom, layout):
    """5. Every byte any lane of any piece fetches lies inside the tensor and inside the plane being staged (rows of the plane,
    columns of the heads), and the rows the workgroup needs are among them.  (Broken once: H = 1 fetched from behind the tensor.)"""
    S, H, eS, eH, shape = geom
    dh, heads, ldf = layout
    NW, CH, KC = SHAPES[shape]
    ld_b, width = ldf * heads * dh * 2, heads * dh * 2          # bytes per row of 1 position; bytes of it that belong to the tensor
    for w in walker(S, H, eS, eH, shape, dh, heads, ldf):
        rows, planes, _ = rules(S, H, eS, eH, shape, w['s'], w['og'])
        for p, base, lo, hi, clo, chi in w['slabs']:
            first, last = p * H * 16, (p + 1) * H * 16 - 1        # the plane's positions
            assert 0 <= first * ld_b <= lo and hi <= last * ld_b + width - 1 <= (S * H * 16 - 1) * ld_b + width - 1, (w['s'], w['og'], p, base)
            assert 0 <= clo and chi <= width - 1
            need = [r for r in (base + (CH // KC) * i for i in range(KC)) if r in rows]
            if need:
                assert lo <= (first + need[0] * 16) * ld_b and hi >= (first + need[-1] * 16 + 15) * ld_b + width - 1
