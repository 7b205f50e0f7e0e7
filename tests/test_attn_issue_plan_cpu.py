"""The row map and the issue plan of the 16-wave whole-plane attention forward (csrc/attn_slab_walk.h: slab_wave_row,
slab_issue_class, slab_issues), checked on the host: tests/attn_issue_plan_host.cpp prints them from the header, built with the
address and undefined-behaviour sanitizers and run stand-alone; the rules are restated here, not read from the header.

Geometry: 16 query rows, one per wave; window of 3 rows either side; a plane's 16 key rows in two parity slabs of 8; a slab image
is 36 pieces of 1 KB (128 padded rows of 288 bytes); waves w, w + 4, w + 8, w + 12 share a SIMD."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'attn_issue_plan_host.cpp')
CXX = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/llvm/bin/clang++')
            if c and os.path.exists(c)), None)
pytestmark = pytest.mark.skipif(CXX is None, reason='no host C++ compiler available')

NW, EH, PIECES, CLASSES = 16, 3, 36, 9


def key_rows(row, par):
    """The plain rule: key rows of parity `par` within EH rows of query row `row`."""
    return [r for r in range(NW) if abs(r - row) <= EH and r % 2 == par]


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('attn_issue_plan') / 'attn_issue_plan_host')
    r = subprocess.run([CXX, '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                        SRC, '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, (out.returncode, out.stderr[-2000:])
    rows, plans, voff, step = {}, {}, {}, None
    for line in out.stdout.split('\n'):
        f = line.split()
        if not f:
            continue
        if f[0] == 'row':
            rows[int(f[1])] = int(f[2])
        elif f[0] == 'plan':
            plans[int(f[1])] = dict(zip(('cls', 'iss0', 'iss1', 'n0', 'n1'), map(int, f[2:])))
        elif f[0] == 'voff':
            voff[int(f[1]), int(f[2])] = int(f[3])
        else:
            assert f[0] == 'step'
            step = int(f[1])
    assert len(rows) == NW and len(plans) == NW and len(voff) == PIECES * 64 and step is not None
    return rows, plans, voff, step


def test_row_map_is_a_permutation(plan):
    rows, *_ = plan
    assert sorted(rows) == list(range(NW)) and sorted(rows.values()) == list(range(NW))


@pytest.mark.parametrize('par', [0, 1])
def test_no_simd_carries_more_than_13_key_rows_of_a_slab(plan, par):
    rows, plans, *_ = plan
    for r in range(NW):                                  # the header counts like the plain rule
        assert plans[r]['n%d' % par] == len(key_rows(r, par))
    per_simd = [sum(len(key_rows(rows[w], par)) for w in range(NW) if w % 4 == simd) for simd in range(4)]
    print(f'parity {par}: key rows per SIMD {per_simd}; with row = wave '
          f'{[sum(len(key_rows(w, par)) for w in range(NW) if w % 4 == simd) for simd in range(4)]}')
    assert sum(per_simd) == 50 and max(per_simd) <= 13


@pytest.mark.parametrize('par', [0, 1])
def test_every_piece_has_exactly_one_issuer_and_no_issuer_has_four_rows(plan, par):
    """During the slab of parity `par`: nine issuers, each owns one class mod 9 (the K and the V image alike: pieces c, c + 9, c +
    18, c + 27), the classes cover the 36 pieces once, and an issuer has fewer than four key rows in that slab."""
    _, plans, *_ = plan
    issuers = [r for r in range(NW) if plans[r]['iss%d' % par]]
    assert len(issuers) == CLASSES
    owners = {}
    for r in issuers:
        c = plans[r]['cls']
        assert 0 <= c < CLASSES
        for p in range(c, PIECES, CLASSES):
            owners.setdefault(p, []).append(r)
        assert len(key_rows(r, par)) < 4, (r, par)
    assert sorted(owners) == list(range(PIECES)) and all(len(v) == 1 for v in owners.values()), owners
    for r in range(NW):                                  # a row that never issues has no class; one that does keeps ONE for both parities
        assert (plans[r]['cls'] >= 0) == bool(plans[r]['iss0'] or plans[r]['iss1'])


def test_pieces_of_a_class_lie_one_step_apart_for_every_lane(plan):
    """Nine pieces are 32 padded rows = two slab rows = four plane rows of 16 tokens of 256 bytes: 16 384 bytes in the plane, and
    9 KB in the image."""
    *_, voff, step = plan
    assert step == 4 * 16 * 256 == 16384 and CLASSES * 1024 == 32 * 288
    for p in range(PIECES - CLASSES):
        for lane in range(64):
            assert voff[p + CLASSES, lane] == voff[p, lane] + step, (p, lane)
    assert max(voff.values()) + 16 <= 15 * 16 * 256        # from parity row 0 or 1, inside the plane either way
