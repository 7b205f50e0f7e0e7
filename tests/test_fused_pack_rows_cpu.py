"""What csrc/fused_pack_rows.h -- the one place that says which blocks the weight streams of the default-width per-token kernels
hold, in which order, with which strides and ownership groups -- enumerates, checked on the host: the header is compiled into
tests/fused_pack_rows_host.cpp by the host compiler and its rows compared with a second statement of the layout kept here (the
block(...) listing fused.PackSet._build carried before it asked the header), so that the GPU check of PackSet against the
per-stream packers -- both fed by the header -- does not become "a thing equals itself"."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'fused_pack_rows_host.cpp')
CXX = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/llvm/bin/clang++')
            if c and os.path.exists(c)), None)
pytestmark = pytest.mark.skipif(CXX is None, reason='no host C++ compiler available')

D_, I_, M_, MC_ = 256, 128, 256, 32
FWD_HEAD, FWD_TAIL, BWD_QKV, BWD_FF = D_ * I_ + 2 * M_ * D_, 3 * I_ * D_, 3 * D_ * I_, 2 * M_ * D_ + D_ * I_
PAD = 32768                                                                             # 64 KB of zeros behind every stream
TOTALS = {'ht': 294912 - PAD, 'h': 294912 - PAD - 98304, 't': 98304, 'q': 98304, 'f': 163840}      # stream elements (head + tail: 294 912 with its padding)
MAX_ROWS = {'ht': 20, 'h': 20, 't': 20, 'q': 3, 'f': 10}


class Fake:
    """A tensor as far as the listing below looks at one: an address."""
    def __init__(self, addr):
        self.addr = addr

    def data_ptr(self):
        return self.addr


def listing(streams, start8):
    """The rows of the streams (the host program's STREAM arguments) on the host program's fake addresses."""
    rows = []
    state = {'g8': start8}

    def ptr(t, off=0):
        return 0 if t is None else t.data_ptr() + 4 * off

    def block(dst, doff, w, woff, rs, ks, N, K, gn, gk, gamma, rgamma):
        rows.append([ptr(w, woff), rs, ks, N, K, gn, gk, ptr(gamma), ptr(rgamma), dst.data_ptr() + 2 * doff, state['g8']])
        state['g8'] += N * K // 8
        return doff + N * K

    out = []
    for i, kind in enumerate(streams):
        first = len(rows)
        slot = [Fake((k + 1) << 32) for k in range(14)]
        dst = Fake((100 + i) << 32)
        if kind in ('ht', 'h', 't'):
            wpack, off = dst, 0
            if 'h' in kind:
                wout, bout, g2, be2, w1, b1, w2, b2 = slot[:8]
                off = block(wpack, off, wout, 0, I_, 1, D_, I_, D_, I_, None, None)
                off = block(wpack, off, w1, 0, D_, 1, MC_, D_, MC_, D_, g2, None)
                for c in range(1, M_ // MC_):
                    off = block(wpack, off, w1, c * MC_ * D_, D_, 1, MC_, D_, MC_, D_, g2, None)
                    off = block(wpack, off, w2, (c - 1) * MC_, M_, 1, D_, MC_, D_, MC_, None, None)
                off = block(wpack, off, w2, (M_ // MC_ - 1) * MC_, M_, 1, D_, MC_, D_, MC_, None, None)
            if 't' in kind:
                g1, be1, wq, wk, wv, bv = slot[-6:]
                off = block(wpack, off, wq, 0, D_, 1, I_, D_, I_, D_, None, None)
                off = block(wpack, off, wk, 0, D_, 1, I_, D_, I_, D_, g1, None)
                off = block(wpack, off, wv, 0, D_, 1, I_, D_, I_, D_, g1, None)
        else:
            wq, wk, wv, g1, wout, w1, g2, w2 = slot[:8]
            if kind == 'q':
                sq = dst
                off = block(sq, 0, wk, 0, 1, D_, D_, I_, 128, 128, None, g1)
                off = block(sq, off, wv, 0, 1, D_, D_, I_, 128, 128, None, g1)
                off = block(sq, off, wq, 0, 1, D_, D_, I_, 128, 128, None, None)
            else:
                sf = dst
                off = 0
                for c in range(M_ // 32):
                    off = block(sf, off, w2, c * 32, 1, M_, 32, D_, 32, 128, None, None)
                off = block(sf, off, w1, 0, 1, D_, D_, M_, 128, 32, None, g2)
                off = block(sf, off, wout, 0, 1, I_, I_, D_, 128, 128, None, None)
        out.append(rows[first:])
    return out


@pytest.fixture(scope='module')
def enumerator(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('fused_pack_rows') / 'fused_pack_rows_host')
    r = subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror', SRC, '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]

    def run(streams, start8):
        out = subprocess.run([exe, str(start8)] + list(streams), capture_output=True, text=True)
        assert out.returncode == 0, (out.returncode, out.stderr)
        got = [[] for _ in streams]
        for line in out.stdout.split('\n'):
            f = line.split()
            if f:
                assert f[0] == 'row' and len(f) == 13
                got[int(f[1])].append([int(v) for v in f[2:]])
        return got
    return run


CASES = [(('ht',), 0), (('h',), 0), (('t',), 0), (('q',), 0), (('f',), 0),
         (('t', 'ht'), 4096), (('q', 'f'), 12345),                        # two streams behind each other, non-zero start8
         (('t', 'ht', 'ht', 'h', 'q', 'f'), 0)]                             # a depth-2 model's table, in PackSet's order


@pytest.mark.parametrize('streams,start8', CASES, ids=lambda v: '+'.join(v) if isinstance(v, tuple) else str(v))
def test_rows_match_the_second_statement_and_tile_the_stream(enumerator, streams, start8):
    got, want = enumerator(streams, start8), listing(streams, start8)
    g8 = start8
    for i, kind in enumerate(streams):
        assert got[i] == want[i], (kind, i)
        assert 0 < len(got[i]) <= MAX_ROWS[kind] and len(got[i]) == {'ht': 20, 'h': 17, 't': 3, 'q': 3, 'f': 10}[kind]
        # the destination ranges tile [0, nw) of the stream in order, without gap or overlap; start8 advances by N K / 8
        at = (100 + i) << 32
        for w, rs, ks, N, K, gn, gk, gamma, rgamma, dst, s8 in got[i]:
            assert dst == at and s8 == g8
            assert N % 32 == 0 and K % 16 == 0 and N % gn == 0 and K % gk == 0 and gn % 32 == 0 and gk % 16 == 0
            at += 2 * N * K
            g8 += N * K // 8
        nw = (at - ((100 + i) << 32)) // 2
        assert nw == TOTALS[kind] == {'ht': FWD_HEAD + FWD_TAIL, 'h': FWD_HEAD, 't': FWD_TAIL, 'q': BWD_QKV, 'f': BWD_FF}[kind]
    assert g8 == start8 + sum(TOTALS[k] for k in streams) // 8


def test_the_library_entry_point_hands_out_the_same_rows():
    """wmz_fused_pack_rows (what fused.PackSet asks) on the host program's fake addresses: the rows of the second statement; widths
    other than 256 / 128 / 256, a missing parameter and an unknown kind are refused with a negative code and the usual message."""
    import ctypes
    import abi_header
    from world_modelz_amd import _lib
    lib = _lib.lib()
    abi_header.assert_bound(lib, 'wmz_fused_pack_rows')
    assert not hasattr(lib, 'wmz_fused_pack_rows_f16')

    def ask(kind, slots, start8, D=D_, I=I_, M=M_):
        buf = (ctypes.c_int64 * (20 * 11))()
        n = lib.wmz_fused_pack_rows(kind, (ctypes.c_void_p * len(slots))(*slots), 100 << 32, start8, D, I, M, buf)
        return n, [list(buf[11 * j:11 * j + 11]) for j in range(max(n, 0))]
    slots = [(k + 1) << 32 for k in range(14)]
    for kind, name, sl in ((0, 'ht', slots), (0, 'h', slots[:8] + [None] * 6), (0, 't', [None] * 8 + slots[8:]), (1, 'q', slots[:8]),
                           (2, 'f', slots[:8])):
        n, rows = ask(kind, sl, 77)
        assert n == len(rows) and rows == listing((name,), 77)[0], name
    refused = ((dict(kind=0, slots=slots, start8=0, D=128), 'built for dim 256 / inner 128 / mlp 256'),
               (dict(kind=0, slots=[None] * 14, start8=0), 'bad arguments'), (dict(kind=1, slots=[None] + slots[1:8], start8=0), 'bad arguments'),
               (dict(kind=3, slots=slots, start8=0), 'bad arguments'))
    for args, msg in refused:
        assert ask(**args)[0] == -abi_header.constants('WMZ_ERR_ARG')['WMZ_ERR_ARG'] and msg in lib.wmz_last_error().decode(), args
