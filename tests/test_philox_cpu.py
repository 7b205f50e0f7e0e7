"""The generator behind the token corruption, the sparse context draw and the samplers (csrc/wmz_philox.h), checked on the host: the
header is compiled into tests/philox_host.cpp by the host compiler and its words compared with a restatement of Philox4x32-10 written
here from Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as easy as 1, 2, 3" (SC 2011), section 3.3 and table 2 -- not from the
header -- and with the known-answer vectors Random123 publishes for philox4x32-10."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'philox_host.cpp')
CXX = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/llvm/bin/clang++')
            if c and os.path.exists(c)), None)
pytestmark = pytest.mark.skipif(CXX is None, reason='no host C++ compiler available')

M32 = 0xFFFFFFFF


def philox4x32(counter, key, rounds=10):
    """The paper's bijection: per round, L' = B_k(R) = mulhi(R, M) ^ k ^ L and R' = mullo(R, M) on the two (L, R) pairs of the
    permuted counter; the key is bumped by the Weyl constants (golden ratio, sqrt(3) - 1) before every round but the first."""
    mult = (0xD2511F53, 0xCD9E8D57)
    weyl = (0x9E3779B9, 0xBB67AE85)
    x = list(counter)
    k = list(key)
    for r in range(rounds):
        if r:
            k = [(k[i] + weyl[i]) & M32 for i in range(2)]
        p0, p1 = mult[0] * x[0], mult[1] * x[2]
        x = [(p1 >> 32) ^ x[1] ^ k[0], p1 & M32, (p0 >> 32) ^ x[3] ^ k[1], p0 & M32]
    return x


def keyed(index, stream, seed):
    """The project's keying: counter = (index, stream), key = seed, low word first."""
    return philox4x32([index & M32, index >> 32, stream & M32, stream >> 32], [seed & M32, seed >> 32])


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('philox') / 'philox_host')
    r = subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror', SRC, '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
        assert out.returncode == 0, (out.returncode, out.stderr)
        return out.stdout.split('\n')[:-1]
    return run


# (index, stream, seed): zero; the layouts the kernels use (a row index, a stream id with a domain bit, the rank and a 40-bit
# counter, a 64-bit seed); index and stream beyond 2^32 with both key words set; all ones
BLOCKS = [(0, 0, 0),
          (1, 0, 0), (0, 1, 0), (0, 0, 1),
          (12345, (1 << 63) | (3 << 40) | 77, 0x0123456789ABCDEF),
          ((1 << 32) + 5, (1 << 32) + 9, (7 << 32) | 11),
          (0xFEDCBA9876543210, 0x0F1E2D3C4B5A6978, 0xDEADBEEFCAFEF00D),
          (M32, M32 << 32, 1 << 32),
          ((1 << 64) - 1, (1 << 64) - 1, (1 << 64) - 1)]


@pytest.mark.parametrize('block', BLOCKS, ids=lambda b: '-'.join('%x' % v for v in b))
def test_block_matches_the_published_algorithm(host, block):
    (line,) = host('b', *block)
    f = line.split()
    assert [int(w, 16) for w in f[:4]] == keyed(*block)
    assert [float.fromhex(u) for u in f[4:]] == [(w >> 8) / 2.0 ** 24 for w in keyed(*block)]       # the float form of the same block


# Random123's kat_vectors for philox4x32 with 10 rounds: (counter, key, result)
KAT = [((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
       ((M32,) * 4, (M32,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), 'd16cfe09 94fdcceb 5001e420 24126ea1')]


@pytest.mark.parametrize('kat', KAT, ids=['zeros', 'ones', 'pi'])
def test_known_answer_vectors(host, kat):
    c, k, want = kat
    assert ' '.join('%08x' % w for w in philox4x32(c, k)) == want            # the restatement itself
    (line,) = host('b', c[0] | (c[1] << 32), c[2] | (c[3] << 32), k[0] | (k[1] << 32))
    assert ' '.join(line.split()[:4]) == want


@pytest.mark.parametrize('word', [0, 0xFF, 0x100, 0x80000000, 0x9E3779B9, 0xFFFFFF00, 0xFFFFFFFF], ids=lambda w: '%08x' % w)
def test_unit_mapping_keeps_the_top_24_bits_and_stays_below_one(host, word):
    (line,) = host('u', word)
    u = float.fromhex(line)
    assert u == (word >> 8) / 2.0 ** 24 and 0.0 <= u < 1.0
