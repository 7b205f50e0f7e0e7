"""Confidence-ordered masking for config 5's sampler, the parts that need no GPU: the two entry points in the binding read from
include/wmz.h, sample_clips' refusals (before any device work), the torch form of the selection law with an explicit count
(sample.lowest_scores_mask(count=) / sample.context_remask_count) against a brute-force sort, and the compiler's resource report
of the new kernels."""
import math
import os
import struct
import subprocess
import sys

import pytest
import torch

import abi_header
from conftest import ROOT

INF = float('inf')


def test_the_two_entry_points_are_declared_with_the_header_s_argument_counts():
    from world_modelz_amd import _lib
    for name, count in (('wmz_categorical_scatter_scored', 22), ('wmz_sparse_draw_context_scored', 23)):
        restype, argtypes = _lib.DECLARATIONS[name]
        assert restype is _lib.c_int and len(argtypes) == count == abi_header.arguments(name).count(',') + 1, name
    # the old entry points' arguments, in place; behind them scores + stride, and scores + stride + noise + the probe
    sig = _lib.SIGNATURES
    assert sig['wmz_categorical_scatter_scored'][:20] == sig['wmz_categorical_scatter_filtered']
    assert sig['wmz_categorical_scatter_scored'][20:] == [_lib.c_void_p, _lib.c_long]
    assert sig['wmz_sparse_draw_context_scored'][:19] == sig['wmz_sparse_draw_context_known']
    assert sig['wmz_sparse_draw_context_scored'][19:] == [_lib.c_void_p, _lib.c_long, _lib.c_float, _lib.c_void_p]
    assert abi_header.constants('WMZ_VERSION')['WMZ_VERSION'] == 115
    abi_header.assert_bound(_lib.lib(), 'wmz_categorical_scatter_scored', 'wmz_sparse_draw_context_scored')


class Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.shape = (8, 4, 4)
        self.embedding = torch.nn.Embedding(25, 8)

    def forward(self, tokens, indices):
        raise AssertionError('the model was reached')


@pytest.mark.parametrize('bad', [dict(remask='best'), dict(remask='confidence', remask_noise=-1), dict(remask='confidence', remask_noise=INF),
                                 dict(remask_noise=-1), dict(remask_noise=INF), dict(remask=None)], ids=str)
def test_sample_clips_refuses_bad_arguments_before_any_device_work(bad, monkeypatch):
    """A remask outside sample.REMASK_MODES, a negative or infinite remask_noise (under either rule): ValueError, with the library
    not loaded and the model not called (a CPU stand-in, 24 codes)."""
    from world_modelz_amd import _lib
    from world_modelz_amd.sparse_diffusion import sample_clips

    def no_library():
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_lib, 'lib', no_library)
    with pytest.raises(ValueError):
        sample_clips(Stub(), 2, 24, 'neighbors', num_context=32, num_eval_iterations=3, **bad)


def test_the_new_arguments_are_keyword_only_and_default_to_the_random_rule():
    import inspect
    from world_modelz_amd.sparse_diffusion import evaluate_model, sample_clips
    from world_modelz_amd.train import draw_sparse_context
    from world_modelz_amd.sparse_diffusion import categorical_scatter
    for fn in (evaluate_model, sample_clips):
        p = inspect.signature(fn).parameters
        for name, default in (('remask', 'random'), ('remask_noise', 0.0)):
            assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default == default, (fn.__name__, name)
    p = inspect.signature(draw_sparse_context).parameters
    assert (p['scores'].default, p['noise'].default, p['slot_scores'].default) == (None, 0.0, None)
    assert inspect.signature(categorical_scatter).parameters['scores'].default is None


# ---------------------------------------------------------------- the torch law against a brute-force sort

def f32(v):
    return struct.unpack('<f', struct.pack('<f', v))[0]


def brute_key(x):
    """The order-preserving key of one fp32 value's bits, in plain Python."""
    b = struct.unpack('<I', struct.pack('<f', x))[0]
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)


def brute_count(r, n):
    """floor(clamp(r, 0, 1) * n): r rounded to fp32, the product (exact in fp64: 24 x 10 bits) rounded to fp32 once."""
    rc = min(max(f32(r), 0.0), 1.0)
    return int(math.floor(f32(rc * float(n))))


def brute_mask(scores, counts, candidates):
    B, n = scores.shape
    out = torch.zeros(B, n, dtype=torch.bool)
    for b in range(B):
        slots = [i for i in range(n) if bool(candidates[b, i])]
        slots.sort(key=lambda i: (brute_key(float(scores[b, i])), i))
        for i in slots[:counts[b]]:
            out[b, i] = True
    return out


def score_cases(n):
    g = torch.Generator().manual_seed(100 + n)
    rnd = torch.randn(3, n, generator=g)
    dup = torch.randint(-2, 3, (3, n), generator=g).float() * 0.5                # five values: duplicates everywhere, +0.0 among them
    special = torch.randn(3, n, generator=g)
    pool = torch.tensor([0.0, -0.0, INF, -INF, -INF, 0.0, -0.0, INF])
    special[:, ::2] = pool[torch.arange(special[:, ::2].shape[1]) % len(pool)]
    start = torch.full((3, n), -INF)                                             # the sampler's first sub-steps: nothing drawn yet
    start[:, n // 3:] = torch.randn(3, n - n // 3, generator=g)
    return {'random': rnd, 'duplicates': dup, 'special': special, 'start': start}


R_VALUES = [0.0, 1.0, 0.5, 1 - 2.0 ** -24, 1 / 3]


@pytest.mark.parametrize('n', [1, 20, 64, 65, 512])
def test_lowest_scores_mask_with_a_count_is_the_brute_force_sort(n):
    """Per clip its own count m = context_remask_count(r, n), r in {0, 1, 0.5, 1 - 2^-24, 1/3} three at a time; scores with
    duplicates, +-0.0, -inf blocks and +inf; all slots candidates, a random half, and a clip with none: the mask is the brute-force
    one (key order, ties to the lower slot) and holds exactly min(m, #candidates) slots.  A plain int count does the same."""
    from world_modelz_amd.sample import context_remask_count, lowest_scores_mask
    g = torch.Generator().manual_seed(9 * n)
    half = torch.rand(3, n, generator=g) < 0.5
    half[2] = False
    cands = {'all': torch.ones(3, n, dtype=torch.bool), 'half': half}
    for name, scores in score_cases(n).items():
        for shift in range(len(R_VALUES)):
            r = [R_VALUES[(shift + j) % len(R_VALUES)] for j in range(3)]
            counts = [brute_count(v, n) for v in r]
            m = context_remask_count(torch.tensor(r), n)
            assert m.dtype == torch.int64 and m.tolist() == counts, (r, n)
            for cname, cand in cands.items():
                want = brute_mask(scores, counts, cand)
                got = lowest_scores_mask(scores, None, None if cname == 'all' else cand, count=m)
                assert got.dtype == torch.bool and torch.equal(got, want), (name, r, cname)
                assert torch.equal(got.sum(-1), torch.minimum(cand.sum(-1), m)), (name, r, cname)
        want = brute_mask(scores, [n // 2] * 3, cands['half'])
        assert torch.equal(lowest_scores_mask(scores, None, cands['half'], count=n // 2), want), name
    # the defaults are the dense sampler's law, as before
    assert torch.equal(lowest_scores_mask(torch.zeros(1, n), 0.5)[0], torch.arange(n) < n // 2)


@pytest.mark.parametrize('n', [1, 20, 32, 511, 512])
def test_context_remask_count_is_one_fp32_multiply(n):
    """r in {0, 1, 0.5, 1 - 2^-24, 1/3} (and values outside [0, 1], clamped) against the arithmetic done by hand: r in fp32, the
    product rounded to fp32 once, floor.  1 - 2^-24 times 512 is 512 - 2^-15: exact in fp32, floor 511 -- not 512; times 1 it hides
    nothing."""
    from world_modelz_amd.sample import context_remask_count
    rs = R_VALUES + [-0.25, 1.5]
    got = context_remask_count(torch.tensor(rs, dtype=torch.float32), n).tolist()
    assert got == [brute_count(v, n) for v in rs]
    assert got[0] == 0 and got[1] == n and got[2] == n // 2 and got[3] == n - 1 and got[5] == 0 and got[6] == n
    third = struct.unpack('<f', struct.pack('<f', 1 / 3))[0]                     # 0x3EAAAAAB: just ABOVE 1/3
    assert third > 1 / 3 and got[4] == int(math.floor(f32(third * n)))
    if n == 512:
        assert got[4] == 170
    assert context_remask_count(0.5, 20).tolist() == [10]


# ---------------------------------------------------------------- the compiler's report

def kres_rows(unit):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'kres.py'), os.path.join(ROOT, 'world_modelz_amd', 'csrc', unit)],
                       capture_output=True, text=True)
    rows = {}
    for line in r.stdout.splitlines():
        name = line.replace('void ', '').split(' vgpr ')[0].strip()
        t = line.split()
        rows[name] = {k: int(t[t.index(k) + 1]) for k in ('vgpr', 'scratch', 'lds')}
    assert rows, r.stdout + r.stderr
    return rows


def test_new_kernels_use_no_scratch():
    """hipcc's resource report (tools/kres.py): the scored variant of sparse_context_kernel spills nothing and asks for exactly the
    LDS of the form without a score, which is still there under its own name; every scored sparse instantiation of the two draw
    kernels of sampler.hip is there and spills nothing."""
    ctx = kres_rows('sparse_context.hip')
    assert 'sparse_context_kernel<false>' in ctx and 'sparse_context_kernel<true>' in ctx, sorted(ctx)
    assert ctx['sparse_context_kernel<true>']['scratch'] == 0 and ctx['sparse_context_kernel<false>']['scratch'] == 0
    assert ctx['sparse_context_kernel<true>']['lds'] == ctx['sparse_context_kernel<false>']['lds']
    loss = kres_rows('sampler.hip')
    want = [f'sample_tokens_kernel<{nv}, {t}, {p}, true, SparseScoredDest>' for nv in (4, 8, 16, 32)
            for t in ('false', 'true') for p in ('false', 'true')] + ['sample_tokens_wide_kernel<SparseScoredDest>']
    for name in want:
        assert name in loss, (name, sorted(loss))
        assert loss[name]['scratch'] == 0, name
