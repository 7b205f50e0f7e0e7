"""Confidence-ordered re-masking on the host: sample.lowest_scores_mask (the torch form of the selection law that include/wmz.h
states next to wmz_remask_lowest_dev) against a brute-force Python sort, the new entry points as the header declares them, and
the compiler's resource report of the new kernels."""
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


def brute_key(x):
    """The order-preserving key of one fp32 value's bits, in plain Python."""
    b = struct.unpack('<I', struct.pack('<f', x))[0]
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)


def brute_m(alpha, rows):
    """floor((1 - alpha) * rows) with alpha, the difference and the product each rounded to fp32 (struct does the rounding)."""
    def f32(v):
        return struct.unpack('<f', struct.pack('<f', v))[0]
    return int(math.floor(f32(f32(1.0 - f32(alpha)) * float(rows))))       # (fp64 ops on fp32 values, rounded once: the fp32 result)


def brute_mask(scores, alpha, candidates=None):
    """Per clip: sort the candidate positions by (key, index) in Python and take the first min(m, #candidates)."""
    B, HW = scores.shape
    m = brute_m(alpha, HW)
    out = torch.zeros(B, HW, dtype=torch.bool)
    for b in range(B):
        rows = [i for i in range(HW) if candidates is None or bool(candidates[b, i])]
        rows.sort(key=lambda i: (brute_key(float(scores[b, i])), i))
        for i in rows[:m]:
            out[b, i] = True
    return out, m


def score_cases(HW):
    g = torch.Generator().manual_seed(HW)
    rnd = torch.randn(3, HW, generator=g)
    equal = torch.full((3, HW), -1.25)
    two = torch.where(torch.rand(3, HW, generator=g) < 0.5, torch.tensor(-2.0), torch.tensor(-0.5))
    special = torch.randn(3, HW, generator=g)
    pool = torch.tensor([0.0, -0.0, INF, -INF, float('nan'), 0.0, -0.0, -INF])
    special[:, ::3] = pool[torch.arange(special[:, ::3].shape[1]) % len(pool)]
    return {'random': rnd, 'equal': equal, 'two-valued': two, 'special': special}


ALPHAS = [0.0, 1.0] + [(i + 1) / 30 for i in range(30)]


@pytest.mark.parametrize('HW', [1, 20, 250, 256])
def test_lowest_scores_mask_is_the_brute_force_sort(HW):
    """All-equal scores (the lowest indices go first), +0.0 / -0.0, +-inf and a NaN, a threshold inside a tie run, fewer candidates
    than m, alpha of 0, of 1 and the thirty values (i + 1) / 30: the mask is the brute-force one and holds exactly
    min(m, #candidates) positions per clip."""
    from world_modelz_amd.sample import lowest_scores_mask, remask_count
    g = torch.Generator().manual_seed(7 * HW)
    few = torch.zeros(3, HW, dtype=torch.bool)
    few[:, :max(1, HW // 7)] = True                                         # fewer candidates than m for the small alphas
    few[2] = False                                                          # ... and a clip with none
    cands = {'all': None, 'half': torch.rand(3, HW, generator=g) < 0.5, 'few': few}
    for name, scores in score_cases(HW).items():
        for alpha in ALPHAS:
            for cname, cand in cands.items():
                want, m = brute_mask(scores, alpha, cand)
                assert m == remask_count(alpha, HW)
                got = lowest_scores_mask(scores, alpha, cand)
                assert got.dtype == torch.bool and torch.equal(got, want), (name, alpha, cname)
                n_cand = torch.full((3,), HW) if cand is None else cand.sum(-1)
                assert torch.equal(got.sum(-1), n_cand.clamp(max=m)), (name, alpha, cname)
    assert remask_count(1.0, HW) == 0 and remask_count(0.0, HW) == HW
    eq = lowest_scores_mask(torch.zeros(1, HW), 0.5)
    assert torch.equal(eq[0], torch.arange(HW) < remask_count(0.5, HW))     # all equal: the lowest indices
    z = torch.tensor([[0.0, -0.0, 0.0, -0.0]])
    assert lowest_scores_mask(z, 0.5).tolist() == [[False, True, False, True]]        # -0.0 orders below +0.0


def test_feeding_the_mask_back_as_candidates_shrinks_it():
    """Consistent masking: each step's mask as the next step's candidates gives a shrinking set, empty at alpha = 1."""
    from world_modelz_amd.sample import lowest_scores_mask
    g = torch.Generator().manual_seed(5)
    B, HW, n = 3, 250, 30
    cand = torch.ones(B, HW, dtype=torch.bool)
    for i in range(n):
        scores = torch.randn(B, HW, generator=g)
        mask = lowest_scores_mask(scores, (i + 1) / n, cand)
        assert bool((mask & ~cand).sum() == 0)
        assert bool((mask.sum(-1) <= cand.sum(-1)).all())
        cand = mask
    assert int(cand.sum()) == 0


def test_torch_scores_follow_the_law():
    """confidence_scores: the fp32 log-softmax of the unfiltered logits at the draw, the Gumbel term only with noise > 0 (u = 0 gives
    -inf), NaN stored as -inf."""
    from world_modelz_amd.sample import confidence_scores, gumbel_from_uniform
    g = torch.Generator().manual_seed(11)
    logits = torch.randn(6, 9, generator=g)
    logits[5] = -INF                                                        # a row without any class: NaN -> -inf
    draws = torch.tensor([0, 3, 8, 1, 2, 4])
    s = confidence_scores(logits, draws, 0.25)
    ref = torch.log_softmax(logits[:5].double(), -1)[torch.arange(5), draws[:5]]
    assert s.dtype == torch.float32 and float((s[:5].double() - ref).abs().max()) < 1e-6 and float(s[5]) == -INF
    u = torch.tensor([0.5, 0.0, 0.25, 0.75, 0.9, 0.5])
    sn = confidence_scores(logits, draws, 0.25, 0.5, u)
    want = ref + 0.5 * 0.75 * -torch.log(-torch.log(u[:5].double()))
    assert float(sn[1]) == -INF and float(sn[5]) == -INF
    keep = torch.tensor([0, 2, 3, 4])
    assert float((sn[keep].double() - want[keep]).abs().max()) < 1e-5
    assert float(gumbel_from_uniform(torch.tensor([0.0]))) == -INF
    assert torch.equal(confidence_scores(logits, draws, 1.0, 0.0, None), confidence_scores(logits, draws, 0.25))


def test_header_declares_the_entry_points():
    from world_modelz_amd import _lib
    want = {'wmz_sample_tokens_scored_dev': 20, 'wmz_remask_lowest_max_rows': 0, 'wmz_remask_lowest_dev': 11}
    for name, n in want.items():
        args = abi_header.arguments(name).strip()
        got = 0 if args in ('', 'void') else len(args.split(','))
        assert got == n, (name, got)
        assert len(_lib.SIGNATURES[name]) == n, name
    assert abi_header.constants('WMZ_VERSION')['WMZ_VERSION'] == 115
    abi_header.assert_bound(_lib.lib(), *want)
    assert _lib.lib().wmz_version() == 115
    sig = _lib.SIGNATURES['wmz_sample_tokens_scored_dev']
    assert sig[5:7] == [_lib.c_float, _lib.c_float] and sig[14] == _lib.c_float                  # top_p, inv_temperature; noise
    from world_modelz_amd import ops
    assert ops.remask_max_rows() == _lib.lib().wmz_remask_lowest_max_rows() >= 4096


def test_new_kernels_use_no_scratch():
    """hipcc's resource report (tools/kres.py) of sampler.hip: every scored instantiation of the two draw kernels and both forms of the
    selection kernel are there and spill nothing; nor does any other sampler kernel."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'kres.py'), os.path.join(ROOT, 'world_modelz_amd', 'csrc', 'sampler.hip')],
                       capture_output=True, text=True)
    rows = {}
    for line in r.stdout.splitlines():
        name = line.replace('void ', '').split(' vgpr ')[0].strip()
        t = line.split()
        rows[name] = int(t[t.index('scratch') + 1])
    assert rows, r.stdout + r.stderr                                        # (kres exits 1 when ANY kernel of the unit spills: not read here)
    want = [f'sample_tokens_kernel<{nv}, {t}, {p}, true, ScoredDest>' for nv in (4, 8, 16, 32) for t in ('false', 'true')
            for p in ('false', 'true')] + ['sample_tokens_wide_kernel<ScoredDest>', 'remask_lowest_kernel<1>', 'remask_lowest_kernel<4>']
    for name in want:
        assert name in rows, (name, sorted(rows))
        assert rows[name] == 0, name
    for name, scratch in rows.items():
        if 'sample_tokens' in name:
            assert scratch == 0, name
