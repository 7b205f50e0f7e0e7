"""Confidence-ordered masking for config 5's sampler on the device: wmz_categorical_scatter_scored (the draw of
wmz_categorical_scatter_filtered plus the log-probability of each draw, written beside its token), wmz_sparse_draw_context_scored
(the context draw of wmz_sparse_draw_context_known with the hidden slots chosen by lowest score) and sample_clips(remask=
'confidence') on top of the pair.  include/wmz.h states the law; its torch form is sample.lowest_scores_mask(count=) /
sample.context_remask_count (held to a brute-force sort in test_sparse_confidence_cpu.py).

The score bound is the one derived in tests/test_confidence_remask_gpu.py for the dense scored draw -- the sparse scored draw runs
the same row bodies --, restated: u = 2^-24.  The kernel computes
    s = fl(fl(l_d - max) - logf(S~)),  S~ = the fp32 sum, in some order, of the C terms __expf(fl(l_c - max)).
  * one term: fl(l_c - max) = x (1 + d), |d| <= u, moves exp(x) by a relative |x| u; __expf(x) is the hardware's 2^y at
    y = fl(x * log2e): the rounding of the product and of the constant move the result by a relative <= 1.5 |x| u, the 2^y
    instruction is accurate to 1 ulp = 2 u.  Together <= (2.5 |x| + 2) u, taken as d(x) = (3 |x| + 2) u.  A term below the smallest
    normal may be flushed to 0: an absolute 2^-126 each.
  * the sum of n positive terms in any order: relative (n - 1) u / (1 - (n - 1) u) (Higham, Accuracy and Stability of Numerical
    Algorithms, eq. 4.4), taken as 2 C u.  So S~ = S (1 + eta), |eta| <= eta_row = sum_c w_c d(x_c) / S + 2 C u + C 2^-126.
  * logf accurate to 1 ulp, taken as 2: |logf(S~) - log S~| <= 4 u |log S~|; |log(1 + eta)| <= 1.01 eta_row for eta_row < 0.01
    (asserted).
  * the two subtractions round once each: u |l_d - max| + u |s|.
  bound = 1.01 eta_row + 4 u (|log S| + 0.01) + u |l_d - max| + u (|s| + 1).
The noise bound, likewise restated: the kernel adds fl(fl(noise * rc) * g~) (or the fused multiply-add of it) to a score s it read
from memory, g~ = -logf(-logf(u)): the inner logf at 2 ulp moves t = -log u by a relative 4 u, hence log t by an absolute 4.04 u,
the outer logf adds 4 u |g|; the amplitude's rounding and the product's a relative 3 u, the final sum one rounding:
  noise_bound = amp (4.04 u + 4 u |g|) + 3 u amp |g| + u (|s + amp g| + 1)."""
import functools
import os
import shutil
import subprocess

import pytest
import torch

from conftest import ROOT, recorded_calls

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
INF = float('inf')
SCORE_SENTINEL = -123.0
TOKEN_SENTINEL = -5
FRAME = 8


def scaled(logits, temperature):
    """l = logits * fp32(1 / temperature): one fp32 multiply, on the CPU."""
    return logits.float().cpu() * torch.tensor(1.0 / temperature, dtype=torch.float32)


def framed(rows, cols, value, dtype):
    """A [rows, cols] view with FRAME sentinel columns either side of every row and FRAME sentinel rows above and below."""
    buf = torch.full((rows + 2 * FRAME, cols + 2 * FRAME), value, dtype=dtype, device='cuda')
    return buf, buf[FRAME:FRAME + rows, FRAME:FRAME + cols]


def frame_intact(buf, rows, cols, value):
    inner = torch.zeros_like(buf, dtype=torch.bool)
    inner[FRAME:FRAME + rows, FRAME:FRAME + cols] = True
    return bool((buf[~inner] == value).all())


# ---------------------------------------------------------------- 1. the scored scatter

SC_R, SC_RPC, SC_G = 60, 20, 50
SETTINGS = [(-1, 1, 1), ('k', 1, 1), (-1, 0.9, 1), ('k200', 0.8, 0.7), (-1, 1, 1.5), (-1, 1e-6, 1)]
CLASSES = [24, 1000, 2052, 8192]


@functools.lru_cache(maxsize=None)
def scatter_inputs(C):
    g = torch.Generator().manual_seed(6000 + C)
    ld = (C + 3) // 4 * 4 + 4
    logits = torch.full((SC_R, ld), 1e30)                                   # padding a kernel must never take for a class
    logits[:, :C] = torch.randn(SC_R, C, generator=g) * 3
    uniforms = torch.rand(SC_R, generator=g)
    idx = torch.cat([torch.randperm(SC_G, generator=g)[:SC_RPC] for _ in range(SC_R // SC_RPC)]).contiguous()
    known = ((torch.arange(SC_G).unsqueeze(0) + torch.arange(SC_R // SC_RPC).unsqueeze(1)) % 3 == 0).to(torch.uint8)
    return logits[:, :C].contiguous(), idx, known, logits.cuda(), uniforms.cuda(), idx.cuda(), known.cuda()


@functools.lru_cache(maxsize=None)
def score_reference(C, temperature):
    """fp64 pieces of the log-softmax of the scaled, unfiltered logits, and eta_row (module docstring): once per case."""
    l = scaled(scatter_inputs(C)[0], temperature).double()
    x = l - l.max(-1, keepdim=True).values
    w = x.exp()
    S = w.sum(-1)
    eta = (w * (3 * x.abs() + 2) * U).sum(-1) / S + 2 * C * U + C * 2.0 ** -126
    return x, S, eta


def raw_scatter(name, logits, C, top_k, top_p, temperature, idx, known, uniforms, *, scores=True):
    """One call of wmz_categorical_scatter_filtered / _scored; z, scores and samples inside sentinel frames.
    -> (samples, z, scores or None) on the CPU."""
    from world_modelz_amd import _lib as L
    R, ld, clips = logits.shape[0], logits.stride(0), SC_R // SC_RPC
    z_buf, z = framed(clips, SC_G, TOKEN_SENTINEL, torch.int64)
    s_buf, s = framed(clips, SC_G, SCORE_SENTINEL, torch.float32)
    d_buf, d = framed(1, R, -7, torch.int64)
    args = [L.ptr(logits), ld, R, C, top_k, float(top_p), 1.0 / float(temperature), L.ptr(idx), L.ptr(z), z.stride(0), SC_RPC, L.ptr(d),
            L.ptr(known), known.stride(0) if known is not None else 0, L.ptr(uniforms), None, 1234, 3 << 40, None, L.stream()]
    if name == 'wmz_categorical_scatter_scored':
        args += [L.ptr(s) if scores else None, s.stride(0)]
    L.call(name, *args)
    torch.cuda.synchronize()
    assert frame_intact(z_buf, clips, SC_G, TOKEN_SENTINEL) and frame_intact(d_buf, 1, R, -7), 'wrote outside its rows'
    assert frame_intact(s_buf, clips, SC_G, SCORE_SENTINEL), 'scores written outside the clip'
    if name != 'wmz_categorical_scatter_scored' or not scores:
        assert bool((s_buf == SCORE_SENTINEL).all())
    return d[0].cpu(), z.cpu(), s.cpu()


@pytest.mark.parametrize('setting', SETTINGS, ids=str)
@pytest.mark.parametrize('C', CLASSES)
def test_scored_scatter_draws_are_unchanged_and_scores_follow_the_law(C, setting):
    """3 clips x 20 rows in both forms of the kernel (registers, LDS), every filter setting of test_sparse_sampler_filters_gpu.py and
    the neutral one, uniforms injected, a third of the positions known: samples and z are torch.equal to
    wmz_categorical_scatter_filtered's given the same probe; every written score lies within the score bound (module docstring) of
    the fp64 log-softmax of the scaled UNFILTERED logits at the draw; scores at known positions, at positions outside indices and
    in the frames keep the sentinel; scores = NULL forwards."""
    top_k, top_p, temperature = setting
    top_k = {'k': 5 if C == 24 else 50, 'k200': min(200, C - 1)}.get(top_k, top_k)
    logits, idx, known, logits_dev, uniforms_dev, idx_dev, known_dev = scatter_inputs(C)
    want_d, want_z, _ = raw_scatter('wmz_categorical_scatter_filtered', logits_dev, C, top_k, top_p, temperature, idx_dev, known_dev, uniforms_dev)
    with recorded_calls() as seen:
        d, z, s = raw_scatter('wmz_categorical_scatter_scored', logits_dev, C, top_k, top_p, temperature, idx_dev, known_dev, uniforms_dev)
    assert seen == ['wmz_categorical_scatter_scored']
    assert torch.equal(d, want_d) and torch.equal(z, want_z)
    rows = torch.arange(SC_R)
    clip = rows // SC_RPC
    kn = known[clip, idx].bool()
    assert 0 < int(kn.sum()) < SC_R
    written = torch.zeros(SC_R // SC_RPC, SC_G, dtype=torch.bool)
    written[clip[~kn], idx[~kn]] = True
    assert bool((s[~written] == SCORE_SENTINEL).all())                      # known positions and positions outside indices
    assert torch.equal(z[written], d[~kn][torch.argsort(clip[~kn] * SC_G + idx[~kn])])
    x, S, eta = score_reference(C, temperature)
    assert float(eta.max()) < 0.01
    ref = x[rows, d] - S.log()
    bound = 1.01 * eta + 4 * U * (S.log().abs() + 0.01) + U * x[rows, d].abs() + U * (ref.abs() + 1)
    got = s[clip, idx].double()
    err = (got - ref).abs()[~kn]
    print(f'[scored scatter C={C} k={top_k} p={top_p} T={temperature}] worst |s - ref| = {float(err.max()):.3e}, worst err / bound = '
          f'{float((err / bound[~kn]).max()):.3f}, bound {float(bound.min()):.3e} .. {float(bound.max()):.3e}')
    assert bool((err <= bound[~kn]).all())
    d0, z0, _ = raw_scatter('wmz_categorical_scatter_scored', logits_dev, C, top_k, top_p, temperature, idx_dev, known_dev, uniforms_dev,
                            scores=False)
    assert torch.equal(d0, want_d) and torch.equal(z0, want_z)


@pytest.mark.parametrize('setting', [(-1, 1, 1), (10, 0.9, 0.7)], ids=str)
@pytest.mark.parametrize('C', CLASSES)
def test_a_row_with_one_finite_logit_scores_exactly_zero(C, setting):
    top_k, top_p, temperature = setting
    torch.manual_seed(C)
    _, idx, _, _, _, idx_dev, _ = scatter_inputs(C)
    ld = (C + 3) // 4 * 4
    logits = torch.full((SC_R, ld), -INF)
    cls = (torch.arange(SC_R) * 13 + 1) % C
    cls[0], cls[1] = 0, C - 1
    logits[torch.arange(SC_R), cls] = torch.randn(SC_R) * 5
    d, z, s = raw_scatter('wmz_categorical_scatter_scored', logits.cuda()[:, :C], C, top_k, top_p, temperature, idx_dev, None,
                          torch.rand(SC_R).cuda())
    assert torch.equal(d, cls)
    clip = torch.arange(SC_R) // SC_RPC
    assert bool((s[clip, idx] == 0).all()), s[clip, idx]
    assert int((s == SCORE_SENTINEL).sum()) == s.numel() - SC_R


def test_more_classes_than_the_limit():
    """16 385 classes: the raw entry point refuses (WMZ_ERR_UNSUPPORTED) and writes nothing; categorical_scatter draws through the
    neutral form of the filtered entry point and scores with torch ops -- the fp32 log-softmax of the scaled unfiltered logits at
    the draw, within 2 C u + 8 u (|ref| + |x_d| + 1) of fp64 (a sum of C terms in any order: (C - 1) u, the exps a few u each, the
    roundings of the subtractions) --, scattered where the position is not known."""
    from world_modelz_amd import _lib, ops
    from world_modelz_amd.sparse_diffusion import categorical_scatter
    C = ops.sample_max_classes() + 1
    torch.manual_seed(1)
    logits = torch.randn(1, 8, C, device='cuda') * 2
    idx = torch.randperm(20, device='cuda')[:8].reshape(1, 8).contiguous()
    z = torch.full((1, 20), TOKEN_SENTINEL, dtype=torch.int64, device='cuda')
    s = torch.full((1, 20), SCORE_SENTINEL, dtype=torch.float32, device='cuda')
    L = _lib
    with pytest.raises(_lib.WmzError, match=rf'code {_lib.CONSTANTS["WMZ_ERR_UNSUPPORTED"]}\b.*16384'):
        L.call('wmz_categorical_scatter_scored', L.ptr(logits), C, 8, C, -1, 1.0, 1.0, L.ptr(idx), L.ptr(z), 20, 8, None, None, 0, None, None,
               3, 0, None, L.stream(), L.ptr(s), 20)
    torch.cuda.synchronize()
    assert bool((z == TOKEN_SENTINEL).all()) and bool((s == SCORE_SENTINEL).all())
    known = torch.zeros(1, 20, dtype=torch.uint8, device='cuda')
    known[0, idx[0, :3]] = 1
    with recorded_calls() as seen:
        categorical_scatter(logits, idx, z, seed=3, call_id=1, top_k=1, temperature=0.8, known=known, scores=s)
    assert seen == ['wmz_categorical_scatter_filtered']
    l = scaled(logits[0], 0.8).double()
    d = l.argmax(-1)
    x = l - l.max(-1, keepdim=True).values
    ref = x[torch.arange(8), d] - x.exp().sum(-1).log()
    got = torch.gather(s, 1, idx)[0].cpu().double()
    assert torch.equal(torch.gather(z, 1, idx)[0, 3:].cpu(), d[3:]) and bool((torch.gather(z, 1, idx)[0, :3] == TOKEN_SENTINEL).all())
    assert bool((got[:3] == SCORE_SENTINEL).all())
    assert bool(((got - ref).abs()[3:] <= 2 * C * U + 8 * U * (ref.abs()[3:] + 1)).all())
    assert int((s == SCORE_SENTINEL).sum()) == 15


# ---------------------------------------------------------------- 2. the scored context draw

CTX_C = 24


def context_scores(B, G, seed):
    """Scores with ties (a grid of quarter steps), blocks of -inf (positions never drawn) and +inf, -0.0 and +0.0."""
    g = torch.Generator().manual_seed(seed)
    s = (torch.randn(B, G, generator=g) * 2).round() * 0.25
    s[:, ::7] = -INF
    s[:, G // 2:G // 2 + max(1, G // 8)] = -INF
    s[:, 3::11] = INF
    s[:, 5::13] = -0.0
    return s


def scored_draw(z, r, n, shape, scores, *, o=None, known=None, noise=0.0, seed=77, rank=1, call_id=9):
    """train.draw_sparse_context with scores; the probe inside a sentinel frame.  -> (indices, tokens, target, slot_scores)."""
    from world_modelz_amd.train import draw_sparse_context
    B = z.shape[0]
    buf = torch.full((B * n + 2 * FRAME,), SCORE_SENTINEL, dtype=torch.float32, device='cuda')
    slot = buf[FRAME:FRAME + B * n].view(B, n)
    with recorded_calls() as seen:
        out = draw_sparse_context(z, r, n, shape, CTX_C, seed=seed, rank=rank, call_id=call_id, o=o, p_uniform=0.0, known=known,
                                  scores=scores, noise=noise, slot_scores=slot)
    assert seen == ['wmz_sparse_draw_context_scored']
    torch.cuda.synchronize()
    assert bool((buf[:FRAME] == SCORE_SENTINEL).all()) and bool((buf[FRAME + B * n:] == SCORE_SENTINEL).all()), 'wrote outside the probe'
    return (*out, slot)


@pytest.mark.parametrize('with_known', [False, True], ids=['all-unknown', 'known'])
@pytest.mark.parametrize('given_o', [True, False], ids=['o-given', 'o-drawn'])
@pytest.mark.parametrize('S,HW,n', [(8, 16, 32), (8, 16, 20), (4, 256, 512), (2, 16, 1)])
def test_scored_context_draw_masks_exactly_the_lowest_scores(S, HW, n, given_o, with_known):
    """B = 3 clips with their own r (0 and 1 among them, two sets), noise = 0: indices and target are torch.equal to
    wmz_sparse_draw_context_known's for the same seed, stream id and call; slot_scores is the gathered score bit for bit; the
    masked set is the torch law on it (ties, -inf blocks, +inf; min(m, #candidates) slots, m = context_remask_count(r, n));
    a known slot is never masked; r = 0 masks nothing, r = 1 every candidate; the scores themselves are not written."""
    from world_modelz_amd.sample import context_remask_count, lowest_scores_mask
    from world_modelz_amd.train import draw_sparse_context
    torch.manual_seed(S * HW + n)
    B, G = 3, S * HW
    H, W = (4, HW // 4)
    z = torch.randint(0, CTX_C, (B, S, H, W), device='cuda')
    s_buf, scores = framed(B, G, SCORE_SENTINEL, torch.float32)
    scores.copy_(context_scores(B, G, n))
    before = s_buf.clone()
    known = (torch.rand(B, G, device='cuda') < 0.4).to(torch.uint8) if with_known else None
    for r in ([0.0, 1.0, 0.37], [0.62, 1 / 3, 1.0]):
        r = torch.tensor(r, device='cuda')
        o = torch.tensor([0.0, 0.5, 0.99], device='cuda') if given_o else None
        ref = draw_sparse_context(z, r, n, (S, H, W), CTX_C, seed=77, rank=1, call_id=9, o=o, p_uniform=0.0,
                                  known=known if with_known else torch.zeros(B, G, dtype=torch.uint8, device='cuda'))
        idx, tok, tgt, slot = scored_draw(z, r, n, (S, H, W), scores, o=o, known=known)
        assert torch.equal(idx, ref[0]) and torch.equal(tgt, ref[2])
        assert torch.equal(tgt, torch.gather(z.view(B, -1), 1, idx))
        assert torch.equal(slot.view(torch.int32), torch.gather(scores, 1, idx).view(torch.int32))
        cand = torch.gather(known, 1, idx) == 0 if with_known else torch.ones_like(idx, dtype=torch.bool)
        m = context_remask_count(r, n)
        want = lowest_scores_mask(slot, None, cand, count=m)
        masked = tok == CTX_C
        assert torch.equal(masked, want)
        assert torch.equal(tok, torch.where(want, torch.full_like(tgt, CTX_C), tgt))
        assert not bool((masked & ~cand).any())
        assert torch.equal(masked.sum(-1), torch.minimum(cand.sum(-1), m.to(cand.device)))
        for b in range(B):
            if float(r[b]) == 0.0:
                assert int(masked[b].sum()) == 0
            if float(r[b]) == 1.0:
                assert torch.equal(masked[b], cand[b])
    assert torch.equal(s_buf, before)


def test_scored_context_draw_refuses_what_the_law_excludes():
    """p_uniform != 0, a NULL scores, a negative or infinite noise: WMZ_ERR_ARG, nothing written."""
    from world_modelz_amd import _lib as L
    B, S, HW, n = 2, 8, 16, 32
    z = torch.randint(0, CTX_C, (B, S * HW), device='cuda')
    r = torch.ones(B, device='cuda')
    out = [torch.full((B, n), TOKEN_SENTINEL, dtype=torch.int64, device='cuda') for _ in range(3)]
    scores = torch.zeros(B, S * HW, device='cuda')

    def call(p_uniform, s, noise):
        L.call('wmz_sparse_draw_context_scored', L.ptr(z), z.stride(0), L.ptr(r), None, *(L.ptr(t) for t in out), B, S, HW, n, CTX_C,
               p_uniform, 5, 1 << 40, None, L.stream(), None, 0, L.ptr(s), S * HW, noise, None)
    for bad in ((0.1, scores, 0.0), (0.0, None, 0.0), (0.0, scores, -1.0), (0.0, scores, INF)):
        with pytest.raises(L.WmzError, match=rf'code {L.CONSTANTS["WMZ_ERR_ARG"]}\b'):
            call(*bad)
    torch.cuda.synchronize()
    assert all(bool((t == TOKEN_SENTINEL).all()) for t in out)
    call(0.0, scores, 0.0)
    torch.cuda.synchronize()
    assert bool((out[1] == CTX_C).all())                                   # (r = 1: every slot hidden)


# ---------------------------------------------------------------- 3. the noise

CXX = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/llvm/bin/clang++')
            if c and os.path.exists(c)), None)


def philox_third_units(tmp_path, indices, stream, seed):
    """u of the third word of philox4(index, stream, seed) for every index, from the generator's own header on the host
    (tests/philox_host.cpp)."""
    assert CXX is not None, 'no host C++ compiler'
    exe = str(tmp_path / 'philox_host')
    r = subprocess.run([CXX, '-std=c++17', '-O1', os.path.join(ROOT, 'tests', 'philox_host.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    args = [exe]
    for i in indices:
        args += ['b', str(i), str(stream), str(seed)]
    out = subprocess.run(args, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return torch.tensor([float.fromhex(line.split()[6]) for line in out.stdout.splitlines()], dtype=torch.float64)


def test_noise_is_the_annealed_gumbel_of_the_slot_s_own_uniform(tmp_path):
    """8 x 16 grid, n = 32, r = (0.5, 1, 0.25), noise = 0.5, a known map: the masked set is the torch law applied to the returned
    slot_scores, exactly; slot_scores - gathered = noise * rc * g(u) within the noise bound (module docstring), u the third word of
    philox4(b n + i, (rank << 40) | call, seed) recomputed on the host; indices and target are the draw's without noise."""
    from world_modelz_amd.sample import context_remask_count, lowest_scores_mask
    torch.manual_seed(2)
    B, S, H, W, n = 3, 8, 4, 4, 32
    G = S * H * W
    z = torch.randint(0, CTX_C, (B, S, H, W), device='cuda')
    scores = (torch.randn(B, G, device='cuda') * 2).contiguous()
    known = (torch.rand(B, G, device='cuda') < 0.3).to(torch.uint8)
    r = torch.tensor([0.5, 1.0, 0.25], device='cuda')
    noise, seed, rank, call = 0.5, 77, 1, 9
    idx0, _, tgt0, slot0 = scored_draw(z, r, n, (S, H, W), scores, known=known, seed=seed, rank=rank, call_id=call)
    idx, tok, tgt, slot = scored_draw(z, r, n, (S, H, W), scores, known=known, noise=noise, seed=seed, rank=rank, call_id=call)
    assert torch.equal(idx, idx0) and torch.equal(tgt, tgt0)
    cand = torch.gather(known, 1, idx) == 0
    want = lowest_scores_mask(slot, None, cand, count=context_remask_count(r, n))
    assert torch.equal(tok == CTX_C, want) and torch.equal(tok, torch.where(want, torch.full_like(tgt, CTX_C), tgt))
    u = philox_third_units(tmp_path, range(B * n), (rank << 40) | call, seed).view(B, n)
    assert float(u.min()) >= 0 and float(u.max()) < 1 and u.unique().numel() > B * n // 2
    g = -torch.log(-torch.log(u))
    amp = (noise * r.cpu().double()).unsqueeze(1)
    s = slot0.cpu().double()
    ref = s + amp * g
    fin = u > 0
    bound = amp * (4.04 * U + 4 * U * g.abs()) + 3 * U * amp * g.abs() + U * (ref.abs() + 1)
    err = (slot.cpu().double() - ref).abs()
    print(f'[context noise] worst err / bound = {float((err[fin] / bound[fin]).max()):.3f}, worst |err| = {float(err[fin].max()):.3e}')
    assert bool((err[fin] <= bound[fin]).all()) and bool((slot.cpu()[~fin] == -INF).all())
    assert float((slot.cpu().double() - s).abs().min()) > 0                # (the noise does act)


def test_noise_alone_hides_every_slot_half_of_the_time():
    """All scores equal, noise = 0.5, n = 32, r = 0.5, 200 call numbers: every clip has exactly 16 hidden slots in every call, and each
    slot of each clip is hidden with a frequency within six binomial standard deviations, 6 sqrt(1 / (4 * 200)), of 1 / 2."""
    torch.manual_seed(3)
    from world_modelz_amd.train import draw_sparse_context
    B, S, H, W, n, calls = 3, 8, 4, 4, 32, 200
    z = torch.randint(0, CTX_C, (B, S, H, W), device='cuda')
    scores = torch.zeros(B, S * H * W, device='cuda')
    r = torch.full((B,), 0.5, device='cuda')
    ctr = torch.zeros(1, dtype=torch.int64, device='cuda')
    hidden = []
    for _ in range(calls):
        ctr.add_(1)
        _, tok, _ = draw_sparse_context(z, r, n, (S, H, W), CTX_C, seed=5, rank=0, counter=ctr, p_uniform=0.0, scores=scores, noise=0.5)
        hidden.append(tok == CTX_C)
    hidden = torch.stack(hidden).cpu()                                      # [calls, B, n]
    assert bool((hidden.sum(-1) == 16).all())
    freq = hidden.double().mean(0)
    sd = (0.25 / calls) ** 0.5
    print(f'[noise only] slot frequencies {float(freq.min()):.3f} .. {float(freq.max()):.3f}, 6 sd = {6 * sd:.3f}')
    assert bool(((freq - 0.5).abs() <= 6 * sd).all())


# ---------------------------------------------------------------- 4. sample_clips, stand-in model

S_, H_, W_, C_, N_ = 8, 4, 4, 24, 32
G_ = S_ * H_ * W_
ITERATIONS = 16           # 80 sub-steps: the first 20 alone, whose windows span 7 of the 8 frames, miss a position with probability
#                           (1 - 32 / 112)^20 ~ 1e-3, the 60 behind them bring that below 1e-10: every position is drawn
OFFSETS = G_ // N_ + 1
SPARSE = ('wmz_sparse_draw_context', 'wmz_sparse_draw_context_known', 'wmz_sparse_draw_context_scored', 'wmz_categorical_scatter',
          'wmz_categorical_scatter_filtered', 'wmz_categorical_scatter_scored')


class Stub(torch.nn.Module):
    """logits = 2 * one_hot(position mod C) + fixed noise of amplitude 0.9: the position's own class is every row's argmax, with a
    probability (the score under sample_topk = 1) that differs from position to position.  Records, on the device, the tokens and
    the indices of every call (row `calls` of two buffers: capturable, nothing returns to the host)."""

    def __init__(self, records):
        super().__init__()
        self.shape = (S_, H_, W_)
        self.embedding = torch.nn.Embedding(C_ + 1, 8)
        self.register_buffer('noise', 0.9 * (2 * torch.rand(G_, C_, generator=torch.Generator().manual_seed(5)) - 1))
        self.register_buffer('calls', torch.zeros(1, dtype=torch.int64))
        self.register_buffer('rec_tokens', torch.full((records, 2, N_), -1, dtype=torch.int64))
        self.register_buffer('rec_indices', torch.full((records, 2, N_), -1, dtype=torch.int64))

    def forward(self, tokens, indices):
        self.rec_tokens.index_copy_(0, self.calls, tokens.unsqueeze(0))
        self.rec_indices.index_copy_(0, self.calls, indices.unsqueeze(0))
        self.calls += 1
        own = torch.arange(C_, device=indices.device) == (indices % C_).unsqueeze(-1)       # (no one_hot: it reads back)
        return 2.0 * own.float() + self.noise[indices]


def prompt_of(with_prompt):
    if not with_prompt:
        return None
    pos = torch.arange(G_, device='cuda')
    prompt = torch.full((2, G_), C_, dtype=torch.int64, device='cuda')
    prompt[:, :G_ // 2] = (pos[:G_ // 2] + 1) % C_                          # frames 0-3 given, and a few scattered positions
    prompt[:, G_ // 2 + 3::17] = 1
    return prompt.view(2, S_, H_, W_)


_RUNS = {}


def run_route(route, with_prompt):
    """One sample_clips(remask='confidence', sample_topk=1, remask_noise=0) call per (route, prompt), shared by the tests below:
    -> (clip [2, G], the entry points reached, the sub-steps' (tokens, indices) on the CPU)."""
    key = (route, with_prompt)
    if key in _RUNS:
        return _RUNS[key]
    from world_modelz_amd import _lib as L
    from world_modelz_amd.sparse_diffusion import sample_clips
    stub = Stub(ITERATIONS * OFFSETS + 2).cuda()
    lib = L.lib()
    supported = lib.wmz_sparse_draw_context_supported
    if route == 'torch-drawn':
        lib.wmz_sparse_draw_context_supported = lambda *a: 0
    try:
        torch.manual_seed(17)
        with recorded_calls() as seen:
            z = sample_clips(stub, 2, C_, 'uniform' if route == 'uniform' else 'neighbors', num_context=N_, num_eval_iterations=ITERATIONS,
                             generator=torch.Generator().manual_seed(3), seed=11, use_graph=route == 'captured', sample_topk=1,
                             prompt=prompt_of(with_prompt), remask='confidence', remask_noise=0.0).view(2, -1)
    finally:
        lib.wmz_sparse_draw_context_supported = supported
    torch.cuda.synchronize()
    first = 1 if route == 'captured' else 0                                 # (the captured route's warm-up sub-step comes first)
    count = int(stub.calls) - first
    records = [(stub.rec_tokens[first + k].cpu(), stub.rec_indices[first + k].cpu()) for k in range(count)]
    _RUNS[key] = (z.cpu(), [s for s in seen if s in SPARSE], records)
    return _RUNS[key]


ROUTES = ['captured', 'eager', 'torch-drawn', 'uniform']


@pytest.mark.parametrize('with_prompt', [False, True], ids=['from-masks', 'prompt'])
@pytest.mark.parametrize('route', ROUTES)
def test_sample_clips_hides_exactly_the_counted_slots_on_every_route(route, with_prompt):
    """Every route finishes with position mod C at every generated position (all are drawn: see ITERATIONS) and the prompt untouched
    at the given ones.  Every sub-step's model input, recorded through the stand-in model: no mask token at a given slot, and among
    the unknown slots exactly max(min(m, #unknown slots), #unknown slots never drawn before) mask tokens, m = context_remask_count of
    the iteration's r: the m lowest-scored slots are hidden, never-drawn ones (score -inf) first, and a never-drawn slot holds
    the mask token whether it is selected or not.  (min(m, #unknown): with a prompt a context can hold fewer unknown slots than m.)
    The fused routes reach the two scored entry points and no other of the sparse family."""
    from world_modelz_amd.sample import context_remask_count
    z, seen, records = run_route(route, with_prompt)
    prompt = prompt_of(with_prompt)
    given = (prompt.view(2, -1) != C_).cpu() if with_prompt else torch.zeros(2, G_, dtype=torch.bool)
    own = (torch.arange(G_) % C_).expand(2, -1)
    if with_prompt:
        assert torch.equal(z[given], prompt.view(2, -1).cpu()[given])
    assert torch.equal(z[~given], own[~given])
    if route in ('captured', 'eager'):
        assert set(seen) == {'wmz_sparse_draw_context_scored', 'wmz_categorical_scatter_scored'}
    else:
        assert set(seen) == {'wmz_categorical_scatter_scored'}
    per_iteration = G_ // N_ if route == 'uniform' else OFFSETS
    assert len(records) == ITERATIONS * per_iteration
    drawn = torch.zeros(2, G_, dtype=torch.bool)
    some_choice = 0
    for k, (tok, idx) in enumerate(records):
        i = k // per_iteration
        r = torch.full((2,), 1.0 - i / (ITERATIONS - 1), dtype=torch.float32)
        m = context_remask_count(r, N_)
        unknown = ~torch.gather(given, 1, idx)
        fresh = unknown & ~torch.gather(drawn, 1, idx)
        masks = tok == C_
        assert not bool((masks & ~unknown).any()), k
        want = torch.maximum(torch.minimum(m, unknown.sum(-1)), fresh.sum(-1))
        assert torch.equal((masks & unknown).sum(-1), want), (k, masks.sum(-1), want)
        assert bool((masks | ~fresh).all()), k
        some_choice += int(((fresh.sum(-1) < m) & (m < unknown.sum(-1))).sum())
        drawn.scatter_(1, idx, torch.ones_like(idx, dtype=torch.bool))
    assert some_choice > ITERATIONS                                          # (sub-steps in which the scores, not the start, decided)


@pytest.mark.parametrize('with_prompt', [False, True], ids=['from-masks', 'prompt'])
def test_sample_clips_routes_agree(with_prompt):
    """Captured and eager-fused are torch.equal -- the clip and every sub-step's model input --; the fused routes and the
    torch-drawn route are torch.equal in the clip."""
    zc, _, rc = run_route('captured', with_prompt)
    ze, _, re_ = run_route('eager', with_prompt)
    zt, _, _ = run_route('torch-drawn', with_prompt)
    assert torch.equal(zc, ze) and len(rc) == len(re_)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(rc, re_))
    assert torch.equal(ze, zt)


@pytest.mark.parametrize('use_graph', [True, False], ids=['captured', 'eager'])
def test_the_random_rule_runs_the_launches_it_always_ran(use_graph):
    """remask='random' with a remask_noise: no scored entry point, and the clip of the default call, bit for bit."""
    from world_modelz_amd.sparse_diffusion import sample_clips
    stub = Stub(5 * OFFSETS + 2).cuda()
    out = []
    for kw in (dict(), dict(remask='random', remask_noise=0.7)):
        stub.calls.zero_()
        with recorded_calls() as seen:
            out.append(sample_clips(stub, 2, C_, 'neighbors', num_context=N_, num_eval_iterations=5, generator=torch.Generator().manual_seed(3),
                                    seed=11, use_graph=use_graph, **kw))
        assert {s for s in seen if s in SPARSE} == {'wmz_sparse_draw_context', 'wmz_categorical_scatter'}
    assert torch.equal(out[0], out[1])
    stub.calls.zero_()
    with recorded_calls() as seen:
        sample_clips(stub, 2, C_, 'neighbors', num_context=N_, num_eval_iterations=5, generator=torch.Generator().manual_seed(3), seed=11,
                     use_graph=use_graph, sample_topk=3, prompt=prompt_of(True), remask='random', remask_noise=0.7)
    assert {s for s in seen if s in SPARSE} == {'wmz_sparse_draw_context_known', 'wmz_categorical_scatter_filtered'}


# ---------------------------------------------------------------- 5. a real small model

REAL_SEED = 13


def test_real_model_captured_and_eager_agree():
    """VqSparseDiffusionModel on a 4 x 8 x 8 grid, dim 64, 40 classes, 16-token contexts, 3 iterations, bf16, remask='confidence' with
    remask_noise = 0.3, top-k 5 and a prompt: the captured sub-step and the eager launches give the same clip through the scored
    entry points; the prompt comes back untouched and every token lies in [0, C).  (3 iterations of 17 contexts draw a position
    with a probability of about 0.96 only, so the prompt leaves two rows of the last frame -- 16 positions a clip -- to generate, and
    REAL_SEED is one for which the contexts -- a function of the seed alone: Philox -- reach all of them.)  evaluate_model passes the
    arguments on."""
    from world_modelz_amd import config
    from world_modelz_amd.sparse_diffusion import VqSparseDiffusionModel, evaluate_model, sample_clips
    torch.manual_seed(4)
    B, S, H, W, C, n = 2, 4, 8, 8, 40, 16
    m = VqSparseDiffusionModel(shape=(S, H, W), dim=64, num_classes=C, depth=2, dim_head=32, mlp_dim=96, heads=2).cuda()
    prompt = torch.randint(0, C, (B, S, H, W), device='cuda')
    prompt[:, 3, :2] = C
    given = prompt != C
    assert int((~given).sum()) == B * 16
    with config.compute_dtype(torch.bfloat16):
        out = []
        for use_graph in (True, False):
            with recorded_calls() as seen:
                out.append(sample_clips(m, B, C, 'neighbors', num_context=n, num_eval_iterations=3, seed=REAL_SEED,
                                        generator=torch.Generator().manual_seed(1), use_graph=use_graph, sample_topk=5, prompt=prompt,
                                        remask='confidence', remask_noise=0.3))
            assert {s for s in seen if s in SPARSE} == {'wmz_sparse_draw_context_scored', 'wmz_categorical_scatter_scored'}
        assert torch.equal(out[0], out[1])
        assert torch.equal(out[0][given], prompt[given])
        assert int(out[0].min()) >= 0 and int(out[0].max()) < C

        class Decoder:
            class vq:
                num_embeddings = C

            @staticmethod
            def decode(tokens):
                return tokens.float().unsqueeze(1)
        with recorded_calls() as seen:
            frames = evaluate_model('cuda', B, m, Decoder, (S, H, W), 'neighbors', n, 3, sample_topk=5, prompt=prompt, remask='confidence',
                                    remask_noise=0.3)
        assert 'wmz_sparse_draw_context_scored' in seen and 'wmz_categorical_scatter_scored' in seen
        assert tuple(frames.shape) == (B, S, 1, H, W)
