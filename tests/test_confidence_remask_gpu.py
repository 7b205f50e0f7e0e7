"""Confidence-ordered re-masking on the device: wmz_sample_tokens_scored_dev (the draw of wmz_sample_tokens_filtered_dev plus the
log-probability of each draw), wmz_remask_lowest_dev (the per-clip selection of the lowest scores) and sample_frames(remask=
'confidence') on top of the pair.  include/wmz.h states the law; its torch form is sample.confidence_scores /
sample.lowest_scores_mask (held to a brute-force sort in test_confidence_remask_cpu.py).

The score bound, from the kernel's operations, u = 2^-24 the unit roundoff of fp32.  The kernel computes
    s = fl(fl(l_d - max) - logf(S~)),  S~ = the fp32 sum, in some order, of the C terms __expf(fl(l_c - max)).
  * one term: fl(l_c - max) = x (1 + d), |d| <= u, moves exp(x) by a relative |x| u; __expf(x) is the hardware's 2^y at
    y = fl(x * log2e) -- the rounding of the product and of the constant move the result by a relative <= 1.5 |x| u, the 2^y
    instruction itself is accurate to 1 ulp = 2 u (AMD's ISA guide; the HIP math tables give __expf 1 ulp on top of its argument
    error).  Together <= (2.5 |x| + 2) u, taken as d(x) = (3 |x| + 2) u.  A term below the smallest normal may be flushed to 0: an
    absolute 2^-126 each.
  * the sum: n positive terms added in any order: relative (n - 1) u / (1 - (n - 1) u) (Higham, Accuracy and Stability of
    Numerical Algorithms, eq. 4.4), taken as 2 C u like test_sampler_filters_gpu.eps_of.
    So S~ = S (1 + eta), |eta| <= eta_row = sum_c w_c d(x_c) / S + 2 C u + C 2^-126 (S >= 1: the maximum's own term is 1), w and
    S in fp64.
  * logf is accurate to 1 ulp (HIP math tables), taken as 2: |logf(S~) - log S~| <= 4 u |log S~|; log S~ = log S + log(1 + eta),
    |log(1 + eta)| <= 1.01 eta_row for the eta_row < 0.01 that these shapes give (asserted).
  * the two subtractions round once each: u |l_d - max| + u |s|.
  bound = 1.01 eta_row + 4 u (|log S| + 0.01) + u |l_d - max| + u (|s| + 1).
With noise the kernel adds fl(fl(noise * fl(1 - alpha)) * g~) (or the fused multiply-add of it), g~ = -logf(-logf(u1)): the inner
logf at 2 ulp moves t = -log u1 by a relative 4 u, hence log t by an absolute 4 u (1.01), the outer logf adds 4 u |g|; the
amplitude's two roundings a relative 2 u, the product and the final sum one rounding each:
  noise_bound = amp (4.04 u + 4 u |g|) + 3 u amp |g| + u (|s + amp g| + 1)."""
import functools
import math

import pytest
import torch

from conftest import recorded_calls

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ALPHA = 0.25
FILTERS = [(-1, 1.0, 1.0), (10, 1.0, 1.0), (-1, 0.9, 0.7)]
CLASSES = [37, 1000, 2052]
R0, CLIPS = 60, 3


def scaled(logits, temperature):
    """l = logits * fp32(1 / temperature): one fp32 multiply, on the CPU."""
    return logits.float().cpu() * torch.tensor(1.0 / temperature, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def inputs(C):
    g = torch.Generator().manual_seed(4000 + C)
    ld = (C + 3) // 4 * 4
    logits = torch.randn(R0, ld, generator=g) * 3
    logits[:, C:] = 1e30                                                    # padding a kernel must never take for a class
    uniforms = torch.rand(R0, 2, generator=g)
    uniforms[0, 1] = 0.0
    uniforms[1, 1] = 1.0 - 2.0 ** -24                                       # the largest fp32 below 1
    return logits, uniforms, logits.cuda(), uniforms.cuda()


@functools.lru_cache(maxsize=None)
def reference(C, temperature):
    """fp64 log-softmax of the scaled, unfiltered logits, its pieces, and eta_row (module docstring): computed once per case."""
    l = scaled(inputs(C)[0][:, :C], temperature).double()
    mx = l.max(-1, keepdim=True).values
    x = l - mx
    w = x.exp()
    S = w.sum(-1)
    eta = (w * (3 * x.abs() + 2) * U).sum(-1) / S + 2 * C * U + C * 2.0 ** -126
    return x, S, eta


def run_scored(logits_dev, C, top_k, top_p, temperature, *, uniforms=None, noise=0.0, alphas=(ALPHA,), counter=0, seed=1234,
               last_mask=None, clips=CLIPS, frame=8):
    """One ops.sample_tokens_confidence call; denoised and scores live inside sentinel frames that must come back intact, the
    tokens in the last frame of a [clips, 2, HW] grid whose first frame must.  -> (draws, tokens [R], scores), on the CPU."""
    from world_modelz_amd import ops
    R = logits_dev.shape[0]
    dev = logits_dev.device
    den_buf = torch.full((R + 2 * frame,), -7, dtype=torch.int64, device=dev)
    sc_buf = torch.full((R + 2 * frame,), -123.0, dtype=torch.float32, device=dev)
    z = torch.full((clips, 2, R // clips), -5, dtype=torch.int64, device=dev)
    ops.sample_tokens_confidence(logits_dev[:, :C], top_k, torch.tensor(alphas, dtype=torch.float32, device=dev), C, z[:, -1],
                                 den_buf[frame:frame + R], torch.tensor([counter], dtype=torch.int64, device=dev), seed, last_mask,
                                 top_p=top_p, temperature=temperature, noise=noise, uniforms=uniforms, scores=sc_buf[frame:frame + R])
    torch.cuda.synchronize()
    for buf, s in ((den_buf, -7), (sc_buf, -123.0)):
        assert bool((buf[:frame] == s).all()) and bool((buf[frame + R:] == s).all()), 'wrote outside its rows'
    assert bool((z[:, 0] == -5).all())
    return den_buf[frame:frame + R].cpu(), z[:, -1].reshape(R).cpu(), sc_buf[frame:frame + R].cpu()


def run_random(logits_dev, C, top_k, top_p, temperature, uniforms):
    from world_modelz_amd import ops
    R = logits_dev.shape[0]
    dev = logits_dev.device
    den = torch.full((R,), -7, dtype=torch.int64, device=dev)
    z = torch.full((CLIPS, 2, R // CLIPS), -5, dtype=torch.int64, device=dev)
    ops.sample_tokens(logits_dev[:, :C], top_k, torch.tensor([ALPHA], dtype=torch.float32, device=dev), C, z[:, -1], den,
                      torch.tensor([0], dtype=torch.int64, device=dev), 1234, None, top_p=top_p, temperature=temperature,
                      uniforms=uniforms)
    torch.cuda.synchronize()
    return den.cpu()


# ---------------------------------------------------------------- 1. the draw is the filtered entry point's, the score the law's

@pytest.mark.parametrize('top_k,top_p,temperature', FILTERS)
@pytest.mark.parametrize('C', CLASSES)
def test_draws_are_unchanged_and_scores_follow_the_law(C, top_k, top_p, temperature):
    """Register kernel small and full, wide kernel; 3 clips of 20 rows; uniforms injected.  denoised is torch.equal to
    wmz_sample_tokens_filtered_dev's; with noise = 0 every score lies within the score bound of the fp64 log-softmax of the scaled
    unfiltered logits at the draw; with noise = 0.5 and injected u1 (0 and the largest fp32 below 1 among them) within
    the score bound + the noise bound of the fp64 formula, -inf exactly at u1 = 0; the selection then masks exactly the m lowest per clip."""
    from world_modelz_amd.sample import lowest_scores_mask, remask_count
    logits, uniforms, logits_dev, uniforms_dev = inputs(C)
    want = run_random(logits_dev, C, top_k, top_p, temperature, uniforms_dev)
    d, tok, s = run_scored(logits_dev, C, top_k, top_p, temperature, uniforms=uniforms_dev)
    assert torch.equal(d, want)
    x, S, eta = reference(C, temperature)
    rows = torch.arange(R0)
    assert float(eta.max()) < 0.01
    ref = x[rows, d] - S.log()
    bound = 1.01 * eta + 4 * U * (S.log().abs() + 0.01) + U * x[rows, d].abs() + U * (ref.abs() + 1)
    err = (s.double() - ref).abs()
    print(f'[score C={C} k={top_k} p={top_p} T={temperature}] worst |s - ref| = {float(err.max()):.3e}, worst err / bound = '
          f'{float((err / bound).max()):.3f}, bound {float(bound.min()):.3e} .. {float(bound.max()):.3e}')
    assert bool((err <= bound).all())
    mask = lowest_scores_mask(s.view(CLIPS, -1), ALPHA)
    assert int(mask.sum(-1).min()) == int(mask.sum(-1).max()) == remask_count(ALPHA, R0 // CLIPS) == 15
    assert torch.equal(tok, torch.where(mask.view(-1), torch.full_like(d, C), d))
    # the Gumbel term
    noise = 0.5
    dn, _, sn = run_scored(logits_dev, C, top_k, top_p, temperature, uniforms=uniforms_dev, noise=noise)
    assert torch.equal(dn, want)
    u1 = uniforms[:, 1].double()
    a32 = torch.tensor(ALPHA, dtype=torch.float32).double()
    amp = noise * (1 - float(a32))
    gum = -torch.log(-torch.log(u1))
    refn = ref + amp * gum
    fin = u1 > 0
    nbound = bound + amp * (4.04 * U + 4 * U * gum.abs()) + 3 * U * amp * gum.abs() + U * (refn.abs() + 1)
    errn = (sn.double() - refn).abs()
    print(f'[score + noise C={C}] worst err / bound = {float((errn[fin] / nbound[fin]).max()):.3f}; u1 = 1 - 2^-24: g = {float(gum[1]):.4f}, '
          f's = {float(sn[1]):.6f} (ref {float(refn[1]):.6f})')
    assert float(sn[0]) == -float('inf') and not bool(fin[0])
    assert bool((errn[fin] <= nbound[fin]).all())


@pytest.mark.parametrize('top_k,top_p,temperature', FILTERS)
@pytest.mark.parametrize('C', CLASSES)
def test_a_row_with_one_finite_logit_scores_exactly_zero(C, top_k, top_p, temperature):
    torch.manual_seed(C)
    ld = (C + 3) // 4 * 4
    logits = torch.full((R0, ld), -float('inf'))
    cls = (torch.arange(R0) * 13 + 1) % C
    cls[0], cls[1] = 0, C - 1
    logits[torch.arange(R0), cls] = torch.randn(R0) * 5
    d, _, s = run_scored(logits.cuda(), C, top_k, top_p, temperature, uniforms=torch.rand(R0, 2).cuda())
    assert torch.equal(d, cls)
    assert bool((s == 0).all()), s


# ---------------------------------------------------------------- 2. the selection is exact

MASK = 99999


def selection_scores(kind, clips, n, g):
    if kind == 'random':
        return torch.randn(clips, n, generator=g)
    if kind == 'equal':
        return torch.full((clips, n), -0.75)
    if kind == 'two-valued':                                                # 30 % low: at alpha = 0.5 the threshold falls inside the run of -0.5
        return torch.where(torch.rand(clips, n, generator=g) < 0.3, torch.tensor(-2.0), torch.tensor(-0.5))
    s = torch.randn(clips, n, generator=g)
    pool = torch.tensor([float('inf'), -float('inf'), 0.0, -0.0, -float('inf'), float('inf')])
    s[:, ::2] = pool[torch.arange(s[:, ::2].shape[1]) % len(pool)]
    return s


def max_rows():
    from world_modelz_amd import ops
    return ops.remask_max_rows()


SEL_ALPHAS = [0.0, 1 / 30, 0.5, 29 / 30, 1.0]


@pytest.mark.parametrize('n', [1, 20, 256, 257, 'max'])
def test_selection_is_exactly_the_lowest_scores(n):
    """wmz_remask_lowest_dev alone on written scores (random, all equal, two-valued with the threshold inside a tie run, +-inf and
    signed zeros), planes of 1, 20, 256 (the one-wave form's last), 257 (the workgroup form's first) and the limit, with and without
    last_mask (half set, fewer ones than m, none), alpha in {0, 1/30, 0.5, 29/30, 1} picked by the counter: out_tokens and
    last_mask are torch.equal to sample.lowest_scores_mask's; everything around them stays."""
    from world_modelz_amd import ops
    from world_modelz_amd.sample import lowest_scores_mask
    n = max_rows() if n == 'max' else n
    clips = 1 if n == max_rows() else 3
    R, frame = clips * n, 8
    g = torch.Generator().manual_seed(n)
    alphas = torch.tensor(SEL_ALPHAS, dtype=torch.float32, device='cuda')
    few = torch.zeros(clips, n, dtype=torch.bool)
    few[:, n // 2: n // 2 + max(1, n // 9)] = True
    masks = {'none given': None, 'half': torch.rand(clips, n, generator=g) < 0.5, 'few': few, 'no candidate': torch.zeros(clips, n, dtype=torch.bool)}
    for kind in ('random', 'equal', 'two-valued', 'special'):
        scores = selection_scores(kind, clips, n, g)
        sc_buf = torch.full((R + 2 * frame,), float('nan'), device='cuda')
        sc_buf[frame:frame + R] = scores.reshape(-1).cuda()
        for i, alpha in enumerate(SEL_ALPHAS):
            for mname, cand in masks.items():
                z = torch.full((clips, 2, n), -5, dtype=torch.int64, device='cuda')
                lm_buf = torch.full((R + 2 * frame,), 7, dtype=torch.uint8, device='cuda')
                lm = None
                if cand is not None:
                    lm = lm_buf[frame:frame + R]
                    lm.copy_(cand.reshape(-1).to(torch.uint8) * 3)                   # (any non-zero byte is a candidate)
                ops.remask_lowest(sc_buf[frame:frame + R], alphas, MASK, z[:, -1], torch.tensor([i + 10], dtype=torch.int64, device='cuda'), lm)
                want = lowest_scores_mask(scores, float(alphas[i].cpu()), cand)
                if alpha in (0.0, 1.0):                                              # every candidate / nothing
                    assert torch.equal(want, (torch.ones(clips, n, dtype=torch.bool) if cand is None else cand) & (alpha == 0.0))
                got = z.cpu()
                assert torch.equal(got[:, -1], torch.where(want, torch.tensor(MASK), torch.tensor(-5))), (kind, alpha, mname)
                assert bool((got[:, 0] == -5).all())
                lmc = lm_buf.cpu()
                assert bool((lmc[:frame] == 7).all()) and bool((lmc[frame + R:] == 7).all())
                if cand is not None:
                    assert torch.equal(lmc[frame:frame + R].view(clips, n), want.to(torch.uint8)), (kind, alpha, mname)
                else:
                    assert bool((lmc == 7).all())


def test_more_rows_than_the_limit_are_refused_and_nothing_is_written():
    from world_modelz_amd import _lib, ops
    n = ops.remask_max_rows() + 1
    assert n == 4097
    scores = torch.randn(n, device='cuda')
    z = torch.full((1, 2, n), -5, dtype=torch.int64, device='cuda')
    lm = torch.ones(n, dtype=torch.uint8, device='cuda')
    with pytest.raises(_lib.WmzError, match=rf'code {_lib.CONSTANTS["WMZ_ERR_UNSUPPORTED"]}\b.*4096'):
        ops.remask_lowest(scores, torch.tensor([0.5], device='cuda'), MASK, z[:, -1], torch.zeros(1, dtype=torch.int64, device='cuda'), lm)
    torch.cuda.synchronize()
    assert bool((z == -5).all()) and bool((lm == 1).all())


# ---------------------------------------------------------------- 3. the pair

@pytest.mark.parametrize('C', [37, 2052])
def test_one_step_masks_the_least_confident_rows_and_the_counter_walks_alpha(C):
    """Row r has one dominant class, its own, with a per-row gap over flat other logits, and a u0 in the middle of that class's CDF
    interval: the draw is that class, its log-probability differs from every other row's by >= 1e-3 (asserted in fp64), far above
    the score bound.  After one step the masked rows of each clip are exactly the m lowest; counters 0, 1, 2 walk alpha through
    `alphas`; with last_mask only earlier-masked rows are candidates and the bytes become the new mask."""
    from world_modelz_amd.sample import remask_count
    HW = R0 // CLIPS
    g = torch.Generator().manual_seed(C)
    gap = math.log(C - 1) + 0.05 * torch.randperm(R0, generator=g).double()           # the dominant class holds 0.5 .. 0.95
    cls = (torch.arange(R0) * 5 + 3) % C
    ld = (C + 3) // 4 * 4
    logits = torch.zeros(R0, ld)
    logits[torch.arange(R0), cls] = gap.float()
    l = logits[:, :C].double()
    lp_all = torch.log_softmax(l, -1)
    lp = lp_all[torch.arange(R0), cls]
    srt = lp.sort().values
    assert float((srt[1:] - srt[:-1]).min()) >= 1e-3
    p = lp_all.exp()
    before = p.cumsum(-1)[torch.arange(R0), cls] - p[torch.arange(R0), cls]
    uniforms = torch.stack([before + 0.5 * lp.exp(), torch.full((R0,), 0.5, dtype=torch.float64)], -1).float()
    assert float(lp.exp().min()) > 0.1
    alphas = (0.2, 0.5, 0.9)
    for ctr, alpha in enumerate(alphas):
        d, tok, s = run_scored(logits.cuda(), C, -1, 1.0, 1.0, uniforms=uniforms.cuda(), alphas=alphas, counter=ctr + 3)
        assert torch.equal(d, cls)
        m = remask_count(alpha, HW)
        assert 0 < m < HW
        want = torch.zeros(CLIPS, HW, dtype=torch.bool)
        for b in range(CLIPS):
            want[b, lp.view(CLIPS, HW)[b].argsort()[:m]] = True
        assert torch.equal(tok, torch.where(want.view(-1), torch.full_like(d, C), d)), alpha
    # consistent masking: candidates are the rows with a non-zero byte
    cand = (torch.arange(R0) % 3 != 1)
    lm = cand.to(torch.uint8).cuda()
    d, tok, s = run_scored(logits.cuda(), C, -1, 1.0, 1.0, uniforms=uniforms.cuda(), alphas=alphas, counter=1, last_mask=lm)
    want = torch.zeros(CLIPS, HW, dtype=torch.bool)
    for b in range(CLIPS):
        rows = torch.nonzero(cand.view(CLIPS, HW)[b]).squeeze(-1)
        want[b, rows[lp.view(CLIPS, HW)[b][rows].argsort()[:remask_count(alphas[1], HW)]]] = True
    assert torch.equal(tok, torch.where(want.view(-1), torch.full_like(d, C), d))
    assert torch.equal(lm.cpu(), want.view(-1).to(torch.uint8))


# ---------------------------------------------------------------- 4. the Philox path, statistically

def test_philox_noise_masks_exactly_m_rows_and_every_row_equally_often():
    """Flat logits (every score equal before the noise), noise = 1, uniforms from the in-kernel generator, HW = 64, 3 clips, 300
    counter values at alpha = 0.5: every step masks exactly m = 32 rows per clip.  The rows of a clip are exchangeable and the
    steps independent, so a row's count is Binomial(300, 1/2): by Hoeffding's inequality P(|K / N - p| >= t) <= 2 exp(-2 N t^2),
    and t = sqrt(ln(2 * 192 / 1e-6) / (2 N)) = 0.182 keeps the union over the 192 rows under 1e-6.  The same counter gives the
    same mask, another counter another."""
    from world_modelz_amd import ops
    C, HW, clips, N = 64, 64, 3, 300
    R = HW * clips
    logits = torch.zeros(R, C, device='cuda')
    alphas = torch.tensor([0.5], device='cuda')
    z = torch.zeros(clips, 2, HW, dtype=torch.int64, device='cuda')
    den = torch.zeros(R, dtype=torch.int64, device='cuda')
    ctr = torch.zeros(1, dtype=torch.int64, device='cuda')
    freq = torch.zeros(clips, HW, dtype=torch.int64, device='cuda')
    wrong = torch.zeros((), dtype=torch.int64, device='cuda')
    firsts = []
    for step in range(N):
        ops.sample_tokens_confidence(logits, -1, alphas, C, z[:, -1], den, ctr, 77, None, noise=1.0)
        masked = z[:, -1] == C
        freq += masked
        wrong += (masked.sum(-1) != 32).sum() + ((z[:, -1] != den.view(clips, HW)) & ~masked).sum()
        if step < 2:
            firsts.append(masked.clone())
        ctr += 1
    ctr.zero_()
    ops.sample_tokens_confidence(logits, -1, alphas, C, z[:, -1], den, ctr, 77, None, noise=1.0)
    assert torch.equal(z[:, -1] == C, firsts[0]) and not torch.equal(firsts[0], firsts[1])
    assert int(wrong) == 0
    t = math.sqrt(math.log(2 * R / 1e-6) / (2 * N))
    dev = (freq.double() / N - 0.5).abs()
    print(f'[philox remask] worst |freq - 1/2| = {float(dev.max()):.4f}, bound {t:.4f}')
    assert float(dev.max()) < t


# ---------------------------------------------------------------- 5. sample_frames

C_SF, N_IT = 256, 4


def tiny_model():
    from world_modelz_amd import main
    torch.manual_seed(9)
    m = main.VqVideoDiffusionModel(data_shape=(3, 8, 8), dim=64, num_classes=C_SF, extents=(1, 1, 1), depth=1, dim_head=32, mlp_dim=128,
                                   heads=2).cuda().eval()
    z = torch.randint(0, C_SF, (2, 3, 8, 8), device='cuda')
    return m, z


def test_sample_frames_confidence_takes_the_fused_route_and_random_stays_as_it_was(monkeypatch):
    """(a) remask='confidence' runs the captured step with the two new launches and never the torch draw; (c) the final frames hold
    no mask token and only classes below C, with and without consistent_masking; reproducible from the generator's seed; (d) a
    default (remask='random') run reaches neither new entry point; (e) bad arguments are refused on the host."""
    from world_modelz_amd import config
    from world_modelz_amd.sample import sample_frames
    m, z = tiny_model()

    def no_torch_draw(*a, **k):
        raise AssertionError('the torch draw was reached')
    with config.compute_dtype(torch.bfloat16):
        monkeypatch.setattr(torch, 'multinomial', no_torch_draw)
        g = torch.Generator().manual_seed(31)
        with recorded_calls() as seen:
            sample_frames(m, z, C_SF, 2, num_eval_iterations=N_IT, sample_topk=100, generator=g)
        assert 'wmz_sample_tokens_dev' in seen
        assert 'wmz_sample_tokens_scored_dev' not in seen and 'wmz_remask_lowest_dev' not in seen
        results = {}
        for cm in (False, True):
            g.manual_seed(31)
            with recorded_calls() as seen:
                frames, zf = sample_frames(m, z, C_SF, 2, num_eval_iterations=N_IT, sample_topk=100, generator=g, consistent_masking=cm,
                                           remask='confidence', remask_noise=0.5)
            assert 'wmz_sample_tokens_scored_dev' in seen and 'wmz_remask_lowest_dev' in seen
            assert 'wmz_sample_tokens_dev' not in seen and 'wmz_sample_tokens_filtered_dev' not in seen
            assert len(frames) == 2 and all(f.shape == (2, 8, 8) and int(f.min()) >= 0 and int(f.max()) < C_SF for f in frames)
            assert int(zf.min()) >= 0 and int(zf.max()) < C_SF
            assert torch.equal(zf[:, 1], frames[1]) and torch.equal(zf[:, 2], frames[1])
            g.manual_seed(31)
            again, _ = sample_frames(m, z, C_SF, 2, num_eval_iterations=N_IT, sample_topk=100, generator=g, consistent_masking=cm,
                                     remask='confidence', remask_noise=0.5)
            assert all(torch.equal(a, b) for a, b in zip(frames, again))
            results[cm] = frames
        keys = list(m._wmz_sampler_sessions)
        assert all('confidence' in k and 0.5 in k for k in keys)           # (two sessions kept: the random one was dropped)
        monkeypatch.undo()
        for bad in (dict(remask='lowest'), dict(remask=None), dict(remask_noise=-0.1), dict(remask_noise=float('inf')),
                    dict(remask_noise=float('nan'))):
            with pytest.raises(ValueError):
                sample_frames(m, z, C_SF, 1, num_eval_iterations=N_IT, **bad)


def test_sample_frames_fused_confidence_equals_the_torch_path_when_everything_is_deterministic(monkeypatch):
    """(b) sample_topk = 1 and remask_noise = 0: draws (the argmax) and ranking are deterministic, so the fused tokens equal the torch
    path's (use_graph=False) token for token.  The schedule's first alpha is 0: a frame's first draw, from the flat start where
    top-k = 1 keeps every tied class and the draw is random, is re-masked whole.  Precondition, asserted on the torch path's own
    scores (recorded from its lowest_scores_mask calls): wherever 0 < m < HW, the gap between the m-th and (m + 1)-th lowest
    score of every clip is >= 1e-4 -- far above the difference between the two paths' fp32 scores; at the flat start every score
    is the same and m = HW.  The seed of the model and of the context is a property of this input."""
    from world_modelz_amd import config, sample
    m, z = tiny_model()
    n, HW = N_IT, 64

    def schedule(frac):
        return 0.0 if frac <= 1 / n else frac
    seen_scores = []
    real = sample.lowest_scores_mask

    def recording(scores, alpha, candidates=None):
        seen_scores.append((scores.detach().cpu().clone(), alpha))
        return real(scores, alpha, candidates)
    with config.compute_dtype(torch.bfloat16):
        monkeypatch.setattr(sample, 'lowest_scores_mask', recording)
        ref, zr = sample.sample_frames(m, z, C_SF, 2, num_eval_iterations=n, sample_topk=1, noise_schedule=schedule, use_graph=False,
                                       remask='confidence')
        monkeypatch.undo()
        assert len(seen_scores) == 2 * n
        worst = float('inf')
        for i, (s, alpha) in enumerate(seen_scores):
            mm = sample.remask_count(alpha, HW)
            if i % n == 0:
                assert mm == HW and bool((s == s[0, 0]).all())
            elif 0 < mm < HW:
                srt = s.sort(-1).values
                worst = min(worst, float((srt[:, mm] - srt[:, mm - 1]).min()))
        print(f'[sample_frames confidence] smallest gap at the selection boundary: {worst:.3e}')
        assert worst >= 1e-4
        with recorded_calls() as seen:
            got, zg = sample.sample_frames(m, z, C_SF, 2, num_eval_iterations=n, sample_topk=1, noise_schedule=schedule, remask='confidence')
        assert 'wmz_remask_lowest_dev' in seen
        assert all(torch.equal(a, b) for a, b in zip(ref, got)) and torch.equal(zr, zg)
        assert int(zg.max()) < C_SF
