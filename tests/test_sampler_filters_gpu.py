"""wmz_sample_tokens_filtered_dev -- the sampler step with a temperature, a nucleus filter and codebooks up to 16 384 classes
(include/wmz.h states its law) -- and sample_frames on top of it.

The reference law is written once, here (`Law`): the scaling in fp32 (the kernel's single multiply), masses and CDF in fp64, on
the CPU.  The kernel is held to it row by row through its two probes: injected uniforms make a call a function of its inputs, and
kept_floor makes the kept set {l >= kept_floor} observable.

eps(C) = C * 2^-23.  A sum of n positive fp32 terms taken in ANY order differs from the exact sum by at most a relative
(n - 1) u / (1 - (n - 1) u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4); C * 2^-23 = 2 C u is
that bound for the kernel's sums over a row with a factor of two in hand, which absorbs the few-ulp error of each fp32 exp
(a relative ~1e-6 per term at worst, against eps >= 1.2e-4 at the smallest C used here)."""
import functools

import pytest
import torch

from conftest import recorded_calls

pytestmark = pytest.mark.gpu

ALPHA = 0.25


def eps_of(C):
    return C * 2.0 ** -23


def scaled(logits, temperature):
    """l = logits * fp32(1 / temperature): one fp32 multiply, on the CPU."""
    return logits.float().cpu() * torch.tensor(1.0 / temperature, dtype=torch.float32)


class Law:
    """The fp64 side of the law for scaled rows l [R, C] (fp32, CPU) behind top-k: w64 = exp(l - max) over what top-k left."""

    def __init__(self, l, top_k):
        self.l = l
        C = l.shape[1]
        self.kth = torch.topk(l, top_k, dim=-1).values[:, [-1]] if 0 < top_k < C else l.min(dim=-1, keepdim=True).values
        self.w = (l.double() - l.double().max(dim=-1, keepdim=True).values).exp() * (l >= self.kth)
        self.total = self.w.sum(-1, keepdim=True)

    def mass(self, keep):
        """Share of the (top-k filtered) distribution that the classes `keep` [R, C] hold."""
        return ((self.w * keep).sum(-1, keepdim=True) / self.total).squeeze(-1)

    def target(self, top_p):
        """The distribution the draws follow, fp64 [R, C]: the nucleus by a sort (the smallest most probable set reaching top_p)."""
        w = self.w
        if top_p < 1:
            ws, _ = torch.sort(w, dim=-1, descending=True)
            j = (ws.cumsum(-1) >= top_p * self.total).double().argmax(dim=-1, keepdim=True)
            w = w * (w >= ws.gather(-1, j))
        return w / w.sum(-1, keepdim=True)


def run(logits, C, top_k, top_p, temperature, *, uniforms=None, kept_floor=True, counter=0, seed=1234, alphas=(ALPHA,), last_mask=None,
        frame=8):
    """One call of the filtered entry point on logits [R, ld >= C] (device).  denoised and kept_floor live inside sentinel frames
    that must come back intact.  -> (draws, tokens, kept_floor or None), on the CPU."""
    from world_modelz_amd import ops
    R = logits.shape[0]
    dev = logits.device
    den_buf = torch.full((R + 2 * frame,), -7, dtype=torch.int64, device=dev)
    kf_buf = torch.full((R + 2 * frame,), -123.0, dtype=torch.float32, device=dev)
    z = torch.full((1, 2, R), -5, dtype=torch.int64, device=dev)
    ops.sample_tokens(logits[:, :C], top_k, torch.tensor(alphas, dtype=torch.float32, device=dev), C, z[:, -1], den_buf[frame:frame + R],
                      torch.tensor([counter], dtype=torch.int64, device=dev), seed, last_mask, top_p=top_p, temperature=temperature,
                      uniforms=uniforms, kept_floor=kf_buf[frame:frame + R] if kept_floor else None)
    torch.cuda.synchronize()
    for buf, s in ((den_buf, -7), (kf_buf, -123.0)):
        assert bool((buf[:frame] == s).all()) and bool((buf[frame + R:] == s).all()), 'wrote outside its rows'
    assert bool((z[:, 0] == -5).all())
    return den_buf[frame:frame + R].cpu(), z[0, -1].cpu(), (kf_buf[frame:frame + R].cpu() if kept_floor else None)


# ---------------------------------------------------------------- 1. wide codebooks run at all

@pytest.mark.parametrize('C,ld', [(2052, 2056), (5003, 5004), (8192, 8196), (16384, 16388)])
def test_wide_codebooks_draw_the_dominant_class_and_never_read_padding(C, ld):
    """More than 2048 classes (the workgroup-per-row kernel): 67 rows -- no multiple of anything -- each with one logit of 60 at
    its own column (first and last class included) must draw that class whatever the filters are; the columns between C and ld
    hold 1e30, so a kernel that took padding for a class would draw it."""
    torch.manual_seed(C)
    R = 67
    logits = torch.randn(R, ld)
    logits[:, C:] = 1e30
    want = (torch.arange(R) * 977 + 5) % C
    want[0], want[1] = 0, C - 1
    logits[torch.arange(R), want] = 60.0
    dev = logits.cuda()
    with recorded_calls() as seen:
        for top_k, top_p, T in ((-1, 1.0, 1.0), (50, 0.9, 0.7)):
            d, tok, kf = run(dev, C, top_k, top_p, T, alphas=(1.0,))
            assert torch.equal(d, want), (top_k, top_p, T)
            assert torch.equal(tok, want)                                  # alpha = 1: nothing re-masked
            assert bool((kf <= scaled(logits[:, :C], T).max(-1).values).all()) and bool((kf > -1e29).all())
    assert seen == ['wmz_sample_tokens_filtered_dev'] * 2


def test_more_classes_than_the_limit_are_refused():
    from world_modelz_amd import _lib, ops
    C = ops.sample_max_classes() + 1
    assert C == 16385
    logits = torch.zeros(4, C + 3, device='cuda')
    with pytest.raises(_lib.WmzError, match=rf'code {_lib.CONSTANTS["WMZ_ERR_UNSUPPORTED"]}\b.*16384'):
        run(logits, C, -1, 1.0, 1.0)


# ---------------------------------------------------------------- 2. the exact law on injected uniforms

LAW_R = 1024


@functools.lru_cache(maxsize=None)
def law_inputs(C):
    g = torch.Generator().manual_seed(1000 + C)
    logits = torch.randn(LAW_R, C, generator=g) * 3
    uniforms = torch.rand(LAW_R, 2, generator=g)
    return logits, uniforms, logits.cuda(), uniforms.cuda()


@pytest.mark.parametrize('top_k,top_p,temperature', [(-1, 1, 1), (50, 1, 1), (-1, 0.9, 1), (200, 0.8, 0.7), (-1, 1, 1.5), (-1, 1e-6, 1)])
@pytest.mark.parametrize('C', [1000, 2052, 8192])
def test_every_row_follows_the_law(C, top_k, top_p, temperature):
    """1024 independent rows (randn * 3) in both forms of the kernel, uniforms injected, kept_floor requested.  With t =
    kept_floor[row] and eps = C * 2^-23 (module docstring), for EVERY row:
      * top-k only: #{l >= t} >= k and #{l > t} < k, exactly; no filter at all: t is the row's minimum;
      * nucleus, over the top-k filtered distribution: mass64{l >= t} >= top_p - eps and mass64{l > t} < top_p + eps;
      * the draw d has l[d] >= t, and u0 * tot lies in [CDF64[d - 1] - eps tot, CDF64[d] + eps tot], the CDF over exactly
        {l >= t} in class order;
      * tokens == where(u1 > alpha, mask_token, d) and denoised == d, exactly;
      * top_p = 1e-6 draws the argmax."""
    logits, uniforms, logits_dev, uniforms_dev = law_inputs(C)
    d, tok, t = run(logits_dev, C, top_k, top_p, temperature, uniforms=uniforms_dev)
    l = scaled(logits, temperature)
    law = Law(l, top_k)
    eps = eps_of(C)
    t = t.unsqueeze(-1)
    ge, gt = l >= t, l > t
    rows = torch.arange(LAW_R)
    assert int(d.min()) >= 0 and int(d.max()) < C
    if top_p >= 1:
        if 0 < top_k < C:
            n_ge, n_gt = ge.sum(-1), gt.sum(-1)
            print(f'[law C={C} k={top_k}] #(l >= t) in [{int(n_ge.min())}, {int(n_ge.max())}], #(l > t) max {int(n_gt.max())}')
            assert bool((n_ge >= top_k).all()) and bool((n_gt < top_k).all())
        else:
            assert torch.equal(t.squeeze(-1), l.min(-1).values)
    else:
        m_ge, m_gt = law.mass(ge), law.mass(gt)
        print(f'[law C={C} k={top_k} p={top_p} T={temperature}] min mass(l >= t) - p = {float((m_ge - top_p).min()):.3e}, '
              f'max mass(l > t) - p = {float((m_gt - top_p).max()):.3e}, eps = {eps:.3e}')
        assert bool((t >= law.kth).all())                                  # the nucleus lies inside the top-k set
        assert bool((m_ge >= top_p - eps).all()) and bool((m_gt < top_p + eps).all())
    assert bool(ge[rows, d].all())                                         # the draw is a kept class
    cdf = (law.w * ge).cumsum(-1)
    tot = cdf[:, -1]
    x = uniforms[:, 0].double() * tot
    hi = cdf[rows, d]
    lo = torch.where(d > 0, cdf[rows, (d - 1).clamp(min=0)], torch.zeros_like(hi))
    print(f'[law C={C} k={top_k} p={top_p} T={temperature}] u0 tot outside [CDF[d-1], CDF[d]] by at most '
          f'{float((torch.maximum(lo - x, x - hi) / tot).max()):.3e} tot (negative: inside; eps = {eps:.3e})')
    assert bool((x >= lo - eps * tot).all()) and bool((x <= hi + eps * tot).all())
    assert torch.equal(tok, torch.where(uniforms[:, 1] > ALPHA, torch.full_like(d, C), d))
    if top_p == 1e-6:
        assert torch.equal(d, l.argmax(-1))


# ---------------------------------------------------------------- 3. neutral arguments are the old kernel

@pytest.mark.parametrize('top_k', [-1, 10])
@pytest.mark.parametrize('C', [37, 700, 1024, 2000])
def test_neutral_arguments_are_the_old_kernel(C, top_k):
    """top_p = 1, inv_temperature = 1, no uniforms, no probe: the new entry point returns the draws, tokens and mask bytes of
    wmz_sample_tokens_dev for the same seed and counter."""
    from world_modelz_amd import _lib as L
    torch.manual_seed(C + top_k)
    R, ld = 333, (C + 3) // 4 * 4
    logits = torch.randn(R, ld, device='cuda') * 2
    alphas = torch.tensor([0.3, 0.7], device='cuda')
    ctr = torch.tensor([5], dtype=torch.int64, device='cuda')
    out = []
    for name, extra_a, extra_b in (('wmz_sample_tokens_dev', (), ()), ('wmz_sample_tokens_filtered_dev', (1.0, 1.0), (None, None))):
        for with_mask in (False, True):
            z = torch.zeros(3, 2, R // 3, dtype=torch.int64, device='cuda')
            den = torch.zeros(R, dtype=torch.int64, device='cuda')
            lm = (torch.arange(R, device='cuda') % 3 != 0).to(torch.uint8) if with_mask else None
            L.call(name, L.ptr(logits), ld, R, C, top_k, *extra_a, L.ptr(alphas), 2, C, L.ptr(z[:, -1]), R // 3, z.stride(0), L.ptr(den),
                   L.ptr(lm), *extra_b, 99, L.ptr(ctr), L.stream())
            torch.cuda.synchronize()
            out.append((den.cpu(), z.cpu(), None if lm is None else lm.cpu()))
    for old, new in zip(out[:2], out[2:]):
        assert torch.equal(old[0], new[0]) and torch.equal(old[1], new[1])
        assert old[2] is None or torch.equal(old[2], new[2])
    assert not torch.equal(out[0][1], out[1][1])                           # (the mask bytes do act)


# ---------------------------------------------------------------- 4. the Philox path, statistically

@pytest.mark.parametrize('C,top_k,top_p,temperature', [(4096, -1, 0.9, 1.0), (8192, 200, 0.8, 0.7)])
def test_philox_draws_follow_the_filtered_distribution(C, top_k, top_p, temperature):
    """16 384 rows sharing one row of logits, uniforms from the in-kernel generator: no draw outside {l >= kept_floor}, and the
    total variation between the draw frequencies and the fp64 target stays under 1.25 x the largest total variation that twenty
    draws of 16 384 samples by torch.multinomial from that target (CPU, fixed seed) show -- the bound is the reference sampler's
    own noise, not the kernel's.  Another counter: other draws, another alpha; the same counter: the same draws."""
    R = 16384
    g = torch.Generator().manual_seed(C)
    row = torch.randn(C, generator=g) * 2.0
    logits = row.cuda().expand(R, C).contiguous()
    l = scaled(row.unsqueeze(0), temperature)
    target = Law(l, top_k).target(top_p)[0]

    def tv(draws):
        return 0.5 * float((torch.bincount(draws, minlength=C).double() / R - target).abs().sum())
    ref = [tv(torch.multinomial(target, R, True, generator=g)) for _ in range(20)]
    bound = 1.25 * max(ref)
    d, tok, kf = run(logits, C, top_k, top_p, temperature, counter=0, alphas=(0.25, 0.6))
    assert bool((kf == kf[0]).all())
    assert bool((l[0][d] >= kf[0]).all())                                  # never outside the kept set
    got = tv(d)
    print(f'[philox C={C} k={top_k} p={top_p} T={temperature}] TV {got:.4f}; reference sampler {min(ref):.4f} .. {max(ref):.4f}, '
          f'bound {bound:.4f}; support {int((target > 0).sum())} classes')
    assert got < bound
    assert abs(float((tok == C).float().mean()) - 0.75) < 0.02 and torch.equal(tok[tok != C], d[tok != C])
    d1, tok1, _ = run(logits, C, top_k, top_p, temperature, counter=1, alphas=(0.25, 0.6))
    assert not torch.equal(d, d1) and abs(float((tok1 == C).float().mean()) - 0.4) < 0.02 and tv(d1) < bound
    d0, tok0, _ = run(logits, C, top_k, top_p, temperature, counter=0, alphas=(0.25, 0.6), kept_floor=False)
    assert torch.equal(d, d0) and torch.equal(tok, tok0)


# ---------------------------------------------------------------- 5. sample_frames end to end

def test_sample_frames_takes_the_fused_route_for_a_wide_codebook(monkeypatch):
    """4096 codes: the default call runs the captured step with wmz_sample_tokens_filtered_dev and never the torch draw; valid
    codes, reproducible from the generator's seed; temperature / sample_topp change the frames and get a session of their own;
    the torch path (injected uniforms) takes them too; bad values are refused on the host."""
    from world_modelz_amd import config, main
    from world_modelz_amd.sample import sample_frames
    torch.manual_seed(9)
    C, n = 4096, 4
    m = main.VqVideoDiffusionModel(data_shape=(3, 8, 8), dim=64, num_classes=C, extents=(1, 1, 1), depth=1, dim_head=32, mlp_dim=128,
                                   heads=2).cuda().eval()
    z = torch.randint(0, C, (2, 3, 8, 8), device='cuda')
    real_multinomial = torch.multinomial

    def no_torch_draw(*a, **k):
        raise AssertionError('the torch draw was reached')
    with config.compute_dtype(torch.bfloat16):
        monkeypatch.setattr(torch, 'multinomial', no_torch_draw)
        g = torch.Generator().manual_seed(31)
        with recorded_calls() as seen:
            frames, zf = sample_frames(m, z, C, 2, num_eval_iterations=n, sample_topk=100, generator=g)
        assert 'wmz_sample_tokens_filtered_dev' in seen and 'wmz_sample_tokens_dev' not in seen
        assert len(frames) == 2 and all(f.shape == (2, 8, 8) and int(f.min()) >= 0 and int(f.max()) < C for f in frames)
        assert torch.equal(zf[:, 0], frames[0]) and torch.equal(zf[:, 1], frames[1]) and torch.equal(zf[:, 2], frames[1])    # shifted twice
        g.manual_seed(31)
        again, _ = sample_frames(m, z, C, 2, num_eval_iterations=n, sample_topk=100, generator=g)
        assert all(torch.equal(a, b) for a, b in zip(frames, again))
        assert len(m._wmz_sampler_sessions) == 1
        g.manual_seed(31)
        with recorded_calls() as seen:
            other, _ = sample_frames(m, z, C, 2, num_eval_iterations=n, sample_topk=100, generator=g, temperature=0.7, sample_topp=0.9)
        assert 'wmz_sample_tokens_filtered_dev' in seen
        assert all(int(f.min()) >= 0 and int(f.max()) < C for f in other)
        assert not all(torch.equal(a, b) for a, b in zip(frames, other))
        assert len(m._wmz_sampler_sessions) == 2 and len({k[-2:] for k in m._wmz_sampler_sessions}) == 2
        monkeypatch.setattr(torch, 'multinomial', real_multinomial)
        gu = torch.Generator().manual_seed(2)
        uniforms = (torch.rand(1, n, 2 * 64, generator=gu), torch.rand(1, n, 2, 64, generator=gu))
        a, _ = sample_frames(m, z, C, 1, num_eval_iterations=n, sample_topk=100, uniforms=uniforms, temperature=0.7, sample_topp=0.9)
        b, _ = sample_frames(m, z, C, 1, num_eval_iterations=n, sample_topk=100, uniforms=uniforms, temperature=0.7, sample_topp=0.9)
        assert torch.equal(a[0], b[0]) and int(a[0].min()) >= 0 and int(a[0].max()) < C
        for bad in (dict(temperature=0), dict(temperature=-1.0), dict(sample_topp=0), dict(sample_topp=1.5)):
            with pytest.raises(ValueError):
                sample_frames(m, z, C, 1, num_eval_iterations=n, **bad)
