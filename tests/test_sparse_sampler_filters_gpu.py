"""Config 5's sampler with a temperature, top-k, a nucleus filter and prompted clips: wmz_categorical_scatter_filtered and
wmz_sparse_draw_context_known (include/wmz.h states their laws), sparse_diffusion.categorical_scatter / sample_clips on top of them.

The reference law is written once, here (`Law`, restated from tests/test_sampler_filters_gpu.py: the dense sampler's kernels follow
the same law): the scaling in fp32 (the kernel's single multiply), masses and CDF in fp64, on the CPU.  The kernel is held to it row
by row through its two probes: injected uniforms (one per row) make a call a function of its inputs, and kept_floor makes the
kept set {l >= kept_floor} observable.

eps(C) = C * 2^-23.  A sum of n positive fp32 terms taken in ANY order differs from the exact sum by at most a relative
(n - 1) u / (1 - (n - 1) u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4); C * 2^-23 = 2 C u is
that bound for the kernel's sums over a row with a factor of two in hand, which absorbs the few-ulp error of each fp32 exp."""
import functools

import pytest
import torch

from conftest import recorded_calls

pytestmark = pytest.mark.gpu

SENTINEL = -5


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


def scatter(logits, C, top_k=-1, top_p=1.0, temperature=1.0, *, indices=None, z=None, rows_per_clip=1, known=None, uniforms=None,
            kept_floor=False, samples=True, seed=1234, stream_id=3 << 40, counter=None, name='wmz_categorical_scatter_filtered', frame=8):
    """One call of a raw entry point on logits [R, ld >= C] (device).  samples and kept_floor live inside sentinel frames that must
    come back intact.  -> (samples or None, kept_floor or None), on the CPU; z is written in place."""
    from world_modelz_amd import _lib as L
    R, ld = logits.shape[0], logits.stride(0)
    dev = logits.device
    s_buf = torch.full((R + 2 * frame,), -7, dtype=torch.int64, device=dev)
    kf_buf = torch.full((R + 2 * frame,), -123.0, dtype=torch.float32, device=dev)
    dest = (L.ptr(indices), L.ptr(z), z.stride(0) if z is not None else 0, rows_per_clip, L.ptr(s_buf[frame:]) if samples else None)
    tail = (seed, stream_id, L.ptr(counter), L.stream())
    if name == 'wmz_categorical_scatter':
        L.call(name, L.ptr(logits), ld, R, C, *dest, *tail)
    else:
        L.call(name, L.ptr(logits), ld, R, C, top_k, float(top_p), 1.0 / float(temperature), *dest, L.ptr(known),
               known.stride(0) if known is not None else 0, L.ptr(uniforms), L.ptr(kf_buf[frame:]) if kept_floor else None, *tail)
    torch.cuda.synchronize()
    for buf, s, used in ((s_buf, -7, samples), (kf_buf, -123.0, kept_floor)):
        assert bool((buf[:frame] == s).all()) and bool((buf[frame + R:] == s).all()), 'wrote outside its rows'
        assert used or bool((buf == s).all())
    return (s_buf[frame:frame + R].cpu() if samples else None), (kf_buf[frame:frame + R].cpu() if kept_floor else None)


def clip_positions(R, rows_per_clip, G, seed):
    """indices [R]: per clip of rows_per_clip rows distinct positions of a grid of G; and an all-sentinel z [clips, G]."""
    g = torch.Generator().manual_seed(seed)
    clips = -(-R // rows_per_clip)
    idx = torch.cat([torch.randperm(G, generator=g)[:rows_per_clip] for _ in range(clips)])[:R].contiguous()
    return idx, torch.full((clips, G), SENTINEL, dtype=torch.int64)


# ---------------------------------------------------------------- 1. the exact law on injected uniforms

LAW_R, LAW_RPC, LAW_G = 257, 64, 100


@functools.lru_cache(maxsize=None)
def law_inputs(C):
    g = torch.Generator().manual_seed(2000 + C)
    ld = (C + 3) // 4 * 4 + 4
    logits = torch.full((LAW_R, ld), 1e30)
    logits[:, :C] = torch.randn(LAW_R, C, generator=g) * 3
    uniforms = torch.rand(LAW_R, generator=g)
    idx, z = clip_positions(LAW_R, LAW_RPC, LAW_G, C)
    return logits[:, :C].contiguous(), uniforms, idx, logits.cuda(), uniforms.cuda(), idx.cuda()


@pytest.mark.parametrize('setting', [('k', 1, 1), (-1, 0.9, 1), ('k200', 0.8, 0.7), (-1, 1, 1.5), (-1, 1e-6, 1)], ids=str)
@pytest.mark.parametrize('C', [24, 1000, 2052, 8192])
def test_every_row_follows_the_law(C, setting):
    """257 independent rows (randn * 3, the columns between C and ld at 1e30) in both forms of the kernel, uniforms injected,
    kept_floor requested, five clips of up to 64 rows scattered into a sentinel-filled z.  With t = kept_floor[row] and
    eps = C * 2^-23 (module docstring), for EVERY row:
      * top-k only: #{l >= t} >= k and #{l > t} < k, exactly; no filter at all: t is the row's minimum;
      * nucleus, over the top-k filtered distribution: mass64{l >= t} >= top_p - eps and mass64{l > t} < top_p + eps;
      * the draw d has l[d] >= t, and u0 * tot lies in [CDF64[d - 1] - eps tot, CDF64[d] + eps tot], the CDF over exactly
        {l >= t} in class order;
      * top_p = 1e-6 draws the argmax;
      * z holds d at indices[row] of the row's clip and the sentinel everywhere else; samples == d; no frame is touched."""
    top_k, top_p, temperature = setting
    top_k = {'k': 5 if C == 24 else 50, 'k200': min(200, C - 1)}.get(top_k, top_k)
    logits, uniforms, idx, logits_dev, uniforms_dev, idx_dev = law_inputs(C)
    z = torch.full((-(-LAW_R // LAW_RPC), LAW_G), SENTINEL, dtype=torch.int64, device='cuda')
    d, t = scatter(logits_dev, C, top_k, top_p, temperature, indices=idx_dev, z=z, rows_per_clip=LAW_RPC, uniforms=uniforms_dev,
                   kept_floor=True)
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
    x = uniforms.double() * tot
    hi = cdf[rows, d]
    lo = torch.where(d > 0, cdf[rows, (d - 1).clamp(min=0)], torch.zeros_like(hi))
    print(f'[law C={C} k={top_k} p={top_p} T={temperature}] u0 tot outside [CDF[d-1], CDF[d]] by at most '
          f'{float((torch.maximum(lo - x, x - hi) / tot).max()):.3e} tot (negative: inside; eps = {eps:.3e})')
    assert bool((x >= lo - eps * tot).all()) and bool((x <= hi + eps * tot).all())
    if top_p == 1e-6:
        assert torch.equal(d, l.argmax(-1))
    want = torch.full((z.shape[0], LAW_G), SENTINEL, dtype=torch.int64)
    want[rows // LAW_RPC, idx] = d
    assert torch.equal(z.cpu(), want)


# ---------------------------------------------------------------- 2. neutral arguments are the old kernel

@pytest.mark.parametrize('C,ld', [(12, 13), (8192, 8192)])
def test_neutral_arguments_are_the_old_kernel(C, ld):
    """top_k = -1 or >= C, top_p = 1, inv_temperature = 1, no uniforms, no probe -- rows off the 16-byte granule included: the new
    entry point gives the z and the samples of wmz_categorical_scatter for the same seed, stream id and device counter; another
    counter value gives other draws."""
    torch.manual_seed(C)
    R, rpc, G = 333, 111, 200
    logits = (torch.randn(R, ld, device='cuda') * 2)[:, :C]
    idx, z0 = clip_positions(R, rpc, G, C)
    idx = idx.cuda()
    ctr = torch.tensor([5], dtype=torch.int64, device='cuda')
    out = {}
    for key, name, top_k in (('old', 'wmz_categorical_scatter', -1), ('new', 'wmz_categorical_scatter_filtered', -1),
                             ('new_k', 'wmz_categorical_scatter_filtered', C), ('new_k+', 'wmz_categorical_scatter_filtered', C + 7)):
        z = z0.cuda()
        s, _ = scatter(logits, C, top_k, indices=idx, z=z, rows_per_clip=rpc, counter=ctr, name=name)
        out[key] = (z.cpu(), s)
    for key in ('new', 'new_k', 'new_k+'):
        assert torch.equal(out['old'][0], out[key][0]) and torch.equal(out['old'][1], out[key][1]), key
    assert int(out['old'][1].min()) >= 0 and int(out['old'][1].max()) < C
    assert torch.equal(out['old'][0][torch.arange(R) // rpc, idx.cpu()], out['old'][1])
    ctr.fill_(6)
    z = z0.cuda()
    s, _ = scatter(logits, C, -1, indices=idx, z=z, rows_per_clip=rpc, counter=ctr)
    assert not torch.equal(s, out['old'][1])


# ---------------------------------------------------------------- 3. known positions

@pytest.mark.parametrize('C,top_k,top_p,temperature', [(1000, 50, 0.9, 0.7), (4096, 100, 1.0, 1.0), (1000, -1, 1.0, 1.0), (13, -1, 1.0, 1.0)])
def test_known_positions_keep_their_tokens(C, top_k, top_p, temperature):
    """A random field of known bytes over z: with filters acting (both forms) and neutral (aligned and not), z keeps its sentinel
    at every known position and holds the draw at the others; samples are those of the call without `known`."""
    torch.manual_seed(C + top_k)
    R, rpc, G = 300, 100, 160
    ld = C if C % 4 == 0 or top_k > 0 else C + 1
    logits = (torch.randn(R, ld, device='cuda') * 2)[:, :C]
    idx, z0 = clip_positions(R, rpc, G, C)
    known = (torch.rand(3, G + 5) < 0.4).to(torch.uint8).cuda()[:, :G]            # (a stride of its own)
    za, zb = z0.cuda(), z0.cuda()
    sa, _ = scatter(logits, C, top_k, top_p, temperature, indices=idx.cuda(), z=za, rows_per_clip=rpc)
    sb, _ = scatter(logits, C, top_k, top_p, temperature, indices=idx.cuda(), z=zb, rows_per_clip=rpc, known=known)
    assert torch.equal(sa, sb)
    clip = torch.arange(R) // rpc
    kn = known.cpu()[clip, idx].bool()
    assert 0 < int(kn.sum()) < R
    want = z0.clone()
    want[clip[~kn], idx[~kn]] = sa[~kn]
    assert torch.equal(zb.cpu(), want)
    assert torch.equal(za.cpu()[clip, idx], sa)


def test_context_draw_leaves_known_slots_as_they_are():
    """wmz_sparse_draw_context_known on an 8 x 4 x 4 grid, n = 32: indices and target are the old entry point's for the same seed,
    stream and counter; tokens are the old entry point's where the position is unknown and the target where it is known; at r = 1
    every unknown slot is the mask token and no known slot is."""
    from world_modelz_amd.train import draw_sparse_context
    torch.manual_seed(0)
    B, S, H, W, C, n = 3, 8, 4, 4, 24, 32
    z = torch.randint(0, C, (B, S, H, W), device='cuda')
    known = (torch.rand(B, S * H * W, device='cuda') < 0.5)
    ctr = torch.tensor([9], dtype=torch.int64, device='cuda')
    for r, p_uniform in ((torch.tensor([0.3, 0.6, 0.9], device='cuda'), 0.1), (torch.ones(B, device='cuda'), 0.0)):
        with recorded_calls() as seen:
            old = draw_sparse_context(z, r, n, (S, H, W), C, seed=77, rank=1, counter=ctr, p_uniform=p_uniform)
            new = draw_sparse_context(z, r, n, (S, H, W), C, seed=77, rank=1, counter=ctr, p_uniform=p_uniform, known=known)
        assert seen == ['wmz_sparse_draw_context', 'wmz_sparse_draw_context_known']
        assert torch.equal(old[0], new[0]) and torch.equal(old[2], new[2])
        kn = torch.gather(known, 1, new[0])
        assert 0 < int(kn.sum()) < kn.numel()
        assert torch.equal(new[1][~kn], old[1][~kn]) and torch.equal(new[1][kn], new[2][kn])
        assert not torch.equal(old[1], old[2])                                 # (the corruption does act)
        if p_uniform == 0.0:
            assert bool((new[1][~kn] == C).all()) and bool((new[1][kn] < C).all())


# ---------------------------------------------------------------- 4. refusal and fallback

def test_more_classes_than_the_limit():
    """A filter acting on 16 385 classes: the raw entry point refuses (WMZ_ERR_UNSUPPORTED) and writes nothing; categorical_scatter
    filters with torch ops and draws through the neutral form of the new entry point -- top_k = 1 gives each row's argmax."""
    from world_modelz_amd import _lib, ops
    from world_modelz_amd.sparse_diffusion import categorical_scatter
    C = ops.sample_max_classes() + 1
    assert C == 16385
    torch.manual_seed(1)
    logits = torch.randn(1, 8, C, device='cuda')
    idx = torch.randperm(20, device='cuda')[:8].reshape(1, 8).contiguous()
    z = torch.full((1, 20), SENTINEL, dtype=torch.int64, device='cuda')
    with pytest.raises(_lib.WmzError, match=rf'code {_lib.CONSTANTS["WMZ_ERR_UNSUPPORTED"]}\b.*16384'):
        scatter(logits[0], C, 1, indices=idx, z=z, rows_per_clip=8)
    torch.cuda.synchronize()
    assert bool((z == SENTINEL).all())
    with recorded_calls() as seen:
        categorical_scatter(logits, idx, z, seed=3, call_id=1, top_k=1)
    assert seen == ['wmz_categorical_scatter_filtered']
    assert torch.equal(torch.gather(z, 1, idx), logits.argmax(-1))
    assert int((z == SENTINEL).sum()) == 12


def test_the_widest_codebook_draws_the_dominant_class():
    """16 384 classes, the limit (69.7 KB of LDS: the instantiation's own dynamic-LDS attribute): 67 rows, each with one logit of 60
    at its own column (first and last class included), draw that class under top-k 50, top-p 0.9, temperature 0.7; the columns
    between C and ld hold 1e30."""
    from world_modelz_amd import ops
    C = ops.sample_max_classes()
    R = 67
    torch.manual_seed(C)
    logits = torch.randn(R, C + 4)
    logits[:, C:] = 1e30
    want = (torch.arange(R) * 977 + 5) % C
    want[0], want[1] = 0, C - 1
    logits[torch.arange(R), want] = 60.0
    d, kf = scatter(logits.cuda(), C, 50, 0.9, 0.7, kept_floor=True)
    assert torch.equal(d, want)
    assert bool((kf <= scaled(logits[:, :C], 0.7).max(-1).values).all()) and bool((kf > -1e29).all())


# ---------------------------------------------------------------- 5. the Philox path, statistically

@pytest.mark.parametrize('C,top_k,top_p,temperature', [(4096, -1, 0.9, 1.0), (300, 40, 0.8, 0.7)])
def test_philox_draws_follow_the_filtered_distribution(C, top_k, top_p, temperature):
    """16 384 rows sharing one row of logits, uniforms from the in-kernel generator: no draw outside {l >= kept_floor}, and the
    total variation between the draw frequencies and the fp64 target stays under 1.25 x the largest total variation that twenty
    draws of 16 384 samples by torch.multinomial from that target (CPU, fixed seed) show -- the bound is the reference sampler's
    own noise, not the kernel's.  Another counter: other draws; the same counter: the same draws."""
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
    ctr = torch.tensor([0], dtype=torch.int64, device='cuda')
    d, kf = scatter(logits, C, top_k, top_p, temperature, counter=ctr, kept_floor=True)
    assert bool((kf == kf[0]).all())
    assert bool((l[0][d] >= kf[0]).all())                                  # never outside the kept set
    got = tv(d)
    print(f'[philox C={C} k={top_k} p={top_p} T={temperature}] TV {got:.4f}; reference sampler {min(ref):.4f} .. {max(ref):.4f}, '
          f'bound {bound:.4f}; support {int((target > 0).sum())} classes')
    assert got < bound
    ctr.fill_(1)
    d1, _ = scatter(logits, C, top_k, top_p, temperature, counter=ctr)
    assert not torch.equal(d, d1) and tv(d1) < bound
    ctr.fill_(0)
    d0, _ = scatter(logits, C, top_k, top_p, temperature, counter=ctr)
    assert torch.equal(d, d0)


# ---------------------------------------------------------------- 6. sample_clips end to end, stand-in model

S_, H_, W_, C_, N_ = 8, 4, 4, 24, 32
G_ = S_ * H_ * W_


class Stub(torch.nn.Module):
    """logits = 2 * one_hot(position mod C) + fixed noise of amplitude 0.9: the position's own class is every row's argmax, with
    a probability of about a quarter under the plain softmax.  Counts, on the device, the mask tokens it was fed at given
    positions (`given`: bool [B, G], or None)."""

    def __init__(self, given=None):
        super().__init__()
        self.shape = (S_, H_, W_)
        self.embedding = torch.nn.Embedding(C_ + 1, 8)
        self.register_buffer('noise', 0.9 * (2 * torch.rand(G_, C_, generator=torch.Generator().manual_seed(5)) - 1))
        self.register_buffer('masked_given', torch.zeros((), dtype=torch.int64))
        self.given = given

    def forward(self, tokens, indices):
        if self.given is not None:
            self.masked_given += ((tokens == C_) & torch.gather(self.given, 1, indices)).sum()
        own = torch.arange(C_, device=indices.device) == (indices % C_).unsqueeze(-1)       # (no one_hot: it reads back)
        return 2.0 * own.float() + self.noise[indices]


def test_sample_clips_top_k_one_draws_every_argmax():
    """sample_topk = 1: every visited position holds position mod C exactly (captured and eager); without it some do not."""
    from world_modelz_amd.sparse_diffusion import sample_clips
    stub = Stub().cuda()
    own = (torch.arange(G_, device='cuda') % C_).expand(3, -1)
    for use_graph in (True, False):
        z = sample_clips(stub, 3, C_, 'neighbors', num_context=N_, num_eval_iterations=5, generator=torch.Generator().manual_seed(3), seed=11,
                         use_graph=use_graph, sample_topk=1).view(3, -1)
        visited = z != C_
        assert float(visited.float().mean()) > 0.9 and bool((z[visited] == own[visited]).all())
    z = sample_clips(stub, 3, C_, 'neighbors', num_context=N_, num_eval_iterations=5, generator=torch.Generator().manual_seed(3), seed=11).view(3, -1)
    visited = z != C_
    assert float(visited.float().mean()) > 0.9 and int(z[visited].max()) < C_
    assert float((z[visited] != own[visited]).float().mean()) > 0.25


@pytest.mark.parametrize('route', ['captured', 'eager', 'torch-drawn', 'uniform'])
def test_sample_clips_completes_a_prompt(route, monkeypatch):
    """Frames 0-3 given as (position + 1) mod C, frames 4-7 to be generated, sample_topk = 1, on each of the four routes: the result
    is the prompt at every given position, position mod C at the generated positions that were visited (most of them), and the
    model never saw a mask token at a given position."""
    from world_modelz_amd import _lib as L
    from world_modelz_amd.sparse_diffusion import sample_clips
    B = 2
    pos = torch.arange(G_, device='cuda')
    prompt = torch.full((B, G_), C_, dtype=torch.int64, device='cuda')
    prompt[:, :G_ // 2] = (pos[:G_ // 2] + 1) % C_
    given = prompt != C_
    stub = Stub(given).cuda()
    if route == 'torch-drawn':
        monkeypatch.setattr(L.lib(), 'wmz_sparse_draw_context_supported', lambda *a: 0)
    with recorded_calls() as seen:
        z = sample_clips(stub, B, C_, 'uniform' if route == 'uniform' else 'neighbors', num_context=N_, num_eval_iterations=5,
                         generator=torch.Generator().manual_seed(3), seed=11, use_graph=route == 'captured', sample_topk=1,
                         prompt=prompt.view(B, S_, H_, W_)).view(B, -1)
    assert 'wmz_categorical_scatter_filtered' in seen and 'wmz_categorical_scatter' not in seen
    assert ('wmz_sparse_draw_context_known' in seen) == (route in ('captured', 'eager')) and 'wmz_sparse_draw_context' not in seen
    assert torch.equal(z[given], prompt[given])
    gen = z[:, G_ // 2:]
    visited = gen != C_
    assert float(visited.float().mean()) > 0.8 and bool((gen[visited] == (pos[G_ // 2:] % C_).expand(B, -1)[visited]).all())
    assert int(stub.masked_given) == 0
    assert bool((prompt.view(B, -1)[:, G_ // 2:] == C_).all())                 # (the caller's prompt is not written)


# ---------------------------------------------------------------- 7. a real small model

def test_real_model_captured_and_eager_agree_with_filters_and_a_prompt():
    """dim 64, depth 2, bf16: with sample_topk = 5, sample_topp = 0.9, temperature = 0.8 and a prompt the captured sub-step and the
    eager launches give the same clip through the filtered entry points; a default call reaches only the entry points it always
    reached."""
    from world_modelz_amd import config
    from world_modelz_amd.sparse_diffusion import VqSparseDiffusionModel, sample_clips
    torch.manual_seed(4)
    B = 2
    m = VqSparseDiffusionModel(shape=(S_, H_, W_), dim=64, num_classes=C_, depth=2, dim_head=32, mlp_dim=96, heads=2).cuda()
    prompt = torch.full((B, S_, H_, W_), C_, dtype=torch.int64, device='cuda')
    prompt[:, :3] = torch.randint(0, C_, (B, 3, H_, W_), device='cuda')
    prompt[:, 6, 1] = 7
    given = prompt != C_
    sparse = ('wmz_sparse_draw_context', 'wmz_sparse_draw_context_known', 'wmz_categorical_scatter', 'wmz_categorical_scatter_filtered')
    with config.compute_dtype(torch.bfloat16):
        out = []
        for use_graph in (True, False):
            with recorded_calls() as seen:
                out.append(sample_clips(m, B, C_, 'neighbors', num_context=N_, num_eval_iterations=3, seed=5,
                                        generator=torch.Generator().manual_seed(1), use_graph=use_graph, sample_topk=5, sample_topp=0.9,
                                        temperature=0.8, prompt=prompt))
            assert {s for s in seen if s in sparse} == {'wmz_sparse_draw_context_known', 'wmz_categorical_scatter_filtered'}
        assert torch.equal(out[0], out[1])
        assert torch.equal(out[0][given], prompt[given]) and int(out[0].min()) >= 0 and int(out[0].max()) <= C_
        with recorded_calls() as seen:
            zd = sample_clips(m, B, C_, 'neighbors', num_context=N_, num_eval_iterations=3, seed=5, generator=torch.Generator().manual_seed(1))
        assert {s for s in seen if s in sparse} == {'wmz_sparse_draw_context', 'wmz_categorical_scatter'}
        assert int(zd.min()) >= 0 and int(zd.max()) <= C_
