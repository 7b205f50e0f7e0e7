"""tests/tail_bounds.py without a GPU: an fp32 torch emulation of each correct kernel passes every bound with no element left
out, at the shapes tests/test_train_tail_gpu.py runs; seeded mistakes -- the ones a stride, a tail or an operation order makes --
fail, each by itself, with the offending element named; the numpy Philox equals the header's word for word, and the corruption
reference has the frequencies of the reference law."""
import re

import numpy as np
import pytest
import torch

import tail_bounds as tb
from test_philox_cpu import BLOCKS, CXX, host  # noqa: F401  (the compiled csrc/wmz_philox.h)

F32, BF16 = torch.float32, torch.bfloat16


def worst_index(err):
    """The element a BoundError names."""
    m = re.search(r'worst at \(([\d, ]*)\)', str(err.value))
    assert m is not None, str(err.value)
    return tuple(int(i) for i in m.group(1).replace(' ', '').split(',') if i)


# ---------------------------------------------------------------------------------------------------- cross-entropy

def emulate_ce(x, t, g, dtype, ld_max=None, onehot_clamped=False, drop_tail=False):
    """ce_fused_kernel in fp32 torch: max, exp(x - m) summed, l = m + log s, loss = l - x[clamped t], (exp(x - l) - one_hot) g."""
    R, C = x.shape
    x = x.float()
    m = (x if ld_max is None else ld_max).max(-1, keepdim=True).values
    s = torch.exp(x - m).sum(-1, keepdim=True)
    l = m + torch.log(s)
    tc = t.clamp(0, C - 1)
    loss = (l - x.gather(1, tc.reshape(R, 1)))[:, 0]
    oh = torch.zeros_like(x)
    hit = torch.ones_like(t, dtype=torch.bool) if onehot_clamped else (t >= 0) & (t < C)
    oh[hit.nonzero()[:, 0], tc[hit]] = 1.0
    d = ((torch.exp(x - l) - oh) * g.float().reshape(R, 1)).to(dtype)
    if drop_tail and C % 4:
        d[:, C - C % 4:] = 0
    return loss, l[:, 0], d


def check_ce(tag, loss, lse, d, r):
    return max(tb.check(tag + ' loss', loss, r['loss'], r['e_loss']), tb.check(tag + ' lse', lse, r['lse'], r['e_lse']),
               tb.check(tag + ' dlogits', d, r['dlogits'], r['e_dlogits']))


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('C', tb.CE_CLASSES)
def test_emulated_cross_entropy_passes_at_every_class_count(dtype, C):
    x, t, g = tb.ce_case(tb.ce_rows(C), C)
    assert check_ce(f'C={C}', *emulate_ce(x, t, g, dtype), tb.ce_ref(x, t, g)) <= 1.0


@pytest.mark.parametrize('regime', tb.CE_REGIMES)
@pytest.mark.parametrize('C', tb.CE_REGIME_CLASSES)
def test_emulated_cross_entropy_passes_in_every_regime(C, regime):
    x, t, g = tb.ce_case(9, C, regime)
    r = tb.ce_ref(x, t, g)
    for dtype in (F32, BF16):
        loss, lse, d = emulate_ce(x, t, g, dtype)
        assert check_ce(f'{regime} C={C}', loss, lse, d, r) <= 1.0
        if regime.startswith('pad'):
            k = int(regime[3:])
            assert not bool(d[:, C - k:].any()) and not bool(r['dlogits'][:, C - k:].any())


def test_cross_entropy_row_sweeps_pass():
    for R in (8192 + 5, 16384 + 3, 1048576 // 12 + 7):
        x, t, g = tb.ce_case(R, 12)
        assert check_ce(f'R={R}', *emulate_ce(x, t, g, F32), tb.ce_ref(x, t, g)) <= 1.0


def test_given_lse_is_an_input_of_the_gradient():
    """wmz_ce_bwd's reference takes the lse it is given as exact: a kernel handed a wrong lse must reproduce exp(x - lse)."""
    x, t, g = tb.ce_case(11, 257)
    lse = (torch.logsumexp(x.double(), -1) + 0.25).float()
    d = ((torch.exp(x - lse[:, None]) - torch.nn.functional.one_hot(t.clamp(0, 256), 257) * ((t >= 0) & (t < 257))[:, None]) * g[:, None])
    r = tb.ce_ref(x, t, g, lse=lse)
    assert tb.check('given lse', d.float(), r['dlogits'], r['e_dlogits']) <= 1.0
    with pytest.raises(tb.BoundError):
        tb.check('own lse', d.float(), tb.ce_ref(x, t, g)['dlogits'], tb.ce_ref(x, t, g)['e_dlogits'])


def test_cross_entropy_mistakes_fail():
    C, R = 1030, 13
    x, t, g = tb.ce_case(R, C)
    r = tb.ce_ref(x, t, g)
    # the maximum over ld columns: the padding behind the classes (here 300) becomes m and every exp(x - m) underflows
    xl = torch.cat([x, torch.full((R, 6), 300.0)], 1)
    with pytest.raises(tb.BoundError, match='loss'):
        check_ce('max over ld', *emulate_ce(x, t, g, F32, ld_max=xl), r)
    # the one-hot at the clamped index of an out-of-range target: rows 2 (t = -1), 3 (t = C) and 4 (t = 2^32 + 1)
    with pytest.raises(tb.BoundError, match='dlogits') as err:
        check_ce('clamped one-hot', *emulate_ce(x, t, g, F32, onehot_clamped=True), r)
    assert worst_index(err) in ((2, 0), (3, C - 1), (4, C - 1))
    # the last partial float4 of a row not stored
    with pytest.raises(tb.BoundError, match='dlogits') as err:
        check_ce('tail dropped', *emulate_ce(x, t, g, BF16, drop_tail=True), r)
    assert worst_index(err)[1] >= C - C % 4


# ---------------------------------------------------------------------------------------------------- AdamW and the norm

def emulate_adamw(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale, mistake=None):
    """adamw_one (csrc/optim.hip) in fp32 torch, operation by operation."""
    f = np.float32
    lr, b1, b2, eps, wd, gs = (f(h) for h in (lr, beta1, beta2, eps, weight_decay, grad_scale))
    bc1, sbc2 = f(1.0 - beta1 ** step), f((1.0 - beta2 ** step) ** 0.5)
    if mistake == 'no_bias_correction':
        bc1 = f(1.0)
    if mistake == 'betas_swapped':
        b1, b2 = b2, b1
    dec = float(f(1.0) - lr * wd)
    gi = g * float(gs)
    pi = p if mistake == 'decay_after' else p * dec
    mi = float(b1) * m + float(f(1.0) - b1) * gi
    vi = float(b2) * v + float(f(1.0) - b2) * gi * gi
    pi = pi - float(lr / bc1) * (mi / (vi.sqrt() / float(sbc2) + float(eps)))
    if mistake == 'decay_after':
        pi = pi * dec
    if mistake == 'tail' and p.numel() % 4:
        k = p.numel() - p.numel() % 4
        pi[k:], mi[k:], vi[k:] = p[k:], m[k:], v[k:]
    return pi, mi, vi


def check_adamw(tag, got, r):
    return max(tb.check(f'{tag} {k}', x, r[k], r['e_' + k]) for k, x in zip('pmv', got))


@pytest.mark.parametrize('n', tb.ADAMW_N)
def test_emulated_adamw_passes(n):
    p, g, m, v = tb.adamw_case(n)
    combos = [(wd, gs, step) for wd in (0.0, tb.f32(0.01)) for gs in (1.0, 0.125) for step in (1, 2, 1000)]
    for wd, gs, step in combos if n < 100000 else combos[4:6]:
        h = dict(tb.ADAMW_HYPER, weight_decay=wd, step=step, grad_scale=gs)
        assert check_adamw(f'n={n} wd={wd} gs={gs} t={step}', emulate_adamw(p, g, m, v, **h), tb.adamw_ref(p, g, m, v, **h)) <= 1.0


def test_emulated_adamw_three_steps_against_torch():
    n = 2049
    p, g, m, v = tb.adamw_case(n)
    grads = [g, tb.adamw_case(n, seed=1)[1], tb.adamw_case(n, seed=2)[1]]
    h = dict(tb.ADAMW_HYPER, weight_decay=tb.f32(0.01), grad_scale=0.125)
    for first in (1, 1000):
        state = (p, m, v)
        for k, gk in enumerate(grads):
            state = emulate_adamw(state[0], gk, state[1], state[2], step=first + k, **h)
        P, e_p, M, e_m, V, e_v = tb.adamw_torch_steps(p, grads, m, v, first_step=first, **h)
        assert max(tb.check('p', state[0], P, e_p), tb.check('m', state[1], M, e_m), tb.check('v', state[2], V, e_v)) <= 1.0


@pytest.mark.parametrize('mistake', ['decay_after', 'no_bias_correction', 'betas_swapped', 'tail'])
def test_adamw_mistakes_fail(mistake):
    n = 2047
    p, g, m, v = tb.adamw_case(n)
    h = dict(tb.ADAMW_HYPER, lr=tb.f32(1e-2), weight_decay=tb.f32(0.1), step=2, grad_scale=1.0)
    r = tb.adamw_ref(p, g, m, v, **h)
    assert check_adamw('correct', emulate_adamw(p, g, m, v, **h), r) <= 1.0
    with pytest.raises(tb.BoundError) as err:
        check_adamw(mistake, emulate_adamw(p, g, m, v, mistake=mistake, **h), r)
    if mistake == 'tail':
        assert worst_index(err)[0] >= n - n % 4


def test_sqnorm_bound():
    g = tb.adamw_case(2049)[1]
    start = float((g * 0.125).pow(2).sum()) / 2               # of the sum's own size: far above the bound, so its loss shows
    ref, e = tb.sqnorm_ref(g, scale=0.125, start=start)
    got = torch.tensor(start) + (g * 0.125).pow(2).sum()
    assert tb.check('sqnorm', got.reshape(1), torch.tensor([ref]), torch.tensor([e])) <= 1.0
    with pytest.raises(tb.BoundError):                          # overwritten instead of accumulated
        tb.check('sqnorm', (g * 0.125).pow(2).sum().reshape(1), torch.tensor([ref]), torch.tensor([e]))


# ---------------------------------------------------------------------------------------------------- embedding

def pos3d_case(B, S, H, W, D, classes, dtype):
    ntok = B * S * H * W
    tok, dx, tabs0 = tb.embed_case(ntok, D, classes, dtype, rows=(S, H, W))
    return tok, tb.pos3d_indices(B, S, H, W), dx, tabs0


def emulate_embed_bwd(tok, idx, dx, tabs0, calls, classes, mistake=None):
    f = dx.float()
    tabs = [t.clone() for t in tabs0]
    if mistake == 'overwrite':
        tabs = [torch.zeros_like(t) for t in tabs]
    for _ in range(calls):
        for t, i in zip(tabs, (tok.clamp(0, classes - 1),) + tuple(idx)):
            t.index_add_(0, i, f)
    if mistake == 'mask_row':
        tabs[0][classes - 1] = tabs0[0][classes - 1]
    return tabs


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('shape,D', [((2, 2, 3, 5), 40), ((1, 3, 4, 16), 72), ((2, 3, 16, 16), 256), ((1, 2, 59, 5), 8)])
def test_emulated_embedding_passes_and_mistakes_fail(dtype, shape, D):
    classes = 9
    tok, idx, dx, tabs0 = pos3d_case(*shape, D, classes, dtype)
    tc = tok.clamp(0, classes - 1)
    x32, x = tb.embed_fwd_ref(tc, *idx, *tabs0, dtype)
    assert torch.equal(x, (tabs0[0][tc] + ((tabs0[1][idx[0]] + tabs0[2][idx[1]]) + tabs0[3][idx[2]])).to(dtype))
    refs = tb.embed_bwd_ref(tc, *idx, dx, tabs0, calls=2)
    for name, got, (ref, e) in zip(('emb', 'pos_s', 'pos_h', 'pos_w'), emulate_embed_bwd(tok, idx, dx, tabs0, 2, classes), refs):
        assert tb.check(name, got, ref, e) <= 1.0
    with pytest.raises(tb.BoundError) as err:
        tb.check('emb', emulate_embed_bwd(tok, idx, dx, tabs0, 2, classes, 'mask_row')[0], *refs[0])
    assert worst_index(err)[0] == classes - 1
    for k, name in enumerate(('emb', 'pos_s', 'pos_h', 'pos_w')):
        with pytest.raises(tb.BoundError):
            tb.check(name, emulate_embed_bwd(tok, idx, dx, tabs0, 2, classes, 'overwrite')[k], *refs[k])


@pytest.mark.parametrize('D', [8, 40, 512])
@pytest.mark.parametrize('ntok', [1, 63, 64, 3072])
def test_emulated_indexed_embedding_backward_passes(ntok, D):
    """The indexed form's shapes: arbitrary (repeated) positions on a 481 x 2 x 2 grid, half the tokens on the mask class."""
    S, H, W, classes = 481, 2, 2, 9
    tok, dx, tabs0 = tb.embed_case(ntok, D, classes, BF16, rows=(S, H, W))
    pos = torch.randint(0, S * H * W, (ntok,), generator=torch.Generator().manual_seed(ntok + D))
    pos[ntok // 3:ntok // 3 + 5] = pos[0]
    idx = (pos // (H * W), (pos // W) % H, pos % W)
    refs = tb.embed_bwd_ref(tok.clamp(0, classes - 1), *idx, dx, tabs0, calls=2)
    for name, got, (ref, e) in zip(('emb', 'pos_s', 'pos_h', 'pos_w'), emulate_embed_bwd(tok, idx, dx, tabs0, 2, classes), refs):
        assert tb.check(name, got, ref, e) <= 1.0


# ---------------------------------------------------------------------------------------------------- Philox and the corruption

@pytest.mark.skipif(CXX is None, reason='no host C++ compiler available')
def test_numpy_philox_equals_the_header_word_for_word(host):  # noqa: F811
    for index, stream, seed in BLOCKS:
        (line,) = host('b', index, stream, seed)
        assert [int(w, 16) for w in line.split()[:4]] == tb.philox4x32_np(np.array([index], dtype=np.uint64), stream, seed)[0].tolist()
    for base, stream, seed in ((0, 0, 0), ((1 << 32) - 150, (3 << 40) | 77, 0x0123456789ABCDEF)):
        idx = np.arange(300, dtype=np.uint64) + np.uint64(base)              # consecutive indices, across the 2^32 carry
        args = [a for i in idx for a in ('b', int(i), stream, seed)]
        want = [[int(w, 16) for w in line.split()[:4]] for line in host(*args)]
        assert want == tb.philox4x32_np(idx, stream, seed).tolist()


@pytest.mark.parametrize('rate', [0.0, 1.0, 0.5])
def test_corrupt_reference_has_the_reference_frequencies(rate):
    C, B, HW = 8, 2, 60000
    z = torch.full((B, HW), 3)
    out = tb.corrupt_ref(z, torch.tensor([rate, rate]), C, seed=11, stream=(1 << 40) | 5)
    if rate == 0.0:
        assert torch.equal(out, z)
    if rate == 1.0:
        assert bool((out == C).all())
    a = 0.1 * rate
    expect = torch.full((C + 1,), (1 - rate) * a / C)
    expect[3] = (1 - rate) * (1 - a + a / C)
    expect[C] = rate
    freq = torch.bincount(out.reshape(-1), minlength=C + 1).double() / (B * HW)
    # binomial: 5 standard deviations of a frequency over B * HW draws, at the most sqrt(0.25 / n) each
    assert float((freq - expect).abs().max()) <= 5 * (0.25 / (B * HW)) ** 0.5, (freq, expect)
    assert not torch.equal(out[0], out[1]) or rate in (0.0, 1.0)            # keyed by the flat index, not by p alone
