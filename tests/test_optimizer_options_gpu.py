"""GPU: the optimizer-option kernels of csrc/optim.hip -- the Adam law (wmz_adam_step, wmz_adam_step_dev), global-norm clipping and
the non-finite-step skip (wmz_optim_step_clipped_dev) -- called through _lib.call, every element of p, m, v against the fp64
references and bounds of tests/optim_bounds.py, every array inside a sentinel frame as in test_train_tail_gpu.py, past both grid
caps and on the n % 4 tail.  The trainers do not reach these entry points yet (profiles/optimizer_options/README.md)."""
import functools
import math

import pytest
import torch

import optim_bounds as ob
import tail_bounds as tb

pytestmark = pytest.mark.gpu

F32 = torch.float32
H = tb.ADAMW_HYPER
N_TAIL, N_NORM_CAP, N_CAP = 4099, 256 * 512 * 4 + 2051, 2048 * 512 * 4 + 2051


@pytest.fixture(scope='module')
def L():
    assert torch.cuda.is_available()
    from world_modelz_amd import _lib
    _lib.lib()
    return _lib


def report(tag, worst):
    print(f'[optim] {tag}: worst |got - ref| / tol = {worst:.3f}')
    return worst


# ---------------------------------------------------------------------------------------------------- kernels

@functools.lru_cache(maxsize=2)
def case(n):
    return tb.adamw_case(n)


def framed_flat(fill):
    buf, view, mask = tb.framed_flat((fill.numel(),), F32, 'cuda', pad=64)
    view.copy_(fill)
    return buf, view, mask


def state(p, m, v):
    """Framed device copies of the state the kernels update in place -> ([views], [(buf, mask)])."""
    fr = [framed_flat(t) for t in (p, m, v)]
    return [f[1] for f in fr], [(f[0], f[2]) for f in fr]


def hyper_tensor(step, lr=H['lr']):
    return torch.tensor([tb.f32(lr), tb.f32(1.0 - H['beta1'] ** step), tb.f32((1.0 - H['beta2'] ** step) ** 0.5)], device='cuda')


def tiled(n, fn):
    """fn on the first min(n, ADAMW_PERIOD) elements, tiled to n (tb.adamw_case repeats with that period; the laws are element-wise)."""
    r = fn(min(n, tb.ADAMW_PERIOD))
    return {key: tb.tile(val, n) for key, val in r.items()}


def step_dev(L, name, s, gd, n, step, wd, gs, sq=None):
    L.call(name, L.ptr(s[0]), L.ptr(gd), L.ptr(s[1]), L.ptr(s[2]), n, L.ptr(hyper_tensor(step)), H['beta1'], H['beta2'], H['eps'], wd, gs,
           None if sq is None else L.ptr(sq), L.stream())


def step_clipped(L, s, gd, n, step, wd, gs, sq, max_norm, decoupled, skip):
    L.call('wmz_optim_step_clipped_dev', L.ptr(s[0]), L.ptr(gd), L.ptr(s[1]), L.ptr(s[2]), n, L.ptr(hyper_tensor(step)), H['beta1'],
           H['beta2'], H['eps'], wd, gs, L.ptr(sq), float(max_norm), int(decoupled), int(skip), L.stream())


def untouched(frames):
    for buf, mask in frames:
        tb.assert_untouched(buf, mask)


@pytest.mark.parametrize('step', [1, 1000])
@pytest.mark.parametrize('gs', [1.0, 0.5])
@pytest.mark.parametrize('wd', [0.0, tb.f32(0.01)], ids=['wd0', 'wd0.01'])
@pytest.mark.parametrize('n', [N_TAIL, N_NORM_CAP, N_CAP])
def test_adam_kernels(L, n, wd, gs, step):
    """wmz_adam_step and wmz_adam_step_dev: bit-identical, every element of p, m, v within its adam_ref bound; the norm that rides
    along is that of grad_scale g (not of gi) and agrees with wmz_grad_sqnorm; wd = 0: torch.equal to the AdamW entry point.
    n % 4 = 3 everywhere; both grid caps: 256 workgroups with the norm (n = 526 339), 2 048 without (n = 4 196 355: that grid only)."""
    p, g, m, v = case(n)
    with_norm = n < N_CAP
    gd = g.cuda()
    sa, fa = state(p, m, v)
    sb, fb = state(p, m, v)
    L.call('wmz_adam_step', L.ptr(sa[0]), L.ptr(gd), L.ptr(sa[1]), L.ptr(sa[2]), n, H['lr'], H['beta1'], H['beta2'], H['eps'], wd, step, gs,
           L.stream())
    total = float((g.double() * gs).pow(2).sum())
    start = tb.f32(total / 2 + 1.0)                              # of the sum's own size: losing it would show
    sq_buf, sq, sq_mask = framed_flat(torch.tensor([start]))
    step_dev(L, 'wmz_adam_step_dev', sb, gd, n, step, wd, gs, sq if with_norm else None)
    n_buf, nsq, n_mask = framed_flat(torch.zeros(1))
    L.call('wmz_grad_sqnorm', L.ptr(gd), n, gs, L.ptr(nsq), L.stream())
    torch.cuda.synchronize()
    untouched(fa + fb + [(sq_buf, sq_mask), (n_buf, n_mask)])
    for name, a, b in zip('pmv', sa, sb):
        assert torch.equal(a, b), f'{name}: wmz_adam_step != wmz_adam_step_dev'
    r = tiled(n, lambda k: ob.adam_ref(p[:k], g[:k], m[:k], v[:k], weight_decay=wd, step=step, grad_scale=gs, **H))
    report(f'adam_step n={n} wd={wd} gs={gs} t={step}', max(tb.check(f'adam {k}', x.cpu(), r[k], r['e_' + k]) for k, x in zip('pmv', sa)))
    if with_norm:
        ref0, e0 = tb.sqnorm_ref(g, gs)
        ref1, e1 = tb.sqnorm_ref(g, gs, start=start)
        tb.check('grad_sqnorm', nsq.cpu(), torch.tensor([ref0]), torch.tensor([e0]))
        tb.check('adam sqnorm_out', sq.cpu(), torch.tensor([ref1]), torch.tensor([e1]))       # the gradient's norm: wd p is not in it
        tol = (e0 + tb.U32 * (ref0 + e0)) + (e1 + tb.U32 * (ref1 + e1))
        assert abs((float(sq) - start) - float(nsq)) <= tol + tb.U32 * start, (float(sq), start, float(nsq), tol)
    else:
        assert float(sq) == start
    if wd == 0.0:
        sc, fc = state(p, m, v)
        step_dev(L, 'wmz_adamw_step_dev', sc, gd, n, step, wd, gs)
        torch.cuda.synchronize()
        untouched(fc)
        for name, a, c in zip('pmv', sa, sc):
            assert torch.equal(a, c), f'{name}: Adam != AdamW at wd = 0'
    else:
        sc, _ = state(p, m, v)
        step_dev(L, 'wmz_adamw_step_dev', sc, gd, n, step, wd, gs)
        assert not torch.equal(sa[1], sc[1]) and not torch.equal(sa[2], sc[2])                # L2, not decoupled: the decay moves m, v


def norm_word(L, gd, n, gs):
    """The squared norm as a training step hands it over: wmz_grad_sqnorm into a zeroed word (framed)."""
    buf, sq, mask = framed_flat(torch.zeros(1))
    L.call('wmz_grad_sqnorm', L.ptr(gd), n, gs, L.ptr(sq), L.stream())
    return buf, sq, mask


@pytest.mark.parametrize('decoupled', [1, 0], ids=['AdamW', 'Adam'])
@pytest.mark.parametrize('n', [N_TAIL, N_CAP])
def test_clipped_form_below_the_threshold_is_the_unclipped_entry_point(L, n, decoupled):
    """sq below max_norm^2 (coef == 1), and max_norm = 0 with the skip armed and a finite sq: bit-identical to wmz_adamw_step_dev /
    wmz_adam_step_dev; sqnorm_in is read, not written."""
    p, g, m, v = case(n)
    gd, wd, gs, step = g.cuda(), tb.f32(0.01), 0.5, 3
    sq_buf, sq, sq_mask = norm_word(L, gd, n, gs)
    word = sq.clone()
    s0, f0 = state(p, m, v)
    step_dev(L, 'wmz_adamw_step_dev' if decoupled else 'wmz_adam_step_dev', s0, gd, n, step, wd, gs)
    for max_norm, skip in ((2.0 * math.sqrt(float(word)), 0), (2.0 * math.sqrt(float(word)), 1), (0.0, 1), (-1.0, 0)):
        s1, f1 = state(p, m, v)
        step_clipped(L, s1, gd, n, step, wd, gs, sq, max_norm, decoupled, skip)
        torch.cuda.synchronize()
        untouched(f0 + f1 + [(sq_buf, sq_mask)])
        assert torch.equal(sq, word)
        for name, a, b in zip('pmv', s0, s1):
            assert torch.equal(a, b), f'{name}: clipped form (max_norm {max_norm}, skip {skip}) != unclipped'


@pytest.mark.parametrize('decoupled', [1, 0], ids=['AdamW', 'Adam'])
@pytest.mark.parametrize('n', [N_TAIL, N_CAP])
def test_clipped_form_above_the_threshold(L, n, decoupled):
    """sq above max_norm^2: every element inside the bound of clip_ref o adam(w)_ref at the word the kernel loaded; at n = 4 099
    also against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam / AdamW on fp64 copies, the norm pass's own bound added."""
    p, g, m, v = case(n)
    gd, wd, gs, step = g.cuda(), tb.f32(0.01), 0.5, 3
    sq_buf, sq, sq_mask = norm_word(L, gd, n, gs)
    word = float(sq)
    max_norm = tb.f32(0.5 * math.sqrt(word))
    s1, f1 = state(p, m, v)
    step_clipped(L, s1, gd, n, step, wd, gs, sq, max_norm, decoupled, 0)
    torch.cuda.synchronize()
    untouched(f1 + [(sq_buf, sq_mask)])
    coef, e_coef = ob.clip_ref(word, max_norm)
    assert abs(coef - 0.5) < 1e-3 and e_coef < 1e-6
    r = tiled(n, lambda k: ob.clipped_ref(bool(decoupled), p[:k], g[:k], m[:k], v[:k], word, max_norm, weight_decay=wd, step=step,
                                          grad_scale=gs, **H))
    report(f'clipped n={n} decoupled={decoupled}', max(tb.check(f'clipped {k}', x.cpu(), r[k], r['e_' + k]) for k, x in zip('pmv', s1)))
    s0, _ = state(p, m, v)
    step_dev(L, 'wmz_adamw_step_dev' if decoupled else 'wmz_adam_step_dev', s0, gd, n, step, wd, gs)
    assert not torch.equal(s0[0], s1[0]) and not torch.equal(s0[1], s1[1])                    # the clip bit
    if n == N_TAIL:
        P, e_p, M, e_m, V, e_v, norms = ob.torch_steps('AdamW' if decoupled else 'Adam', p, [g], m, v, weight_decay=wd, first_step=step,
                                                       grad_scale=gs, max_norm=max_norm, **H)
        assert abs(norms[0] - math.sqrt(word)) <= 1e-3 * norms[0]
        report(f'clipped vs torch pair decoupled={decoupled}',
               max(tb.check('p', s1[0].cpu(), P, e_p), tb.check('m', s1[1].cpu(), M, e_m), tb.check('v', s1[2].cpu(), V, e_v)))


@pytest.mark.parametrize('decoupled', [1, 0], ids=['AdamW', 'Adam'])
@pytest.mark.parametrize('bad', [float('inf'), float('nan'), -float('nan')], ids=['inf', 'nan', '-nan'])
@pytest.mark.parametrize('n', [N_TAIL, N_CAP])
def test_clipped_form_skips_a_non_finite_norm(L, n, bad, decoupled):
    """sq = inf / NaN under skip_nonfinite: p, m, v and every frame bit-unchanged, with and without a max_norm."""
    p, g, m, v = case(n)
    gd = g.clone()
    gd[5] = bad
    gd = gd.cuda()
    sq_buf, sq, sq_mask = framed_flat(torch.tensor([bad]))
    s1, f1 = state(p, m, v)
    before = [t.clone() for t in s1]
    for max_norm in (0.0, 1.0):
        step_clipped(L, s1, gd, n, 3, tb.f32(0.01), 0.5, sq, max_norm, decoupled, 1)
    torch.cuda.synchronize()
    untouched(f1 + [(sq_buf, sq_mask)])
    for name, a, b in zip('pmv', before, s1):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f'{name} was written by a skipped step'
