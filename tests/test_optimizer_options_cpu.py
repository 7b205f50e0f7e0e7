"""CPU: the references of tests/optim_bounds.py against torch.optim.Adam / AdamW and torch.nn.utils.clip_grad_norm_ on fp64 tensors
(independent of the kernels' formulas), and the three optimizer-option entry points in the header and the binding."""
import math

import pytest
import torch

import abi_header
import optim_bounds as ob
import tail_bounds as tb

H = tb.ADAMW_HYPER
NEW = {'wmz_adam_step': 13, 'wmz_adam_step_dev': 13, 'wmz_optim_step_clipped_dev': 16}


def close(got, ref, e, what):
    """got (fp64, from torch) within the law's own bound of ref: the two evaluate one formula in fp64, so they agree far inside it;
    the bound must also be finite and, where the value moves at all, positive."""
    assert torch.isfinite(e).all(), what
    assert bool(((got - ref).abs() <= 1e-3 * e + 1e-12 * ref.abs() + 1e-300).all()), (what, float((got - ref).abs().max()))


@pytest.mark.parametrize('first', [1, 1000])
@pytest.mark.parametrize('wd', [0.0, tb.f32(0.01)])
@pytest.mark.parametrize('gs', [1.0, 0.5])
def test_adam_ref_is_torch_adam(first, wd, gs):
    """adam_ref, step by step over three seeded steps, against torch.optim.Adam(foreach=False) on fp64 copies."""
    n = 257
    p, g, m, v = tb.adamw_case(n)
    grads = [g, tb.adamw_case(n, seed=1)[1], tb.adamw_case(n, seed=2)[1]]
    P, M, V = p.double(), m.double(), v.double()
    for k, gk in enumerate(grads):
        r = ob.adam_ref(P, gk, M, V, weight_decay=wd, step=first + k, grad_scale=gs, **H)
        Pt, _, Mt, _, Vt, _, _ = ob.torch_steps('Adam', P, [gk], M, V, weight_decay=wd, first_step=first + k, grad_scale=gs, **H)
        for name, got, ref in (('p', Pt, r['p']), ('m', Mt, r['m']), ('v', Vt, r['v'])):
            close(got, ref, r['e_' + name], (name, k))
        P, M, V = Pt, Mt, Vt
    if wd:                                                       # L2, not decoupled: the decay moves m and v
        r0 = ob.adam_ref(p, g, m, v, weight_decay=0.0, step=first, grad_scale=gs, **H)
        r1 = ob.adam_ref(p, g, m, v, weight_decay=wd, step=first, grad_scale=gs, **H)
        assert not torch.equal(r0['m'], r1['m']) and not torch.equal(r0['v'], r1['v'])


def test_decoupled_law_ref_is_tail_bounds_adamw_ref_and_no_tighter():
    p, g, m, v = tb.adamw_case(513)
    for wd in (0.0, tb.f32(0.01)):
        a = tb.adamw_ref(p, g, m, v, weight_decay=wd, step=3, grad_scale=0.125, **H)
        b = ob.law_ref(True, p, g, m, v, weight_decay=wd, step=3, grad_scale=0.125, **H)
        for k in 'pmv':
            assert torch.equal(a[k], b[k]), k
            assert bool((b['e_' + k] >= a['e_' + k] * (1 - 1e-9)).all()), k
            assert bool((b['e_' + k] <= 4 * a['e_' + k] + 1e-300).all()), k     # ... nor loose: the rigorous sqrt costs a factor <= 2


def test_adam_with_zero_decay_is_the_adamw_law():
    p, g, m, v = tb.adamw_case(300)
    a = ob.adam_ref(p, g, m, v, weight_decay=0.0, step=2, grad_scale=0.5, **H)
    b = tb.adamw_ref(p, g, m, v, weight_decay=0.0, step=2, grad_scale=0.5, **H)
    for k in 'pmv':
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize('optimizer', ['Adam', 'AdamW'])
@pytest.mark.parametrize('frac', [0.5, 0.01, 3.0])
def test_clip_ref_is_clip_grad_norm(optimizer, frac):
    """clip_ref against the coefficient clip_grad_norm_ applied (read off the gradient it rescaled) and the norm it returned, then
    three clipped steps of the fp64 torch pair against clipped_ref."""
    n = 257
    p, g, m, v = tb.adamw_case(n)
    gs = 0.5
    sq, _ = tb.sqnorm_ref(g, gs)
    max_norm = tb.f32(frac * math.sqrt(sq))
    G = torch.nn.Parameter(torch.zeros(n, dtype=torch.float64))
    G.grad = g.double() * gs
    total = float(torch.nn.utils.clip_grad_norm_([G], max_norm, norm_type=2, foreach=False))
    assert abs(total - math.sqrt(sq)) <= 1e-12 * total           # the returned norm is the pre-clip one
    coef, e_coef = ob.clip_ref(sq, max_norm)
    k = int(g.abs().argmax())
    applied = float(G.grad[k] / (g.double()[k] * gs))
    assert abs(applied - coef) <= e_coef + 1e-12 and 0 <= e_coef < 1e-5
    assert (coef == 1.0) == (frac > 1) and (frac > 1 or abs(coef - frac) < 1e-3)
    assert ob.clip_ref(sq, 0.0) == (1.0, 0.0) and ob.clip_ref(sq, -1.0) == (1.0, 0.0)
    grads = [g, tb.adamw_case(n, seed=1)[1], tb.adamw_case(n, seed=2)[1]]
    P, M, V = p.double(), m.double(), v.double()
    wd = tb.f32(0.01)
    for j, gk in enumerate(grads):
        sqk, _ = tb.sqnorm_ref(gk, gs)
        r = ob.clipped_ref(optimizer == 'AdamW', P, gk, M, V, sqk, max_norm, weight_decay=wd, step=5 + j, grad_scale=gs, **H)
        Pt, _, Mt, _, Vt, _, norms = ob.torch_steps(optimizer, P, [gk], M, V, weight_decay=wd, first_step=5 + j, grad_scale=gs,
                                                    max_norm=max_norm, **H)
        assert abs(norms[0] - math.sqrt(sqk)) <= 1e-12 * norms[0]
        for name, got, ref in (('p', Pt, r['p']), ('m', Mt, r['m']), ('v', Vt, r['v'])):
            close(got, ref, r['e_' + name], (name, j))
        P, M, V = Pt, Mt, Vt


def test_new_entry_points_are_declared_and_bound_and_the_abi_did_not_move():
    from world_modelz_amd import _lib
    for name, count in NEW.items():
        assert name in abi_header.declared(), name
        assert abi_header.arguments(name).count(',') + 1 == count == len(_lib.SIGNATURES[name]), name
    assert _lib.SIGNATURES['wmz_adam_step'] == _lib.SIGNATURES['wmz_adamw_step']
    assert _lib.SIGNATURES['wmz_adam_step_dev'] == _lib.SIGNATURES['wmz_adamw_step_dev']
    assert abi_header.constants('WMZ_VERSION')['WMZ_VERSION'] == 115 == _lib.EXPECTED_VERSION
    assert len(_lib.CONSTANTS) == 21
    abi_header.assert_bound(_lib.lib(), *NEW)
