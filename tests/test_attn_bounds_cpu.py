"""tests/attn_bounds.py held to account on the CPU, for every case the GPU test (tests/test_attn_bwd_routes_gpu.py) runs:
the dense fp64 reference equals torch.autograd over the oracle; an fp32 emulation of the kernels' arithmetic (their rounding
points, another summation order) is inside the bound; each of seven seeded errors is outside it; the inputs are such that
nearly every single query-key pair is visible to the element-wise check; and the cases reach every kernel instantiation the
backward dispatch can launch."""
import pytest
import torch

import attn_bounds as ab
import gemm_bounds as gb
from oracle import attention as oat

IDS = [c.id for c in ab.CASES]


def _args(c, x):
    return (x.q, x.k, x.v, x.do, x.out, x.lse, c.ext, c.heads)


def _worst(c, x, got):
    """Largest |got - ref| / tol over dq, dk, dv; gemm_bounds.check must raise exactly where it is above 1."""
    worst = 0.0
    for name, g in zip(('dq', 'dk', 'dv'), got):
        w = float(((gb.f64(g) - x.ref[name]).abs() / ab.tolerance(x.ref[name], x.ref['e_' + name], g.dtype)).max())
        try:
            assert gb.check(name, g, x.ref[name], x.ref['e_' + name]) == w <= 1.0
        except gb.BoundError:
            assert w > 1.0
        worst = max(worst, w)
    return worst


@pytest.mark.parametrize('cid', IDS)
def test_reference_equals_autograd_over_the_oracle(cid):
    """bwd_ref, fed the fp64 oracle's own out and lse, against autograd over oracle.attention.local_attention in double: 1e-12
    absolute.  dense_fwd (the probes' forward) against the oracle alike."""
    c, x = ab.CASE[cid], ab.case_inputs(cid)
    q, k, v = (t.double().requires_grad_(True) for t in (x.q, x.k, x.v))
    out = oat.local_attention(k, v, q, c.ext, c.heads)
    out.backward(x.do.double())
    assert torch.equal(out.detach(), x.out64)
    ref = ab.bwd_ref(x.q.double(), x.k.double(), x.v.double(), x.do.double(), x.out64, x.lse64, c.ext, c.heads)
    I = c.heads * c.dh
    for name, g in (('dq', q.grad), ('dk', k.grad), ('dv', v.grad)):
        err = float((ref[name] - g.reshape(-1, I)).abs().max())
        assert err <= 1e-12, (name, err)
    out_d, lse_d = ab.dense_fwd(x.q, x.k, x.v, c.ext, c.heads)
    assert float((out_d - x.out64).abs().max()) <= 1e-12 and float((lse_d - x.lse64).abs().max()) <= 1e-12


@pytest.mark.parametrize('cid', IDS)
def test_emulation_inside_the_bound_and_seeded_errors_outside(cid):
    c, x = ab.CASE[cid], ab.case_inputs(cid)
    B, S, H, W = c.shape
    fam = ab.case_family(c)
    mask = ab.window_mask(S, H, W, c.ext)
    clean = _worst(c, x, ab.emulate_bwd(*_args(c, x), route=fam))
    other = _worst(c, x, ab.emulate_bwd(*_args(c, x), route=fam, seed=6))
    print(f'[{cid}] emulation ({fam}) worst ratio {clean:.3f}, another key order {other:.3f}')
    assert clean <= 1.0 and other <= 1.0

    seeded = {}
    drop = mask.clone()
    drop[0, int(mask[0].nonzero().max())] = False                     # query 0's last in-window key
    seeded['rim pair dropped'] = dict(mask=drop)
    for ax, name in enumerate(('S', 'H', 'W')):
        grow = tuple(int(a == ax) for a in range(3))
        seeded[f'window widened in {name}'] = dict(mask=ab.shifted_mask(S, H, W, c.ext, grow=grow))
    seeded['window shifted by one column'] = dict(mask=ab.shifted_mask(S, H, W, c.ext, shift=(0, 0, 1)))
    DHp = 32 if c.dh <= 32 else (64 if c.dh <= 64 else 128)
    seeded['scale of the wrong head width'] = dict(scale_dh=DHp if DHp != c.dh else 2 * c.dh)
    seeded['delta left out'] = dict(no_delta=True)
    for name, kw in seeded.items():
        if 'mask' in kw and torch.equal(kw['mask'], mask):
            continue                                                   # this window already spans the axis: the same mask, no error seeded
        w = _worst(c, x, ab.emulate_bwd(*_args(c, x), route=fam, **kw))
        print(f'[{cid}] seeded: {name}: worst ratio {w:.3g}')
        assert w > 1.0, (name, w)


TRUNCATED = [c.id for c in ab.CASES if c.dtype == ab.BF16]


@pytest.mark.parametrize('cid', TRUNCATED)
def test_truncated_p_outside_the_bound(cid):
    """bf16: P truncated to the operand type, not rounded.  A truncated P is up to 2 u below its value where a rounded one is within
    u.  Over a sum of many pairs that halves no element's margin reliably (the bound is the worst case of every term, the mean
    truncation error is u), so the error is seeded where each dv element is ONE term: dO non-zero on a lattice of queries whose
    windows share no key (spacing 2 e + 1 per axis).  There dv_j = P_ij dO_i, the tolerance is u + u_out = 2 u of it, and
    truncation (up to 2 u) plus the output rounding (up to u) passes it for about one element in fifty; every case has more than
    700 such elements.  The rounded emulation stays inside on the same inputs."""
    c, x = ab.CASE[cid], ab.case_inputs(cid)
    B, S, H, W = c.shape
    keep = torch.zeros(S, H, W, dtype=torch.bool)
    keep[::2 * c.ext[0] + 1, ::2 * c.ext[1] + 1, ::2 * c.ext[2] + 1] = True
    do = x.do * keep[None, :, :, :, None]
    assert int(ab.window_mask(S, H, W, c.ext)[keep.reshape(-1)].sum(0).max()) == 1          # no key sees two of them
    assert B * S * H * W * c.heads * c.dh >= 700
    fam = ab.case_family(c)
    y = ab.types.SimpleNamespace(q=x.q, k=x.k, v=x.v, do=do, out=x.out, lse=x.lse,
                                 ref=ab.bwd_ref(x.q, x.k, x.v, do, x.out, x.lse, c.ext, c.heads, fam))
    assert _worst(c, y, ab.emulate_bwd(*_args(c, y), route=fam)) <= 1.0
    w = _worst(c, y, ab.emulate_bwd(*_args(c, y), route=fam, truncate_p=True))
    print(f'[{cid}] seeded: P truncated: worst ratio {w:.3g}')
    assert w > 1.0, w


@pytest.mark.parametrize('cid', IDS)
def test_pair_visibility(cid):
    """A condition on the inputs: the share of in-window pairs whose removal alone moves some element of dq, dk or dv past twice
    its tolerance is at least 0.90 in bf16 and 0.999 in fp32."""
    c, x = ab.CASE[cid], ab.case_inputs(cid)
    assert x.ref['n'] <= 75 or c.dtype == ab.F32
    share = ab.pair_visibility(*_args(c, x), x.ref)
    print(f'[{cid}] window population {x.ref["n"]}, pair visibility {share:.5f}')
    assert share >= (0.90 if c.dtype == ab.BF16 else 0.999), share


def test_every_instantiation_has_a_case():
    reached = {}
    for c in ab.CASES:
        for thirds in ((False, True) if c.id in ab.THIRDS else (False,)):
            for name in ab.case_routes(c, thirds=thirds):
                reached.setdefault(name, []).append(c.id)
    assert set(reached) <= set(ab.ALL_INSTANTIATIONS), set(reached) - set(ab.ALL_INSTANTIATIONS)
    missing = [n for n in ab.ALL_INSTANTIATIONS if n not in reached]
    assert not missing, missing
    assert len(ab.ALL_INSTANTIATIONS) == 74
    for cid in ab.PROBES:
        assert cid in ab.CASE and len(ab.PROBES[cid]) <= 7
    assert set(ab.THIRDS) <= set(ab.CASE)


def test_route_table_reads_the_dispatch():
    """bwd_route against the conditions of attn_bwd_impl / launch_both / launch_both32, spelled out once more."""
    r = ab.bwd_route
    assert r((1, 8, 16, 16), 128, ab.BF16) == ('attn_bwd_row16_kernel<128, 0, 16, 8, true, false>', 'attn_bwd_kvplane_kernel<128, true>')
    assert r((1, 8, 16, 16), 128, ab.BF16, thirds=True)[1] == 'attn_bwd_kvplane_kernel<128, false>'
    assert r((1, 8, 16, 16), 128, ab.BF16, general=True) == ('attn_bwd_kernel<bf16_t, 128, 2, 8, 0>', 'attn_bwd_kernel<bf16_t, 128, 1, 8, 1>')
    assert r((1, 2, 17, 16), 64, ab.BF16) == ('attn_bwd_row16_kernel<64, 0, 16, 8, false, false>', 'attn_bwd_row16_kernel<64, 1, 8, 8, false, false>')
    assert r((1, 2, 16, 16), 128, ab.F32) == ('attn_bwd_kernel<float, 128, 1, 4, 0>', 'attn_bwd_kernel<float, 128, 1, 4, 1>')
    assert r((1, 2, 16, 16), 96, ab.BF16)[0] == 'attn_bwd_kernel<bf16_t, 128, 2, 8, 0>'
    assert r((1, 2, 7, 8), 128, ab.BF16)[0] == 'attn_bwd_kernel<bf16_t, 128, 2, 8, 0>'
    assert r((1, 2, 16, 8), 128, ab.BF16) == ('attn_bwd_row16_kernel<128, 0, 4, 2, true, true>', 'attn_bwd_row16_kernel<128, 1, 4, 2, true, true>')
    assert r((1, 2, 18, 8), 64, ab.BF16) == ('attn_bwd_row16_kernel<64, 0, 8, 8, false, true>', 'attn_bwd_row16_kernel<64, 1, 8, 8, false, true>')
    assert r((1, 2, 32, 8), 32, ab.BF16) == ('attn_bwd_row16_kernel<32, 0, 8, 8, true, true>', 'attn_bwd_row16_kernel<32, 1, 8, 8, true, true>')
    assert r((1, 2, 2, 32), 64, ab.BF16) == ('attn_bwd_row16_kernel<64, 2, 4, 2, true, false>', 'attn_bwd_row16_kernel<64, 3, 4, 2, true, false>')
    assert r((1, 2, 8, 32), 128, ab.BF16) == ('attn_bwd_row16_kernel<128, 2, 16, 8, false, false>', 'attn_bwd_row16_kernel<128, 3, 8, 8, true, false>')
    assert r((1, 2, 8, 32), 64, ab.BF16)[0] == 'attn_bwd_row16_kernel<64, 2, 16, 8, true, false>'
