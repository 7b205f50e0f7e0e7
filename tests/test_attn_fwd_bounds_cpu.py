"""tests/attn_fwd_bounds.py held to account on the CPU, for every case the GPU test (tests/test_attn_fwd_routes_gpu.py) runs: the
dense fp64 reference equals the oracle (symmetric windows) and tests/causal_ref.py (causal and asymmetric ones); an fp32 emulation of
the kernels' arithmetic (their rounding points, a deferred reference, another summation order) is inside the bound in every logit
regime; each seeded error is outside it on a case of every route family; the inputs are such that EVERY single query-key pair is
visible to the indicator launches and next to no element of a plain launch cancels below its own bound; and the cases reach every
kernel instantiation the forward dispatch can launch."""
import pytest
import torch

import attn_fwd_bounds as fb
import causal_ref
import gemm_bounds as gb
from oracle import attention as oat

IDS = [c.id for c in fb.CASES]


def _worst(got, ref, e_in):
    """Largest |got - ref| / tol; gemm_bounds.check must raise exactly where it is above 1."""
    ratio = (gb.f64(got) - ref).abs() / fb.tolerance(ref, e_in, got.dtype)
    w = float(torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float('inf'))).max())      # a NaN result is outside
    try:
        assert gb.check('emulation', got, ref, e_in) == w <= 1.0
    except gb.BoundError:
        assert w > 1.0
    return w


def _worst_both(ref, got):
    return max(_worst(got[0], ref.out, ref.e_out), _worst(got[1], ref.lse, ref.e_lse))


@pytest.mark.parametrize('cid', [c.id for c in fb.CASES if c.dtype != fb.F16])
def test_reference_equals_the_oracle(cid):
    """fwd_ref in double against oracle.attention.local_attention (symmetric windows) or tests/causal_ref.py (the others): out, lse
    and every in-window slot of the probe's layout within 1e-12, the same slots masked.  (The half cases are the bf16 cases' shapes.)"""
    c = fb.CASE[cid]
    q, k, v = (t.double() for t in fb.make_qkv(c))
    eb, ef, eH, eW = c.ext
    if eb == ef:
        out, dots = oat.local_attention(k, v, q, (eb, eH, eW), c.heads, return_logits=True)
    else:
        out, dots = causal_ref.local_attention(k, v, q, (eb, eH, eW), c.heads, window=(eb, ef), return_logits=True)
    ref = fb.fwd_ref(q, k, v, c.ext, c.heads, fb.case_family(c))
    I = c.heads * c.dh
    assert float((ref.out - out.reshape(-1, I)).abs().max()) <= 1e-12
    assert float((ref.lse - torch.logsumexp(dots, -1).reshape(-1, c.heads)).abs().max()) <= 1e-12
    lg, e = fb.probe_ref(ref, c.shape, c.ext, c.heads)
    dots = dots.reshape(lg.shape)
    inside = dots > -1e8
    assert torch.equal(inside, lg > -1e8) and torch.equal(e > 0, inside | (e > 0)) and not bool((e[~inside] != 0).any())
    assert float((lg - dots)[inside].abs().max()) <= 1e-12


def _runs(family):
    """(case, regime) of a family: every case on randn, the family's regime cases in every regime."""
    for c in fb.CASES:
        if fb.case_group(c) == family:
            for regime in (fb.REGIMES if c.id in fb.REGIME_CASES else ('randn',)):
                yield c, regime


@pytest.mark.parametrize('family', fb.FAMILIES)
def test_emulation_inside_the_bound_and_seeded_errors_outside(family):
    """Every case of the family (and its regime cases in every regime): the emulation, in two key orders, inside the bound of out
    and lse.  Every seeded error outside it -- gemm_bounds.check raises BoundError -- on at least one of them."""
    caught = {}
    assert any(c.id in fb.REGIME_CASES for c, _ in _runs(family))
    for c, regime in _runs(family):
        B, S, H, W = c.shape
        x = fb.case_inputs(c.id, regime)
        fam = fb.case_family(c)
        args = (x.q, x.k, x.v, c.ext, c.heads)
        clean = _worst_both(x.ref, fb.emulate_fwd(*args, route=fam))
        other = _worst_both(x.ref, fb.emulate_fwd(*args, route=fam, seed=6))
        assert clean <= 1.0 and other <= 1.0, (c.id, regime, clean, other)
        mask = fb.window_mask4(S, H, W, c.ext)
        seeded = {}
        for ax, name in enumerate('SHW'):
            one = tuple(int(a == ax) for a in range(3))
            seeded[f'window grown in {name}'] = dict(mask=fb.window_mask4(S, H, W, c.ext, grow=one))
            seeded[f'window shifted by one in {name}'] = dict(mask=fb.window_mask4(S, H, W, c.ext, shift=one))
        seeded['eS_fwd taken for eS_back'] = dict(mask=fb.window_mask4(S, H, W, (c.ext[1], c.ext[0]) + c.ext[2:]))
        DHp = 32 if c.dh <= 32 else (64 if c.dh <= 64 else 128)
        seeded['scale of a wrong dim_head'] = dict(scale_dh=DHp if DHp != c.dh else 2 * c.dh)
        seeded['o not rescaled where l is'] = dict(no_o_rescale=True)
        seeded['lse without the ln 2 on m_run'] = dict(lse_no_ln2=True)
        line = []
        for name, kw in seeded.items():
            if 'mask' in kw and torch.equal(kw['mask'], mask):
                continue                                               # the same mask: no error seeded
            w = _worst_both(x.ref, fb.emulate_fwd(*args, route=fam, **kw))
            caught[name] = max(caught.get(name, 0.0), w)
            line.append(f'{name} {w:.3g}')
        print(f'[{c.id} {regime}] emulation ({fam}) {clean:.3f}, another key order {other:.3f}; seeded: ' + '; '.join(line))
    assert len(caught) == 10, sorted(caught)
    missed = {n: w for n, w in caught.items() if not w > 1.0}
    assert not missed, (family, missed)


@pytest.mark.parametrize('family', [f for f in fb.FAMILIES if f not in ('general-f32', 'half')])
def test_truncated_p_outside_the_bound_on_the_indicator_launches(family):
    """bf16: P truncated to the operand type, not rounded -- up to 2 u below its value where a rounded one is within u.  Over a sum of
    many pairs that is not reliably outside a worst-case bound, so it is seeded where every output element is ONE term: the indicator
    launches, out[i, c] = P_ij.  The rounded emulation stays inside on the same inputs."""
    worst = 0.0
    for cid in fb.indicator_cases():
        c = fb.CASE[cid]
        if fb.case_group(c) != family:
            continue
        x, ref = fb.case_inputs(cid), fb.case_pairs(cid)
        fam = fb.case_family(c)
        for g in range(fb.n_indicator_launches(c)):
            v = fb.indicator_v(c.shape, c.heads, c.dh, c.ext, g, c.dtype)
            out, e = ref.with_v(v)
            assert _worst(fb.emulate_fwd(x.q, x.k, v, c.ext, c.heads, route=fam)[0], out, e) <= 1.0
            w = _worst(fb.emulate_fwd(x.q, x.k, v, c.ext, c.heads, route=fam, truncate_p=True)[0], out, e)
            worst = max(worst, w)
        print(f'[{cid}] seeded: P truncated: worst ratio so far {worst:.3g}')
        if worst > 1.0:
            break
    assert worst > 1.0, (family, worst)


@pytest.mark.parametrize('cid', fb.indicator_cases())
def test_every_pair_is_visible_in_the_indicator_launches(cid):
    """A condition on the inputs, checked on the reference alone: over the ceil(slots / dh) indicator launches of a case every
    in-window pair appears as exactly one output element, and that element is above twice its own tolerance -- a pair that is missed
    leaves a zero no tolerance covers.  Every other element is exactly zero with a zero e_in."""
    c = fb.CASE[cid]
    ref = fb.case_pairs(cid)
    B, S, H, W = c.shape
    pairs, seen, low = int(ref.mask.sum()) * B * c.heads, 0, 1e30
    for g in range(fb.n_indicator_launches(c)):
        out, e = ref.with_v(fb.indicator_v(c.shape, c.heads, c.dh, c.ext, g, c.dtype))
        live = out > 0
        assert not bool((e[~live] != 0).any())
        margin = out[live] / fb.tolerance(out[live], e[live], c.dtype)
        seen += int((margin > 2.0).sum())
        low = min(low, float(margin.min())) if margin.numel() else low
    print(f'[{cid}] {pairs} pairs in {fb.n_indicator_launches(c)} launches, smallest P / tol {low:.3g}')
    assert seen == pairs, (seen, pairs)                                # a share of 1.0


@pytest.mark.parametrize('cid', IDS)
def test_next_to_no_element_is_cancelled(cid):
    """A condition on the inputs: in the plain launches the share of output elements below their own e_in is at most 1e-3, so the
    Frobenius bars of the GPU test keep their meaning."""
    for regime in (fb.REGIMES if cid in fb.REGIME_CASES else ('randn',)):
        r = fb.case_inputs(cid, regime).ref
        share = float((r.out.abs() < r.e_out).double().mean())
        assert share <= 1e-3, (cid, regime, share)


def test_every_instantiation_has_a_case():
    reached = {}
    for c in fb.CASES:
        reached.setdefault(fb.case_route(c), []).append(c.id)
        if c.id in fb.INFER_CASES:
            reached.setdefault(fb.case_route(c, lse=False), []).append(c.id)
    assert set(reached) <= set(fb.PLAIN_INSTANTIATIONS), set(reached) - set(fb.PLAIN_INSTANTIATIONS)
    missing = [n for n in fb.PLAIN_INSTANTIATIONS if n not in reached]
    assert not missing, missing
    assert len(fb.PLAIN_INSTANTIATIONS) == 6 + 2 * (6 + 12 + 12) + 2
    # PROBE = true: one instantiation per family -- 16-wide, 8-wide small and big, 32-wide small and big in bf16, one of each width
    # in half -- and both dtypes of the general kernel, whose probe is a run-time branch
    probed = [fb.case_route(fb.CASE[cid], probe=True) for cid in fb.PROBED]
    assert len(set(probed)) == len(probed) and all(', true, false, ' in n or 'attn_fwd_kernel<' in n for n in probed)
    assert {fb.case_group(fb.CASE[cid]) for cid in fb.PROBED} == set(fb.FAMILIES)
    assert {fb.case_group(fb.CASE[cid]) for cid in fb.REGIME_CASES} == set(fb.FAMILIES)
    assert {fb.case_group(fb.CASE[cid]) for cid in fb.THIRDS} == set(fb.FAMILIES)
    for cid in fb.PLANES:
        assert fb.CASE[cid].shape[0] == 1 and fb.CASE[cid].shape[1] >= 3
    assert max(c.shape[0] * c.shape[1] * c.shape[2] * c.shape[3] for c in fb.CASES) <= 1300
    # B = 2 and two or three heads somewhere in each family
    for fam in fb.FAMILIES:
        mine = [c for c in fb.CASES if fb.case_group(c) == fam]
        assert any(c.shape[0] == 2 for c in mine) and any(c.heads >= 2 for c in mine), fam


def test_route_table_reads_the_dispatch():
    """fwd_route against the conditions of attn_fwd_impl, by_dh / by_dh2 and wmz_attn_fwd_row16_infer_takes, spelled out once more."""
    r = fb.fwd_route
    row, f16, r32 = 'attn_fwd_row16.hip: ', 'attn_fwd_row16_f16.hip: ', 'attn_fwd_row32.hip: '
    assert r((1, 2, 16, 16), 128, fb.F32) == 'attn_fwd.hip: attn_fwd_kernel<float, 128, 1, 4, 8>'
    assert r((1, 2, 16, 16), 64, fb.F32) == 'attn_fwd.hip: attn_fwd_kernel<float, 64, 1, 8, 8>'
    assert r((1, 2, 16, 16), 96, fb.BF16) == 'attn_fwd.hip: attn_fwd_kernel<bf16_t, 128, 1, 8, 16>'
    assert r((1, 2, 7, 8), 32, fb.BF16) == 'attn_fwd.hip: attn_fwd_kernel<bf16_t, 32, 1, 8, 16>'
    assert r((1, 2, 16, 16), 128, fb.BF16, general=True) == 'attn_fwd.hip: attn_fwd_kernel<bf16_t, 128, 1, 8, 16>'
    assert r((1, 2, 16, 16), 128, fb.BF16) == row + 'attn_fwd_row16_kernel<128, Big, 9, true, false, false, false>'
    assert r((1, 2, 16, 16), 128, fb.BF16, probe=True) == row + 'attn_fwd_row16_kernel<128, Big, 9, true, true, false, false>'
    assert r((1, 2, 4, 16), 64, fb.BF16) == row + 'attn_fwd_row16_kernel<64, Big, 9, false, false, false, false>'     # 16-wide: never Small
    assert r((1, 2, 17, 16), 32, fb.F16) == f16 + 'attn_fwd_row16_kernel<32, Big, 9, false, false, false, false>'
    # 8-wide: Small iff H / 2 <= 8, aligned on 4 (Small) or 16 (Big) tile rows
    assert r((1, 2, 16, 8), 128, fb.BF16) == row + 'attn_fwd_row16_kernel<128, Small, 9, true, false, false, true>'
    assert r((1, 2, 12, 8), 128, fb.BF16) == row + 'attn_fwd_row16_kernel<128, Small, 9, false, false, false, true>'
    assert r((1, 2, 18, 8), 64, fb.BF16) == row + 'attn_fwd_row16_kernel<64, Big, 9, false, false, false, true>'
    assert r((1, 2, 24, 8), 64, fb.BF16) == row + 'attn_fwd_row16_kernel<64, Big, 9, false, false, false, true>'      # 12 tile rows: % 4 does not align Big
    assert r((1, 2, 32, 8), 32, fb.F16) == f16 + 'attn_fwd_row16_kernel<32, Big, 9, true, false, false, true>'
    # 32-wide: Small iff 2 H <= 8
    assert r((1, 2, 4, 32), 64, fb.BF16) == r32 + 'attn_fwd_row16_kernel<64, Small, 25, true, false, false, false>'
    assert r((1, 2, 3, 32), 64, fb.BF16) == r32 + 'attn_fwd_row16_kernel<64, Small, 25, false, false, false, false>'
    assert r((1, 2, 5, 32), 128, fb.BF16) == r32 + 'attn_fwd_row16_kernel<128, Big, 25, false, false, false, false>'
    assert r((1, 2, 8, 32), 128, fb.F16, probe=True) == 'attn_fwd_row32_f16.hip: attn_fwd_row16_kernel<128, Big, 25, true, true, false, false>'
    # half off the row shapes, dim_head above 128: WMZ_ERR_UNSUPPORTED
    assert r((1, 2, 5, 7), 64, fb.F16) is None and r((1, 2, 16, 16), 40, fb.F16) is None and r((1, 2, 7, 8), 64, fb.F16) is None
    assert r((1, 2, 16, 16), 128, fb.F16, general=True) is None and r((1, 2, 16, 16), 136, fb.BF16) is None
    # the inference unit: bf16, no lse, no probe, symmetric time window, 16x16 planes, dh 128, one head, every row stride 128,
    # in-plane extents (3, 3) or (1, 1)
    u33, u11 = fb.INFER.format(3), fb.INFER.format(1)
    geo = dict(ext=(1, 1, 3, 3), heads=1)
    assert r((2, 5, 16, 16), 128, fb.BF16, lse=False, **geo) == u33
    assert r((2, 5, 16, 16), 128, fb.BF16, lse=False, ext=(4, 4, 1, 1)) == u11
    rt = row + 'attn_fwd_row16_kernel<128, Big, 9, true, false, false, false>'
    assert r((2, 5, 16, 16), 128, fb.BF16, lse=True, **geo) == rt
    assert r((2, 5, 16, 16), 128, fb.BF16, lse=False, probe=True, **geo) == rt.replace('true, false, false, false', 'true, true, false, false')
    assert r((2, 5, 16, 16), 128, fb.BF16, lse=False, ext=(1, 0, 3, 3)) == rt                      # causal: not the unit's
    assert r((2, 5, 16, 16), 128, fb.BF16, lse=False, ext=(1, 1, 3, 1)) == rt
    assert r((2, 5, 16, 16), 128, fb.BF16, lse=False, ld=(128, 128, 128, 144), **geo) == rt        # a framed output
    assert r((2, 5, 16, 16), 128, fb.BF16, lse=False, ld=(384, 384, 384, 128), **geo) == rt        # column thirds
    assert r((2, 5, 16, 16), 128, fb.F16, lse=False, **geo) == f16 + rt[len(row):]
    assert r((2, 5, 16, 16), 128, fb.BF16, lse=False, general=True, **geo) == 'attn_fwd.hip: attn_fwd_kernel<bf16_t, 128, 1, 8, 16>'
    assert r((2, 5, 16, 16), 64, fb.BF16, lse=False, ext=(1, 1, 3, 3), heads=2).startswith(row)
    assert r((2, 5, 12, 16), 128, fb.BF16, lse=False, **geo).startswith(row)
