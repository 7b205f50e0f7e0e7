"""tests/gemm_bounds.py without a GPU: an fp32 torch emulation of a correct kernel (fp32 accumulation, one rounding to the output
type) passes every bound with no element left out, at the shapes tests/test_linear_family_gpu.py runs; seeded wrong results --
the mistakes a tile edge makes -- fail, with the wrong element named."""
import re

import pytest
import torch

import gemm_bounds as gb

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
GELU = torch.nn.functional.gelu


def operands(M, N, K, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    a = (torch.randn(M, K, generator=g) * 1.5 + 0.3).to(dtype)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dtype)
    bias = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g).to(dtype)
    gam, bet = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.1
    return a, w, bias, res, gam, bet


def emulate_linear(a, w, bias=None, residual=None, ln=None, gelu=False, gelu_in=False, dgelu_z=None, out_dtype=None):
    """What a correct kernel computes: prologue in fp32 rounded to the operand type, fp32 accumulation, fp32 epilogue, one rounding."""
    x = a.float()
    if ln is not None:
        x = torch.nn.functional.layer_norm(x, x.shape[-1:], ln[0], ln[1], 1e-5).to(a.dtype).float()
    if gelu_in:
        x = GELU(x).to(a.dtype).float()
    v = x @ w.float().t()
    if bias is not None:
        v = v + bias
    if gelu:
        v = GELU(v)
    if dgelu_z is not None:
        z = dgelu_z.float()
        v = v * (0.5 * (1 + torch.erf(z * 0.7071067811865476)) + z * 0.3989422804014327 * torch.exp(-0.5 * z * z))
    elif residual is not None:
        v = v + residual.float()
    return v.to(out_dtype or a.dtype)


SHAPES = [(77, 50, 24), (130, 136, 72), (130, 136, 256), (1300, 3720, 72)]


@pytest.mark.parametrize('dtype', [F32, BF16, F16])
@pytest.mark.parametrize('M,N,K', SHAPES)
def test_emulated_forward_passes_with_nothing_left_out(dtype, M, N, K):
    a, w, bias, res, gam, bet = operands(M, N, K, dtype)
    z = (torch.linspace(-6, 6, M * N).reshape(M, N)).to(dtype)
    worst = {}
    for tag, kw in [('plain', {}), ('bias', dict(bias=bias)), ('gelu', dict(bias=bias, gelu=True)),
                    ('residual', dict(bias=bias, residual=res)), ('gelu+residual', dict(bias=bias, gelu=True, residual=res)),
                    ('ln', dict(bias=bias, ln=(gam, bet))), ('gelu_in', dict(gelu_in=True)), ('dgelu', dict(dgelu_z=z))]:
        r = gb.linear_ref(a, w, **kw)
        worst[tag] = gb.check(tag, emulate_linear(a, w, **kw), r['ref'], r['e_in'])
        if dtype != F32 and tag in ('plain', 'bias', 'ln'):
            worst[tag + '/f32'] = gb.check(tag, emulate_linear(a, w, out_dtype=F32, **kw), r['ref'], r['e_in'])
    print(f'[bounds] forward {dtype} {M}x{N}x{K}: ' + ' '.join(f'{k}={v:.3f}' for k, v in worst.items()))
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize('dtype', [F32, BF16])
@pytest.mark.parametrize('M', [63, 65, 1000])
@pytest.mark.parametrize('N,K', [(136, 72), (56, 264)])
def test_emulated_wgrad_passes(dtype, M, N, K):
    g = torch.Generator().manual_seed(1)
    dc = (torch.randn(M, N, generator=g) * 0.3).to(dtype)
    a = (torch.randn(M, K, generator=g) * 1.3 + 0.2).to(dtype)
    gam, bet = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.1
    dw0, db0 = torch.randn(N, K, generator=g), torch.randn(N, generator=g)
    for ln, gin in ((None, False), ((gam, bet), False), (None, True)):
        x = a.float()
        if ln is not None:
            x = torch.nn.functional.layer_norm(x, (K,), gam, bet, 1e-5).to(dtype).float()
        if gin:
            x = GELU(x).to(dtype).float()
        for init in (True, False):
            dw, e, db, eb = gb.wgrad_ref(dc, a, dw0 if init else None, db0 if init else None, ln=ln, gelu_in=gin)
            got = dc.float().t() @ x + (dw0 if init else 0)
            gotb = dc.float().sum(0) + (db0 if init else 0)
            assert gb.check('dw', got, dw, e, norm_tol=3e-5 if dtype == F32 else 2e-3) <= 1.0
            assert gb.check('dbias', gotb, db, eb) <= 1.0


def emulate_ln_bwd(x, dy, gam, skip, skip2, dg0, db0):
    xf, dyf = x.float(), dy.float()
    mu = xf.mean(-1, keepdim=True)
    rs = ((xf - mu).pow(2).mean(-1, keepdim=True) + 1e-5).rsqrt()
    xh = (xf - mu) * rs
    gd = gam * dyf
    dx = rs * (gd - gd.mean(-1, keepdim=True) - xh * (gd * xh).mean(-1, keepdim=True))
    for s in (skip, skip2):
        if s is not None:
            dx = dx + s.float()
    return dx.to(x.dtype), dg0 + (dyf * xh).sum(0), db0 + dyf.sum(0)


def ln_bwd_operands(M, K, dtype, seed=2):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, K, generator=g) * 1.5 + 0.4).to(dtype)
    dy = (torch.randn(M, K, generator=g) * 0.5).to(dtype)
    sk, sk2 = torch.randn(M, K, generator=g).to(dtype), torch.randn(M, K, generator=g).to(dtype)
    gam = torch.rand(K, generator=g) + 0.5
    return x, dy, sk, sk2, gam, torch.randn(K, generator=g), torch.randn(K, generator=g)


@pytest.mark.parametrize('dtype', [F32, BF16])
@pytest.mark.parametrize('M,K', [(1, 24), (7, 260), (129, 516), (129, 1024), (4100, 24)])
def test_emulated_layernorm_passes(dtype, M, K):
    x, dy, sk, sk2, gam, dg0, db0 = ln_bwd_operands(M, K, dtype)
    for s, s2 in ((None, None), (sk, None), (None, sk2), (sk, sk2)):
        r = gb.ln_bwd_ref(x, dy, gam, s, s2, dg0, db0)
        dx, dg, db = emulate_ln_bwd(x, dy, gam, s, s2, dg0, db0)
        assert gb.check('dx', dx, r['dx'], r['e_dx']) <= 1.0
        assert gb.check('dgamma', dg, r['dgamma'], r['e_dgamma']) <= 1.0
        assert gb.check('dbeta', db, r['dbeta'], r['e_dbeta']) <= 1.0
    mean, e_mean, rstd, e_rstd = gb.ln_stats_ref(x, 1e-5)
    xf = x.float()
    mu = xf.mean(-1)
    assert gb.check('mean', mu, mean, e_mean) <= 1.0
    assert gb.check('rstd', ((xf - mu[:, None]).pow(2).mean(-1) + 1e-5).rsqrt(), rstd, e_rstd) <= 1.0


# ------------------------------------------------------------------------------------------ seeded wrong results must fail

def fails_at(name, got, ref, e, where):
    with pytest.raises(gb.BoundError) as info:
        gb.check(name, got, ref, e)
    m = re.search(r'worst at \(([^)]*)\)', str(info.value))
    assert m is not None, str(info.value)
    idx = tuple(int(s) for s in m.group(1).split(',') if s.strip())
    assert idx in where, f'{name}: named {idx}, seeded {sorted(where)[:4]}: {info.value}'


@pytest.mark.parametrize('dtype', [F32, BF16, F16])
@pytest.mark.parametrize('M,N,K', [(130, 136, 72), (130, 136, 1024), (1300, 3720, 72)])
def test_seeded_forward_errors_fail(dtype, M, N, K):
    a, w, bias, res, gam, bet = operands(M, N, K, dtype, seed=3)
    r = gb.linear_ref(a, w, bias=bias)
    good = emulate_linear(a, w, bias=bias)
    assert gb.check('good', good, r['ref'], r['e_in']) <= 1.0
    # one 8-element K-chunk dropped from one output of the last row
    bad = good.clone()
    n = N // 2
    bad[M - 1, n] = (good[M - 1, n].float() - (a[M - 1, K - 8:].float() * w[n, K - 8:].float()).sum()).to(dtype)
    fails_at('chunk', bad, r['ref'], r['e_in'], {(M - 1, n)})
    # the bias missing on the last partial column chunk
    bad = good.clone()
    c0 = N // 8 * 8 if N % 8 else N - 8
    bad[:, c0:] = emulate_linear(a, w[c0:])
    fails_at('bias', bad, r['ref'], r['e_in'], {(m, c) for m in range(M) for c in range(c0, N)})
    # two rows swapped inside the last row tile
    bad = good.clone()
    r0 = (M - 1) // 64 * 64
    bad[[r0, M - 1]] = good[[M - 1, r0]]
    fails_at('rows', bad, r['ref'], r['e_in'], {(m, c) for m in (r0, M - 1) for c in range(N)})
    # a stale value in column N - 1
    bad = good.clone()
    bad[M // 2, N - 1] = good[M // 2 - 1, N - 1]
    fails_at('stale', bad, r['ref'], r['e_in'], {(M // 2, N - 1)})


@pytest.mark.parametrize('dtype', [F32, BF16])
def test_seeded_backward_errors_fail(dtype):
    M, K = 129, 260
    x, dy, sk, sk2, gam, dg0, db0 = ln_bwd_operands(M, K, dtype)
    r = gb.ln_bwd_ref(x, dy, gam, sk, sk2, dg0, db0)
    dx, dg, db = emulate_ln_bwd(x, dy, gam, sk, sk2, dg0, db0)
    assert gb.check('dx', dx, r['dx'], r['e_dx']) <= 1.0
    # skip2 ignored
    with pytest.raises(gb.BoundError):
        gb.check('dx', emulate_ln_bwd(x, dy, gam, sk, None, dg0, db0)[0], r['dx'], r['e_dx'])
    # skip forgotten on the last row only
    bad = dx.clone()
    bad[M - 1] = emulate_ln_bwd(x[M - 1:], dy[M - 1:], gam, None, sk2[M - 1:], dg0, db0)[0][0]
    fails_at('dx', bad, r['dx'], r['e_dx'], {(M - 1, k) for k in range(K)})
    # dgamma / dbeta missing one row's contribution
    dx1, dg1, db1 = emulate_ln_bwd(x[:-1], dy[:-1], gam, None, None, dg0, db0)
    with pytest.raises(gb.BoundError):
        gb.check('dgamma', dg1, r['dgamma'], r['e_dgamma'])
    with pytest.raises(gb.BoundError):
        gb.check('dbeta', db1, r['dbeta'], r['e_dbeta'])
    # overwrite treated as accumulate
    N = 56
    dc = (torch.randn(M, N) * 0.3).to(dtype)
    dw0 = torch.randn(N, K)
    dw, e, _, _ = gb.wgrad_ref(dc, x, None, None)
    assert gb.check('dw', dc.float().t() @ x.float(), dw, e) <= 1.0
    with pytest.raises(gb.BoundError):
        gb.check('dw', dw0 + dc.float().t() @ x.float(), dw, e)


@pytest.mark.parametrize('dtype', [F32, BF16, F16])
def test_sentinel_frame(dtype):
    buf, out, mask = gb.framed(5, 12, dtype, ld=29)
    assert out.shape == (5, 12) and out.stride(0) == 29 and int(mask.sum()) == 60
    out.copy_(torch.randn(5, 12).to(dtype))
    gb.assert_untouched(buf, mask)
    for where in ((0, 7), (2, 20), (4, 28), (5, 8), (7, 0)):        # left of, right of and below the output
        b2 = buf.clone()
        b2[where] = 0.0
        with pytest.raises(gb.BoundError, match=re.escape(str(where))):
            gb.assert_untouched(b2, mask)
    # an output element the kernel never wrote still holds the sentinel: the checker refuses it
    buf, out, mask = gb.framed(5, 12, dtype)
    ref = torch.zeros(5, 12, dtype=torch.float64)
    out.zero_()
    assert gb.check('written', out, ref, ref + 1e-6) == 0.0
    buf2, out2, _ = gb.framed(5, 12, dtype)
    fails_at('unwritten', out2, ref, ref + 1e-6, {(m, c) for m in range(5) for c in range(12)})
