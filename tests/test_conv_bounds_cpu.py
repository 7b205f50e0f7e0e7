"""tests/conv_bounds.py without a GPU: an fp32 torch emulation of a correct convolution kernel (operands rounded to the operand
type, fp32 accumulation, fp32 epilogue, one rounding to the output type) passes every bound with no element left out at every
shape tests/test_conv_family_gpu.py runs; seeded wrong results -- the mistakes a halo, a tile edge, a channel pass or a crop
makes -- fail, with the wrong element named.  The [bound] lines are the figures of profiles/conv_family_bounds/README.md."""
import re

import pytest
import torch
import torch.nn.functional as F

import conv_bounds as cb
import gemm_bounds as gb

F32, BF16, F16 = cb.F32, cb.BF16, cb.F16
SLOPE = 0.01


# ------------------------------------------------------------------------------------------------ the emulated kernels

def conv32(x, w_op, k, stride, pad):
    """fp32 convolution of NHWC values (already exact in fp32) -> NHWC fp32"""
    Cout, Cin = w_op.shape[0], x.shape[-1]
    w4 = w_op.float().view(Cout, k, k, Cin).permute(0, 3, 1, 2)
    return F.conv2d(x.float().permute(0, 3, 1, 2), w4, None, stride=stride, padding=pad).permute(0, 2, 3, 1).contiguous()


def prologue32(x, sc, sh, dtype):
    """round_op(LeakyReLU(fma(x, sc, sh))) in fp32 (the fma as one rounding of the fp64 value)"""
    y = (x.double() * sc.double() + sh.double()).float()
    return torch.where(y > 0, y, y * torch.tensor(SLOPE, dtype=F32)).to(dtype)


def epilogue32(v, bias=None, scale=None, shift=None, residual=None, leaky=False):
    if bias is not None:
        v = v + bias
    if scale is not None:
        v = v * scale + shift
    if residual is not None:
        v = v + residual.float()
    if leaky:
        v = torch.where(v > 0, v, v * torch.tensor(SLOPE, dtype=F32))
    return v


def stats32(y, drop_last=False):
    """[REPLICAS, C] fp32 partial sums of the stored output, rows dealt round-robin to the replicas"""
    Y = y.float().reshape(-1, y.shape[-1])
    if drop_last:
        Y = Y[:-1]
    return (torch.stack([Y[r::cb.REPLICAS].sum(0) for r in range(cb.REPLICAS)]),
            torch.stack([(Y[r::cb.REPLICAS] * Y[r::cb.REPLICAS]).sum(0) for r in range(cb.REPLICAS)]))


def bn_fold32(s, q, count, gamma, beta, eps):
    """csrc/bn_lazy.h bn_channel, operation by operation, in fp32"""
    n = torch.tensor(float(count), dtype=F32)
    s1, s2 = s[0].clone(), q[0].clone()
    for r in range(1, s.shape[0]):
        s1, s2 = s1 + s[r], s2 + q[r]
    mean = s1 / n
    var = (s2 / n - mean * mean).clamp_min(0)
    rs = (var + torch.tensor(eps, dtype=F32)).rsqrt()
    return gamma * rs, beta - mean * gamma * rs


def emulated(case, dtype, o, a_op=None):
    """run() of conv_bounds.forward_case on the emulation.  a_op: the prologue's result in the operand type."""
    k, stride, pad = case[5:8]
    base = conv32(o['x'] if a_op is None else a_op, o['w'], k, stride, pad)

    def run(kw, stats):
        y = epilogue32(base, **kw).to(dtype)
        s, q = stats32(y) if stats else (None, None)
        return y, s, q
    return run


def prologue_of(case, dtype, o):
    """-> (A', (A fp64, e_A)) of a case's input prologue, statistics emulated for the raw form; (None, None) without one."""
    kind = case[8]
    if kind is None:
        return None, None
    if kind == 'affine':
        sc, sh, e_sc, e_sh = o['in_scale'], o['in_shift'], None, None
    else:
        s, q = stats32(o['x'])
        count = o['x'].numel() // o['x'].shape[-1]
        sc, sh = bn_fold32(s, q, count, o['gamma'], o['beta'], 1e-5)
        f = cb.bn_fold_ref(s, q, count, o['gamma'], o['beta'], 1e-5)
        print(f'[bound] emulated bn fold: scale={gb.check("bn.scale", sc, f["scale"], f["e_scale"]):.3f} '
              f'shift={gb.check("bn.shift", sh, f["shift"], f["e_shift"]):.3f}')
        # the reference prologue starts from the EXACT scale / shift of the received sums and carries their fp32 error
        return prologue32(o['x'], sc, sh, dtype), cb.prologue(o['x'], f['scale'], f['shift'], SLOPE, dtype, f['e_scale'], f['e_shift'])
    return prologue32(o['x'], sc, sh, dtype), cb.prologue(o['x'], sc, sh, SLOPE, dtype, e_sc, e_sh)


# ------------------------------------------------------------------------------------------------ the emulation passes

FWD = ([('gemm', c, dt) for c in cb.GEMM_CASES for dt in (F32, BF16)]
       + [('direct', c, dt) for c in cb.DIRECT_CASES for dt in (BF16, F16)]
       + [('point', c, dt) for c in cb.POINT_CASES + cb.POINT_PERSISTENT for dt in (BF16, F16)])


@pytest.mark.parametrize('fam,case,dtype', FWD, ids=[f'{f}-{cb.NAMES[d]}-{cb.case_id(c)}' for f, c, d in FWD])
def test_emulated_forward_passes_with_nothing_left_out(fam, case, dtype):
    o = cb.fwd_operands(case, dtype, seed=5)
    a_op, pre = prologue_of(case, dtype, o)
    only = ('bias+leaky+stats', 'bias+affine') if case in cb.POINT_PERSISTENT else None
    worst = cb.forward_case(case, dtype, o, emulated(case, dtype, o, a_op), residual=fam != 'point', pre=pre, only=only)
    cb.report(f'emulated {fam} {cb.NAMES[dtype]} {cb.case_id(case)}', worst)


def test_every_direct_instantiation_is_in_the_case_list():
    want = {(dt, ncb, tw, npass, 1) for dt in (BF16, F16) for ncb in (1, 2, 4) for tw in (32, 16) for npass in (1, 2)} \
        | {(dt, 4, 16, npass, 2) for dt in (BF16, F16) for npass in (1, 2)}
    got = {(dt,) + cb.direct_instantiation(c) for c in cb.DIRECT_CASES for dt in (BF16, F16)}
    assert got == want and len(got) == 28


def test_persistent_cases_give_some_wave_a_second_run():
    for c in cb.POINT_PERSISTENT:
        runs, waves = cb.point_runs(c)
        assert waves == 2048 and runs > waves, (c, runs, waves)
    assert [cb.point_runs(c)[0] for c in cb.POINT_PERSISTENT] == [2049, 2052]
    assert cb.point_runs(cb.POINT_CASES[0]) == (1, 4)


DG = [(c, dt) for c in cb.DGRAD_CASES for dt in (F32, BF16)]


@pytest.mark.parametrize('case,dtype', DG, ids=[f'{cb.NAMES[d]}-{cb.case_id(c)}' for c, d in DG])
def test_emulated_data_gradient_passes_and_equals_autograd(case, dtype):
    B, Hi, Wi, ci, co, k, stride, pad = case
    g = torch.Generator().manual_seed(6)
    Ho, Wo = cb.out_hw(Hi, Wi, k, stride, pad)
    weight = (torch.randn(co, ci, k, k, generator=g) / (k * k * co) ** 0.5).to(dtype)
    dy = F.pad((torch.randn(B, Ho, Wo, co, generator=g) * 0.5 + 0.1), (0, -co % 8)).to(dtype)
    dskip = torch.randn(B, Hi, Wi, ci + -ci % 8, generator=g).to(dtype)
    wt = cb.flipped_operand(weight, dtype)
    auto = cb.dgrad_autograd64(dy, weight, stride, pad, Hi, Wi)
    Hz, Wz = cb.dgrad_plane(Hi, Wi, Ho, Wo, k, stride, pad)
    dz = cb.dilate_ref(dy, Hz, Wz, stride) if stride > 1 else dy
    worst = {}
    for tag, sk in (('plain', None), ('dskip', dskip)):
        r = cb.dgrad_ref(dy, wt, k, stride, pad, Hi, Wi, sk)
        want = auto + (0 if sk is None else sk.double())
        assert float((r['ref'] - want).abs().max()) <= 1e-12 * float(want.abs().max()), 'the data-gradient reference is not autograd\'s'
        got = epilogue32(conv32(dz, wt, k, 1, k - 1 - pad), residual=sk).to(dtype)
        worst[tag] = gb.check(tag, got, r['ref'], r['e_in'])
    cb.report(f'emulated dgrad {cb.NAMES[dtype]} {cb.case_id(case)}', worst)


def wgrad32(o, case, dw0=None, db0=None, times=1):
    """dy^T im2col(x) by fp32 autograd of the fp32 convolution, added `times` times"""
    B, H, W, Cin, Cout, k, stride, pad = case
    w = torch.zeros(Cout, Cin, k, k, requires_grad=True)
    b = torch.zeros(Cout, requires_grad=True)
    y = F.conv2d(o['x'].float().permute(0, 3, 1, 2), w, b, stride=stride, padding=pad)
    (y * o['dy'].float().permute(0, 3, 1, 2)).sum().backward()
    g, gbias = cb.gemm_layout(w.grad), b.grad
    dw = torch.zeros_like(g) if dw0 is None else dw0.clone()
    db = torch.zeros_like(gbias) if db0 is None else db0.clone()
    for _ in range(times):
        dw, db = dw + g, db + gbias
    return dw, db


WG = [(c, dt) for c in cb.WGRAD_IMPLICIT for dt in (F32, BF16)] + [(c, BF16) for c in cb.WGRAD_DIRECT]


@pytest.mark.parametrize('case,dtype', WG, ids=[f'{cb.NAMES[d]}-{cb.case_id(c)}' for c, d in WG])
def test_emulated_weight_gradient_passes(case, dtype):
    B, H, W, Cin, Cout, k, stride, pad = case
    o = cb.wgrad_operands(case, dtype, seed=7)
    co, ci = cb.crop(Cout, Cin)
    worst = {}
    for tag, dw0, db0, times in (('overwrite', None, None, 1), ('accumulate', o['dw0'], o['db0'], 1), ('twice', o['dw0'], o['db0'], 2)):
        rw, ew, rb, eb = cb.conv_wgrad_ref(o['x'], o['dy'], k, k, stride, pad, dw0, db0, times)
        dw, db = wgrad32(o, case, dw0, db0, times)
        worst[tag] = gb.check(tag, dw, rw, ew)
        worst[tag + '.b'] = gb.check(tag + '.dbias', db, rb, eb)
        if times == 2:          # the nn.Conv2d layout, cropped
            worst['layout'] = gb.check('layout', cb.conv_layout(dw, k, k, co, ci), cb.conv_layout(rw, k, k, co, ci), cb.conv_layout(ew, k, k, co, ci))
    cb.report(f'emulated wgrad {cb.NAMES[dtype]} {cb.case_id(case)}', worst)


def test_weight_gradient_reference_is_the_im2col_product():
    """conv_wgrad_ref's dy^T im2col(x) against an explicit unfold, on the stride-2 geometry with an unused last input row"""
    case = (1, 16, 16, 24, 16, 3, 2, 1)
    B, H, W, Cin, Cout, k, stride, pad = case
    o = cb.wgrad_operands(case, F32, seed=8)
    cols = F.unfold(o['x'].double().permute(0, 3, 1, 2), k, padding=pad, stride=stride)            # [B, Cin k k, L]
    cols = cols.view(B, Cin, k * k, -1).permute(0, 3, 2, 1).reshape(-1, k * k * Cin)               # [M, k k Cin] tap-major
    want = o['dy'].double().reshape(-1, Cout).t() @ cols
    rw, ew, rb, eb = cb.conv_wgrad_ref(o['x'], o['dy'], k, k, stride, pad)
    assert float((rw - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert float((rb - o['dy'].double().reshape(-1, Cout).sum(0)).abs().max()) <= 1e-12


# ------------------------------------------------------------------------------------------------ seeded wrong results must fail

def fails_at(name, got, ref, e, where):
    with pytest.raises(gb.BoundError) as info:
        gb.check(name, got, ref, e)
    m = re.search(r'worst at \(([^)]*)\)', str(info.value))
    assert m is not None, str(info.value)
    idx = tuple(int(s) for s in m.group(1).split(',') if s.strip())
    assert idx in where, f'{name}: named {idx}, seeded {sorted(where)[:4]}: {info.value}'


def tap_sum(o, b, hi, wi, tap, c0, c1):
    """[Cout]: what channels c0..c1 of input pixel (b, hi, wi) add through tap `tap` (fp32)"""
    Cin = o['x'].shape[-1]
    return o['w'].float()[:, tap * Cin + c0:tap * Cin + c1] @ o['x'].float()[b, hi, wi, c0:c1]


@pytest.mark.parametrize('dtype', [F32, BF16, F16])
@pytest.mark.parametrize('case', [(2, 9, 11, 8, 136, 3, 1, 1, None), (3, 16, 64, 128, 128, 3, 1, 1, None)], ids=cb.case_id)
def test_seeded_forward_errors_fail(case, dtype):
    B, H, W, Cin, Cout, k, stride, pad = case[:8]
    o = cb.fwd_operands(case, dtype, seed=9)
    kw = dict(bias=o['bias'], residual=o['residual'], leaky=True)
    r = cb.conv_fwd_ref(o['x'], o['w'], k, k, stride, pad, **kw)
    base = conv32(o['x'], o['w'], k, stride, pad)
    good = epilogue32(base, **kw).to(dtype)
    assert gb.check('good', good, r['ref'], r['e_in']) <= 1.0
    every = range(Cout)

    def with_base(b2):
        return epilogue32(b2, **kw).to(dtype)

    # one tap dropped at a corner pixel: output (0, 0, 0) loses tap (2, 2) = input pixel (1, 1)
    b2 = base.clone()
    b2[0, 0, 0] -= tap_sum(o, 0, 1, 1, 8, 0, Cin)
    fails_at('tap', with_base(b2), r['ref'], r['e_in'], {(0, 0, 0, c) for c in every})
    # the halo row below image 0 taken from image 1 (its first row) instead of the zero padding
    xp = F.pad(o['x'].float(), (0, 0, 1, 1, 1, 1))
    xp[0, H + 1, 1:W + 1] = o['x'].float()[1, 0]
    b2 = base.clone()
    b2[0, H - 1] = conv32(xp[:1], o['w'], k, 1, 0)[0, H - 1]
    fails_at('halo', with_base(b2), r['ref'], r['e_in'], {(0, H - 1, x, c) for x in range(W) for c in every})
    # the bias missing on the last 8 output channels
    bad = good.clone()
    bad[..., Cout - 8:] = epilogue32(base, residual=o['residual'], leaky=True).to(dtype)[..., Cout - 8:]
    fails_at('bias', bad, r['ref'], r['e_in'], {(b, y, x, c) for b in range(B) for y in range(H) for x in range(W) for c in range(Cout - 8, Cout)})
    # the residual skipped on the last pixel
    bad = good.clone()
    bad[B - 1, H - 1, W - 1] = epilogue32(base, bias=o['bias'], leaky=True).to(dtype)[B - 1, H - 1, W - 1]
    fails_at('residual', bad, r['ref'], r['e_in'], {(B - 1, H - 1, W - 1, c) for c in every})
    if Cin == 128:
        # one 8-channel chunk of the second channel pass dropped: channels 72..79 of the centre tap at one pixel
        b2 = base.clone()
        b2[1, 3, 5] -= tap_sum(o, 1, 3, 5, 4, 72, 80)
        fails_at('chunk', with_base(b2), r['ref'], r['e_in'], {(1, 3, 5, c) for c in every})
    # the statistics missing the last pixel
    rs, es, rq, eq = cb.stats_ref(good)
    s, q = stats32(good)
    assert gb.check('sum', cb.stats_got(s), rs, es) <= 1.0 and gb.check('sq', cb.stats_got(q), rq, eq) <= 1.0
    s, q = stats32(good, drop_last=True)
    fails_at('sum', cb.stats_got(s), rs, es, {(c,) for c in every})
    fails_at('sq', cb.stats_got(q), rq, eq, {(c,) for c in every})


@pytest.mark.parametrize('case,dtype', [((2, 9, 11, 8, 40, 3, 1, 1), F32), ((2, 9, 11, 8, 40, 3, 1, 1), BF16),
                                        ((1, 16, 32, 64, 128, 3, 1, 1), BF16)], ids=lambda v: cb.case_id(v) if isinstance(v, tuple) else cb.NAMES[v])
def test_seeded_weight_gradient_errors_fail(case, dtype):
    B, H, W, Cin, Cout, k, stride, pad = case
    o = cb.wgrad_operands(case, dtype, seed=10)
    rw, ew, rb, eb = cb.conv_wgrad_ref(o['x'], o['dy'], k, k, stride, pad, o['dw0'], o['db0'])
    dw, db = wgrad32(o, case, o['dw0'], o['db0'])
    assert gb.check('dw', dw, rw, ew) <= 1.0 and gb.check('db', db, rb, eb) <= 1.0
    # one border pixel missing from one tap: output pixel (0, H - 1, W - 1) through tap (0, 0) = input pixel (H - 2, W - 2)
    bad = dw.clone()
    bad[:, :Cin] -= torch.outer(o['dy'].float()[0, H - 1, W - 1], o['x'].float()[0, H - 2, W - 2])
    fails_at('border', bad, rw, ew, {(n, c) for n in range(Cout) for c in range(Cin)})
    # accumulate treated as overwrite
    over, ob = wgrad32(o, case)
    fails_at('overwrite', over, rw, ew, {(n, c) for n in range(Cout) for c in range(k * k * Cin)})
    fails_at('overwrite.b', ob, rb, eb, {(n,) for n in range(Cout)})
    # the channel crop of the nn.Conv2d layout off by one input channel
    co, ci = cb.crop(Cout, Cin)
    lay = lambda t: cb.conv_layout(t, k, k, co, ci)
    assert gb.check('layout', lay(dw), lay(rw), lay(ew)) <= 1.0
    shifted = dw.view(Cout, k, k, Cin)[:co, :, :, 1:ci + 1].permute(0, 3, 1, 2).contiguous()
    fails_at('crop', shifted, lay(rw), lay(ew), {(n, c, a, b) for n in range(co) for c in range(ci) for a in range(k) for b in range(k)})


@pytest.mark.parametrize('dtype', [F32, BF16, F16])
def test_an_element_written_in_front_of_an_output_fails(dtype):
    buf, out, mask = gb.framed_flat((2, 4, 5, 8), dtype)
    out.copy_(torch.randn(2, 4, 5, 8).to(dtype))
    gb.assert_untouched(buf, mask)
    for where in (63, 64 + 320):
        b2 = buf.clone()
        b2[where] = 0.0
        with pytest.raises(gb.BoundError, match=re.escape(f'first at ({where},)')):
            gb.assert_untouched(b2, mask)


def test_dilate_reference():
    dy = torch.arange(2 * 3 * 4 * 8, dtype=F32).reshape(2, 3, 4, 8) + 1
    dz = cb.dilate_ref(dy, 6, 7, 2)
    assert torch.equal(dz[:, 0:5:2, 0:7:2], dy) and float(dz.sum()) == float(dy.sum()) and not bool(dz[:, 5].any()) and not bool(dz[:, :, 1::2].any())
