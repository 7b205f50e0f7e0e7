"""GPU: the kernels at the two ends of the denoiser's training step -- token corruption, token + position embedding forward and
backward, cross-entropy, the gradient norm and AdamW -- on every route, each output element against the fp64 references and
bounds of tests/tail_bounds.py (the corruption and the embedding forward: exactly), every output inside a sentinel frame, input
padding filled with NaN.  The C entry points are called through _lib.call, so the route is the one the test names; where a Python
wrapper chooses, recorded_calls says which.  profiles/train_tail_bounds/README.md holds the derivations and the measured room."""
import functools

import pytest
import torch

import tail_bounds as tb
from conftest import recorded_calls

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
NAMES = {F32: 'f32', BF16: 'bf16'}
NAN = float('nan')


@pytest.fixture(scope='module')
def L():
    assert torch.cuda.is_available()
    from world_modelz_amd import _lib
    _lib.lib()
    return _lib


def dev(t):
    return None if t is None else t.cuda()


def report(tag, worst):
    print(f'[tail] {tag}: worst |got - ref| / tol = {worst:.3f}')
    return worst


def flat(shape, dtype, fill=None, pad=64):
    """A framed contiguous device buffer (tb.framed_flat), optionally holding `fill` -> (buf, view, mask)."""
    buf, view, mask = tb.framed_flat(tuple(shape), dtype, 'cuda', pad=pad)
    if fill is not None:
        view.copy_(fill.to(dtype))
    return buf, view, mask


def nan_padded(x, ld=None, rows_after=2, offset=0):
    """x [R, C] on the device inside a NaN-filled buffer: row stride ld, `rows_after` NaN rows behind, the base `offset` elements
    into the allocation -> the [R, C] view (its data_ptr is the base the kernel gets)."""
    R, C = x.shape
    ld = C if ld is None else ld
    buf = torch.full(((R + rows_after) * ld + offset + 8,), NAN, dtype=x.dtype, device='cuda')
    view = buf[offset:offset + R * ld].view(R, ld)[:, :C]
    view.copy_(x)
    return view


# ---------------------------------------------------------------------------------------------------- cross-entropy

def run_ce(L, x, t, g, dtype, ld=None, route='fwd_bwd', in_off=0, out_off=0, lse_in=None):
    """One cross-entropy route on framed outputs -> dict(loss, lse, d) on the CPU (what the route does not write: None).
    route: 'fwd_bwd' (wmz_ce_fwd_bwd), 'fwd' (wmz_ce_fwd), 'bwd' (wmz_ce_bwd on lse_in), 'two' (wmz_ce_fwd, then wmz_ce_bwd on its lse)."""
    R, C = x.shape
    xv = nan_padded(x, ld, offset=in_off)
    ldx = xv.stride(0)
    td, gd = dev(t), dev(g)
    frames = []
    out = dict(loss=None, lse=None, d=None)

    def framed_out(shape, dt, pad=64):
        buf, view, mask = flat(shape, dt, pad=pad)
        frames.append((buf, mask))
        return view
    if route != 'bwd':
        lo, ls = framed_out((R,), F32), framed_out((R,), F32)
    if route != 'fwd':
        d = framed_out((R, C), dtype, pad=64 + out_off)
    code = L.dtype_code(dtype)
    if route == 'fwd_bwd':
        L.call('wmz_ce_fwd_bwd', L.ptr(xv), ldx, L.ptr(td), L.ptr(lo), L.ptr(ls), L.ptr(gd), L.ptr(d), R, C, code, L.stream())
    if route in ('fwd', 'two'):
        L.call('wmz_ce_fwd', L.ptr(xv), ldx, L.ptr(td), L.ptr(lo), L.ptr(ls), R, C, L.stream())
    if route in ('bwd', 'two'):
        lsd = ls if route == 'two' else dev(lse_in)
        L.call('wmz_ce_bwd', L.ptr(xv), ldx, L.ptr(td), L.ptr(lsd), L.ptr(gd), L.ptr(d), R, C, code, L.stream())
    torch.cuda.synchronize()
    for buf, mask in frames:
        tb.assert_untouched(buf, mask)
    if route != 'bwd':
        out.update(loss=lo.cpu(), lse=ls.cpu())
    if route != 'fwd':
        out.update(d=d.cpu())
    return out


def check_ce(tag, got, r):
    w = [0.0]
    for k, rk in (('loss', 'loss'), ('lse', 'lse'), ('d', 'dlogits')):
        if got[k] is not None:
            w.append(tb.check(f'{tag} {k}', got[k], r[rk], r['e_' + rk]))
    return max(w)


def one_pass(C, ld):
    """Whether wmz_ce_fwd_bwd takes ce_fused_kernel for aligned bases (include/wmz.h)."""
    return C <= 8192 and ld % 4 == 0


def ce_all_routes(L, x, t, g, dtype, ld, tag):
    """The three entry points on one input: each within its bound of fp64, wmz_ce_fwd_bwd == the two launches bit for bit where it
    IS the two launches, and its gradient == wmz_ce_bwd on its own lse bit for bit where it is the one-pass kernel: both evaluate
    (__expf(x - l) - one_hot) * g on the same l.  (Their forward halves do not share arithmetic: ce_fwd_kernel adds a lane's classes
    c, c + 64, .., ce_fused_kernel four consecutive classes per lane and float4: another summation order, so loss and lse agree within
    the bounds only.)"""
    C = x.shape[1]
    r = tb.ce_ref(x, t, g)
    fused = run_ce(L, x, t, g, dtype, ld, 'fwd_bwd')
    two = run_ce(L, x, t, g, dtype, ld, 'two')
    worst = {'fwd_bwd': check_ce(tag + ' fwd_bwd', fused, r),
             'fwd': check_ce(tag + ' fwd', dict(two, d=None), r),
             'bwd': tb.check(tag + ' bwd d', two['d'], *[tb.ce_ref(x, t, g, lse=two['lse'])[k] for k in ('dlogits', 'e_dlogits')])}
    if one_pass(C, ld):
        again = run_ce(L, x, t, g, dtype, ld, 'bwd', lse_in=fused['lse'])
        assert torch.equal(again['d'].view(torch.uint8), fused['d'].view(torch.uint8)), f'{tag}: one-pass gradient != wmz_ce_bwd on its lse'
    else:
        for k in ('loss', 'lse', 'd'):
            assert torch.equal(fused[k].view(torch.uint8), two[k].view(torch.uint8)), f'{tag}: {k} is not the two launches\' result'
    return r, fused, two, worst


@pytest.mark.parametrize('dtype', [F32, BF16], ids=NAMES.get)
@pytest.mark.parametrize('C', tb.CE_CLASSES)
def test_cross_entropy_every_class_count(L, C, dtype):
    """Every NCH boundary of the one-pass kernel, C % 4 != 0 with an aligned stride (its scalar store path), ld = C (the two launches
    when C % 4 != 0) and a padded stride; targets 0, C-1, -1, C and 2^32 + 1 on the first rows."""
    x, t, g = tb.ce_case(tb.ce_rows(C), C)
    for ld in (C, (C + 3) // 4 * 4 + 4):
        _, _, _, worst = ce_all_routes(L, x, t, g, dtype, ld, f'ce C={C} ld={ld} {NAMES[dtype]}')
        for k, v in worst.items():
            report(f'ce_{k} C={C} ld={ld} {NAMES[dtype]} ({"one pass" if one_pass(C, ld) else "two launches"})', v)


@pytest.mark.parametrize('dtype', [F32, BF16], ids=NAMES.get)
@pytest.mark.parametrize('how', ['odd_ld', 'offset_logits', 'offset_dlogits'])
def test_cross_entropy_unaligned_rows_take_the_two_launches(L, how, dtype):
    """An odd row stride, a logits base 4 bytes off a 16-byte boundary, a gradient base half a vector store off: wmz_ce_fwd_bwd gives
    the two launches' results, bit for bit."""
    R, C = 9, 1024
    x, t, g = tb.ce_case(R, C)
    kw = dict(odd_ld=dict(ld=1027), offset_logits=dict(ld=1028, in_off=1), offset_dlogits=dict(ld=1028, out_off=2))[how]
    r = tb.ce_ref(x, t, g)
    got = run_ce(L, x, t, g, dtype, route='fwd_bwd', **kw)
    two = run_ce(L, x, t, g, dtype, ld=kw['ld'], route='two')
    report(f'ce_fwd_bwd {how} {NAMES[dtype]} (two launches)', check_ce(how, got, r))
    for k in ('loss', 'lse', 'd'):
        assert torch.equal(got[k].view(torch.uint8), two[k].view(torch.uint8)), k


@pytest.mark.parametrize('route,R', [('fwd', 8192 + 5), ('fwd_bwd', 16384 + 3), ('bwd', 1048576 // 12 + 7)])
def test_cross_entropy_row_sweeps(L, route, R):
    """Past each grid cap: 2 048 workgroups of 4 rows (wmz_ce_fwd), 4 096 of 4 rows (wmz_ce_fwd_bwd), 4 096 of 256 elements (wmz_ce_bwd)."""
    C = 12
    x, t, g = tb.ce_case(R, C)
    r = tb.ce_ref(x, t, g)
    lse_in = r['lse'].float() if route == 'bwd' else None
    got = run_ce(L, x, t, g, BF16 if route == 'bwd' else F32, ld=16, route=route, lse_in=lse_in)
    if route == 'bwd':
        r = tb.ce_ref(x, t, g, lse=lse_in)
    report(f'ce_{route} R={R} C={C} (row sweep)', check_ce(f'sweep {route}', got, r))


@pytest.mark.parametrize('regime', tb.CE_REGIMES)
@pytest.mark.parametrize('C', tb.CE_REGIME_CLASSES)
def test_cross_entropy_data_regimes(L, C, regime):
    """Peaked rows (p_target - 1 cancels: the bound is absolute there), a common shift of 1e4, equal logits, tied maxima, and the
    -1e30 padding classes of _LinearCrossEntropy, whose probability and gradient must be exactly 0."""
    x, t, g = tb.ce_case(9, C, regime)
    for dtype in (F32, BF16):
        _, fused, two, worst = ce_all_routes(L, x, t, g, dtype, (C + 3) // 4 * 4 + 4, f'ce {regime} C={C} {NAMES[dtype]}')
        report(f'ce {regime} C={C} {NAMES[dtype]}', max(worst.values()))
        if regime.startswith('pad'):
            k = int(regime[3:])
            assert not bool(fused['d'][:, C - k:].any()) and not bool(two['d'][:, C - k:].any())


# ---------------------------------------------------------------------------------------------------- AdamW and the norm

@functools.lru_cache(maxsize=2)
def adamw_case(n):
    return tb.adamw_case(n)


def adamw_state(p, m, v):
    """Framed device copies of the state the kernels update in place -> ([views], [(buf, mask)])."""
    fr = [flat((p.numel(),), F32, fill=t) for t in (p, m, v)]
    return [f[1] for f in fr], [(f[0], f[2]) for f in fr]


def adamw_hyper_tensor(lr, beta1, beta2, step):
    return torch.tensor([tb.f32(lr), tb.f32(1.0 - beta1 ** step), tb.f32((1.0 - beta2 ** step) ** 0.5)], device='cuda')


def tiled_ref(n, fn):
    """fn on the first min(n, ADAMW_PERIOD) elements, tiled to n (tb.adamw_case repeats with that period)."""
    k = min(n, tb.ADAMW_PERIOD)
    r = fn(k)
    return {key: tb.tile(val, n) for key, val in r.items()}


@pytest.mark.parametrize('step', [1, 2, 1000])
@pytest.mark.parametrize('gs', [1.0, 0.125])
@pytest.mark.parametrize('wd', [0.0, tb.f32(0.01)], ids=['wd0', 'wd0.01'])
@pytest.mark.parametrize('n', tb.ADAMW_N)
def test_adamw_and_norm(L, n, wd, gs, step):
    """wmz_adamw_step and wmz_adamw_step_dev: bit-identical, every element of p, m, v within its bound of the fp64 law; the norm that
    rides along is += onto a non-zero start and agrees with wmz_grad_sqnorm and with fp64.  n % 4 != 0, and both grid caps: 256
    workgroups with the norm (n = 2 * 524 288 + 6 147), 2 048 without (n = 4 194 304 + 2 051: that grid only)."""
    p, g, m, v = adamw_case(n)
    h = tb.ADAMW_HYPER
    with_norm = n <= 4194304
    gd = dev(g)
    (pa, ma, va), fa = adamw_state(p, m, v)
    (pb, mb, vb), fb = adamw_state(p, m, v)
    L.call('wmz_adamw_step', L.ptr(pa), L.ptr(gd), L.ptr(ma), L.ptr(va), n, h['lr'], h['beta1'], h['beta2'], h['eps'], wd, step, gs,
           L.stream())
    hyper = adamw_hyper_tensor(h['lr'], h['beta1'], h['beta2'], step)
    total = float((g.double() * gs).pow(2).sum())
    start = tb.f32(total / 2 + 1.0)                              # of the sum's own size: losing it would show
    sq_buf, sq, sq_mask = flat((1,), F32, fill=torch.tensor([start]))
    L.call('wmz_adamw_step_dev', L.ptr(pb), L.ptr(gd), L.ptr(mb), L.ptr(vb), n, L.ptr(hyper), h['beta1'], h['beta2'], h['eps'], wd, gs,
           L.ptr(sq) if with_norm else None, L.stream())
    n_buf, nsq, n_mask = flat((1,), F32, fill=torch.zeros(1))
    L.call('wmz_grad_sqnorm', L.ptr(gd), n, gs, L.ptr(nsq), L.stream())
    torch.cuda.synchronize()
    for buf, mask in fa + fb + [(sq_buf, sq_mask), (n_buf, n_mask)]:
        tb.assert_untouched(buf, mask)
    for name, a, b in (('p', pa, pb), ('m', ma, mb), ('v', va, vb)):
        assert torch.equal(a, b), f'{name}: wmz_adamw_step != wmz_adamw_step_dev'
    r = tiled_ref(n, lambda k: tb.adamw_ref(p[:k], g[:k], m[:k], v[:k], weight_decay=wd, step=step, grad_scale=gs, **h))
    worst = max(tb.check(f'adamw {k}', x.cpu(), r[k], r['e_' + k]) for k, x in zip('pmv', (pa, ma, va)))
    report(f'adamw_step n={n} wd={wd} gs={gs} t={step}', worst)
    ref0, e0 = tb.sqnorm_ref(g, gs)
    w_norm = tb.check('grad_sqnorm', nsq.cpu(), torch.tensor([ref0]), torch.tensor([e0]))
    if with_norm:
        ref1, e1 = tb.sqnorm_ref(g, gs, start=start)
        w_norm = max(w_norm, tb.check('adamw sqnorm_out', sq.cpu(), torch.tensor([ref1]), torch.tensor([e1])))
        tol = (e0 + tb.U32 * (ref0 + e0)) + (e1 + tb.U32 * (ref1 + e1))
        assert abs((float(sq) - start) - float(nsq)) <= tol + tb.U32 * start, (float(sq), start, float(nsq), tol)
    report(f'sqnorm n={n} gs={gs}', w_norm)


@pytest.mark.parametrize('first', [1, 1000])
def test_adamw_three_steps_against_torch(L, first):
    """Three successive steps, a new gradient each, against torch.optim.AdamW on fp64 CPU copies, the bound compounded."""
    n = 2049
    p, g, m, v = tb.adamw_case(n)
    grads = [g, tb.adamw_case(n, seed=1)[1], tb.adamw_case(n, seed=2)[1]]
    h = dict(tb.ADAMW_HYPER, weight_decay=tb.f32(0.01))
    gs = 0.125
    (pa, ma, va), fa = adamw_state(p, m, v)
    (pb, mb, vb), fb = adamw_state(p, m, v)
    for k, gk in enumerate(grads):
        gd = dev(gk)
        L.call('wmz_adamw_step', L.ptr(pa), L.ptr(gd), L.ptr(ma), L.ptr(va), n, h['lr'], h['beta1'], h['beta2'], h['eps'],
               h['weight_decay'], first + k, gs, L.stream())
        hyper = adamw_hyper_tensor(h['lr'], h['beta1'], h['beta2'], first + k)
        L.call('wmz_adamw_step_dev', L.ptr(pb), L.ptr(gd), L.ptr(mb), L.ptr(vb), n, L.ptr(hyper), h['beta1'], h['beta2'], h['eps'],
               h['weight_decay'], gs, None, L.stream())
        torch.cuda.synchronize()
    for buf, mask in fa + fb:
        tb.assert_untouched(buf, mask)
    assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb)
    P, e_p, M, e_m, V, e_v = tb.adamw_torch_steps(p, grads, m, v, first_step=first, grad_scale=gs, **h)
    report(f'adamw 3 steps from t={first} vs torch.optim.AdamW',
           max(tb.check('p', pa.cpu(), P, e_p), tb.check('m', ma.cpu(), M, e_m), tb.check('v', va.cpu(), V, e_v)))


# ---------------------------------------------------------------------------------------------------- corruption

def run_corrupt(L, z_clip, S, HW, r, C, seed, stream_id, with_target, counter=None, stream_hi=None):
    """wmz_corrupt_tokens (or _dev with counter) on the last of S frames of z_clip [B, S * HW] into frame 2 of a framed
    [B, out_stride] buffer with another stride -> (out [B, HW], target [B, HW] or None) on the CPU."""
    B = z_clip.shape[0]
    out_stride = 5 * HW + 3
    off = 2 * HW
    buf = torch.empty((B, out_stride), dtype=torch.int64, device='cuda')
    buf.view(torch.uint8).fill_(0x7E)
    mask = torch.zeros((B, out_stride), dtype=torch.bool)
    mask[:, off:off + HW] = True
    zd, rd = dev(z_clip), dev(r)
    z_last = zd[:, (S - 1) * HW:]
    out = buf[:, off:]
    tgt = flat((B * HW,), torch.int64) if with_target else None
    args = (L.ptr(z_last), S * HW, L.ptr(rd), L.ptr(out), out_stride, L.ptr(tgt[1]) if with_target else None, B, HW, C, seed)
    if counter is None:
        L.call('wmz_corrupt_tokens', *args, stream_id, L.stream())
    else:
        cd = torch.tensor([counter - (1 << 64) if counter >= 1 << 63 else counter], dtype=torch.int64, device='cuda')
        L.call('wmz_corrupt_tokens_dev', *args, stream_hi, L.ptr(cd), L.stream())
    torch.cuda.synchronize()
    tb.assert_untouched(buf, mask)
    if with_target:
        tb.assert_untouched(tgt[0], tgt[2])
    return buf[:, off:off + HW].cpu(), (tgt[1].cpu().view(B, HW) if with_target else None)


@pytest.mark.parametrize('with_target', [True, False], ids=['target', 'no-target'])
@pytest.mark.parametrize('C', [7, 8192])
def test_corruption_equals_the_reference_at_every_position(L, C, with_target):
    """Keyed by the flat index b * HW + p, read at clip_stride and written at out_stride; the other frames of out untouched."""
    B, HW, S = 3, 77, 4
    gen = torch.Generator().manual_seed(C)
    z = torch.randint(0, C, (B, S * HW), generator=gen)
    r = torch.tensor([0.0, 1.0, 0.37])
    seed, sid = 0x0123456789ABCDEF, (2 << 40) | 99
    out, tgt = run_corrupt(L, z, S, HW, r, C, seed, sid, with_target)
    want = tb.corrupt_ref(z[:, (S - 1) * HW:], r, C, seed, sid)
    assert torch.equal(out, want), (out != want).nonzero()[:5]
    assert torch.equal(out[0], z[0, (S - 1) * HW:]) and bool((out[1] == C).all())
    if with_target:
        assert torch.equal(tgt, z[:, (S - 1) * HW:])


def test_corruption_past_the_grid_cap_and_the_device_counter(L):
    """2 x 140 000 positions (more than 1 024 workgroups of 256); _dev with counter bits above 40 and low bits of stream_hi set
    equals the plain entry point at the composed stream id."""
    B, HW, S, C = 2, 140000, 1, 8192
    gen = torch.Generator().manual_seed(3)
    z = torch.randint(0, C, (B, S * HW), generator=gen)
    r = torch.tensor([0.37, 0.8])
    seed = 77
    counter, hi = (0xABC << 40) | 0x12345678, (5 << 40) | 0xFFFF
    sid = (5 << 40) | 0x12345678
    plain, _ = run_corrupt(L, z, S, HW, r, C, seed, sid, False)
    devd, tgt = run_corrupt(L, z, S, HW, r, C, seed, None, True, counter=counter, stream_hi=hi)
    want = tb.corrupt_ref(z, r, C, seed, sid)
    assert torch.equal(plain, want), (plain != want).nonzero()[:5]
    assert torch.equal(devd, want), (devd != want).nonzero()[:5]
    assert torch.equal(tgt, z)


# ---------------------------------------------------------------------------------------------------- embedding forward

def indexed_positions(ntok, S, H, W, gen):
    """Flat grid positions with repeats and two out of range (clamped to 0 / G - 1) -> (pos as given, clamped)."""
    G = S * H * W
    pos = torch.randint(0, G, (ntok,), generator=gen)
    pos[ntok // 3:ntok // 3 + 5] = pos[0]                       # repeated positions
    if ntok > 4:
        pos[1], pos[3] = -7, G + 11
    return pos, pos.clamp(0, G - 1)


def split_pos(pc, H, W):
    return pc // (H * W), (pc // W) % H, pc % W


@pytest.mark.parametrize('dtype', [F32, BF16], ids=NAMES.get)
@pytest.mark.parametrize('kind', ['pos3d', 'indexed'])
@pytest.mark.parametrize('shape,D', [((2, 3, 5, 7), 4), ((2, 3, 5, 7), 40), ((2, 3, 5, 7), 256), ((2, 3, 5, 7), 260), ((2, 9, 16, 16), 512)],
                         ids=['D4', 'D40', 'D256', 'D260', 'past-the-grid-cap'])
def test_embedding_forward_is_exact(L, kind, shape, D, dtype):
    """emb[tok] + ((pos_s + pos_h) + pos_w), three IEEE additions and one rounding: bit for bit.  Ids include the mask class and values
    out of range (clamped), the indexed form's positions too; 4 608 tokens x 512 is past the 2 048-workgroup cap."""
    B, S, H, W = shape
    ntok, classes = B * S * H * W, 11
    tok, _, tabs = tb.embed_case(ntok, D, classes, F32, rows=(S, H, W))
    tc = tok.clamp(0, classes - 1)
    if kind == 'pos3d':
        idx = tb.pos3d_indices(B, S, H, W)
    else:
        pos, pc = indexed_positions(ntok, S, H, W, torch.Generator().manual_seed(D))
        idx = split_pos(pc, H, W)
    x32, want = tb.embed_fwd_ref(tc, *idx, *tabs, dtype)
    buf, x, mask = flat((ntok, D), dtype)
    td, tokd = [dev(t) for t in tabs], dev(tok)
    if kind == 'pos3d':
        L.call('wmz_embed_pos3d_fwd', L.ptr(tokd), *[L.ptr(t) for t in td], L.ptr(x), B, S, H, W, D, classes, L.dtype_code(dtype),
               L.stream())
    else:
        posd = dev(pos)
        L.call('wmz_embed_indexed_fwd', L.ptr(tokd), L.ptr(posd), *[L.ptr(t) for t in td], L.ptr(x), ntok, S, H, W, D, classes,
               L.dtype_code(dtype), L.stream())
    torch.cuda.synchronize()
    tb.assert_untouched(buf, mask)
    tb.check(f'embed_{kind}_fwd', x.cpu(), x32, torch.zeros_like(x32))
    assert torch.equal(x.cpu().view(torch.uint8), want.view(torch.uint8))


# ---------------------------------------------------------------------------------------------------- embedding backward

def pos3d_bwd_kernel(W, D):
    """White box (csrc/capi_core.hip, wmz_embed_pos3d_bwd): which kernel the scatter entry point launches.  The W == 16 kernel reads
    the plane row's ids from lanes 0..15 of every working wave, so it is taken only where D % 64 is 0 or at least 16."""
    return 'embed_pos3d_bwd16_kernel' if W == 16 and (D % 64 == 0 or D % 64 >= 16) else 'embed_pos3d_bwd_kernel'


def nan_rows_after(dx):
    """dx [ntok, D] on the device with two NaN rows behind it."""
    buf = torch.full((dx.shape[0] + 2, dx.shape[1]), NAN, dtype=dx.dtype, device='cuda')
    buf[:dx.shape[0]].copy_(dx)
    return buf[:dx.shape[0]]


def run_embed_bwd(tabs0, launch, calls=2):
    """`launch(tables)` `calls` times over framed device copies of the non-zero starting tables -> the tables on the CPU."""
    fr = [flat(t.shape, F32, fill=t) for t in tabs0]
    views = [f[1] for f in fr]
    for _ in range(calls):
        launch(views)
    torch.cuda.synchronize()
    for buf, _, mask in fr:
        tb.assert_untouched(buf, mask)
    return [v.cpu() for v in views]


def check_tables(tag, got, refs):
    return max(tb.check(f'{tag} {name}', g, ref, e) for name, g, (ref, e) in zip(('emb', 'pos_s', 'pos_h', 'pos_w'), got, refs))


def pos3d_scatter(L, shape, D, classes, dtype, tag):
    B, S, H, W = shape
    ntok = B * S * H * W
    tok, dx, tabs0 = tb.embed_case(ntok, D, classes, dtype, rows=(S, H, W))
    idx = tb.pos3d_indices(B, S, H, W)
    zd, dxd = dev(tok), nan_rows_after(dx)
    got = run_embed_bwd(tabs0, lambda tv: L.call('wmz_embed_pos3d_bwd', L.ptr(zd), L.ptr(dxd), *[L.ptr(t) for t in tv], B, S, H, W, D,
                                                 classes, L.dtype_code(dtype), L.stream()))
    refs = tb.embed_bwd_ref(tok.clamp(0, classes - 1), *idx, dx, tabs0, calls=2)
    print(f'[tail] embed_pos3d_bwd {shape} D={D} {NAMES[dtype]} -> {pos3d_bwd_kernel(W, D)}')
    return report(f'{tag} {shape} D={D} {NAMES[dtype]}', check_tables(tag, got, refs))


@pytest.mark.parametrize('dtype', [F32, BF16], ids=NAMES.get)
@pytest.mark.parametrize('shape,D', [((2, 2, 4, 3), 8), ((2, 2, 4, 3), 40), ((2, 2, 4, 3), 256), ((2, 2, 4, 3), 300),
                                     ((1, 2, 6, 5), 8), ((1, 2, 6, 5), 40), ((1, 2, 6, 5), 256), ((1, 2, 6, 5), 300),
                                     ((1, 1, 59, 5), 8)])
def test_embedding_backward_general_kernel(L, shape, D, dtype):
    """embed_pos3d_bwd_kernel: W = 3 and 5, one and two sweeps of 256 features, H + W = 64 (all of its LDS)."""
    assert pos3d_bwd_kernel(shape[3], D) == 'embed_pos3d_bwd_kernel'
    pos3d_scatter(L, shape, D, 9, dtype, 'embed_pos3d_bwd general')


@pytest.mark.parametrize('dtype', [F32, BF16], ids=NAMES.get)
@pytest.mark.parametrize('D', [16, 32, 64, 80, 256, 272])
def test_embedding_backward_w16_kernel(L, D, dtype):
    """embed_pos3d_bwd16_kernel at the widths that meet its precondition: a last wave of exactly 16 lanes (16, 80, 272), full waves."""
    assert pos3d_bwd_kernel(16, D) == 'embed_pos3d_bwd16_kernel'
    pos3d_scatter(L, (2, 2, 3, 16), D, 9, dtype, 'embed_pos3d_bwd w16')


@pytest.mark.parametrize('dtype', [F32, BF16], ids=NAMES.get)
@pytest.mark.parametrize('D', [8, 12, 72, 264])
def test_embedding_backward_w16_narrow_last_wave_is_diverted(L, D, dtype):
    """W = 16 with D % 64 in 1..15: the last wave would hand out token ids from lanes that never loaded them, so these widths take
    the general kernel (white box: pos3d_bwd_kernel above restates the rule of wmz_embed_pos3d_bwd); the Python wrapper reaches
    the scatter entry point for them."""
    from world_modelz_amd import ops
    assert pos3d_bwd_kernel(16, D) == 'embed_pos3d_bwd_kernel'
    shape, classes = (2, 2, 3, 16), 9
    pos3d_scatter(L, shape, D, classes, dtype, 'embed_pos3d_bwd w16 diverted')
    B, S, H, W = shape
    tok, dx, tabs0 = tb.embed_case(B * S * H * W, D, classes, dtype, rows=(S, H, W))
    tabs = [dev(t) for t in tabs0]
    with recorded_calls() as seen:
        ops.embed_pos3d_bwd(dev(tok).view(shape), dev(dx).view(*shape, D), tabs)
    torch.cuda.synchronize()
    assert seen == ['wmz_embed_pos3d_bwd']
    refs = tb.embed_bwd_ref(tok.clamp(0, classes - 1), *tb.pos3d_indices(B, S, H, W), dx, tabs0, calls=1)
    check_tables('wrapper', [t.cpu() for t in tabs], refs)


@pytest.mark.parametrize('shape,classes', [((1, 2, 3, 16), 7), ((2, 3, 5, 16), 40), ((2, 3, 16, 16), 65)])
def test_embedding_backward_sorted_route_agrees_with_the_scatter_route(L, shape, classes):
    """wmz_embed_pos3d_bwd_sorted (what the wrapper takes at W = 16, D = 256, bf16) and wmz_embed_pos3d_bwd on the same inputs: each
    within its bound of fp64, and of each other within both."""
    from world_modelz_amd import ops
    B, S, H, W = shape
    D = 256
    tok, dx, tabs0 = tb.embed_case(B * S * H * W, D, classes, BF16, rows=(S, H, W))
    zd, dxd = dev(tok).view(shape), nan_rows_after(dx)
    seen_all = []

    def sorted_route(tv):
        with recorded_calls() as seen:
            ops.embed_pos3d_bwd(zd, dxd.view(*shape, D), tv)
        seen_all.extend(seen)
    got_sorted = run_embed_bwd(tabs0, sorted_route)
    assert seen_all == ['wmz_embed_pos3d_bwd_sorted'] * 2
    got_scatter = run_embed_bwd(tabs0, lambda tv: L.call('wmz_embed_pos3d_bwd', L.ptr(zd), L.ptr(dxd), *[L.ptr(t) for t in tv], B, S, H,
                                                         W, D, classes, L.dtype_code(BF16), L.stream()))
    refs = tb.embed_bwd_ref(tok.clamp(0, classes - 1), *tb.pos3d_indices(B, S, H, W), dx, tabs0, calls=2)
    report(f'embed_pos3d_bwd_sorted {shape}', check_tables('sorted', got_sorted, refs))
    report(f'embed_pos3d_bwd {shape} D=256 bf16 (scatter, embed_pos3d_bwd16_kernel)', check_tables('scatter', got_scatter, refs))
    for a, b, (ref, e) in zip(got_sorted, got_scatter, refs):
        tol = 2 * (e + tb.U32 * (ref.abs() + e)) + tb.TINY[F32]
        assert bool(((a.double() - b.double()).abs() <= tol).all())


@pytest.mark.parametrize('dtype', [F32, BF16], ids=NAMES.get)
@pytest.mark.parametrize('D', [8, 40, 512])
@pytest.mark.parametrize('ntok', [1, 63, 64, 3072])
@pytest.mark.parametrize('grid', [(4, 5, 6), (481, 2, 2)], ids=['lds-tables', 'no-lds'])
def test_embedding_backward_indexed(L, grid, ntok, D, dtype):
    """embed_indexed_bwd_kernel with its LDS tables and without (S + H + W + 1 = 486 rows > 480), one token group (ntok < 128) and
    many, a partial slab of 32 columns (D = 8, 40), half the tokens on the mask class, repeated and out-of-range positions."""
    S, H, W = grid
    classes = 9
    tok, dx, tabs0 = tb.embed_case(ntok, D, classes, dtype, rows=grid)
    pos, pc = indexed_positions(ntok, S, H, W, torch.Generator().manual_seed(ntok + D))
    td, pd, dxd = dev(tok), dev(pos), nan_rows_after(dx)
    got = run_embed_bwd(tabs0, lambda tv: L.call('wmz_embed_indexed_bwd', L.ptr(td), L.ptr(pd), L.ptr(dxd), *[L.ptr(t) for t in tv], ntok,
                                                 S, H, W, D, classes, L.dtype_code(dtype), L.stream()))
    refs = tb.embed_bwd_ref(tok.clamp(0, classes - 1), *split_pos(pc, H, W), dx, tabs0, calls=2)
    report(f'embed_indexed_bwd {"lds" if S + H + W + 1 <= 480 else "no-lds"} ntok={ntok} D={D} {NAMES[dtype]}',
           check_tables('indexed', got, refs))
