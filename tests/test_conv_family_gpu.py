"""The convolution kernel family (csrc/conv2d.hip, conv_direct.hip, conv_point.hip and their half units, conv_wgrad.hip, the
implicit weight gradient of csrc/linear_bwd.hip, wmz_dilate_nhwc) on every route, element by element: each result against an fp64
reference under the derived per-element bound of tests/conv_bounds.py (no element left out) AND under the entry point's norm
tolerance, each output -- activation, both statistics tensors, dW, dbias -- inside a frame of sentinel bytes that must come back
untouched.  Which kernel a case runs is asked of the host (ops.conv_family, wmz_conv2d_nhwc_wgrad_is_direct) and of the entry
points the call reached (recorded_calls); the instantiation follows from the launch rule the case table mirrors.  Every test prints
its largest error-to-bound ratio ([bound] lines: profiles/conv_family_bounds/README.md)."""
import pytest
import torch
import torch.nn.functional as F

import conv_bounds as cb
import gemm_bounds as gb
from conftest import recorded_calls

pytestmark = pytest.mark.gpu

F32, BF16, F16 = cb.F32, cb.BF16, cb.F16
NAMES = cb.NAMES
SLOPE = 0.01
# Frobenius-norm tolerances the entry points are held to today (tests/test_autoencoder_gpu.py, tests/test_precise_conv_gpu.py;
# fp16: the bf16 figure times 2^-11 / 2^-8)
NORM = {F32: 2e-6, BF16: 6e-3, F16: 7.5e-4}
NORM_PRO = {F32: 1e-5, BF16: 2e-2, F16: 1e-3}          # input prologue, reference not rounded to the operand type
NORM_DIRECT = {BF16: 4e-3, F16: 6e-4}
NORM_DGRAD = {F32: 5e-6, BF16: 6e-3}
NORM_WGRAD = {F32: 5e-6, BF16: 2e-5}
FWD_PRE, DIRECT, POINT = 'wmz_conv2d_nhwc_fwd_pre', 'wmz_conv3x3_direct_fwd_strided', 'wmz_conv_point_fwd_bn'
WGRAD_WS = 'wmz_conv2d_nhwc_wgrad_ws'


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'gpu tests need a ROCm device'
    from world_modelz_amd import ops as _ops
    return _ops


def dev(t):
    return t.cuda() if torch.is_tensor(t) else t


def frame(shape, dtype, fill=None):
    """(buffer, view, mask) of a sentinel frame on the device; fill: the view's starting value (a tensor, or 0)"""
    buf, view, mask = gb.framed_flat(tuple(shape), dtype, 'cuda')
    if fill is not None:
        view.copy_(fill) if torch.is_tensor(fill) else view.fill_(fill)
    return buf, view, mask


def untouched(*frames):
    torch.cuda.synchronize()
    for buf, _, mask in frames:
        gb.assert_untouched(buf.cpu(), mask)


def launches(seen):
    """the entry points a call reached, without the weight packs (cached per operand) in front of them"""
    return [n for n in seen if not n.endswith('_pack')]


def kernel_run(ops, case, dtype, od, entry, pre=None):
    """run() of conv_bounds.forward_case on ops.conv2d_nhwc: every output framed, the entry point asserted.  pre: a function
    that makes the launch's `pre` argument (a BnLazy is consumed by one launch)."""
    B, H, W, Cin, Cout, k, stride, pad = case[:8]
    Ho, Wo = cb.out_hw(H, W, k, stride, pad)

    def run(kw, stats):
        fy = frame((B, Ho, Wo, Cout), dtype)
        frames, out = [fy], fy[1]
        if stats:
            fs, fq = frame((cb.REPLICAS, Cout), F32, 0), frame((cb.REPLICAS, Cout), F32, 0)
            frames += [fs, fq]
            out = (fy[1], fs[1], fq[1])
        p = pre() if pre is not None else None
        with recorded_calls() as seen:
            ops.conv2d_nhwc(od['x'], od['w'], k, k, stride, pad, slope=SLOPE, stats=stats, pre=p, out=out,
                            **{n: dev(v) for n, v in kw.items()})
        assert launches(seen) == [entry], seen
        untouched(*frames)
        return fy[1].cpu(), (fs[1].cpu() if stats else None), (fq[1].cpu() if stats else None)
    return run


def operands(case, dtype, seed):
    o = cb.fwd_operands(case, dtype, seed)
    return o, {n: dev(v) for n, v in o.items()}


# ---------------------------------------------------------------------------------------------- implicit GEMM, fp32 and bf16

@pytest.mark.parametrize('case', cb.GEMM_CASES, ids=cb.case_id)
@pytest.mark.parametrize('dtype', [F32, BF16], ids=NAMES.get)
def test_implicit_gemm_forward(ops, dtype, case):
    """conv2d_kernel<T, TALL>: the 128 x 128 tile with a second column tile of 8 columns and a ragged last row tile, the 256 x 64
    tile at Cout 40 and 8, one full and one partial bf16 slab (K = 72), strides, and the in_scale / in_shift prologue at Cin 160."""
    B, H, W, Cin, Cout, k, stride, pad, kind = case
    o, od = operands(case, dtype, seed=51)
    pre = pre_fn = None
    if kind == 'affine':
        pre = cb.prologue(o['x'], o['in_scale'], o['in_shift'], SLOPE, dtype)
        pre_fn = lambda: (od['in_scale'], od['in_shift'], SLOPE)
    keep = ops.DIRECT_CONV
    try:
        # (the prologue at 160 channels is wider than the streaming kernel's: the route answers 'gemm' with the other kernels on)
        ops.DIRECT_CONV = kind is not None
        if dtype == BF16:
            for res in (False, True):
                assert ops.conv_family(B, H, W, Cin, Cout, k, k, stride, pad, res, kind is not None, SLOPE) == 'gemm'
        worst = cb.forward_case(case, dtype, o, kernel_run(ops, case, dtype, od, FWD_PRE, pre_fn), pre=pre,
                                norm_tol=(NORM_PRO if kind else NORM)[dtype])
    finally:
        ops.DIRECT_CONV = keep
    cb.report(f'gemm {NAMES[dtype]} {cb.case_id(case)} tile {"256x64" if Cout <= 64 else "128x128"}', worst)


# ---------------------------------------------------------------------------------------------- direct 3x3, bf16 and half

@pytest.mark.parametrize('case', cb.DIRECT_CASES, ids=cb.case_id)
@pytest.mark.parametrize('dtype', [BF16, F16], ids=NAMES.get)
def test_direct_forward(ops, dtype, case):
    """convr_kernel<NCB, TW, NPASS, STRIDE>: all fourteen instantiations in both operand formats, B = 3 (a tile count that is no
    multiple of 8), with and without the residual epilogue."""
    B, H, W, Cin, Cout, k, stride, pad, _ = case
    assert ops.DIRECT_CONV
    for res in (False, True):
        assert ops.conv_family(B, H, W, Cin, Cout, 3, 3, stride, 1, res, False, SLOPE) == 'direct'
    o, od = operands(case, dtype, seed=52)
    worst = cb.forward_case(case, dtype, o, kernel_run(ops, case, dtype, od, ops.L.half_form(DIRECT, dtype)), norm_tol=NORM_DIRECT[dtype])
    cb.report(f'direct {NAMES[dtype]} {cb.case_id(case)} convr_kernel<%d, %d, %d, %d>' % cb.direct_instantiation(case), worst)


def test_every_direct_instantiation_is_listed(ops):
    """12 stride-1 instantiations (NCB 1 / 2 / 4 x plane width 32 / 16 x one or two channel passes) and 2 stride-2 ones, each in
    bf16 and half: the case list reaches all 28, every case on a shape the direct kernel answers for."""
    want = {(dt, ncb, tw, npass, 1) for dt in (BF16, F16) for ncb in (1, 2, 4) for tw in (32, 16) for npass in (1, 2)} \
        | {(dt, 4, 16, npass, 2) for dt in (BF16, F16) for npass in (1, 2)}
    got = set()
    for c in cb.DIRECT_CASES:
        B, H, W, Cin, Cout, k, stride, pad, _ = c
        assert ops.L.lib().wmz_conv3x3_direct_supported_strided(H, W, Cin, Cout, stride), c
        got |= {(dt,) + cb.direct_instantiation(c) for dt in (BF16, F16)}
    assert got == want and len(got) == 28


# ---------------------------------------------------------------------------------------------- small-K streaming, bf16 and half

def raw_prologue(ops, o, od, dtype, count):
    """The raw-statistics prologue of a case: the sums on the device (what the kernel receives), the reference prologue with
    the error of the kernel's own finalisation, and a maker of fresh BnLazy objects (one launch consumes one)."""
    Cin = o['x'].shape[-1]
    s, q = ops.channel_stats_nhwc(od['x'])
    s, q = s.clone(), q.clone()
    f = cb.bn_fold_ref(s.cpu(), q.cpu(), count, o['gamma'], o['beta'], 1e-5)
    made = []

    def make():
        bn = torch.nn.BatchNorm2d(Cin, eps=1e-5).cuda().train()
        with torch.no_grad():
            bn.weight.copy_(od['gamma'])
            bn.bias.copy_(od['beta'])
        lz = ops.bn_lazy(bn, s, q, count, want_stats=True)
        assert not lz.done
        made.append(lz)
        return (lz, None, SLOPE)
    return f, cb.prologue(o['x'], f['scale'], f['shift'], SLOPE, dtype, f['e_scale'], f['e_shift']), make, made


@pytest.mark.parametrize('case', cb.POINT_CASES + cb.POINT_PERSISTENT, ids=cb.case_id)
@pytest.mark.parametrize('dtype', [BF16, F16], ids=NAMES.get)
def test_small_k_forward(ops, dtype, case):
    """convp_kernel<NCB, NPB, PAD>: K from 8 to the cap of 256, every prologue form (none, in_scale / in_shift, raw statistics
    finalised by the launch), padded and strided geometries, and two launches in which a wave takes a second run."""
    B, H, W, Cin, Cout, k, stride, pad, kind = case
    assert ops.DIRECT_CONV and ops.conv_family(B, H, W, Cin, Cout, k, k, stride, pad, False, kind is not None, SLOPE) == 'point'
    runs, waves = cb.point_runs(case)
    only = None
    if case in cb.POINT_PERSISTENT:
        assert waves == 2048 and runs > waves
        only = ('bias+leaky+stats', 'bias+affine')
    o, od = operands(case, dtype, seed=53)
    pre = pre_fn = fold = made = None
    if kind == 'affine':
        pre = cb.prologue(o['x'], o['in_scale'], o['in_shift'], SLOPE, dtype)
        pre_fn = lambda: (od['in_scale'], od['in_shift'], SLOPE)
    elif kind == 'raw':
        fold, pre, pre_fn, made = raw_prologue(ops, o, od, dtype, B * H * W)
    worst = cb.forward_case(case, dtype, o, kernel_run(ops, case, dtype, od, ops.L.half_form(POINT, dtype), pre_fn), residual=False,
                            pre=pre, norm_tol=(NORM_PRO if kind else NORM)[dtype], only=only)
    if kind == 'raw':       # what the launch's first workgroup published for the backward pass
        lz = made[-1]
        assert lz.done
        for n in ('scale', 'shift', 'mean', 'rstd'):
            worst['bn.' + n] = gb.check('bn.' + n, getattr(lz, n).cpu(), fold[n], fold['e_' + n])
    cb.report(f'point {NAMES[dtype]} {cb.case_id(case)} runs {runs} waves {waves}', worst)


# ---------------------------------------------------------------------------------------------- data gradient

@pytest.mark.parametrize('case', cb.DGRAD_CASES, ids=cb.case_id)
@pytest.mark.parametrize('dtype', [F32, BF16], ids=NAMES.get)
def test_data_gradient(ops, dtype, case):
    """The forward kernel as the data gradient: autoencoder._wT_op's flipped operand, pad k - 1 - pad, the zero-inserted plane at
    stride 2 (with and without output padding), dskip as the residual operand -- against fp64 autograd of F.conv2d."""
    from world_modelz_amd import autoencoder as ae
    B, Hi, Wi, ci, co, k, stride, pad = case
    g = torch.Generator().manual_seed(54)
    Ho, Wo = cb.out_hw(Hi, Wi, k, stride, pad)
    weight = (torch.randn(co, ci, k, k, generator=g) / (k * k * co) ** 0.5).to(dtype)
    dy = F.pad((torch.randn(B, Ho, Wo, co, generator=g) * 0.5 + 0.1), (0, -co % 8)).to(dtype)
    dskip = torch.randn(B, Hi, Wi, ci + -ci % 8, generator=g).to(dtype)
    wd = weight.cuda()
    wt = ae._wT_op(wd, dtype)
    assert torch.equal(wt.cpu(), cb.flipped_operand(weight, dtype))
    auto = cb.dgrad_autograd64(dy, weight, stride, pad, Hi, Wi)
    Hz, Wz = cb.dgrad_plane(Hi, Wi, Ho, Wo, k, stride, pad)
    dyd = dy.cuda()
    worst = {}
    if stride > 1:
        fz = frame((B, Hz, Wz, dy.shape[-1]), dtype)
        with recorded_calls() as seen:
            dz = ops.dilate_nhwc(dyd, Hz, Wz, stride, out=fz[1])
        assert seen == ['wmz_dilate_nhwc']
        untouched(fz)
        assert torch.equal(dz.cpu(), cb.dilate_ref(dy, Hz, Wz, stride)), 'the zero-inserted plane is not exact'
    else:
        dz = dyd
    Cz, Cx = dy.shape[-1], dskip.shape[-1]
    for tag, sk in (('plain', None), ('dskip', dskip)):
        r = cb.dgrad_ref(dy, wt.cpu(), k, stride, pad, Hi, Wi, sk)
        want = auto + (0 if sk is None else sk.double())
        assert float((r['ref'] - want).abs().max()) <= 1e-12 * float(want.abs().max())
        fam = ops.conv_family(B, Hz, Wz, Cz, Cx, k, k, 1, k - 1 - pad, sk is not None, False, SLOPE) if dtype != F32 else 'gemm'
        fx = frame((B, Hi, Wi, Cx), dtype)
        with recorded_calls() as seen:
            ops.conv2d_nhwc(dz, wt, k, k, 1, k - 1 - pad, residual=dev(sk), out=fx[1])
        assert launches(seen) == [dict(gemm=FWD_PRE, point=POINT, direct=DIRECT)[fam]], (fam, seen)
        untouched(fx)
        worst[f'{tag}/{fam}'] = gb.check(tag, fx[1].cpu(), r['ref'], r['e_in'], norm_tol=NORM_DGRAD[dtype])
    cb.report(f'dgrad {NAMES[dtype]} {cb.case_id(case)}', worst)


@pytest.mark.parametrize('dtype', [F32, BF16], ids=NAMES.get)
def test_dilate_alone(ops, dtype):
    """wmz_dilate_nhwc bit for bit inside a frame: stride 2 with output padding 0 and 1, stride 3, a plane wider than one
    workgroup's 256 vectors."""
    g = torch.Generator().manual_seed(55)
    for (B, Ho, Wo, C, stride, oph, opw) in [(2, 5, 7, 8, 2, 0, 0), (2, 5, 7, 8, 2, 1, 1), (3, 4, 6, 40, 2, 1, 0), (1, 3, 5, 16, 3, 2, 1),
                                             (1, 2, 70, 16, 2, 0, 1)]:
        dy = torch.randn(B, Ho, Wo, C, generator=g).to(dtype)
        Hz, Wz = (Ho - 1) * stride + 1 + oph, (Wo - 1) * stride + 1 + opw
        fz = frame((B, Hz, Wz, C), dtype)
        with recorded_calls() as seen:
            ops.dilate_nhwc(dy.cuda(), Hz, Wz, stride, out=fz[1])
        assert seen == ['wmz_dilate_nhwc']
        untouched(fz)
        assert torch.equal(fz[1].cpu(), cb.dilate_ref(dy, Hz, Wz, stride)), (B, Ho, Wo, C, stride, oph, opw)
        assert torch.equal(ops.dilate_nhwc(dy.cuda(), Hz, Wz, stride).cpu(), fz[1].cpu())


# ---------------------------------------------------------------------------------------------- weight gradient

def wgrad_forms(ops, case, dtype, direct):
    """One weight-gradient geometry in three forms: (a) overwrite into a frame, (b) accumulate onto random dW0 / db0, (c) the
    nn.Conv2d layout through into=, channels cropped, called twice so the second call adds."""
    L = ops.L
    B, H, W, Cin, Cout, k, stride, pad = case
    dt = L.dtype_code(dtype)
    assert bool(L.lib().wmz_conv2d_nhwc_wgrad_is_direct(B, H, W, Cin, Cout, k, k, stride, pad, dt)) == direct
    o = cb.wgrad_operands(case, dtype, seed=56)
    xd, dyd = o['x'].cuda(), o['dy'].cuda()
    K = k * k * Cin
    norm = NORM_WGRAD[dtype]
    worst = {}
    # (a)
    fw, fb = frame((Cout, K), F32), frame((Cout,), F32)
    with recorded_calls() as seen:
        ops.conv2d_nhwc_wgrad(xd, dyd, k, k, stride, pad, True, out=(fw[1], fb[1]))
    assert seen == [WGRAD_WS], seen
    untouched(fw, fb)
    rw, ew, rb, eb = cb.conv_wgrad_ref(o['x'], o['dy'], k, k, stride, pad)
    worst['overwrite'] = gb.check('overwrite', fw[1].cpu(), rw, ew, norm_tol=norm)
    worst['overwrite.b'] = gb.check('overwrite.dbias', fb[1].cpu(), rb, eb, norm_tol=norm)
    # (b) the plain layout accumulates through the entry point itself (ops stores or takes into=)
    fw, fb = frame((Cout, K), F32, o['dw0']), frame((Cout,), F32, o['db0'])
    need = L.lib().wmz_conv2d_nhwc_wgrad_workspace_floats(B, H, W, Cin, Cout, k, k, stride, pad, dt)
    ws = ops._workspace(xd.device, need)
    L.call(WGRAD_WS, L.ptr(xd), L.ptr(dyd), L.ptr(fw[1]), L.ptr(fb[1]), B, H, W, Cin, Cout, k, k, stride, pad, 0, 0, 0, L.ptr(ws),
           ws.numel(), dt, L.stream())
    untouched(fw, fb)
    rw1, ew1, rb1, eb1 = cb.conv_wgrad_ref(o['x'], o['dy'], k, k, stride, pad, o['dw0'], o['db0'])
    worst['accumulate'] = gb.check('accumulate', fw[1].cpu(), rw1, ew1, norm_tol=norm)
    worst['accumulate.b'] = gb.check('accumulate.dbias', fb[1].cpu(), rb1, eb1, norm_tol=norm)
    # (c)
    co, ci = cb.crop(Cout, Cin)
    lay = lambda t: cb.conv_layout(t, k, k, co, ci)
    fw, fb = frame((co, ci, k, k), F32, lay(o['dw0'])), frame((co,), F32, o['db0'][:co])
    with recorded_calls() as seen:
        for _ in range(2):
            ops.conv2d_nhwc_wgrad(xd, dyd, k, k, stride, pad, True, into=(fw[1], fb[1]))
        ops.wgrad_join()
    assert seen == [WGRAD_WS, WGRAD_WS], seen
    untouched(fw, fb)
    rw2, ew2, rb2, eb2 = cb.conv_wgrad_ref(o['x'], o['dy'], k, k, stride, pad, o['dw0'], o['db0'], times=2)
    worst['layout x2'] = gb.check('layout', fw[1].cpu(), lay(rw2), lay(ew2), norm_tol=norm)
    worst['layout x2.b'] = gb.check('layout.dbias', fb[1].cpu(), rb2[:co], eb2[:co], norm_tol=norm)
    return worst


@pytest.mark.parametrize('case', cb.WGRAD_IMPLICIT, ids=cb.case_id)
@pytest.mark.parametrize('dtype', [F32, BF16], ids=NAMES.get)
def test_implicit_weight_gradient(ops, dtype, case):
    cb.report(f'wgrad implicit {NAMES[dtype]} {cb.case_id(case)}', wgrad_forms(ops, case, dtype, direct=False))


@pytest.mark.parametrize('case', cb.WGRAD_DIRECT, ids=cb.case_id)
def test_direct_weight_gradient(ops, case):
    """convw_kernel<4> (Cout 128) and <1> (Cout 8 / 24 / 32) at Cin 64 and 128: one tile, B = 1 (fewer tiles than workgroups) and
    B = 70 of 16 x 32 (280 tiles: more than one per workgroup)."""
    cb.report(f'wgrad direct bf16 {cb.case_id(case)} convw_kernel<{4 if case[4] == 128 else 1}>', wgrad_forms(ops, case, BF16, direct=True))


@pytest.mark.parametrize('dtype', [F32, BF16], ids=NAMES.get)
def test_weight_gradient_batch(ops, dtype):
    """wmz_conv2d_nhwc_wgrad_batch: three problems of different geometry by one launch pair, host tables as ops builds them for
    its queue -- one accumulating in the plain layout, one in the nn.Conv2d layout with dbias NULL, one in overwrite mode; then a
    layer the direct kernel answers for, placed alone through wmz_conv2d_nhwc_wgrad_ws as include/wmz.h advises."""
    L = ops.L
    dt = L.dtype_code(dtype)
    rows, probs, need = [], [], 0
    for i, (case, over, layout, bias) in enumerate(cb.WGRAD_BATCH):
        B, H, W, Cin, Cout, k, stride, pad = case
        assert not L.lib().wmz_conv2d_nhwc_wgrad_is_direct(B, H, W, Cin, Cout, k, k, stride, pad, dt)
        o = cb.wgrad_operands(case, dtype, seed=57 + i)
        co, ci = cb.crop(Cout, Cin) if layout else (0, 0)
        lay = (lambda t, k=k, co=co, ci=ci: cb.conv_layout(t, k, k, co, ci)) if layout else (lambda t: t)
        fw = frame(lay(o['dw0']).shape, F32, lay(o['dw0']))
        fb = frame((co if layout else Cout,), F32, o['db0'][:co] if layout else o['db0'])
        xd, dyd = o['x'].cuda(), o['dy'].cuda()
        rows.append((L.ptr(xd), L.ptr(dyd), L.ptr(fw[1]), L.ptr(fb[1]) if bias else None, B, H, W, Cin, Cout, k, k, stride, pad,
                     1 if over else 0, co, ci))
        need += L.lib().wmz_conv2d_nhwc_wgrad_workspace_floats(B, H, W, Cin, Cout, k, k, stride, pad, dt)
        probs.append((case, over, bias, o, lay, co if layout else Cout, fw, fb, xd, dyd))
    ws = ops._workspace(torch.device('cuda', torch.cuda.current_device()), need)
    with recorded_calls() as seen:
        L.call('wmz_conv2d_nhwc_wgrad_batch', len(rows), *L.columns(rows, 'pppp' + 'i' * 12), L.ptr(ws), ws.numel(), dt, L.stream())
    assert seen == ['wmz_conv2d_nhwc_wgrad_batch']
    worst = {}
    for i, (case, over, bias, o, lay, nb, fw, fb, xd, dyd) in enumerate(probs):
        B, H, W, Cin, Cout, k, stride, pad = case
        untouched(fw, fb)
        rw, ew, rb, eb = cb.conv_wgrad_ref(o['x'], o['dy'], k, k, stride, pad, None if over else o['dw0'], None if over else o['db0'])
        worst[f'p{i}'] = gb.check(f'problem {i} dW', fw[1].cpu(), lay(rw), lay(ew), norm_tol=NORM_WGRAD[dtype])
        if bias:
            worst[f'p{i}.b'] = gb.check(f'problem {i} dbias', fb[1].cpu(), rb[:nb], eb[:nb], norm_tol=NORM_WGRAD[dtype])
        else:
            assert torch.equal(fb[1].cpu(), o['db0'][:nb]), 'dbias NULL: the bias gradient is not the launch\'s to write'
    if dtype == BF16:
        case = cb.WGRAD_DIRECT[0]
        worst.update({'alone/' + n: v for n, v in wgrad_forms(ops, case, dtype, direct=True).items() if n.startswith('overwrite')})
    cb.report(f'wgrad batch {NAMES[dtype]}', worst)
