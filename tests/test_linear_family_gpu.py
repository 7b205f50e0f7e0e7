"""The nn.Linear / LayerNorm kernel family (csrc/linear_fwd.hip, its half unit, the linear and LayerNorm part of
csrc/linear_bwd.hip) on every route, element by element: each result against an fp64 reference under the derived per-element
bound of tests/gemm_bounds.py (no element left out) AND under the entry point's norm tolerance, each output inside a frame of
sentinel bytes that must come back untouched.  Which linear_kernel instantiation a case runs is asked of the library
(wmz_debug_linear_route: the launch's own decision); the last test lists all sixteen as reached.  Every test prints its largest
error-to-bound ratio ([bound] lines: profiles/linear_family_bounds/README.md)."""
import pytest
import torch

import gemm_bounds as gb

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
NAMES = {F32: 'fp32', BF16: 'bf16', F16: 'fp16'}
EPS = 1e-5
# Frobenius-norm tolerances of tests/test_kernels_gpu.py (fp16: the bf16 figure times 2^-11 / 2^-8)
NORM = {F32: 2e-6, BF16: 6e-3, F16: 7.5e-4}
NORM_PRO = {F32: 3e-6, BF16: 8e-3, F16: 1e-3}          # LayerNorm / GELU-in prologue, reference not rounded to the operand type
NORM_F32_OUT = {F32: 2e-6, BF16: 1e-5, F16: 1e-5}      # fp32 output of exact products


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'gpu tests need a ROCm device'
    from world_modelz_amd import ops as _ops
    return _ops


def dev(t):
    return None if t is None else t.cuda()


def route(a, w, M, N, K, prologue=0, out_f32=False, lda=None, block_stride=0):
    """(row-tile height, LDS-DMA ring taken) of the launch linear_launch would make for these operands."""
    from world_modelz_amd import _lib as L
    r = L.lib().wmz_debug_linear_route(a.data_ptr(), K if lda is None else lda, w.data_ptr(), block_stride, M, N, K, prologue,
                                       1 if out_f32 else 0, L.dtype_code(a.dtype))
    assert r & 255 in (64, 128), r
    return r & 255, bool(r >> 8)


def framed_run(M, N, dtype, launch, ld=None, left=8):
    """launch(out) writes an [M, N] view of a sentinel frame; the frame outside it must come back bit-identical -> result on the host."""
    buf, out, mask = gb.framed(M, N, dtype, 'cuda', ld=ld, left=left)
    launch(out)
    torch.cuda.synchronize()
    host = buf.cpu()
    gb.assert_untouched(host, mask)
    return host[:M, left:left + N]


def operands(M, N, K, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    a = (torch.randn(M, K, generator=g) * 1.5 + 0.3).to(dtype)          # rows with a non-zero mean
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dtype)
    bias = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g).to(dtype)
    gam, bet = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.1
    return a, w, bias, res, gam, bet


def stats_of(ops, a_dev):
    """layernorm_stats takes fp32 / bf16; half rows are exact in fp32"""
    return ops.layernorm_stats(a_dev.float() if a_dev.dtype == F16 else a_dev, EPS)


def report(tag, worst):
    print(f'[bound] {tag}: ' + ' '.join(f'{k}={v:.3f}' for k, v in worst.items()) + f' | max {max(worst.values()):.3f}')
    assert max(worst.values()) <= 1.0


# ---------------------------------------------------------------------------------------------- forward: the route table

SMALL, ODD, BIG, BIG_F32OUT = (130, 136, 72), (77, 50, 24), (1300, 3720, 72), (1300, 2184, 72)
# (dtype, prologue, shape, out_f32, row-tile height): every instantiation linear_launch can launch, and the shapes beside them
ROUTES = ([(dt, pro, SMALL, False, 64) for dt in (BF16, F16) for pro in (0, 1, 2)]
          + [(dt, pro, BIG, False, 128) for dt in (BF16, F16) for pro in (0, 1, 2)]
          + [(F32, 0, SMALL, False, 64), (F32, 0, BIG, False, 128), (F32, 1, SMALL, False, 128), (F32, 2, SMALL, False, 128)]
          + [(dt, 0, ODD, False, 64) for dt in (F32, BF16, F16)]
          + [(dt, 0, BIG_F32OUT, True, 128) for dt in (BF16, F16)]
          + [(dt, 0, BIG_F32OUT, False, 64) for dt in (BF16, F16)])        # the same 198 tiles below the 16-bit outputs' bar
INSTANTIATIONS = ({(dt, pro, bm) for dt in (BF16, F16) for pro in (0, 1, 2) for bm in (64, 128)}
                  | {(F32, 0, 64), (F32, 0, 128), (F32, 1, 128), (F32, 2, 128)})


def route_id(c):
    dt, pro, (M, N, K), f32, bm = c
    return f'{NAMES[dt]}-{("plain", "ln", "gelu_in")[pro]}-{M}x{N}x{K}{"-f32out" if f32 else ""}-bm{bm}'


@pytest.mark.parametrize('case', ROUTES, ids=route_id)
def test_forward_route(ops, case):
    dtype, pro, (M, N, K), out_f32, bm = case
    a, w, bias, res, gam, bet = operands(M, N, K, dtype, seed=11)
    ad, wd, bd = dev(a), dev(w), dev(bias)
    assert route(ad, wd, M, N, K, pro, out_f32) == (bm, False), 'the shape no longer reaches the tile it is here for'
    odt = F32 if out_f32 else dtype
    ln = (gam, bet) if pro == 1 else None
    kw = dict(ln=(dev(gam), dev(bet))) if pro == 1 else (dict(gelu_in=True) if pro == 2 else {})
    r = gb.linear_ref(a, w, bias=bias, ln=ln, gelu_in=pro == 2)
    norm = (NORM_PRO if pro else (NORM_F32_OUT if out_f32 else NORM))[dtype]
    worst = {}
    y = framed_run(M, N, odt, lambda out: ops.linear_fwd(ad, wd, bias=bd, out_f32=out_f32, out=out, **kw))
    worst['bias'] = gb.check('bias', y, r['ref'], r['e_in'], norm_tol=norm)
    if pro == 1:
        st = stats_of(ops, ad)
        y = framed_run(M, N, odt, lambda out: ops.linear_fwd(ad, wd, bias=bd, out_f32=out_f32, out=out, ln_stats=st, **kw))
        worst['ln_stats'] = gb.check('ln_stats', y, r['ref'], r['e_in'], norm_tol=norm)
    report(route_id(case), worst)


def test_every_instantiation_is_reached():
    """The route table above, asked of the launch's own decision: all sixteen (type, prologue, tile) instantiations are there.  A
    change of the 320 / 192 tile thresholds fails here (and in the cases themselves) instead of moving coverage silently."""
    reached = set()
    for dtype, pro, (M, N, K), out_f32, bm in ROUTES:
        a, w = torch.empty(M, K, dtype=dtype, device='cuda'), torch.empty(N, K, dtype=dtype, device='cuda')
        got, _ = route(a, w, M, N, K, pro, out_f32)
        assert got == bm, route_id((dtype, pro, (M, N, K), out_f32, bm))
        reached.add((dtype, pro, got))
    print('[bound] instantiations reached: ' + ', '.join(sorted(f'{NAMES[d]}/{("plain", "ln", "gelu_in")[p]}/{b}' for d, p, b in reached)))
    assert reached == INSTANTIATIONS and len(reached) == 16


# ---------------------------------------------------------------------------------------------- forward: epilogues per tile height

@pytest.mark.parametrize('shape,bm', [(SMALL, 64), (ODD, 64), (BIG, 128)], ids=['bm64', 'bm64-odd', 'bm128'])
@pytest.mark.parametrize('dtype', [F32, BF16, F16], ids=NAMES.get)
def test_forward_epilogues(ops, dtype, shape, bm):
    M, N, K = shape
    a, w, bias, res, gam, bet = operands(M, N, K, dtype, seed=12)
    ad, wd, bd, rd = dev(a), dev(w), dev(bias), dev(res)
    worst = {}
    for tag, kw, f32 in [('plain', {}, False), ('bias', dict(bias=bias), False), ('gelu', dict(bias=bias, gelu=True), False),
                         ('residual', dict(bias=bias, residual=res), False),
                         ('gelu+residual', dict(bias=bias, gelu=True, residual=res), False),
                         ('f32out', dict(bias=bias), True), ('f32out+residual', dict(bias=bias, residual=res), True)]:
        # (an fp32 output lowers the tile bar to 192: the 128-row shape stays above it, the small ones below)
        assert route(ad, wd, M, N, K, 0, f32) == (bm, False)
        r = gb.linear_ref(a, w, **kw)
        dkw = {k: (dev(v) if torch.is_tensor(v) else v) for k, v in kw.items()}
        odt = F32 if f32 else dtype
        y = framed_run(M, N, odt, lambda out: ops.linear_fwd(ad, wd, out_f32=f32, out=out, **dkw))
        # (a residual of the operand type is not an exact product: the fp32 output's norm tolerance is the fp32 kernel's)
        worst[tag] = gb.check(tag, y, r['ref'], r['e_in'], norm_tol=(NORM_F32_OUT if f32 else NORM)[dtype])
    report(f'epilogues {NAMES[dtype]} {M}x{N}x{K} bm{bm}', worst)


# ---------------------------------------------------------------------------------------------- forward: the LDS-DMA ring

@pytest.mark.parametrize('K', [64, 128, 192, 256])
@pytest.mark.parametrize('dtype', [BF16, F16], ids=NAMES.get)
def test_forward_dma_ring(ops, dtype, K):
    """One to four slabs through the three-buffer ring; bf16 again on the register-staged loop (the development knob belongs to
    the bf16 / fp32 unit: the half unit has no switch)."""
    from world_modelz_amd import _lib as L
    M, N = 130, 136
    a, w, bias, res, gam, bet = operands(M, N, K, dtype, seed=13)
    ad, wd, bd, rd = dev(a), dev(w), dev(bias), dev(res)
    r = gb.linear_ref(a, w, bias=bias, residual=res)
    assert route(ad, wd, M, N, K) == (64, True)
    worst = {}
    y = framed_run(M, N, dtype, lambda out: ops.linear_fwd(ad, wd, bias=bd, residual=rd, out=out))
    worst['ring'] = gb.check('ring', y, r['ref'], r['e_in'], norm_tol=NORM[dtype])
    if dtype == BF16:
        L.lib().wmz_debug_linear_knobs(0)
        try:
            assert route(ad, wd, M, N, K) == (64, False)
            y2 = framed_run(M, N, dtype, lambda out: ops.linear_fwd(ad, wd, bias=bd, residual=rd, out=out))
        finally:
            L.lib().wmz_debug_linear_knobs(1)
        worst['registers'] = gb.check('registers', y2, r['ref'], r['e_in'], norm_tol=NORM[dtype])
        print(f'[bound] ring and register-staged loop bit-equal at K={K}: {torch.equal(y, y2)}')
    report(f'dma ring {NAMES[dtype]} K={K}', worst)


# ---------------------------------------------------------------------------------------------- forward: row strides

@pytest.mark.parametrize('dtype', [F32, BF16, F16], ids=NAMES.get)
def test_forward_row_strides(ops, dtype):
    M, N, K = SMALL
    a, w, bias, res, gam, bet = operands(M, N, K, dtype, seed=14)
    g = torch.Generator().manual_seed(15)
    a3 = (torch.randn(M, 3 * K, generator=g) * 1.5 + 0.3).to(dtype)
    a3[:, K:2 * K] = a
    r2 = torch.randn(M, 2 * N, generator=g).to(dtype)
    r2[:, N:] = res
    a3d, wd, bd, r2d = dev(a3), dev(w), dev(bias), dev(r2)
    amid, rsl = a3d[:, K:2 * K], r2d[:, N:]
    assert amid.stride(0) == 3 * K and rsl.stride(0) == 2 * N
    r = gb.linear_ref(a, w, bias=bias, residual=res)
    rl = gb.linear_ref(a, w, bias=bias, ln=(gam, bet))
    rb = gb.linear_ref(a, w, bias=bias)
    worst = {}
    # a = the middle third of [M, 3K], residual = a slice of [M, 2N], out = a slice of [M, 2N + 16]
    y = framed_run(M, N, dtype, lambda out: ops.linear_fwd(amid, wd, bias=bd, residual=rsl, out=out), ld=2 * N + 16, left=N)
    worst['lda/ldr/ldc'] = gb.check('strided', y, r['ref'], r['e_in'], norm_tol=NORM[dtype])
    y = framed_run(M, N, dtype, lambda out: ops.linear_fwd(amid, wd, bias=bd, ln=(dev(gam), dev(bet)), out=out), ld=2 * N + 16, left=N)
    worst['lda+ln'] = gb.check('strided ln', y, rl['ref'], rl['e_in'], norm_tol=NORM_PRO[dtype])
    # ldc % 8 != 0 (ldc % 4 != 0 for the fp32 output): the unstaged epilogue
    y = framed_run(M, N, dtype, lambda out: ops.linear_fwd(amid, wd, bias=bd, residual=rsl, out=out), ld=N + 8 + 5, left=8)
    worst['ldc%8'] = gb.check('ldc % 8', y, r['ref'], r['e_in'], norm_tol=NORM[dtype])
    y = framed_run(M, N, F32, lambda out: ops.linear_fwd(amid, wd, bias=bd, out_f32=True, out=out), ld=N + 8 + 5, left=8)
    worst['f32 ldc%4'] = gb.check('f32 ldc % 4', y, rb['ref'], rb['e_in'], norm_tol=NORM_F32_OUT[dtype])
    y = framed_run(M, N, F32, lambda out: ops.linear_fwd(amid, wd, bias=bd, out_f32=True, out=out), ld=2 * N + 16, left=N)
    worst['f32 ldc'] = gb.check('f32 ldc', y, rb['ref'], rb['e_in'], norm_tol=NORM_F32_OUT[dtype])
    # the staged epilogue (row stride a multiple of 8) with a last column chunk of 2: N = 50 inside rows of 72
    Mo, No, Ko = ODD
    a, w, bias, res, gam, bet = operands(Mo, No, Ko, dtype, seed=16)
    ro = gb.linear_ref(a, w, bias=bias, gelu=True)
    y = framed_run(Mo, No, dtype, lambda out: ops.linear_fwd(dev(a), dev(w), bias=dev(bias), gelu=True, out=out), ld=72, left=8)
    worst['staged tail'] = gb.check('staged tail', y, ro['ref'], ro['e_in'], norm_tol=NORM[dtype])
    rf = gb.linear_ref(a, w, bias=bias)
    y = framed_run(Mo, No, F32, lambda out: ops.linear_fwd(dev(a), dev(w), bias=dev(bias), out_f32=True, out=out), ld=72, left=8)
    worst['staged f32 tail'] = gb.check('staged f32 tail', y, rf['ref'], rf['e_in'], norm_tol=NORM_F32_OUT[dtype])
    report(f'row strides {NAMES[dtype]}', worst)


# ---------------------------------------------------------------------------------------------- the pair and the training forward

@pytest.mark.parametrize('shape', [SMALL, BIG], ids=['130x136x72', '1300x3720x72'])
@pytest.mark.parametrize('dtype', [F32, BF16], ids=NAMES.get)
def test_gelu_pair_and_train(ops, dtype, shape):
    M, N, K = shape
    a, w, bias, res, gam, bet = operands(M, N, K, dtype, seed=17)
    ad, wd, bd, ln = dev(a), dev(w), dev(bias), (dev(gam), dev(bet))
    worst = {}

    def three(tag, launch, r, norm, want_an):
        zb, z, zm = gb.framed(M, N, dtype, 'cuda')
        hb, h, hm = gb.framed(M, N, dtype, 'cuda', ld=N + 24)
        nb, an, nm = gb.framed(M, K, dtype, 'cuda')
        launch(z, h, an)
        torch.cuda.synchronize()
        for b, m in ((zb, zm), (hb, hm)) + (((nb, nm),) if want_an else ()):
            gb.assert_untouched(b.cpu(), m)
        rh_e = gb.gelu_err(r['pre'], r['e_pre'])
        worst[tag + '.z'] = gb.check(tag + '.z', z.cpu(), r['pre'], r['e_pre'], norm_tol=norm)
        worst[tag + '.h'] = gb.check(tag + '.h', h.cpu(), gb.gelu64(r['pre']), rh_e, norm_tol=norm)
        if want_an:       # complete at the K tail and on the last rows, and the operand rounding of the kernel's own LayerNorm
            y_an, e_an = gb.ln_apply(a, gam, bet, EPS, F32)          # (the rounding to the operand type is this output's own)
            worst[tag + '.an'] = gb.check(tag + '.an', an.cpu(), y_an, e_an, norm_tol=3e-6 if dtype == F32 else 4e-3)

    rp = gb.linear_ref(a, w, bias=bias)
    three('pair', lambda z, h, an: ops.linear_fwd_gelu_pair(ad, wd, bias=bd, out=(z, h)), rp, NORM[dtype], False)
    rl = gb.linear_ref(a, w, bias=bias, ln=(gam, bet))
    st = ops.layernorm_stats(ad, EPS)
    three('pair+ln', lambda z, h, an: ops.linear_fwd_gelu_pair(ad, wd, bias=bd, ln=ln, ln_stats=st, out=(z, h)), rl, NORM_PRO[dtype], False)
    three('train', lambda z, h, an: ops.linear_fwd_train(ad, wd, bd, ln, EPS, st, want_gelu=True, want_norm=True, out=(z, h, an)),
          rl, NORM_PRO[dtype], True)
    three('train/own stats', lambda z, h, an: ops.linear_fwd_train(ad, wd, bd, ln, EPS, None, want_gelu=True, want_norm=True, out=(z, h, an)),
          rl, NORM_PRO[dtype], True)
    report(f'pair / train {NAMES[dtype]} {M}x{N}x{K}', worst)


# ---------------------------------------------------------------------------------------------- the last-frame blocks

@pytest.mark.parametrize('B,S,HW,D,N', [(3, 4, 20, 24, 50), (5, 2, 77, 72, 136)])
@pytest.mark.parametrize('dtype', [F32, BF16, F16], ids=NAMES.get)
def test_forward_blocks(ops, dtype, B, S, HW, D, N):
    """64-row tiles that straddle a block boundary (20 and 77 rows per block)."""
    g = torch.Generator().manual_seed(18)
    x = (torch.randn(B, S, HW, D, generator=g) * 1.5 + 0.3).to(dtype)
    w = (torch.randn(N, D, generator=g) / D ** 0.5).to(dtype)
    bias = torch.randn(N, generator=g)
    xd, wd, bd = dev(x), dev(w), dev(bias)
    last = xd[:, -1]
    assert not last.is_contiguous()
    M = B * HW
    assert route(last, wd, M, N, D, 0, True, lda=D, block_stride=last.stride(0))[0] == 64
    r = gb.linear_ref(x[:, -1].reshape(M, D), w, bias=bias)
    worst = {}
    y = framed_run(M, N, F32, lambda out: ops.linear_fwd_blocks(last, wd, bd, out_f32=True, out=out))
    worst['f32out'] = gb.check('f32out', y, r['ref'], r['e_in'], norm_tol=NORM_F32_OUT[dtype])
    y = framed_run(M, N, dtype, lambda out: ops.linear_fwd_blocks(last, wd, bd, out=out))
    worst['out'] = gb.check('out', y, r['ref'], r['e_in'], norm_tol=NORM[dtype])
    report(f'blocks {NAMES[dtype]} {B}x{S}x{HW}x{D}->{N}', worst)


# ---------------------------------------------------------------------------------------------- dgrad

@pytest.mark.parametrize('strided', [False, True], ids=['contiguous', 'first-third'])
@pytest.mark.parametrize('M,N,K', [(130, 136, 72), (77, 56, 24)])
@pytest.mark.parametrize('dtype', [F32, BF16], ids=NAMES.get)
def test_linear_dgrad(ops, dtype, M, N, K, strided):
    """dA = dC @ W, plain and times gelu'(z) with z across [-6, 6] (both tails of gelu')."""
    g = torch.Generator().manual_seed(19)
    dc = (torch.randn(M, N, generator=g) * 0.5 + 0.1).to(dtype)
    wt = (torch.randn(K, N, generator=g) / N ** 0.5).to(dtype)           # W^T [K, N]: the GEMM's "weight" operand
    z = (torch.rand(M, K, generator=g) * 12 - 6).to(dtype)
    z[0, 0], z[M - 1, K - 1] = -6.0, 6.0
    if strided:
        big = (torch.randn(M, 3 * N, generator=g)).to(dtype)
        big[:, :N] = dc
        dcd = dev(big)[:, :N]
        assert dcd.stride(0) == 3 * N
    else:
        dcd = dev(dc)
    wtd, zd = dev(wt), dev(z)
    worst = {}
    r = gb.linear_ref(dc, wt)
    y = framed_run(M, K, dtype, lambda out: ops.linear_dgrad(dcd, wtd, out=out))
    worst['plain'] = gb.check('plain', y, r['ref'], r['e_in'], norm_tol=NORM[dtype])
    r = gb.linear_ref(dc, wt, dgelu_z=z)
    y = framed_run(M, K, dtype, lambda out: ops.linear_dgrad(dcd, wtd, dgelu_z=zd, out=out))
    worst['dgelu'] = gb.check('dgelu', y, r['ref'], r['e_in'], norm_tol=NORM[dtype])
    # z as a row-strided view, into the unstaged epilogue as well
    z2 = dev(torch.cat([z, z], 1))[:, K:]
    y = framed_run(M, K, dtype, lambda out: ops.linear_dgrad(dcd, wtd, dgelu_z=z2, out=out), ld=K + 8 + 3)
    worst['dgelu/unstaged'] = gb.check('dgelu unstaged', y, r['ref'], r['e_in'], norm_tol=NORM[dtype])
    report(f'dgrad {NAMES[dtype]} {M}x{N}x{K} {"strided" if strided else "contiguous"}', worst)


# ---------------------------------------------------------------------------------------------- wgrad (one problem)

@pytest.mark.parametrize('pro', ['plain', 'ln', 'gelu_in'])
@pytest.mark.parametrize('N,K', [(136, 72), (56, 264)])
@pytest.mark.parametrize('dtype', [F32, BF16], ids=NAMES.get)
def test_linear_wgrad(ops, dtype, N, K, pro):
    """M: one slab minus a row, exactly one, one plus a row, one past a split of four slabs, several slices with a ragged last one
    (a slab is 64 rows in bf16, 32 in fp32).  Alternating: dc contiguous / the second half of [M, 2N]; accumulate / overwrite."""
    worst = {}
    for i, M in enumerate([63, 64, 65, 257, 1000]):
        g = torch.Generator().manual_seed(20 + i)
        dc = (torch.randn(M, N, generator=g) * 0.3).to(dtype)
        a = (torch.randn(M, K, generator=g) * 1.3 + 0.2).to(dtype)
        gam, bet = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.1
        dw0, db0 = torch.randn(N, K, generator=g), torch.randn(N, generator=g)
        dc2 = torch.randn(M, 2 * N, generator=g).to(dtype)
        dc2[:, N:] = dc
        ad = dev(a)
        ln = (gam, bet) if pro == 'ln' else None
        kw = dict(ln=(dev(gam), dev(bet)), ln_stats=ops.layernorm_stats(ad, EPS)) if pro == 'ln' else dict(gelu_in=pro == 'gelu_in')
        # the norm tolerances of test_kernels_gpu.py were set against a prologue rounded to the operand type
        nref = None
        if pro != 'plain' and dtype == BF16:
            an = gb.ln_apply(a, gam, bet, EPS, dtype)[0] if pro == 'ln' else gb.gelu64(gb.f64(a))
            nref = gb.f64(dc).t() @ an.to(dtype).double()
        for strided, over, with_bias in ((False, False, True), (True, True, True), (i % 2 == 0, i % 2 == 1, False)):
            dcd = dev(dc2)[:, N:] if strided else dev(dc)
            wbuf, dw, wmask = gb.framed_flat((N, K), F32, 'cuda')
            bbuf, db, bmask = gb.framed_flat((N,), F32, 'cuda')
            dw.copy_(dw0)
            db.copy_(db0)
            ops.linear_wgrad(dcd, ad, dw, db if with_bias else None, overwrite=over, **kw)
            torch.cuda.synchronize()
            gb.assert_untouched(wbuf.cpu(), wmask)
            gb.assert_untouched(bbuf.cpu(), bmask)
            rw, ew, rb, eb = gb.wgrad_ref(dc, a, None if over else dw0, None if over else db0, ln=ln, gelu_in=pro == 'gelu_in')
            tag = f'M{M}/{"strided" if strided else "contig"}/{"overwrite" if over else "accumulate"}'
            nr = None if nref is None else nref + (0 if over else gb.f64(dw0))
            worst[tag] = gb.check(tag, dw.cpu(), rw, ew, norm_tol=3e-5 if dtype == F32 else 2e-3, norm_ref=nr)
            if with_bias:
                worst[tag + '.b'] = gb.check(tag + '.dbias', db.cpu(), rb, eb, norm_tol=3e-5 if dtype == F32 else 2e-3)
            else:
                assert torch.equal(db.cpu(), db0), 'dbias=None: the bias gradient is not the launch\'s to write'
    report(f'wgrad {NAMES[dtype]} {N}x{K} {pro}', worst)


# ---------------------------------------------------------------------------------------------- LayerNorm

def ln_operands(M, K, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x2 = (torch.randn(M, 2 * K, generator=g) * 1.5 + 0.4).to(dtype)
    dy2 = (torch.randn(M, 2 * K, generator=g) * 0.5).to(dtype)
    sk2 = torch.randn(M, 3 * K, generator=g).to(dtype)
    gam = torch.rand(K, generator=g) + 0.5
    return x2, dy2, sk2, gam, torch.randn(K, generator=g), torch.randn(K, generator=g)


@pytest.mark.parametrize('K', [24, 256, 260, 1024])
@pytest.mark.parametrize('dtype', [F32, BF16], ids=NAMES.get)
def test_layernorm_stats(ops, dtype, K):
    """M = 4100 is past 2048 workgroups of four rows: the grid-stride loop.  x contiguous and as the second half of [M, 2K]."""
    worst = {}
    for M in (1, 7, 4100):
        x2 = ln_operands(M, K, dtype, seed=30 + M % 7)[0]
        for strided in (False, True):
            xh = x2[:, K:]
            xd = dev(x2)[:, K:] if strided else dev(xh.contiguous())
            mb, mean, mm = gb.framed_flat((M,), F32, 'cuda')
            rb, rstd, rm = gb.framed_flat((M,), F32, 'cuda')
            ops.layernorm_stats(xd, EPS, out=(mean, rstd))
            torch.cuda.synchronize()
            gb.assert_untouched(mb.cpu(), mm)
            gb.assert_untouched(rb.cpu(), rm)
            mu, e_mu, rs, e_rs = gb.ln_stats_ref(xh, EPS)
            tag = f'M{M}{"s" if strided else ""}'
            worst[tag + '.mean'] = gb.check(tag + '.mean', mean.cpu(), mu, e_mu, norm_tol=1e-5)
            worst[tag + '.rstd'] = gb.check(tag + '.rstd', rstd.cpu(), rs, e_rs, norm_tol=1e-5)
    report(f'layernorm_stats {NAMES[dtype]} K={K}', worst)


def ln_bwd_case(ops, dtype, M, K, worst, seed, strided=True):
    x2, dy2, sk3, gam, dg0, db0 = ln_operands(M, K, dtype, seed)
    x, dy, sk, skb = x2[:, K:], dy2[:, :K], sk3[:, K:2 * K], sk3[:, 2 * K:]
    if strided:
        x2d, dy2d, sk3d = dev(x2), dev(dy2), dev(sk3)
        xd, dyd, skd, skbd = x2d[:, K:], dy2d[:, :K], sk3d[:, K:2 * K], sk3d[:, 2 * K:]
    else:
        xd, dyd, skd, skbd = (dev(t.contiguous()) for t in (x, dy, sk, skb))
    gd = dev(gam)
    for tag, s, s2, sd, s2d in (('none', None, None, None, None), ('skip', sk, None, skd, None),
                                ('skip2', None, skb, None, skbd), ('both', sk, skb, skd, skbd)):
        gbuf, dg, gmask = gb.framed_flat((K,), F32, 'cuda')
        bbuf, dbt, bmask = gb.framed_flat((K,), F32, 'cuda')
        dg.copy_(dg0)
        dbt.copy_(db0)
        dx = framed_run(M, K, dtype, lambda out: ops.layernorm_bwd(xd, dyd, gd, dg, dbt, skip=sd, eps=EPS, skip2=s2d, out=out))
        gb.assert_untouched(gbuf.cpu(), gmask)
        gb.assert_untouched(bbuf.cpu(), bmask)
        r = gb.ln_bwd_ref(x, dy, gam, s, s2, dg0, db0, EPS)
        t = f'M{M}/{tag}'
        worst[t + '.dx'] = gb.check(t + '.dx', dx, r['dx'], r['e_dx'], norm_tol=1e-5 if dtype == F32 else 6e-3)
        worst[t + '.dg'] = gb.check(t + '.dgamma', dg.cpu(), r['dgamma'], r['e_dgamma'], norm_tol=3e-5)
        worst[t + '.db'] = gb.check(t + '.dbeta', dbt.cpu(), r['dbeta'], r['e_dbeta'], norm_tol=3e-5)


@pytest.mark.parametrize('K', [24, 256, 260, 512, 516, 1024])
@pytest.mark.parametrize('dtype', [F32, BF16], ids=NAMES.get)
def test_layernorm_bwd(ops, dtype, K):
    """KG = 1, 1, 2, 2, 4, 4 with a partial lane group at 24, 260 and 516; M = 1 and 7 leave the second row of a wave's pair dead;
    x, dyhat and the skips are column slices of wider buffers; dgamma / dbeta start from non-zero values."""
    worst = {}
    for M in (1, 7, 129):
        ln_bwd_case(ops, dtype, M, K, worst, seed=40 + M % 5)
    report(f'layernorm_bwd {NAMES[dtype]} K={K}', worst)


@pytest.mark.parametrize('dtype', [F32, BF16], ids=NAMES.get)
def test_layernorm_bwd_past_the_grid_cap(ops, dtype):
    """M = 16 389 at K = 24: 256 workgroups x 16 waves x 2 rows = 8 192 rows per sweep, so the outer loop runs three times and
    ends on a dead second row."""
    worst = {}
    ln_bwd_case(ops, dtype, 16389, 24, worst, seed=45, strided=False)
    report(f'layernorm_bwd {NAMES[dtype]} M=16389', worst)


def test_layernorm_bwd_refuses_k_above_1024(ops):
    from world_modelz_amd import _lib as L
    M, K = 7, 1028
    x2, dy2, sk3, gam, dg0, db0 = ln_operands(M, K, F32, seed=46)
    gbuf, dg, gmask = gb.framed_flat((K,), F32, 'cuda')
    bbuf, dbt, bmask = gb.framed_flat((K,), F32, 'cuda')
    dg.copy_(dg0)
    dbt.copy_(db0)
    buf, out, mask = gb.framed(M, K, F32, 'cuda')
    with pytest.raises(L.WmzError, match=rf'code {L.CONSTANTS["WMZ_ERR_UNSUPPORTED"]}\b.*K=1028'):
        ops.layernorm_bwd(dev(x2)[:, K:], dev(dy2)[:, :K], dev(gam), dg, dbt, out=out)
    torch.cuda.synchronize()
    gb.assert_untouched(buf.cpu(), torch.zeros_like(mask))
    assert torch.equal(dg.cpu(), dg0) and torch.equal(dbt.cpu(), db0)
    gb.assert_untouched(gbuf.cpu(), gmask)
    gb.assert_untouched(bbuf.cpu(), bmask)
