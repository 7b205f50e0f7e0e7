"""Element-wise error bounds for the convolution kernel family (csrc/conv2d.hip, conv_direct.hip, conv_point.hip and their half
units, conv_wgrad.hip, the implicit weight gradient of csrc/linear_bwd.hip) and the table of cases both
tests/test_conv_family_gpu.py (on the kernels) and tests/test_conv_bounds_cpu.py (on an fp32 emulation) run.  A plain helper
module next to tests/gemm_bounds.py, whose checker, sentinel frames and constants it reuses: no fixtures, nothing collected.

Every reference is computed on the CPU in fp64 from the operand values the kernel receives.  Every output element gets

    tol = e_in + u_out * (|ref| + e_in) + TINY                                   (gemm_bounds.check: no element left out)

where e_in does not depend on the order the kernel adds in: (n + C_OPS) * 2^-24 * sum |terms| for a sum of n terms with the
epilogue's operations around it, plus the first-order propagated error of an input prologue.  Nothing in here comes from a GPU
run; the derivations are written out in profiles/conv_family_bounds/README.md.
"""
import torch
import torch.nn.functional as F

from gemm_bounds import C_OPS, U32, UNIT, f64

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
NAMES = {F32: 'fp32', BF16: 'bf16', F16: 'fp16'}
REPLICAS = 8                # include/wmz.h WMZ_STAT_REPLICAS: rows of a statistics tensor


def f32_value(v):
    """The value a `float` kernel argument holds for the Python number v (slopes, eps)."""
    return float(torch.tensor(v, dtype=torch.float32))


def out_hw(Hi, Wi, k, stride, pad):
    return (Hi + 2 * pad - k) // stride + 1, (Wi + 2 * pad - k) // stride + 1


# ---------------------------------------------------------------------------------------------------- fp64 building blocks

def conv64(x, w_op, KH, KW, stride, pad):
    """x [B, H, W, Cin], w_op [Cout, KH * KW * Cin] (tap-major, channel fastest: the GEMM operand) -> fp64 [B, Ho, Wo, Cout]."""
    X = f64(x).permute(0, 3, 1, 2)
    Cin, Cout = X.shape[1], w_op.shape[0]
    W4 = f64(w_op).view(Cout, KH, KW, Cin).permute(0, 3, 1, 2)
    return F.conv2d(X, W4, None, stride=stride, padding=pad).permute(0, 2, 3, 1).contiguous()


def leaky64(v, slope):
    return torch.where(v > 0, v, v * f32_value(slope))


def bn_fold_ref(s, q, count, gamma, beta, eps):
    """bn_channel of csrc/bn_lazy.h from the raw statistics s, q [REPLICAS, C] AS THE KERNEL RECEIVES THEM: fp64 values of
    mean, rstd, scale = gamma rstd, shift = beta - mean gamma rstd and how far its fp32 evaluation can be off (e_*, absolute).
    var = sq / n - mean^2 is a difference of two rounded numbers: its absolute error u (sq / n + 3 mean^2 + ..) stays however
    small var is -- the cancellation term -- and reaches scale and shift through rstd as e_v / (2 (var + eps))."""
    S, Q = f64(s), f64(q)
    R = S.shape[0]
    n = float(count)
    assert n < 2 ** 24                                     # (float)count is exact
    s1, s2 = S.sum(0), Q.sum(0)
    e_s1, e_s2 = R * U32 * S.abs().sum(0), R * U32 * Q.abs().sum(0)
    mean = s1 / n
    e_mean = e_s1 / n + U32 * (mean.abs() + e_s1 / n)
    t = s2 / n
    e_t = e_s2 / n + U32 * (t.abs() + e_s2 / n)
    m2 = mean * mean
    e_m2 = 2 * mean.abs() * e_mean + e_mean * e_mean + U32 * (m2 + 2 * mean.abs() * e_mean)
    raw = t - m2
    e_var = e_t + e_m2 + U32 * (raw.abs() + e_t + e_m2)    # (a contracted fma rounds once less)
    var = raw.clamp_min(0.0)                               # fmaxf(.., 0): 1-Lipschitz
    v = var + f32_value(eps)
    e_v = e_var + U32 * (v + e_var)
    rs = v.rsqrt()
    # (v - e)^-1/2 / v^-1/2 - 1 <= e / (2 (v - e)); 2 u: the hardware's rsqrt
    r_rs = torch.where(v > e_v, 0.5 * e_v / (v - e_v).clamp_min(1e-300), torch.full_like(v, float('inf'))) + 2 * U32
    g = f64(gamma) if gamma is not None else torch.ones_like(rs)
    b = f64(beta) if beta is not None else torch.zeros_like(rs)
    sc = g * rs
    e_sc = sc.abs() * ((1 + r_rs) * (1 + U32) - 1)
    p = mean * g * rs                                      # (mean * g) * rs
    e_p = (g * rs).abs() * e_mean * (1 + r_rs) * (1 + 2 * U32) + p.abs() * ((1 + r_rs) * (1 + U32) ** 2 - 1)
    sh = b - p
    e_sh = e_p + U32 * (sh.abs() + e_p)
    return dict(mean=mean, e_mean=e_mean, rstd=rs, e_rstd=rs * r_rs, scale=sc, e_scale=e_sc, shift=sh, e_shift=e_sh)


def prologue(x, in_scale, in_shift, slope, op_dtype, e_scale=None, e_shift=None):
    """A' = round_op(LeakyReLU(x * in_scale + in_shift)) as a 1x1 layer's input prologue hands it to the matrix cores
    -> (A fp64 unrounded, e_A per element): one fma, the slope's multiplication (LeakyReLU with slope in [0, 1] is 1-Lipschitz),
    the errors of scale / shift themselves (raw statistics: bn_fold_ref) and the rounding to the operand type (0 for fp32)."""
    X, sc, sh = f64(x), f64(in_scale), f64(in_shift)
    y = X * sc + sh
    e = torch.zeros_like(y)
    if e_scale is not None:
        e = X.abs() * f64(e_scale) + f64(e_shift)
    e = e + U32 * (y.abs() + e)
    a = leaky64(y, slope)
    e = e + U32 * (a.abs() + e)
    u_op = 0.0 if op_dtype == F32 else UNIT[op_dtype]
    return a, e + u_op * (a.abs() + e)


# ---------------------------------------------------------------------------------------------------- references

def conv_parts(x, w_op, KH, KW, stride, pad, pre=None):
    """The convolution in front of an epilogue, once for every epilogue of a case -> (conv(A, w), conv(|A|, |w|), conv(e_A, |w|)
    or None, K): A = x, or pre = (A, e_A) of prologue()."""
    A = f64(x) if pre is None else pre[0]
    Wa = f64(w_op).abs()
    return (conv64(A, w_op, KH, KW, stride, pad), conv64(A.abs(), Wa, KH, KW, stride, pad),
            None if pre is None else conv64(pre[1], Wa, KH, KW, stride, pad), KH * KW * x.shape[-1])


def epilogue_ref(parts, bias=None, scale=None, shift=None, residual=None, leaky=False, slope=0.01):
    """act(((conv + bias) * scale + shift) + residual) -> dict(ref, e_in, pre).
    terms = (conv(|A|, |w|) + |bias|) |scale| + |shift| + |residual|, e_in = (K + C_OPS) u terms with K = KH KW Cin (however
    many channel passes or slabs the kernel adds them in), plus e_A carried through |w| and |scale|."""
    acc, terms, e_a, K = parts
    v = acc
    if bias is not None:
        v, terms = v + f64(bias), terms + f64(bias).abs()
    if scale is not None:
        sc, sh = f64(scale), f64(shift)
        v, terms = v * sc + sh, terms * sc.abs() + sh.abs()
        e_a = None if e_a is None else e_a * sc.abs()
    if residual is not None:
        v, terms = v + f64(residual), terms + f64(residual).abs()
    e = (K + C_OPS) * U32 * terms
    if e_a is not None:
        e = e + (1 + (K + C_OPS) * U32) * e_a
    return dict(ref=leaky64(v, slope) if leaky else v, e_in=e, pre=acc)


def conv_fwd_ref(x, w_op, KH, KW, stride, pad, pre=None, **epilogue):
    return epilogue_ref(conv_parts(x, w_op, KH, KW, stride, pad, pre), **epilogue)


def stats_ref(y):
    """The statistics side outputs: per-channel sum and sum of squares of the STORED output y [.., C], replicas added
    -> (sum, e_sum, sq, e_sq).  The kernels accumulate the stored, rounded value (re-read from the packed word), so the terms
    are exact numbers: only the M additions (and the square's rounding) remain."""
    Y = f64(y).reshape(-1, y.shape[-1])
    M = Y.shape[0]
    return Y.sum(0), (M + C_OPS) * U32 * Y.abs().sum(0), (Y * Y).sum(0), (M + C_OPS + 1) * U32 * (Y * Y).sum(0)


def stats_got(s):
    """[REPLICAS, C] fp32 partial sums -> their fp64 sum, as one fp32 number per channel (that rounding is check()'s u_out)."""
    return f64(s).sum(0).float()


def conv_wgrad_ref(x, dy, KH, KW, stride, pad, dw0=None, db0=None, times=1):
    """dW [Cout, KH KW Cin] = dW0 + times * dy^T im2col(x), dbias = db0 + times * colsum(dy) -> (dw, e_dw, db, e_db).
    times = 2: the accumulating call made twice.  e = (times M + C_OPS) u (times |dy|^T im2col(|x|) + |dW0|), M = B Ho Wo."""
    X, DY = f64(x).permute(0, 3, 1, 2), f64(dy).permute(0, 3, 1, 2)
    Cin, Cout = X.shape[1], DY.shape[1]
    M = DY.shape[0] * DY.shape[2] * DY.shape[3]
    size = (Cout, Cin, KH, KW)
    g = torch.nn.grad.conv2d_weight(X, size, DY, stride=stride, padding=pad).permute(0, 2, 3, 1).reshape(Cout, -1)
    t = torch.nn.grad.conv2d_weight(X.abs(), size, DY.abs(), stride=stride, padding=pad).permute(0, 2, 3, 1).reshape(Cout, -1)
    dw, terms = times * g, times * t
    db, tb = times * DY.sum((0, 2, 3)), times * DY.abs().sum((0, 2, 3))
    if dw0 is not None:
        dw, terms = dw + f64(dw0), terms + f64(dw0).abs()
    if db0 is not None:
        db, tb = db + f64(db0), tb + f64(db0).abs()
    n = times * M + C_OPS
    return dw, n * U32 * terms, db, n * U32 * tb


def conv_layout(dw, KH, KW, co, ci):
    """[Cout, KH KW Cin] (GEMM layout) -> nn.Conv2d's [co, ci, KH, KW]: channel padding cropped, taps transposed."""
    Cout = dw.shape[0]
    return dw.view(Cout, KH, KW, -1)[:co, :, :, :ci].permute(0, 3, 1, 2).contiguous()


def gemm_layout(w):
    """nn.Conv2d's [co, ci, KH, KW] -> [co, KH KW ci]"""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def dilate_ref(dy, Hz, Wz, stride):
    B, Ho, Wo, C = dy.shape
    dz = torch.zeros((B, Hz, Wz, C), dtype=dy.dtype)
    dz[:, 0:(Ho - 1) * stride + 1:stride, 0:(Wo - 1) * stride + 1:stride] = dy.cpu()
    return dz


def dgrad_plane(Hi, Wi, Ho, Wo, k, stride, pad):
    """(Hz, Wz) of the zero-inserted plane the data gradient runs on: the dilated gradient plus the output padding."""
    return ((Ho - 1) * stride + 1 + Hi - ((Ho - 1) * stride - 2 * pad + k), (Wo - 1) * stride + 1 + Wi - ((Wo - 1) * stride - 2 * pad + k))


def flipped_operand(weight, dtype):
    """autoencoder._wT_op's operand on the host: w'[ci, kh', kw', co] = w[co, ci, k-1-kh', k-1-kw'] as [Ci8, k k Co8]."""
    co, ci = weight.shape[:2]
    wt = weight.flip(2, 3).permute(1, 2, 3, 0)
    wt = F.pad(wt, (0, -co % 8, 0, 0, 0, 0, 0, -ci % 8))
    return wt.reshape(ci + -ci % 8, -1).to(dtype).contiguous()


def dgrad_ref(dy, wt_op, k, stride, pad, Hi, Wi, dskip=None):
    """dx = conv(dilate(dy), flipped operand, stride 1, pad k - 1 - pad) + dskip: the forward reference on the data gradient's
    operands -> dict(ref, e_in)."""
    Ho, Wo = dy.shape[1:3]
    dz = dy.cpu() if stride == 1 else dilate_ref(dy, *dgrad_plane(Hi, Wi, Ho, Wo, k, stride, pad), stride)
    return conv_fwd_ref(dz, wt_op, k, k, 1, k - 1 - pad, residual=dskip)


def dgrad_autograd64(dy, weight, stride, pad, Hi, Wi):
    """fp64 autograd of F.conv2d for the same values: dy [B, Ho, Wo, Co8] (padding channels ignored), weight [co, ci, k, k]
    -> dx [B, Hi, Wi, Ci8] (padding channels zero)."""
    co, ci = weight.shape[:2]
    x = torch.zeros((dy.shape[0], ci, Hi, Wi), dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, f64(weight), None, stride=stride, padding=pad)
    (y * f64(dy)[..., :co].permute(0, 3, 1, 2)).sum().backward()
    return F.pad(x.grad.permute(0, 2, 3, 1), (0, -ci % 8)).contiguous()


# ---------------------------------------------------------------------------------------------------- operands

def fwd_operands(case, dtype, seed):
    """case = (B, H, W, Cin, Cout, k, stride, pad, ...) -> dict of host tensors: x (|mean| of the order of its deviation),
    w (scaled by K^-1/2), bias, scale, shift, residual, in_scale, in_shift."""
    B, H, W, Cin, Cout, k, stride, pad = case[:8]
    g = torch.Generator().manual_seed(seed)
    K = k * k * Cin
    Ho, Wo = out_hw(H, W, k, stride, pad)
    x = (torch.randn(B, H, W, Cin, generator=g) * 0.7 + 0.2).to(dtype)
    w = (torch.randn(Cout, K, generator=g) / K ** 0.5).to(dtype)
    return dict(x=x, w=w, bias=torch.randn(Cout, generator=g), scale=torch.rand(Cout, generator=g) + 0.5,
                shift=torch.randn(Cout, generator=g), residual=torch.randn(B, Ho, Wo, Cout, generator=g).to(dtype),
                in_scale=torch.rand(Cin, generator=g) + 0.5, in_shift=torch.randn(Cin, generator=g) * 0.3,
                gamma=torch.rand(Cin, generator=g) + 0.5, beta=torch.randn(Cin, generator=g) * 0.3)


def wgrad_operands(case, dtype, seed):
    B, H, W, Cin, Cout, k, stride, pad = case[:8]
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = out_hw(H, W, k, stride, pad)
    return dict(x=(torch.randn(B, H, W, Cin, generator=g) * 0.7 + 0.2).to(dtype),
                dy=(torch.randn(B, Ho, Wo, Cout, generator=g) * 0.5 + 0.1).to(dtype),
                dw0=torch.randn(Cout, k * k * Cin, generator=g), db0=torch.randn(Cout, generator=g))


def crop(Cout, Cin):
    """The (co, ci) an nn.Conv2d of these padded sizes could have: 125 of 128, 61 of 64, 3 of 8."""
    return (Cout - 3 if Cout > 8 else 3), (Cin - 3 if Cin > 8 else 3)


def epilogues(o, residual=True):
    """Every epilogue combination the models use -> [(tag, kwargs of host tensors, stats)]."""
    out = [('none', {}, False), ('bias+leaky+stats', dict(bias=o['bias'], leaky=True), True),
           ('affine+leaky', dict(scale=o['scale'], shift=o['shift'], leaky=True), False), ('stats', {}, True)]
    if residual:
        out += [('bias+affine+res', dict(bias=o['bias'], scale=o['scale'], shift=o['shift'], residual=o['residual']), False),
                ('res', dict(residual=o['residual']), False)]
    else:
        out += [('bias+affine', dict(bias=o['bias'], scale=o['scale'], shift=o['shift']), False)]
    return out


# ---------------------------------------------------------------------------------------------------- one case, every epilogue

def forward_case(case, dtype, o, run, residual=True, pre=None, norm_tol=None, only=None):
    """Every epilogue of a forward case, each result element-wise under its bound (and under norm_tol), the statistics side
    outputs against the stored result.  run(kwargs of host tensors, stats) -> (y, sum, sq) host tensors: the kernel
    (tests/test_conv_family_gpu.py) or its fp32 emulation (tests/test_conv_bounds_cpu.py).  pre: (A, e_A) of prologue().
    -> {tag: largest error-to-bound ratio}."""
    from gemm_bounds import check
    B, H, W, Cin, Cout, k, stride, pad = case[:8]
    parts = conv_parts(o['x'], o['w'], k, k, stride, pad, pre)
    worst = {}
    for tag, kw, stats in epilogues(o, residual):
        if only is not None and tag not in only:
            continue
        r = epilogue_ref(parts, **kw)
        y, s, q = run(kw, stats)
        assert y.dtype == dtype and tuple(y.shape) == tuple(r['ref'].shape), (tag, y.dtype, y.shape)
        worst[tag] = check(tag, y, r['ref'], r['e_in'], norm_tol=norm_tol)
        if stats:
            rs, es, rq, eq = stats_ref(y)
            worst[tag + '.sum'] = check(tag + '.sum', stats_got(s), rs, es)
            worst[tag + '.sq'] = check(tag + '.sq', stats_got(q), rq, eq)
    return worst


def report(tag, worst):
    print(f'[bound] {tag}: ' + ' '.join(f'{k}={v:.3f}' for k, v in worst.items()) + f' | max {max(worst.values()):.3f}')
    assert max(worst.values()) <= 1.0


# ---------------------------------------------------------------------------------------------------- the cases
# forward cases: (B, H, W, Cin, Cout, k, stride, pad, prologue): prologue None | 'affine' (in_scale / in_shift) | 'raw' (BnLazy)

# conv2d_kernel<T, TALL>: TALL (256 x 64 tile) at Cout <= 64, else 128 x 128
GEMM_CASES = [
    (2, 9, 11, 8, 136, 3, 1, 1, None),        # 128 x 128: second column tile of 8 columns, M = 198: ragged last row tile; K = 72
    (2, 9, 11, 24, 136, 3, 1, 1, None),       # K = 216
    (3, 10, 11, 8, 40, 3, 1, 1, None),        # 256 x 64: M = 330
    (3, 10, 11, 8, 8, 3, 1, 1, None),
    (2, 15, 17, 8, 40, 3, 2, 1, None),        # stride 2 on an odd plane
    (2, 15, 17, 8, 136, 3, 2, 1, None),
    (2, 10, 12, 16, 136, 2, 2, 0, None),      # 2x2 / stride 2
    (2, 10, 12, 16, 8, 2, 2, 0, None),
    (2, 8, 8, 160, 128, 1, 1, 0, 'affine'),   # wider than the streaming kernel's prologue: 'gemm' with the direct kernels on
    (2, 8, 8, 160, 40, 1, 1, 0, 'affine'),
]

# convr_kernel<NCB, TW, NPASS, STRIDE>: NCB 1 / 2 / 4 at Cout <= 32 / <= 64 / <= 128, TW 32 at W % 32 == 0 else 16 (W = 16),
# NPASS = Cin / 64; stride 2: <4, 16, NPASS, 2>
DIRECT_COUT = {1: (8, 32), 2: (40, 64), 4: (72, 128)}
DIRECT_PLANES = {32: ((8, 32), (16, 64)), 16: ((16, 16), (32, 16))}
DIRECT_CASES = ([(3, *DIRECT_PLANES[tw][i ^ (cin == 128)], cin, DIRECT_COUT[ncb][i], 3, 1, 1, None)
                 for ncb in (1, 2, 4) for tw in (32, 16) for cin in (64, 128) for i in (0, 1)]
                + [(3, h, w, cin, 128, 3, 2, 1, None) for cin in (64, 128) for (h, w) in ((16, 32), (32, 64))])


def direct_instantiation(case):
    """(NCB, tile width, channel passes, stride) of the convr_kernel the host rule of csrc/conv_direct.hip launches for a case."""
    B, H, W, Cin, Cout, k, stride, pad = case[:8]
    if stride == 2:
        return 4, 16, Cin // 64, 2
    return (1 if Cout <= 32 else 2 if Cout <= 64 else 4), (32 if W >= 32 else 16), Cin // 64, 1


# convp_kernel<NCB, NPB, PAD>: <2, 2, .> (runs of 64 pixels) at Cout <= 64, <4, 1, .> (runs of 32) above; PAD = pad > 0
POINT_CASES = ([(1, 8, 8, 8, 8, 1, 1, 0, None)]                                                  # the smallest K, exactly one run
               + [(2, 8, 8, 128, co, 1, 1, 0, pre) for co in (64, 128) for pre in (None, 'affine', 'raw')]
               + [(2, 16, 16, 64, 64, 2, 2, 0, None),                                            # K = 256: the cap
                  (1, 8, 8, 8, 128, 3, 1, 1, None), (2, 16, 16, 16, 40, 3, 2, 1, None)])
# persistent: more runs than the 512 workgroups x 4 waves of the largest grid, so some wave takes a second run
POINT_PERSISTENT = [(683, 12, 16, 8, 8, 1, 1, 0, None), (342, 12, 16, 8, 72, 1, 1, 0, None)]


def point_runs(case):
    """(runs, waves of the launch) by the grid rule of wmz_conv_point_fwd_bn: runs of 64 pixels at Cout <= 64, of 32 above; 256
    workgroups per resident workgroup of a CU (two while the LDS image stays within 80 KB), never more than the runs need."""
    B, H, W, Cin, Cout, k, stride, pad = case[:8]
    Ho, Wo = out_hw(H, W, k, stride, pad)
    ncb = 2 if Cout <= 64 else 4
    runs = B * Ho * Wo // (64 if ncb == 2 else 32)
    lds = (k * k * Cin + 63) // 64 * 4 * ncb * 1024 + 1024 + 4 * 64 * 144
    grid = min(256 * (2 if lds <= 81920 else 1), (runs + 3) // 4)
    return runs, 4 * grid


# data gradient: (B, Hi, Wi, ci, co, k, stride, pad) of the nn.Conv2d (channel counts unpadded)
DGRAD_CASES = [(2, 9, 11, 8, 40, 3, 1, 1), (2, 16, 15, 8, 16, 3, 2, 1),        # output padding 1 in h, 0 in w
               (2, 11, 12, 8, 8, 2, 2, 0), (2, 8, 8, 16, 40, 1, 1, 0), (1, 8, 8, 3, 16, 3, 1, 1), (1, 8, 8, 16, 3, 3, 1, 1)]

# weight gradient: (B, H, W, Cin, Cout, k, stride, pad), channels padded; the six geometries of test_conv_backward_kernels_vs_torch
WGRAD_IMPLICIT = [(2, 9, 11, 8, 40, 3, 1, 1), (1, 16, 16, 24, 16, 3, 2, 1), (2, 8, 8, 16, 136, 1, 1, 0), (2, 10, 6, 8, 8, 2, 2, 0),
                  (1, 8, 8, 8, 16, 3, 1, 1), (1, 8, 8, 16, 8, 3, 1, 1)]
# convw_kernel<NCOB>: 4 at Cout = 128, 1 at Cout <= 32 (bf16, 3x3 / stride 1 / pad 1, Cin 64 or 128, H % 8 == 0, W % 16 == 0)
WGRAD_DIRECT = [(1, 8, 16, 64, 128, 3, 1, 1), (1, 16, 32, 128, 128, 3, 1, 1), (1, 8, 16, 128, 8, 3, 1, 1),
                (1, 16, 32, 64, 24, 3, 1, 1), (1, 8, 16, 64, 32, 3, 1, 1), (1, 16, 32, 128, 32, 3, 1, 1),
                (70, 16, 32, 64, 128, 3, 1, 1), (70, 16, 32, 128, 8, 3, 1, 1)]          # 280 tiles: more than one per workgroup
# one wmz_conv2d_nhwc_wgrad_batch call: (case, overwrite, nn.Conv2d layout, dbias)
WGRAD_BATCH = [((2, 8, 8, 16, 136, 1, 1, 0), False, False, True), ((2, 10, 6, 8, 8, 2, 2, 0), False, True, False),
               ((1, 16, 16, 24, 16, 3, 2, 1), True, False, True)]


def case_id(c):
    B, H, W, Cin, Cout, k, stride, pad = c[:8]
    pre = f'-{c[8]}' if len(c) > 8 and c[8] else ''
    return f'{B}x{H}x{W}x{Cin}-{Cout}-k{k}s{stride}p{pad}{pre}'
