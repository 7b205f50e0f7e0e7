"""References and element-wise error bounds for the kernels at the two ends of the denoiser's training step: token corruption,
token + position embedding forward and backward (csrc/capi_core.hip, csrc/embed_bwd.hip), cross-entropy (csrc/loss.hip), the
gradient norm and AdamW (csrc/optim.hip).  A plain helper module for tests/test_tail_bounds_cpu.py and
tests/test_train_tail_gpu.py: no fixtures, nothing collected from here.  The checker, the sentinel frames and the unit round-offs
are those of tests/gemm_bounds.py.

Every reference is computed on the CPU in fp64 from the values the kernel receives, and comes with e_in: how far the kernel's
fp32 evaluation may be from the exact value, whatever order it adds in -- first-order running-error analysis, one u = 2^-24 per
fp32 operation at the size of its result, plus the propagated errors of its inputs.  gemm_bounds.check then allows
tol = e_in + u_out (|ref| + e_in) + TINY per element.  The corruption has no tolerance: its reference is the exact output.
Nothing in here comes from a GPU run; the derivations are written out in profiles/train_tail_bounds/README.md.
"""
import numpy as np
import torch

from gemm_bounds import (TINY, U32, UNIT, BoundError, assert_untouched, check, f64, framed,   # noqa: F401  (re-exported: the
                         framed_flat)                                                         # tests take them from here)

FLUSH = 2.0 ** -126         # a subnormal fp32 result flushed to zero
EXP2_ULPS = 1               # V_EXP_F32 ("base 2 exponent"), AMD Instinct CDNA3 / CDNA4 ISA reference guide: 1 ULP = 2 u
LOG_ULPS = 3                # logf: the OpenCL full-profile bound (3 ulp) the device math library is built to; HIP documents 1
DIV_SQRT_U = 2              # x / y and sqrtf in units of u: correctly rounded (1 u) as the library is built; the 1-ULP hardware
                            # forms (2 u) are covered as well
C_SUM = 8                   # fp32 operations around a long sum (scales, the partial sums' hand-over)
C_ADD = 4                   # the same around a scatter-add (the mask row's and the position tables' partial sums)


def f32(x):
    """A Python number rounded to fp32 (what a `(float)` cast of a double argument gives), as a Python float."""
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------------------- cross-entropy

def exp_err(val, a, e_a):
    """|__expf(a') - exp(a)| for val = exp(a) and |a' - a| <= e_a, with __expf(a') = exp2(fl(a' * log2e)): relative, the argument's
    error (expm1: not only to first order -- e_a reaches 1e-3 for logits around 1e4), the rounded constant log2e and the rounded
    product (each u relative on an argument of size |a| log2e: |a| u apiece in the result) and the exp2 itself; absolute, a
    subnormal result flushed.  Where exp(a) is 0 in fp64 (the -1e30 padding classes) only the flush remains."""
    rel = torch.expm1(e_a.clamp_max(80.0)) + (2 * a.abs() + 2 * EXP2_ULPS + 1) * U32
    return torch.where(val > 0, val * rel, torch.zeros_like(val)) + FLUSH


def ce_ref(logits, target, grad_rows, lse=None):
    """wmz_ce_fwd / wmz_ce_bwd / wmz_ce_fwd_bwd on logits [R, C] (the C classes only), target [R] int64, grad_rows [R]
    -> dict(loss, e_loss, lse, e_lse, dlogits, e_dlogits), fp64.
    loss is taken at the target clamped to [0, C-1]; an out-of-range target has no one-hot term in the gradient (include/wmz.h).
    lse (optional): the log-sum-exp wmz_ce_bwd is GIVEN -- an input, error-free -- ; else the gradient's p = exp(x - l) carries
    the error e_l of the l the one-pass kernel computed itself."""
    x = f64(logits)
    R, C = x.shape
    t = target.detach().cpu().long()
    g = f64(grad_rows).reshape(R, 1)
    m = x.max(-1, keepdim=True).values                         # exact in fp32: a maximum rounds nothing
    a = x - m
    e_a = U32 * a.abs()                                          # one rounding of x - m
    ex = torch.exp(a)
    e_ex = exp_err(ex, a, e_a)
    s = ex.sum(-1, keepdim=True)                                 # >= 1: the maximum's own term
    e_s = e_ex.sum(-1, keepdim=True) + (C + C_SUM) * U32 * s     # C non-negative terms in any order
    logs = torch.log(s)
    e_logs = e_s / s + 2 * LOG_ULPS * U32 * logs.abs()
    l = m + logs
    e_l = e_logs + U32 * l.abs()                                 # the rounding of m + log s: what the kernel holds and stores
    tc = t.clamp(0, C - 1)
    xt = x.gather(1, tc.reshape(R, 1))
    out = dict(lse=l[:, 0], e_lse=e_logs[:, 0], loss=(l - xt)[:, 0], e_loss=e_l[:, 0])
    if lse is not None:
        l, e_l = f64(lse).reshape(R, 1), torch.zeros(R, 1, dtype=torch.float64)
    b = x - l
    p = torch.exp(b)
    e_p = exp_err(p, b, e_l + U32 * b.abs())
    onehot = torch.zeros_like(x)
    inr = (t >= 0) & (t < C)
    onehot[inr.nonzero()[:, 0], t[inr]] = 1.0
    q = p - onehot
    e_q = e_p + U32 * q.abs()                                    # ABSOLUTE where p_target ~ 1: e_p stays ~ (e_l + 3 u) while q -> 0
    out.update(dlogits=q * g, e_dlogits=g.abs() * e_q + U32 * (q * g).abs())
    return out


# ---------------------------------------------------------------------------------------------------- AdamW and the norm

def adamw_ref(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale, e_p=None, e_m=None, e_v=None):
    """The law of wmz_adamw_step (include/wmz.h) in fp64, at the fp32 casts of the hyper-parameters the kernel takes by value:
        gi = gs g;  p *= 1 - lr wd;  m = b1 m + (1 - b1) gi;  v = b2 v + (1 - b2) gi^2;  p -= (lr / bc1) m / (sqrt(v) / sbc2 + eps)
    with bc1 = 1 - b1^step, sbc2 = sqrt(1 - b2^step) in double (the kernel receives their fp32 roundings: 1 u each, in the bound).
    e_p / e_m / e_v: what the incoming state may already be off by (compounding over steps).
    -> dict(p, e_p, m, e_m, v, e_v): the new state."""
    p, g, m, v = (f64(t) for t in (p, g, m, v))
    z = torch.zeros_like(p)
    e_p0, e_m0, e_v0 = (z if e is None else f64(e) for e in (e_p, e_m, e_v))
    lr, b1, b2, eps, wd, gs = (f32(h) for h in (lr, beta1, beta2, eps, weight_decay, grad_scale))
    bc1, sbc2 = 1.0 - beta1 ** step, (1.0 - beta2 ** step) ** 0.5
    u = U32
    gi = g * gs
    e_gi = u * gi.abs()
    dec = 1.0 - lr * wd
    e_dec = u * lr * wd + u * abs(dec)
    p0 = p * dec
    e_p0s = p.abs() * e_dec + u * p0.abs() + abs(dec) * e_p0
    om1, om2 = 1.0 - b1, 1.0 - b2                                # each one fp32 subtraction: u relative
    t1, t2 = b1 * m, om1 * gi
    mi = t1 + t2
    e_mi = 2 * u * t1.abs() + 4 * u * t2.abs() + b1 * e_m0       # products, the factor 1 - b1, gi's rounding, the sum
    s1, s2 = b2 * v, om2 * gi * gi
    vi = s1 + s2
    e_vi = 2 * u * s1.abs() + 6 * u * s2.abs() + b2 * e_v0
    r_v = torch.where(vi > 0, e_vi / vi.clamp_min(1e-300), z)    # a sum of non-negative terms: relative, and 0 at vi = 0
    sq = vi.sqrt()
    e_sq = sq * (0.5 * r_v + DIV_SQRT_U * u)
    qd = sq / sbc2
    e_qd = e_sq / sbc2 + (DIV_SQRT_U + 1) * u * qd               # the division, and sbc2's own rounding to fp32
    den = qd + eps
    e_den = e_qd + u * den
    ratio = mi / den
    e_ratio = e_mi / den + mi.abs() * e_den / (den * den) + DIV_SQRT_U * u * ratio.abs()
    stp = lr / bc1
    e_stp = (DIV_SQRT_U + 1) * u * stp                           # the division, and bc1's own rounding to fp32
    upd = stp * ratio
    e_upd = ratio.abs() * e_stp + stp * e_ratio + u * upd.abs()
    pn = p0 - upd
    e_pn = e_p0s + e_upd + u * pn.abs()
    return dict(p=pn, e_p=e_pn, m=mi, e_m=e_mi, v=vi, e_v=e_vi)


def adamw_torch_steps(p, grads, m, v, lr, beta1, beta2, eps, weight_decay, first_step, grad_scale):
    """len(grads) successive steps of torch.optim.AdamW on fp64 CPU copies, the first one being step `first_step` (state seeded
    with m, v and the step count) -- independent of the kernel's formula -- and the bound of adamw_ref compounded along them
    -> (p, e_p, m, e_m, v, e_v) after the last step."""
    P = torch.nn.Parameter(f64(p).clone())
    opt = torch.optim.AdamW([P], lr=lr, betas=(beta1, beta2), eps=eps, weight_decay=weight_decay, amsgrad=False, foreach=False)
    opt.state[P] = dict(step=torch.tensor(float(first_step - 1)), exp_avg=f64(m).clone(), exp_avg_sq=f64(v).clone())
    e_p = e_m = e_v = None
    for k, g in enumerate(grads):
        st = opt.state[P]
        r = adamw_ref(P.detach(), g, st['exp_avg'], st['exp_avg_sq'], lr, beta1, beta2, eps, weight_decay, first_step + k,
                      grad_scale, e_p, e_m, e_v)
        e_p, e_m, e_v = r['e_p'], r['e_m'], r['e_v']
        P.grad = f64(g) * grad_scale
        opt.step()
    st = opt.state[P]
    return P.detach().clone(), e_p, st['exp_avg'].clone(), e_m, st['exp_avg_sq'].clone(), e_v


def sqnorm_ref(g, scale=1.0, start=0.0):
    """start + scale^2 sum g^2 -> (value, e_in): n + 1 non-negative terms in any order, (n + c) u of their sum."""
    g = f64(g).reshape(-1)
    tot = float((g * g).sum()) * f32(scale) ** 2
    return start + tot, (g.numel() + C_SUM) * U32 * (abs(start) + tot)


# ---------------------------------------------------------------------------------------------------- embedding

def pos3d_indices(B, S, H, W):
    t = torch.arange(B * S * H * W)
    return (t // (H * W)) % S, (t // W) % H, t % W


def embed_fwd_ref(tok, si, hi, wi, emb, pos_s, pos_h, pos_w, dtype):
    """x[t] = emb[tok] + ((pos_s[s] + pos_h[h]) + pos_w[w]): three fp32 additions in that order -- IEEE additions, which the CPU
    rounds exactly as the GPU does -- then one rounding to `dtype`.  tok / si / hi / wi: per-token indices, already clamped.
    -> (x in fp32 before the last rounding, x in `dtype`): the kernel's output is expected bit for bit."""
    e, a, b, c = (t.detach().cpu().float() for t in (emb, pos_s, pos_h, pos_w))
    x = e[tok] + ((a[si] + b[hi]) + c[wi])
    return x, x.to(dtype)


def embed_bwd_ref(tok, si, hi, wi, dx, tabs0, calls=1):
    """Scatter-add of dx [ntok, D] into the four fp32 tables [emb, pos_s, pos_h, pos_w] starting from tabs0, `calls` times over:
    fp64 index_add.  Per element the bound is (count + c) u sum |terms|, count = the contributions to that element, the table's
    initial value included.  -> [(ref, e_in)] * 4."""
    f = f64(dx).reshape(len(tok), -1)
    out = []
    for idx, t0 in zip((tok, si, hi, wi), tabs0):
        t0 = f64(t0)
        ref = t0.clone().index_add_(0, idx, calls * f)
        mag = t0.abs().index_add_(0, idx, calls * f.abs())
        cnt = torch.bincount(idx, minlength=t0.shape[0]).double().reshape(-1, 1) * calls + 1
        out.append((ref, (cnt + C_ADD) * U32 * mag))
    return out


# ---------------------------------------------------------------------------------------------------- corruption

M32 = np.uint64(0xFFFFFFFF)


def philox4x32_np(index, stream, seed):
    """Philox4x32-10 on the project's keying (tests/test_philox_cpu.py: counter = (index, stream), key = seed, low word first),
    vectorised over `index` (any integer array) -> uint32 [len(index), 4]."""
    idx = np.asarray(index).astype(np.uint64).reshape(-1)
    stream, seed = int(stream) & (2 ** 64 - 1), int(seed) & (2 ** 64 - 1)
    x = [idx & M32, idx >> np.uint64(32), np.full_like(idx, stream & 0xFFFFFFFF), np.full_like(idx, stream >> 32)]
    k = [seed & 0xFFFFFFFF, seed >> 32]
    mult = (np.uint64(0xD2511F53), np.uint64(0xCD9E8D57))
    weyl = (0x9E3779B9, 0xBB67AE85)
    for r in range(10):
        if r:
            k = [(k[i] + weyl[i]) & 0xFFFFFFFF for i in range(2)]
        p0, p1 = mult[0] * x[0], mult[1] * x[2]                 # 32 x 32 bits: fits 64
        x = [(p1 >> np.uint64(32)) ^ x[1] ^ np.uint64(k[0]), p1 & M32, (p0 >> np.uint64(32)) ^ x[3] ^ np.uint64(k[1]), p0 & M32]
    return np.stack(x, -1).astype(np.uint32)


def corrupt_ref(z_last, r, C, seed, stream):
    """wmz_corrupt_tokens, exactly: z_last [B, HW] int64, r [B] fp32 -> out [B, HW] int64.  Per flat index i = b * HW + p the
    block philox4x32(i, stream, seed); u_k = (word_k >> 8) / 2^24; redraw iff u0 < fl32(r[b] * 0.1f), the redrawn code
    min(int(fl32(u1 * C)), C - 1); mask (token C) iff u2 < r[b]."""
    z = z_last.detach().cpu().long().numpy()
    B, HW = z.shape
    rb = np.repeat(r.detach().cpu().numpy().astype(np.float32), HW)
    w = philox4x32_np(np.arange(B * HW), stream, seed)
    u = (w >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)          # exact: 24 bits
    out = z.reshape(-1).copy()
    redraw = u[:, 0] < rb * np.float32(0.1)
    k = np.minimum((u[:, 1] * np.float32(C)).astype(np.int64), C - 1)
    out[redraw] = k[redraw]
    out[u[:, 2] < rb] = C
    return torch.from_numpy(out.reshape(B, HW))


# ---------------------------------------------------------------------------------------------------- the cases both test files run

CE_CLASSES = [1, 3, 50, 255, 257, 1024, 1025, 1030, 2048, 2049, 4096, 4097, 8192, 8193, 9001]     # every NCH boundary of the one-pass kernel
CE_REGIME_CLASSES = [50, 2049, 8192]             # NCH = 4, 16 and 32
CE_REGIMES = ['randn3', 'randn30', 'shift1e4', 'equal', 'tied', 'pad1', 'pad7']
ADAMW_N = [1, 2, 3, 4, 5, 2047, 2049, 524288 * 2 + 6147, 4194304 + 2051]
ADAMW_HYPER = dict(lr=f32(1e-3), beta1=f32(0.9), beta2=f32(0.999), eps=f32(1e-8))     # fp32-representable: kernel and torch get the same


def ce_rows(C):
    """R in 5..37, another one per class count."""
    return 5 + (C * 7) % 33


def ce_case(R, C, regime='randn3', seed=0):
    """(logits [R, C] fp32, target [R] int64 -- 0, C-1, -1, C, 2^32 + 1 on the first rows, in range behind --, grad_rows [R])."""
    g = torch.Generator().manual_seed(1000 * seed + C + R)
    x = torch.randn(R, C, generator=g) * 3
    if regime == 'randn30':
        x = x * 10                                              # peaked rows: p_target - 1 cancels
    elif regime == 'shift1e4':
        x = x + 1e4
    elif regime == 'equal':
        x = torch.randn(R, 1, generator=g).expand(R, C).contiguous()
    elif regime == 'tied':
        x[:, torch.randperm(C, generator=g)[:min(C, 3)]] = 7.5     # three classes share the maximum
    elif regime.startswith('pad'):
        x[:, C - min(int(regime[3:]), C - 1):] = -1e30          # _LinearCrossEntropy's padding classes: probability exactly 0
    t = torch.randint(0, C, (R,), generator=g)
    if regime == 'randn30':
        t[R // 2:] = x[R // 2:].argmax(-1)                      # half the rows aim at the peak
    if regime.startswith('pad'):
        t = t.clamp_max(C - 1 - min(int(regime[3:]), C - 1))
    else:
        for i, v in enumerate((0, C - 1, -1, C, 2 ** 32 + 1)):
            t[i] = v
    return x, t, torch.rand(R, generator=g) + 0.05


ADAMW_PERIOD = 4099        # prime: the arenas past the grid caps repeat a pool of this length, so their fp64 reference is computed
                           # once per pool element and tiled (an element-wise law); no tile, sweep or grid stride divides it


def tile(t, n):
    """t repeated to length n."""
    return t.repeat(-(-n // t.numel()))[:n].clone()


def adamw_case(n, seed=0):
    """(p, g, m, v) fp32 [n]: gradients over 1e-8 .. 1e3 in magnitude, non-zero moments, and every 7th element at g = m = v = 0.
    n > ADAMW_PERIOD: the case of ADAMW_PERIOD elements, tiled."""
    if n > ADAMW_PERIOD:
        return tuple(tile(t, n) for t in adamw_case(ADAMW_PERIOD, seed))
    gen = torch.Generator().manual_seed(77 + seed + n % 1000)
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen).sign() * 10 ** (torch.rand(n, generator=gen) * 11 - 8)
    m = torch.randn(n, generator=gen) * 0.1 * g.abs()
    v = (torch.rand(n, generator=gen) + 0.01) * g * g
    zero = torch.arange(n) % 7 == 3
    g[zero], m[zero], v[zero] = 0.0, 0.0, 0.0
    return p, g, m, v


def embed_case(ntok, D, classes, dtype, seed=0, rows=(1, 1, 1)):
    """(tok [ntok] with half the tokens on the mask class (the table's last row) and two ids out of range, dx [ntok, D] in `dtype`,
    the four non-zero starting tables: classes / rows[0] / rows[1] / rows[2] rows)."""
    gen = torch.Generator().manual_seed(500 + seed + ntok + D)
    tok = torch.randint(0, classes, (ntok,), generator=gen)
    tok[torch.rand(ntok, generator=gen) < 0.5] = classes - 1
    if ntok > 2:
        tok[0], tok[ntok // 2] = -5, classes + 9                # clamped to 0 / classes - 1
    dx = torch.randn(ntok, D, generator=gen).to(dtype)
    tabs0 = [torch.randn(n, D, generator=gen) for n in (classes,) + tuple(rows)]
    return tok, dx, tabs0
