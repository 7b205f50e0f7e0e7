"""Element-wise error bounds for the nn.Linear / LayerNorm kernel family (csrc/linear_fwd.hip, csrc/linear_bwd.hip), and the
sentinel frame that shows a kernel wrote only inside its output.  A plain helper module for tests/test_linear_family_gpu.py,
tests/test_gemm_bounds_cpu.py and tests/test_kernels_gpu.py: no fixtures, nothing collected from here.

Every reference is computed on the CPU in fp64 from the operand values the kernel receives (already rounded to the operand
type).  Every output element gets its own tolerance

    tol = e_in + u_out * (|ref| + e_in) + TINY

u_out: unit round-off of the output type (one rounding of a value that is within e_in of ref).  e_in bounds what the kernel's
fp32 evaluation may differ from the exact value by, whatever order it adds in: the running-error bound (n + c) * 2^-24 *
sum |terms| of a sum of n terms with c further fp32 operations around it, plus -- where an operation has them -- the
first-order propagated errors of its inputs (the rounding of a prologue's result to the operand type, the cancellation in
x - mean, the documented error of the erf / fitted GELU).  Nothing in here comes from a GPU run; the derivations are written
out in profiles/linear_family_bounds/README.md.
"""
import math

import torch

U32 = 2.0 ** -24
UNIT = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
# the absolute floor of a tolerance: fp32 subnormal intermediates flushed to zero (at most n * 2^-126, n < 2^26), and half the
# smallest subnormal of the output type where that is larger (IEEE half: results below 2^-14 round on a fixed grid of 2^-24)
TINY = {torch.float32: 2.0 ** -100, torch.bfloat16: 2.0 ** -100, torch.float16: 2.0 ** -25}
C_OPS = 8                   # fp32 operations around a sum: bias, residual, scale, fused multiply-adds of an epilogue
GELU_LIPSCHITZ = 1.13       # max |gelu'| = 1.1290
ERF_ERR = 1.5e-7 + 13 * U32     # wmz_common.h: |erf error| <= 1.5e-7 for the formula; its fp32 evaluation adds: the argument's
                                # rounding (erf'(x) x <= 0.5: 1 u), rcp (2 u), four fma of the polynomial with coefficients
                                # <= 1.46 and |t| <= 1 (6 u), p * t * exp (3 u), 1 - .. (1 u)
GELU_FAST_ERR = 2.6e-5      # wmz_common.h: max |wmz_gelu_fast - exact-erf GELU| over [-9, 9], absolute
SENTINEL = 0x7E             # every byte of a frame: bf16 / fp32 8.4e37, half NaN -- never a result


def f64(t):
    return t.detach().cpu().double()


def gelu64(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def dgelu64(v):
    return 0.5 * (1.0 + torch.erf(v / math.sqrt(2.0))) + v * torch.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)


def gelu_err(v, e_v):
    """|kernel gelu(v') - gelu(v)| for |v' - v| <= e_v: Lipschitz, the erf error, three roundings of 0.5 * v * (1 + erf)."""
    return GELU_LIPSCHITZ * e_v + 0.5 * (v.abs() + e_v) * ERF_ERR + 3 * U32 * (gelu64(v).abs() + e_v)


def dgelu_err(z):
    """|wmz_dgelu(z) - gelu'(z)| for an exact z: the erf error halved, exp of an argument rounded at z^2 / 2, three roundings."""
    phi = z.abs() * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    return 0.5 * ERF_ERR + (z * z + 6) * U32 * phi + 3 * U32 * dgelu64(z).abs()


# ---------------------------------------------------------------------------------------------------- LayerNorm pieces

def ln_parts(x, eps):
    """fp64 statistics of the rows of x [M, K] and how far an fp32 two-pass evaluation (any summation order) can be off:
    dict with mean, rstd, xhat and the bounds e_mean (absolute), r_rstd (RELATIVE), e_xhat (absolute, per element)."""
    x = f64(x)
    K = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(-1, keepdim=True)
    rstd = (var + eps).rsqrt()
    xhat = d * rstd
    # mean: K additions and one division
    e_mean = (K + 2) * U32 * x.abs().mean(-1, keepdim=True)
    # d = x - mean': the mean's error and one rounding at the size of the operands
    e_d = e_mean + U32 * (x.abs() + mean.abs())
    # var' = sum d'^2 / K + eps: K + 3 operations on non-negative terms, and 2 |d| e_d per term
    e_var = (K + 4) * U32 * (var + eps) + 2 * (d.abs() * e_d).mean(-1, keepdim=True) + (e_d * e_d).mean(-1, keepdim=True)
    # rsqrt: half the relative error of its argument, and 2 u of the hardware approximation
    r_rstd = 0.5 * e_var / (var + eps) + 2 * U32
    e_xhat = rstd * e_d + xhat.abs() * r_rstd + 2 * U32 * xhat.abs()
    return dict(mean=mean, rstd=rstd, xhat=xhat, e_mean=e_mean, r_rstd=r_rstd, e_xhat=e_xhat, e_d=e_d)


def ln_stats_ref(x, eps):
    """wmz_layernorm_stats -> (mean, e_mean, rstd, e_rstd), each [M]."""
    p = ln_parts(x, eps)
    return (p['mean'][:, 0], (p['e_mean'] + U32 * p['mean'].abs())[:, 0], p['rstd'][:, 0], (p['rstd'] * p['r_rstd'])[:, 0])


def ln_apply(x, gamma, beta, eps, op_dtype):
    """LN(x) * gamma + beta as a GEMM prologue hands it to the matrix cores -> (y fp64 unrounded, e_y): e_y holds the fp32
    evaluation and the rounding of the result to the operand type (0 for fp32 operands)."""
    p = ln_parts(x, eps)
    g, b = f64(gamma), f64(beta)
    y = p['xhat'] * g + b
    e = g.abs() * p['e_xhat'] + 3 * U32 * ((p['xhat'] * g).abs() + b.abs())
    u_op = 0.0 if op_dtype == torch.float32 else UNIT[op_dtype]
    return y, e + u_op * (y.abs() + e)


def gelu_apply(x, op_dtype, fast=False):
    """GELU(x) as a GEMM prologue hands it over -> (y, e_y).  fast: the fitted form (wmz_gelu_fast, bf16 weight gradient)."""
    x = f64(x)
    y = gelu64(x)
    e = (GELU_FAST_ERR + 8 * U32 * x.abs()) if fast else gelu_err(x, torch.zeros_like(x))
    u_op = 0.0 if op_dtype == torch.float32 else UNIT[op_dtype]
    return y, e + u_op * (y.abs() + e)


# ---------------------------------------------------------------------------------------------------- references

def linear_ref(a, w, bias=None, residual=None, ln=None, eps=1e-5, gelu=False, gelu_in=False, dgelu_z=None):
    """act(PRO(a) @ w^T + bias) (+ residual | * gelu'(dgelu_z)) -> dict(ref, e_in, pre, e_pre, an, e_an): pre = the value before
    the activation / residual (the pair kernel's z), an = the prologue's result.  a: [M, K], w: [N, K] in the operand type."""
    op = a.dtype
    A, W = f64(a), f64(w)
    K = A.shape[-1]
    e_A = None
    if ln is not None:
        A, e_A = ln_apply(a, ln[0], ln[1], eps, op)
    elif gelu_in:
        A, e_A = gelu_apply(a, op)
    acc = A @ W.t()
    terms = A.abs() @ W.abs().t()
    if bias is not None:
        acc = acc + f64(bias)
        terms = terms + f64(bias).abs()
    e = (K + C_OPS) * U32 * terms
    if e_A is not None:
        e = e + e_A @ W.abs().t() + (K + C_OPS) * U32 * (e_A @ W.abs().t())
    out = dict(pre=acc, e_pre=e, an=A if e_A is not None else None, e_an=e_A)
    ref = acc
    if gelu:
        ref, e = gelu64(acc), gelu_err(acc, e)
    if dgelu_z is not None:
        z = f64(dgelu_z)
        dg = dgelu64(z)
        e = e * (dg.abs() + dgelu_err(z)) + ref.abs() * dgelu_err(z) + 2 * U32 * (ref * dg).abs()
        ref = ref * dg
    elif residual is not None:
        r = f64(residual)
        e = e + 2 * U32 * (ref.abs() + r.abs())
        ref = ref + r
    out.update(ref=ref, e_in=e)
    return out


def wgrad_ref(dc, a, dw0=None, db0=None, ln=None, eps=1e-5, gelu_in=False, want_bias=True):
    """dw = dw0 + dc^T @ PRO(a), dbias = db0 + colsum(dc) (dw0 / db0 None: overwrite) -> (dw, e_dw, dbias, e_db)."""
    op = a.dtype
    DC, A = f64(dc), f64(a)
    M = DC.shape[0]
    e_A = None
    if ln is not None:
        A, e_A = ln_apply(a, ln[0], ln[1], eps, op)
    elif gelu_in:
        A, e_A = gelu_apply(a, op, fast=op == torch.bfloat16)
    dw = DC.t() @ A
    terms = DC.abs().t() @ A.abs()
    db = DC.sum(0)
    tb = DC.abs().sum(0)
    if dw0 is not None:
        dw, terms = dw + f64(dw0), terms + f64(dw0).abs()
    if db0 is not None:
        db, tb = db + f64(db0), tb + f64(db0).abs()
    e = (M + C_OPS) * U32 * terms
    if e_A is not None:
        e = e + (1 + (M + C_OPS) * U32) * (DC.abs().t() @ e_A)
    return dw, e, (db if want_bias else None), (M + C_OPS) * U32 * tb


def ln_bwd_ref(x, dy, gamma, skip=None, skip2=None, dgamma0=None, dbeta0=None, eps=1e-5):
    """wmz_layernorm_bwd: dx = rstd * (g dy - mean_k(g dy) - xhat * mean_k(g dy xhat)) + skip + skip2; dgamma = dgamma0 +
    sum_m dy xhat; dbeta = dbeta0 + sum_m dy -> dict(dx, e_dx, dgamma, e_dgamma, dbeta, e_dbeta)."""
    p = ln_parts(x, eps)
    DY, g = f64(dy), f64(gamma)
    M, K = DY.shape
    xh, rs = p['xhat'], p['rstd']
    gd = g * DY
    c1 = gd.mean(-1, keepdim=True)
    c2 = (gd * xh).mean(-1, keepdim=True)
    e_gd = U32 * gd.abs()
    e_c1 = (K + 3) * U32 * gd.abs().mean(-1, keepdim=True)
    e_c2 = (K + 4) * U32 * (gd * xh).abs().mean(-1, keepdim=True) + (gd.abs() * p['e_xhat']).mean(-1, keepdim=True)
    inner = gd - c1 - xh * c2
    e_inner = (e_gd + e_c1 + xh.abs() * e_c2 + c2.abs() * p['e_xhat'] + 4 * U32 * (gd.abs() + c1.abs() + (xh * c2).abs()))
    core = rs * inner
    e = rs * e_inner + (p['r_rstd'] + U32) * core.abs()
    sk = torch.zeros_like(core)
    for s in (skip, skip2):
        if s is not None:
            sk = sk + f64(s)
    dx = core + sk
    e = e + 2 * U32 * (core.abs() + sk.abs())
    # column sums over the M rows (per wave, per workgroup, then float atomics: some order of M + 1 terms)
    tg = (DY * xh).abs().sum(0)
    dgam = (DY * xh).sum(0)
    dbet = DY.sum(0)
    tb = DY.abs().sum(0)
    if dgamma0 is not None:
        dgam, tg = dgam + f64(dgamma0), tg + f64(dgamma0).abs()
    if dbeta0 is not None:
        dbet, tb = dbet + f64(dbeta0), tb + f64(dbeta0).abs()
    e_dg = (M + C_OPS) * U32 * tg + (DY.abs() * p['e_xhat']).sum(0)
    e_db = (M + C_OPS) * U32 * tb
    return dict(dx=dx, e_dx=e, dgamma=dgam, e_dgamma=e_dg, dbeta=dbet, e_dbeta=e_db)


# ---------------------------------------------------------------------------------------------------- the checker

class BoundError(AssertionError):
    pass


def check(name, got, ref, e_in, norm_tol=None, norm_ref=None):
    """Every element of got within tol = e_in + u_out (|ref| + e_in) + TINY of ref (u_out from got's dtype; no element left out),
    and, with norm_tol, the Frobenius-norm ratio below it (against norm_ref where the entry point's existing norm tolerance was
    set against a reference with the prologue rounded to the operand type).  Returns the largest |got - ref| / tol; raises
    BoundError naming the worst element."""
    u_out = UNIT[got.dtype]
    g = f64(got)
    ref, e_in = f64(ref), f64(e_in)
    assert g.shape == ref.shape == e_in.shape, (name, g.shape, ref.shape, e_in.shape)
    tol = e_in + u_out * (ref.abs() + e_in) + TINY[got.dtype]
    ratio = (g - ref).abs() / tol
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float('inf')))       # NaN / inf results fail
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if not worst <= 1.0:
        flat = int(ratio.reshape(-1).argmax())
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ratio.shape)) if ratio.dim() else ()
        nbad = int((ratio > 1.0).sum())
        raise BoundError(f'{name}: {nbad} of {ratio.numel()} elements outside their bound; worst at {idx}: got {float(g[idx])!r}, '
                         f'reference {float(ref[idx])!r}, tolerance {float(tol[idx]):.3e}, ratio {worst:.3e}')
    if norm_tol is not None:
        nr = ref if norm_ref is None else f64(norm_ref)
        r = float((g - nr).norm() / (nr.norm() + 1e-30))
        assert r < norm_tol, f'{name}: Frobenius ratio {r:.3e} >= {norm_tol:.1e}'
    return worst


# ---------------------------------------------------------------------------------------------------- the sentinel frame

def framed(M, N, dtype, device='cpu', ld=None, left=8, rows_after=3):
    """A [M, N] output inside a larger buffer filled with SENTINEL bytes: `left` columns before it, ld - left - N after it,
    rows_after rows below -> (buf [M + rows_after, ld], the [M, N] view, written_mask of buf)."""
    ld = left + N + 8 if ld is None else ld
    assert ld >= left + N
    buf = torch.empty((M + rows_after, ld), dtype=dtype, device=device)
    buf.view(torch.uint8).fill_(SENTINEL)
    mask = torch.zeros((M + rows_after, ld), dtype=torch.bool)
    mask[:M, left:left + N] = True
    return buf, buf[:M, left:left + N], mask


def framed_flat(shape, dtype, device='cpu', pad=64):
    """A CONTIGUOUS output of `shape` (a weight gradient) with `pad` sentinel elements in front of and behind it
    -> (buf 1-D, the view, written_mask of buf)."""
    n = math.prod(shape)
    buf = torch.empty((n + 2 * pad,), dtype=dtype, device=device)
    buf.view(torch.uint8).fill_(SENTINEL)
    mask = torch.zeros((n + 2 * pad,), dtype=torch.bool)
    mask[pad:pad + n] = True
    return buf, buf[pad:pad + n].view(shape), mask


def assert_untouched(buf, written_mask, sentinel=SENTINEL):
    """Everything of buf outside written_mask still holds the sentinel bytes, bit for bit."""
    raw = buf.detach().cpu().contiguous().view(torch.uint8).reshape(tuple(buf.shape) + (buf.element_size(),))
    changed = (raw != sentinel).any(-1) & ~written_mask
    if bool(changed.any()):
        idx = tuple(int(i) for i in changed.nonzero()[0])
        raise BoundError(f'{int(changed.sum())} elements outside the output were written; first at {idx} '
                         f'(output spans {tuple(int(i) for i in written_mask.nonzero()[0])} .. '
                         f'{tuple(int(i) for i in written_mask.nonzero()[-1])})')
