"""Element-wise error bounds for the attention backward kernels (csrc/attn_bwd.hip, csrc/attn_bwd_row16.hip), the route each shape
takes through their dispatch, and the case table shared by tests/test_attn_bounds_cpu.py and tests/test_attn_bwd_routes_gpu.py.
A plain helper module like tests/gemm_bounds.py (whose UNIT, TINY, check, framed, assert_untouched and BoundError it uses): no
fixtures, nothing collected from here.

The reference is dense fp64 over all N = S H W tokens of a batch element and head, computed from exactly what the kernel is
handed: q, k, v, dO, out already rounded to the kernel's type and lse in fp32.  Forward error is therefore no part of a bound.
Every output element gets  tol = e_in + u_out (|ref| + e_in) + TINY  (gemm_bounds.check); e_in is first order, free of the
summation order and read from the kernels' code -- the derivation, rounding by rounding with the line each is read from, is
profiles/attn_bwd_bounds/README.md.  Nothing in here comes from a GPU run.
"""
import functools
import math
import types

import torch

import gemm_bounds as gb
from gemm_bounds import U32, UNIT, f64
from oracle import attention as oat

C_OPS = 8           # fp32 operations around a sum (gemm_bounds.C_OPS): accumulator start values, the epilogue's scale
F32, BF16 = torch.float32, torch.bfloat16
L2E = 1.4426950408889634


# ------------------------------------------------------------------------------------------------------------ the window

def window_mask(S, H, W, ext):
    """bool [N, N], N = S H W: pair (i, j) is inside the window iff |ds| <= eS and |dh| <= eH and |dw| <= eW (symmetric)."""
    eS, eH, eW = ext
    s, h, w = (t.reshape(-1) for t in torch.meshgrid(torch.arange(S), torch.arange(H), torch.arange(W), indexing='ij'))
    return (((s[:, None] - s[None, :]).abs() <= eS) & ((h[:, None] - h[None, :]).abs() <= eH)
            & ((w[:, None] - w[None, :]).abs() <= eW))


def shifted_mask(S, H, W, ext, shift=(0, 0, 0), grow=(0, 0, 0)):
    """A WRONG window for the seeded-error tests: every extent grown by `grow`, the key offset moved by `shift` (query i sees key j
    iff |s_j - s_i - shift_s| <= eS + grow_s, ...)."""
    s, h, w = (t.reshape(-1) for t in torch.meshgrid(torch.arange(S), torch.arange(H), torch.arange(W), indexing='ij'))
    m = torch.ones((s.numel(), s.numel()), dtype=torch.bool)
    for c, e, sh, gr in zip((s, h, w), ext, shift, grow):
        m &= (c[None, :] - c[:, None] - sh).abs() <= e + gr
    return m


def _heads_first(t, heads, dtype):
    """[B, S, H, W, heads * dh] -> [B, heads, N, dh]"""
    B, I = t.shape[0], t.shape[-1]
    return t.detach().cpu().to(dtype).reshape(B, -1, heads, I // heads).permute(0, 2, 1, 3)


def _tokens_first(t):
    """[B, heads, N, dh] -> [B * N, heads * dh]"""
    B, heads, N, dh = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * N, heads * dh)


def dense_fwd(q, k, v, ext, heads):
    """Dense fp64 forward -> (out [B, S, H, W, I], lse [B * N, heads]): the oracle's attention without its walk over window
    offsets (tests/test_attn_bounds_cpu.py holds it against oracle.attention), for the probes' inputs."""
    B, S, H, W, I = q.shape
    dh = I // heads
    Q, K, V = (_heads_first(t, heads, torch.float64) for t in (q, k, v))
    mask = window_mask(S, H, W, ext)
    s = (Q @ K.transpose(-1, -2)) * dh ** -0.5
    s = torch.where(mask, s, torch.full_like(s, -math.inf))
    lse = torch.logsumexp(s, -1)
    out = torch.exp(s - lse[..., None]) @ V
    return _tokens_first(out).reshape(B, S, H, W, I), lse.permute(0, 2, 1).reshape(-1, heads)


# ------------------------------------------------------------------------------------------------------------ the reference

def bwd_ref(q, k, v, do, out, lse, ext, heads, route='general'):
    """Dense fp64 dq, dk, dv ([B * N, I] each) of
        s = q k^T,  P = exp(scale s - lse_i) mask,  delta_i = sum_c do_ic out_ic,  dP = do v^T,  dS = P (dP - delta),
        dq = scale dS k,  dk = scale dS^T q,  dv = P^T do
    and their per-element e_in.  route: 'general' (attn_bwd.hip) or 'row' (attn_bwd_row16.hip: the logit and dP - delta sums
    start at -lse / scale and -delta, so |lse| / scale and |delta| are among the terms of those running sums).
    -> dict(dq, dk, dv, e_dq, e_dk, e_dv, n)."""
    assert route in ('general', 'row'), route
    B, S, H, W, I = q.shape
    dh = I // heads
    scale = dh ** -0.5
    u = UNIT[q.dtype] if q.dtype in (torch.bfloat16, torch.float16) else 0.0       # rounding of P and dS to the operand type
    mask = window_mask(S, H, W, ext)
    n = int(mask.sum(1).max())
    Q, K, V, DO, O = (_heads_first(t, heads, torch.float64) for t in (q, k, v, do, out))
    L = f64(lse).reshape(B, -1, heads).permute(0, 2, 1)[..., None]                  # [B, heads, N, 1]
    T = lambda t: t.transpose(-1, -2)                                               # noqa: E731
    s = Q @ T(K)
    P = torch.where(mask, torch.exp(scale * s - L), torch.zeros_like(s))
    delta = (DO * O).sum(-1, keepdim=True)
    dP = DO @ T(V)
    dS = P * (dP - delta)
    dq, dk, dv = scale * (dS @ K), scale * (T(dS) @ Q), T(P) @ DO

    kd = (dh + C_OPS) * U32
    e_s = kd * (Q.abs() @ T(K.abs()))
    r_P = scale * e_s + 3 * U32 * (scale * s.abs() + L.abs()) + 2 * U32
    e_dd = kd * (DO.abs() @ T(V.abs())) + kd * (DO * O).abs().sum(-1, keepdim=True)           # e_dP + e_delta
    if route == 'row':
        r_P = r_P + (kd + 3 * U32) * L.abs()           # the start value -lse / scale: a term of the sum, and its own three roundings
        e_dd = e_dd + kd * delta.abs()
    e_dS = P * ((r_P + u + 4 * U32) * (dP - delta).abs() + (1 + r_P + u) * e_dd)
    kn = (n + C_OPS) * U32
    e_dq = scale * (e_dS @ K.abs()) + kn * scale * (dS.abs() @ K.abs())
    e_dk = scale * (T(e_dS) @ Q.abs()) + kn * scale * (T(dS.abs()) @ Q.abs())
    e_dv = T(P * (r_P + u)) @ DO.abs() + kn * (T(P) @ DO.abs())
    res = dict(dq=dq, dk=dk, dv=dv, e_dq=e_dq, e_dk=e_dk, e_dv=e_dv)
    res = {name: _tokens_first(t) for name, t in res.items()}
    res['n'] = n
    return res


# ------------------------------------------------------------------------------------------------------------ the emulation

def _round_to(x, dtype, truncate=False):
    """fp32 x as the MFMA operand of type dtype sees it (round-to-nearest-even; truncate: the seeded error)."""
    if dtype == torch.float32:
        return x
    if truncate:
        assert dtype == torch.bfloat16
        return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)
    return x.to(dtype).float()


def emulate_bwd(q, k, v, do, out, lse, ext, heads, route='general', mask=None, scale_dh=None, no_delta=False, truncate_p=False,
                seed=5):
    """The kernels' arithmetic in fp32 on the CPU -> dq, dk, dv [B * N, I] in the kernel's type: P and dS rounded to the operand
    type, fp32 accumulation, one rounding of the result; route 'row' starts the logit sum at -lse / scale and the dP sum at
    -delta and applies scale in the epilogue.  Keys (dq) and queries (dk, dv) are added in slabs of 32 of a random permutation,
    not in the reference's order.  mask / scale_dh / no_delta / truncate_p seed an error (tests/test_attn_bounds_cpu.py)."""
    B, S, H, W, I = q.shape
    dh = I // heads
    op = q.dtype
    f = torch.float32
    Q, K, V, DO, O = (_heads_first(t, heads, f) for t in (q, k, v, do, out))
    L = lse.detach().cpu().float().reshape(B, -1, heads).permute(0, 2, 1)[..., None]
    T = lambda t: t.transpose(-1, -2)                                               # noqa: E731
    mask = window_mask(S, H, W, ext) if mask is None else mask
    scale = (torch.ones((), dtype=f) / torch.tensor(float(dh if scale_dh is None else scale_dh), dtype=f).sqrt())
    c2 = scale * torch.tensor(L2E, dtype=f)
    delta = torch.zeros_like(L) if no_delta else (DO * O).sum(-1, keepdim=True)
    if route == 'row':
        sacc = (-(L * L2E) / c2) + Q @ T(K)
        P = torch.exp2(sacc * c2)
        dacc = (-delta) + DO @ T(V)
        ds_mul, out_mul = torch.ones((), dtype=f), scale
    else:
        P = torch.exp2((Q @ T(K)) * c2 - L * L2E)
        dacc = DO @ T(V) - delta
        ds_mul, out_mul = scale, torch.ones((), dtype=f)
    P = torch.where(mask, P, torch.zeros_like(P))
    dS = _round_to(P * dacc * ds_mul, op)
    Pr = _round_to(P, op, truncate=truncate_p)
    N = Q.shape[2]
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(seed))
    dq, dk, dv = torch.zeros_like(Q), torch.zeros_like(Q), torch.zeros_like(Q)
    for c in perm.split(32):
        dq += dS[..., c] @ K[..., c, :]
        dk += T(dS[..., c, :]) @ Q[..., c, :]
        dv += T(Pr[..., c, :]) @ DO[..., c, :]
    return tuple(_tokens_first(t).to(op) for t in (dq * out_mul, dk * out_mul, dv))


# ------------------------------------------------------------------------------------------------------------ pair visibility

def tolerance(ref, e_in, dtype):
    return e_in + UNIT[dtype] * (ref.abs() + e_in) + gb.TINY[dtype]


def pair_visibility(q, k, v, do, out, lse, ext, heads, ref, chunk=64):
    """The share of in-window pairs whose removal ALONE (P_ij := 0, everything else as it is) moves some element of dq, dk or
    dv past twice its tolerance: dq_i loses scale dS_ij k_j, dk_j loses scale dS_ij q_i, dv_j loses P_ij do_i."""
    B, S, H, W, I = q.shape
    dh = I // heads
    scale = dh ** -0.5
    mask = window_mask(S, H, W, ext)
    Q, K, V, DO, O = (_heads_first(t, heads, torch.float64) for t in (q, k, v, do, out))
    L = f64(lse).reshape(B, -1, heads).permute(0, 2, 1)[..., None]
    N = Q.shape[2]
    hf = lambda t: t.reshape(B, N, heads, dh).permute(0, 2, 1, 3)                  # noqa: E731
    tq, tk, tv = (hf(tolerance(ref[n], ref['e_' + n], q.dtype)) for n in ('dq', 'dk', 'dv'))
    delta = (DO * O).sum(-1, keepdim=True)
    seen, total = 0, 0
    for i0 in range(0, N, chunk):
        sl = slice(i0, i0 + chunk)
        m = mask[sl]
        P = torch.where(m, torch.exp(scale * (Q[:, :, sl] @ K.transpose(-1, -2)) - L[:, :, sl]), torch.zeros(()).double())
        dS = (P * (DO[:, :, sl] @ V.transpose(-1, -2) - delta[:, :, sl])).abs() * scale         # [B, heads, c, N]
        vis = dS * (K.abs()[:, :, None] / tq[:, :, sl, None]).amax(-1) > 2.0                       # dq[i]: over the channels of k_j
        vis |= dS * (Q.abs()[:, :, sl, None] / tk[:, :, None]).amax(-1) > 2.0                      # dk[j]: channels of q_i
        vis |= P * (DO.abs()[:, :, sl, None] / tv[:, :, None]).amax(-1) > 2.0                      # dv[j]: channels of do_i
        seen += int((vis & m).sum())
        total += int(m.sum()) * B * heads
    return seen / total


# ------------------------------------------------------------------------------------------------------------ the dispatch

def _general_names(dtype, dh):
    T = 'bf16_t' if dtype == BF16 else 'float'
    DHp = 32 if dh <= 32 else (64 if dh <= 64 else 128)
    KC = 4 if (dtype == F32 and DHp == 128) else 8
    return (f'attn_bwd_kernel<{T}, {DHp}, {2 if dtype == BF16 else 1}, {KC}, 0>', f'attn_bwd_kernel<{T}, {DHp}, 1, {KC}, 1>')


def _row(dh, mode, nw, kc, aligned, w8):
    return f'attn_bwd_row16_kernel<{dh}, {mode}, {nw}, {kc}, {str(bool(aligned)).lower()}, {str(bool(w8)).lower()}>'


def bwd_route(shape, dh, dtype, general=False, thirds=False):
    """The kernel instantiations wmz_local3d_attn_bwd launches -> (dq pass, dk|dv pass), as the dispatch of attn_bwd.hip
    (attn_bwd_impl) and attn_bwd_row16.hip (launch_both, launch_both32, launch_one) decides.  thirds: q | k | v are the column
    thirds of one buffer while dO is contiguous (the dk|dv plane kernel is compiled once per `both visitors share a row stride`)."""
    B, S, H, W = shape
    assert dh % 8 == 0 and dh <= 128 and dtype in (F32, BF16)
    row = dtype == BF16 and dh in (32, 64, 128) and not general
    if row and W == 16:
        dq = _row(dh, 0, 16, 8, H % 16 == 0, False)
        if H % 16 == 0:
            return dq, f'attn_bwd_kvplane_kernel<{dh}, {str(not thirds).lower()}>'
        return dq, _row(dh, 1, 8, 8, False, False)
    if row and W == 32:
        Ht = 2 * H
        if Ht <= 8:
            return _row(dh, 2, 4, 2, Ht % 4 == 0, False), _row(dh, 3, 4, 2, Ht % 4 == 0, False)
        return _row(dh, 2, 16, 8, Ht % 16 == 0 and dh < 128, False), _row(dh, 3, 8, 8, Ht % 16 == 0, False)
    if row and W == 8 and H % 2 == 0:
        Ht = H // 2
        if Ht <= 8:
            return _row(dh, 0, 4, 2, Ht % 4 == 0, True), _row(dh, 1, 4, 2, Ht % 4 == 0, True)
        return _row(dh, 0, 8, 8, Ht % 16 == 0, True), _row(dh, 1, 8, 8, Ht % 16 == 0, True)
    return _general_names(dtype, dh)


def route_family(name):
    """'general' or 'row': which form of the bound a kernel instantiation is held to."""
    return 'general' if name.startswith('attn_bwd_kernel<') else 'row'


def _all_instantiations():
    names = []
    for dt in (F32, BF16):
        for dh in (32, 64, 128):
            names += _general_names(dt, dh)
    for dh in (32, 64, 128):
        for al in (True, False):                                     # 16-wide planes
            names.append(_row(dh, 0, 16, 8, al, False))
            names.append(f'attn_bwd_kvplane_kernel<{dh}, {str(al).lower()}>')       # (here: SAME_LD)
        names.append(_row(dh, 1, 8, 8, False, False))
        for al in (True, False):                                     # 8-wide planes: small and big workgroups
            names += [_row(dh, 0, 4, 2, al, True), _row(dh, 1, 4, 2, al, True), _row(dh, 0, 8, 8, al, True), _row(dh, 1, 8, 8, al, True)]
        for al in (True, False):                                     # 32-wide planes
            names += [_row(dh, 2, 4, 2, al, False), _row(dh, 3, 4, 2, al, False), _row(dh, 3, 8, 8, al, False)]
            if not (al and dh == 128):                               # launch_both32: the dq pass's whole-chunks form only below dh 128
                names.append(_row(dh, 2, 16, 8, al, False))
    assert len(names) == len(set(names))
    return tuple(names)


# every kernel instantiation the backward dispatch can launch: 12 general, 15 on 16-wide, 24 on 8-wide, 23 on 32-wide planes
ALL_INSTANTIATIONS = _all_instantiations()


# ------------------------------------------------------------------------------------------------------------ the cases

def _case(id, shape, heads, dh, ext, dtype):
    return types.SimpleNamespace(id=id, shape=shape, heads=heads, dh=dh, ext=ext, dtype=dtype)


CASES = [
    _case('gen-f32-15tok', (1, 2, 3, 5), 3, 8, (1, 1, 1), F32),          # HW = 15 < one tile; narrowest dh; padded lanes beside next head
    _case('gen-f32-dh40', (2, 3, 6, 7), 2, 40, (1, 2, 2), F32),          # HW = 42 ragged tile, DHp = 64, B = 2
    _case('gen-f32-dh128', (1, 2, 9, 16), 1, 128, (1, 4, 3), F32),       # KC = 4 form: 3 slabs per plane, ragged last one; 3 workgroups
    _case('gen-f32-w20', (1, 3, 10, 20), 1, 32, (2, 1, 9), F32),         # tiles straddle plane rows; 13 tiles
    _case('gen-f32-all', (1, 2, 4, 4), 1, 64, (5, 7, 9), F32),           # window larger than the grid
    _case('gen-f32-self', (1, 2, 3, 8), 1, 32, (0, 0, 0), F32),          # every token sees itself only
    _case('gen-bf16-15tok', (1, 2, 3, 5), 3, 8, (1, 1, 1), BF16),        # OPW = 2 with the second tile inactive
    _case('gen-bf16-dh40', (2, 3, 6, 7), 2, 40, (1, 2, 2), BF16),
    _case('gen-bf16-w8-oddH', (1, 2, 7, 8), 1, 128, (1, 2, 2), BF16),    # W = 8, odd H falls off the row route
    _case('gen-bf16-dh16', (1, 2, 9, 16), 2, 16, (1, 1, 3), BF16),       # W = 16 but dh 16: 9 tiles, second dq workgroup holds one tile
    _case('gen-bf16-w20-dh96', (1, 3, 10, 20), 1, 96, (2, 1, 2), BF16),  # DHp = 128 padded, straddling tiles
    _case('w16-plane-128', (1, 2, 16, 16), 1, 128, (1, 1, 1), BF16),     # dq aligned 16-wave; the dk|dv plane kernel
    _case('w16-plane-64', (1, 2, 16, 16), 1, 64, (1, 2, 1), BF16),
    _case('w16-plane-32-two-wg', (2, 2, 32, 16), 1, 32, (1, 3, 1), BF16),        # two plane workgroups; window crosses them
    _case('w16-one-row', (1, 2, 1, 16), 4, 32, (1, 0, 16), BF16),        # one row per plane, whole row visible
    _case('w16-h17', (1, 2, 17, 16), 1, 64, (1, 2, 2), BF16),            # ragged dq, 8-wave dk|dv with 3 workgroups
    _case('w16-h3-whole-plane', (1, 2, 3, 16), 1, 128, (0, 3, 15), BF16),
    _case('w16-h40', (1, 2, 40, 16), 1, 32, (1, 1, 2), BF16),            # 3 dq workgroups, 5 dk|dv workgroups
    _case('w16-time-only', (1, 3, 5, 16), 2, 64, (2, 0, 0), BF16),       # eH = eW = 0
    _case('w8-t1', (1, 2, 2, 8), 1, 128, (1, 1, 3), BF16),               # one tile row = two plane rows
    _case('w8-t4', (1, 2, 8, 8), 1, 64, (1, 2, 2), BF16),                # small aligned
    _case('w8-t6', (2, 2, 12, 8), 2, 32, (1, 1, 1), BF16),               # small ragged, two workgroups
    _case('w8-t8-row', (1, 2, 16, 8), 1, 128, (0, 3, 7), BF16),          # small aligned, whole row visible
    _case('w8-t9', (1, 2, 18, 8), 1, 64, (0, 5, 2), BF16),               # smallest big form, ragged
    _case('w8-t16', (1, 2, 32, 8), 1, 32, (1, 2, 1), BF16),              # big aligned
    _case('w8-t12-col', (1, 1, 24, 8), 1, 128, (0, 1, 0), BF16),         # eW = 0: nothing across the in-tile seam
    _case('w32-small', (1, 2, 2, 32), 1, 64, (1, 1, 3), BF16),           # 32-wide mode under the same bound
    _case('w32-big', (1, 2, 5, 32), 1, 128, (0, 2, 2), BF16),
    # ---- the smallest shapes for the instantiations bwd_route shows the table above does not reach
    _case('w8-t2-64', (1, 2, 4, 8), 1, 64, (1, 1, 2), BF16),             # 8-wide small ragged, dh 64
    _case('w8-t4-32', (1, 2, 8, 8), 2, 32, (1, 3, 1), BF16),             # small aligned, dh 32 (odd eH: the rim rows' select)
    _case('w8-t9-32', (1, 2, 18, 8), 1, 32, (1, 2, 1), BF16),            # big ragged, dh 32
    _case('w8-t16-64', (1, 2, 32, 8), 1, 64, (1, 1, 2), BF16),           # big aligned, dh 64
    _case('w8-t16-128', (1, 1, 32, 8), 1, 128, (0, 3, 2), BF16),         # big aligned, dh 128
    _case('w32-h1-32', (1, 2, 1, 32), 2, 32, (1, 0, 3), BF16),           # 32-wide small ragged
    _case('w32-h3-64', (1, 2, 3, 32), 1, 64, (1, 1, 2), BF16),
    _case('w32-h1-128', (1, 3, 1, 32), 1, 128, (1, 0, 5), BF16),
    _case('w32-h2-32', (1, 2, 2, 32), 2, 32, (1, 1, 1), BF16),           # small aligned
    _case('w32-h4-128', (1, 1, 4, 32), 1, 128, (0, 2, 3), BF16),
    _case('w32-h5-32', (1, 2, 5, 32), 2, 32, (1, 1, 2), BF16),           # big ragged
    _case('w32-h7-64', (1, 1, 7, 32), 1, 64, (0, 3, 2), BF16),
    _case('w32-h8-32', (1, 1, 8, 32), 1, 32, (0, 2, 3), BF16),           # big aligned
    _case('w32-h8-64', (1, 2, 8, 32), 1, 64, (1, 1, 1), BF16),
    _case('w32-h8-128', (1, 1, 8, 32), 1, 128, (0, 1, 4), BF16),
]
CASE = {c.id: c for c in CASES}

# one case per route family takes the q | k | v column-thirds call as well (and every dim_head of the dk|dv plane kernel: its
# SAME_LD = false form is launched by nothing else)
THIRDS = ('gen-f32-dh40', 'gen-bf16-dh40', 'w8-t6', 'w8-t16', 'w16-plane-128', 'w16-plane-64', 'w16-plane-32-two-wg', 'w16-h17',
          'w32-small')

# support probes: (s, h, w) of batch element 0, at most 7 per case -- the plane's corners in the first and last plane, its
# middle, and both sides of every seam the route has
PROBES = {
    # general, W = 20: flat positions 15 | 16 of a plane, the first and last token of the ragged tile (192 .. 199)
    'gen-f32-w20': [(0, 0, 0), (2, 9, 19), (1, 5, 10), (0, 0, 15), (2, 0, 16), (0, 9, 12), (1, 0, 19)],
    'gen-bf16-w20-dh96': [(0, 0, 0), (2, 9, 19), (1, 5, 10), (2, 0, 15), (0, 0, 16), (2, 9, 12), (1, 9, 0)],
    # general, HW = 42: flat 15 | 16 and 31 | 32, the last token of the ragged tile (41)
    'gen-bf16-dh40': [(0, 0, 0), (2, 5, 6), (1, 3, 3), (0, 2, 1), (2, 2, 2), (0, 4, 3), (2, 4, 4)],
    # 16-wide: rows 15 | 16, the last row of the ragged chunk (16)
    'w16-h17': [(0, 0, 0), (1, 16, 15), (0, 8, 8), (0, 15, 5), (1, 16, 9), (1, 15, 15), (0, 16, 0)],
    'w16-plane-32-two-wg': [(0, 0, 0), (1, 31, 15), (0, 16, 8), (1, 15, 0), (0, 16, 15), (0, 15, 7), (1, 0, 15)],
    # 8-wide: (h odd, w = 0) and (h even, w = 7) inside a tile row; plane rows 7 | 8 = tile rows 3 | 4, the workgroup and chunk seam
    'w8-t6': [(0, 0, 0), (1, 11, 7), (0, 6, 4), (0, 7, 0), (1, 8, 7), (1, 3, 0), (0, 4, 7)],
    # plane rows 15 | 16 = tile rows 7 | 8, the seam between the two 8-wave workgroups
    'w8-t16': [(0, 0, 0), (1, 31, 7), (0, 14, 3), (0, 15, 0), (1, 16, 7), (1, 1, 0), (0, 2, 7)],
}

SEED = 0


def case_routes(c, thirds=False):
    return bwd_route(c.shape, c.dh, c.dtype, thirds=thirds)


def case_family(c):
    fam = {route_family(n) for n in case_routes(c)}
    assert len(fam) == 1
    return fam.pop()


def make_inputs(c, q, k, v, do, fwd=dense_fwd):
    """q, k, v, dO (rounded to the case's type) -> the kernel's whole input set and the reference for it: out and lse from the fp64
    forward `fwd` of those values, out rounded to the type, lse to fp32."""
    out64, lse64 = fwd(q.double(), k.double(), v.double(), c.ext, c.heads)
    out, lse = out64.to(c.dtype), lse64.float()
    ref = bwd_ref(q, k, v, do, out, lse, c.ext, c.heads, case_family(c))
    return types.SimpleNamespace(q=q, k=k, v=v, do=do, out=out, lse=lse, out64=out64, lse64=lse64, ref=ref)


def oracle_fwd(q, k, v, ext, heads):
    """oracle.attention in double -> (out, lse [B * N, heads])"""
    out, dots = oat.local_attention(k, v, q, ext, heads, return_logits=True)
    return out, torch.logsumexp(dots, -1).reshape(-1, heads)


@functools.lru_cache(maxsize=None)
def case_inputs(case_id):
    """The inputs of a case (torch.randn at SEED, rounded to its type; out and lse from the fp64 oracle) and its reference.  Computed
    once per process and shared: nobody writes to it."""
    c = CASE[case_id]
    B, S, H, W = c.shape
    gen = torch.Generator().manual_seed(SEED)
    q, k, v, do = (torch.randn(B, S, H, W, c.heads * c.dh, generator=gen).to(c.dtype) for _ in range(4))
    return make_inputs(c, q, k, v, do, fwd=oracle_fwd)
