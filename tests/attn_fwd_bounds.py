"""Element-wise error bounds for the attention forward kernels (csrc/attn_fwd.hip, attn_fwd_row16.hip and the units that compile it:
attn_fwd_row16_f16.hip, attn_fwd_row32.hip, attn_fwd_row32_f16.hip; attn_fwd_row16_infer.hip), the instantiation each launch takes
through attn_fwd_impl, and the case table shared by tests/test_attn_fwd_bounds_cpu.py and tests/test_attn_fwd_routes_gpu.py.  A plain
helper module like tests/attn_bounds.py (whose window_mask, _heads_first, _tokens_first it uses) and tests/gemm_bounds.py (UNIT, TINY,
U32, check, framed, framed_flat, assert_untouched, BoundError): no fixtures, nothing collected from here.

The reference is dense fp64 over all N = S H W tokens of a batch element and head, computed from exactly what the kernel is handed:
q, k, v already rounded to the kernel's type.  Every element of out, lse and the probed logits gets
    tol = e_in + u_out (|ref| + e_in) + TINY                    (gemm_bounds.check)
e_in is first order, free of the summation order and read from the kernels' code -- the derivation, rounding by rounding with the
line each is read from, is profiles/attn_fwd_bounds/README.md.  Nothing in here comes from a GPU run.
"""
import functools
import math
import types

import torch

from attn_bounds import _heads_first, _tokens_first, window_mask
from gemm_bounds import TINY, U32, UNIT, BoundError, assert_untouched, check, f64, framed, framed_flat      # noqa: F401
from tail_bounds import DIV_SQRT_U, EXP2_ULPS, LOG_ULPS

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
C_OPS = 8                   # fp32 operations around a sum (gemm_bounds.C_OPS)
L2E = 1.4426950408889634
LN2 = 0.6931471805599453
DEFER = 8.0                 # attn_row16_step.h:37, log2 units: how far a logit may stand above the row kernels' deferred reference
R_SCALE = 4                 # G.scale = 1.0f / sqrtf(dh) (attn_fwd.hip:326): sqrtf and the division, DIV_SQRT_U each
R_C2 = R_SCALE + 2          # c2 = G.scale * 1.4426950408889634f: the constant's own rounding and the product
HALF_GRID = 2.0 ** -25      # IEEE half below 2^-14: a fixed grid of 2^-24, kept (not flushed) by v_cvt_f16_f32 and the MFMA


# ------------------------------------------------------------------------------------------------------------ the window

def _coords(S, H, W):
    return tuple(t.reshape(-1) for t in torch.meshgrid(torch.arange(S), torch.arange(H), torch.arange(W), indexing='ij'))


def window_mask4(S, H, W, ext, shift=(0, 0, 0), grow=(0, 0, 0)):
    """bool [N, N]: query i sees key j iff -eS_back <= s_j - s_i <= eS_fwd and |dh| <= eH and |dw| <= eW, ext = (eS_back, eS_fwd, eH,
    eW) (wmz_local3d_attn_fwd_window's law; eS_back == eS_fwd is attn_bounds.window_mask).  shift / grow: a WRONG window for the
    seeded-error tests -- the key offset moved by `shift`, every extent grown by `grow` on both sides."""
    eb, ef, eH, eW = ext
    if eb == ef and shift == (0, 0, 0) and grow == (0, 0, 0):
        return window_mask(S, H, W, (eb, eH, eW))
    s, h, w = _coords(S, H, W)
    ds = s[None, :] - s[:, None] - shift[0]
    m = (ds >= -(eb + grow[0])) & (ds <= ef + grow[0])
    for c, e, sh, gr in ((h, eH, shift[1], grow[1]), (w, eW, shift[2], grow[2])):
        m &= (c[None, :] - c[:, None] - sh).abs() <= e + gr
    return m


def _tiles_seen(S, H, W, mask):
    """[N]: in how many 16-token tiles of the key planes (a key row of the row kernels, a key tile of the general kernel) a query
    has a visible key: no more steps than that can move its running maximum."""
    s, h, w = _coords(S, H, W)
    tpp = (H * W + 15) // 16
    tile = s * tpp + (h * W + w) // 16
    onehot = torch.zeros(s.numel(), S * tpp, dtype=torch.float64)
    onehot[torch.arange(s.numel()), tile] = 1.0
    return ((mask.double() @ onehot) > 0).sum(1)


# ------------------------------------------------------------------------------------------------------------ the reference

def fwd_ref(q, k, v, ext, heads, route='general'):
    """Dense fp64 out [B * N, I], lse [B * N, heads] and scaled logits of
        x = scale q k^T,  lse_i = log sum_j exp(x_ij),  P = exp(x - lse) mask,  out = P v
    with their per-element e_in (README: the logit, the exponent, the running maximum, P and l, the output, lse).  route: 'general'
    (attn_fwd.hip: fma(s, c2, -m_new c2), a rescale at every step that moves the maximum, lse = m scale + logf(l)) or 'row' (the row
    kernels: fma(s, c2, -m_run) with a reference that moves in the rare branch only, lse = m_run ln 2 + logf(l)).
    -> namespace(out, e_out, lse, e_lse, x, e_x, mask, n, P, E, r_l, with_v)."""
    assert route in ('general', 'row'), route
    B, S, H, W, I = q.shape
    dh = I // heads
    scale = dh ** -0.5
    u = UNIT[q.dtype] if q.dtype in (BF16, F16) else 0.0                  # rounding of P to the operand type of the PV product
    mask = window_mask4(S, H, W, ext)
    n_i = mask.sum(1).double()[:, None]
    moves = _tiles_seen(S, H, W, mask).double()[:, None]
    Q, K = (_heads_first(t, heads, torch.float64) for t in (q, k))
    x = scale * (Q @ K.transpose(-1, -2))
    xm = torch.where(mask, x, torch.full_like(x, -math.inf))
    lse = torch.logsumexp(xm, -1, keepdim=True)
    P = torch.exp(xm - lse)
    absx = torch.where(mask, x.abs(), torch.zeros_like(x))
    X = absx.amax(-1, keepdim=True)                                             # the largest |scaled logit| a query sees
    D = xm.amax(-1, keepdim=True) - torch.where(mask, x, torch.full_like(x, math.inf)).amin(-1, keepdim=True)

    e_s = (dh + C_OPS) * U32 * scale * (Q.abs() @ K.abs().transpose(-1, -2))    # the logit, in units of x
    if route == 'general':
        # exponent: c2's roundings on the product and on -m_new c2, that product's own rounding, the fma's; exp2f
        r_pair = e_s + R_C2 * U32 * (absx + X) + U32 * X + U32 * D + 2 * EXP2_ULPS * U32
        # a move: alpha = exp2f((m_old - m_new) c2) -- the difference and the product rounded (2 U32 |dx|, dx summing to <= D),
        # exp2f, and the product with l / o
        rho = moves * (2 * EXP2_ULPS + 1) * U32 + 2 * U32 * D
        log_l = torch.log(n_i)
    else:
        # exponent: c2's roundings on the product alone (m_run is a number of the log2 domain), the fma's rounding and that of
        # `t -= gm` in a step that moves the reference; exp2
        r_pair = e_s + R_C2 * U32 * absx + 2 * U32 * (D + DEFER * LN2) + 2 * EXP2_ULPS * U32
        # a move: alpha = exp2(-gm) and its product with l / o, and m_run += gm rounded at |m_run| ln 2 <= X
        rho = moves * ((2 * EXP2_ULPS + 1) * U32 + U32 * X)
        log_l = torch.log(n_i) + DEFER * LN2
    kn = (n_i + C_OPS) * U32
    E = P * (r_pair + rho + u + kn)                          # |error| of one pair's term of the PV sum, per unit of |v|
    r_l = (P * r_pair).sum(-1, keepdim=True) + rho + kn      # relative error of l: the unrounded p, any order
    e_lse = r_l + (R_SCALE + 1) * U32 * X + 2 * LOG_ULPS * U32 * log_l
    e_x = e_s + (R_SCALE + 1) * U32 * absx                   # the probe: sc * G.scale

    def with_v(v):
        """out and e_out for these q, k and the values v"""
        V = _heads_first(v, heads, torch.float64)
        out = P @ V
        e = E @ V.abs() + (r_l + (DIV_SQRT_U + 1) * U32) * out.abs()            # inv = 1.f / l and o * inv
        if q.dtype == F16:
            e = e + HALF_GRID * (mask.double() @ V.abs())    # a p below 2^-14 of the reference (l >= 1): absolute, per key
        return _tokens_first(out), _tokens_first(e)

    out, e_out = with_v(v)
    flat = lambda t: t.permute(0, 2, 1, 3).reshape(-1, heads)                   # noqa: E731  [B, heads, N, 1] -> [B * N, heads]
    return types.SimpleNamespace(out=out, e_out=e_out, lse=flat(lse), e_lse=flat(e_lse), x=x, e_x=e_x, mask=mask, n=int(n_i.max()),
                                 P=P, E=E, r_l=r_l, with_v=with_v)


def tolerance(ref, e_in, dtype):
    return e_in + UNIT[dtype] * (ref.abs() + e_in) + TINY[dtype]


def probe_ref(ref, shape, ext, heads):
    """The probe's layout: [B * N, heads, (eS_back + eS_fwd + 1)(2 eH + 1)(2 eW + 1)], slot ((ds + eS_back)(2 eH + 1) + dh + eH)
    (2 eW + 1) + dw + eW, the caller's -1e9 (exact: e = 0) where the slot is outside the window or the grid -> (logits, e)."""
    B, S, H, W = shape
    eb, ef, eH, eW = ext
    kh, kw = 2 * eH + 1, 2 * eW + 1
    nk = (eb + ef + 1) * kh * kw
    s, h, w = _coords(S, H, W)
    i, j = ref.mask.nonzero(as_tuple=True)
    slot = ((s[j] - s[i] + eb) * kh + h[j] - h[i] + eH) * kw + w[j] - w[i] + eW
    N = S * H * W
    lg = torch.full((B, heads, N, nk), -1e9, dtype=torch.float64)
    e = torch.zeros_like(lg)
    lg[:, :, i, slot] = ref.x[:, :, i, j]
    e[:, :, i, slot] = ref.e_x[:, :, i, j]
    back = lambda t: t.permute(0, 2, 1, 3).reshape(B * N, heads, nk)            # noqa: E731
    return back(lg), back(e)


# ------------------------------------------------------------------------------------------------------------ key-indicator V

def n_slots(ext):
    eb, ef, eH, eW = ext
    return (eb + ef + 1) * (2 * eH + 1) * (2 * eW + 1)


def n_indicator_launches(c):
    return -(-n_slots(c.ext) // c.dh)


def indicator_v(shape, heads, dh, ext, g, dtype):
    """V_j = e_{slot(j) - g dh} where that index lies in [0, dh), else 0 (every head alike), with
        slot(j) = ((s_j mod eS)(2 eH + 1) + h_j mod (2 eH + 1))(2 eW + 1) + w_j mod (2 eW + 1),   eS = eS_back + eS_fwd + 1:
    injective inside any window, so out[i, c] is the single probability P_ij of at most one key."""
    B, S, H, W = shape
    eb, ef, eH, eW = ext
    s, h, w = _coords(S, H, W)
    slot = ((s % (eb + ef + 1)) * (2 * eH + 1) + h % (2 * eH + 1)) * (2 * eW + 1) + w % (2 * eW + 1)
    ch = slot - g * dh
    v = torch.zeros(S * H * W, dh)
    ok = (ch >= 0) & (ch < dh)
    v[ok.nonzero()[:, 0], ch[ok]] = 1.0
    return v.repeat(1, heads).reshape(1, S, H, W, heads * dh).expand(B, S, H, W, heads * dh).contiguous().to(dtype)


# ------------------------------------------------------------------------------------------------------------ the emulation

def _round_to(x, dtype, truncate=False):
    """fp32 x as the MFMA operand of type dtype sees it (round-to-nearest-even; truncate: the seeded error)."""
    if dtype == F32:
        return x
    if truncate:
        assert dtype == BF16
        return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)
    return x.to(dtype).float()


def emulate_fwd(q, k, v, ext, heads, route='general', mask=None, scale_dh=None, truncate_p=False, no_o_rescale=False,
                lse_no_ln2=False, seed=5):
    """The kernels' arithmetic in fp32 on the CPU -> (out [B * N, I] in the kernel's type, lse [B * N, heads] fp32): an online
    softmax over slabs of 32 keys of a random permutation, the exponent by one fma-like step against a reference that moves when a
    logit stands more than DEFER log2 units above it (route 'row'; 'general': at every new maximum), l from the unrounded p, P
    rounded to the operand type, one rounding of the result.  mask / scale_dh / truncate_p / no_o_rescale / lse_no_ln2 seed an error
    (tests/test_attn_fwd_bounds_cpu.py)."""
    B, S, H, W, I = q.shape
    dh = I // heads
    op = q.dtype
    f = torch.float32
    Q, K, V = (_heads_first(t, heads, f) for t in (q, k, v))
    mask = window_mask4(S, H, W, ext) if mask is None else mask
    scale = torch.ones((), dtype=f) / torch.tensor(float(dh if scale_dh is None else scale_dh), dtype=f).sqrt()
    c2 = scale * torch.tensor(L2E, dtype=f)
    defer = DEFER if route == 'row' else 0.0
    N = Q.shape[2]
    ninf = torch.tensor(-math.inf, dtype=f)
    m = torch.zeros(B, heads, N, 1, dtype=f)                 # the reference, log2 units
    started = torch.zeros(B, heads, N, 1, dtype=torch.bool)
    l = torch.zeros_like(m)
    o = torch.zeros_like(Q)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(seed))
    for c in perm.split(32):
        t = torch.where(mask[:, c], (Q @ K[..., c, :].transpose(-1, -2)) * c2 - m, ninf)
        mx = t.amax(-1, keepdim=True)
        move = torch.isfinite(mx) & (~started | (mx > defer))
        gm = torch.where(move, mx, torch.zeros_like(mx))
        alpha = torch.where(move & started, torch.exp2(-gm), torch.ones_like(gm))
        l = l * alpha
        if not no_o_rescale:
            o = o * alpha
        m = m + gm
        started = started | move
        p = torch.exp2(t - gm)
        l = l + p.sum(-1, keepdim=True)
        o = o + _round_to(p, op, truncate=truncate_p) @ V[..., c, :]
    out = _tokens_first(o * (1.0 / l)).to(op)
    lse = (m if lse_no_ln2 else m * torch.tensor(LN2, dtype=f)) + torch.log(l)
    return out, lse.permute(0, 2, 1, 3).reshape(-1, heads)


# ------------------------------------------------------------------------------------------------------------ the dispatch

UNIT_OF = {(BF16, False): 'attn_fwd_row16.hip', (F16, False): 'attn_fwd_row16_f16.hip',
           (BF16, True): 'attn_fwd_row32.hip', (F16, True): 'attn_fwd_row32_f16.hip'}
MODE = 9                    # WMZ_ATTN_MODE of the product (attn_fwd_row16.hip:413); the 32-wide units add bit 4
INFER = 'attn_fwd_row16_infer.hip: attn_fwd_row16_infer_kernel<{0}, {0}>'


def _general_name(dtype, dh):
    DHp = 32 if dh <= 32 else (64 if dh <= 64 else 128)
    if dtype == BF16:
        return f'attn_fwd.hip: attn_fwd_kernel<bf16_t, {DHp}, 1, 8, 16>'
    return f'attn_fwd.hip: attn_fwd_kernel<float, {DHp}, 1, {4 if DHp == 128 else 8}, 8>'


def _row_name(dtype, w32, dh, big, aligned, probe, w8):
    b = lambda v: str(bool(v)).lower()                                          # noqa: E731
    return (f'{UNIT_OF[(dtype, w32)]}: attn_fwd_row16_kernel<{dh}, {"Big" if big else "Small"}, {MODE | 16 if w32 else MODE}, '
            f'{b(aligned)}, {b(probe)}, false, {b(w8)}>')


def infer_takes(shape, dh, heads, ext, ld):
    """wmz_attn_fwd_row16_infer_takes (attn_fwd_row16_infer.hip:325) without the development knobs; ld = (ldq, ldk, ldv, ldo)."""
    B, S, H, W = shape
    eb, ef, eH, eW = ext
    return (ef == eb and W == 16 and H == 16 and dh == 128 and heads == 1 and tuple(ld) == (128,) * 4
            and (eH, eW) in ((3, 3), (1, 1)) and B * S * 256 <= 2 ** 31 and B * S * S <= 2 ** 31 and (S + eb) * (2 * eb + 1) <= 2 ** 31)


def fwd_route(shape, dh, dtype, general=False, lse=True, probe=False, ext=None, heads=1, ld=None):
    """The kernel instantiation attn_fwd_impl (attn_fwd.hip:308) launches, or None where it returns WMZ_ERR_UNSUPPORTED.  lse / probe:
    whether those pointers are given.  ext, heads, ld = (ldq, ldk, ldv, ldo) matter to the inference unit's hand-over only (default:
    contiguous operands and the extents of no unit)."""
    B, S, H, W = shape
    assert dh % 8 == 0 and dtype in (F32, BF16, F16)
    if dh > 128:
        return None
    ld = (heads * dh,) * 4 if ld is None else ld
    if dtype != F32 and dh in (32, 64, 128) and not general:
        if dtype == BF16 and not lse and not probe and ext is not None and infer_takes(shape, dh, heads, ext, ld):
            return INFER.format(ext[2])
        if W == 16:                                          # by_dh: ALIGNED iff G.H % CH == 0, CH = 16 (Big) or 4 (Small)
            return _row_name(dtype, False, dh, True, H % 16 == 0, probe, False)
        if W == 8 and H % 2 == 0:
            Ht = H // 2
            return _row_name(dtype, False, dh, Ht > 8, Ht % (16 if Ht > 8 else 4) == 0, probe, True)
        if W == 32:
            Ht = 2 * H
            return _row_name(dtype, True, dh, Ht > 8, Ht % (16 if Ht > 8 else 4) == 0, probe, False)
    if dtype == F16:
        return None
    return _general_name(dtype, dh)


def route_family(name):
    """'general' or 'row': which form of the bound an instantiation is held to."""
    return 'general' if 'attn_fwd_kernel<' in name else 'row'


def _all_instantiations():
    names = [_general_name(dt, dh) for dt in (F32, BF16) for dh in (32, 64, 128)]
    for dt in (BF16, F16):
        for dh in (32, 64, 128):
            for al in (True, False):
                names.append(_row_name(dt, False, dh, True, al, False, False))               # 16-wide planes: always Big
                for big in (False, True):
                    names.append(_row_name(dt, False, dh, big, al, False, True))             # 8-wide
                    names.append(_row_name(dt, True, dh, big, al, False, False))             # 32-wide
    names += [INFER.format(3), INFER.format(1)]
    assert len(names) == len(set(names))
    return tuple(names)


# every instantiation a product launch without the probe can reach: 6 general, 2 x 6 on 16-wide, 2 x 12 on 8-wide, 2 x 12 on 32-wide
# planes (bf16 and half units), 2 inference-unit kernels
PLAIN_INSTANTIATIONS = _all_instantiations()
# PROBE = true (a logits_dbg pointer) compiles each row instantiation once more; one per family is launched by the cases of PROBED
# below (the general kernel's probe is a run-time branch of the same instantiation)
PROBED = ('gen-f32-dh40', 'gen-bf16-dh40', 'w16-h17', 'w8-t6', 'w8-t16', 'w32-small', 'w32-big', 'h-w16-plane-64', 'h-w8-t9', 'h-w32-h3-64')


# ------------------------------------------------------------------------------------------------------------ the cases

def _case(id, shape, heads, dh, ext, dtype, seed=0):
    ext = (ext[0], ext[0], ext[1], ext[2]) if len(ext) == 3 else tuple(ext)
    return types.SimpleNamespace(id=id, shape=shape, heads=heads, dh=dh, ext=ext, dtype=dtype, seed=seed)


_GENERAL = [
    _case('gen-f32-15tok', (1, 2, 3, 5), 3, 8, (1, 1, 1), F32),          # HW = 15 < one tile; narrowest dh; padded lanes beside next head
    _case('gen-f32-dh40', (2, 3, 6, 7), 2, 40, (1, 2, 2), F32),          # HW = 42 ragged tile, DHp = 64, B = 2
    _case('gen-f32-dh128', (1, 2, 9, 16), 1, 128, (1, 4, 3), F32),       # KC = 4 form: 3 slabs per plane, ragged last one; 2 workgroups
    _case('gen-f32-w20', (1, 3, 10, 20), 1, 32, (2, 1, 9), F32),         # tiles straddle plane rows; the column-range test bites
    _case('gen-f32-all', (1, 2, 4, 4), 1, 64, (5, 7, 9), F32),           # window larger than the grid
    _case('gen-f32-self', (1, 2, 3, 8), 1, 32, (0, 0, 0), F32),          # every token sees itself only
    _case('gen-bf16-15tok', (1, 2, 3, 5), 3, 8, (1, 1, 1), BF16),
    _case('gen-bf16-dh40', (2, 3, 6, 7), 2, 40, (1, 2, 2), BF16),
    _case('gen-bf16-w8-oddH', (1, 2, 7, 8), 1, 128, (1, 2, 2), BF16),    # W = 8, odd H falls off the row route
    _case('gen-bf16-dh16', (1, 2, 9, 16), 2, 16, (1, 1, 3), BF16),       # W = 16 but dh 16
    _case('gen-bf16-w20-dh96', (1, 3, 10, 20), 1, 96, (2, 1, 2), BF16),  # DHp = 128 padded, straddling tiles
    _case('gen-bf16-h17x16', (1, 2, 17, 16), 1, 64, (1, 2, 2), BF16),    # a row-route shape: taken through wmz_local3d_attn_fwd_general
    _case('gen-f32-causal', (1, 4, 6, 7), 2, 40, (2, 0, 1, 2), F32),     # causal (2, 0)
    _case('gen-bf16-asym', (1, 4, 6, 7), 1, 32, (2, 1, 2, 1), BF16),     # asymmetric (2, 1)
]
# the row shapes: each runs in bf16 (id as it stands) and in IEEE half ('h-' + id)
_ROW = [
    _case('w16-plane-128', (1, 2, 16, 16), 1, 128, (1, 1, 1), BF16),     # aligned: a whole 16x16 plane per workgroup
    _case('w16-plane-64', (2, 2, 16, 16), 2, 64, (1, 2, 1), BF16),       # B = 2, two heads
    _case('w16-plane-32-two-wg', (1, 2, 32, 16), 1, 32, (1, 3, 1), BF16),        # two workgroups per plane; the window crosses them
    _case('w16-one-row', (1, 2, 1, 16), 4, 32, (1, 0, 16), BF16),        # one row per plane (H = 1: no row of phase 1), whole row visible
    _case('w16-h17', (1, 2, 17, 16), 1, 64, (1, 2, 2), BF16),            # ragged: a second chunk of one row
    _case('w16-h3-whole-plane', (1, 2, 3, 16), 1, 128, (0, 3, 15), BF16),
    _case('w16-h40', (1, 2, 40, 16), 1, 32, (1, 1, 2), BF16),            # 3 workgroups, ragged last chunk of 8 rows
    _case('w16-time-only', (1, 3, 5, 16), 2, 64, (2, 0, 0), BF16),       # eH = eW = 0
    _case('w16-all', (1, 2, 4, 16), 1, 64, (3, 9, 20), BF16),            # window larger than the grid
    _case('w16-self', (1, 2, 3, 16), 1, 32, (0, 0, 0), BF16),            # extents (0, 0, 0)
    _case('w16-causal', (1, 4, 5, 16), 3, 32, (2, 0, 1, 2), BF16),       # causal; three heads
    _case('w16-asym', (1, 5, 16, 16), 1, 128, (2, 1, 1, 1), BF16),       # asymmetric (2, 1): the plane rotation by its own length
    _case('w8-t1', (1, 2, 2, 8), 1, 128, (1, 1, 3), BF16),               # one tile row = two plane rows
    _case('w8-t4', (1, 2, 8, 8), 1, 64, (1, 2, 2), BF16),                # small aligned
    _case('w8-t6', (2, 2, 12, 8), 2, 32, (1, 1, 1), BF16),               # small ragged, two workgroups; odd eH: the rim select
    _case('w8-t8-row', (1, 2, 16, 8), 1, 128, (0, 3, 7), BF16),          # small aligned, whole row visible
    _case('w8-t9', (1, 2, 18, 8), 1, 64, (0, 5, 2), BF16),               # smallest big form, ragged
    _case('w8-t16', (1, 2, 32, 8), 1, 32, (1, 2, 1), BF16),              # big aligned
    _case('w8-t12-col', (1, 1, 24, 8), 1, 128, (0, 1, 0), BF16),         # eW = 0: nothing across the in-tile seam
    _case('w8-t2-64', (1, 2, 4, 8), 1, 64, (1, 1, 2), BF16),             # small ragged, dh 64
    _case('w8-t4-32', (1, 2, 8, 8), 2, 32, (1, 3, 1), BF16),             # small aligned, dh 32
    _case('w8-t9-32', (1, 2, 18, 8), 1, 32, (1, 2, 1), BF16),            # big ragged, dh 32
    _case('w8-t16-64', (1, 2, 32, 8), 1, 64, (1, 1, 2), BF16),           # big aligned, dh 64
    _case('w8-t16-128', (1, 1, 32, 8), 1, 128, (0, 3, 2), BF16),         # big aligned, dh 128
    _case('w8-eH0', (1, 2, 6, 8), 1, 64, (1, 0, 2), BF16),               # eH = 0: both sub-rows of a tile row are rim
    _case('w8-asym', (1, 4, 8, 8), 2, 64, (2, 1, 1, 2), BF16),           # asymmetric (2, 1)
    _case('w32-small', (1, 2, 2, 32), 1, 64, (1, 1, 3), BF16),           # small aligned
    _case('w32-big', (1, 2, 5, 32), 1, 128, (0, 2, 2), BF16),            # big ragged
    _case('w32-h1-32', (1, 2, 1, 32), 2, 32, (1, 0, 3), BF16),           # small ragged
    _case('w32-h3-64', (2, 2, 3, 32), 1, 64, (1, 1, 2), BF16),
    _case('w32-h1-128', (1, 3, 1, 32), 1, 128, (1, 0, 5), BF16),
    _case('w32-h2-32', (1, 2, 2, 32), 2, 32, (1, 1, 1), BF16),           # small aligned
    _case('w32-h4-128', (1, 1, 4, 32), 1, 128, (0, 2, 3), BF16),
    _case('w32-h5-32', (1, 2, 5, 32), 2, 32, (1, 1, 2), BF16),           # big ragged
    _case('w32-h7-64', (1, 1, 7, 32), 1, 64, (0, 3, 2), BF16),
    _case('w32-h8-32', (1, 1, 8, 32), 1, 32, (0, 2, 3), BF16),           # big aligned
    _case('w32-h8-64', (1, 2, 8, 32), 1, 64, (1, 1, 1), BF16),
    _case('w32-h8-128', (1, 1, 8, 32), 1, 128, (0, 1, 4), BF16),
    _case('w32-eW0', (1, 2, 3, 32), 1, 32, (1, 1, 0), BF16, seed=1),     # eW = 0: nothing across the seam between the halves (seed 0: 7 of 6144 cancelled)
    _case('w32-wide', (1, 1, 3, 32), 1, 64, (0, 1, 17), BF16),           # eW > 16: the seam mask admits columns of the same index
    _case('w32-asym', (1, 4, 2, 32), 1, 64, (2, 1, 1, 2), BF16),         # asymmetric (2, 1)
    # the inference unit's geometry: with lse = None these two reach attn_fwd_row16_infer_kernel, with lse the run-time kernel
    _case('infer-33', (1, 3, 16, 16), 1, 128, (1, 3, 3), BF16),
    _case('infer-11', (2, 2, 16, 16), 1, 128, (1, 1, 1), BF16),
]
INFER_CASES = ('infer-33', 'infer-11')


def _half(c):
    return types.SimpleNamespace(**{**vars(c), 'id': 'h-' + c.id, 'dtype': F16})


CASES = _GENERAL + _ROW + [_half(c) for c in _ROW if c.id not in INFER_CASES]
CASE = {c.id: c for c in CASES}

# one case per family takes the logit regimes, the q | k | v column-thirds call and the planes entry point
REGIMES = ('randn', 'peaked', 'rising', 'jump', 'equal', 'offset')
REGIME_CASES = ('gen-f32-dh40', 'gen-bf16-dh40', 'w16-h17', 'w8-t6', 'w8-t9-32', 'w32-h5-32', 'h-w16-h17', 'h-w8-t6', 'h-w32-h5-32')
THIRDS = ('gen-f32-dh40', 'gen-bf16-dh40', 'w16-plane-64', 'w8-t6', 'w32-h5-32', 'h-w16-plane-64', 'h-w32-small')
PLANES = ('gen-f32-w20', 'gen-bf16-w20-dh96', 'w16-asym', 'w8-asym', 'w32-asym', 'h-w16-asym', 'infer-33')     # B = 1, S >= 3
FAMILIES = ('general-f32', 'general-bf16', 'w16', 'w8', 'w32', 'half')


def case_route(c, lse=True, probe=False, general=False, ld=None):
    return fwd_route(c.shape, c.dh, c.dtype, general=general, lse=lse, probe=probe, ext=c.ext, heads=c.heads, ld=ld)


def case_family(c, general=False):
    return route_family(case_route(c, general=general))


def case_group(c):
    """Which of FAMILIES a case belongs to (the seeded errors are asked of each)."""
    name = case_route(c)
    if route_family(name) == 'general':
        return 'general-f32' if c.dtype == F32 else 'general-bf16'
    if c.dtype == F16:
        return 'half'
    return 'w32' if 'row32' in name else ('w8' if name.endswith('true>') else 'w16')


def indicator_cases():
    return [c.id for c in CASES if n_indicator_launches(c) <= 8]


def _walk_rank(S, H, W):
    """About where in a row kernel's walk a key is met: planes upwards, inside a plane the even 16-token rows, then the odd ones."""
    s, h, w = _coords(S, H, W)
    row = (h * W + w) // 16
    rows = (H * W + 15) // 16
    return (s * rows + (row % 2) * ((rows + 1) // 2) + row // 2).float(), rows * S


def make_qkv(c, regime='randn'):
    """q, k, v of a case in one of the logit regimes, rounded to its type."""
    B, S, H, W = c.shape
    I = c.heads * c.dh
    gen = torch.Generator().manual_seed(c.seed)
    q, k, v = (torch.randn(B, S, H, W, I, generator=gen) for _ in range(3))
    v = v + 1.0             # off zero: an output that cancels below its own bound (|out| < u sum P |v|) would escape the norm bar
    scale = c.dh ** -0.5
    heads_view = lambda t: t.view(B, S, H, W, c.heads, c.dh)                    # noqa: E731
    if regime == 'peaked':                                   # the scaled logits reach +-30
        x = scale * torch.einsum('bihc,bjhc->bhij', q.reshape(B, -1, c.heads, c.dh), k.reshape(B, -1, c.heads, c.dh))
        q = q * (30.0 / float(x.abs().max()))
    elif regime == 'rising':                                 # 3 log2 units per key row along the walk: under DEFER per 2-row step
        rank, _ = _walk_rank(S, H, W)
        q, k = 0.05 * q, 0.05 * k
        heads_view(q)[..., 0] = 2.0
        heads_view(k)[..., 0] = (rank * (3.0 * LN2 / (2.0 * scale))).view(S, H, W, 1)
    elif regime == 'jump':                                   # keys of every plane's last row: 20 log2 units above the rest
        heads_view(q)[..., 0] = 2.0
        heads_view(k)[..., 0] = 0.0
        heads_view(k)[:, :, H - 1, 2::5, :, 0] = 20.0 * LN2 / (2.0 * scale)
    elif regime == 'equal':                                  # all logits tied
        q, k = torch.zeros_like(q), torch.zeros_like(k)
        heads_view(q)[..., 0] = 2.0
        heads_view(k)[..., 0] = 1.5
    elif regime == 'offset':                                 # a common term of 200 in every scaled logit
        heads_view(q)[..., 0] = 16.0
        heads_view(k)[..., 0] = 12.5 / scale
    else:
        assert regime == 'randn', regime
    return q.to(c.dtype), k.to(c.dtype), v.to(c.dtype)


@functools.lru_cache(maxsize=None)
def _case_inputs(case_id, regime, general):
    c = CASE[case_id]
    q, k, v = make_qkv(c, regime)
    ref = fwd_ref(q, k, v, c.ext, c.heads, 'general' if general else case_family(c))
    slim = types.SimpleNamespace(out=ref.out, e_out=ref.e_out, lse=ref.lse, e_lse=ref.e_lse, n=ref.n)
    return types.SimpleNamespace(q=q, k=k, v=v, ref=slim)


def case_inputs(case_id, regime='randn', general=False):
    """The inputs of a case and out / lse with their bounds.  Computed once per process and shared: nobody writes to it.  (The pair
    matrices are not kept: case_pairs.)  general: the bound of the general kernel at a row-route shape."""
    return _case_inputs(case_id, regime, bool(general) and case_family(CASE[case_id]) != 'general')


@functools.lru_cache(maxsize=2)
def case_pairs(case_id, regime='randn'):
    """The full reference of a case, pair matrices included (the indicator launches, the probe)."""
    c = CASE[case_id]
    x = case_inputs(case_id, regime)
    return fwd_ref(x.q, x.k, x.v, c.ext, c.heads, case_family(c))
