"""References and element-wise error bounds for the optimizer options of csrc/optim.hip: the Adam law (wmz_adam_step, wmz_adam_step_dev),
the clip coefficient and either law behind it (wmz_optim_step_clipped_dev).  A plain helper module for
tests/test_optimizer_options_cpu.py and tests/test_optimizer_options_gpu.py: no fixtures, nothing collected from here.  The checker,
the frames, the unit round-offs and the cases are those of tests/tail_bounds.py, and the derivation follows tail_bounds.adamw_ref:
fp64 on the CPU from the values the kernel receives, one u = 2^-24 per fp32 operation at the size of its result, plus the
propagated errors of its inputs.  Nothing in here comes from a GPU run.

Where the Adam law differs from AdamW's in what can go wrong: gi = gs g + wd p is a SUM that may cancel, so v = b2 v + (1 - b2) gi^2
is no longer known to a relative u-multiple when gi is small against its terms.  The bound therefore carries gi's absolute error
through gi^2 to second order, and takes sqrt's error from |sqrt(x') - sqrt(x)| = |x' - x| / (sqrt(x') + sqrt(x)) <= min(|x' - x| /
sqrt(x), sqrt(|x' - x|)), which holds at any size of the perturbation, not from the first-order half-relative form; the
denominator sqrt(v) / sbc2 + eps is bounded below by eps in the exact and in the computed evaluation alike.
"""
import torch

from tail_bounds import DIV_SQRT_U, U32, f32, f64

CLIP_EPS = 1e-6             # torch.nn.utils.clip_grad_norm_: max_norm / (total_norm + 1e-6)


def law_ref(decoupled, p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale, e_scale=0.0, e_p=None, e_m=None, e_v=None):
    """One step of AdamW (decoupled) or Adam (L2 decay) in fp64 at the fp32 casts of the hyper-parameters:
        AdamW: gi = s g;          p *= 1 - lr wd;  m, v, p as below
        Adam:  gi = s g + wd p;                    m = b1 m + (1 - b1) gi;  v = b2 v + (1 - b2) gi^2;
                                                   p -= (lr / bc1) m / (sqrt(v) / sbc2 + eps)
    s = grad_scale: the exact gradient scale; the kernel holds it to within e_scale (0: a hyper-parameter given by value; behind
    the clip: clip_ref's).  e_p / e_m / e_v: what the incoming state may already be off by.  -> dict(p, e_p, m, e_m, v, e_v)."""
    p, g, m, v = (f64(t) for t in (p, g, m, v))
    z = torch.zeros_like(p)
    e_p0, e_m0, e_v0 = (z if e is None else f64(e) for e in (e_p, e_m, e_v))
    lr, b1, b2, eps, wd = (f32(h) for h in (lr, beta1, beta2, eps, weight_decay))
    gs = float(grad_scale)
    bc1, sbc2 = 1.0 - beta1 ** step, (1.0 - beta2 ** step) ** 0.5
    u = U32
    sg = g * gs
    e_sg = u * sg.abs() + g.abs() * e_scale                     # the product, and the scale's own error
    if decoupled:
        gi, e_gi = sg, e_sg
        dec = 1.0 - lr * wd
        e_dec = u * lr * wd + u * abs(dec)
        p0 = p * dec
        e_p0s = p.abs() * e_dec + u * p0.abs() + abs(dec) * e_p0
    else:
        wp = wd * p                                              # one extra product and one extra sum; no decay factor
        e_wp = u * wp.abs() + wd * e_p0
        gi = sg + wp
        e_gi = e_sg + e_wp + u * gi.abs()
        p0, e_p0s = p, e_p0
    om1, om2 = 1.0 - b1, 1.0 - b2                                # each one fp32 subtraction: u relative
    t1, t2 = b1 * m, om1 * gi
    mi = t1 + t2
    e_mi = 2 * u * t1.abs() + 3 * u * t2.abs() + om1 * e_gi + b1 * e_m0       # products, the factor 1 - b1, the sum; gi's error
    s1, s2 = b2 * v, om2 * gi * gi
    vi = s1 + s2
    e_vi = 2 * u * s1.abs() + 4 * u * s2.abs() + om2 * (2 * gi.abs() * e_gi + e_gi * e_gi) + b2 * e_v0
    sq = vi.sqrt()
    e_sq = torch.where(vi > 0, torch.minimum(e_vi / sq.clamp_min(1e-300), e_vi.sqrt()), e_vi.sqrt()) + DIV_SQRT_U * u * sq
    qd = sq / sbc2
    e_qd = e_sq / sbc2 + (DIV_SQRT_U + 1) * u * qd               # the division, and sbc2's own rounding to fp32
    den = qd + eps
    e_den = e_qd + u * den
    den_lo = (den - e_den).clamp_min(eps * (1 - 4 * u))          # the computed denominator is >= eps (1 - u) whatever v is
    ratio = mi / den
    e_ratio = e_mi / den_lo + mi.abs() * e_den / (den * den_lo) + DIV_SQRT_U * u * (ratio.abs() + e_mi / den_lo)
    stp = lr / bc1
    e_stp = (DIV_SQRT_U + 1) * u * stp                           # the division, and bc1's own rounding to fp32
    upd = stp * ratio
    e_upd = ratio.abs() * e_stp + stp * e_ratio + u * upd.abs()
    pn = p0 - upd
    e_pn = e_p0s + e_upd + u * pn.abs()
    return dict(p=pn, e_p=e_pn, m=mi, e_m=e_mi, v=vi, e_v=e_vi)


def adam_ref(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale, e_scale=0.0, e_p=None, e_m=None, e_v=None):
    """The law of wmz_adam_step (include/wmz.h) with its bound."""
    return law_ref(False, p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, f32(grad_scale) if e_scale == 0.0 else grad_scale,
                   e_scale, e_p, e_m, e_v)


def clip_ref(sq, max_norm, e_sq=0.0):
    """coef = min(1, max_norm / (sqrt(sq) + 1e-6)) as wmz_optim_step_clipped_dev evaluates it in fp32 from the squared norm sq
    (e_sq: how far the word the kernel loads may be from sq) -> (coef, e_coef).  max_norm <= 0: (1, 0)."""
    if max_norm <= 0:
        return 1.0, 0.0
    u = U32
    mx, ce = f32(max_norm), f32(CLIP_EPS)
    s = float(sq) ** 0.5
    e_s = (min(e_sq / s, e_sq ** 0.5) if s > 0 else e_sq ** 0.5) + DIV_SQRT_U * u * s
    d = s + ce
    e_d = e_s + u * d + abs(ce - CLIP_EPS)
    q = mx / d
    e_q = q * e_d / (d - e_d) + DIV_SQRT_U * u * q + abs(mx - max_norm) / d      # (max_norm's own cast to fp32)
    q = max_norm / d
    if q - e_q >= 1.0:
        return 1.0, 0.0                                          # clamped in the kernel and in the reference alike
    return min(1.0, q), e_q


def clipped_ref(decoupled, p, g, m, v, sq, max_norm, lr, beta1, beta2, eps, weight_decay, step, grad_scale, e_sq=0.0, **state_err):
    """clip_ref o the law: the kernel reads the gradient as fl(grad_scale coef) g."""
    coef, e_coef = clip_ref(sq, max_norm, e_sq)
    gs = f32(grad_scale)
    scale = gs * coef
    e_scale = gs * e_coef + (U32 * scale if coef != 1.0 else 0.0)            # coef's error, and the product's rounding
    return law_ref(decoupled, p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, scale, e_scale, **state_err)


def torch_steps(optimizer, p, grads, m, v, lr, beta1, beta2, eps, weight_decay, first_step, grad_scale, max_norm=None):
    """len(grads) successive steps of torch.optim.Adam / AdamW (foreach=False) on fp64 CPU copies, the first one being step
    `first_step` (state seeded with m, v and the step count), each behind torch.nn.utils.clip_grad_norm_(max_norm) when max_norm
    is given -- independent of the kernel's formula -- and the bound of clipped_ref compounded along them, the squared norm taken
    as the fp64 one with the fp32 norm pass's own bound (tail_bounds.sqnorm_ref) as e_sq
    -> (p, e_p, m, e_m, v, e_v, [the pre-clip norms clip_grad_norm_ returned])."""
    from tail_bounds import sqnorm_ref
    P = torch.nn.Parameter(f64(p).clone())
    cls = torch.optim.AdamW if optimizer == 'AdamW' else torch.optim.Adam
    opt = cls([P], lr=lr, betas=(beta1, beta2), eps=eps, weight_decay=weight_decay, amsgrad=False, foreach=False)
    opt.state[P] = dict(step=torch.tensor(float(first_step - 1)), exp_avg=f64(m).clone(), exp_avg_sq=f64(v).clone())
    err = dict(e_p=None, e_m=None, e_v=None)
    norms = []
    for k, g in enumerate(grads):
        st = opt.state[P]
        sq, e_in = sqnorm_ref(g, grad_scale)
        r = clipped_ref(optimizer == 'AdamW', P.detach(), g, st['exp_avg'], st['exp_avg_sq'], sq, max_norm or 0.0, lr, beta1, beta2,
                        eps, weight_decay, first_step + k, grad_scale, e_sq=e_in + U32 * (sq + e_in), **err)
        err = dict(e_p=r['e_p'], e_m=r['e_m'], e_v=r['e_v'])
        P.grad = f64(g) * f32(grad_scale)
        if max_norm is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_([P], max_norm, norm_type=2, foreach=False)))
        opt.step()
    st = opt.state[P]
    return P.detach().clone(), err['e_p'], st['exp_avg'].clone(), err['e_m'], st['exp_avg_sq'].clone(), err['e_v'], norms
