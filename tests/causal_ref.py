"""Reference of the time-causal (and, at the kernel level, of any one- or two-sided) attention window, built from the CPU oracle
without restating it.

The law: with the time window (back, fwd) query plane s sees the key planes max(0, s - back) .. min(S - 1, s + fwd); causal is
(eS, 0).  The oracle's attention is symmetric, but run on the planes [lo, hi] = [max(0, p - back), min(S - 1, p + fwd)] ALONE, with
a time extent that covers them all, plane p sees exactly those planes: every other slot of its window falls outside the slice, is
masked with the literal -1e9 and weighs exactly 0 in fp32.  For the causal window that slice is the prefix [:, :p + 1] of the clip
(of which plane p sees the last back + 1 planes only, so the earlier ones are not fed), read at plane p.  Everything per token --
projections, LayerNorm, feed-forward, embedding, logit_proj -- is the oracle's own function, called as it is; all of it is torch
on the CPU, so autograd through these functions is the gradient reference.
"""
import torch
import torch.nn.functional as F

from oracle import attention as oat
from oracle import denoiser as oden


def causal(extents):
    return (int(extents[0]), 0)


def _slice(S, p, window):
    back, fwd = window
    return max(0, p - back), min(S - 1, p + fwd)


def _ext(extents, window):
    return (max(window), int(extents[1]), int(extents[2]))


def local_attention(k, v, q, extents, heads, window=None, return_logits=False):
    """oracle.attention.local_attention under the time window `window` (default: causal).  [B,S,H,W,heads*dh]; with return_logits
    also the masked, scaled logits [B,S,H,W,heads,(back+fwd+1)(2eH+1)(2eW+1)], plane slot ds + back (the kernels' probe order)."""
    window = causal(extents) if window is None else window
    back, fwd = window
    S = q.shape[1]
    e = _ext(extents, window)
    khw = (2 * e[1] + 1) * (2 * e[2] + 1)
    outs, logits = [], []
    for p in range(S):
        lo, hi = _slice(S, p, window)
        o, lg = oat.local_attention(k[:, lo:hi + 1], v[:, lo:hi + 1], q[:, lo:hi + 1], e, heads, return_logits=True)
        outs.append(o[:, p - lo])
        logits.append(lg[:, p - lo, ..., (e[0] - back) * khw:(e[0] + fwd + 1) * khw])       # plane slots ds = -back .. fwd
    out = torch.stack(outs, dim=1)
    return (out, torch.stack(logits, dim=1)) if return_logits else out


def attention_module(params, prefix, x, q, extents, heads, window=None):
    """oracle.attention.attention_module (Local3dAttention.forward(x, q)) under the time window."""
    window = causal(extents) if window is None else window
    S = q.shape[1]
    outs = []
    for p in range(S):
        lo, hi = _slice(S, p, window)
        outs.append(oat.attention_module(params, prefix, x[:, lo:hi + 1], q[:, lo:hi + 1], _ext(extents, window), heads)[:, p - lo])
    return torch.stack(outs, dim=1)


def transformer_layer(params, lp, x, extents, heads):
    """oracle.denoiser.transformer_layer with the causal window: everything but the attention is per token, so the layer on the
    slice, read at plane p, is the causal layer's plane p."""
    window = causal(extents)
    S = x.shape[1]
    outs = []
    for p in range(S):
        lo, hi = _slice(S, p, window)
        outs.append(oden.transformer_layer(params, lp, x[:, lo:hi + 1], _ext(extents, window), heads)[:, p - lo])
    return torch.stack(outs, dim=1)


def transformer_forward(params, z, extents, heads, prefix='transformer.'):
    """The causal Local3dAttentionTransformer: the oracle's embedding, then its layers one by one under the causal window (a whole
    stack cannot run on a slice: its second layer would see, through plane p - 1, what plane p - 1 must not see)."""
    x = oden.embed_tokens(params, z, prefix)
    for l in range(oden.depth_of(params, prefix)):
        x = transformer_layer(params, f'{prefix}layers.{l}.', x, extents, heads)
    return x


def denoiser_forward(params, z, extents, heads):
    """The causal VqVideoDiffusionModel: logits of the last frame."""
    x = transformer_forward(params, z, extents, heads)
    return F.linear(x[:, -1], params['logit_proj.weight'], params['logit_proj.bias'])


def step_grads(params, z, target, extents, heads):
    """oracle.train_step.step_grads over the causal denoiser -> (logits, per-sample loss [B], mean loss, {name: gradient})."""
    leaves = {k: (v.detach().clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in params.items()}
    y = denoiser_forward(leaves, z, extents, heads)
    C = y.shape[-1]
    loss = F.cross_entropy(y.reshape(-1, C), target.reshape(-1), reduction='none')
    per_sample = loss.view(z.shape[0], -1).mean(dim=1)
    loss.mean().backward()
    return y.detach(), per_sample.detach(), loss.mean().detach(), {k: v.grad for k, v in leaves.items() if v.is_floating_point()}
