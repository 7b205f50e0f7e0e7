"""MI355X drop-in for the model class of vq-video-diffusion/main.py (VqVideoDiffusionModel, :25-36)."""
import torch
from torch import nn

from . import functional as Fw
from .local_3d_attention import Local3dAttentionTransformer


class VqVideoDiffusionModel(nn.Module):
    """Denoiser: tokens [B,S,H,W] (vocabulary num_classes + 1, the extra id is the mask token) ->
    fp32 logits [B,H,W,num_classes] of the LAST frame only (reference :33-36; quirk Q5).  causal: every attention layer's time
    window is one-sided (Local3dAttention), so no context frame's activation depends on the frame being generated."""

    def __init__(self, *, data_shape, dim, num_classes, extents, depth, dim_head, mlp_dim, heads=1, dropout=.0, causal=False):
        super().__init__()
        self.causal = bool(causal)
        self.transformer = Local3dAttentionTransformer(data_shape=data_shape, dim=dim, num_classes=num_classes + 1,
                                                       extents=extents, depth=depth, heads=heads, dim_head=dim_head,
                                                       mlp_dim=mlp_dim, dropout=dropout, causal=causal)
        self.logit_proj = nn.Linear(dim, num_classes)

    def forward(self, x):
        if not torch.is_grad_enabled() and x.is_cuda:
            from . import config, fused, half_guard
            # (the precise mode with config.half_guard on, where the stack takes the half route: one read-back at the end of the call)
            if half_guard.wanted() and fused.inference_route(self.transformer, config.get_fused_dtype(), x.shape[2], x.shape[3],
                                                             x.numel()) in ('fused', 'chain'):
                return half_guard.guarded('VqVideoDiffusionModel.forward', self, x.device, lambda: self._forward(x))
        return self._forward(x)

    def _forward(self, x):
        if not torch.is_grad_enabled() and x.is_cuda:
            from . import config, fused
            tr = self.transformer
            _, S, H, W = x.shape
            if config.get_last_frame_cone() and fused.inference_route(tr, config.get_fused_dtype(), H, W, x.numel()) == 'fused':
                if S > tr.pos_emb_s.num_embeddings or H > tr.pos_emb_h.num_embeddings or W > tr.pos_emb_w.num_embeddings:
                    raise IndexError('token grid larger than the position-embedding tables')
                last = fused.transformer_forward_last(tr, x)      # only the planes the last frame depends on
                return self._logits(last)
        h = self.transformer.forward_compute(x)
        return self._logits(h[:, -1])         # [B,H,W,D] view: uniform row stride, no copy

    # ---- the context cache (config.context_cache; fused.ContextCache): a causal model's context K / V once per frame

    def _context_cache_refusal(self, z):
        """Why context_prefill / forward_last cannot run on the token grid z now (None: they can)."""
        from . import config, fused
        tr = self.transformer
        if not self.causal:
            return 'the model is not causal: its context planes depend on the frame being generated'
        if len({int(a.fn.extents[0]) for a, _ in tr.layers}) != 1:
            return 'the layers do not share one time extent'
        if torch.is_grad_enabled() or not z.is_cuda:
            return 'the context cache is an inference path on the GPU (call it under torch.no_grad())'
        if z.dim() != 4:
            return f'the token grid is [B, S, H, W], not {tuple(z.shape)}'
        _, S, H, W = z.shape
        dt = config.get_fused_dtype()
        if dt not in (torch.bfloat16, torch.float16) or self._context_cache_family(z) is None:
            return ('only a model whose uncached forward runs the fused or the chain kernels at this grid, in bf16 or in the precise '
                    'mode, keeps a context cache (op-by-op widths, grids the chain kernels do not take, and fp32 run the uncached forward)')
        if S > tr.pos_emb_s.num_embeddings or H > tr.pos_emb_h.num_embeddings or W > tr.pos_emb_w.num_embeddings:
            return 'token grid larger than the position-embedding tables'
        return None

    def _context_cache_family(self, z):
        """The kernel family of the cached passes on the token grid z: that of the UNCACHED forward at this grid -- 'fused', 'chain'
        (the widths of csrc/chain_widths.h where the chain kernels take the grid: always in the precise mode, by config.chain_policy
        in bf16) -- or None."""
        from . import config, fused
        route = fused.inference_route(self.transformer, config.get_fused_dtype(), z.shape[2], z.shape[3], z.numel())
        return route if route in ('fused', 'chain') else None

    def context_cache_eligible(self, z):
        """Whether context_prefill(z) / forward_last(z, cache) would run: a causal model with one time extent, without grad on
        the GPU, on the fused or the chain inference route in bf16 or in the precise mode."""
        return self._context_cache_refusal(z) is None

    def _context_cache_check(self, z):
        why = self._context_cache_refusal(z)
        if why is not None:
            raise ValueError(f'VqVideoDiffusionModel: no context cache here -- {why}')

    def context_prefill(self, z, cache=None):
        """The context pass over z [B, S, H, W] -- everything of z[:, :-1] the last frame can see -- kept as a fused.ContextCache
        (a given cache is refilled in place).  ValueError where context_cache_eligible(z) is False.
        config.half_guard: neither this call nor forward_last is a guarded call of its own -- an overflow of the prefill would have
        to fail every later forward_last on the cache.  Their caller is: sample.sample_frames guards the whole call and repeats
        it uncached on the fp32 route."""
        from . import fused
        self._context_cache_check(z)
        return fused.context_prefill(self.transformer, z, cache, self._context_cache_family(z))

    def forward_last(self, z, cache):
        """forward(z) -- fp32 logits [B, H, W, C] of the last frame, bit for bit -- reading z[:, -1] only: everything of the
        context comes from `cache`, the context_prefill of a grid with the same z[:, :-1].  One plane per launch.  ValueError
        where context_cache_eligible(z) is False."""
        from . import fused
        self._context_cache_check(z)
        return self._logits(fused.transformer_forward_last_cached(self.transformer, z, cache, self._context_cache_family(z)))

    def _logits(self, last):
        # (a half stream -- the precise mode -- takes the half unit of the same GEMM: fp32 accumulation, fp32 logits)
        return Fw.linear(last, self.logit_proj.weight, self.logit_proj.bias, out_f32=True)
