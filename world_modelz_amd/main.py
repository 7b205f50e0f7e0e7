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

    def _logits(self, last):
        # (a half stream -- the precise mode -- takes the half unit of the same GEMM: fp32 accumulation, fp32 logits)
        return Fw.linear(last, self.logit_proj.weight, self.logit_proj.bias, out_f32=True)
