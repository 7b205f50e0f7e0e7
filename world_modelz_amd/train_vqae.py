"""MI355X drop-in for the model class of vq-video-diffusion/train_vqae.py (VqAutoEncoder, :22-55)."""
import torch
import torch.nn as nn

from ._lib import WmzError
from .autoencoder import SimpleResidualDecoder, SimpleResidualEncoder, _grad_path, _pad8, conv_route
from .config import get_compute_dtype
from .vq import VectorQuantizerEMA


class VqAutoEncoder(nn.Module):
    """encoder -> VectorQuantizerEMA -> decoder.  The encoder emits NHWC latents straight into the codebook search
    and the gathered rows go straight into the decoder: the reference's BCHW<->BHWC permutes (:37-41, :47, :53) are
    layout no-ops here."""

    def __init__(self, embedding_dim, num_embeddings, downscale_steps=2, hidden_planes=128, in_channels=3):
        super().__init__()
        self.encoder = SimpleResidualEncoder(in_channels, embedding_dim, downscale_steps, hidden_planes)
        decoder_cfg = [hidden_planes for _ in range(downscale_steps)]
        self.decoder = SimpleResidualDecoder(decoder_cfg, in_channels=embedding_dim, out_channels=in_channels)
        self.vq = VectorQuantizerEMA(embedding_dim, num_embeddings)

    def _latents(self, x):
        return self.encoder.forward_nhwc(x).float()          # [B,h,w,E]; the codebook search is fp32 (whatever route the encoder took)

    def _decode_latents(self, q):
        E = q.shape[-1]
        if _pad8(E) != E:
            q = torch.nn.functional.pad(q, (0, _pad8(E) - E))
        # (the decoder pass's own dtype: the compute dtype, or float16 on the precise mode's half conv route)
        dt = conv_route(self.decoder, q.shape, _grad_path(q, self.decoder))
        return self.decoder.forward_nhwc(q.to(dt).contiguous()).float()

    def _quantized_nhwc(self, x):
        """frames -> (straight-through latents in the decoder's operand dtype, channel-padded for its first conv; commitment loss;
        perplexity): the encoder's NHWC output goes to the quantiser as it is, whose tail kernel writes the decoder's operand."""
        h = self.encoder.forward_nhwc(x)
        st, _, latent_loss, perplexity = self.vq.forward_fused(h, get_compute_dtype(), True)
        return st, latent_loss, perplexity

    def forward(self, x):
        st, latent_loss, perplexity = self._quantized_nhwc(x)
        return self.decoder.forward_nhwc(st).float(), latent_loss, perplexity

    def training_losses(self, x, loss_kind):
        """(reconstruction loss, commitment loss, perplexity) of train_vqae.py:139-150 without the reconstruction as an NCHW fp32
        tensor: the loss (ops.recon_loss: 'SmoothL1' | 'MSE' | 'MAE' | 'L1', reduction mean) reads the decoder's NHWC output in
        place and its backward writes that layout.  x: NCHW fp32 frames on the GPU."""
        from . import ops
        st, latent_loss, perplexity = self._quantized_nhwc(x)
        y = self.decoder.forward_nhwc(st, raw=True)
        return ops.recon_loss(y, x.contiguous(), loss_kind), latent_loss, perplexity

    def encode(self, x):
        h = self._latents(x)
        return self.vq.encode(h).view(h.shape[:-1])

    def decode(self, z):
        return self._decode_latents(self.vq.decode(z))

    # Byte frames at both ends (the reference's data arrives as uint8 [B, T, H, W, C] -- minecraft/main2.py:51-56 -- and every
    # consumer of generated frames wants uint8 [H, W, C] -- main.py:121-132): the raw bytes are uploaded and finished bytes come
    # back; / 255 on the way in and save_image's mul(255).add(0.5).clamp(0, 255) on the way out ride in the two layout launches.

    def encode_frames(self, frames, channels_last=True):
        """uint8 frames [..., H, W, C] (channels_last) or [..., C, H, W] on the GPU -> int64 tokens [..., h, w]: encode() of the
        frames as the reference's transform_batch prepares them (NCHW fp32, byte / 255), without that tensor."""
        if frames.dtype != torch.uint8:
            raise WmzError(f'encode_frames takes uint8 frames, not {frames.dtype} (float frames: encode)')
        h = self.encoder.forward_nhwc(frames, channels_last).float()
        return self.vq.encode(h).view(*frames.shape[:-3], *h.shape[1:-1])

    def decode_frames(self, z, channels_last=True):
        """int64 tokens [..., h, w] -> uint8 frames [..., H, W, C] (channels_last) or [..., C, H, W]: decode() followed by
        save_image's law (ops.nhwc8_to_frames_u8 on the decoder's raw output: no fp32 image, no permute).  All of z is ONE decoder
        batch: with BatchNorm in training mode (quirk Q3) decode what the reference decodes together."""
        from . import ops
        q = self.vq.decode(z)
        lead = q.shape[:-3]
        q = q.reshape(-1, *q.shape[-3:])
        E = q.shape[-1]
        if _pad8(E) != E:
            q = torch.nn.functional.pad(q, (0, _pad8(E) - E))
        dt = conv_route(self.decoder, q.shape, _grad_path(q, self.decoder))          # (the route of _decode_latents)
        y = self.decoder.forward_nhwc(q.to(dt).contiguous(), raw=True)
        out = ops.nhwc8_to_frames_u8(y.detach(), self.decoder.decoder_stack[-1].out_channels, channels_last)
        return out.view(*lead, *out.shape[1:])
