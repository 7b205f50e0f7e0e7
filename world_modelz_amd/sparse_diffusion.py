"""MI355X drop-in for the model side of minecraft/sparse_diffusion.py (config 5): VqSparseDiffusionModel :75-111 and
the position samplers :31-72.  The training script around them (MineRL loader, wandb) is out of scope."""
import math

import torch
import torch.nn as nn

from . import functional as Fw
from .local_3d_attention import check_model_width
from .transformer import Transformer


def _ranks_of_random_keys(rows, cols, device, generator=None):
    """[rows, cols] int64: row i is a uniform random permutation of 0..cols-1 (argsort of i.i.d. uniform keys)."""
    return torch.rand(rows, cols, device=device, generator=generator).argsort(dim=1)


def sample_flat_positions(batch_size, context_length, s, h, w, device):
    """batch_size * context_length flat grid positions, laid out as consecutive passes over the s*h*w grid, every pass a
    uniform permutation without replacement (semantics of reference :31-41).  One batched argsort instead of the
    reference's randperm-per-pass loop: pass k of the flattened request is row k of the permutation matrix."""
    grid, want = s * h * w, batch_size * context_length
    passes = -(-want // grid)
    perms = _ranks_of_random_keys(passes, grid, device)
    return perms.reshape(-1)[:want].reshape(batch_size, context_length)


def time_window(context_length, s, h, w, t, o=None):
    """Frame window (first frame, number of frames) per batch item for diffusion time t in [0, 1] (reference :53-64):
    the window spans at least ceil(context_length / (h w)) frames, grows linearly with t and is placed by o in [0, 1)
    (uniform when None).  Returns int64 tensors (first, frames)."""
    t = t.reshape(-1).clamp(0, 1)
    need = -(-context_length // (h * w))                     # frames that hold context_length positions
    assert context_length > 0 and need < s
    frames = (need + t * (s - need + 1)).floor().clamp(max=s - need)
    o = torch.rand_like(t) if o is None else o.reshape(-1).to(t.device).clamp(0, 1 - 1e-5)
    first = (o * (s - frames + 1)).floor()
    return first.long(), frames.long()


def sample_time_dependent(batch_size, context_length, s, h, w, t, device, o=None):
    """context_length distinct positions per item, uniform inside the item's frame window (reference :44-72).  The
    reference draws one randperm per batch item in a Python loop; here every item ranks i.i.d. uniform keys over the
    grid, keys outside its window pushed past 1, and keeps the context_length smallest -- the same law (uniform without
    replacement inside the window), one device op for the whole batch."""
    first, frames = time_window(context_length, s, h, w, t.to(device), o)
    grid = s * h * w
    inside = torch.arange(grid, device=device).unsqueeze(0) < (frames * (h * w)).unsqueeze(1)
    keys = torch.where(inside, torch.rand(batch_size, grid, device=device), torch.full((), 2.0, device=device))
    picked = keys.topk(context_length, dim=1, largest=False).indices
    return picked + (first * (h * w)).unsqueeze(1)


class VqSparseDiffusionModel(nn.Module):
    """tokens [B,n] (vocabulary num_classes + 1) at flat grid positions `indices` [B,n] -> logits [B,n,num_classes]."""

    def __init__(self, *, shape, dim, num_classes, depth, dim_head, mlp_dim, heads=1, dropout=0.0):
        super().__init__()
        self.shape = shape
        S, H, W = shape
        self.pos_emb_s = nn.Embedding(S, dim)
        self.pos_emb_h = nn.Embedding(H, dim)
        self.pos_emb_w = nn.Embedding(W, dim)
        self.embedding = nn.Embedding(num_classes + 1, dim)
        self.transformer = Transformer(dim=dim, depth=depth, heads=heads, dim_head=dim_head, mlp_dim=mlp_dim,
                                       dropout=dropout)
        self.logit_proj = nn.Linear(dim, num_classes)

    def pos_embedding_3d(self, indices):
        """fp32 position embedding of flat indices (reference :101-105); inspection helper, torch ops."""
        _, H, W = self.shape
        plane, in_plane = torch.div(indices, H * W, rounding_mode='floor'), indices.remainder(H * W)
        row, col = torch.div(in_plane, W, rounding_mode='floor'), in_plane.remainder(W)
        tables = (self.pos_emb_s.weight, self.pos_emb_h.weight, self.pos_emb_w.weight)
        return sum(tab[ix] for tab, ix in zip(tables, (plane, row, col)))

    def forward(self, x, indices):
        check_model_width(self.embedding.weight.shape[1], 'VqSparseDiffusionModel')
        h = Fw.embed_tokens_indexed(x, indices, self.embedding.weight, self.pos_emb_s.weight, self.pos_emb_h.weight,
                                    self.pos_emb_w.weight, self.shape)
        h = self.transformer.forward_compute(h)
        return Fw.linear(h, self.logit_proj.weight, self.logit_proj.bias, out_f32=True)


# ------------------------------------------------------------------------------------------------ the sampler (reference :99-202)
def categorical_scatter(logits, indices, z_flat, seed, call_id=0, rank=0, counter=None, *, top_k=-1, top_p=1.0, temperature=1.0,
                        known=None, uniforms=None, kept_floor=None, samples=None, scores=None):
    """One multinomial draw per row from softmax(logits) (reference :190-194), written into the clips at the rows' positions
    (:197 `full_z_flat.scatter_`): logits fp32 [B, n, C] (rows at one stride, classes contiguous), indices int64 [B, n], z_flat
    int64 [B, G] (in place).  The draw's Philox stream: (seed, rank, call_id) -- or, with counter (device int64 [1]), the call
    number read on the device.
    temperature (> 0), top_k (<= 0 or >= C: all) and top_p (nucleus, (0, 1]) filter the row by the law include/wmz.h states for
    wmz_categorical_scatter_filtered; known (bool / uint8 [B, G]): positions of z_flat that are given and stay as they are;
    uniforms fp32 [B * n] (u0 per row instead of the generator's), kept_floor fp32 [B * n] (probe: the smallest kept scaled
    logit per row) and samples int64 [B * n] (every row's draw, known or not) as there.  The route: neutral filters and no known --
    wmz_categorical_scatter, as ever; else wmz_categorical_scatter_filtered, rows off the 16-byte granule staged through a padded
    buffer; a filter acting on more classes than ops.sample_max_classes() is applied with torch ops (sample.top_k_logits /
    top_p_logits on the scaled logits) in front of the neutral form of that entry point.
    scores (fp32 [B, G], in place; sample_clips' remask='confidence'): the log-probability of every draw under the softmax of the
    scaled UNFILTERED logits, written where its token is written and nowhere else (wmz_categorical_scatter_scored, which counts it
    as a probe: the row-read-once kernels whatever the filters are); above ops.sample_max_classes(): sample.drawn_log_prob at the
    draws, scattered with torch ops where the position is not known."""
    from . import _lib as L
    B, n, C = logits.shape
    assert logits.dtype == torch.float32 and logits.stride(2) == 1 and indices.is_contiguous() and z_flat.stride(1) == 1
    ld, R = (logits.stride(1) if n > 1 else logits.stride(0) if B > 1 else C), B * n
    assert ld >= C and (B == 1 or logits.stride(0) == n * ld)
    sid = (int(rank) << 40) | (0 if counter is not None else int(call_id) & ((1 << 40) - 1))
    tail = (int(seed) & 0xFFFFFFFFFFFFFFFF, sid, L.ptr(counter), L.stream())
    assert samples is None or (samples.dtype == torch.int64 and samples.is_contiguous() and samples.numel() == R)
    assert scores is None or (scores.dtype == torch.float32 and scores.shape == z_flat.shape and scores.stride(1) == 1)
    probes = uniforms is not None or kept_floor is not None
    acting = 0 < top_k < C or top_p < 1.0 or temperature != 1.0 or probes or scores is not None
    if not acting and known is None:
        L.call('wmz_categorical_scatter', L.ptr(logits), ld, R, C, L.ptr(indices), L.ptr(z_flat), z_flat.stride(0), n, L.ptr(samples), *tail)
        return
    assert uniforms is None or (uniforms.dtype == torch.float32 and uniforms.is_contiguous() and uniforms.numel() == R)
    assert kept_floor is None or (kept_floor.dtype == torch.float32 and kept_floor.is_contiguous() and kept_floor.numel() == R)
    if known is not None:
        assert known.dtype in (torch.bool, torch.uint8) and known.shape == z_flat.shape and known.stride(1) == 1
    given = (L.ptr(known), known.stride(0) if known is not None else 0)
    k, p, inv_t = int(top_k), float(top_p), 1.0 / float(temperature)
    unfiltered = None                                   # the scaled rows whose scores torch ops compute (codebooks above the kernels' limit)
    if acting:
        from . import ops
        from .sample import top_k_logits, top_p_logits
        if C > ops.sample_max_classes():
            if probes:
                raise ValueError(f'uniforms / kept_floor are built for <= {ops.sample_max_classes()} classes (got {C})')
            rows = logits.reshape(R, C) * torch.tensor(inv_t, dtype=torch.float32, device=logits.device)
            if scores is not None:
                unfiltered = rows
                samples = torch.empty(R, dtype=torch.int64, device=logits.device) if samples is None else samples
            if 0 < k < C:
                rows = top_k_logits(rows, k)
            logits, ld, k, p, inv_t = top_p_logits(rows, p).contiguous(), C, -1, 1.0, 1.0
        elif ld % 4 != 0 or logits.data_ptr() % 16 != 0:
            ld = (C + 3) // 4 * 4
            staged = torch.empty(R, ld, dtype=torch.float32, device=logits.device)
            staged[:, :C].copy_(logits.reshape(R, C))
            logits = staged
    dest = (L.ptr(indices), L.ptr(z_flat), z_flat.stride(0), n, L.ptr(samples))
    if scores is None or unfiltered is not None:
        L.call('wmz_categorical_scatter_filtered', L.ptr(logits), ld, R, C, k, p, inv_t, *dest, *given, L.ptr(uniforms),
               L.ptr(kept_floor), *tail)
    else:
        L.call('wmz_categorical_scatter_scored', L.ptr(logits), ld, R, C, k, p, inv_t, *dest, *given, L.ptr(uniforms),
               L.ptr(kept_floor), *tail, L.ptr(scores), scores.stride(0))
    if unfiltered is not None:
        from .sample import drawn_log_prob
        s = drawn_log_prob(unfiltered, samples).view(B, n)
        s = torch.where(s != s, torch.full_like(s, -float('inf')), s)
        if known is not None:                           # (a known position keeps its score as it keeps its token)
            s = torch.where(torch.gather(known, 1, indices) != 0, torch.gather(scores, 1, indices), s)
        scores.scatter_(1, indices, s)


def _check_sampler_arguments(temperature, sample_topp, prompt, shape, num_embeddings, device):
    """sample_clips' filters are sample_frames' (same names, same refusals); prompt: int64 [batch_size, S, H, W] on the model's
    device, tokens in [0, num_embeddings] -- num_embeddings, the mask token, marks what is to be generated."""
    if not temperature > 0 or not temperature < float('inf'):
        raise ValueError(f'temperature must be positive and finite (got {temperature})')
    if not 0 < sample_topp <= 1:
        raise ValueError(f'sample_topp must lie in (0, 1] (got {sample_topp})')
    if prompt is None:
        return
    if not torch.is_tensor(prompt) or prompt.dtype != torch.int64 or tuple(prompt.shape) != tuple(shape):
        raise ValueError(f'prompt must be an int64 tensor of shape {tuple(shape)} '
                         f'(got {tuple(prompt.shape) if torch.is_tensor(prompt) else type(prompt).__name__})')
    if prompt.device != device:
        raise ValueError(f'prompt must live on the model\'s device {device} (got {prompt.device})')
    if prompt.numel() and (int(prompt.min()) < 0 or int(prompt.max()) > int(num_embeddings)):
        raise ValueError(f'prompt tokens must lie in [0, {int(num_embeddings)}] ({int(num_embeddings)}: the mask token, to be generated)')


@torch.no_grad()
def sample_clips(model, batch_size, num_embeddings, sampling_type='neighbors', num_context=512, num_eval_iterations=100,
                 generator=None, seed=None, use_graph=True, *, temperature=1.0, sample_topk=-1, sample_topp=1.0, prompt=None,
                 remask='random', remask_noise=0.0):
    """The token side of the reference's evaluate_model (:139-202): clips [batch_size, S, H, W] that start fully masked and are
    re-drawn num_eval_iterations times -- per iteration G // num_context + 1 contexts, each gathered from the clip, masked with
    probability 1 - i / (iterations - 1), denoised by the model, sampled from softmax(logits) and scattered back.  'neighbors' (the
    reference's default): a context = num_context positions of a frame window of width t = 1 - frac placed at the k-th of the
    iteration's shuffled offsets (sample_time_dependent with o given) -- window, positions, gather and masking are ONE launch
    (wmz_sparse_draw_context with p_uniform = 0), the draw and the scatter another (wmz_categorical_scatter); nothing returns to
    the host inside the loop, and with use_graph the whole sub-step (draw, forward, sample, scatter; the call number counted on
    the device) is ONE hipGraph launch -- same tokens as the eager launches, bit for bit.  'uniform': consecutive num_context-wide slices of one permutation per iteration (the reference
    slices at k * max_index, which is empty from k = 1 on; the evident intent -- k * num_context -- is what runs here).
    temperature (> 0), sample_topk (<= 0: all) and sample_topp ((0, 1]) filter every draw as in sample_frames (the reference's
    results were sampled with top-k 100); ValueError for anything else.  prompt: int64 [batch_size, S, H, W] on the model's device
    -- the clip starts as the prompt instead of all masks; tokens in [0, num_embeddings) are GIVEN: fed to the model as they are,
    never masked, never redrawn; num_embeddings (the mask token) marks what is generated.  ValueError for another shape, device or
    value.  Every route takes them (the fused launches become wmz_sparse_draw_context_known / wmz_categorical_scatter_filtered);
    the defaults run the launches they always ran.
    remask: 'random' -- the reference's law: every context slot is hidden from the model with probability 1 - frac, a coin per slot,
    whatever remask_noise is -- or 'confidence': per context exactly the floor((1 - frac) * num_context) slots the model was least
    sure of are hidden (MaskGIT's rule, as in sample_frames).  The sparse sampler masks when it gathers, so the order lives in a
    score per clip position kept between sub-steps: fp32 [batch_size, G], -inf to start with (a position never drawn is hidden
    first), the log-probability of the position's last draw under the unfiltered tempered softmax afterwards, written by the draw
    beside the token (wmz_categorical_scatter_scored) and read by the next gathers (wmz_sparse_draw_context_scored; include/wmz.h
    states the law, sample.lowest_scores_mask / context_remask_count are its torch form, which the torch-drawn and 'uniform' routes
    apply).  Given positions are never hidden.  remask_noise >= 0 (finite) scales Gumbel noise added to the slot scores, annealed by
    1 - frac.  The captured sub-step stays one hipGraph launch: draw, forward, scored scatter.  ValueError for anything else."""
    if sampling_type not in ('uniform', 'neighbors'):
        raise ValueError('Specified sampling_type not supported')                 # reference :182
    from .sample import REMASK_MODES, context_remask_count, gumbel_from_uniform, lowest_scores_mask
    if remask not in REMASK_MODES:
        raise ValueError(f'remask must be one of {REMASK_MODES} (got {remask!r})')
    if not 0 <= remask_noise < float('inf'):
        raise ValueError(f'remask_noise must be non-negative and finite (got {remask_noise})')
    if num_eval_iterations < 2:
        raise ValueError('num_eval_iterations must be at least 2 (the schedule divides by iterations - 1)')
    S, H, W = (int(v) for v in model.shape)
    G = S * H * W
    dev = model.embedding.weight.device
    _check_sampler_arguments(temperature, sample_topp, prompt, (batch_size, S, H, W), num_embeddings, dev)
    from . import _lib as L
    from .train import draw_sparse_context
    n = int(num_context)
    if prompt is None:
        full_z = torch.full((batch_size, S, H, W), int(num_embeddings), dtype=torch.int64, device=dev)  # all mask tokens (:153-155)
        known = None
    else:
        full_z = prompt.clone()
        known = (prompt != int(num_embeddings)).view(batch_size, -1).to(torch.uint8)        # static: what is given stays given
    flat = full_z.view(batch_size, -1)
    draw = dict(top_k=int(sample_topk), top_p=float(sample_topp), temperature=float(temperature), known=known)
    scores, ordered = None, {}
    if remask == 'confidence':
        scores = torch.full((batch_size, G), -float('inf'), dtype=torch.float32, device=dev)
        draw['scores'] = scores
        ordered = dict(scores=scores, noise=float(remask_noise))
    if seed is None:
        seed = generator.initial_seed() if generator is not None else torch.initial_seed()
    fused = sampling_type == 'neighbors' and bool(L.lib().wmz_sparse_draw_context_supported(S, H * W, n))
    offset_count = G // n + 1
    was_training = model.training
    model.eval()
    graph = None

    def mask_unknown(tokens, indices, frac, r):
        """The torch-drawn routes' masking (:185-187), given positions left as they are; remask='confidence': the torch form of
        wmz_sparse_draw_context_scored's law on the gathered scores."""
        unknown = torch.gather(known, 1, indices) == 0 if known is not None else None
        if scores is None:
            hide = torch.rand(tokens.shape, device=dev) > frac
            if unknown is not None:
                hide &= unknown
        else:
            s = torch.gather(scores, 1, indices)
            if remask_noise > 0:
                amp = torch.tensor(remask_noise, dtype=torch.float32, device=dev) * r.clamp(0, 1)
                s = s + amp.unsqueeze(1) * gumbel_from_uniform(torch.rand(tokens.shape, device=dev))
                s = torch.where(s != s, torch.full_like(s, -float('inf')), s)
            hide = lowest_scores_mask(s, None, unknown, count=context_remask_count(r, tokens.shape[1]))
        return torch.where(hide, torch.full_like(tokens, num_embeddings), tokens)
    if fused and use_graph:
        # one captured sub-step on static inputs: the noise level / window width r, the window placement o, the call counter
        r_s = torch.ones(batch_size, dtype=torch.float32, device=dev)
        o_s = torch.zeros(batch_size, dtype=torch.float32, device=dev)
        ctr = torch.zeros(1, dtype=torch.int64, device=dev)

        def substep():
            ctr.add_(1)
            indices, tokens, _ = draw_sparse_context(full_z, r_s, n, (S, H, W), num_embeddings, seed=seed, rank=0, counter=ctr, o=o_s,
                                                     p_uniform=0.0, known=known, **ordered)
            logits = model(tokens, indices)
            categorical_scatter(logits.float().contiguous(), indices, flat, seed, counter=ctr, **draw)
        from . import config as _cfg
        side = _cfg.shared_stream('warmup')
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            substep()                                   # (allocations and operand caches settle outside the capture)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        from .graph import capture_mode
        with torch.cuda.graph(graph, capture_error_mode=capture_mode()):
            substep()
        # the warm-up wrote tokens (and their scores): start from all masks (or the prompt), call number 0 (+ bit 38)
        if prompt is None:
            full_z.fill_(int(num_embeddings))
        else:
            full_z.copy_(prompt)
        if scores is not None:
            scores.fill_(-float('inf'))
        ctr.fill_(1 << 38)
    try:
        for i in range(num_eval_iterations):
            frac = i / (num_eval_iterations - 1)
            order = torch.randperm(offset_count, generator=generator)                                    # :168 (host)
            if sampling_type == 'uniform':
                perm = torch.randperm(G, device=dev)
            r = torch.full((batch_size,), 1.0 - frac, dtype=torch.float32, device=dev)
            o_rows = (order.float() / (offset_count - 1)).to(dev)[:, None].expand(-1, batch_size).contiguous()
            if graph is not None:
                r_s.copy_(r)
            for k in range(offset_count):
                # the draw's Philox stream id: a function of the seed and the step (bit 38: apart from the trainers' eager call numbers)
                call = (1 << 38) + i * offset_count + k + 1
                if graph is not None:
                    o_s.copy_(o_rows[k])
                    graph.replay()
                    continue
                if sampling_type == 'uniform':
                    idx = perm[k * n:(k + 1) * n]
                    if idx.numel() == 0:
                        continue
                    indices = idx.unsqueeze(0).expand(batch_size, -1).contiguous()
                    tokens = mask_unknown(torch.gather(flat, 1, indices), indices, frac, r)
                elif fused:
                    indices, tokens, _ = draw_sparse_context(full_z, r, n, (S, H, W), num_embeddings, seed=seed, rank=0, o=o_rows[k],
                                                             p_uniform=0.0, call_id=call, known=known, **ordered)
                else:
                    indices = sample_time_dependent(batch_size, n, S, H, W, r, dev, o=o_rows[k])
                    tokens = mask_unknown(torch.gather(flat, 1, indices), indices, frac, r)
                logits = model(tokens, indices)                                                         # [B, n, C] fp32
                categorical_scatter(logits.float().contiguous(), indices, flat, seed, call, **draw)
    finally:
        model.train(was_training)
    return full_z


def decode(decoder_model, batch, decode_N=16):
    """Token clips [B, S, H, W] -> frames [B, S, C, h, w] through the VQ auto-encoder, decode_N frames at a time (reference
    :115-136; tokens beyond the codebook -- left-over mask tokens -- decode as code 0)."""
    batch = batch.clone()
    batch[batch >= decoder_model.vq.num_embeddings] = 0
    shape = batch.shape
    flat = batch.view(-1, shape[2], shape[3])
    frames = torch.cat([decoder_model.decode(flat[i:i + decode_N]) for i in range(0, flat.shape[0], decode_N)])
    return frames.view(shape[0], -1, *frames.shape[1:])


@torch.no_grad()
def evaluate_model(device, batch_size, model, decoder_model, shape, sampling_type, num_context=512, num_eval_iterations=100, *,
                   temperature=1.0, sample_topk=-1, sample_topp=1.0, prompt=None, remask='random', remask_noise=0.0):
    """The reference's evaluate_model (:139-202), same positional signature: sampled clips decoded to frames.  temperature,
    sample_topk, sample_topp, prompt, remask and remask_noise (keyword-only) are sample_clips'."""
    assert tuple(int(v) for v in shape) == tuple(int(v) for v in model.shape)
    z = sample_clips(model, batch_size, decoder_model.vq.num_embeddings, sampling_type, num_context, num_eval_iterations,
                     temperature=temperature, sample_topk=sample_topk, sample_topp=sample_topp, prompt=prompt, remask=remask,
                     remask_noise=remask_noise)
    return decode(decoder_model, z)
