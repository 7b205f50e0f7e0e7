"""Iterative-unmasking sampler (the inference caller of the denoiser): build-owned counterpart of
vq-video-diffusion/main.py:evaluate_model (:50-117) -- SURVEY 8f N2.

Per generated frame: the last latent frame starts fully masked; 30 denoise iterations of
{top-k filter -> softmax -> multinomial -> re-mask a (1 - frac) share -> write into the last frame -> model.forward};
then the frames shift by one.  Everything stays on the GPU: the forward is ONE hipGraph launch per iteration
(GraphedForward), sampling uses device RNG, and there is no host sync inside a frame.
"""
import torch
import torch.nn.functional as F

from .graph import GraphedForward


def top_k_logits(logits, k):
    """Keep the k largest logits per row, -inf elsewhere (main.py:39-43)."""
    v, _ = torch.topk(logits, k, largest=True, sorted=True)
    return logits.masked_fill(logits < v[:, [-1]], -float('inf'))


def top_p_logits(logits, p):
    """Nucleus filter: per row keep {w >= t}, w = exp(logits - max) and t the largest weight whose classes {w >= t} hold at least
    p of the row's total weight -- the smallest set of most probable classes whose mass reaches p, ties with its weakest member
    kept -- and -inf elsewhere (rows already filtered by top_k_logits: their -inf entries weigh 0 and stay out).  p >= 1: the
    logits as they are.  The law of the fused kernel (include/wmz.h wmz_sample_tokens_filtered_dev)."""
    if p >= 1.0:
        return logits
    w = (logits - logits.max(dim=-1, keepdim=True).values).exp()
    ws, _ = torch.sort(w, dim=-1, descending=True)
    mass = ws.cumsum(dim=-1)                                     # mass[j] = weight of {w >= ws[j]} once ties are passed ...
    reached = mass >= p * mass[:, [-1]]
    first = reached.float().argmax(dim=-1, keepdim=True)         # ... so the first j that reaches p names the threshold weight
    return logits.masked_fill(w < ws.gather(-1, first), -float('inf'))


def categorical_from_uniform(p, u):
    """Inverse-CDF categorical draw: the first class whose cumulative weight exceeds u * total (u in [0, 1), one per row).
    This is the definition the sampler-parity fixtures are captured with (torch.multinomial replaced by it inside the
    reference's evaluate_model, tests/golden/make_golden.py), so with the same uniforms the draws are the reference's."""
    cdf = p.cumsum(dim=-1)
    x = (u.to(cdf.dtype) * cdf[:, -1]).unsqueeze(-1)
    return (cdf <= x).sum(dim=-1).clamp(max=p.shape[-1] - 1)


# Confidence-ordered re-masking, the torch form of the law that include/wmz.h states next to wmz_sample_tokens_scored_dev and
# wmz_remask_lowest_dev: what the torch path of sample_frames applies and what the two kernels are held to.

def drawn_log_prob(logits, draws):
    """Score of each row's draw: its log-probability under the softmax of `logits` [R, C] -- the scaled logits BEFORE top-k and the
    nucleus -- in fp32 (log_softmax gathered at draws [R]).  Over all classes, not the kept set: under top-k = 1 the kept-set
    probability is 1 in every row and would order nothing."""
    return F.log_softmax(logits.float(), dim=-1).gather(-1, draws.reshape(-1, 1)).squeeze(-1)


def gumbel_from_uniform(u):
    """g = -log(-log(u)) in fp32 for u in [0, 1): u = 0 gives -inf (that row is re-masked first)."""
    return -torch.log(-torch.log(u.float()))


def confidence_scores(logits, draws, alpha, noise=0.0, u=None):
    """drawn_log_prob, plus noise * (1 - alpha) * gumbel_from_uniform(u) where noise > 0 (fp32 throughout; with noise == 0 the term
    is not evaluated: no 0 * inf); a NaN score becomes -inf."""
    s = drawn_log_prob(logits, draws)
    if noise > 0:
        one, a = torch.tensor(1.0, dtype=torch.float32), torch.tensor(alpha, dtype=torch.float32)
        s = s + (torch.tensor(noise, dtype=torch.float32) * (one - a)).to(s.device) * gumbel_from_uniform(u.reshape(-1))
    return torch.where(s != s, torch.full_like(s, -float('inf')), s)


def remask_count(alpha, rows):
    """m = floor((1 - alpha) * rows) as the kernel computes it: alpha and rows in fp32, one subtract, one multiply."""
    one, a = torch.tensor(1.0, dtype=torch.float32), torch.tensor(alpha, dtype=torch.float32)
    return int(torch.floor((one - a) * torch.tensor(float(rows), dtype=torch.float32)))


def score_keys(scores):
    """Order-preserving integer key of an fp32 score's bits (all bits of a negative flipped, the sign bit of the others set -- the
    transform of the kernels' threshold searches), as int64: -inf < ... < -0.0 < +0.0 < ... < +inf, NaNs by their bits."""
    b = scores.float().contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return torch.where(b >= 0x80000000, 0xFFFFFFFF - b, b + 0x80000000)


def context_remask_count(r, n):
    """Config 5's count: m = floor(clamp(r, 0, 1) * n) per clip as wmz_sparse_draw_context_scored computes it -- r [B] and n in fp32,
    one multiply.  -> int64 [B]."""
    rc = torch.as_tensor(r, dtype=torch.float32).reshape(-1).clamp(0, 1)
    return torch.floor(rc * torch.tensor(float(n), dtype=torch.float32, device=rc.device)).to(torch.int64)


def lowest_scores_mask(scores, alpha, candidates=None, count=None):
    """Which positions go back to the mask token: per clip (row of scores [B, HW]) the min(m, #candidates) candidates with the lowest
    scores, m = remask_count(alpha, HW) -- or, with count (an int, or int64 [B]: context_remask_count, the sparse sampler's, whose
    m comes from r), that count, alpha unread; candidates: bool [B, HW] (default: all).  Order by score_keys, ties to the lower
    index.  -> bool [B, HW]."""
    B, HW = scores.shape
    m = remask_count(alpha, HW) if count is None else count
    if torch.is_tensor(m):
        m = m.to(scores.device).reshape(B, 1)
    cand = torch.ones(B, HW, dtype=torch.bool, device=scores.device) if candidates is None else candidates.to(torch.bool)
    idx = torch.arange(HW, device=scores.device)
    # one unique sort key per position: (non-candidates last, key, index)
    order = (torch.where(cand, score_keys(scores), torch.full((), 1 << 32, dtype=torch.int64, device=scores.device)) * HW + idx).argsort(dim=-1)
    rank = torch.empty_like(order).scatter_(-1, order, idx.expand(B, HW))
    return cand & (rank < torch.minimum(cand.sum(-1, keepdim=True), torch.as_tensor(m, device=scores.device)))


REMASK_MODES = ('random', 'confidence')


def _use_context_cache(model, batch_z, context_cache):
    """sample_frames' context_cache argument resolved: None reads config.context_cache and keeps the uncached path on a model that
    is not eligible (VqVideoDiffusionModel.context_cache_eligible); True on such a model is a ValueError."""
    from . import config
    if not (config.get_context_cache() if context_cache is None else bool(context_cache)):
        return False
    eligible = getattr(model, 'context_cache_eligible', None)
    if eligible is not None and eligible(batch_z):
        return True
    if context_cache is None:
        return False
    if eligible is None:
        raise ValueError(f'context_cache=True: {type(model).__name__} has no context cache (VqVideoDiffusionModel.context_prefill)')
    model._context_cache_check(batch_z)                           # raises, naming what is missing


@torch.no_grad()
def sample_frames(model, batch_z, num_embeddings, num_frames, num_eval_iterations=30, sample_topk=-1, noise_schedule=None,
                  consistent_masking=False, generator=None, use_graph=True, uniforms=None, trace=None, temperature=1.0,
                  sample_topp=1.0, *, remask='random', remask_noise=0.0, context_cache=None):
    """batch_z: int64 [B,S,H,W] context tokens on the GPU (the last frame is overwritten).  Returns the list of generated
    latent frames [B,H,W] (decode them with VqAutoEncoder.decode) and the final batch_z.

    uniforms = (u_multi [num_frames, num_eval_iterations, B*H*W], u_mask [num_frames, num_eval_iterations, B, H*W]):
    injected randomness -- the categorical draw becomes categorical_from_uniform and the re-mask field u_mask > alpha
    (main.py:85, :97-100), which makes the loop a deterministic function of its inputs (parity tests); default: device RNG.
    trace: optional list that receives every last frame fed to the model.
    temperature (> 0) divides the logits in front of the filters; sample_topp in (0, 1] is the nucleus filter (top_p_logits)
    behind top-k: ValueError for anything else.  The defaults leave every draw as it was.
    remask: 'random' -- the reference's law: a position goes back to the mask token where its uniform exceeds alpha -- or
    'confidence': per clip exactly the floor((1 - alpha) * H * W) positions whose draws the model was least sure of
    (confidence_scores + lowest_scores_mask above; with consistent_masking among the positions masked before), the rule of
    masked-token decoders (MaskGIT).  remask_noise >= 0 (finite) scales the Gumbel noise added to the scores, annealed by
    (1 - alpha); its uniform is u_mask[f, i] when injected.  ValueError for anything else.  (Config 5's sampler,
    sparse_diffusion.sample_clips, takes all of these too: it masks when it gathers a context, so its 'confidence' orders that
    masking by a score kept per clip position between sub-steps.)
    context_cache: True -- a causal model on the fused or the chain kernels' widths computes the context planes' K / V once per frame
    (model.context_prefill) and the generated plane alone per iteration (model.forward_last): the same logits bit for bit, hence
    the same tokens; ValueError on a model that is not eligible.  None (default) reads config.context_cache and keeps the
    uncached path where the model is not eligible; False: the uncached path."""
    assert batch_z.is_cuda
    if remask not in REMASK_MODES:
        raise ValueError(f'remask must be one of {REMASK_MODES} (got {remask!r})')
    if not 0 <= remask_noise < float('inf'):
        raise ValueError(f'remask_noise must be non-negative and finite (got {remask_noise})')
    if not temperature > 0 or not temperature < float('inf'):
        raise ValueError(f'temperature must be positive and finite (got {temperature})')
    if not 0 < sample_topp <= 1:
        raise ValueError(f'sample_topp must lie in (0, 1] (got {sample_topp})')
    from . import half_guard
    use_cache = _use_context_cache(model, batch_z, context_cache)
    if half_guard.wanted():
        # config.half_guard: the whole call is one guarded call (its forwards only accumulate into the word); a fallback repeats
        # it on the fp32 route with the random state it started from, so the tokens are the fp32 mode's
        gens = [generator] if generator is not None else [torch.default_generator, torch.cuda.default_generators[batch_z.device.index]]
        states = [g.get_state() for g in gens]
        args = (model, batch_z, num_embeddings, num_frames, num_eval_iterations, sample_topk, noise_schedule, consistent_masking,
                generator, use_graph, uniforms)

        def again():
            for g, st in zip(gens, states):
                g.set_state(st)
            if trace is not None:
                del trace[:]
            return sample_frames(*args, context_cache=False, **kwargs)     # (the fp32 route keeps no context cache)
        kwargs = dict(trace=trace, temperature=temperature, sample_topp=sample_topp, remask=remask, remask_noise=remask_noise)
        return half_guard.guarded('sample.sample_frames', model, batch_z.device,
                                  lambda: sample_frames(*args, context_cache=use_cache, **kwargs), again)
    B, S, H, W = batch_z.shape
    mask_token = num_embeddings
    batch_z = batch_z.clone()
    batch_z[:, -1] = mask_token                                   # destroy all information in the last frame (:62)
    from . import ops
    confidence = remask == 'confidence'
    if (use_graph and uniforms is None and trace is None and num_embeddings <= ops.sample_max_classes()
            and (not confidence or H * W <= ops.remask_max_rows())):
        return _sample_frames_fused(model, batch_z, num_embeddings, num_frames, num_eval_iterations, sample_topk, noise_schedule,
                                    consistent_masking, generator, temperature, sample_topp, remask, remask_noise, use_cache)
    fwd = GraphedForward(model, batch_z) if use_graph and not use_cache else None     # (the cached steps run eagerly here)
    cache = None
    if fwd is not None:
        batch_z = fwd.static_in                                   # the loop edits the graph's own input buffer: no staging copy
    dev = batch_z.device
    if uniforms is not None:
        u_multi, u_mask = (t.to(dev) for t in uniforms)
        assert u_multi.shape[:2] == (num_frames, num_eval_iterations) and u_mask.shape[:2] == (num_frames, num_eval_iterations)
    inv_temperature = torch.tensor(1.0 / temperature, dtype=torch.float32, device=dev)     # (the fp32 value the kernel multiplies by)
    out = []
    for f in range(num_frames):
        logits = torch.zeros(B * H * W, num_embeddings, device=dev)      # flat start (:71)
        last_mask = torch.ones(B, H * W, dtype=torch.bool, device=dev)
        if use_cache:
            cache = model.context_prefill(batch_z, cache)         # the frame's context: fixed until the shift below
        for i in range(num_eval_iterations):
            if temperature != 1.0:
                logits = logits * inv_temperature
            unfiltered = logits
            if sample_topk > 0:
                logits = top_k_logits(logits, sample_topk)
            logits = top_p_logits(logits, sample_topp)
            p = F.softmax(logits, dim=-1)
            if uniforms is not None:
                denoised = categorical_from_uniform(p, u_multi[f, i].reshape(-1)).view(B, H * W)
            else:
                denoised = torch.multinomial(p, 1, True, generator=generator).view(B, H * W)
            frac = (i + 1) / num_eval_iterations
            alpha = min(max(noise_schedule(frac) if noise_schedule is not None else frac, 0.0), 1.0)
            if not confidence or remask_noise > 0:
                u = u_mask[f, i].view(B, H * W) if uniforms is not None else torch.rand(B, H * W, device=dev, generator=generator)
            if confidence:
                scores = confidence_scores(unfiltered, denoised, alpha, remask_noise, u if remask_noise > 0 else None).view(B, H * W)
                mask = lowest_scores_mask(scores, alpha, last_mask if consistent_masking else None)
                if consistent_masking:
                    last_mask = mask
            else:
                mask = u > alpha
                if consistent_masking:
                    mask = last_mask & mask
                    last_mask = mask
            frame = torch.where(mask, torch.full_like(denoised, mask_token), denoised)
            batch_z[:, -1] = frame.view(B, H, W)
            if trace is not None:
                trace.append(frame.view(B, H, W).clone())
            if i + 1 < num_eval_iterations:                       # (the reference runs the model behind a frame's last draw too, :111,
                #                                                    and never reads those logits)
                y = model.forward_last(batch_z, cache) if use_cache else (fwd(batch_z) if fwd is not None else model(batch_z))
                logits = y.reshape(B * H * W, num_embeddings).float()
        out.append(denoised.view(B, H, W).clone())
        batch_z[:, :-1] = batch_z[:, 1:].clone()                  # shift frames (:115)
    return out, (batch_z.clone() if fwd is not None else batch_z)   # (never hand out the graph's own buffer)


@torch.no_grad()
def predict_frames(model, ae, context, num_embeddings, num_frames, channels_last=True, **sampler_kwargs):
    """The reference's evaluate_model (main.py:50-132) with the context frames given instead of drawn from a dataset, bytes in and
    bytes out: context uint8 [B, S-1, H, W, C] (channels_last; else [B, S-1, C, H, W]) on the GPU -> (frames uint8
    [B, num_frames, H, W, C] (or [B, num_frames, C, H, W]), the final batch_z).  VqAutoEncoder.encode_frames on the context (one
    encoder batch of B (S-1) frames), a mask frame appended, sample_frames(**sampler_kwargs), VqAutoEncoder.decode_frames on ONE
    generated frame -- B images -- at a time as main.py:113 does: the decoder's BatchNorm runs in training mode there (quirk Q3),
    and another decode batch would be other statistics."""
    if context.dim() != 5:
        raise ValueError(f'context is uint8 [B, S-1, H, W, C] or [B, S-1, C, H, W], not {tuple(context.shape)}')
    z = ae.encode_frames(context, channels_last)                                      # [B, S-1, h, w]
    batch_z = torch.cat([z, torch.full_like(z[:, :1], num_embeddings)], dim=1)        # (sample_frames masks the last frame itself)
    latents, batch_z = sample_frames(model, batch_z, num_embeddings, num_frames, **sampler_kwargs)
    frames = torch.stack([ae.decode_frames(zf, channels_last) for zf in latents], dim=1)
    return frames, batch_z


MAX_SESSIONS = 2          # captured sampler steps kept per model (least recently used beyond that are dropped: a graph, its
#                           buffers and its references to the operand copies are ~tens of MB each)


class _Sessions(dict):
    """The model's captured sampler steps, most recently used last.  They belong to THIS module object on THIS device: a copy of the
    model (copy.deepcopy, pickling the module) starts without them instead of failing on the hipGraph inside."""

    def __deepcopy__(self, memo):
        return _Sessions()

    def __reduce__(self):
        return (_Sessions, ())

    def touch(self, key, make):
        ses = self.pop(key, None)
        if ses is None:
            ses = make()
        self[key] = ses                                   # (re-inserted: dicts keep insertion order)
        while len(self) > MAX_SESSIONS:
            del self[next(iter(self))]
        return ses


class _WeakModel:
    """What a session's graph runner holds instead of the model: a weak reference.  model -> sessions -> session -> runner -> model
    was a reference cycle -- a dropped model, its hipGraphs and their private pools were freed only by the cyclic collector,
    whenever that ran (possibly in the middle of another stream capture); now dropping the model frees them at once."""

    def __init__(self, model, call=None):
        """call(model, z): what the runner captures instead of model(z) (the cached sampler's prefill and decode step)."""
        import weakref
        self._ref = weakref.ref(model)
        self._call = call

    def _model(self):
        m = self._ref()
        if m is None:
            raise RuntimeError('the model of this sampler session no longer exists')
        return m

    def parameters(self):
        return self._model().parameters()

    def buffers(self):
        return self._model().buffers()

    def __call__(self, z):
        return self._model()(z) if self._call is None else self._call(self._model(), z)


def release_sampler_sessions(model):
    """Drop the captured sampler steps kept with `model` (their graphs, device buffers and operand references) now."""
    ses = model.__dict__.pop('_wmz_sampler_sessions', None)
    if ses is not None:
        ses.clear()


_SEED_KEY = 0x9E3779B97F4A7C15                   # the captured kernels' Philox key (a kernel ARGUMENT, i.e. baked into the graph):
#                                                   what varies per call is the device-side counter's starting value
# (the sessions live ON the model -- `model._wmz_sampler_sessions`, {configuration: captured sampler step + its device buffers},
#  at most MAX_SESSIONS of them -- and die with it: the graph runner of a session holds the model weakly (_WeakModel))


class _Session:
    """One captured sampler step (forward + draw of the next iteration + counter) and the device state it works on, kept with the
    model across sample_frames calls: capturing costs ~4 ms, a frame of 30 iterations ~11 (GraphedForward re-captures by itself
    when the weights, the compute dtype or the run-time configuration changed).  context_cache: the session owns a
    fused.ContextCache and TWO graphs on one token grid -- the prefill (once per frame) and the decode step (model.forward_last
    between today's pre / post work)."""

    def __init__(self, model, batch_z, C, n_iter, sample_topk, consistent_masking, temperature=1.0, sample_topp=1.0, remask='random',
                 remask_noise=0.0, context_cache=False):
        from . import config, fused, ops
        B, S, H, W = batch_z.shape
        dev = batch_z.device
        R = B * H * W
        self.alphas = torch.zeros(n_iter, dtype=torch.float32, device=dev)
        self.logits = torch.zeros(R, (C + 3) // 4 * 4, dtype=torch.float32, device=dev)[:, :C]     # rows 16-byte aligned whatever C is
        self.denoised = torch.zeros(R, dtype=torch.int64, device=dev)
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)
        self.last_mask = torch.ones(R, dtype=torch.uint8, device=dev) if consistent_masking else None
        self.scores = torch.zeros(R, dtype=torch.float32, device=dev) if remask == 'confidence' else None     # (the graph's own)
        aligned = C % 4 == 0
        holder = {}

        def draw(src, z):
            if remask == 'confidence':
                ops.sample_tokens_confidence(src, sample_topk, self.alphas, C, z[:, -1], self.denoised, self.counter, _SEED_KEY,
                                             self.last_mask, top_p=sample_topp, temperature=temperature, noise=remask_noise,
                                             scores=self.scores)
            else:
                ops.sample_tokens(src, sample_topk, self.alphas, C, z[:, -1], self.denoised, self.counter, _SEED_KEY, self.last_mask,
                                  top_p=sample_topp, temperature=temperature)
            self.counter.add_(1)

        def pre(z):
            holder['z'] = z

        def post(y):
            src = y.reshape(R, C)
            if not aligned:
                self.logits.copy_(src)
                src = self.logits
            draw(src, holder['z'])
        self.draw = draw
        self.prefill = None
        if not context_cache:
            self.fwd = GraphedForward(_WeakModel(model), batch_z, pre=pre, post=post)
            return
        cache = self.cache = fused.ContextCache(model.transformer, B, S, H, W, config.get_fused_dtype(), dev)
        self.fwd = GraphedForward(_WeakModel(model, lambda m, z: m.forward_last(z, cache)), batch_z, pre=pre, post=post)
        self.prefill = GraphedForward(_WeakModel(model, lambda m, z: m.context_prefill(z, cache).q[0]), batch_z,
                                      static_in=self.fwd.static_in)


def _sample_frames_fused(model, batch_z, num_embeddings, num_frames, num_eval_iterations, sample_topk, noise_schedule,
                         consistent_masking, generator, temperature=1.0, sample_topp=1.0, remask='random', remask_noise=0.0,
                         context_cache=False):
    """The same loop with NO host work inside a frame but one graph launch per iteration: the draw + re-mask step is one
    kernel (wmz_sample_tokens_dev, or wmz_sample_tokens_filtered_dev with a temperature, a nucleus filter or more than 2048 classes
    -- up to ops.sample_max_classes(): temperature, top-k, softmax, top-p, inverse-CDF draw and re-mask per row, uniforms from in-kernel Philox indexed
    by a device-side iteration counter that starts, per call, at a draw from the caller's generator) captured BEHIND the forward
    whose logits it reads, the counter increment behind it.  One graph replay = the forward on the current grid + the draw of the
    NEXT iteration from its logits (read where the graph leaves them: no hand-over copy when the rows are 16-byte aligned).  A
    frame's first draw (from the flat start, :71) is one eager launch in front of its replays, and the forward behind a frame's
    LAST draw -- whose logits the reference computes (:111) and never reads -- is not run: n - 1 forwards per frame instead of n.
    The captured step stays with the model between calls (_Session).  Same distribution as the torch path (which stays for
    injected uniforms: the parity fixtures), different random stream.
    remask = 'confidence': the step is TWO kernels -- the scored draw (wmz_sample_tokens_scored_dev) and the per-clip selection of the
    lowest scores (wmz_remask_lowest_dev) -- captured in the same place.
    context_cache: a frame is one replay of the prefill graph, then n - 1 replays of the decode graph (forward_last + draw + counter):
    still no host sync inside a frame, one graph launch per iteration plus one per frame."""
    from . import config
    B, S, H, W = batch_z.shape
    n = num_eval_iterations
    # (the cached session's buffers are in the fused dtype: another mode is another session, not a re-capture)
    key = (B, S, H, W, num_embeddings, n, int(sample_topk), bool(consistent_masking), batch_z.device,
           bool(context_cache), config.get_fused_dtype() if context_cache else None, str(remask), float(remask_noise),
           float(temperature), float(sample_topp))
    per_model = model.__dict__.setdefault('_wmz_sampler_sessions', _Sessions())
    ses = per_model.touch(key, lambda: _Session(model, batch_z, num_embeddings, n, sample_topk, consistent_masking,
                                                     temperature, sample_topp, remask, remask_noise, context_cache))
    ses.alphas.copy_(torch.tensor([min(max(noise_schedule((i + 1) / n) if noise_schedule is not None else (i + 1) / n, 0.0), 1.0)
                                   for i in range(n)], dtype=torch.float32))
    # The Philox stream is indexed by the counter; a call starts it at a 62-bit draw from the caller's generator (the global CPU
    # generator when none is passed) rounded to a multiple of n (the kernel takes alpha = alphas[counter % n]), which advances
    # that generator like the reference's torch.multinomial / torch.rand do: two calls in a row see different noise, reseeding
    # the generator reproduces a call.  (A CUDA generator costs one device sync per call here.)
    base = int(torch.randint(0, 1 << 62, (1,), generator=generator,
                             device=generator.device if generator is not None else 'cpu').item()) // n * n
    fwd = ses.fwd
    fwd.refresh()                                                 # (a re-capture draws: before the call's state is set up, not inside it)
    if ses.prefill is not None:
        ses.prefill.refresh()
    z = fwd.static_in
    z.copy_(batch_z)                                              # (the capture / the previous call drew into the last frame)
    ses.counter.fill_(base)
    out = []
    for f in range(num_frames):
        if ses.prefill is not None:
            ses.prefill(z)                                        # the frame's context K / V: fixed until the shift below
        ses.logits.zero_()                                        # flat start (:71)
        if ses.last_mask is not None:
            ses.last_mask.fill_(1)
        ses.draw(ses.logits, z)                                   # iteration 0
        for i in range(1, n):
            fwd(z)                                                # forward of iteration i - 1, draw of iteration i
        out.append(ses.denoised.view(B, H, W).clone())
        z[:, :-1] = z[:, 1:].clone()                              # shift frames (:115)
    return out, z.clone()
