#!/usr/bin/env python3
"""Timing driver of the sampler's context cache (profiles/context_cache/README.md).  One process, device events, the two arms
alternated in groups, warm-up discarded, min / median / max over the groups reported; one JSON line per (mode, batch).

    python tools/time_context_cache.py [--iters 20] [--groups 5] [--batches 1,8,32] [--modes bf16,precise]
                                       [--widths dim,heads,dim_head,mlp] [--depth N] [--clip S,H,W] [--arms uncached,cached]

The benchmark geometry with causal=True (clips of 32 x 16 x 16, codebook 1024, dim 256, one head of 128, window 7 x 7 x 7, depth 4):
  iteration/uncached   one replay of the captured sampler step as it is today: last-frame cone forward + draw + counter
  iteration/cached     one replay of the cached step: model.forward_last on the kept context + draw + counter
  prefill              one replay of the prefill graph (once per frame)
  frame/*              sample_frames, one frame of 30 iterations, end to end (host work and the call's one synchronisation included)
  launch/attention/l   the decode step's attention launch of layer l (one query plane over a[l] + 1 slots)
  launch/per_token/l   the decode step's per-token launch behind layer l, forced to 8 waves per workgroup (one workgroup per clip
                       at 16 x 16; wmz_debug_fused_slots_waves)
  launch/embed         the decode step's embedding launch, forced to 8 waves
  launch/*_w4          the same two on the small-workgroup build (csrc/layer_fused_slots_w4.hip: 4 waves, two workgroups per clip --
                       what the entry points choose for a decode step), captured in the same process, alternated with the 8-wave arms
The iteration, prefill and frame figures run the product rule.
--widths / --depth / --clip time another causal model on the same codebook and window -- a chain-width one
(profiles/context_cache_chain/README.md: --widths 96,1,128,256 --depth 12 --clip 6,16,16): its per-token launches are the chain
kernels' (launch/embed = the embedding launch of one plane plus the chain launch without a head; one workgroup size, no *_w4 arms),
and the line carries the model.  --arms uncached times the uncached arm alone (iteration/uncached, frame/uncached): it runs on a
tree without the cached passes for these widths too.
The launch figures are replays of a graph that holds 20 copies of the launch, divided by 20.  At most 16 host threads."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CFG = dict(S=32, H=16, W=16, C=1024, dim=256, dim_head=128, heads=1, extents=(3, 3, 3), depth=4, mlp_dim=256)     # bench.py's CFG
N_ITER = 30
COPIES = 20


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def alternate(arms, iters, n, scale=1.0):
    """{name: fn} -> {name: stats in us}: every arm once per group, in turn, a discarded warm-up in front."""
    for fn in arms.values():
        timed(fn, 3)
    g = {k: [] for k in arms}
    for _ in range(n):
        for k, fn in arms.items():
            g[k].append(timed(fn, iters) * scale)
    return {k: {'median_us': round(1e3 * statistics.median(v), 2), 'min_us': round(1e3 * min(v), 2), 'max_us': round(1e3 * max(v), 2)}
            for k, v in g.items()}


def copies(fn, waves=0):
    """A graph of COPIES back-to-back copies of the launch fn() -> its replay.  waves: the per-token build the launches are
    captured on (4: the small-workgroup form; the choice is made when a launch is issued, so it is baked into the graph)."""
    from world_modelz_amd import _lib, config
    _lib.call('wmz_debug_fused_slots_waves', waves)
    try:
        return _copies(fn, config)
    finally:
        _lib.call('wmz_debug_fused_slots_waves', 0)


def _copies(fn, config):
    s = config.shared_stream('warmup')
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(COPIES):
            fn()
    return g.replay


def model_config(args):
    """CFG with --widths / --depth / --clip applied (the defaults: CFG itself)."""
    c = dict(CFG)
    if args.widths:
        c['dim'], c['heads'], c['dim_head'], c['mlp_dim'] = (int(v) for v in args.widths.split(','))
    if args.depth:
        c['depth'] = args.depth
    if args.clip:
        c['S'], c['H'], c['W'] = (int(v) for v in args.clip.split(','))
    return c


def measure(mode, B, args):
    from world_modelz_amd import config, fused, sample
    from world_modelz_amd.main import VqVideoDiffusionModel
    torch.manual_seed(0)
    c = model_config(args)
    arms = args.arms.split(',')
    m = VqVideoDiffusionModel(data_shape=(c['S'], c['H'], c['W']), dim=c['dim'], num_classes=c['C'], extents=c['extents'],
                              depth=c['depth'], dim_head=c['dim_head'], mlp_dim=c['mlp_dim'], heads=c['heads'], causal=True).cuda()
    z = torch.randint(0, c['C'], (B, c['S'], c['H'], c['W'])).cuda()
    out = {'mode': mode, 'B': B, 'iters': args.iters, 'groups': args.groups, 'device': torch.cuda.get_device_name(0)}
    if c != CFG:
        out['model'] = {k: c[k] for k in ('dim', 'heads', 'dim_head', 'mlp_dim', 'depth', 'S', 'H', 'W')}
    with config.compute_dtype(mode), torch.no_grad():
        def frame(cache):
            return sample.sample_frames(m, z, c['C'], 1, N_ITER, generator=torch.Generator().manual_seed(1), context_cache=cache)
        if arms == ['uncached']:
            frame(False)
            plain = [s for s in m._wmz_sampler_sessions.values() if s.prefill is None][0]
            out['route'] = fused.inference_route(m.transformer, config.get_fused_dtype(), c['H'], c['W'], z.numel())
            out.update({f'iteration/{k}': v for k, v in alternate({'uncached': lambda: plain.fwd(plain.fwd.static_in)},
                                                                  args.iters, args.groups).items()})
            out.update({f'frame/{k}': v for k, v in alternate({'uncached': lambda: frame(False)}, max(2, args.iters // 5),
                                                              args.groups).items()})
            sample.release_sampler_sessions(m)
            return out
        same = all(torch.equal(a, b) for a, b in zip(frame(True)[0], frame(False)[0]))
        out['same_tokens'] = bool(same)
        ses = {bool(s.prefill is not None): s for s in m._wmz_sampler_sessions.values()}
        cached, plain = ses[True], ses[False]
        out['a'] = cached.cache.a
        out['cone'] = dict(zip(('need', 'src'), fused.cone_planes(c['S'], c['extents'][0], c['depth'])))
        out.update({f'iteration/{k}': v for k, v in alternate(
            {'uncached': lambda: plain.fwd(plain.fwd.static_in), 'cached': lambda: cached.fwd(cached.fwd.static_in)},
            args.iters, args.groups).items()})
        out['prefill'] = alternate({'prefill': lambda: cached.prefill(cached.prefill.static_in)}, args.iters, args.groups)['prefill']
        out.update({f'frame/{k}': v for k, v in alternate({'uncached': lambda: frame(False), 'cached': lambda: frame(True)},
                                                          max(2, args.iters // 5), args.groups).items()})
        # ---- the decode step's launches, one by one
        tr = m.transformer
        layers = list(tr.layers)
        cache = m.context_prefill(z)
        a = cache.a
        bf = cache.dtype
        zc = z.contiguous()
        if cache.family == 'chain':
            out.update(alternate(chain_launches(fused, tr, layers, cache, zc), max(2, args.iters // 2), args.groups, scale=1.0 / COPIES))
            out['family'], out['dtype'] = 'chain', str(bf)
            sample.release_sampler_sessions(m)
            return out
        arms = {'launch/embed': copies(lambda: fused._slots_embed(tr, cache, zc, 1, a[0], True), 8),
                'launch/embed_w4': copies(lambda: fused._slots_embed(tr, cache, zc, 1, a[0], True), 4)}
        x = fused._slots_embed(tr, cache, zc, 1, a[0], True)
        for l, (attn, ff) in enumerate(layers):
            o = fused._slots_attention(cache, l, attn, a[l], 1)
            tail = layers[l + 1] if l + 1 < len(layers) else None
            arms[f'launch/attention/{l}'] = copies(lambda l=l, attn=attn: fused._slots_attention(cache, l, attn, a[l], 1))
            per_token = lambda l=l, o=o, x=x, attn=attn, ff=ff, tail=tail: fused._slots_layer(       # noqa: E731
                cache, l, o, x, 1, 1, (attn, ff), tail, a[l + 1] if tail is not None else 0, True)
            arms[f'launch/per_token/{l}'] = copies(per_token, 8)
            if tail is not None:                 # (the last layer has no tail: the trailing-planes launch, no small form)
                arms[f'launch/per_token_w4/{l}'] = copies(per_token, 4)
            x = fused._slots_layer(cache, l, o, x, 1, 1, (attn, ff), tail, a[l + 1] if tail is not None else 0, True)
        out.update(alternate(arms, max(2, args.iters // 2), args.groups, scale=1.0 / COPIES))
        out['waves_per_workgroup'] = [8, 4]
        out['dtype'] = str(bf)
    sample.release_sampler_sessions(m)
    return out


def chain_launches(fused, tr, layers, cache, zc):
    """The decode step's launches of a chain-width model, one by one (one workgroup size: no small form)."""
    a = cache.a
    arms = {'launch/embed': copies(lambda: fused._slots_embed_chain(tr, cache, zc, 1, a[0]))}
    x = fused._slots_embed_chain(tr, cache, zc, 1, a[0])
    for l, (attn, ff) in enumerate(layers):
        o = fused._slots_attention(cache, l, attn, a[l], 1)
        tail = layers[l + 1] if l + 1 < len(layers) else None
        arms[f'launch/attention/{l}'] = copies(lambda l=l, attn=attn: fused._slots_attention(cache, l, attn, a[l], 1))
        arms[f'launch/per_token/{l}'] = copies(lambda l=l, o=o, x=x, attn=attn, ff=ff, tail=tail: fused._slots_layer_chain(
            cache, l, o, x, 1, 1, (attn, ff), tail, a[l + 1] if tail is not None else 0))
        x = fused._slots_layer_chain(cache, l, o, x, 1, 1, (attn, ff), tail, a[l + 1] if tail is not None else 0)
    return arms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--groups', type=int, default=5)
    ap.add_argument('--batches', default='1,8,32')
    ap.add_argument('--modes', default='bf16,precise')
    ap.add_argument('--widths', default=None, help='dim,heads,dim_head,mlp of the model (default: the benchmark widths)')
    ap.add_argument('--depth', type=int, default=0, help='layers (default: the benchmark depth)')
    ap.add_argument('--clip', default=None, help='S,H,W of a clip (default: the benchmark clip)')
    ap.add_argument('--arms', default='uncached,cached', choices=['uncached,cached', 'uncached'])
    ap.add_argument('--out', default=None, help='append the JSON lines to this file too')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'timings need the GPU'
    torch.set_num_threads(min(16, torch.get_num_threads()))
    for mode in args.modes.split(','):
        for B in (int(b) for b in args.batches.split(',')):
            line = json.dumps(measure(mode, B, args))
            print(line, flush=True)
            if args.out:
                with open(args.out, 'a') as f:
                    f.write(line + '\n')


if __name__ == '__main__':
    main()
