#!/usr/bin/env python3
"""Timing driver of the time-causal attention window (profiles/causal_window/README.md): causal against symmetric in the same
process, eager launches timed with device events, medians over groups; one JSON line.

    python tools/time_causal_window.py kernels [--iters 50] [--groups 5]
        attention forward and backward (dq pass + dk | dv pass, one call) at 8 x 32 x 16 x 16, one head of 128, extents (3, 3, 3):
        symmetric (the entry points without a window), causal (3, 0), symmetric, causal.
    python tools/time_causal_window.py model [--iters 20] [--groups 5]
        the default denoiser (dim 256, one head of 128, depth 4, mlp 256, extents (3, 3, 3)) on 32 clips of (8, 16, 16): bf16 forward
        (last-frame cone and full grid) and the captured training step, symmetric and causal models alternating.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def groups(fn, iters, n):
    timed(fn, 5)
    g = [timed(fn, iters) for _ in range(n)]
    return {'median_us': round(1e3 * statistics.median(g), 2), 'min_us': round(1e3 * min(g), 2), 'max_us': round(1e3 * max(g), 2)}


def kernels(args):
    from world_modelz_amd import ops
    out = {}
    ext, heads, dh = (3, 3, 3), 1, 128
    torch.manual_seed(1)
    q, k, v, do = (torch.randn(8, 32, 16, 16, dh, device='cuda').bfloat16() for _ in range(4))
    saved = {}
    for name, win in (('symmetric', None), ('causal', (3, 0))):
        o, lse, _ = ops.local3d_attention_fwd(q, k, v, ext, heads, need_lse=True, time_window=win)
        saved[name] = (o, lse)
    for rep in range(2):
        for name, win in (('symmetric', None), ('causal', (3, 0))):
            o, lse = saved[name]
            out[f'fwd/{name}/{rep}'] = groups(lambda: ops.local3d_attention_fwd(q, k, v, ext, heads, time_window=win), args.iters, args.groups)
            out[f'fwd_lse/{name}/{rep}'] = groups(lambda: ops.local3d_attention_fwd(q, k, v, ext, heads, need_lse=True, time_window=win),
                                                  args.iters, args.groups)
            out[f'bwd/{name}/{rep}'] = groups(lambda: ops.local3d_attention_bwd(q, k, v, o, lse, do, ext, heads, time_window=win),
                                              args.iters, args.groups)
    return out


def model(args):
    from world_modelz_amd import config, train
    from world_modelz_amd.main import VqVideoDiffusionModel
    out = {}
    C, B, clip = 1024, 32, (8, 16, 16)
    torch.manual_seed(2)
    z = torch.randint(0, C, (B,) + clip, device='cuda')
    with config.compute_dtype(torch.bfloat16):
        models, trainers = {}, {}
        for name in ('symmetric', 'causal'):
            torch.manual_seed(3)
            m = VqVideoDiffusionModel(data_shape=clip, dim=256, num_classes=C, extents=(3, 3, 3), depth=4, dim_head=128, mlp_dim=256,
                                      heads=1, causal=name == 'causal').cuda()
            models[name] = m
            trainers[name] = train.DenoiserTrainer(m, C, lr=1e-4, warmup=2, max_steps=1000, distributed=False)
            trainers[name].enable_graph(z, warmup=2)
        for rep in range(2):
            for name in ('symmetric', 'causal'):
                m, tr = models[name], trainers[name]
                with torch.no_grad():
                    out[f'forward_cone/{name}/{rep}'] = groups(lambda: m(z), args.iters, args.groups)
                    with config.last_frame_cone(False):
                        out[f'forward_full/{name}/{rep}'] = groups(lambda: m(z), args.iters, args.groups)
                out[f'train_step_captured/{name}/{rep}'] = groups(lambda: tr.train_step(z), args.iters, args.groups)
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=['kernels', 'model'])
    ap.add_argument('--iters', type=int, default=None)
    ap.add_argument('--groups', type=int, default=5)
    a = ap.parse_args()
    if a.iters is None:
        a.iters = 50 if a.what == 'kernels' else 20
    res = kernels(a) if a.what == 'kernels' else model(a)
    print(json.dumps({'what': a.what, **res}))
