#!/usr/bin/env python3
"""Timing driver of the sampler loop over narrow and wide codebooks (profiles/sampler_filters/README.md): sample_frames on
8 clips of 32x16x16 latents (2048 rows per draw), the default denoiser, bf16, 30 denoise iterations, top-k 100, with

    c1024    1024 codes, default arguments: the register kernel, the route every tree takes
    c8192    8192 codes, default arguments: the workgroup-per-row kernel inside the captured step -- or, in a tree whose fused
             route stops at 2048 classes, the host-driven loop (torch.topk / softmax / torch.multinomial between graph replays)
    c8192_f  8192 codes with temperature 0.7 and sample_topp 0.9 (trees that take them)

in ONE process, in alternating groups, host clock around calls that end in a synchronise.

    python tools/time_sampler_filters.py [--calls 10] [--groups 7] [--root DIR]
        one JSON line: median / min / max ms per denoise iteration over the groups, (max - min) / median as the spread.
        --root: the tree to import world_modelz_amd from (compare two checkouts by running the tool once for each)
    python tools/time_sampler_filters.py --replay 8192|16384 [--calls 2] [--filters]
        nothing but that many sample_frames calls at that codebook size: the program to put behind
        `rocprofv3 --kernel-trace --stats --`
"""
import argparse
import inspect
import json
import statistics
import sys
import time

import torch

SHAPE, CLIPS, N_ITER, TOP_K = (32, 16, 16), 8, 30, 100
FILTERS = dict(temperature=0.7, sample_topp=0.9)


def build(C, **kw):
    from world_modelz_amd.main import VqVideoDiffusionModel
    from world_modelz_amd.sample import sample_frames
    torch.manual_seed(42)
    m = VqVideoDiffusionModel(data_shape=SHAPE, dim=256, num_classes=C, extents=(3, 3, 3), depth=4, dim_head=128, mlp_dim=256,
                              heads=1).cuda().eval()
    z = torch.randint(0, C, (CLIPS,) + SHAPE, device='cuda')
    def call():                                         # (the global generators: what both the fused and the host-driven loop take)
        sample_frames(m, z, C, 1, num_eval_iterations=N_ITER, sample_topk=TOP_K, **kw)
    return call


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (calls * N_ITER) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--groups', type=int, default=7)
    ap.add_argument('--root', default='.')
    ap.add_argument('--replay', type=int, default=None)
    ap.add_argument('--filters', action='store_true')
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    from world_modelz_amd import config, sample
    if not torch.cuda.is_available():
        raise SystemExit('no GPU: a timing from anywhere else says nothing')
    config.set_compute_dtype(torch.bfloat16)
    has_filters = 'sample_topp' in inspect.signature(sample.sample_frames).parameters
    if args.replay:
        fn = build(args.replay, **(FILTERS if args.filters else {}))
        for _ in range(args.calls):
            fn()
        torch.cuda.synchronize()
        return
    variants = {'c1024': build(1024), 'c8192': build(8192)}
    if has_filters:
        variants['c8192_f'] = build(8192, **FILTERS)
    for fn in variants.values():                        # every shape warm (captures, operand copies, allocator) before a clock starts
        timed(fn, 2)
    groups = {name: [] for name in variants}
    for _ in range(args.groups):                        # a, b, c, a, b, c, ...: a drift of the box lands on every variant alike
        for name, fn in variants.items():
            groups[name].append(timed(fn, args.calls))
    out = {'root': args.root, 'package': sample.__file__, 'shape': f'{CLIPS} clips of {SHAPE}, default denoiser, bf16, {N_ITER} iterations, top-k {TOP_K}',
           'calls_per_group': args.calls, 'groups': args.groups, 'unit': 'ms per denoise iteration'}
    for name, g in groups.items():
        med = statistics.median(g)
        out[name] = {'median_ms': round(med, 4), 'min_ms': round(min(g), 4), 'max_ms': round(max(g), 4),
                     'spread': round((max(g) - min(g)) / med, 4)}
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
