#!/usr/bin/env python3
"""Timing driver of gradient accumulation inside the captured training step (profiles/graph_accumulation/README.md): one
optimizer step over K = 2 micro-batches, three ways in ONE process, in alternating groups --

    graph_k2   DenoiserTrainer(accumulation_steps=2).enable_graph([z0, z1]): one hipGraph, one read-back
    eager_k2   the same trainer without a graph: the eager accumulation step (all a tree without the capture can run)
    graph_k1x2 two replays of the captured single-micro-batch step (two optimizer tails, two re-packs, two read-backs)

at config 4's per-GPU shape (2 x 8 clips of 32x16x16, default model) and at the reference's geometry (64 clips of (6,8,8) split
in two, dim 384 / 20 layers); bf16, noise levels from the trainer's own sampler, host clock around steps that end in a read-back.

    python tools/time_graph_accumulation.py [--iters 30] [--groups 7] [--case config4|refgeo|both] [--root DIR]
        one JSON line per case: median / min / max ms per optimizer step over the groups, (max - min) / median as the spread.
        --root: the tree to import world_modelz_amd from (a checkout without the capture reports eager_k2 and graph_k1x2 only)
    python tools/time_graph_accumulation.py --replay graph_k2|graph_k1x2 [--case config4] [--steps 8]
        nothing but that many optimizer steps of one variant: the program to put behind `rocprofv3 --kernel-trace --stats --`
        (tools/trace_step.py reads a step out of the trace; its marker kernel, AdamW, runs once per replay)
"""
import argparse
import json
import statistics
import sys
import time

import torch

CASES = {
    # name: (data_shape, dim, mlp, depth, extents, codebook, clips per micro-batch)
    'config4': ((32, 16, 16), 256, 256, 4, (3, 3, 3), 1024, 8),
    'refgeo': ((6, 8, 8), 384, 512, 20, (3, 1, 1), 512, 32),
}
K = 2


def build(case, variants):
    from world_modelz_amd.main import VqVideoDiffusionModel
    from world_modelz_amd.train import DenoiserTrainer
    shape, dim, mlp, depth, ext, C, B = CASES[case]
    g = torch.Generator().manual_seed(42)
    micro = [torch.randint(0, C, (B,) + shape, generator=g).cuda() for _ in range(K)]

    def trainer(k):
        torch.manual_seed(42)
        m = VqVideoDiffusionModel(data_shape=shape, dim=dim, num_classes=C, extents=ext, depth=depth, dim_head=128, mlp_dim=mlp,
                                  heads=1).cuda()
        return DenoiserTrainer(m, C, lr=1e-4, warmup=500, max_steps=200000, distributed=False, accumulation_steps=k)
    steps = {}
    if 'graph_k2' in variants:
        tk = trainer(K)
        try:
            tk.enable_graph(micro)
            steps['graph_k2'] = lambda: tk.train_step(micro)
        except AssertionError as e:                  # a tree whose captured step is one micro-batch per optimizer step
            print(f'# graph_k2 not available here: {e}', file=sys.stderr)
    if 'eager_k2' in variants:
        te = trainer(K)
        steps['eager_k2'] = lambda: te.train_step(micro)
    if 'graph_k1x2' in variants:
        t1 = trainer(1)
        t1.enable_graph(micro[0])

        def two():
            for z in micro:
                t1.train_step(z)
        steps['graph_k1x2'] = two
    return steps


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()                                         # (every variant's step ends in its read-back: the device is idle here)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--groups', type=int, default=7)
    ap.add_argument('--case', default='both', choices=['config4', 'refgeo', 'both'])
    ap.add_argument('--root', default='.')
    ap.add_argument('--replay', default=None, choices=['graph_k2', 'graph_k1x2'])
    ap.add_argument('--steps', type=int, default=8)
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    from world_modelz_amd import config
    if not torch.cuda.is_available():
        raise SystemExit('no GPU: a timing from anywhere else says nothing')
    config.set_compute_dtype(torch.bfloat16)
    cases = ['config4', 'refgeo'] if args.case == 'both' else [args.case]
    if args.replay:
        step = build(cases[0], [args.replay])[args.replay]
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        return
    for case in cases:
        steps = build(case, ['graph_k2', 'eager_k2', 'graph_k1x2'])
        for fn in steps.values():
            timed(fn, 5)
        groups = {name: [] for name in steps}
        for _ in range(args.groups):                 # a, b, c, a, b, c, ...: a drift of the box lands on every variant alike
            for name, fn in steps.items():
                groups[name].append(timed(fn, args.iters))
        shape, dim, mlp, depth, ext, C, B = CASES[case]
        out = {'case': case, 'shape': f'{K} micro-batches x {B} clips of {shape}, dim {dim} / mlp {mlp} / depth {depth} / extents {ext}, '
                                      f'codebook {C}, bf16', 'iters_per_group': args.iters, 'groups': args.groups,
               'unit': 'ms per optimizer step (2 micro-batches)'}
        for name, g in groups.items():
            med = statistics.median(g)
            out[name] = {'median_ms': round(med, 4), 'min_ms': round(min(g), 4), 'max_ms': round(max(g), 4),
                         'spread': round((max(g) - min(g)) / med, 4)}
        print(json.dumps(out), flush=True)
        del steps
        import gc
        gc.collect()
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
