#!/usr/bin/env python3
"""Timing driver of the sampler loop with position-blind and confidence-ordered re-masking (profiles/confidence_remask/README.md):
sample_frames on 8 clips of 32x16x16 latents (2048 rows per draw, 256 per clip: the bench's sampler geometry), the default
denoiser, bf16, 30 denoise iterations, top-k 100, at 1024 and at 8192 codes, with

    random       remask='random': the default arguments, one launch per step (also what a tree without the option runs)
    confidence   remask='confidence': the scored draw + the per-clip selection, two launches per step
    noisy        the same with remask_noise=0.5 (the Gumbel term evaluated)

in ONE process, in alternating groups, host clock around calls that end in a synchronise.

    python tools/time_confidence_remask.py [--calls 10] [--groups 7]
        one JSON line: median / min / max ms per denoise iteration over the groups, (max - min) / median as the spread
    python tools/time_confidence_remask.py --replay 1024|8192 [--remask confidence] [--calls 2]
        nothing but that many sample_frames calls: the program to put behind `rocprofv3 --kernel-trace --stats --`
    python tools/time_confidence_remask.py --select ROWS [--clips 8] [--launches 200]
        nothing but wmz_remask_lowest_dev on random scores, ROWS rows per clip (256: the one-wave form's last plane, 257: the
        workgroup form's first, 4096: the limit), alpha walking through 30 values: likewise for a kernel trace
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPE, CLIPS, N_ITER, TOP_K = (32, 16, 16), 8, 30, 100
MODES = {'random': {}, 'confidence': dict(remask='confidence'), 'noisy': dict(remask='confidence', remask_noise=0.5)}


def build(C):
    from world_modelz_amd.main import VqVideoDiffusionModel
    torch.manual_seed(42)
    m = VqVideoDiffusionModel(data_shape=SHAPE, dim=256, num_classes=C, extents=(3, 3, 3), depth=4, dim_head=128, mlp_dim=256,
                              heads=1).cuda().eval()
    return m, torch.randint(0, C, (CLIPS,) + SHAPE, device='cuda')


def caller(C, **kw):
    from world_modelz_amd.sample import sample_frames
    m, z = build(C)                                     # (a model keeps two captured sampler steps: one model per variant)

    def call():
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
    ap.add_argument('--replay', type=int, default=None)
    ap.add_argument('--remask', default='random')
    ap.add_argument('--select', type=int, default=None)
    ap.add_argument('--clips', type=int, default=CLIPS)
    ap.add_argument('--launches', type=int, default=200)
    args = ap.parse_args()
    from world_modelz_amd import config, ops, sample
    if not torch.cuda.is_available():
        raise SystemExit('no GPU: a timing from anywhere else says nothing')
    config.set_compute_dtype(torch.bfloat16)
    if args.select:
        n, clips = args.select, args.clips
        scores = torch.randn(clips * n, device='cuda')
        alphas = torch.tensor([(i + 1) / 30 for i in range(30)], device='cuda')
        z = torch.zeros(clips, 1, n, dtype=torch.int64, device='cuda')
        ctr = torch.zeros(1, dtype=torch.int64, device='cuda')
        for _ in range(args.launches):
            ops.remask_lowest(scores, alphas, 1, z[:, -1], ctr)
            ctr += 1
        torch.cuda.synchronize()
        return
    if args.replay:
        fn = caller(args.replay, **MODES[args.remask])
        for _ in range(args.calls):
            fn()
        torch.cuda.synchronize()
        return
    variants = {f'c{C}_{mode}': caller(C, **kw) for C in (1024, 8192) for mode, kw in MODES.items()}
    for fn in variants.values():                        # every variant warm (captures, operand copies, allocator) before a clock starts
        timed(fn, 2)
    groups = {name: [] for name in variants}
    for _ in range(args.groups):                        # a, b, c, a, b, c, ...: a drift of the box lands on every variant alike
        for name, fn in variants.items():
            groups[name].append(timed(fn, args.calls))
    out = {'package': sample.__file__, 'shape': f'{CLIPS} clips of {SHAPE}, default denoiser, bf16, {N_ITER} iterations, top-k {TOP_K}',
           'calls_per_group': args.calls, 'groups': args.groups, 'unit': 'ms per denoise iteration'}
    for name, g in groups.items():
        med = statistics.median(g)
        out[name] = {'median_ms': round(med, 4), 'min_ms': round(min(g), 4), 'max_ms': round(max(g), 4),
                     'spread': round((max(g) - min(g)) / med, 4)}
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
