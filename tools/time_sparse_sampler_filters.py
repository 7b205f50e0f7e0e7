#!/usr/bin/env python3
"""Timing driver of config 5's sampler with its filters and a prompt (profiles/sparse_sampler_filters/README.md):
sparse_diffusion.sample_clips at the sampler's full size -- 8 clips of 64x16x16 latents, 8192 classes, 512-token contexts (4096
rows per draw), VqSparseDiffusionModel dim 512 / 4 x 128 / depth 8 / mlp 1024, bf16, the captured sub-step -- with

    default   default arguments: wmz_sparse_draw_context + wmz_categorical_scatter, the route every tree takes
    topk      sample_topk=100
    all       sample_topk=100, sample_topp=0.9, temperature=0.7
    prompt    the same with a prompt that gives the first half of the frames
    confidence        remask='confidence' (wmz_sparse_draw_context_scored + wmz_categorical_scatter_scored), no filter
    confidence+topk   the same with sample_topk=100

(all but the first in trees that take them), in ONE process, in alternating groups.  A call captures its own graph, so a group times
two calls that differ in the number of iterations only and reports the DIFFERENCE per sub-step: the capture, the warm-up sub-step
and the set-up are in both and cancel.

    python tools/time_sparse_sampler_filters.py [--groups 7] [--root DIR] [--variants default,topk,...]
        one JSON line: median / min / max ms per captured sub-step over the groups, (max - min) / median as the spread.
        --variants: only these (a process that holds one model is the like-for-like of a tree that has only `default`)
        --root: the tree to import world_modelz_amd from (compare two checkouts by running the tool once for each)
    python tools/time_sparse_sampler_filters.py --replay default|topk|all|prompt|confidence|confidence+topk [--iterations 3]
        nothing but one sample_clips call of that variant: the program to put behind `rocprofv3 --kernel-trace --stats --`
"""
import argparse
import inspect
import json
import statistics
import sys
import time

import torch

SHAPE, CLIPS, CODES, CONTEXT = (64, 16, 16), 8, 8192, 512
SUBSTEPS = SHAPE[0] * SHAPE[1] * SHAPE[2] // CONTEXT + 1            # per iteration
SHORT, LONG = 2, 6                                                   # iterations of the two calls of a group
FILTERS = {'default': {}, 'topk': dict(sample_topk=100), 'all': dict(sample_topk=100, sample_topp=0.9, temperature=0.7),
           'prompt': dict(sample_topk=100, sample_topp=0.9, temperature=0.7),
           'confidence': dict(remask='confidence'), 'confidence+topk': dict(remask='confidence', sample_topk=100)}


def build(name):
    from world_modelz_amd.sparse_diffusion import VqSparseDiffusionModel, sample_clips
    torch.manual_seed(42)
    m = VqSparseDiffusionModel(shape=SHAPE, dim=512, num_classes=CODES, depth=8, dim_head=128, mlp_dim=1024, heads=4).cuda().eval()
    kw = dict(FILTERS[name])
    if name == 'prompt':
        prompt = torch.full((CLIPS,) + SHAPE, CODES, dtype=torch.int64, device='cuda')
        prompt[:, :SHAPE[0] // 2] = torch.randint(0, CODES, (CLIPS, SHAPE[0] // 2) + SHAPE[1:], device='cuda')
        kw['prompt'] = prompt

    def call(iterations):
        return sample_clips(m, CLIPS, CODES, 'neighbors', CONTEXT, iterations, seed=1, **kw)
    return call


def timed(fn, iterations):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(iterations)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--groups', type=int, default=7)
    ap.add_argument('--root', default='.')
    ap.add_argument('--variants', default=','.join(FILTERS))
    ap.add_argument('--replay', default=None, choices=sorted(FILTERS))
    ap.add_argument('--iterations', type=int, default=3)
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    from world_modelz_amd import config, sparse_diffusion
    if not torch.cuda.is_available():
        raise SystemExit('no GPU: a timing from anywhere else says nothing')
    config.set_compute_dtype(torch.bfloat16)
    taken = inspect.signature(sparse_diffusion.sample_clips).parameters
    if args.replay:
        build(args.replay)(args.iterations)
        torch.cuda.synchronize()
        return
    variants = {name: build(name) for name in args.variants.split(',') if all(k in taken for k in FILTERS[name])}
    for fn in variants.values():                        # every variant warm (operand copies, allocator) before a clock starts
        timed(fn, SHORT)
    groups = {name: [] for name in variants}
    for _ in range(args.groups):                        # a, b, c, d, a, b, c, d, ...: a drift of the box lands on every variant alike
        for name, fn in variants.items():
            short, long = timed(fn, SHORT), timed(fn, LONG)
            groups[name].append((long - short) / ((LONG - SHORT) * SUBSTEPS) * 1e3)
    out = {'root': args.root, 'package': sparse_diffusion.__file__,
           'shape': f'{CLIPS} clips of {SHAPE}, {CODES} classes, {CONTEXT}-token contexts, dim 512 / depth 8, bf16, captured sub-step',
           'sub_steps_per_group': (LONG - SHORT) * SUBSTEPS, 'groups': args.groups, 'unit': 'ms per captured sub-step'}
    for name, g in groups.items():
        med = statistics.median(g)
        out[name] = {'median_ms': round(med, 4), 'min_ms': round(min(g), 4), 'max_ms': round(max(g), 4),
                     'spread': round((max(g) - min(g)) / med, 4)}
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
