#!/usr/bin/env python3
"""Timing driver of the half guard (profiles/half_guard/README.md): the precise mode's config-4 forward step and the published
dim-384 x 20 forward, eager launches timed with events, under config.half_guard 'off' and (unless the library is older than the
guard: WMZ_LIB_PATH A / B runs) 'raise' on clean input, read-back included.

    python tools/time_half_guard.py [--iters 30] [--groups 5]          # one JSON line: medians over the groups, ms per forward
"""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, '.')
from world_modelz_amd import _lib, config                      # noqa: E402
from world_modelz_amd.main import VqVideoDiffusionModel         # noqa: E402


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--groups', type=int, default=5)
    args = ap.parse_args()
    config.set_compute_dtype(torch.float16)
    config.set_last_frame_cone(False)
    torch.manual_seed(42)
    cases = {
        'config4_step': (VqVideoDiffusionModel(data_shape=(32, 16, 16), dim=256, num_classes=1024, extents=(3, 3, 3), depth=4,
                                               dim_head=128, mlp_dim=256, heads=1), (8, 32, 16, 16), 1025),
        'dim384x20_forward': (VqVideoDiffusionModel(data_shape=(6, 8, 8), dim=384, num_classes=1024, extents=(2, 2, 2), depth=20,
                                                    dim_head=128, mlp_dim=512, heads=1), (64, 6, 8, 8), 1025),
    }
    has_guard = hasattr(_lib.lib(), 'wmz_half_guard_bind')
    out = {'has_guard': has_guard}
    for name, (m, shape, C) in cases.items():
        m = m.cuda().eval()
        z = torch.randint(0, C, shape, device='cuda')
        for policy in (('off', 'raise') if has_guard else ('off',)):
            with torch.no_grad(), config.half_guard(policy):
                timed(lambda: m(z), 5)
                g = [timed(lambda: m(z), args.iters) for _ in range(args.groups)]
            out[f'{name}/{policy}'] = {'median_ms': round(statistics.median(g), 5), 'min_ms': round(min(g), 5), 'max_ms': round(max(g), 5)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
