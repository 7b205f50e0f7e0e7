#!/usr/bin/env python3
"""Timing driver of the fused weight-stream packers (profiles/fused_pack_layout/README.md), for A / B runs of two libraries
(WMZ_LIB_PATH) or two trees: PackSet.refresh() of the config-4 stack (what training runs after every optimizer step) and a cold
_layer_pack of one boundary (an inference cache miss: _cast.clear() before every call), eager launches timed with events.

    python tools/time_fused_packs.py [--iters 200] [--groups 5]          # one JSON line: per group, microseconds per call
"""
import argparse
import json
import sys

import torch

sys.path.insert(0, '.')
from world_modelz_amd import _cast, fused                                              # noqa: E402
from world_modelz_amd.local_3d_attention import Local3dAttentionTransformer             # noqa: E402


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1000.0 * a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--groups', type=int, default=5)
    args = ap.parse_args()
    torch.manual_seed(42)
    tr = Local3dAttentionTransformer(data_shape=(32, 16, 16), dim=256, num_classes=1024, extents=(3, 3, 3), depth=4, mlp_dim=256,
                                     dim_head=128, heads=1).cuda()
    layers = list(tr.layers)
    ps = fused.PackSet(tr)

    def cold():
        _cast.clear()
        fused._layer_pack(layers[0], layers[1])

    out = {}
    for name, fn in (('pack_set_refresh_us', ps.refresh), ('cold_layer_pack_us', cold)):
        timed(fn, 20)
        out[name] = [round(timed(fn, args.iters), 3) for _ in range(args.groups)]
    print(json.dumps(out))


if __name__ == '__main__':
    main()
