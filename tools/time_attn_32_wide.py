#!/usr/bin/env python3
"""Timing driver of the attention row kernel on 32-wide planes (profiles/attn_32_wide/README.md).  Eager launches timed with
events, medians over groups; one JSON line.

    python tools/time_attn_32_wide.py kernels [--iters 50] [--groups 5]
        attention forward on 32x32 planes, one head of 128, extents (3,3,3): 8 clips x 8 planes (config 4's 65 536 tokens) and
        1 x 8 planes -- bf16 row kernel against the general kernel (general=True) in the same process, forward and backward, and
        the half row kernel's forward.
    python tools/time_attn_32_wide.py model [--root DIR]
        the default denoiser on (8, 32, 32) clips, batch 8: forward in bf16 and in the precise mode, and a bf16 training step's
        forward + backward.  --root: the tree whose package is timed (a checkout of another commit, built), so that two commits
        alternate from one shell loop.
"""
import argparse
import json
import statistics
import sys

import torch


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
    for B in (8, 1):
        torch.manual_seed(1)
        q, k, v = (torch.randn(B, 8, 32, 32, dh, device='cuda').bfloat16() for _ in range(3))
        row, _, _ = ops.local3d_attention_fwd(q, k, v, ext, heads)
        gen, _, _ = ops.local3d_attention_fwd(q, k, v, ext, heads, general=True)
        out[f'fwd/B{B}/row_vs_general_rel'] = float((row.float() - gen.float()).norm() / gen.float().norm())
        # alternate the two inside the process as well: row, general, row, general
        for rep in range(2):
            out[f'fwd/B{B}/bf16_row/{rep}'] = groups(lambda: ops.local3d_attention_fwd(q, k, v, ext, heads), args.iters, args.groups)
            out[f'fwd/B{B}/bf16_general/{rep}'] = groups(lambda: ops.local3d_attention_fwd(q, k, v, ext, heads, general=True), args.iters, args.groups)
        do = torch.randn_like(q)
        o_r, lse_r, _ = ops.local3d_attention_fwd(q, k, v, ext, heads, need_lse=True)
        o_g, lse_g, _ = ops.local3d_attention_fwd(q, k, v, ext, heads, need_lse=True, general=True)
        dq_r, dkv_r = ops.local3d_attention_bwd(q, k, v, o_r, lse_r, do, ext, heads)
        dq_g, dkv_g = ops.local3d_attention_bwd(q, k, v, o_g, lse_g, do, ext, heads, general=True)
        out[f'bwd/B{B}/row_vs_general_rel'] = [float((a.float() - b.float()).norm() / b.float().norm()) for a, b in ((dq_r, dq_g), (dkv_r, dkv_g))]
        for rep in range(2):
            out[f'bwd/B{B}/bf16_row/{rep}'] = groups(lambda: ops.local3d_attention_bwd(q, k, v, o_r, lse_r, do, ext, heads), args.iters, args.groups)
            out[f'bwd/B{B}/bf16_general/{rep}'] = groups(lambda: ops.local3d_attention_bwd(q, k, v, o_g, lse_g, do, ext, heads, general=True), args.iters, args.groups)
        qh, kh, vh = q.half(), k.half(), v.half()
        out[f'fwd/B{B}/half_row'] = groups(lambda: ops.local3d_attention_fwd(qh, kh, vh, ext, heads), args.iters, args.groups)
    return out


def model(args):
    from world_modelz_amd import config
    from world_modelz_amd.main import VqVideoDiffusionModel
    torch.manual_seed(42)
    m = VqVideoDiffusionModel(data_shape=(8, 32, 32), dim=256, num_classes=1024, extents=(3, 3, 3), depth=4, dim_head=128,
                              mlp_dim=256, heads=1).cuda().eval()
    z = torch.randint(0, 1025, (8, 8, 32, 32), device='cuda')
    out = {}
    with torch.no_grad():
        for name, dt in (('bf16', torch.bfloat16), ('precise', torch.float16)):
            with config.compute_dtype(dt):
                out[f'model/{name}'] = groups(lambda: m(z), args.iters, args.groups)
    # one bf16 training step's forward + backward (no optimizer update), eager
    from world_modelz_amd import train
    target = torch.randint(0, 1024, (8, 32, 32), device='cuda')
    with config.compute_dtype(torch.bfloat16):
        tr = train.DenoiserTrainer(m.train(), 1024, lr=1e-4, warmup=0, max_steps=100, distributed=False)

        def step():
            tr.arena.zero_grad()
            tr.forward_backward(z, target)
        out['model/bf16_forward_backward'] = groups(step, max(args.iters // 5, 4), args.groups)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=('kernels', 'model'))
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--groups', type=int, default=5)
    ap.add_argument('--root', default='.')
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    assert torch.cuda.is_available(), 'timings need the GPU'
    out = {'what': args.what, 'root': args.root}
    out.update(kernels(args) if args.what == 'kernels' else model(args))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
