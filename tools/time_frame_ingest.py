#!/usr/bin/env python3
"""Timing driver of the byte-frame ingest and egress (profiles/frame_bytes/README.md).  One process, device events for GPU work and
the host's wall clock for host work, the paths alternated in groups; one JSON line.

    python tools/time_frame_ingest.py [--iters 20] [--groups 5]

At 256 frames of 64 x 64 x 3 and at a main2.py-sized batch (10 clips x 16 frames), the flagship auto-encoder (64-wide codes, 1024
of them, hidden 128, two down-scalings; BatchNorm in training mode as main.py runs it), bf16 mode:
  parent        uint8 numpy batch -> transform_batch on the host (main2.py:51-56: permute, fp32, / 255) -> upload -> encode
  bytes/eager   pinned uint8 -> upload -> encode_frames
  bytes/graph   pinned uint8 -> GraphedEncoder (one asynchronous copy + one graph launch)
each as host_ms (host work in front of the upload), copy_ms (the upload, device events), device_ms (the encoder, device events)
and wall_ms (everything, to the synchronisation behind the tokens); then the ingest launch beside wmz_nchw_to_nhwc8 on the same
frames, and the egress launch beside the torch device ops it replaces.  At most 16 host threads."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
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


def transform_batch(batch):
    """minecraft/main2.py:51-56 on the host: uint8 [..., H, W, C] numpy -> fp32 NCHW in [0, 1]."""
    x = torch.from_numpy(batch).reshape((-1,) + batch.shape[-3:]).permute(0, 3, 1, 2)
    return x.to(torch.float32).div(255).contiguous()


def staged(prepare, upload, run, iters):
    """One path, `iters` times: medians of host_ms / copy_ms / device_ms / wall_ms."""
    rows = []
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = prepare()
        t1 = time.perf_counter()
        ev[0].record()
        d = upload(h)
        ev[1].record()
        run(d)
        ev[2].record()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        rows.append((1e3 * (t1 - t0), ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), 1e3 * (t2 - t0)))
    return {k: round(statistics.median(r[j] for r in rows), 4) for j, k in enumerate(('host_ms', 'copy_ms', 'device_ms', 'wall_ms'))}


def pipeline(ae, shape, args):
    from world_modelz_amd.graph import GraphedEncoder
    rng = np.random.default_rng(0)
    batch = rng.integers(0, 256, size=shape, dtype=np.uint8)
    pinned = torch.from_numpy(batch).pin_memory()
    enc = GraphedEncoder(ae, pinned.cuda())
    paths = {
        'parent': (lambda: transform_batch(batch), lambda h: h.cuda(), ae.encode),
        'bytes/eager': (lambda: pinned, lambda h: h.cuda(non_blocking=True), ae.encode_frames),
        # (the copy is the replay's own: it is inside device_ms)
        'bytes/graph': (lambda: pinned, lambda h: h, enc),
    }
    out = {}
    for name, path in paths.items():
        staged(*path, 3)
    for rep in range(args.groups):                                  # alternate: parent, eager, graph, parent, ...
        for name, path in paths.items():
            out[f'{name}/{rep}'] = staged(*path, args.iters)
    return out


def launches(shape, args):
    from world_modelz_amd import ops
    rng = np.random.default_rng(1)
    batch = rng.integers(0, 256, size=shape, dtype=np.uint8)
    xb = torch.from_numpy(batch).cuda()
    xf = transform_batch(batch).cuda()
    xb_cf = xb.reshape((-1,) + shape[-3:]).permute(0, 3, 1, 2).contiguous()
    out = {}
    for dt, tag in ((torch.bfloat16, 'bf16'), (torch.float32, 'fp32')):
        assert torch.equal(ops.frames_u8_to_nhwc8(xb, dt), ops.nchw_to_nhwc8(xf, dt))
        for rep in range(2):
            out[f'ingest/{tag}/bytes_hwc/{rep}'] = groups(lambda: ops.frames_u8_to_nhwc8(xb, dt), args.iters, args.groups)
            out[f'ingest/{tag}/bytes_chw/{rep}'] = groups(lambda: ops.frames_u8_to_nhwc8(xb_cf, dt, channels_last=False), args.iters, args.groups)
            out[f'ingest/{tag}/nchw_to_nhwc8/{rep}'] = groups(lambda: ops.nchw_to_nhwc8(xf, dt), args.iters, args.groups)
        raw = ops.nchw_to_nhwc8(xf, dt)

        def torch_law(channels_last):
            y = raw[..., :3].float().mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)
            return y if channels_last else y.permute(0, 3, 1, 2).contiguous()
        assert torch.equal(ops.nhwc8_to_frames_u8(raw, 3), torch_law(True))
        for rep in range(2):
            for cl, lay in ((True, 'hwc'), (False, 'chw')):
                out[f'egress/{tag}/bytes_{lay}/{rep}'] = groups(lambda: ops.nhwc8_to_frames_u8(raw, 3, cl), args.iters, args.groups)
                out[f'egress/{tag}/torch_{lay}/{rep}'] = groups(lambda: torch_law(cl), args.iters, args.groups)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--groups', type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'timings need the GPU'
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from world_modelz_amd import config
    from world_modelz_amd.train_vqae import VqAutoEncoder
    torch.manual_seed(0)
    ae = VqAutoEncoder(embedding_dim=64, num_embeddings=1024, downscale_steps=2, hidden_planes=128).cuda().train()
    out = {'host_threads': torch.get_num_threads()}
    with config.compute_dtype(torch.bfloat16), torch.no_grad():
        for tag, shape in (('256x64x64x3', (256, 64, 64, 3)), ('10x16x64x64x3', (10, 16, 64, 64, 3))):
            out.update({f'{tag}/{k}': v for k, v in pipeline(ae, shape, args).items()})
            out.update({f'{tag}/{k}': v for k, v in launches(shape, args).items()})
    print(json.dumps(out))


if __name__ == '__main__':
    main()
