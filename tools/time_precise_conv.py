"""Same-process A/B of the conv encoder's routes: VqAutoEncoder.encode of 256 frames of 64 x 64 (bench.py's frame_encoder geometry:
E 64, C 1024, hidden 128, BatchNorm in training mode -- main.py:229-237 -- replayed through graph.GraphedEncoder as bench.py does)
on
    bf16            the speed mode (the route bench.py times),
    precise+conv    the precise mode with config.precise_conv on: the half conv kernels (conv_direct_f16.hip, conv_point_f16.hip),
    precise         the precise mode as it is by default: the fp32 conv route (implicit GEMM, exact-f32 MFMA).
The routes alternate over the repeats (after a warm-up), so drift hits all three alike; the spread over repeats is reported.  Per
route also: the decoder's ms on the same batch (eager VqAutoEncoder.decode of the route's tokens), and on 16 frames the latents'
relative error and the token agreement against the fp32 CPU oracle (oracle.autoencoder).

    python tools/time_precise_conv.py [--frames 256] [--repeats 5] [--iters 20] [--json PATH]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from world_modelz_amd import config                           # noqa: E402
from world_modelz_amd.graph import GraphedEncoder             # noqa: E402
from world_modelz_amd.train_vqae import VqAutoEncoder         # noqa: E402

ROUTES = {'bf16': (torch.bfloat16, False), 'precise+conv': (torch.float16, True), 'precise': (torch.float16, False)}


def mode(name):
    import contextlib
    dt, sw = ROUTES[name]
    st = contextlib.ExitStack()
    st.enter_context(config.compute_dtype(dt))
    st.enter_context(config.precise_conv(sw))
    st.enter_context(torch.no_grad())
    return st


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def oracle_agreement(ae, name, n=16):
    from oracle import autoencoder as oae
    from oracle import vq as ovq
    torch.manual_seed(12)
    frames = torch.rand(n, 3, 64, 64)
    sd = {k: v.detach().cpu().clone() for k, v in ae.state_dict().items()}
    lat_ref = oae.encoder_forward(sd, frames, training=True).permute(0, 2, 3, 1).reshape(-1, 64)
    tok_ref = ovq.encode(lat_ref, sd['vq.embedding']).reshape(-1)
    with mode(name):
        lat = ae._latents(frames.cuda())
        tok = ae.vq.encode(lat).reshape(-1).cpu()
    lat = lat.float().cpu().reshape(-1, 64)
    return float((lat - lat_ref).norm() / lat_ref.norm()), float((tok == tok_ref).float().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    torch.manual_seed(11)
    ae = VqAutoEncoder(embedding_dim=64, num_embeddings=1024, downscale_steps=2, hidden_planes=128).cuda()
    ae.train()
    frames = torch.rand(a.frames, 3, 64, 64, device='cuda')
    encs, toks = {}, {}
    for name in ROUTES:                 # (a captured encoder keeps the route it was captured with: one graph per route)
        with mode(name):
            encs[name] = GraphedEncoder(ae, frames)
            toks[name] = encs[name](frames).clone()
    enc_ms = {n: [] for n in ROUTES}
    dec_ms = {n: [] for n in ROUTES}
    for rep in range(a.repeats + 1):                             # repeat 0: warm-up, not recorded
        for name in ROUTES:
            with mode(name):
                e = timed(lambda: encs[name](frames), a.iters)
                d = timed(lambda: ae.decode(toks[name]), max(2, a.iters // 4))
            if rep:
                enc_ms[name].append(e)
                dec_ms[name].append(d)
    res = {}
    for name in ROUTES:
        e_lat, agree = oracle_agreement(ae, name)
        em, dm = enc_ms[name], dec_ms[name]
        res[name] = dict(encoder_ms=statistics.median(em), encoder_ms_min=min(em), encoder_ms_max=max(em),
                         decoder_ms=statistics.median(dm), decoder_ms_min=min(dm), decoder_ms_max=max(dm),
                         latents_rel_vs_fp32_oracle=e_lat, token_agreement_vs_fp32_oracle=agree)
        print(f'{name:13s} encoder {statistics.median(em):7.3f} ms [{min(em):.3f} .. {max(em):.3f}] per {a.frames} frames   '
              f'decoder {statistics.median(dm):7.3f} ms [{min(dm):.3f} .. {max(dm):.3f}]   latents rel {e_lat:.3e}   '
              f'token agreement {agree:.4f} (16 frames vs the fp32 oracle)')
    ratio = res['precise+conv']['encoder_ms'] / res['bf16']['encoder_ms']
    print(f'precise+conv / bf16 encoder: {ratio:.3f} (target <= 1.10); fp32 route / bf16: '
          f'{res["precise"]["encoder_ms"] / res["bf16"]["encoder_ms"]:.2f}')
    out = dict(frames=a.frames, repeats=a.repeats, iters=a.iters, routes=res, half_over_bf16_encoder=ratio,
               device=torch.cuda.get_device_name())
    print(json.dumps(out))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
