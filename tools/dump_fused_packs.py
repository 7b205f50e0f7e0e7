#!/usr/bin/env python3
"""Every packed weight stream the fused and chain per-token kernels read, written to one file: the acceptance of a change to the
packers that must not move a byte (profiles/fused_pack_layout/README.md).  Run once on each tree (from that tree's root, seeded),
then compare the two files:

    python tools/dump_fused_packs.py OUT.pt                  # dump
    python tools/dump_fused_packs.py --compare A.pt B.pt     # torch.equal per tensor; exit status 1 on any difference

Dumped: a depth-3 default-width stack -- every stream and vector block from PackSet.refresh() and from the per-stream packers
(_layer_pack / _layer_pack_bwd) in bfloat16, the forward streams of the _f16 unit --, and the chain kernels' wpack / vec from
_chain_pack and ChainPackSet at dim 96 / 128 / 256."""
import sys

import torch

sys.path.insert(0, '.')


def perturbed(tr):
    with torch.no_grad():
        for p in tr.parameters():
            if p.dim() == 1:
                p.add_(0.3 * torch.randn_like(p))
    return tr


def dump(path):
    from world_modelz_amd import _cast, fused
    from world_modelz_amd.local_3d_attention import Local3dAttentionTransformer
    from world_modelz_amd.parallel import FlatArena
    out = {}
    torch.manual_seed(6)
    tr = perturbed(Local3dAttentionTransformer(data_shape=(2, 16, 16), dim=256, num_classes=32, extents=(1, 1, 1), depth=3,
                                               mlp_dim=256, dim_head=128, heads=1).cuda())
    layers = list(tr.layers)
    bounds = [(None, layers[0])] + [(layers[l], layers[l + 1] if l + 1 < 3 else None) for l in range(3)]

    def streams(tag, dts):
        for dt in dts:
            for i, (head, tail) in enumerate(bounds):
                for name, t in zip(('wpack', 'vec'), fused._layer_pack(head, tail, dt)):
                    out[f'{tag}/fwd{i}/{str(dt)[6:]}/{name}'] = t.clone().cpu()
        for l, (attn, ff) in enumerate(layers):
            for name, t in zip(('qkv', 'ff'), fused._layer_pack_bwd(attn, ff)):
                out[f'{tag}/bwd{l}/{name}'] = t.clone().cpu()
    _cast.clear()
    streams('per_stream', (torch.bfloat16, torch.float16))
    _cast.clear()
    fused.PackSet(tr).refresh()
    streams('pack_set', (torch.bfloat16,))                     # cache hits: the PackSet's buffers
    for dim, heads, mlp in ((96, 1, 256), (128, 2, 256), (256, 1, 512)):      # inner 128 (dim 128: two heads -- one as wide as dim has no to_out)
        _cast.clear()
        torch.manual_seed(dim)
        tr = perturbed(Local3dAttentionTransformer(data_shape=(2, 8, 8), dim=dim, num_classes=32, extents=(1, 1, 1), depth=2,
                                                   mlp_dim=mlp, dim_head=128 // heads, heads=heads).cuda())
        D, I, M, MC = fused.chain_widths(tr)
        layers = list(tr.layers)
        for i, (head, tail) in enumerate([(None, layers[0]), (layers[0], layers[1]), (layers[1], None)]):
            for dt in (torch.bfloat16, torch.float16):
                for name, t in zip(('wpack', 'vec'), fused._chain_pack(head, tail, D, I, M, MC, dt)):
                    out[f'chain{dim}/pack{i}/{str(dt)[6:]}/{name}'] = t.clone().cpu()
        cps = fused.ChainPackSet(tr, FlatArena(tr))
        out[f'chain{dim}/set/wpack'], out[f'chain{dim}/set/vec'] = cps.wpack.clone().cpu(), cps.vec.clone().cpu()
        out[f'chain{dim}/set/slices'] = torch.tensor([cps.slices[k] for k in sorted(cps.slices)])
    torch.cuda.synchronize()
    torch.save(out, path)
    print(f'{len(out)} tensors, {sum(t.numel() * t.element_size() for t in out.values())} bytes -> {path}')


def compare(a, b):
    A, B = torch.load(a), torch.load(b)
    bad = sorted(set(A) ^ set(B)) + [k for k in sorted(set(A) & set(B))
                                     if A[k].dtype != B[k].dtype or A[k].shape != B[k].shape
                                     or not torch.equal(A[k].view(torch.uint8), B[k].view(torch.uint8))]
    print(f'{len(set(A) & set(B)) - len([k for k in bad if k in A and k in B])} of {len(set(A) | set(B))} tensors identical byte for byte')
    for k in bad:
        print('DIFFERS:', k)
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(compare(*sys.argv[2:4]) if sys.argv[1] == '--compare' else dump(sys.argv[1]))
