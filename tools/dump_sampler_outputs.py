#!/usr/bin/env python3
"""Every output of the sampler's entry points on seeded inputs, for comparing two trees bit by bit (profiles/sampler_forms/README.md).

    python tools/dump_sampler_outputs.py [--root DIR] OUT.npz
        --root: the tree to import world_modelz_amd from (run the tool once for each checkout)
    python tools/dump_sampler_outputs.py --compare A.npz B.npz
        every array of A against the one of the same name in B, floats as their bits; exits 1 on any difference

Calls, through _lib.call, wmz_sample_tokens_dev / _filtered_dev / _scored_dev, wmz_remask_lowest_dev, wmz_categorical_scatter /
_filtered / _scored (and the two limits) on R = 333 rows in 3 clips at C in {37, 300, 700, 2000, 2049, 8192} -- every NV of the
register kernel, the narrowest wide row, config 5's width; ld = C rounded up to 4, and once ld > C -- with the filters neutral,
top_k = 10, top_p = 0.9, temperature 0.7 and all three; each with the in-kernel generator and with given uniforms (then also the
kept_floor probe), with and without last_mask / known; the scored forms with noise 0 and 0.5.  Then the selection at 100 and 700
rows per clip and wmz_sparse_draw_context / _known / _scored at S, HW, n = 4, 16, 24 with and without a device counter.
A tool and a recorded result, not a fixture: a later ROCm may change __expf.
"""
import argparse
import sys

import numpy as np
import torch

R, CLIPS = 333, 3
ROWS = R // CLIPS
WIDTHS = [(37, 40), (300, 300), (300, 312), (700, 700), (2000, 2000), (2049, 2052), (8192, 8192)]       # (C, ld)
SETTINGS = {'neutral': (-1, 1.0, 1.0), 'topk': (10, 1.0, 1.0), 'topp': (-1, 0.9, 1.0), 'temp': (-1, 1.0, 0.7), 'all': (10, 0.9, 0.7)}
SEED, G = 1234, 256                                       # Philox seed; positions per clip of the sparse destination


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in a.files:
        if k in b.files:
            x, y = a[k], b[k]
            if x.dtype.kind == 'f':
                x, y = x.view(np.uint32), y.view(np.uint32)
            if not np.array_equal(x, y):
                bad.append(k)
    print(f'{len(a.files)} arrays in {a_path}, {len(b.files)} in {b_path}: ' + ('all equal bit for bit' if not bad else f'{len(bad)} DIFFER: {bad[:20]}'))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default='.')
    ap.add_argument('--compare', default=None)
    ap.add_argument('out')
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(args.compare, args.out))
    sys.path.insert(0, args.root)
    from world_modelz_amd import _lib as L
    if not torch.cuda.is_available():
        raise SystemExit('no GPU')
    g = torch.Generator().manual_seed(7)
    dev = lambda t: t.cuda()
    print('package', L.__file__)
    out = {'max_classes': np.array(L.lib().wmz_sample_tokens_max_classes()), 'remask_max_rows': np.array(L.lib().wmz_remask_lowest_max_rows())}

    def keep(name, **tensors):
        for k, t in tensors.items():
            if t is not None:
                out[f'{name}/{k}'] = t.cpu().numpy()

    alphas = dev(torch.linspace(0.1, 0.9, 8))
    counter = dev(torch.tensor([5], dtype=torch.int64))                      # alpha = alphas[5], Philox stream id 5
    ucounter = dev(torch.tensor([7], dtype=torch.int64))                     # (the sparse entry points read it as unsigned)
    u2 = dev(torch.rand(R, 2, generator=g))
    u1 = dev(torch.rand(R, generator=g))
    mask0 = dev((torch.rand(R, generator=g) < 0.6).to(torch.uint8))
    indices = dev(torch.stack([torch.randperm(G, generator=g)[:ROWS] for _ in range(CLIPS)]).reshape(-1))
    known = dev((torch.rand(CLIPS, G, generator=g) < 0.3).to(torch.uint8))
    s = L.stream
    for C, ld in WIDTHS:
        store = dev(torch.randn(R, ld, generator=g) * 3.0)
        logits = store[:, :C]
        head = (L.ptr(logits), ld, R, C)
        for sname, (top_k, top_p, temp) in SETTINGS.items():
            filt = (top_k, float(top_p), 1.0 / temp)
            for given in (False, True):
                for second in (False, True):                                 # last_mask (dense) / known (sparse); noise 0.5 (scored dense)
                    tag = f'C{C}_ld{ld}/{sname}/{"given" if given else "philox"}/{int(second)}'
                    frame = dev(torch.full((CLIPS, ROWS), -1, dtype=torch.int64))
                    den = dev(torch.full((R,), -1, dtype=torch.int64))
                    lm = mask0.clone() if second else None
                    floor = dev(torch.full((R,), -5.0)) if given else None
                    step_out = (L.ptr(frame), ROWS, frame.stride(0), L.ptr(den))
                    if not given and top_p == 1.0 and temp == 1.0 and C <= 2048:
                        L.call('wmz_sample_tokens_dev', *head, top_k, L.ptr(alphas), 8, C, *step_out, L.ptr(lm), SEED, L.ptr(counter), s())
                        keep(tag + '/dev', frame=frame, denoised=den, last_mask=lm)
                        frame.fill_(-1), den.fill_(-1)
                        lm = mask0.clone() if second else None
                    L.call('wmz_sample_tokens_filtered_dev', *head, *filt, L.ptr(alphas), 8, C, *step_out, L.ptr(lm),
                           L.ptr(u2 if given else None), L.ptr(floor), SEED, L.ptr(counter), s())
                    keep(tag + '/filtered', frame=frame, denoised=den, last_mask=lm, kept_floor=floor)
                    frame.fill_(-1), den.fill_(-1)
                    scores = dev(torch.full((R,), -7.0))
                    floor = dev(torch.full((R,), -5.0)) if given else None
                    L.call('wmz_sample_tokens_scored_dev', *head, *filt, L.ptr(alphas), 8, *step_out, L.ptr(scores), 0.5 if second else 0.0,
                           L.ptr(u2 if given else None), L.ptr(floor), SEED, L.ptr(counter), s())
                    keep(tag + '/scored', frame=frame, denoised=den, scores=scores, kept_floor=floor)
                    # the sparse destination: counter given where `known` is
                    sp_tail = (SEED, 3 << 40, L.ptr(ucounter if second else None), s())
                    for form in ('filtered', 'scored'):
                        z = dev(torch.full((CLIPS, G), -1, dtype=torch.int64))
                        samples = dev(torch.full((R,), -1, dtype=torch.int64))
                        floor = dev(torch.full((R,), -5.0)) if given else None
                        zs = dev(torch.full((CLIPS, G), -7.0)) if form == 'scored' else None
                        more = (L.ptr(zs), G) if form == 'scored' else ()
                        L.call('wmz_categorical_scatter_' + form, *head, *filt, L.ptr(indices), L.ptr(z), G, ROWS, L.ptr(samples),
                               L.ptr(known if second else None), G, L.ptr(u1 if given else None), L.ptr(floor), *sp_tail, *more)
                        keep(tag + '/scatter_' + form, z=z, samples=samples, kept_floor=floor, scores=zs)
        for with_counter in (False, True):
            z = dev(torch.full((CLIPS, G), -1, dtype=torch.int64))
            samples = dev(torch.full((R,), -1, dtype=torch.int64))
            L.call('wmz_categorical_scatter', *head, L.ptr(indices), L.ptr(z), G, ROWS, L.ptr(samples), SEED, 3 << 40,
                   L.ptr(ucounter if with_counter else None), s())
            keep(f'C{C}_ld{ld}/scatter/{int(with_counter)}', z=z, samples=samples)
    for rows in (100, 700):                                                  # the one-wave and the four-wave selection
        sc = dev(torch.randn(CLIPS * rows, generator=g))
        sc[::17] = sc[3]                                                     # ties: ranked in row order
        cand = dev((torch.rand(CLIPS * rows, generator=g) < 0.6).to(torch.uint8))
        for with_mask in (False, True):
            frame = dev(torch.arange(CLIPS * rows, dtype=torch.int64).reshape(CLIPS, rows))
            lm = cand.clone() if with_mask else None
            L.call('wmz_remask_lowest_dev', L.ptr(sc), CLIPS * rows, rows, L.ptr(alphas), 8, -3, L.ptr(frame), frame.stride(0), L.ptr(lm),
                   L.ptr(counter), s())
            keep(f'remask/{rows}/{int(with_mask)}', frame=frame, last_mask=lm)
    S, HW, n, C, B = 4, 16, 24, 512, 3                                       # the context draw
    z = dev(torch.randint(0, C, (B, S * HW), generator=g))
    r = dev(torch.tensor([0.2, 0.55, 0.9]))
    kn = dev((torch.rand(B, S * HW, generator=g) < 0.3).to(torch.uint8))
    zsc = dev(torch.randn(B, S * HW, generator=g))
    for with_counter in (False, True):
        for form in ('plain', 'known', 'scored', 'scored_noise'):
            idx, tok, tgt = (dev(torch.full((B, n), -1, dtype=torch.int64)) for _ in range(3))
            common = (L.ptr(z), S * HW, L.ptr(r), None, L.ptr(idx), L.ptr(tok), L.ptr(tgt), B, S, HW, n, C,
                      0.1 if form in ('plain', 'known') else 0.0, SEED, 3 << 40, L.ptr(ucounter if with_counter else None), s())
            slot = None
            if form == 'plain':
                L.call('wmz_sparse_draw_context', *common)
            elif form == 'known':
                L.call('wmz_sparse_draw_context_known', *common, L.ptr(kn), S * HW)
            else:
                slot = dev(torch.full((B, n), -7.0))
                L.call('wmz_sparse_draw_context_scored', *common, L.ptr(kn), S * HW, L.ptr(zsc), S * HW, 0.5 if form == 'scored_noise' else 0.0,
                       L.ptr(slot))
            keep(f'context/{form}/{int(with_counter)}', indices=idx, tokens=tok, target=tgt, slot_scores=slot)
    torch.cuda.synchronize()
    np.savez_compressed(args.out, **out)
    print(f'{len(out)} arrays -> {args.out}')


if __name__ == '__main__':
    main()
