#!/usr/bin/env python3
"""Timing driver of the nearest-code search at every width of csrc/vq_screen_widths.h (profiles/vq_screen_widths/README.md):
N = 65 536 Gaussian rows against Gaussian codebooks of C = 512, 1 024, 8 192 and (ragged) 1 000 codes, per shape

    screened   wmz_vq_argmin_screened                  the screened search, what ops.vq_argmin(x, cb) runs (its result is
                                                       compared with the full scan's first)
    exact      ops.vq_argmin(x, cb, exact_scan=True)   the full scan in the pinned order (wmz_vq_argmin): what a tree without
                                                       this width on the screened route runs for the shape
    parent     wmz_vq_argmin_screened of another build of the library (--parent-lib), at the shapes that build accepts
               (E = 64 with a multiple of 64 codes before the table): shows that shape has not become slower.  `screened` and
               `parent` go through the same bare ctypes call with preallocated outputs, so they differ in the library alone

in ONE process, in alternating groups (order reversed every other round), device events around each group, every shape warmed first.  Also the share of rows the
screening sent to the exact re-check (flag count in the workspace header).

    python tools/time_vq_screen.py [--groups 7] [--parent-lib libwmz_hip_parent.so] [--widths 16,32,...]
        one JSON line per shape: median / min / max us per call over the groups, (max - min) / median as the spread
"""
import argparse
import contextlib
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 65536
CODEBOOKS = (512, 1024, 8192, 1000)


def table_widths():
    import re
    with open(os.path.join(ROOT, 'world_modelz_amd', 'csrc', 'vq_screen_widths.h')) as f:
        return [int(w) for w in re.findall(r'X\((\d+)\)', next(ln for ln in f if ln.startswith('#define WMZ_VQ_SCREEN_WIDTHS')))]


def group_us(fn, reps):
    """us per call: device events around `reps` back-to-back calls"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / reps


@contextlib.contextmanager
def recorded_calls():
    """the C-ABI entry points a block of code reaches, in order"""
    from world_modelz_amd import _lib
    seen, orig = [], _lib.call

    def call(name, *a):
        seen.append(name)
        return orig(name, *a)
    _lib.call = call
    try:
        yield seen
    finally:
        _lib.call = orig


def flag_share(ws):
    torch.cuda.synchronize()
    return int(ws[4:8].view(torch.int32).item()) / N


def bare_call(path):
    """wmz_vq_argmin_screened of this tree's build (path None) or of another one, bound with this tree's signatures (they have
    not changed)"""
    from world_modelz_amd import _lib as L
    P = L.lib() if path is None else ctypes.CDLL(path)
    for name in ('wmz_vq_argmin_screened', 'wmz_vq_argmin_screened_workspace_bytes'):
        getattr(P, name).restype, getattr(P, name).argtypes = L.DECLARATIONS[name]

    def make(x, cb):
        C, E = cb.shape
        need = P.wmz_vq_argmin_screened_workspace_bytes(N, C, E)
        if need == 0:
            return None, None
        ws = torch.empty(need, dtype=torch.uint8, device=x.device)
        idx = torch.empty(N, dtype=torch.int64, device=x.device)

        def call():
            rc = P.wmz_vq_argmin_screened(L.ptr(x), E, L.ptr(cb), L.ptr(idx), None, N, C, E, L.ptr(ws), need, L.stream())
            assert rc == 0, rc
            return idx
        return call, ws
    return make


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--groups', type=int, default=7)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--widths', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('no GPU: a timing from anywhere else says nothing')
    from world_modelz_amd import ops
    widths = [int(w) for w in args.widths.split(',')] if args.widths else table_widths()
    this = bare_call(None)
    parent = bare_call(args.parent_lib) if args.parent_lib else None
    for E in widths:
        for C in CODEBOOKS:
            g = torch.Generator().manual_seed(0)
            x, cb = torch.randn(N, E, generator=g).cuda(), torch.randn(C, E, generator=g).cuda()
            call, ws = this(x, cb)
            variants = {'screened': call, 'exact': lambda: ops.vq_argmin(x, cb, exact_scan=True)}
            pws = None
            if parent is not None:
                pcall, pws = parent(x, cb)
                if pcall is not None:
                    variants['parent'] = pcall
            with recorded_calls() as seen:
                same = torch.equal(ops.vq_argmin(x, cb), variants['exact']())
            assert seen == ['wmz_vq_argmin_screened', 'wmz_vq_argmin'], seen       # (the shape does take the screened route)
            same = same and torch.equal(call(), variants['exact']())
            out = {'N': N, 'C': C, 'E': E, 'unit': 'us per call', 'groups': args.groups, 'equal_to_exact_scan': same,
                   'flagged_share': round(flag_share(ws), 5)}
            if 'parent' in variants:
                same_p = torch.equal(variants['parent'](), variants['exact']())
                out['parent_equal_to_exact_scan'], out['parent_flagged_share'] = same_p, round(flag_share(pws), 5)
            reps = {}
            for name, fn in variants.items():                 # warm, then enough calls per group for ~50 ms of device time
                group_us(fn, 3)
                reps[name] = max(3, min(200, int(5e4 / group_us(fn, 3))))
            groups = {name: [] for name in variants}
            for i in range(args.groups):                      # a, b, c, c, b, a, ...: a drift of the box, and what a variant inherits
                order = list(variants.items())                #  from the one in front of it, land on every variant alike
                for name, fn in (order if i % 2 == 0 else reversed(order)):
                    groups[name].append(group_us(fn, reps[name]))
            for name, t in groups.items():
                med = statistics.median(t)
                out[name] = {'median_us': round(med, 2), 'min_us': round(min(t), 2), 'max_us': round(max(t), 2),
                             'spread': round((max(t) - min(t)) / med, 4), 'calls_per_group': reps[name]}
            out['exact_over_screened'] = round(out['exact']['median_us'] / out['screened']['median_us'], 2)
            print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
