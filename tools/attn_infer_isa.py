"""Instruction counts of the row16 attention forward at the headline shape: the run-time kernel (csrc/attn_fwd_row16.hip,
attn_fwd_row16_kernel<128, Big, 9, aligned, no probe, no stamps, 16-wide>) beside the inference unit
(csrc/attn_fwd_row16_infer.hip, attn_fwd_row16_infer_kernel<EH, EW>), for the whole kernel and for one slab iteration.

    python tools/attn_infer_isa.py [--markdown]

Classes, by the prefixes s_, v_, ds_, global_ only (counting as tools/fused_infer_isa.py): MFMA (v_mfma*), vector (every other v_*),
scalar (every s_*, waits, barriers and branches included), conditional branches (s_cbranch*), waits (s_waitcnt*), VMEM (global_*),
LDS (ds_*).  One slab iteration: the basic blocks of the kernel's outermost loop that holds MFMAs -- the
slab loop of the run-time kernel; the key-plane loop of the unit, whose body is the two parity slabs written out, so its counts are
halved (rounded up)."""
import argparse
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fused_infer_isa import CSRC, compile_asm, count, hipcc  # noqa: E402,F401

RUNTIME = r'attn_fwd_row16_kernelILi128ENS_5ShapeILi16ELi16ELi8EEELi9ELb1ELb0ELb0ELb0EE'
INFER = r'attn_fwd_row16_infer_kernelILi(\d+)ELi(\d+)EE'
COLS = ('mfma', 'vector', 'scalar', 'cbranch', 'waits', 'vmem', 'lds', 'total')


def kernels(asm, pattern):
    """{extents or None: {'name', 'whole', 'loop', 'vgprs', 'scratch'}} of the kernels whose mangled name holds `pattern`."""
    meta = {m.group(1): m.group(2) for m in re.finditer(r'^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)\.end_amdhsa_kernel', asm, flags=re.S | re.M)}
    out = {}
    for m in re.finditer(r'^(_ZN\S*?' + pattern + r'\S*):[^\n]*\n(.*?)s_endpgm', asm, flags=re.S | re.M):
        lines = m.group(m.lastindex).split('\n')
        loop = outer_loop(lines)
        g = lambda k: int(re.search(r'\.' + k + r'\s+(\d+)', meta[m.group(1)]).group(1))          # noqa: E731
        key = tuple(int(x) for x in m.groups()[1:-1]) or None
        out[key] = {'name': m.group(1), 'whole': count(lines), 'loop': count(loop) if loop else None,
                    'vgprs': g('amdhsa_next_free_vgpr'), 'scratch': g('amdhsa_private_segment_fixed_size')}
    return out


def outer_loop(lines):
    """The lines of the outermost loop that holds MFMAs: from the first to the last basic block the compiler's comments place in it
    (its header, `in Loop: Header=`, `Parent Loop`: the latch may be laid out in front of the header).  None without such a loop."""
    labels = [(i, re.match(r'\.L(BB\d+_\d+):(.*)', l)) for i, l in enumerate(lines)]
    labels = [(i, m.group(1), m.group(2)) for i, m in labels if m]
    best = None
    for _, name, note in labels:
        if 'Loop Header: Depth=1' not in note:
            continue
        inside = [k for k, (i, n, c) in enumerate(labels) if n == name or re.search(r'(Header=|Parent Loop )' + name + r'\b', c)]
        end = labels[inside[-1] + 1][0] if inside[-1] + 1 < len(labels) else len(lines)
        span = lines[labels[inside[0]][0]:end]
        if count(span)['mfma'] and (best is None or count(span)['mfma'] > count(best)['mfma']):
            best = span
    return best


def per_slab(c, slabs):
    return {k: -(-v // slabs) for k, v in c.items()}


def listing():
    """[(label, {'whole', 'slab', 'vgprs', 'scratch', 'name'})]: the run-time headline instantiation, then the unit's kernels."""
    rt = kernels(compile_asm(os.path.join(CSRC, 'attn_fwd_row16.hip')), RUNTIME)
    inf = kernels(compile_asm(os.path.join(CSRC, 'attn_fwd_row16_infer.hip')), INFER)
    rows = [('runtime <128, Big, 9>', dict(k, slab=k['loop'])) for k in rt.values()]
    rows += [(f'infer <{e[0]}, {e[1]}>', dict(k, slab=per_slab(k['loop'], 2) if k['loop'] else None)) for e, k in sorted(inf.items(), reverse=True)]
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--markdown', action='store_true')
    a = ap.parse_args()
    if a.markdown:
        print('| kernel | span | ' + ' | '.join(COLS) + ' | VGPRs | scratch |')
        print('|---|---|' + '---|' * (len(COLS) + 2))
    for label, k in listing():
        for span in ('whole', 'slab'):
            c = k[span]
            if c is None:
                continue
            if a.markdown:
                print(f'| {label} | {span} | ' + ' | '.join(str(c[x]) for x in COLS) + f' | {k["vgprs"]} | {k["scratch"]} |')
            else:
                print(f'{label:24s} {span:5s} ' + ' '.join(f'{x} {c[x]:5d}' for x in COLS) + f'  vgprs {k["vgprs"]} scratch {k["scratch"]}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
