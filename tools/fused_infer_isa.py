"""Instruction counts of the fused per-token forward kernels (csrc/layer_fused.hip), per kernel and for the feed-forward chunk
loop alone: the inference unit (layer_fused_infer_kernel) beside the run-time kernel (layer_fused_kernel) of the same build.

    python tools/fused_infer_isa.py [--source FILE.hip | --asm FILE.s] [--markdown]

Classes: MFMA (v_mfma*), vector (every other v_*), scalar (every s_*, waits, barriers and branches included), conditional
branches (s_cbranch*), waits (s_waitcnt*), VMEM (global_*), LDS (ds_*).  The chunk loop is the span from the header of the
kernel's one loop that holds MFMAs to its back edge."""
import argparse
import os
import re
import shutil
import subprocess
import sys

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'world_modelz_amd', 'csrc')
KINDS = {(True, True): 'head + tail', (True, False): 'head only', (False, True): 'embedding + tail'}


def hipcc():
    return shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)


def compile_asm(source):
    r = subprocess.run([hipcc(), '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', source, '-o', '-'],
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-4000:])
    return r.stdout


def count(lines):
    ops = [l.split()[0] for l in lines if re.match(r'\s+[a-z]', l)]
    n = lambda pred: sum(1 for o in ops if pred(o))          # noqa: E731
    return {'mfma': n(lambda o: o.startswith('v_mfma')),
            'vector': n(lambda o: o.startswith('v_') and not o.startswith('v_mfma')),
            'scalar': n(lambda o: o.startswith('s_')),
            'cbranch': n(lambda o: o.startswith('s_cbranch')),
            'waits': n(lambda o: o.startswith('s_waitcnt')),
            'vmem': n(lambda o: o.startswith('global_')),
            'lds': n(lambda o: o.startswith('ds_')),
            'total': len(ops)}


def chunk_loop(lines):
    """The lines of the loop that holds MFMAs: header label .. last branch back to it.  None if the kernel has no such loop."""
    best = None
    for i, l in enumerate(lines):
        m = re.match(r'(\.LBB\d+_\d+):.*Loop Header', l)
        if not m:
            continue
        back = [j for j in range(i + 1, len(lines)) if re.match(r'\s+s_c?branch\S*\s+' + re.escape(m.group(1)) + r'\s*$', lines[j])]
        if not back:
            continue
        span = lines[i:back[-1] + 1]
        if count(span)['mfma'] and (best is None or count(span)['mfma'] > count(best)['mfma']):
            best = span
    return best


def kernels(asm):
    """{(unit, head, tail): {'name', 'whole', 'loop', 'vgprs', 'scratch'}} with unit 'infer' or 'runtime'."""
    meta = {m.group(1): m.group(2) for m in re.finditer(r'^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)\.end_amdhsa_kernel', asm, flags=re.S | re.M)}
    out = {}
    for m in re.finditer(r'^(_ZN\S*?(layer_fused_infer_kernelILb(\d)ELb(\d)E|layer_fused_kernelILi256ELi128ELi256ELb(\d)ELb(\d)E)\S*):[^\n]*\n(.*?)s_endpgm',
                         asm, flags=re.S | re.M):
        infer = m.group(3) is not None
        head, tail = (m.group(3), m.group(4)) if infer else (m.group(5), m.group(6))
        lines = m.group(7).split('\n')
        loop = chunk_loop(lines)
        g = lambda k: int(re.search(r'\.' + k + r'\s+(\d+)', meta[m.group(1)]).group(1))          # noqa: E731
        out[('infer' if infer else 'runtime', head == '1', tail == '1')] = {
            'name': m.group(1), 'whole': count(lines), 'loop': count(loop) if loop else None,
            'vgprs': g('amdhsa_next_free_vgpr'), 'scratch': g('amdhsa_private_segment_fixed_size')}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--source', default=os.path.join(CSRC, 'layer_fused.hip'))
    ap.add_argument('--asm', help='count an assembly listing made earlier instead of compiling')
    ap.add_argument('--markdown', action='store_true')
    a = ap.parse_args()
    ks = kernels(open(a.asm).read() if a.asm else compile_asm(a.source))
    cols = ('mfma', 'vector', 'scalar', 'cbranch', 'waits', 'vmem', 'lds', 'total')
    if a.markdown:
        print('| kernel | span | ' + ' | '.join(cols) + ' | per MFMA | VGPRs | scratch |')
        print('|---|---|' + '---|' * (len(cols) + 3))
    for (unit, head, tail), k in sorted(ks.items(), key=lambda kv: (not kv[0][1], not kv[0][2], kv[0][0] != 'runtime')):
        for span in ('whole', 'loop'):
            c = k[span]
            if c is None:
                continue
            per = (c['total'] - c['mfma']) / c['mfma']
            label = f'{KINDS[(head, tail)]}, {unit}'
            if a.markdown:
                print(f'| {label} | {span} | ' + ' | '.join(str(c[x]) for x in cols) + f' | {per:.1f} | {k["vgprs"]} | {k["scratch"]} |')
            else:
                print(f'{label:32s} {span:5s} ' + ' '.join(f'{x} {c[x]:5d}' for x in cols) + f'  other/MFMA {per:5.1f}  vgprs {k["vgprs"]} scratch {k["scratch"]}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
