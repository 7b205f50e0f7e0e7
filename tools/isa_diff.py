"""Compare the device assembly of two builds, function by function.

    python tools/isa_diff.py DIR_A DIR_B

DIR_A / DIR_B hold one <unit>.s per csrc/*.hip unit, made with
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only [the unit's flags from build.py] csrc/<unit>.hip -o DIR/<unit>.s
Comments are stripped and local labels renumbered in order of appearance; a function is identical when its instruction text and its
.amdhsa_kernel block (registers, scratch, LDS) are.  Prints a markdown table (unit | functions | identical) and every difference;
exit status 1 when anything differs.
"""
import os
import re
import sys

LABEL = re.compile(r'\.L[A-Za-z_]*\d+(?:_\d+)?')


def functions(path):
    """{symbol: (instruction lines, .amdhsa_kernel lines)}"""
    body, meta = {}, {}
    cur = kern = None
    is_func = set()
    for raw in open(path):
        line = raw.split(';', 1)[0].strip()
        if not line:
            continue
        m = re.match(r'\.type\s+([^,]+),@function', line)
        if m:
            is_func.add(m.group(1))
            continue
        if line.startswith('.amdhsa_kernel '):
            kern = line.split()[1]
            meta[kern] = []
            continue
        if line == '.end_amdhsa_kernel':
            kern = None
            continue
        if kern is not None:
            meta[kern].append(line)
            continue
        if line.endswith(':') and line[:-1] in is_func:
            cur = line[:-1]
            body[cur] = []
            continue
        if line.startswith('.Lfunc_end'):
            cur = None
            continue
        if cur is not None and not line.startswith(('.p2align', '.loc', '.file', '.cfi')):
            body[cur].append(line)
    out = {}
    for name, lines in body.items():
        names = {}
        text = [LABEL.sub(lambda m: names.setdefault(m.group(0), '.L%d' % len(names)), l) for l in lines]
        out[name] = (text, meta.get(name, []))
    return out


def main(a, b):
    units = sorted(f for f in os.listdir(a) if f.endswith('.s'))
    bad = sorted(set(units) ^ set(f for f in os.listdir(b) if f.endswith('.s')))
    print('| unit | functions | identical |\n| --- | --- | --- |')
    notes = ['unit only on one side: %s' % u for u in bad]
    for u in units:
        if u in bad:
            continue
        fa, fb = functions(os.path.join(a, u)), functions(os.path.join(b, u))
        same = 0
        for name in sorted(set(fa) | set(fb)):
            if name not in fa or name not in fb:
                notes.append('%s: %s only in %s' % (u, name, a if name in fa else b))
            elif fa[name][0] != fb[name][0]:
                notes.append('%s: %s: instructions differ (%d / %d lines)' % (u, name, len(fa[name][0]), len(fb[name][0])))
            elif fa[name][1] != fb[name][1]:
                notes.append('%s: %s: kernel descriptor differs' % (u, name))
            else:
                same += 1
        print('| `%s` | %d | %d |' % (u[:-2] + '.hip', len(fa), same))
    print('\n'.join(notes))
    return 1 if notes else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1], sys.argv[2]))
