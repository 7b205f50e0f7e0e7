"""Are the neutral sampler kernels of two builds the same code?

    hipcc -O3 --offload-arch=gfx950 -std=c++17 -S --cuda-device-only -o a.s <one checkout>/world_modelz_amd/csrc/loss.hip
    hipcc ...                                                        -o b.s <the other>/world_modelz_amd/csrc/loss.hip
    python tools/compare_sampler_isa.py a.s b.s

Compares the bodies of the four sample_tokens_kernel<NV> functions (the kernels wmz_sample_tokens_dev launches) instruction by
instruction (and their kernel descriptors field by field), with comments stripped, the kernel's own symbol masked and the local labels renumbered in order of appearance (their numbers depend on what else the
translation unit holds).  With --filtered also the sixteen sample_tokens_kernel<NV, TEMP, TOPP, SampleExtras> and the wide kernel (what
wmz_sample_tokens_filtered_dev launches; the wide kernel is the empty instantiation of a template since the scored form exists).
Exit status 0 when all compared kernels are equal."""
import re
import sys

# (mangled: <NV> alone before the filters were template flags, <NV, false, false, {}> -- no extras -- since)
NAMES = ['sample_tokens_kernelILi%dE(?:Lb0ELb0EJE)?EE' % nv for nv in (4, 8, 16, 32)]
FILTERED = ['sample_tokens_kernelILi%dELb%dELb%dEJNS_12SampleExtrasEEEE' % (nv, t, p) for nv in (4, 8, 16, 32) for t in (0, 1) for p in (0, 1)]
WIDE = 'sample_tokens_wide_kernel(?:IJEEE|E)'


def body(text, name):
    m = re.search(r'^(_ZN\w*?%sv?P\w*):\s*(?:;.*)?$' % name, text, flags=re.M)
    if m is None:
        raise SystemExit(f'{name}: not found')
    end = text.index('.Lfunc_end', m.end())
    lines, labels = [], {}
    for line in text[m.end():end].splitlines():
        line = line.split(';')[0].strip()
        if line:
            lines.append(line)
    code = '\n'.join(lines).replace(m.group(1), '<this kernel>')        # (its own symbol: the kernel descriptor names it)
    for lab in re.findall(r'\.LBB\d+_\d+', code):
        labels.setdefault(lab, f'.L{len(labels)}')
    return re.sub(r'\.LBB\d+_\d+', lambda k: labels[k.group(0)], code).splitlines()


def main(a, b, filtered=False):
    ta, tb = open(a).read(), open(b).read()
    same = True
    for name in NAMES + (FILTERED + [WIDE] if filtered else []):
        la, lb = body(ta, name), body(tb, name)
        eq = la == lb
        same &= eq
        print(f'{name}: {len(la)} / {len(lb)} lines, {"identical" if eq else "DIFFERENT"}')
        if not eq:
            for i, (x, y) in enumerate(zip(la, lb)):
                if x != y:
                    print(f'  first difference at line {i}: `{x}` / `{y}`')
                    break
    return 0 if same else 1


if __name__ == '__main__':
    paths = [a for a in sys.argv[1:] if a != '--filtered']
    sys.exit(main(*paths[:2], filtered='--filtered' in sys.argv[1:]))
