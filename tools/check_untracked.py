"""Build-time check for csrc/layer_fused.hip: the residual rows are fetched by inline-asm loads hipcc does not track, so
nothing may read or overwrite their destination registers between the load and the counted s_waitcnt that retires them.
Compiles the kernel to ISA and scans the span.   python tools/check_untracked.py
Second part: the inline-asm written-through (sc1) stores of the inference units (csrc/mem_policy.h; layer_fused.hip and
attn_fwd_row16_infer.hip) -- their own wait states behind the data registers, no scalar base fresh from the VALU, none outside the units."""
import re, subprocess, sys, os
src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'world_modelz_amd', 'csrc', 'layer_fused.hip')
asm = subprocess.run(['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', src, '-o', '-'],
                     capture_output=True, text=True).stdout
bad_total = 0
# (layer_fused_kernel: every caller's kernel; layer_fused_infer_kernel: the inference unit, whose loads take a scalar base)
for name, body in re.findall(r'^(_ZN\S*layer_fused(?:_infer)?_kernel\S*):\s*;.*?\n(.*?)s_endpgm', asm, flags=re.S | re.M):
    lines = body.split('\n')
    loads = []
    for i, l in enumerate(lines):
        m = re.match(r'\s*global_load_dwordx4 v\[(\d+):(\d+)\], (?:v\[\d+:\d+\], off|v\d+, s\[\d+:\d+\] offset:(?:0x[0-9a-f]+|\d+))\s*$', l)
        if m and i and '#ASMSTART' in lines[i - 1]:
            loads.append((i, int(m.group(1)), int(m.group(2))))
    if not loads:
        continue
    waits = [i for i, l in enumerate(lines) if re.search(r's_waitcnt vmcnt\((6|4)\)', l) and '#ASMSTART' in lines[i - 1] and i > loads[-1][0]]
    end = waits[0]
    bad = []
    for i in range(loads[0][0], end):
        l = lines[i]
        if not re.match(r'\s+[a-z]', l) or ('global_load_dwordx4' in l and '#ASMSTART' in lines[i - 1]):
            continue
        for m in re.finditer(r'v\[(\d+):(\d+)\]|v(\d+)', l):
            rr = [int(m.group(3))] if m.group(3) else range(int(m.group(1)), int(m.group(2)) + 1)
            for r in rr:
                for li, a, b in loads:
                    if a <= r <= b and i > li:
                        bad.append((i, l.strip()))
    print(f'{name[:70]}: {len(loads)} untracked loads, wait at line {end}, touches in between: {len(bad)}')
    bad_total += len(bad)

# The written-through hand-off stores of the inference units (csrc/mem_policy.h): inline-asm `global_store_dwordx4 ... sc1`, which
# hipcc does not look into.  Per store: (a) its string carries its own `s_nop 1` -- two wait states before the next instruction may
# overwrite the data registers; (b) in the scalar-base form, nothing within the five wait states in front of it is a vector instruction
# that writes a scalar register overlapping the base pair (v_readfirstlane, v_cmp, a carry-out: an SGPR written by the VALU needs
# five wait states before VMEM reads it), and no label stands in that window;
# (c) it stands in an inference unit -- no run-time kernel holds one.
asm2 = subprocess.run(['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only',
                       os.path.join(os.path.dirname(src), 'attn_fwd_row16_infer.hip'), '-o', '-'], capture_output=True, text=True).stdout
for name, body in re.findall(r'^(_Z\w+):[^\n]*\n(.*?)s_endpgm', asm + asm2, flags=re.S | re.M):
    lines = [l.strip() for l in body.split('\n')]
    stores = [i for i, l in enumerate(lines) if re.match(r'global_store_dwordx4 .*\bsc1\b', l)]
    if not stores:
        continue
    unpadded = hazard = 0
    for i in stores:
        unpadded += not (lines[i - 1].startswith(';;#ASMSTART') and lines[i + 1].startswith('s_nop 1'))
        m = re.search(r's\[(\d+):(\d+)\]', lines[i])
        if not m:
            continue                                       # (64-bit per-lane address: no scalar base)
        lo, hi = int(m.group(1)), int(m.group(2))
        # walk back over five wait states (an instruction is one, s_nop N is N + 1).  A label inside the window means another path
        # may join there with anything in front of it: counted as a hazard, not guessed at.  A vector instruction may name a scalar
        # destination as its first or second operand (v_readfirstlane / v_readlane / v_cmp; the carry-out of v_add_co): any scalar
        # register or tuple there that overlaps the base counts.
        states, j = 0, i - 1
        while states < 5 and j >= 0:
            l = lines[j]
            j -= 1
            if re.match(r'\.?[A-Za-z_][\w.$]*:', l):
                hazard += 1
                break
            if not re.match(r'[a-z]', l):
                continue
            ops = l.replace(',', ' ').split()
            nop = re.match(r's_nop (\d+)', l)
            states += int(nop.group(1)) + 1 if nop else 1
            if ops[0].startswith('v_'):
                for o in ops[1:3]:
                    r = re.fullmatch(r's\[(\d+):(\d+)\]|s(\d+)', o)
                    if r:
                        a, b = (int(r.group(3)),) * 2 if r.group(3) else (int(r.group(1)), int(r.group(2)))
                        hazard += a <= hi and b >= lo
    outside = 'infer_kernel' not in name
    print(f'{name[:70]}: {len(stores)} written-through stores, unpadded: {unpadded}, base fresh from the VALU: {hazard}'
          + (', OUTSIDE an inference unit' if outside else ''))
    bad_total += unpadded + hazard + outside
sys.exit(1 if bad_total else 0)
