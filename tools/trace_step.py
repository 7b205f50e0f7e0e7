"""One steady-state step out of a rocprofv3 --kernel-trace csv of graph replays: the step boundary is found from a kernel that runs once
a step (the AdamW launch), the step = the kernels between its last two occurrences -> the timeline (start offset, duration, gap to the previous end, queue, grid),
and a summary of the torch / runtime glue kernels (at::native, rocclr) in it.
    python3 tools/trace_step.py <kernel_trace.csv> [marker substring = adamw] [out.txt]

The hand-offs of the inference step (bench.py's headline: clip chains of per-token and attention launches, then one logits launch that
ends the step): per chain and consecutive pair of launches the gap from the predecessor's end to the successor's start, grouped by the
predecessor's kind, beside the launch times by kernel and grid -- every step of the trace, warm-up and capture (steps more than 1.5
times the median span) left out.
    python3 tools/trace_step.py --handoff <dir-or-kernel_trace.csv> [out prefix]      -> <prefix>_gaps.csv, <prefix>_by_grid.csv, a table
"""
import collections, csv, glob, os, re, statistics, sys

KINDS = ('embedding + tail', 'head + tail', 'attention', 'head only')


def load(src):
    if os.path.isdir(src):
        src = sorted(glob.glob(os.path.join(src, '**', '*_kernel_trace.csv'), recursive=True))[-1]
    rows = list(csv.DictReader(open(src)))
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    return rows


def workgroups(r):
    g = w = 1
    for ax in 'XYZ':
        g *= int(r.get('Grid_Size_' + ax, 1) or 1)
        w *= int(r.get('Workgroup_Size_' + ax, 1) or 1)
    return g // max(w, 1)


def short_name(name):
    s = name.replace('void ', '').replace('(anonymous namespace)::', '')
    return s[:s.index('>(') + 1] if '>(' in s else s.split('(')[0]


def kind_of(name):
    """Kind of a chain launch (KINDS), 'logits' for the step's last launch, None for anything else."""
    m = re.search(r'layer_fused(?:_infer)?_kernel<.*?(true|false), (true|false)>', name)
    if m:
        head, tail = m.group(1) == 'true', m.group(2) == 'true'
        return 'head + tail' if head and tail else ('head only' if head else 'embedding + tail')
    if 'attn_fwd_row16' in name:
        return 'attention'
    if 'linear_kernel' in name:
        return 'logits'
    return None


def chains_of(step):
    """Split a step's chain launches (start order) into chains: by queue where every queue holds whole chains in order, else by
    walking the launches in start order and handing each to the chain that waits for its kind and ended earliest."""
    def whole(seq):
        ks = [k for k, _ in seq]
        n = len(ks)
        return (n >= 3 and n % 2 == 1 and ks[0] == 'embedding + tail' and ks[-1] == 'head only'
                and all(k == 'attention' for k in ks[1::2]) and all(k == 'head + tail' for k in ks[2:-1:2]))
    by_q = collections.defaultdict(list)
    for k, r in step:
        by_q[r.get('Queue_Id', '')].append((k, r))
    if len(by_q) > 1 and all(whole(c) for c in by_q.values()):
        return list(by_q.values())
    chains = []
    for k, r in step:
        s = int(r['Start_Timestamp'])
        if k == 'embedding + tail':
            chains.append([(k, r)])
            continue
        want = ('embedding + tail', 'head + tail') if k == 'attention' else ('attention',)
        open_ = [c for c in chains if c[-1][0] in want and int(c[-1][1]['End_Timestamp']) <= s]
        if not open_:
            return None
        min(open_, key=lambda c: int(c[-1][1]['End_Timestamp'])).append((k, r))
    return chains if chains and all(whole(c) for c in chains) else None


def handoff(src, prefix):
    rows = load(src)
    # launch times by kernel and grid, as profiles/*/..._by_grid.csv
    groups = collections.defaultdict(list)
    for r in rows:
        if kind_of(r['Kernel_Name']):
            groups[(short_name(r['Kernel_Name']), workgroups(r))].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    with open(prefix + '_by_grid.csv', 'w') as f:
        f.write('kernel,workgroups,calls,avg_us,min_us\n')
        for (n, wg), d in sorted(groups.items(), key=lambda kv: -sum(kv[1])):
            f.write(f'"{n}",{wg},{len(d)},{sum(d) / len(d):.2f},{min(d):.2f}\n')
    # steps: the chain launches up to and including a logits launch
    steps, cur = [], []
    for r in rows:
        k = kind_of(r['Kernel_Name'])
        if k is None:
            continue
        cur.append((k, r))
        if k == 'logits':
            steps.append(cur)
            cur = []
    span = lambda st: int(st[-1][1]['End_Timestamp']) - int(st[0][1]['Start_Timestamp'])
    med = statistics.median(span(s) for s in steps)
    launch, gap = collections.defaultdict(list), collections.defaultdict(list)
    chain_sum, join_gap, spans, used, nchains = [], [], [], 0, collections.Counter()
    for st in steps:
        if span(st) > 1.5 * med:
            continue
        ch = chains_of(st[:-1])
        if ch is None:
            continue
        used += 1
        nchains[len(ch)] += 1
        spans.append(span(st) / 1e3)
        for c in ch:
            for i, (k, r) in enumerate(c):
                launch[k].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
                if i + 1 < len(c):
                    gap[k].append((int(c[i + 1][1]['Start_Timestamp']) - int(r['End_Timestamp'])) / 1e3)
            chain_sum.append((int(c[-1][1]['End_Timestamp']) - int(c[0][1]['Start_Timestamp'])) / 1e3)
        join_gap.append((int(st[-1][1]['Start_Timestamp']) - max(int(c[-1][1]['End_Timestamp']) for c in ch)) / 1e3)
    avg = lambda d: sum(d) / len(d) if d else float('nan')
    md = lambda d: statistics.median(d) if d else float('nan')
    out = [f'steps in the trace {len(steps)}, used {used} (median span {med / 1e3:.1f} us; chains per step {dict(nchains)})', '',
           '| predecessor | pairs | launch avg | launch median | gap behind it avg | median | min | launch + gap avg |', '|---|---|---|---|---|---|---|---|']
    with open(prefix + '_gaps.csv', 'w') as f:
        f.write('predecessor,launches,launch_avg_us,launch_median_us,pairs,gap_avg_us,gap_median_us,gap_min_us\n')
        for k in KINDS:
            g = gap[k]
            f.write(f'{k},{len(launch[k])},{avg(launch[k]):.2f},{md(launch[k]):.2f},{len(g)},{avg(g):.2f},{md(g):.2f},{min(g) if g else float("nan"):.2f}\n')
            out.append(f'| {k} | {len(g)} | {avg(launch[k]):.2f} | {md(launch[k]):.2f} | {avg(g):.2f} | {md(g):.2f} | {min(g) if g else float("nan"):.2f} | '
                       f'{avg(launch[k]) + (avg(g) if g else 0):.2f} |')
        f.write(f'chain first start to last end,{len(chain_sum)},{avg(chain_sum):.2f},{md(chain_sum):.2f},,,,\n')
        f.write(f'last chain end to logits start,{len(join_gap)},,,{len(join_gap)},{avg(join_gap):.2f},{md(join_gap):.2f},{min(join_gap) if join_gap else float("nan"):.2f}\n')
        f.write(f'step first start to logits end,{len(spans)},{avg(spans):.2f},{md(spans):.2f},,,,\n')
    out += ['', f'chain, first start to last end (launches + gaps): avg {avg(chain_sum):.2f} us, median {md(chain_sum):.2f}',
            f'last chain end to logits start: avg {avg(join_gap):.2f} us, median {md(join_gap):.2f}',
            f'step, first start to logits end: avg {avg(spans):.2f} us, median {md(spans):.2f}']
    print('\n'.join(out))


def timeline():
    rows = load(sys.argv[1])
    marker = sys.argv[2] if len(sys.argv) > 2 else 'adamw'
    out = open(sys.argv[3], 'w') if len(sys.argv) > 3 else sys.stdout
    marks = [i for i, r in enumerate(rows) if marker in r['Kernel_Name']]
    step = rows[marks[-2] + 1:marks[-1] + 1]
    t0 = int(step[0]['Start_Timestamp'])
    end_prev, busy, total, glue, glue_t = t0, 0, 0, 0, 0
    cur_s = cur_e = None
    for r in step:
        s, e = int(r['Start_Timestamp']), int(r['End_Timestamp'])
        total += e - s
        if cur_s is None:
            cur_s, cur_e = s, e
        elif s <= cur_e:
            cur_e = max(cur_e, e)
        else:
            busy += cur_e - cur_s
            cur_s, cur_e = s, e
        gap = s - end_prev
        end_prev = max(end_prev, e)
        name = r['Kernel_Name']
        is_glue = 'at::native' in name or 'rocclr' in name
        glue += is_glue
        glue_t += (e - s) if is_glue else 0
        print(f"{(s - t0) / 1e3:9.1f} us  +{(e - s) / 1e3:7.1f}  gap {gap / 1e3:6.1f}  q{r.get('Queue_Id', '?'):>3s}  grid {r.get('Grid_Size_X', '?'):>8s}  "
              f"{'* ' if is_glue else '  '}{name[:110]}", file=out)
    busy += cur_e - cur_s
    print(f'step: {len(step)} kernels, span {(end_prev - t0) / 1e3:.1f} us, busy union {busy / 1e3:.1f} us, sum of durations {total / 1e3:.1f} us; '
          f'torch / runtime glue (*): {glue} kernels, {glue_t / 1e3:.1f} us', file=out)


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--handoff':
        handoff(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else 'handoff')
    else:
        timeline()
