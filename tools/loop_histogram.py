#!/usr/bin/env python3
"""Opcode histogram of the loops of one kernel in a gfx950 assembly file (hipcc ... --cuda-device-only -S with the Makefile's flags).
A loop is a backward branch: the lines from the branch target to the branch.  Without --loop the loops of the kernel are listed in
source order with their nesting depth, instruction count and the counts the change log quotes (VALU, DPP, LDS, scalar loads,
v_mov_b64, compares, selects); --loop N prints the whole histogram of loop N of that list, --innermost only lists loops that hold no
other loop.  --blocks (with --loop N) prints the same counts for every basic block of the loop (from one local label to the next) with
the branches that leave it: a loop with a branch inside (the pair loop of the P1 uniform-tile kernels: tiles with / without the validity
test) is counted per path by adding the blocks of that path.
usage: loop_histogram.py FILE.s KERNEL_REGEX [--innermost] [--loop N [--blocks]]
KERNEL_REGEX is matched against the demangled name, e.g. 'k_tile_uniform<3, 3, 2, true>'   (no GPU needed)"""
import collections, re, subprocess, sys


def functions(path):
    """{mangled name: [lines]} of the kernels (.amdhsa_kernel names) of the file"""
    text = open(path).read().split('\n')
    kernels = set(re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', '\n'.join(text), re.M))
    out, name = {}, None
    for ln in text:
        m = re.match(r'^([A-Za-z_][\w$.]*):', ln)
        if m and m.group(1) in kernels:
            name = m.group(1)
            out[name] = []
            continue
        if name and re.match(r'^\.Lfunc_end', ln):
            name = None
        if name:
            out[name].append(ln)
    return out


def loops(lines):
    """[(first, last, depth)] by line index: label ... backward branch to it"""
    label = {}
    for i, ln in enumerate(lines):
        m = re.match(r'^(\.LBB\d+_\d+):', ln)
        if m:
            label[m.group(1)] = i
    found = []
    for i, ln in enumerate(lines):
        m = re.match(r'^\s+s_c?branch\S*\s+(\.LBB\d+_\d+)', ln)
        if m and label.get(m.group(1), i+1) <= i:
            found.append((label[m.group(1)], i))
    # one entry per header: the widest range of its back edges
    by_head = {}
    for a, b in found:
        by_head[a] = max(b, by_head.get(a, b))
    rng = sorted(by_head.items())
    return [(a, b, sum(1 for c, d in rng if c <= a and b <= d)) for a, b in rng]


def opcodes(lines):
    ops = []
    for ln in lines:
        ln = ln.split(';')[0].strip()
        if not ln or ln.endswith(':') or ln.startswith('.'):
            continue
        ops.append((ln.split()[0], ln))
    return ops


def summary(ops):
    c = collections.Counter()
    for op, ln in ops:
        c['all'] += 1
        if op.startswith('v_'):
            c['valu'] += 1
            if re.search(r'\b(row_|wave_|quad_perm|row_bcast)', ln):
                c['dpp'] += 1
            if op.startswith('v_cmp'):
                c['v_cmp'] += 1
            if op.startswith('v_cndmask'):
                c['v_cndmask'] += 1
            if op.startswith('v_mov_b64'):
                c['v_mov_b64'] += 1
        elif op.startswith('ds_'):
            c['lds'] += 1
            if op.startswith('ds_add'):
                c['ds_add'] += 1
        elif op.startswith('s_load') or op.startswith('s_buffer_load'):
            c['s_load'] += 1
        elif op.startswith('s_waitcnt'):
            c['s_waitcnt'] += 1
        elif op.startswith('scratch_') or op.startswith('buffer_'):
            c['scratch/buffer'] += 1
    return c


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    pick = int(sys.argv[sys.argv.index('--loop')+1]) if '--loop' in sys.argv else None
    if pick is not None:
        args.remove(str(pick))
    path, want = args
    fns = functions(path)
    names = subprocess.run(['c++filt'], input='\n'.join(fns), capture_output=True, text=True).stdout.split('\n')
    keys = ('all', 'valu', 'dpp', 'lds', 'ds_add', 's_load', 's_waitcnt', 'v_mov_b64', 'v_cmp', 'v_cndmask', 'scratch/buffer')
    for sym, dem in zip(fns, names):
        if not re.search(want, dem):
            continue
        lines = fns[sym]
        ls = loops(lines)
        print(re.sub(r'\(.*', '', dem))
        for n, (a, b, depth) in enumerate(ls):
            inner = not any(c > a and d <= b for c, d, _ in ls if (c, d) != (a, b))
            if '--innermost' in sys.argv and not inner:
                continue
            if pick is not None and n != pick:
                continue
            ops = opcodes(lines[a:b+1])
            c = summary(ops)
            print('  loop {:2d} depth {} {:9s} {}'.format(n, depth, 'innermost' if inner else '', ' '.join('{} {}'.format(k, c[k]) for k in keys)))
            if pick is not None and '--blocks' in sys.argv:
                blocks, cur = [], ['(header)', []]
                for ln in lines[a:b+1]:
                    m = re.match(r'^(\.LBB\d+_\d+):', ln)
                    if m:
                        blocks.append(cur)
                        cur = [m.group(1), []]
                    else:
                        cur[1].append(ln)
                blocks.append(cur)
                for name, body in blocks:
                    cb = summary(opcodes(body))
                    if not cb['all']:
                        continue
                    out = [o[1] for o in opcodes(body) if re.match(r's_c?branch', o[0])]
                    print('      {:12s} {}   {}'.format(name, ' '.join('{} {}'.format(k, cb[k]) for k in keys[:4]+keys[8:10]), '; '.join(out)))
            elif pick is not None:
                for op, k in sorted(collections.Counter(op for op, _ in ops).items(), key=lambda t: (-t[1], t[0])):
                    print('      {:5d} {}'.format(k, op))


if __name__ == '__main__':
    main()
