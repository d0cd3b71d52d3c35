#!/usr/bin/env python3
"""Kernel by kernel comparison of two builds of libpnl_hip.so (two object directories, make BUILD=... OUT=...): for every kernel
symbol of the gfx950 code objects the units that hold it, a digest of its instruction stream (llvm-objdump -d without addresses,
branch targets and the padding behind the last instruction) and its resources (VGPR / AGPR / SGPR / scratch / static LDS of the code
object's notes).  A kernel whose stream differs only in the literal added to s_getpc_b64 (the distance to a table in .rodata,
which depends on what else the code object holds) is reported as "pc-relative" with the number of such sites.  Prints what moved,
what vanished, what is new, what differs, and the digest of every unit's .text.
usage: unit_kernels.py OLD_BUILD_DIR NEW_BUILD_DIR [-v] [--old-name REGEX REPL]
(no GPU needed; -v lists every kernel, not only the differences; --old-name rewrites the demangled names of the OLD build before the
two are matched, for a kernel that has gained a template parameter:
--old-name '(k_tile_distant<[^>]*)>' '\\1, false>' compares every old instantiation with the new one whose added flag is off)"""
import hashlib, os, re, subprocess, sys, tempfile
LLVM = '/opt/rocm/lib/llvm/bin'


def code_object(obj, tmp):
    fat, co = os.path.join(tmp, 'fat.bin'), os.path.join(tmp, os.path.basename(obj)+'.co')
    subprocess.run([LLVM+'/llvm-objcopy', '-O', 'binary', '--only-section=.hip_fatbin', obj, fat], check=True)
    r = subprocess.run([LLVM+'/clang-offload-bundler', '--type=o', '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--input='+fat,
                        '--output='+co, '--unbundle'], capture_output=True)
    return co if r.returncode == 0 and os.path.exists(co) and os.path.getsize(co) else None


def kernels_of(co):
    """{symbol: (digest of the instructions, the same with the pc-relative literals masked, number of such literals, number of
    instructions, resources)} and the digest of .text"""
    notes = subprocess.run([LLVM+'/llvm-readelf', '--notes', co], capture_output=True, text=True).stdout
    res = {}
    for b in re.split(r'\n\s+- \.agpr_count', notes)[1:]:
        b = '.agpr_count'+b
        g = lambda k: (re.search(r'\.%s:\s+(\S+)' % k, b) or [None, '?'])[1]
        res[g('name')] = 'vgpr {} agpr {} sgpr {} scratch {} lds {}'.format(g('vgpr_count'), g('agpr_count'), g('sgpr_count'),
                                                                           g('private_segment_fixed_size'), g('group_segment_fixed_size'))
    dis = subprocess.run([LLVM+'/llvm-objdump', '-d', '--no-show-raw-insn', '--no-leading-addr', co], capture_output=True, text=True).stdout
    out, name, lines = {}, None, []
    sha = lambda ls: hashlib.sha256('\n'.join(ls).encode()).hexdigest()[:16]
    def close():
        if name in res:
            while lines and lines[-1] in ('s_nop 0', 's_code_end'):      # fill up to the alignment of the next symbol
                lines.pop()
            masked, sites = list(lines), 0
            for i, ln in enumerate(lines[:-1]):
                if ln.startswith('s_getpc_b64') and lines[i+1].startswith('s_add_u32'):
                    masked[i+1] = re.sub(r'\S+$', 'PCREL', lines[i+1])
                    sites += 1
            out[name] = (sha(lines), sha(masked), sites, len(lines), res[name])
    for ln in dis.split('\n'):
        m = re.match(r'^[0-9a-f]* ?<(.+)>:$', ln)
        if m:
            close()
            name, lines = m.group(1), []
            continue
        ln = re.sub(r'\s*//.*$', '', ln).strip()
        if not ln or ln == '...' or re.match(r'^<[^>]+>:$', ln):       # zero padding, local labels of a kernel
            continue
        ln = re.sub(r'<[^>]+>', '<>', ln)               # branch targets
        lines.append(ln)
    close()
    subprocess.run([LLVM+'/llvm-objcopy', '-O', 'binary', '--only-section=.text', co, co+'.text'], check=True)
    return out, hashlib.sha256(open(co+'.text', 'rb').read()).hexdigest()[:16]


def build(d, tmp):
    units = {}
    for obj in sorted(os.listdir(d)):
        if obj.endswith('.o'):
            co = code_object(os.path.join(d, obj), tmp)
            if co:
                units[obj[:-2]] = kernels_of(co)
    return units


def by_symbol(units, rename=None):
    """keyed by the demangled name without any `(anonymous namespace)::`, in the kernel's name and in its parameter types: a kernel
    that moves into or out of an unnamed namespace stays the same kernel"""
    syms = sorted({k for ks, _ in units.values() for k in ks})
    names = subprocess.run(['c++filt'], input='\n'.join(syms), capture_output=True, text=True).stdout.split('\n')
    plain = {k: d.replace('(anonymous namespace)::', '') for k, d in zip(syms, names)}
    if rename:
        plain = {k: re.sub(rename[0], rename[1], d, count=1) for k, d in plain.items()}
    sym = {}
    for u, (ks, _) in units.items():
        for k, v in ks.items():
            sym.setdefault(plain[k], {})[u] = v
    return sym


def main():
    verbose = '-v' in sys.argv
    args, rename = [a for a in sys.argv[1:] if a != '-v'], None
    if '--old-name' in args:
        i = args.index('--old-name')
        rename = (args[i+1], args[i+2])
        del args[i:i+3]
    old_dir, new_dir = args
    with tempfile.TemporaryDirectory() as t1, tempfile.TemporaryDirectory() as t2:
        old, new = build(old_dir, t1), build(new_dir, t2)
    print('== .text of the units (digest old -> new)')
    for u in sorted(set(old) | set(new)):
        a, b = old.get(u, ({}, '-')), new.get(u, ({}, '-'))
        print('{:14s} {:4d} -> {:4d} kernels   {} -> {}   {}'.format(u, len(a[0]), len(b[0]), a[1], b[1], 'identical' if a[1] == b[1] else 'CHANGED'))
    so, sn = by_symbol(old, rename), by_symbol(new)
    short = {k: re.sub(r'^void ', '', k)[:110] for k in set(so) | set(sn)}
    count = {'same': 0, 'moved': 0, 'copies dropped': 0, 'vanished': 0, 'new': 0, 'pc-relative': 0, 'differs': 0}
    print('== kernels (symbol: units old -> units new)')
    for k in sorted(set(so) | set(sn), key=lambda k: short[k]):
        a, b = so.get(k, {}), sn.get(k, {})
        what = []
        if not b:
            kind = 'vanished'
        elif not a:
            kind = 'new'
        else:
            # every copy that is left against every copy there was (the copies of one build agree or are reported)
            da, db = {v[0] for v in a.values()}, {v[0] for v in b.values()}
            ma, mb = {v[1:] for v in a.values()}, {v[1:] for v in b.values()}
            if ma != mb:
                kind = 'differs'
                what = ['   old '+u+' '+' '.join(map(str, v)) for u, v in sorted(a.items())]+['   new '+u+' '+' '.join(map(str, v)) for u, v in sorted(b.items())]
            elif da != db:
                kind = 'pc-relative'
                what = ['   {} literals of s_getpc_b64 + s_add_u32 differ at most, nothing else'.format(max(v[2] for v in b.values()))]
            elif set(a) == set(b):
                kind = 'same'
            elif set(b) < set(a):
                kind = 'copies dropped'
            else:
                kind = 'moved'
        count[kind] += 1
        if verbose or kind != 'same':
            print('{:15s} {}: {} -> {}'.format(kind, short[k], ','.join(sorted(a)) or '-', ','.join(sorted(b)) or '-'))
            for w in what:
                print(w)
    print('== '+', '.join('{} {}'.format(v, k) for k, v in count.items()))


if __name__ == '__main__':
    main()
