"""Compare the gfx950 machine code of the library's kernels between two source trees (a refactor's "same code" check; no GPU needed).

    python tools/isa_compare.py PARENT_TREE BRANCH_TREE [-o profiles/NAME.txt] [--keep DIR] [-D NAME[=VALUE] ...]
                                [--renamed 'FILE: OLD=FILE: NEW' ...] [--only FILE ...] [--show KERNEL]

Both trees are compiled with build.py's flags plus --save-temps (and every -D given, e.g. a profiler build of both); for every kernel of
every source in build.py's SOURCES the table gives registers, scratch, LDS, occupancy, instruction counts by class (parent | branch) and
whether the instruction streams are identical after dropping comments, directives and the function number inside local labels.  A kernel
that the branch renamed is compared under its new name with --renamed (both names as the table prints them).  Exit status 1 if any
kernel differs.  --only compiles and compares just the named sources (the loop of a search on one file; a committed record is made from
the full run), --show prints the differing regions of one kernel (a name as the table prints it, or a part of one) with register
numbers normalised.
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from transeditor_amd.build import EXTRA_FLAGS, FLAGS, SOURCES, _hipcc  # noqa: E402

FILES = [s[:-len('.hip')] for s in SOURCES]
RES = [('VGPR', r'; NumVgprs: (\d+)'), ('AGPR', r'; NumAgprs: (\d+)'), ('SGPR', r'; TotalNumSgprs: (\d+)'),
       ('scratch', r'; ScratchSize: (\d+)'), ('LDS', r'; LDSByteSize: (\d+)'), ('occ', r'; Occupancy: (\d+)')]
CLASSES = [('MFMA', r'v_mfma'), ('ds_read', r'ds_read|ds_load'), ('ds_write', r'ds_write|ds_store'), ('gload_lds', r'global_load_lds|buffer_load.* lds'),
           ('gload', r'(global|buffer)_load'), ('gstore', r'(global|buffer)_store'), ('VALU', r'v_'), ('s_waitcnt', r's_waitcnt'),
           ('s_barrier', r's_barrier')]


def compile_tree(tree, out, defines=(), files=FILES):
    os.makedirs(out, exist_ok=True)
    procs = []
    for f in files:
        src = os.path.join(os.path.abspath(tree), 'transeditor_amd', 'csrc', f + '.hip')
        if not os.path.exists(src):                            # a source the other tree added: its kernels are listed as 'only in'
            continue
        cmd = [_hipcc(), *FLAGS, *EXTRA_FLAGS.get(f + '.hip', []), *('-D' + d for d in defines), '--save-temps', '-Rpass-analysis=kernel-resource-usage', '-c', src, '-o', f + '.o']
        procs.append((f, subprocess.Popen(cmd, cwd=out, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for f, p in procs:
        log, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError(f'hipcc failed on {tree}/{f}.hip:\n{log.decode()}')


def kernels(out, files=FILES):
    """{demangled-ish kernel name: (resources, instruction list)} of every kernel in the device assembly of a compiled tree."""
    found = {}
    for f in files:
        path = os.path.join(out, f + '-hip-amdgcn-amd-amdhsa-gfx950.s')
        if not os.path.exists(path):
            continue
        text = open(path).read()
        for m in re.finditer(r'^(_Z\w+):.*?^\.Lfunc_end\d+:(.*?^; Occupancy: \d+)', text, re.S | re.M):
            name = subprocess.check_output(['c++filt', m.group(1)]).decode().strip()
            name = re.sub(r'\(anonymous namespace\)::|\(.*\)$|^void ', '', name)
            ins = []
            for line in m.group(0).split('\n')[1:]:
                line = line.split(';')[0].strip()
                if not line or line.startswith('.') and not line.endswith(':'):
                    continue
                ins.append(re.sub(r'\.L(BB|func_end)\d+', r'.L\1', re.sub(r'\s+', ' ', line)))
            res = {k: int(re.search(pat, m.group(2)).group(1)) for k, pat in RES}
            found[f + ': ' + name] = (res, ins)
    return found


def classify(ins):
    counts = {k: 0 for k, _ in CLASSES}
    for line in ins:
        for k, pat in CLASSES:
            if re.match(pat, line):
                counts[k] += 1
                break
    return counts


def show(name, ip, ib):
    """The regions in which two instruction lists differ once register numbers are dropped, as text."""
    def norm(ins):
        return [re.sub(r'\b([vsa])(\d+|\[\d+:\d+\])', r'\1#', line) for line in ins]
    np_, nb = norm(ip), norm(ib)
    ops = [o for o in difflib.SequenceMatcher(None, np_, nb, autojunk=False).get_opcodes() if o[0] != 'equal']
    lines = [f'{name}: {len(ops)} regions differ with register numbers normalised (parent line | branch line)']
    for _, i1, i2, j1, j2 in ops:
        lines.append(f'  @ {i1 + 1} | {j1 + 1}')
        lines += ['    - ' + x for x in np_[i1:i2]] + ['    + ' + x for x in nb[j1:j2]]
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('parent')
    ap.add_argument('branch')
    ap.add_argument('-o', '--output')
    ap.add_argument('--keep', help='directory for the compiler outputs (default: a temporary one)')
    ap.add_argument('--renamed', action='append', default=[], metavar='OLD=NEW', help='a parent kernel and its name in the branch')
    ap.add_argument('-D', dest='defines', action='append', default=[], metavar='NAME[=VALUE]', help='extra define for both trees')
    ap.add_argument('--only', nargs='+', default=[], metavar='FILE', help='compile and compare only these sources of build.py\'s SOURCES')
    ap.add_argument('--show', metavar='KERNEL', help='print the differing regions of this kernel, register numbers normalised')
    a = ap.parse_args()
    files = [f[:-len('.hip')] if f.endswith('.hip') else f for f in map(os.path.basename, a.only)] or FILES
    if set(files) - set(FILES):
        ap.error('not in build.py\'s SOURCES: ' + ', '.join(sorted(set(files) - set(FILES))))
    with tempfile.TemporaryDirectory() as tmp:
        base = a.keep or tmp
        sides = []
        for tag, tree in (('parent', a.parent), ('branch', a.branch)):
            compile_tree(tree, os.path.join(base, tag), a.defines, files)
            sides.append(kernels(os.path.join(base, tag), files))
    par, br = sides
    for pair in a.renamed:
        old, new = pair.split('=')
        par[f'{new} (parent: {old})'] = par.pop(old)
        br[f'{new} (parent: {old})'] = br.pop(new)
    lines = ['machine code of the library\'s kernels, parent | branch (build.py flags' + ''.join(' -D' + d for d in a.defines) + ' + --save-temps, gfx950)'
             + (', only ' + ' '.join(f + '.hip' for f in files) if a.only else ''), '']
    ndiff = 0
    for name in sorted(set(par) | set(br)):
        if name not in par or name not in br:
            lines.append(f'{name}: only in {"parent" if name in par else "branch"}')
            ndiff += 1
            continue
        (rp, ip), (rb, ib) = par[name], br[name]
        cp, cb = classify(ip), classify(ib)
        same = ip == ib
        ndiff += not same or rp != rb
        lines.append(f'{name}: instruction stream {"IDENTICAL" if same else "DIFFERS"} ({len(ip)} | {len(ib)} lines)')
        lines.append('    ' + '  '.join(f'{k} {rp[k]}|{rb[k]}' for k, _ in RES) + ('' if rp == rb else '   <-- RESOURCES DIFFER'))
        lines.append('    ' + '  '.join(f'{k} {cp[k]}|{cb[k]}' for k, _ in CLASSES))
    lines += ['', f'{len(par)} kernels in the parent, {len(br)} in the branch, {ndiff} differ']
    if a.show:
        for name in sorted(set(par) & set(br)):
            if a.show in name:
                lines += [''] + show(name, par[name][1], br[name][1])
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if a.output:
        open(a.output, 'w').write(text)
    return 1 if ndiff else 0


if __name__ == '__main__':
    sys.exit(main())
