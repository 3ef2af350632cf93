#!/usr/bin/env python3
"""
Compare the device assembly of two revisions, kernel by kernel.

    python tools/diff_device_asm.py REV_A [REV_B|worktree] [--allow REGEX] [-j N] [--keep]

Each side is exported into a temporary directory (`git archive` for a revision; for `worktree`, the default second
side, a copy of the checkout's files as they stand, ignored ones left out; the checkout itself is left alone) and
`make asm` (csrc/Makefile: every object's own flags plus --offload-device-only -S) is run there.  Every `.s` file is split into its functions --
the body `_Z...:` .. `.Lfunc_end<N>:` plus the kernel's `.amdhsa_kernel` .. `.end_amdhsa_kernel` descriptor block --
with `;` comments stripped and the `.L` labels renumbered in order of appearance, so that a kernel reads the same
wherever it stands in its object.  The per-translation-unit `__hip_cuid_*` symbol, the only difference between two
builds of the same code, lies outside every function and is never looked at.

Kernels are matched by name over the union of the objects, so one that moves between objects is still compared.  The
report: kernels on one side only, kernels whose text differs (demangled), and the number of identical kernels per
object.  Exit status 1 on any difference that --allow (a regular expression searched in the demangled name) does not
cover.  The tool compares text and nothing else; it needs hipcc and no GPU.  A revision from before the `asm` target
existed is built with this checkout's Makefile (said so in the output).
"""
import argparse
import difflib
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join('pfb_clean_amd', 'csrc')
FUNC = re.compile(r'^(_Z\w+):')
FEND = re.compile(r'^\.Lfunc_end\d+:')
KBEG = re.compile(r'^\s*\.amdhsa_kernel\s+(\S+)')
KEND = re.compile(r'^\s*\.end_amdhsa_kernel')
LABEL = re.compile(r'\.L[\w$.]+')


def export(rev, dst):
    """the tree of `rev` (or the checkout's files as they stand, ignored ones left out) under dst"""
    if rev == 'worktree':
        names = subprocess.check_output(['git', '-C', ROOT, 'ls-files', '-z', '-co', '--exclude-standard', '--', 'pfb_clean_amd', 'include'])
        for n in names.decode().split('\0'):
            if n and os.path.isfile(os.path.join(ROOT, n)):
                os.makedirs(os.path.dirname(os.path.join(dst, n)), exist_ok=True)
                shutil.copy2(os.path.join(ROOT, n), os.path.join(dst, n))
    else:
        ar = subprocess.Popen(['git', '-C', ROOT, 'archive', rev, '--', 'pfb_clean_amd', 'include'], stdout=subprocess.PIPE)
        subprocess.check_call(['tar', '-x', '-C', dst], stdin=ar.stdout)
        if ar.wait():
            sys.exit(f'git archive {rev} failed')


def build_asm(tree, jobs):
    """make asm in the tree -> {object name: path of its .s}"""
    csrc, out = os.path.join(tree, CSRC), os.path.join(tree, 'asm')
    os.makedirs(out)
    cmd = ['make', '-C', csrc, 'asm', 'OBJDIR=' + out, '-j', str(jobs)]
    if not re.search(r'^asm:', open(os.path.join(csrc, 'Makefile')).read(), re.M):
        print(f'  ({os.path.basename(tree)}: its Makefile has no asm target; built with this checkout\'s Makefile)')
        cmd[3:3] = ['-f', os.path.join(ROOT, CSRC, 'Makefile')]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode:
        sys.exit(r.stdout[-4000:] + f'\nmake asm failed in {tree}')
    return {os.path.basename(p)[:-2]: p for p in sorted(glob.glob(os.path.join(out, '*.s')))}


def functions(path):
    """{symbol: normalised text} of one .s file: body and kernel descriptor, comments out, .L labels renumbered"""
    body, desc, cur, kcur = {}, {}, None, None
    for line in open(path):
        line = line.split(';', 1)[0].rstrip()
        if cur is None and kcur is None:
            m = FUNC.match(line)
            k = KBEG.match(line)
            if m:
                cur = m.group(1)
                body[cur] = []
            elif k:
                kcur = k.group(1)
                desc[kcur] = [line.strip()]
            continue
        if cur is not None:
            if FEND.match(line):
                cur = None
            elif line:
                body[cur].append(line)
        else:
            desc[kcur].append(line.strip())
            if KEND.match(line):
                kcur = None
    out = {}
    for name, lines in body.items():
        ids = {}
        text = '\n'.join(lines + desc.get(name, []))
        out[name] = LABEL.sub(lambda m: ids.setdefault(m.group(0), f'.L{len(ids)}'), text)
    return out


def demangle(names):
    names = list(names)
    if not names:
        return {}
    try:
        r = subprocess.run(['c++filt'], input='\n'.join(names), stdout=subprocess.PIPE, text=True, check=True)
        return dict(zip(names, r.stdout.split('\n')))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('rev_a')
    ap.add_argument('rev_b', nargs='?', default='worktree')
    ap.add_argument('--allow', metavar='REGEX', help='differing or one-sided kernels whose demangled name matches are reported but do not fail')
    ap.add_argument('-j', type=int, default=16, dest='jobs')
    ap.add_argument('--keep', action='store_true', help='keep the temporary trees (their paths are printed)')
    ap.add_argument('--show', type=int, default=0, metavar='N', help='print the first N lines of each differing kernel\'s unified diff')
    a = ap.parse_args()

    tmp = tempfile.mkdtemp(prefix='devasm_')
    try:
        sides = []
        for tag, rev in (('a', a.rev_a), ('b', a.rev_b)):
            tree = os.path.join(tmp, tag)
            os.makedirs(tree)
            export(rev, tree)
            print(f'{tag}: {rev}: make asm ...', flush=True)
            fns, where = {}, {}
            for obj, path in build_asm(tree, a.jobs).items():
                for name, text in functions(path).items():
                    fns[name], where[name] = text, obj
            sides.append((fns, where))
        (fa, wa), (fb, wb) = sides
        dm = demangle(set(fa) | set(fb))
        allow = re.compile(a.allow) if a.allow else None
        bad = 0

        def flag(name):
            nonlocal bad
            ok = allow is not None and allow.search(dm[name])
            bad += not ok
            return ' (allowed)' if ok else ''

        for tag, rev, only, where in (('a', a.rev_a, set(fa) - set(fb), wa), ('b', a.rev_b, set(fb) - set(fa), wb)):
            for n in sorted(only):
                print(f'only in {rev} [{where[n]}]{flag(n)}: {dm[n]}')
        same = {}
        for n in sorted(set(fa) & set(fb)):
            if fa[n] == fb[n]:
                same[wb[n]] = same.get(wb[n], 0) + 1
                if wa[n] != wb[n]:
                    print(f'moved {wa[n]} -> {wb[n]}, identical: {dm[n]}')
                continue
            la, lb = fa[n].split('\n'), fb[n].split('\n')
            print(f'DIFFERS [{wa[n]} / {wb[n]}]{flag(n)}: {dm[n]}   ({len(la)} / {len(lb)} lines)')
            for line in list(difflib.unified_diff(la, lb, a.rev_a, a.rev_b, lineterm='', n=1))[:a.show]:
                print('    ' + line)
        for obj in sorted(set(wa.values()) | set(wb.values())):
            na, nb = sum(o == obj for o in wa.values()), sum(o == obj for o in wb.values())
            print(f'{obj:20s} {same.get(obj, 0):4d} identical   ({na} in {a.rev_a}, {nb} in {a.rev_b})')
        print('FAIL: %d kernel(s) differ or are missing' % bad if bad else 'OK: every kernel identical' + (' or allowed' if allow else ''))
        return 1 if bad else 0
    finally:
        if a.keep:
            print('kept', tmp)
        else:
            shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    sys.exit(main())
