#!/usr/bin/env python3
"""
Same machine code?  Compiles every em_pose_amd/csrc/*.hip of two git revisions to gfx950 assembly with FLAGS of
em_pose_amd/build.py (plus --cuda-device-only -S) and diffs the two outputs per file.  CPU only: hipcc cross-compiles.

    python scripts/dev/asm_diff.py HEAD~1 HEAD         # two revisions
    python scripts/dev/asm_diff.py HEAD .              # a revision against the working tree ('.' = the files on disk)
    python scripts/dev/asm_diff.py HEAD~1 . --by-kernel   # ... when kernels moved between files

Both revisions are compiled at the SAME temporary path, one after the other, so that nothing that depends on the
path of a source (the compilation-unit id, debug directives) differs.  The comparison is a plain text diff;
only comment lines, .file/.ident/.loc/.cfi/.section-.debug directives and lines that carry the source path are left out.
Everything else -- instructions, labels, .amdhsa_ fields, the metadata note, device variables -- has to be equal.
Exit status 0 when every file is identical, 1 otherwise.

--by-kernel: for a change that moves kernels from one file to another.  Files present in both revisions are compared
as above; in addition every .s is cut into its functions (the symbol's body with its .amdhsa_kernel block and .set lines),
its entries of the metadata note and its device variables, and these are compared BY NAME across all files of the two
revisions.  Local labels (.LBB3_7, .Lfunc_end3: numbered by position in the file) are renumbered in order of appearance
within a function and comments at the end of a line are dropped; nothing else is normalised.  A name on one side only, or twice on one side, counts as a difference;
a file on one side only does not.  Exit status 0 when every common file and every name is identical.
"""
import difflib
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from em_pose_amd import build as B   # noqa: E402  (the flags and the compiler come from the build itself)

FLAGS = B.FLAGS
DEBUG_DIRECTIVES = ('.file', '.ident', '.loc', '.cfi_', '.section\t.debug', '.section .debug')


def checkout(rev, dst):
    """The csrc/ and include/ of a revision (or of the working tree for '.') under dst."""
    if rev == '.':
        for sub in ('em_pose_amd/csrc', 'include'):
            if os.path.isdir(os.path.join(ROOT, sub)):
                shutil.copytree(os.path.join(ROOT, sub), os.path.join(dst, sub),
                                ignore=shutil.ignore_patterns('*.o', '*.so', '*.s'))
        return
    tar = subprocess.run(['git', '-C', ROOT, 'archive', rev, 'em_pose_amd/csrc', 'include'],
                         stdout=subprocess.PIPE, check=True).stdout
    subprocess.run(['tar', '-x', '-C', dst], input=tar, check=True)


def compile_all(rev, work, out):
    """Compile a revision at work/ (always the same path) and move the .s files to out/."""
    shutil.rmtree(work, ignore_errors=True)
    os.makedirs(work)
    os.makedirs(out)
    checkout(rev, work)
    srcs = sorted(glob.glob(os.path.join(work, 'em_pose_amd', 'csrc', '*.hip')))

    def one(src):
        p = subprocess.run([B._hipcc()] + FLAGS + ['--cuda-device-only', '-S', src, '-o', src[:-4] + '.s'],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        if p.returncode != 0:
            raise RuntimeError('hipcc failed on {} of {}:\n{}'.format(os.path.basename(src), rev, p.stdout.decode()))
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        list(ex.map(one, srcs))
    for src in srcs:
        shutil.move(src[:-4] + '.s', os.path.join(out, os.path.basename(src)[:-4] + '.s'))


def kept_lines(path, work):
    lines = []
    with open(path) as f:
        for line in f:
            s = line.strip()
            if not s or s.startswith(';') or s.startswith('//') or s.startswith(DEBUG_DIRECTIVES) or work in s:
                continue
            lines.append(line.rstrip())
    return lines


LOCAL_LABEL = re.compile(r'\.L[A-Za-z_]+[0-9]+(?:_[0-9]+)?')


def renumbered(lines):
    """Local labels by order of first appearance: their numbers count functions and blocks of the whole file."""
    seen = {}
    return [LOCAL_LABEL.sub(lambda m: seen.setdefault(m.group(0), '.L{}'.format(len(seen))), line.split(';')[0].rstrip())
            for line in lines]   # (trailing comments name blocks by their number in the file: left out)


def pieces(lines):
    """{(kind, name): [lines]} of one file: 'function' (a kernel with its descriptor, or a device function that was not
    inlined), 'metadata' (a kernel's entry of the note), 'variable' (a device or LDS variable)."""
    out = {}
    i, n = 0, len(lines)
    while i < n:
        m = re.match(r'\s*\.type\s+(\S+),@(function|object)', lines[i])
        if not m:
            i += 1
            continue
        name, kind = m.group(1), m.group(2)
        if kind == 'object':
            j = i
            while j < n and not re.match(r'\s*\.size\s+' + re.escape(name) + ',', lines[j]):
                j += 1
            if not name.startswith('__hip_cuid_'):   # (the compilation-unit id: a hash of the file, not code)
                out[('variable', name)] = lines[i:j + 1]
            i = j + 1
            continue
        # back over .protected / .globl / .weak / .p2align to the .section or .text that opens the function
        b = i
        while b > 0 and not re.match(r'\s*\.(section|text)\b', lines[b]):
            b -= 1
        j = i
        while j < n and not re.match(r'\s*\.size\s+' + re.escape(name) + ',', lines[j]):
            j += 1
        j += 1
        while j < n and lines[j].lstrip().startswith('.set ' + name + '.'):
            j += 1
        out[('function', name)] = renumbered(lines[b:j])
        i = j
    if 'amdhsa.kernels:' in lines:
        i = lines.index('amdhsa.kernels:') + 1
        while i < n and lines[i].startswith('  '):
            j = i + 1
            while j < n and lines[j].startswith('   '):
                j += 1
            entry = lines[i:j]
            names = [l.split(':', 1)[1].strip() for l in entry if l.startswith('    .name:')]
            out[('metadata', names[0] if names else '?')] = entry
            i = j
    return out


def by_kernel(tmp, work, rev_a, rev_b):
    """Functions, metadata entries and variables by name across all files; returns the number of differences."""
    sides = []
    bad = 0
    for rev, sub in ((rev_a, 'a'), (rev_b, 'b')):
        found = {}
        for name in sorted(os.listdir(os.path.join(tmp, sub))):
            for key, body in pieces(kept_lines(os.path.join(tmp, sub, name), work)).items():
                if key in found and key[0] != 'function':
                    continue   # (a kernel defined twice is reported once, through its function)
                if key in found:
                    print('{:<9s} {}  TWICE in {}: {} and {}'.format(key[0], key[1], rev, found[key][0], name))
                    bad += 1
                found[key] = (name, body)
        sides.append(found)
    a, b = sides
    moved = 0
    for key in sorted(set(a) | set(b)):
        if key not in a or key not in b:
            print('{:<9s} {}  ONLY IN {} ({})'.format(key[0], key[1], rev_a if key in a else rev_b, (a.get(key) or b.get(key))[0]))
            bad += 1
        elif a[key][1] != b[key][1]:
            bad += 1
            diff = list(difflib.unified_diff(a[key][1], b[key][1], rev_a, rev_b, lineterm='', n=1))
            print('{:<9s} {}  DIFFERENT ({} -> {}, {} diff lines)'.format(key[0], key[1], a[key][0], b[key][0], len(diff)))
            print('\n'.join('    ' + d for d in diff[:40]))
        elif a[key][0] != b[key][0]:
            moved += 1
            print('{:<9s} {}  identical  ({} lines)  {} -> {}'.format(key[0], key[1], len(a[key][1]), a[key][0], b[key][0]))
    same_place = len(set(a) & set(b)) - moved
    print('{} names ({} functions) compared: {} moved between files, {} where they were; {} differ, are missing or double'.format(
        len(set(a) | set(b)), sum(1 for k in set(a) | set(b) if k[0] == 'function'), moved, same_place, bad))
    return bad


def main():
    args = [x for x in sys.argv[1:] if x != '--by-kernel']
    kernels = '--by-kernel' in sys.argv[1:]
    if len(args) != 2:
        sys.exit(__doc__)
    rev_a, rev_b = args
    tmp = tempfile.mkdtemp(prefix='asm_diff_')
    work = os.path.join(tmp, 'tree')
    try:
        compile_all(rev_a, work, os.path.join(tmp, 'a'))
        compile_all(rev_b, work, os.path.join(tmp, 'b'))
        names = sorted(set(os.listdir(os.path.join(tmp, 'a'))) | set(os.listdir(os.path.join(tmp, 'b'))))
        bad = 0
        for name in names:
            pa, pb = os.path.join(tmp, 'a', name), os.path.join(tmp, 'b', name)
            if not (os.path.exists(pa) and os.path.exists(pb)):
                print('{:<24s} ONLY IN {}'.format(name, rev_a if os.path.exists(pa) else rev_b))
                bad += 0 if kernels else 1   # (by kernel: what the file held is looked for by name below)
                continue
            a, b = kept_lines(pa, work), kept_lines(pb, work)
            if a == b:
                print('{:<24s} identical  ({} lines)'.format(name, len(a)))
            else:
                bad += 1
                diff = list(difflib.unified_diff(a, b, rev_a, rev_b, lineterm='', n=1))
                print('{:<24s} DIFFERENT  ({} / {} lines, {} diff lines)'.format(name, len(a), len(b), len(diff)))
                print('\n'.join('    ' + d for d in diff[:40]))
        print('{} of {} files differ between {} and {}'.format(bad, len(names), rev_a, rev_b))
        if kernels:
            bad += by_kernel(tmp, work, rev_a, rev_b)
        return 1 if bad else 0
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    sys.exit(main())
