#!/usr/bin/env python3
"""
Same machine code?  Compiles every em_pose_amd/csrc/*.hip of two git revisions to gfx950 assembly with the flags of
em_pose_amd/build.py (plus --cuda-device-only -S) and diffs the two outputs per file.  CPU only: hipcc cross-compiles.

    python scripts/dev/asm_diff.py HEAD~1 HEAD         # two revisions
    python scripts/dev/asm_diff.py HEAD .              # a revision against the working tree ('.' = the files on disk)

Both revisions are compiled at the SAME temporary path, one after the other, so that nothing that depends on the
path of a source (the compilation-unit id, debug directives) differs.  The comparison is a plain text diff;
only comment lines, .file/.ident/.loc/.cfi/.section-.debug directives and lines that carry the source path are left out.
Everything else -- instructions, labels, .amdhsa_ fields, the metadata note, device variables -- has to be equal.
Exit status 0 when every file is identical, 1 otherwise.
"""
import difflib
import glob
import os
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from em_pose_amd import build as B   # noqa: E402  (the flags and the compiler come from the build itself)

FLAGS = ['--offload-arch=' + B.ARCH, '-O3', '-std=c++17', '-fPIC', '-munsafe-fp-atomics', '-Wno-unused-result']
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


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    rev_a, rev_b = sys.argv[1], sys.argv[2]
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
                bad += 1
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
        return 1 if bad else 0
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    sys.exit(main())
