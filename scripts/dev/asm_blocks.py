#!/usr/bin/env python3
"""
Dev: the basic blocks of one kernel in a gfx950 assembly file (hipcc ... --cuda-device-only -S), CPU only.

    python scripts/dev/asm_blocks.py FILE.s KERNEL_SUBSTRING [--min N] [--count MNEMONIC_PREFIX ...]

Per block (a label up to the next label): its instruction count, how many of them are MFMAs, and the number of
instructions whose mnemonic starts with each --count prefix; blocks below --min instructions are summed into one line.
Then the kernel's totals and its scratch / spill fields.  Two files compared block by block say whether the blocks that
hold MFMAs kept their size and where an epilogue's instructions went.
"""
import argparse
import re
import sys

LABEL = re.compile(r'^([.\w$]+):')


def kernel_lines(path, name):
    out, inside = [], False
    with open(path) as f:
        for line in f:
            m = LABEL.match(line)
            if m and not m.group(1).startswith('.'):
                inside = name in m.group(1) and not inside and not out
            if inside:
                if line.strip().startswith('.Lfunc_end'):
                    break
                out.append(line.rstrip())
    return out


def blocks(lines):
    cur, res = ['entry', []], []
    for line in lines:
        s = line.strip()
        m = LABEL.match(s)
        if m:
            if m.group(1).startswith('.L'):
                res.append(cur)
                cur = [m.group(1), []]
            continue
        if not s or s[0] in ';./' or s.startswith('//'):
            continue
        cur[1].append(s.split()[0])
    res.append(cur)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('file')
    ap.add_argument('kernel')
    ap.add_argument('--min', type=int, default=40)
    ap.add_argument('--count', nargs='*', default=['ds_bpermute', 'v_readlane', 'v_writelane', 'v_cndmask', 'v_cmp', 'ds_write',
                                                   'ds_max', 'v_max_u32_dpp', 'v_mov_b32_dpp', 's_waitcnt'])
    a = ap.parse_args()
    lines = kernel_lines(a.file, a.kernel)
    if not lines:
        sys.exit('no kernel matching %r' % a.kernel)
    print('%-14s %6s %5s  %s' % ('block', 'instr', 'mfma', '  '.join(a.count)))
    small, total = [0, 0] + [0] * len(a.count), [0, 0] + [0] * len(a.count)
    for label, ins in blocks(lines):
        row = [len(ins), sum(i.startswith('v_mfma') for i in ins)] + [sum(i.startswith(c) for i in ins) for c in a.count]
        total = [x + y for x, y in zip(total, row)]
        if row[0] < a.min and not row[1]:
            small = [x + y for x, y in zip(small, row)]
            continue
        print('%-14s %6d %5d  %s' % (label, row[0], row[1], '  '.join('%*d' % (len(c), v) for c, v in zip(a.count, row[2:]))))
    for tag, row in (('(small blocks)', small), ('TOTAL', total)):
        print('%-14s %6d %5d  %s' % (tag, row[0], row[1], '  '.join('%*d' % (len(c), v) for c, v in zip(a.count, row[2:]))))
    with open(a.file) as f:
        for line in f:
            if a.kernel in line and ('private_seg_size' in line or 'uses_flat_scratch' in line or 'num_vgpr' in line):
                print(line.strip())


if __name__ == '__main__':
    main()
