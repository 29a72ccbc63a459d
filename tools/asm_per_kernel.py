#!/usr/bin/env python3
"""Compares the device assembly of one translation unit built from two trees kernel by kernel, for a change that moves host code
and with it the order in which the kernel instantiations are emitted.

    hipcc <FLAGS of build.py> --cuda-device-only -S csrc/<unit>.hip -o <a|b>.s      (once per tree)
    tools/asm_per_kernel.py a.s b.s [table.txt]

A kernel's text runs from its `.section .text.<symbol>` line to the next kernel's.  What depends on a kernel's position in the file and
on nothing else is normalised away: the function index in block labels (`.LBB<i>_<n>`, `BB<i>_<n>` in comments, `.Lfunc_end<i>`) and the
column the assembler aligns comments to.  Lines containing __hip_cuid_ are dropped as in profiles/r21_sched_asm.txt.  Prints one line
per kernel: demangled name, lines, sha256 of the normalised text in the first file, and whether the second file's is identical."""
import hashlib
import re
import subprocess
import sys


def norm(line):
    line = re.sub(r'BB\d+_', 'BB_', line)
    line = re.sub(r'\.Lfunc_(end|begin)\d+', r'.Lfunc_\1', line)
    return re.sub(r' +;', ' ;', line)


def split(path):
    """(symbols in emission order, {symbol: normalised text}, lines in front of the first kernel, lines behind the last)"""
    txt = [ln for ln in open(path).read().split('\n') if '__hip_cuid_' not in ln]
    starts = [i - 1 for i, ln in enumerate(txt) if re.match(r'\s*\.protected\s+_Z\S+\s*; -- Begin function', ln)]
    end = next(i for i, ln in enumerate(txt) if i > starts[-1] and ('.AMDGPU.gpr_maximums' in ln or ln.startswith('\t.amdgpu_metadata')))
    order = [txt[i + 1].split()[1] for i in starts]
    bodies = {}
    for n, i in enumerate(starts):
        bodies[order[n]] = '\n'.join(norm(ln) for ln in txt[i:starts[n + 1] if n + 1 < len(starts) else end])
    return order, bodies, txt[:starts[0]], txt[end:]


def main():
    oa, ca, ha, ta = split(sys.argv[1])
    ob, cb, hb, tb = split(sys.argv[2])
    names = subprocess.run(['c++filt'], input='\n'.join(oa).replace('DF16b', 'u6__bf16'), capture_output=True, text=True).stdout.split('\n')
    short = lambda s: re.sub(r'\(.*', '', s).replace('void cdrl::', '').replace('__bf16', 'bf16').replace('(bool)', '').replace(' ', '')     # noqa: E731
    out = open(sys.argv[3], 'w') if len(sys.argv) > 3 else sys.stdout
    same = 0
    for sym, name in sorted(zip(oa, names), key=lambda t: t[1]):
        eq = ca[sym] == cb.get(sym)
        same += eq
        out.write('%s %d %s %s\n' % (short(name), ca[sym].count('\n') + 1, hashlib.sha256(ca[sym].encode()).hexdigest(), 'yes' if eq else 'NO'))
    out.write('# kernels: %d and %d, the same symbols: %s, emitted in the same order: %s, identical bodies: %d\n'
              % (len(oa), len(ob), set(oa) == set(ob), oa == ob, same))
    out.write('# lines in front of the first kernel identical: %s; lines behind the last kernel (register maxima, the metadata with one entry per '
              'kernel in emission order): %d and %d, equal as sorted lists: %s\n' % (ha == hb, len(ta), len(tb), sorted(ta) == sorted(tb)))
    return 0 if same == len(oa) == len(ob) and set(oa) == set(ob) else 1


if __name__ == '__main__':
    sys.exit(main())
