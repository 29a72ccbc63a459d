#!/usr/bin/env python3
"""The sequence of depthwise-block dispatches of a rocprofv3 kernel trace (csv): kernel name, grid, workgroup, LDS bytes of every
dwf_*, dws_* and dws2_* dispatch in dispatch order.  With two traces: compares the sequences and prints a summary per kernel.

    rocprofv3 --kernel-trace --output-format csv -d <dir> -o t -- python -m pytest tests/test_gpu_dw_variants.py -m gpu
    tools/dw_dispatch_seq.py <a>/t_kernel_trace.csv [<b>/t_kernel_trace.csv]"""
import collections
import csv
import re
import subprocess
import sys


def sequence(path):
    rows = [r for r in csv.DictReader(open(path)) if re.search(r'cdrl\d+(dwf|dws2?)_', r['Kernel_Name']) or re.search(r'cdrl::(dwf|dws2?)_', r['Kernel_Name'])]
    rows.sort(key=lambda r: int(r['Dispatch_Id']))
    return [(r['Kernel_Name'], tuple(int(r[f'Grid_Size_{a}']) for a in 'XYZ'), tuple(int(r[f'Workgroup_Size_{a}']) for a in 'XYZ'),
             int(r['LDS_Block_Size'])) for r in rows]


def short(names):
    out = subprocess.run(['c++filt'], input='\n'.join(n.replace('DF16b', 'u6__bf16') for n in names), capture_output=True, text=True).stdout.split('\n')
    return [re.sub(r'\(.*', '', s).replace('void cdrl::', '').replace('__bf16', 'bf16').replace('(bool)', '').replace(' ', '') for s in out]


def main():
    a = sequence(sys.argv[1])
    per = collections.OrderedDict()
    for name, grid, wg, lds in a:
        d = per.setdefault(name, [0, set()])
        d[0] += 1
        d[1].add((grid[0] // wg[0], wg[0], wg[1], lds))
    names = sorted(per)
    print(f'# {len(a)} dispatches of {len(per)} kernels')
    print('# kernel  dispatches  distinct (workgroups, block x, block y, LDS bytes)')
    for n, s in zip(names, short(names)):
        print(s, per[n][0], len(per[n][1]))
    if len(sys.argv) > 2:
        b = sequence(sys.argv[2])
        same = a == b
        print(f'# second trace: {len(b)} dispatches; sequence of (kernel, grid, workgroup, LDS bytes) identical: {same}')
        if not same:
            for i, (x, y) in enumerate(zip(a, b)):
                if x != y:
                    print('# first difference at', i, x, y)
                    break
            return 1
    return 0


if __name__ == '__main__':
    sys.exit(main())
