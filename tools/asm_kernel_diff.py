#!/usr/bin/env python3
"""Which kernels of two device assembly listings (hipcc -S --cuda-device-only; the product's
command is _build.compile_cmd(src, out, kind='asm')) have the same code: per kernel symbol,
the text from its label to its .Lfunc_end, and its .amdhsa_ descriptor block, compared line by
line with the __hip_cuid_<hash> symbol (a hash of the translation unit) masked.  Kernels are
matched by demangled name without the argument list, and a kernel's own symbol and the function
number in its block labels (.LBB<n>_) are masked: an argument type renamed, or a kernel defined
ahead of it, changes those and no instruction.  No GPU needed.

usage: tools/asm_kernel_diff.py A.s B.s [name-filter]     (exit status 1 if a listed kernel differs)
"""
import re
import subprocess
import sys


def kernels(path):
    text = re.sub(r'__hip_cuid_[0-9a-f]+', '__hip_cuid_X', open(path).read())
    out = {}
    for m in re.finditer(r'^(\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:\n', text, re.S | re.M):
        out[m.group(1)] = [re.sub(r'BB\d+_', 'BBn_', m.group(2)).replace(m.group(1), 'KERNEL')]
    for m in re.finditer(r'^\s*\.amdhsa_kernel (\w+)\n(.*?)^\s*\.end_amdhsa_kernel', text, re.S | re.M):
        if m.group(1) in out:
            out[m.group(1)].append(m.group(2).replace(m.group(1), 'KERNEL'))
    names = list(out)
    dem = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout.splitlines()
    return {re.sub(r'\(anonymous namespace\)::', '', d).split('(')[0]: out[n] for n, d in zip(names, dem)}


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    flt = sys.argv[3] if len(sys.argv) > 3 else ''
    bad = 0
    for n in sorted(set(a) | set(b)):
        d = n
        if flt not in d:
            continue
        if n not in a or n not in b:
            state = 'only in ' + (sys.argv[1] if n in a else sys.argv[2])
        elif a[n] == b[n]:
            state = 'identical (%d lines)' % a[n][0].count('\n')
        else:
            la, lb = a[n][0].splitlines(), b[n][0].splitlines()
            state = 'DIFFERS (%d vs %d lines, descriptor %s)' % (
                len(la), len(lb), 'same' if a[n][1:] == b[n][1:] else 'differs')
        bad += not state.startswith('identical')
        print('%-90s %s' % (d, state))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
