#!/usr/bin/env python3
"""Which kernels of two `make asm` listings differ: every kernel's instruction text (labels, directives and comments left out)
compared by name.  Shows that a change to shared source reached only the instantiations it was meant for.

    python tools/asm_same_kernels.py before.s after.s"""
import re
import sys


def funcs(path):
    d, cur = {}, None
    for l in open(path):
        m = re.match(r"^(_Z\w+):", l)
        if m:
            cur = m.group(1)
            d[cur] = []
        elif l.startswith(".Lfunc_end"):
            cur = None
        elif cur:
            t = l.split(";")[0].strip()                # (trailing comments: loop notes on label lines, which name labels too)
            if t and not t.startswith(".loc"):
                # (local labels carry the function's number in the listing, which shifts when kernels are added: .LBB17_4 -> .LBB_4)
                d[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    return d


a, b = funcs(sys.argv[1]), funcs(sys.argv[2])
diff = [k for k in a if a[k] != b.get(k)]
print("kernels: %d before, %d after; identical text: %d; different: %d" % (len(a), len(b), len(a) - len(diff), len(diff)))
for k in diff:
    print("  %s  %d -> %d lines" % (re.sub(r"EEvP15HIP.*", "E", k), len(a[k]), len(b.get(k, []))))
